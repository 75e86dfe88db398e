// sample_kernels.hip — token selection for num_beams == 1 on gfx950 (C ABI: include/smt_sample.h).
//
// transformers' _sample picks a token with a float copy, the repetition penalty's gather / where /
// scatter, a division, a topk, a whole-vocabulary sort, softmax / cumsum / scatter / masked_fill, a
// second softmax and torch.multinomial, all over [R, V] fp32 tensors. Here it is two launches:
//   1. sample_z_kernel       one workgroup per (row, chunk of CHUNK elements): z = penalised, suppressed
//                            logits / temperature as fp32, and the chunk's maximum      -> workspace
//   2. sample_select_kernel  one workgroup per row: the top-k and top-p thresholds by radix selection,
//                            then one pass that applies min-p, counts the kept set, finds its smallest
//                            value and takes the (Gumbel) argmax
// All three filters are thresholds on z, so selection means "find a key": a key is the order-preserving
// 32 bits of z. A selection first cuts the row into 256 bins of width 1/8 below the row's maximum M
// (bin = floor(fl(M - z) * 8), monotone in z; logits spread over tens of bins there, where the top bits
// of a float key would put nearly the whole row into two or three), picks the bin that holds the
// threshold from the bins' counts (top-k) or masses (top-p), gathers that bin's keys into a list and
// runs four 8-bit radix passes over the list. Masses are integers, round(expf(z - M) * 2^40), added
// with integer LDS atomics: no float is ever added by an atomic, integer sums do not depend on the
// order, and neither does the result on the order of the gathered list. A thread adds a run of equal
// bins in registers and issues the atomics when the bin changes, so a row of equal values costs no
// atomics at all. The time does not depend on top_k.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "smt_hip.h"
#include "smt_sample.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int CHUNK = SMT_SAMPLE_CHUNK;
constexpr int THREADS = 256;                     // first launch
constexpr int WAVES = THREADS / 64;
constexpr int EPT = CHUNK / THREADS;             // elements per thread: one 16-byte load of a 16-bit row
constexpr int SEL_THREADS = 1024;                // second launch
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int BINS = 256;
static_assert(EPT == 8, "load8 reads 8 consecutive elements per thread");

struct Suppressed {
    int64_t id[SMT_SAMPLE_MAX_SUPPRESSED];
    int32_t n;
};

template <int F> struct Elem { using type = uint16_t; };
template <> struct Elem<SMT_DTYPE_FP32> { using type = float; };

template <int F> __device__ __forceinline__ float to_f32(typename Elem<F>::type b) {
    if constexpr (F == SMT_DTYPE_FP32) return b;
    else if constexpr (F == SMT_DTYPE_FP16) return (float)__builtin_bit_cast(_Float16, b);
    else return __uint_as_float((uint32_t)b << 16);
}

// Elements [v0, v0 + 8) of a row as fp32 (exact); v0 % 8 == 0 and the row is 16-byte aligned. Elements
// at v >= V are not read and come back as -inf.
template <int F>
__device__ __forceinline__ void load8(const typename Elem<F>::type* row, int64_t v0, int64_t V, float (&x)[EPT]) {
    using T = typename Elem<F>::type;
    if (v0 + EPT <= V) {
        if constexpr (F == SMT_DTYPE_FP32) {
            const float4 a = *reinterpret_cast<const float4*>(row + v0);
            const float4 b = *reinterpret_cast<const float4*>(row + v0 + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
            x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
            const uint4 a = *reinterpret_cast<const uint4*>(row + v0);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[2 * i] = to_f32<F>((T)(w[i] & 0xffffu));
                x[2 * i + 1] = to_f32<F>((T)(w[i] >> 16));
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < EPT; ++i) x[i] = (v0 + i < V) ? to_f32<F>(row[v0 + i]) : -INFINITY;
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint64_t wave_max_key(uint64_t k) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)k, o), hi = __shfl_xor((uint32_t)(k >> 32), o);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        k = other > k ? other : k;
    }
    return k;
}

// fp32 -> uint32 with the order of the floats (-0 was made +0 by the caller); NaNs land at either end.
__device__ __forceinline__ uint32_t order_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float order_float(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x21F0AAADu; x ^= x >> 15; x *= 0x735A2D97u; x ^= x >> 15;
    return x;
}

// g_v of the header: the Gumbel variate of token v under `row_key`
__device__ __forceinline__ float gumbel(uint32_t row_key, uint32_t v) {
    const uint32_t word = mix(row_key ^ (v * 0x9E3779B1u));
    float u = ((float)(word >> 8) + 0.5f) * 0x1p-24f;
    u = fminf(u, 0x1.fffffep-1f);
    return -logf(-logf(u));
}

template <int F>
__global__ __launch_bounds__(THREADS) void sample_z_kernel(
    const void* __restrict__ logits, int64_t ld, int64_t V, int32_t nchunks, const int64_t* __restrict__ sequences,
    int64_t seq_ld, int32_t cur_len, float penalty, Suppressed sup, float temperature, float* __restrict__ z_out,
    float* __restrict__ cmax) {
    __shared__ float red[WAVES];
    __shared__ uint32_t seen_words[CHUNK / 4];
    uint8_t* seen = reinterpret_cast<uint8_t*>(seen_words);
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / nchunks;
    const int64_t chunk = blockIdx.x - row * nchunks;
    const int64_t lo = chunk * CHUNK;

    // which tokens of this chunk occur in the row's history: plain byte stores of the same value
    for (int i = tid; i < CHUNK / 4; i += THREADS) seen_words[i] = 0u;
    __syncthreads();
    if (penalty != 1.0f) {                       // x * 1 == x / 1 == x: nothing to mark
        const int64_t* hist = sequences + row * seq_ld;
        for (int i = tid; i < cur_len; i += THREADS) {
            const int64_t id = hist[i];
            const int64_t off = id - lo;
            if (off >= 0 && off < CHUNK && id < V) seen[off] = 1;       // ids outside [0, V) form no address
        }
    }
    __syncthreads();

    const auto* x_row = static_cast<const typename Elem<F>::type*>(logits) + row * ld;
    const int64_t v0 = lo + (int64_t)tid * EPT;
    float x[EPT];
    load8<F>(x_row, v0, V, x);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int64_t v = v0 + i;
        float y = x[i];
        if (v < V && seen[v - lo]) y = y < 0.f ? y * penalty : y / penalty;
        for (int j = 0; j < sup.n; ++j)
            if (sup.id[j] == v) y = -INFINITY;
        float z = y / temperature;
        if (z == 0.f) z = 0.f;                  // -0 -> +0: equal values get equal bits
        x[i] = v < V ? z : -INFINITY;
        m = fmaxf(m, x[i]);
    }
    // the workspace row is nchunks * CHUNK wide: the padding of the last chunk is written as -inf
    float* z_row = z_out + row * (int64_t)nchunks * CHUNK;
    *reinterpret_cast<float4*>(z_row + v0) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(z_row + v0 + 4) = make_float4(x[4], x[5], x[6], x[7]);

    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float r = red[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) r = fmaxf(r, red[w]);
        cmax[blockIdx.x] = r;
    }
}

// ---- second launch ---------------------------------------------------------------------------------

struct Selected {
    uint32_t digit, cnt_above, cnt_at;
    uint64_t mass_above, mass_at;
};

struct SelectShared {
    uint32_t cnt[2][BINS];                       // [0]: the bins below M of the whole row, [1]: a radix pass
    uint64_t mass[2][BINS];
    Selected sel;
    uint64_t total_mass;
    uint32_t list_n;
    float fred[SEL_WAVES];
    uint32_t ured[2][SEL_WAVES];
    uint64_t kred[SEL_WAVES];
};

// round(expf(fl(z - M)) * 2^40); 0 for anything that is not <= M (NaN, or M not the maximum of a NaN row)
__device__ __forceinline__ uint64_t mass_q(float z, float M) {
    const float d = z - M;
    return d <= 0.f ? (uint64_t)__double2ll_rn((double)expf(d) * 1099511627776.0) : 0ull;
}

// 255 - bin, bin = floor(fl(M - z) * 8) capped at 255: a higher digit is a larger z
__device__ __forceinline__ int lin_digit(float z, float M) {
    const float d = M - z;
    const int bin = (d >= 0.f && d < 31.875f) ? (int)(d * 8.f) : 255;
    return 255 - bin;
}

// A run of equal digits is added in registers; the atomics go out when the digit changes.
struct Run {
    int digit = -1;
    uint32_t c = 0;
    uint64_t m = 0;
    __device__ __forceinline__ void flush(uint32_t* cnt, uint64_t* mass) {
        if (c) {
            atomicAdd(&cnt[digit], c);
            if (m) atomicAdd(reinterpret_cast<unsigned long long*>(&mass[digit]), (unsigned long long)m);
        }
        c = 0;
        m = 0;
    }
    __device__ __forceinline__ void add(int d, uint64_t q, uint32_t* cnt, uint64_t* mass) {
        if (d != digit) {
            flush(cnt, mass);
            digit = d;
        }
        c += 1;
        m += q;
    }
};

__device__ __forceinline__ void zero_hist(SelectShared& s, int which) {
    for (int i = threadIdx.x; i < BINS; i += SEL_THREADS) {
        s.cnt[which][i] = 0u;
        s.mass[which][i] = 0ull;
    }
    __syncthreads();
}

// The digit d with sum_{b >= d} h[b] >= target > sum_{b > d} h[b], h the counts or the masses, together
// with both sums above it. Called after a barrier behind the histogram's last atomic. Integer sums: the
// 256 threads that each add their own suffix agree whatever the order. No such digit (target above the
// total, possible only for NaN rows): digit 0 with nothing above.
__device__ __forceinline__ Selected select_digit(SelectShared& s, int which, bool by_mass, uint64_t target) {
    const int tid = threadIdx.x;
    if (tid == 0) s.sel = Selected{0u, 0u, s.cnt[which][0], 0ull, s.mass[which][0]};
    __syncthreads();
    if (tid < BINS) {
        uint32_t ca = 0;
        uint64_t ma = 0;
        for (int b = tid + 1; b < BINS; ++b) {
            ca += s.cnt[which][b];
            ma += s.mass[which][b];
        }
        const uint32_t c = s.cnt[which][tid];
        const uint64_t m = s.mass[which][tid];
        const uint64_t excl = by_mass ? ma : (uint64_t)ca;
        const uint64_t incl = by_mass ? ma + m : (uint64_t)ca + c;
        if (incl >= target && excl < target) s.sel = Selected{(uint32_t)tid, ca, c, ma, m};
        if (tid == 0) s.total_mass = ma + m;
    }
    __syncthreads();
    const Selected r = s.sel;
    __syncthreads();
    return r;
}

// f(v, z) for every v < V of the row, four consecutive elements per thread and step
template <typename Fn>
__device__ __forceinline__ void for_row(const float* __restrict__ z_row, int64_t V, Fn f) {
    for (int64_t v0 = (int64_t)threadIdx.x * 4; v0 < V; v0 += (int64_t)SEL_THREADS * 4) {
        const float4 a = *reinterpret_cast<const float4*>(z_row + v0);       // the row is padded to whole chunks
        const float e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (v0 + i < V) f(v0 + i, e[i]);
    }
}

// The largest key t with  count{key >= t} >= target  (by_mass: mass{key >= t} >= target) among the keys of
// the row whose linear digit is `lin` -- the bin select_digit picked from the row's histogram, with
// `target` already less what lies above that bin. Returns t; *mass_ge is the mass of the bin's keys >= t.
__device__ __forceinline__ uint32_t refine(SelectShared& s, const float* __restrict__ z_row, int64_t V, float M, int lin,
                                           uint32_t* __restrict__ list, bool by_mass, bool need_mass, uint64_t target,
                                           uint64_t* mass_ge) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s.list_n = 0u;
    __syncthreads();
    for_row(z_row, V, [&](int64_t v, float z) {
        const bool mine = lin_digit(z, M) == lin;
        const uint64_t votes = __ballot(mine);
        if (mine) {                              // the active lanes here are exactly `votes`
            const int leader = __ffsll((unsigned long long)votes) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&s.list_n, (uint32_t)__popcll(votes));
            base = __shfl(base, leader);
            list[base + __popcll(votes & ((1ull << lane) - 1ull))] = order_bits(z);     // at most V entries
        }
    });
    __syncthreads();
    const uint32_t n = s.list_n;
    uint32_t prefix = 0u, mask = 0u;
    uint64_t above = 0ull, at = 0ull;
    for (int shift = 24; shift >= 0; shift -= 8) {
        zero_hist(s, 1);
        Run run;
        for (uint32_t i = tid; i < n; i += SEL_THREADS) {
            const uint32_t key = list[i];
            if ((key & mask) == prefix)
                run.add((int)((key >> shift) & 255u), need_mass ? mass_q(order_float(key), M) : 0ull, s.cnt[1], s.mass[1]);
        }
        run.flush(s.cnt[1], s.mass[1]);
        __syncthreads();
        const Selected r = select_digit(s, 1, by_mass, target);
        target -= by_mass ? r.mass_above : (uint64_t)r.cnt_above;
        above += r.mass_above;
        at = r.mass_at;
        prefix |= r.digit << shift;
        mask |= 255u << shift;
    }
    *mass_ge = above + at;
    return prefix;
}

__global__ __launch_bounds__(SEL_THREADS) void sample_select_kernel(
    const float* __restrict__ z_all, const float* __restrict__ cmax, uint32_t* __restrict__ list_all, int64_t V,
    int32_t nchunks, int32_t top_k, float top_p_thr, int32_t use_top_p, float log_min_p, int32_t use_min_p, int32_t mode,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t row0, int32_t* __restrict__ token,
    float* __restrict__ threshold, int32_t* __restrict__ kept) {
    __shared__ SelectShared s;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t vp = (int64_t)nchunks * CHUNK;
    const float* z_row = z_all + row * vp;
    uint32_t* list = list_all + row * vp;

    // M: the row's maximum (fmaxf in any order gives the same value)
    float M = -INFINITY;
    for (int c = tid; c < nchunks; c += SEL_THREADS) M = fmaxf(M, cmax[row * nchunks + c]);
    M = wave_max(M);
    if ((tid & 63) == 0) s.fred[tid >> 6] = M;
    __syncthreads();
    M = s.fred[0];
#pragma unroll
    for (int w = 1; w < SEL_WAVES; ++w) M = fmaxf(M, s.fred[w]);

    const bool use_top_k = top_k > 0 && (int64_t)top_k < V;
    uint32_t t_key = 0u;                         // below the key of every number: no threshold
    if (use_top_k || use_top_p) {
        zero_hist(s, 0);
        Run run;
        for_row(z_row, V, [&](int64_t, float z) {
            run.add(lin_digit(z, M), use_top_p ? mass_q(z, M) : 0ull, s.cnt[0], s.mass[0]);
        });
        run.flush(s.cnt[0], s.mass[0]);
        __syncthreads();
        uint64_t W = 0ull;                       // the mass of the top-k survivors
        if (use_top_k) {
            const Selected r = select_digit(s, 0, false, (uint64_t)top_k);
            uint64_t in_bin = 0ull;
            t_key = refine(s, z_row, V, M, (int)r.digit, list, false, use_top_p != 0, (uint64_t)top_k - r.cnt_above, &in_bin);
            W = r.mass_above + in_bin;
        }
        if (use_top_p) {
            if (!use_top_k) {
                select_digit(s, 0, true, ~0ull);
                W = s.total_mass;                // written before select_digit's last two barriers
            }
            // v stays iff mass{z_j > z_v} < (1 - thr) * W: t_p is the largest t with mass{z_j >= t} >= P
            const double pd = ceil((double)W * (1.0 - (double)top_p_thr));
            uint64_t P = pd >= 1.0 ? (uint64_t)pd : 1ull;
            const Selected r = select_digit(s, 0, true, P);
            uint64_t in_bin = 0ull;
            const uint32_t t_p = refine(s, z_row, V, M, (int)r.digit, list, true, true, P - r.mass_above, &in_bin);
            t_key = t_p > t_key ? t_p : t_key;
        }
    }

    // the kept set, its smallest value, and the argmax of z (+ g) over it
    const uint32_t row_key = mix((mix(seed_lo + (row0 + (uint32_t)row) * 0x9E3779B9u) ^ seed_hi) + step * 0x85EBCA6Bu);
    uint32_t n_kept = 0u, min_key = 0xffffffffu;
    uint64_t best = 0ull;
    for_row(z_row, V, [&](int64_t v, float z) {
        const uint32_t key = order_bits(z);
        bool keep = key >= t_key;
        if (use_min_p && (z - M) < log_min_p) keep = false;
        if (keep) {
            n_kept += 1u;
            min_key = key < min_key ? key : min_key;
            float score = z;
            if (mode == SMT_SAMPLE_DRAW) {
                score = z + gumbel(row_key, (uint32_t)v);
                if (score == 0.f) score = 0.f;
            }
            const uint64_t k = ((uint64_t)order_bits(score) << 32) | (uint32_t)~(uint32_t)v;
            best = k > best ? k : best;
        }
    });
    n_kept = wave_sum_u32(n_kept);
    min_key = wave_min_u32(min_key);
    best = wave_max_key(best);
    if ((tid & 63) == 0) {
        s.ured[0][tid >> 6] = n_kept;
        s.ured[1][tid >> 6] = min_key;
        s.kred[tid >> 6] = best;
    }
    __syncthreads();
    if (tid == 0) {
        n_kept = 0u;
        min_key = 0xffffffffu;
        best = 0ull;
        for (int w = 0; w < SEL_WAVES; ++w) {
            n_kept += s.ured[0][w];
            min_key = s.ured[1][w] < min_key ? s.ured[1][w] : min_key;
            best = s.kred[w] > best ? s.kred[w] : best;
        }
        // nothing kept is possible only for NaN rows: token 0 keeps the output in range
        const uint32_t v = best ? ~(uint32_t)best : 0u;
        token[row] = (int64_t)v < V ? (int32_t)v : 0;
        threshold[row] = order_float(min_key);
        kept[row] = (int32_t)n_kept;
    }
}

inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

const char* check_sizes(int32_t R, int64_t V) {
    if (R < 1 || V < 1) return "R and V must be >= 1";
    if (V > (int64_t)INT32_MAX) return "V must be < 2^31 (int32 token)";
    const int64_t nchunks = (V + CHUNK - 1) / CHUNK;
    if ((int64_t)R > (int64_t)0xffffff / nchunks) return "R * chunks must be < 2^24 (grid size)";
    return nullptr;
}

template <int F>
int launch(const void* logits, int64_t ld, int32_t R, int64_t V, const int64_t* sequences, int64_t seq_ld, int32_t cur_len,
           float penalty, const Suppressed& sup, float temperature, int32_t top_k, float thr, int32_t use_top_p,
           float log_min_p, int32_t use_min_p, int32_t mode, uint64_t seed, uint32_t step, uint32_t row0, int32_t* token,
           float* threshold, int32_t* kept, void* workspace, hipStream_t stream) {
    const int32_t nchunks = (int32_t)((V + CHUNK - 1) / CHUNK);
    const int64_t slots = (int64_t)R * nchunks * CHUNK;
    float* z = static_cast<float*>(workspace);
    uint32_t* list = reinterpret_cast<uint32_t*>(z + slots);
    float* cmax = reinterpret_cast<float*>(list + slots);
    hipLaunchKernelGGL((sample_z_kernel<F>), dim3((uint32_t)((int64_t)R * nchunks)), dim3(THREADS), 0, stream, logits, ld, V,
                       nchunks, sequences, seq_ld, cur_len, penalty, sup, temperature, z, cmax);
    hipLaunchKernelGGL(sample_select_kernel, dim3((uint32_t)R), dim3(SEL_THREADS), 0, stream, z, cmax, list, V, nchunks, top_k,
                       thr, use_top_p, log_min_p, use_min_p, mode, (uint32_t)seed, (uint32_t)(seed >> 32), step, row0, token,
                       threshold, kept);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "smt_sample_token: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char* smt_sample_last_error(void) { return g_err; }

int64_t smt_sample_workspace(int32_t R, int64_t V) {
    if (const char* why = check_sizes(R, V)) return fail(-1, "smt_sample_workspace: %s", why);
    const int64_t nchunks = (V + CHUNK - 1) / CHUNK;
    return round16((int64_t)R * nchunks * CHUNK * 8 + (int64_t)R * nchunks * 4);
}

int smt_sample_token(const void* logits, int64_t ld, int32_t dtype, int32_t R, int64_t V, const int64_t* sequences,
                     int64_t seq_ld, int32_t cur_len, float penalty, const int64_t* suppressed, int32_t n_suppressed,
                     float temperature, int32_t top_k, float top_p, float min_p, int32_t mode, uint64_t seed, uint32_t step,
                     uint32_t row0, int32_t* token, float* threshold, int32_t* kept, void* workspace, hipStream_t stream) {
    if (const char* why = check_sizes(R, V)) return fail(-1, "smt_sample_token: %s", why);
    if (dtype != SMT_DTYPE_BF16 && dtype != SMT_DTYPE_FP16 && dtype != SMT_DTYPE_FP32)
        return fail(-1, "smt_sample_token: dtype %d is not SMT_DTYPE_BF16 / _FP16 / _FP32", (int)dtype);
    if (ld < V) return fail(-1, "smt_sample_token: ld %lld < V %lld", (long long)ld, (long long)V);
    if (cur_len < 0) return fail(-1, "smt_sample_token: negative cur_len %d", (int)cur_len);
    if (seq_ld < cur_len) return fail(-1, "smt_sample_token: seq_ld %lld < cur_len %d", (long long)seq_ld, (int)cur_len);
    if (!(penalty > 0.f)) return fail(-1, "smt_sample_token: penalty must be > 0 (got %g)", (double)penalty);
    if (n_suppressed < 0 || n_suppressed > SMT_SAMPLE_MAX_SUPPRESSED)
        return fail(-1, "smt_sample_token: n_suppressed %d outside [0, 8]", (int)n_suppressed);
    if (n_suppressed > 0 && !suppressed) return fail(-1, "smt_sample_token: null suppressed list");
    if (!(temperature > 0.f) || !(temperature < INFINITY))
        return fail(-1, "smt_sample_token: temperature must be > 0 and finite (got %g)", (double)temperature);
    if (!(top_p > 0.f)) return fail(-1, "smt_sample_token: top_p must be > 0 (got %g)", (double)top_p);
    if (!(min_p <= 1.f)) return fail(-1, "smt_sample_token: min_p must be <= 1 (got %g)", (double)min_p);
    if (mode != SMT_SAMPLE_GREEDY && mode != SMT_SAMPLE_DRAW)
        return fail(-1, "smt_sample_token: mode %d is not SMT_SAMPLE_GREEDY / _DRAW", (int)mode);
    if (!logits || !token || !threshold || !kept) return fail(-1, "smt_sample_token: null buffer");
    if (!sequences && cur_len > 0) return fail(-1, "smt_sample_token: null sequences with cur_len %d", (int)cur_len);
    if (!workspace) return fail(-1, "smt_sample_token: null workspace");
    const int64_t esize = dtype == SMT_DTYPE_FP32 ? 4 : 2;
    if (!aligned(logits, 16) || (ld * esize) % 16 != 0)
        return fail(-2, "smt_sample_token: logits rows must be 16-byte aligned (ld %lld)", (long long)ld);
    if (!aligned(workspace, 16) || !aligned(token, 4) || !aligned(threshold, 4) || !aligned(kept, 4) || !aligned(sequences, 8))
        return fail(-2, "smt_sample_token: misaligned buffer");
    Suppressed sup = {};
    sup.n = n_suppressed;
    for (int i = 0; i < n_suppressed; ++i) sup.id[i] = suppressed[i];
    const int32_t use_top_p = top_p < 1.f, use_min_p = min_p > 0.f;
    const float thr = (float)(1.0 - (double)top_p);
    const float log_min_p = use_min_p ? (float)log((double)min_p) : 0.f;
#define SAMPLE_LAUNCH(F)                                                                                                  \
    launch<F>(logits, ld, R, V, sequences, seq_ld, cur_len, penalty, sup, temperature, top_k, thr, use_top_p, log_min_p, \
              use_min_p, mode, seed, step, row0, token, threshold, kept, workspace, stream)
    if (dtype == SMT_DTYPE_BF16) return SAMPLE_LAUNCH(SMT_DTYPE_BF16);
    if (dtype == SMT_DTYPE_FP16) return SAMPLE_LAUNCH(SMT_DTYPE_FP16);
    return SAMPLE_LAUNCH(SMT_DTYPE_FP32);
#undef SAMPLE_LAUNCH
}

}  // extern "C"
