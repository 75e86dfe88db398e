// beam_kernels.hip — one beam-search scoring step on gfx950 (C ABI: include/smt_beam.h).
//
// transformers' _beam_search scores a token with about a dozen launches over [R, V] fp32 tensors
// (float copy, log_softmax, the repetition penalty's gather / where / scatter, the suppression, the add
// of the running beam scores, topk over [N, nb*V]). Here it is three launches that read the logits in
// their own format twice (4 MB at R 16, V 128256 in bf16: the second read comes from the L2 / Infinity
// Cache) and write K candidates per sample:
//   1. beam_partial_kernel     one workgroup per (row, chunk of CHUNK elements): the chunk's max and
//                              sum of exp(x - max)                                  -> workspace
//   2. beam_chunk_topk_kernel  one workgroup per (row, chunk): the row's lse from its chunk partials
//                              (the same fixed order in every workgroup of the row), the chunk's
//                              scores in registers, its K best as sortable 64-bit keys -> workspace
//   3. beam_merge_kernel       one workgroup per sample: the K best of the nb * nchunks * K keys
// A key is (order-preserving bits of the fp32 score) << 32 | ~flat_index, so "larger key" is "higher
// score, then lower flat index", keys of one sample are distinct, and key 0 means "no candidate".
// Selection is K rounds of a workgroup-wide max over keys: no atomics, a fixed order, bit-reproducible.
// R 16 x 63 chunks = 1008 workgroups of 256 threads, about four per CU of the 256.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "smt_hip.h"
#include "smt_beam.h"

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

constexpr int CHUNK = SMT_BEAM_CHUNK;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int EPT = CHUNK / THREADS;             // elements per thread: one 16-byte load of a 16-bit row
constexpr int MERGE_LDS_KEYS = 6144;             // 48 KiB of keys staged in the LDS by the merge
static_assert(EPT == 8, "load8 reads 8 consecutive elements per thread");

struct Suppressed {
    int64_t id[SMT_BEAM_MAX_SUPPRESSED];
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

// butterfly: every lane adds the same pairs at every level (a + b == b + a), so all 64 lanes hold the
// same bits and the order is fixed
__device__ __forceinline__ float wave_sum(float v) {
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

// Workgroup-wide reductions through `red[WAVES]`; the trailing barrier frees `red` for the next call.
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = fmaxf(r, red[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r += red[w];
    __syncthreads();
    return r;
}

// One barrier per call: round j uses kred[j & 1], and nobody writes kred[(j + 1) & 1] again before
// every thread has passed round j's barrier, that is, has finished reading round j - 1.
__device__ __forceinline__ uint64_t block_max_key(uint64_t k, uint64_t (*kred)[WAVES], int round) {
    k = wave_max_key(k);
    uint64_t* slot = kred[round & 1];
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = k;
    __syncthreads();
    uint64_t r = slot[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = slot[w] > r ? slot[w] : r;
    return r;
}

// fp32 -> uint32 with the order of the floats (-0 was made +0 by the caller); NaNs land at either end.
__device__ __forceinline__ uint32_t order_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float order_float(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <int F>
__global__ __launch_bounds__(THREADS) void beam_partial_kernel(const void* __restrict__ logits, int64_t ld, int64_t V,
                                                               int32_t nchunks, float2* __restrict__ partial) {
    __shared__ float red[WAVES];
    const int64_t row = blockIdx.x / nchunks;
    const int64_t chunk = blockIdx.x - row * nchunks;
    const auto* x_row = static_cast<const typename Elem<F>::type*>(logits) + row * ld;
    float x[EPT];
    load8<F>(x_row, chunk * CHUNK + (int64_t)threadIdx.x * EPT, V, x);
    float m = x[0];
#pragma unroll
    for (int i = 1; i < EPT; ++i) m = fmaxf(m, x[i]);
    m = block_max(m, red);
    float s = 0.f;
    if (m > -INFINITY) {                        // an all -inf chunk contributes nothing (no inf - inf)
#pragma unroll
        for (int i = 0; i < EPT; ++i) s += expf(x[i] - m);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(m, s);
}

template <int F>
__global__ __launch_bounds__(THREADS) void beam_chunk_topk_kernel(
    const void* __restrict__ logits, int64_t ld, int64_t V, int32_t nchunks, int32_t nb,
    const float2* __restrict__ partial, const float* __restrict__ beam_scores, const int64_t* __restrict__ sequences,
    int64_t seq_ld, int32_t cur_len, float penalty, Suppressed sup, int32_t K, uint64_t* __restrict__ cand) {
    __shared__ float red[WAVES];
    __shared__ uint64_t kred[2][WAVES];
    __shared__ uint32_t seen_words[CHUNK / 4];
    uint8_t* seen = reinterpret_cast<uint8_t*>(seen_words);
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / nchunks;
    const int64_t chunk = blockIdx.x - row * nchunks;
    const int64_t lo = chunk * CHUNK;

    // the row's lse: every workgroup of the row combines the same partials in the same order
    const float2* p_row = partial + row * nchunks;
    float m = -INFINITY;
    for (int c = tid; c < nchunks; c += THREADS) m = fmaxf(m, p_row[c].x);
    m = block_max(m, red);
    float s = 0.f;
    for (int c = tid; c < nchunks; c += THREADS) {
        const float2 p = p_row[c];
        if (p.x > -INFINITY) s += p.y * expf(p.x - m);
    }
    s = block_sum(s, red);
    const float lse = m + logf(s);

    // which tokens of this chunk occur in the row's history: plain byte stores of the same value
    for (int i = tid; i < CHUNK / 4; i += THREADS) seen_words[i] = 0u;
    __syncthreads();
    if (penalty != 1.0f) {                       // lp * 1 == lp / 1 == lp: nothing to mark
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
    const float bs = beam_scores[row];
    const int64_t flat0 = (row % nb) * V;
    uint64_t key[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int64_t v = v0 + i;
        float lp = x[i] - lse;
        if (v < V && seen[v - lo]) lp = lp < 0.f ? lp * penalty : lp / penalty;
        for (int j = 0; j < sup.n; ++j)
            if (sup.id[j] == v) lp = -INFINITY;
        float score = lp + bs;
        if (score == 0.f) score = 0.f;          // -0 -> +0: equal scores get equal bits
        key[i] = v < V ? ((uint64_t)order_bits(score) << 32) | (uint32_t)~(uint32_t)(flat0 + v) : 0ull;
    }

    uint64_t* out = cand + (int64_t)blockIdx.x * K;
    for (int j = 0; j < K; ++j) {
        uint64_t best = key[0];
#pragma unroll
        for (int i = 1; i < EPT; ++i) best = key[i] > best ? key[i] : best;
        best = block_max_key(best, kred, j);
        if (tid == 0) out[j] = best;            // 0 once the chunk has fewer than j + 1 elements
#pragma unroll
        for (int i = 0; i < EPT; ++i)
            if (key[i] == best) key[i] = 0ull;
    }
}

template <bool IN_LDS>
__global__ __launch_bounds__(THREADS) void beam_merge_kernel(const uint64_t* __restrict__ cand, int64_t per_sample, int32_t K,
                                                             float* __restrict__ top_scores, int32_t* __restrict__ top_index) {
    __shared__ uint64_t kred[2][WAVES];
    __shared__ uint64_t staged[IN_LDS ? MERGE_LDS_KEYS : 1];
    const int tid = threadIdx.x;
    const uint64_t* src = cand + (int64_t)blockIdx.x * per_sample;
    if constexpr (IN_LDS) {
        for (int64_t i = tid; i < per_sample; i += THREADS) staged[i] = src[i];
        __syncthreads();
    }
    uint64_t prev = ~0ull;                       // above every key: the low word of a key is ~flat, flat >= 0
    for (int j = 0; j < K; ++j) {
        uint64_t best = 0ull;
        for (int64_t i = tid; i < per_sample; i += THREADS) {
            uint64_t k;
            if constexpr (IN_LDS) k = staged[i];
            else k = src[i];
            if (k < prev && k > best) best = k;
        }
        best = block_max_key(best, kred, j);
        if (tid == 0) {
            // K <= nb*V keeps `best` a real key; the guard keeps the index in range regardless
            top_scores[(int64_t)blockIdx.x * K + j] = best ? order_float((uint32_t)(best >> 32)) : -INFINITY;
            top_index[(int64_t)blockIdx.x * K + j] = best ? (int32_t)~(uint32_t)best : 0;
        }
        prev = best;
    }
}

inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

const char* check_sizes(int32_t N, int32_t nb, int64_t V, int32_t K) {
    if (N < 1 || nb < 1 || V < 1) return "N, nb and V must be >= 1";
    if (K < 1 || K > SMT_BEAM_MAX_K) return "K must lie in [1, 32]";
    if ((int64_t)nb > ((int64_t)INT32_MAX) / V) return "nb * V must be < 2^31 (int32 flat index)";
    if ((int64_t)K > (int64_t)nb * V) return "K must be <= nb * V";
    const int64_t nchunks = (V + CHUNK - 1) / CHUNK;
    if ((int64_t)N * nb > (int64_t)0xffffff / nchunks) return "N * nb * chunks must be < 2^24 (grid size)";
    return nullptr;
}

template <int F>
int launch(const void* logits, int64_t ld, int32_t N, int32_t nb, int64_t V, const float* beam_scores,
           const int64_t* sequences, int64_t seq_ld, int32_t cur_len, float penalty, const Suppressed& sup, int32_t K,
           float* top_scores, int32_t* top_index, void* workspace, hipStream_t stream) {
    const int32_t nchunks = (int32_t)((V + CHUNK - 1) / CHUNK);
    const int64_t R = (int64_t)N * nb;
    float2* partial = static_cast<float2*>(workspace);
    uint64_t* cand = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + round16(R * nchunks * (int64_t)sizeof(float2)));
    const dim3 grid((uint32_t)(R * nchunks)), block(THREADS);
    hipLaunchKernelGGL((beam_partial_kernel<F>), grid, block, 0, stream, logits, ld, V, nchunks, partial);
    hipLaunchKernelGGL((beam_chunk_topk_kernel<F>), grid, block, 0, stream, logits, ld, V, nchunks, nb, partial, beam_scores,
                       sequences, seq_ld, cur_len, penalty, sup, K, cand);
    const int64_t per_sample = (int64_t)nb * nchunks * K;
    if (per_sample <= MERGE_LDS_KEYS)
        hipLaunchKernelGGL((beam_merge_kernel<true>), dim3(N), block, 0, stream, cand, per_sample, K, top_scores, top_index);
    else
        hipLaunchKernelGGL((beam_merge_kernel<false>), dim3(N), block, 0, stream, cand, per_sample, K, top_scores, top_index);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "smt_beam_topk: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char* smt_beam_last_error(void) { return g_err; }

int64_t smt_beam_topk_workspace(int32_t N, int32_t nb, int64_t V, int32_t K) {
    if (const char* why = check_sizes(N, nb, V, K)) return fail(-1, "smt_beam_topk_workspace: %s", why);
    const int64_t slots = (int64_t)N * nb * ((V + CHUNK - 1) / CHUNK);
    return round16(slots * (int64_t)sizeof(float2)) + slots * K * (int64_t)sizeof(uint64_t);
}

int smt_beam_topk(const void* logits, int64_t ld, int32_t dtype, int32_t N, int32_t nb, int64_t V,
                  const float* beam_scores, const int64_t* sequences, int64_t seq_ld, int32_t cur_len, float penalty,
                  const int64_t* suppressed, int32_t n_suppressed, int32_t K, float* top_scores, int32_t* top_index,
                  void* workspace, hipStream_t stream) {
    if (const char* why = check_sizes(N, nb, V, K)) return fail(-1, "smt_beam_topk: %s", why);
    if (dtype != SMT_DTYPE_BF16 && dtype != SMT_DTYPE_FP16 && dtype != SMT_DTYPE_FP32)
        return fail(-1, "smt_beam_topk: dtype %d is not SMT_DTYPE_BF16 / _FP16 / _FP32", (int)dtype);
    if (ld < V) return fail(-1, "smt_beam_topk: ld %lld < V %lld", (long long)ld, (long long)V);
    if (cur_len < 0) return fail(-1, "smt_beam_topk: negative cur_len %d", (int)cur_len);
    if (seq_ld < cur_len) return fail(-1, "smt_beam_topk: seq_ld %lld < cur_len %d", (long long)seq_ld, (int)cur_len);
    if (!(penalty > 0.f)) return fail(-1, "smt_beam_topk: penalty must be > 0 (got %g)", (double)penalty);
    if (n_suppressed < 0 || n_suppressed > SMT_BEAM_MAX_SUPPRESSED)
        return fail(-1, "smt_beam_topk: n_suppressed %d outside [0, 8]", (int)n_suppressed);
    if (n_suppressed > 0 && !suppressed) return fail(-1, "smt_beam_topk: null suppressed list");
    if (!logits || !beam_scores || !top_scores || !top_index) return fail(-1, "smt_beam_topk: null buffer");
    if (!sequences && cur_len > 0) return fail(-1, "smt_beam_topk: null sequences with cur_len %d", (int)cur_len);
    if (!workspace) return fail(-1, "smt_beam_topk: null workspace");
    const int64_t esize = dtype == SMT_DTYPE_FP32 ? 4 : 2;
    if (!aligned(logits, 16) || (ld * esize) % 16 != 0)
        return fail(-2, "smt_beam_topk: logits rows must be 16-byte aligned (ld %lld)", (long long)ld);
    if (!aligned(workspace, 16) || !aligned(beam_scores, 4) || !aligned(top_scores, 4) || !aligned(top_index, 4) ||
        !aligned(sequences, 8))
        return fail(-2, "smt_beam_topk: misaligned buffer");
    Suppressed sup = {};
    sup.n = n_suppressed;
    for (int i = 0; i < n_suppressed; ++i) sup.id[i] = suppressed[i];
#define BEAM_LAUNCH(F)                                                                                                  \
    launch<F>(logits, ld, N, nb, V, beam_scores, sequences, seq_ld, cur_len, penalty, sup, K, top_scores, top_index, \
              workspace, stream)
    if (dtype == SMT_DTYPE_BF16) return BEAM_LAUNCH(SMT_DTYPE_BF16);
    if (dtype == SMT_DTYPE_FP16) return BEAM_LAUNCH(SMT_DTYPE_FP16);
    return BEAM_LAUNCH(SMT_DTYPE_FP32);
#undef BEAM_LAUNCH
}

}  // extern "C"
