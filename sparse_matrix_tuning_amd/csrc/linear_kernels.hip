// linear_kernels.hip — the decode linears on gfx950 (C ABI: include/smt_linear.h).
//
// y[M, N] = x[M, K] * W[N, K]^T for M <= 16: one read of W and almost no arithmetic, so the kernel is a
// weight stream. One workgroup of WAVES waves owns 16 output features (one MFMA tile) of one output:
//   - wave w takes the contiguous K-slice [w * c, (w + 1) * c) of the K / 32 steps, c = ceil(steps / WAVES);
//   - a step is one v_mfma_f32_16x16x32 with W as the A operand (lane l: W[n0 + (l & 15)][k0 + 8 (l >> 4) + j],
//     one non-temporal 16-byte load, no LDS staging) and x as the B operand (lane l: x[l & 15][same k], a
//     default-policy 16-byte load that the L2 serves; lanes of rows >= M read row 0 and their column is dropped);
//   - two batches of U steps' loads are in flight: the next batch is issued before the current one's MFMAs;
//     a slice's last, partial batch is loaded whole too (clamped to the slice) and its spare MFMAs are skipped;
//   - the waves' fp32 partials go through the LDS and wave 0 adds them in wave order, rounds once and
//     stores: lane l holds features n0 + 4 (l >> 4) + 0..3 of x row l & 15, 8 contiguous bytes of y.
// The x row is a column of the MFMA and columns never mix, so a row's result is a function of that row
// and of W alone. Nothing here can wait for another workgroup.
// SWIGLU: the workgroup streams the same 16 features of the gate and the up weight into two accumulators
// and applies the SwiGLU forward of llama_kernels.hip to the two rounded products.
// Bias (smt_linear_skinny_bias, PLAIN): an instantiation of its own on BiasParams; wave 0 reads the 16 bias
// features of its tile and adds them in fp32 to the summed accumulator before the one rounding. The plain
// instantiations are compiled from the same text and keep their instructions (profiles/r22_isa_compare.txt).
//
// skinny_fp8_kernel is the same stream on e4m3 bytes (smt_linear_skinny_fp8): a step is 64 K-elements, again
// one 16-byte load per lane of W and of x (lane l: bytes k0 + 16 (l >> 4) + 0..15 of row l & 15), feeding two
// v_mfma_f32_16x16x32_fp8_fp8 (the low and the high 8 bytes of both loads); wave 0 multiplies the summed
// accumulator by RN32(sx[m] * sw[n]) before the one rounding.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "smt_hip.h"
#include "smt_linear.h"
#include "silu_math.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int WAVES = SMT_LINEAR_KSPLIT;
constexpr int THREADS = WAVES * 64;

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// the 16-bit formats as llama_kernels.hip handles them (the SWIGLU epilogue must give its bits)
template <int F> __device__ __forceinline__ float u2f(uint32_t b16) {
    if constexpr (F == SMT_DTYPE_FP16) return (float)__builtin_bit_cast(_Float16, (uint16_t)b16);
    else return __uint_as_float(b16 << 16);
}
template <int F> __device__ __forceinline__ uint32_t f2u(float f) {
    if constexpr (F == SMT_DTYPE_FP16) {
        asm("" : "+v"(f));
        return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    } else return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f);
}
template <int F> __device__ __forceinline__ float rnd(float f) {
    uint32_t b = f2u<F>(f);
    if constexpr (F == SMT_DTYPE_FP16) asm("" : "+v"(b));
    return u2f<F>(b);
}

template <int F> __device__ __forceinline__ f32x4 mfma(const u32x4 a, const u32x4 b, const f32x4 c) {
    if constexpr (F == SMT_DTYPE_FP16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

struct Params {
    const uint16_t* x;
    int64_t ldx;
    const uint16_t* w[SMT_LINEAR_MAX_OUT];
    int64_t ldw[SMT_LINEAR_MAX_OUT];
    uint16_t* y[SMT_LINEAR_MAX_OUT];
    int64_t ldy[SMT_LINEAR_MAX_OUT];
    int32_t tile_end[SMT_LINEAR_MAX_OUT];      // PLAIN: running count of 16-feature tiles over the outputs
    int32_t M, K;
    static constexpr bool kBias = false;
};

// smt_linear_skinny_bias: the same, and one [N] bias of the dtype per output (NULL: none)
struct BiasParams : Params {
    const uint16_t* b[SMT_LINEAR_MAX_OUT];
    static constexpr bool kBias = true;
};

// Steps [s, s + U) of a slice that ends at s_end, a step past the end replaced by the slice's last one (its
// loads stay inside the slice and its MFMA is skipped; wave-uniform, so the clamp is scalar arithmetic): U
// non-temporal 16-byte loads of each weight stream, U default-policy loads of x.
template <int NW, int U>
__device__ __forceinline__ void load_batch(u32x4 (&a)[NW][U], u32x4 (&b)[U], const uint16_t* const (&wp)[NW],
                                           const uint16_t* xp, int s, int s_end) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t off = (int64_t)min(s + u, s_end - 1) * 32;
#pragma unroll
        for (int i = 0; i < NW; ++i) a[i][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[i] + off));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) b[u] = *reinterpret_cast<const u32x4*>(xp + (int64_t)min(s + u, s_end - 1) * 32);
}

// NW weight streams (1: PLAIN, 2: SWIGLU's gate and up) against one x stream, U steps per batch. P: Params, or
// BiasParams (NW == 1 only): wave 0 adds the output's bias to the summed accumulator, one fp32 add before the
// one rounding; an output whose bias is NULL gets no add at all, so its bits are the plain form's.
template <int F, int NW, int U, typename P = Params>
__global__ __launch_bounds__(THREADS)
void skinny_kernel(const P p) {
    __shared__ f32x4 part[NW][WAVES][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, h = lane >> 4;

    int out = 0, tile = blockIdx.x;
    if constexpr (NW == 1) {
        out = (tile >= p.tile_end[0]) + (tile >= p.tile_end[1]);      // tile_end[i] is the total for i >= n_out
        if (out) tile -= p.tile_end[out - 1];
    }
    const int n0 = tile * 16;
    // the bias of this lane's four features, 8 bytes with the default cache policy: wave 0 alone asks for the
    // workgroup's 16 features (32 bytes), first of all its loads, so the stream below hides the latency
    const uint16_t* bp = nullptr;
    uint2 bias = make_uint2(0u, 0u);
    if constexpr (P::kBias) {
        static_assert(NW == 1, "the bias epilogue is PLAIN's");
        bp = p.b[out];
        if (wave == 0 && bp) bias = *reinterpret_cast<const uint2*>(bp + n0 + 4 * h);
    }
    const uint16_t* wp[NW];
    if constexpr (NW == 1) wp[0] = p.w[out] + (int64_t)(n0 + r) * p.ldw[out] + 8 * h;
    else {
        wp[0] = p.w[0] + (int64_t)(n0 + r) * p.ldw[0] + 8 * h;
        wp[1] = p.w[1] + (int64_t)(n0 + r) * p.ldw[1] + 8 * h;
    }
    // lanes of rows >= M read row 0 instead (rows >= M are never touched); their column of the MFMA is
    // computed and dropped, and no column reaches another
    const bool row_live = r < p.M;
    const uint16_t* xp = p.x + (int64_t)(row_live ? r : 0) * p.ldx + 8 * h;

    const int steps = p.K >> 5;
    const int per = (steps + WAVES - 1) / WAVES;
    int s = wave * per;
    const int s_end = min(steps, s + per);

    f32x4 acc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // batches of U steps, two in flight: the next batch's loads are issued before the current one's MFMAs
    // wait for theirs. Only the last batch can be partial; no condition stands around a load (a branch there
    // costs a vmcnt(0) each), the steps past the end are dropped at their MFMA.
    const int n = s_end - s;
    const int nb = (n + U - 1) / U;
    if (nb > 0) {
        u32x4 a[NW][U], b[U];
        load_batch<NW, U>(a, b, wp, xp, s, s_end);
        for (int i = 1; i < nb; ++i) {
            u32x4 an[NW][U], bn[U];
            load_batch<NW, U>(an, bn, wp, xp, s + i * U, s_end);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < NW; ++j) { acc[j] = mfma<F>(a[j][u], b[u], acc[j]); a[j][u] = an[j][u]; }
                b[u] = bn[u];
            }
        }
        const int left = n - (nb - 1) * U;                  // 1..U steps of the last batch are real
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < left) {
#pragma unroll
                for (int j = 0; j < NW; ++j) acc[j] = mfma<F>(a[j][u], b[u], acc[j]);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < NW; ++i) part[i][wave][lane] = acc[i];
    __syncthreads();
    if (wave != 0 || !row_live) return;

    f32x4 sum[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        sum[i] = part[i][0][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum[i] += part[i][w][lane];
    }
    if constexpr (P::kBias) {
        if (bp) {                                           // uniform over the workgroup
            sum[0][0] += u2f<F>(bias.x & 0xffffu);
            sum[0][1] += u2f<F>(bias.x >> 16);
            sum[0][2] += u2f<F>(bias.y & 0xffffu);
            sum[0][3] += u2f<F>(bias.y >> 16);
        }
    }
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (NW == 1) o[j] = f2u<F>(sum[0][j]);
        else {
            const float g = rnd<F>(sum[0][j]), up = rnd<F>(sum[1][j]);
            const float sg = rnd<F>(g * smt_sigmoid(g));
            o[j] = f2u<F>(sg * up);
        }
    }
    uint16_t* yp = (NW == 1 ? p.y[out] + (int64_t)r * p.ldy[out] : p.y[0] + (int64_t)r * p.ldy[0]) + n0 + 4 * h;
    *reinterpret_cast<uint2*>(yp) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
}


// ---------------------------------------------------------------------------------------------- e4m3 operands
struct Fp8Params {
    const uint8_t* x;
    int64_t ldx;
    const float* sx;
    const uint8_t* w[SMT_LINEAR_MAX_OUT];
    const float* sw[SMT_LINEAR_MAX_OUT];
    int64_t ldw[SMT_LINEAR_MAX_OUT];
    uint16_t* y[SMT_LINEAR_MAX_OUT];
    int64_t ldy[SMT_LINEAR_MAX_OUT];
    int32_t tile_end[SMT_LINEAR_MAX_OUT];
    int32_t M, K;
};

// load_batch on bytes: a step is 64 bytes of a row here too.
template <int NW, int U>
__device__ __forceinline__ void load_batch8(u32x4 (&a)[NW][U], u32x4 (&b)[U], const uint8_t* const (&wp)[NW],
                                            const uint8_t* xp, int s, int s_end) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t off = (int64_t)min(s + u, s_end - 1) * 64;
#pragma unroll
        for (int i = 0; i < NW; ++i) a[i][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[i] + off));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) b[u] = *reinterpret_cast<const u32x4*>(xp + (int64_t)min(s + u, s_end - 1) * 64);
}

// one step: the low 8 bytes of both operands, then the high 8
__device__ __forceinline__ f32x4 mfma8(const u32x4 a, const u32x4 b, f32x4 c) {
    using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, u32x2{a.x, a.y}),
                                                   __builtin_bit_cast(long, u32x2{b.x, b.y}), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, u32x2{a.z, a.w}),
                                                      __builtin_bit_cast(long, u32x2{b.z, b.w}), c, 0, 0, 0);
}

// F: the output dtype. The schedule is skinny_kernel's.
template <int F, int NW, int U>
__global__ __launch_bounds__(THREADS)
void skinny_fp8_kernel(const Fp8Params p) {
    __shared__ f32x4 part[NW][WAVES][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, h = lane >> 4;

    int out = 0, tile = blockIdx.x;
    if constexpr (NW == 1) {
        out = (tile >= p.tile_end[0]) + (tile >= p.tile_end[1]);
        if (out) tile -= p.tile_end[out - 1];
    }
    const int n0 = tile * 16;
    const uint8_t* wp[NW];
    if constexpr (NW == 1) wp[0] = p.w[out] + (int64_t)(n0 + r) * p.ldw[out] + 16 * h;
    else {
        wp[0] = p.w[0] + (int64_t)(n0 + r) * p.ldw[0] + 16 * h;
        wp[1] = p.w[1] + (int64_t)(n0 + r) * p.ldw[1] + 16 * h;
    }
    const bool row_live = r < p.M;                  // rows >= M: row 0's bytes, the column is dropped
    const uint8_t* xp = p.x + (int64_t)(row_live ? r : 0) * p.ldx + 16 * h;

    const int steps = p.K >> 6;
    const int per = (steps + WAVES - 1) / WAVES;
    const int s = wave * per;
    const int s_end = min(steps, s + per);

    f32x4 acc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int n = s_end - s;
    const int nb = (n + U - 1) / U;
    if (nb > 0) {
        u32x4 a[NW][U], b[U];
        load_batch8<NW, U>(a, b, wp, xp, s, s_end);
        for (int i = 1; i < nb; ++i) {
            u32x4 an[NW][U], bn[U];
            load_batch8<NW, U>(an, bn, wp, xp, s + i * U, s_end);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < NW; ++j) { acc[j] = mfma8(a[j][u], b[u], acc[j]); a[j][u] = an[j][u]; }
                b[u] = bn[u];
            }
        }
        const int left = n - (nb - 1) * U;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < left) {
#pragma unroll
                for (int j = 0; j < NW; ++j) acc[j] = mfma8(a[j][u], b[u], acc[j]);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < NW; ++i) part[i][wave][lane] = acc[i];
    __syncthreads();
    if (wave != 0 || !row_live) return;

    // lane l: features n0 + 4 (l >> 4) + 0..3 of row l & 15; sx of a live row only
    const float sx = p.sx[r];
    f32x4 v[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        f32x4 sum = part[i][0][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum += part[i][w][lane];
        const f32x4 sw = *reinterpret_cast<const f32x4*>(p.sw[NW == 1 ? out : i] + n0 + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = sum[j] * (sx * sw[j]);
    }
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (NW == 1) o[j] = f2u<F>(v[0][j]);
        else {
            const float g = rnd<F>(v[0][j]), up = rnd<F>(v[1][j]);
            const float sg = rnd<F>(g * smt_sigmoid(g));
            o[j] = f2u<F>(sg * up);
        }
    }
    uint16_t* yp = (NW == 1 ? p.y[out] + (int64_t)r * p.ldy[out] : p.y[0] + (int64_t)r * p.ldy[0]) + n0 + 4 * h;
    *reinterpret_cast<uint2*>(yp) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
}

// KSTEP: the K-elements of one step, 32 (16-bit operands) or 64 (bytes)
template <int KSTEP, typename Out>
const char* check_sizes(int32_t M, int32_t K, const Out* outs, int32_t n_out, int32_t epilogue) {
    if (M < 1 || M > SMT_LINEAR_MAX_M) return "M must lie in [1, 16]";
    if (K < KSTEP || (K % KSTEP)) return KSTEP == 32 ? "K must be a positive multiple of 32" : "K must be a positive multiple of 64";
    if (epilogue != SMT_SKINNY_PLAIN && epilogue != SMT_SKINNY_SWIGLU) return "unknown epilogue";
    if (n_out < 1 || n_out > SMT_LINEAR_MAX_OUT) return "n_out must lie in [1, 3]";
    if (!outs) return "null outs";
    int64_t tiles = 0;
    for (int i = 0; i < n_out; ++i) {
        if (outs[i].N < 16 || (outs[i].N & 15)) return "N must be a positive multiple of 16";
        tiles += outs[i].N / 16;
    }
    if (tiles > 0x7fffffffLL) return "too many output features (grid size)";
    if (epilogue == SMT_SKINNY_SWIGLU && (n_out != 2 || outs[0].N != outs[1].N)) return "SWIGLU takes two outputs of equal N";
    return nullptr;
}

// The checks of smt_linear_skinny (sizes, null pointers and extents: -1; alignment: -2) and, if they pass, the
// kernel's parameters and its grid. `fn` names the entry point in the message.
int fill_params(const char* fn, const void* x, int64_t ldx, int32_t M, int32_t K, int32_t dtype, const SmtSkinnyOut* outs,
                int32_t n_out, int32_t epilogue, Params& p, uint32_t& grid) {
    if (const char* why = check_sizes<32>(M, K, outs, n_out, epilogue)) return fail(-1, "%s: %s", fn, why);
    if (dtype != SMT_DTYPE_BF16 && dtype != SMT_DTYPE_FP16)
        return fail(-1, "%s: dtype %d is not SMT_DTYPE_BF16 / _FP16", fn, (int)dtype);
    const int n_y = epilogue == SMT_SKINNY_SWIGLU ? 1 : n_out;
    if (!x) return fail(-1, "%s: null x", fn);
    if (ldx < K) return fail(-1, "%s: ldx %lld < K %d", fn, (long long)ldx, (int)K);
    for (int i = 0; i < n_out; ++i) {
        if (!outs[i].w || (i < n_y && !outs[i].y)) return fail(-1, "%s: null w or y of output %d", fn, i);
        if (outs[i].ldw < K || (i < n_y && outs[i].ldy < outs[i].N))
            return fail(-1, "%s: ldw or ldy of output %d below its extent", fn, i);
    }
    if (!aligned16(x) || (ldx & 7)) return fail(-2, "%s: x must be 16-byte aligned, ldx %lld a multiple of 8", fn, (long long)ldx);
    for (int i = 0; i < n_out; ++i) {
        if (!aligned16(outs[i].w) || (outs[i].ldw & 7) || (i < n_y && (!aligned16(outs[i].y) || (outs[i].ldy & 7))))
            return fail(-2, "%s: w, y of output %d must be 16-byte aligned, ldw, ldy multiples of 8", fn, i);
    }
    p.x = static_cast<const uint16_t*>(x);
    p.ldx = ldx;
    p.M = M;
    p.K = K;
    int32_t tiles = 0;
    for (int i = 0; i < SMT_LINEAR_MAX_OUT; ++i) {
        if (i < n_out) {
            p.w[i] = static_cast<const uint16_t*>(outs[i].w);
            p.ldw[i] = outs[i].ldw;
            p.y[i] = static_cast<uint16_t*>(outs[i].y);
            p.ldy[i] = outs[i].ldy;
            tiles += outs[i].N / 16;
        }
        p.tile_end[i] = tiles;
    }
    grid = (uint32_t)(epilogue == SMT_SKINNY_SWIGLU ? outs[0].N / 16 : tiles);
    return 0;
}

template <int F>
int launch(const Params& p, int32_t epilogue, uint32_t grid, hipStream_t stream) {
    if (epilogue == SMT_SKINNY_SWIGLU)
        hipLaunchKernelGGL((skinny_kernel<F, 2, 4>), dim3(grid), dim3(THREADS), 0, stream, p);
    else
        hipLaunchKernelGGL((skinny_kernel<F, 1, 8>), dim3(grid), dim3(THREADS), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "smt_linear_skinny: %s", hipGetErrorString(e));
    return 0;
}

template <int F>
int launch_fp8(const Fp8Params& p, int32_t epilogue, uint32_t grid, hipStream_t stream) {
    if (epilogue == SMT_SKINNY_SWIGLU)
        hipLaunchKernelGGL((skinny_fp8_kernel<F, 2, 4>), dim3(grid), dim3(THREADS), 0, stream, p);
    else
        hipLaunchKernelGGL((skinny_fp8_kernel<F, 1, 8>), dim3(grid), dim3(THREADS), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "smt_linear_skinny_fp8: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char* smt_linear_last_error(void) { return g_err; }

int64_t smt_linear_skinny_workspace(int32_t M, int32_t K, const SmtSkinnyOut* outs, int32_t n_out, int32_t epilogue) {
    if (const char* why = check_sizes<32>(M, K, outs, n_out, epilogue)) return fail(-1, "smt_linear_skinny_workspace: %s", why);
    return 0;
}

int smt_linear_skinny(const void* x, int64_t ldx, int32_t M, int32_t K, int32_t dtype, const SmtSkinnyOut* outs,
                      int32_t n_out, int32_t epilogue, void* workspace, hipStream_t stream) {
    (void)workspace;
    Params p = {};
    uint32_t grid = 0;
    if (const int rc = fill_params("smt_linear_skinny", x, ldx, M, K, dtype, outs, n_out, epilogue, p, grid)) return rc;
    if (dtype == SMT_DTYPE_BF16) return launch<SMT_DTYPE_BF16>(p, epilogue, grid, stream);
    return launch<SMT_DTYPE_FP16>(p, epilogue, grid, stream);
}

int smt_linear_skinny_bias(const void* x, int64_t ldx, int32_t M, int32_t K, int32_t dtype, const SmtSkinnyOut* outs,
                           const void* const* biases, int32_t n_out, int32_t epilogue, void* workspace,
                           hipStream_t stream) {
    (void)workspace;
    BiasParams p = {};
    uint32_t grid = 0;
    if (const int rc = fill_params("smt_linear_skinny_bias", x, ldx, M, K, dtype, outs, n_out, epilogue, p, grid)) return rc;
    if (!biases) return fail(-1, "smt_linear_skinny_bias: null biases (an array of n_out pointers, each of which may be null)");
    bool any = false;
    for (int i = 0; i < n_out; ++i) {
        p.b[i] = static_cast<const uint16_t*>(biases[i]);
        any = any || biases[i];
    }
    if (any && epilogue != SMT_SKINNY_PLAIN) return fail(-1, "smt_linear_skinny_bias: a bias goes with SMT_SKINNY_PLAIN only");
    for (int i = 0; i < n_out; ++i)
        if (!aligned16(biases[i])) return fail(-2, "smt_linear_skinny_bias: the bias of output %d must be 16-byte aligned", i);
    if (!any) {                                              // nothing to add: the plain kernels
        if (dtype == SMT_DTYPE_BF16) return launch<SMT_DTYPE_BF16>(p, epilogue, grid, stream);
        return launch<SMT_DTYPE_FP16>(p, epilogue, grid, stream);
    }
    if (dtype == SMT_DTYPE_BF16) hipLaunchKernelGGL((skinny_kernel<SMT_DTYPE_BF16, 1, 8, BiasParams>), dim3(grid), dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((skinny_kernel<SMT_DTYPE_FP16, 1, 8, BiasParams>), dim3(grid), dim3(THREADS), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "smt_linear_skinny_bias: %s", hipGetErrorString(e));
    return 0;
}

int64_t smt_linear_skinny_fp8_workspace(int32_t M, int32_t K, const SmtSkinnyFp8Out* outs, int32_t n_out,
                                        int32_t epilogue) {
    if (const char* why = check_sizes<64>(M, K, outs, n_out, epilogue)) return fail(-1, "smt_linear_skinny_fp8_workspace: %s", why);
    return 0;
}

int smt_linear_skinny_fp8(const void* x8, int64_t ldx, const float* sx, int32_t M, int32_t K, int32_t out_dtype,
                          const SmtSkinnyFp8Out* outs, int32_t n_out, int32_t epilogue, void* workspace,
                          hipStream_t stream) {
    (void)workspace;
    if (const char* why = check_sizes<64>(M, K, outs, n_out, epilogue)) return fail(-1, "smt_linear_skinny_fp8: %s", why);
    if (out_dtype != SMT_DTYPE_BF16 && out_dtype != SMT_DTYPE_FP16)
        return fail(-1, "smt_linear_skinny_fp8: out_dtype %d is not SMT_DTYPE_BF16 / _FP16", (int)out_dtype);
    const int n_y = epilogue == SMT_SKINNY_SWIGLU ? 1 : n_out;
    if (!x8 || !sx) return fail(-1, "smt_linear_skinny_fp8: null x8 or sx");
    if (ldx < K) return fail(-1, "smt_linear_skinny_fp8: ldx %lld < K %d", (long long)ldx, (int)K);
    for (int i = 0; i < n_out; ++i) {
        if (!outs[i].w8 || !outs[i].sw || (i < n_y && !outs[i].y))
            return fail(-1, "smt_linear_skinny_fp8: null w8, sw or y of output %d", i);
        if (outs[i].ldw < K || (i < n_y && outs[i].ldy < outs[i].N))
            return fail(-1, "smt_linear_skinny_fp8: ldw or ldy of output %d below its extent", i);
    }
    if (!aligned16(x8) || (ldx & 15) || (reinterpret_cast<uintptr_t>(sx) & 3u))
        return fail(-2, "smt_linear_skinny_fp8: x8 must be 16-byte aligned, ldx %lld a multiple of 16, sx 4-byte aligned", (long long)ldx);
    for (int i = 0; i < n_out; ++i) {
        if (!aligned16(outs[i].w8) || !aligned16(outs[i].sw) || (outs[i].ldw & 15) ||
            (i < n_y && (!aligned16(outs[i].y) || (outs[i].ldy & 7))))
            return fail(-2, "smt_linear_skinny_fp8: w8, sw, y of output %d must be 16-byte aligned, ldw a multiple of 16, ldy of 8", i);
    }
    Fp8Params p = {};
    p.x = static_cast<const uint8_t*>(x8);
    p.ldx = ldx;
    p.sx = sx;
    p.M = M;
    p.K = K;
    int32_t tiles = 0;
    for (int i = 0; i < SMT_LINEAR_MAX_OUT; ++i) {
        if (i < n_out) {
            p.w[i] = static_cast<const uint8_t*>(outs[i].w8);
            p.sw[i] = outs[i].sw;
            p.ldw[i] = outs[i].ldw;
            p.y[i] = static_cast<uint16_t*>(outs[i].y);
            p.ldy[i] = outs[i].ldy;
            tiles += outs[i].N / 16;
        }
        p.tile_end[i] = tiles;
    }
    const uint32_t grid = (uint32_t)(epilogue == SMT_SKINNY_SWIGLU ? outs[0].N / 16 : tiles);
    if (out_dtype == SMT_DTYPE_BF16) return launch_fp8<SMT_DTYPE_BF16>(p, epilogue, grid, stream);
    return launch_fp8<SMT_DTYPE_FP16>(p, epilogue, grid, stream);
}

}  // extern "C"
