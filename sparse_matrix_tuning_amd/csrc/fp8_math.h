// e4m3 (OCP float8_e4m3fn) helpers shared by the quantisation kernels (fp8_kernels.hip) and the
// producers that quantise their own output (llama_kernels.hip: RMSNorm).
#pragma once
#include <stdint.h>

constexpr float kE4M3Max = 448.f;
constexpr float kInvE4M3Max = 1.f / 448.f;          // fp32-rounded reciprocal: scale = amax * (1/448)

// x / scale, correctly rounded (so bit-identical to torch's IEEE division) without a per-element
// division: with rs = RN(1/scale), q0 = RN(x * rs) is within an ulp of the quotient, the residual
// q0 * scale - x is exact in one FMA, and RN(q0 - residual * rs) is the correctly rounded quotient
// (Markstein). 1/scale is loop-invariant per row / column, so the one real division is hoisted.
//
// The quotient stays within +-448 (|x| <= amax = 448 * scale), but 1/scale and the residual do not
// stay in range for every finite bf16 row: below scale = 2^-128 (amax < 1.75 * 2^-120) 1/scale is
// inf, and up to amax = 2^-105 the residual can fall below 2^-149 and be rounded. Rows with
// scale < 2^-100 are therefore lifted by 2^64 first, which is exact for x and for scale (both stay
// far below overflow, and subnormal ones become normal) and leaves the quotient unchanged; the
// select and the division are row-uniform, which leaves one multiply per element (qv2: per pair).
//
// The residual is taken as q0 * scale - x and subtracted, not as x - q0 * scale and added: the two
// are the same number, but for x = -0.0 (q0 = -0) the first form gives (-0) + (+0) = +0 and then
// q = (-0) + (-0) = -0, as the division does, where the second gives (+0) + (-0) = +0 and
// q = (+0) + (-0) = +0. x = +0.0 gives +0 either way.
//
// With both the result is the correctly rounded quotient, sign of zero included, for every finite
// bf16 x and every scale e4m3_scale() can return (tests/test_fp8_ref_host.py emulates this form and
// the plain one; tests/test_gpu_fp8_exact.py holds the kernels to it). Non-finite inputs are
// outside the contract.
constexpr float kTinyScale = 0x1p-100f;
constexpr float kTinyLift = 0x1p64f;

// Two quotients at once, the same operations on both halves of a register pair: v_pk_mul_f32 and
// v_pk_fma_f32 run two fp32 lanes per cycle and round each lane as the scalar forms do, which pays
// for the lift's multiply (profiles/r19_fp8_quant_bench.jsonl).
typedef float qv_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ qv_f2 qv2(qv_f2 x, float scale) {
    const float lift = scale < kTinyScale ? kTinyLift : 1.f;
    const float s = scale * lift;
    const float rs = 1.f / s;
    const qv_f2 xl = x * lift;
    const qv_f2 q0 = xl * rs;
    const qv_f2 r = __builtin_elementwise_fma(q0, (qv_f2)(s), -xl);
    const qv_f2 q = __builtin_elementwise_fma(-r, (qv_f2)(rs), q0);
    return qv_f2{__builtin_amdgcn_fmed3f(q.x, kE4M3Max, -kE4M3Max), __builtin_amdgcn_fmed3f(q.y, kE4M3Max, -kE4M3Max)};
}

// four values -> four e4m3 bytes (little endian: a is byte 0)
__device__ __forceinline__ uint32_t pack4(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}

// e4m3 bytes of a / scale, b / scale, c / scale, d / scale
__device__ __forceinline__ uint32_t quant4(float a, float b, float c, float d, float scale) {
    const qv_f2 lo = qv2(qv_f2{a, b}, scale), hi = qv2(qv_f2{c, d}, scale);
    return pack4(lo.x, lo.y, hi.x, hi.y);
}

// the scale of a row / column with this amax (1 for an all-zero one)
__device__ __forceinline__ float e4m3_scale(float amax) { return amax > 0.f ? amax * kInvE4M3Max : 1.f; }
