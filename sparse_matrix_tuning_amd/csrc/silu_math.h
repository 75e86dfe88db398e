// SiLU pieces shared by every SwiGLU kernel (llama_kernels.hip, and the fp8 fusions in
// fp8_kernels.hip, which must produce bit-identical bf16 values to the unfused kernels).
// sigmoid(x) = 1 / (1 + 2^(-x log2 e)) with the hardware v_exp_f32 / v_rcp_f32 (about 1 ulp each)
// instead of the libm-accurate expf and an IEEE division: a few fp32 ulps from transformers' eager
// silu (x / (1 + exp(-x))), i.e. after the bf16 rounding an occasional one-step difference, which
// the tests bound (tests/test_gpu_fused_llama.py, <= 1e-3 of the values one bf16 step apart).
#pragma once

// v_rcp_f32 returns zero where its result would be denormal (e > 2^126, x below about -87.3), while
// the eager sigmoid keeps the denormal until exp overflows (x < -88.7); with an infinite incoming
// gradient the backward then gave 0 * inf = NaN where eager gives inf. There the reciprocal is taken
// of e * 2^-64 + 1 (the 1 is far below half a step of either sum there) and scaled back by a multiply,
// which keeps denormals; elsewhere k = 1, and fma(e, 1, 1) and the multiply by 1 are the same values
// as before. No branch.
__device__ __forceinline__ float smt_sigmoid(float x) {
    const float e = __builtin_amdgcn_exp2f(-x * 1.4426950408889634f);
    const float k = e > 0x1p126f ? 0x1p-64f : 1.0f;
    return __builtin_amdgcn_rcpf(__builtin_fmaf(e, k, 1.0f)) * k;
}
