/*
 * smt_linear.h — C-ABI of the decode linears (csrc/linear_kernels.hip, same library libsmt_hip.so):
 * y[M, N] = x[M, K] * W[N, K]^T for 1 <= M <= 16 rows, the shape of every dense linear of a decode step
 * (prompts x beams rows). At these M a GEMM is one read of W with a trivial amount of arithmetic, so the
 * kernel is a weight stream: W is read once, as it lies in the model (nn.Linear.weight, row-major [N][K],
 * no repack and no copy), with non-temporal 16-byte loads straight into the A operand of
 * v_mfma_f32_16x16x32_{bf16,f16}; x is the B operand. fp32 accumulation, one rounding to the dtype at
 * the store.
 *
 * Sizes and alignment: K % 32 == 0, N % 16 == 0; ldx, ldw, ldy multiples of 8 elements with ldx >= K,
 * ldw >= K, ldy >= N; every pointer 16-byte aligned. K / 32 need not divide by anything.
 *
 * Determinism: no atomics, a fixed reduction order, bit-reproducible. One workgroup owns 16 output
 * features; its SMT_LINEAR_KSPLIT waves take one contiguous K-slice each (a function of K alone) and
 * their fp32 partials are added in wave order through the LDS. The x row is a COLUMN of the MFMA, and
 * columns never mix, so a row's output is a function of that row of x and of W alone: not of M, of the
 * row's index, or of what the other rows hold.
 *
 * Memory: rows >= M of x are never read; nothing of y is written outside [0, M) x [0, N).
 *
 * No synchronisation between workgroups: no persistent loop, no grid barrier, no spin, no ticket, no
 * split of K across workgroups. smt_linear_skinny_workspace therefore returns 0 for every valid shape
 * and `workspace` may be NULL; both exist so that a later split-K form (fp32 partials plus a second,
 * ordinary launch) needs no ABI change.
 *
 * One launch on `stream`, no allocation, no host synchronisation; launch parameters depend on shapes and
 * pointers only, so a captured call replays.
 * Return 0, -1 (invalid argument, before any HIP call), -2 (misaligned pointer or leading dimension,
 * before any HIP call), -4 (launch failure); smt_linear_last_error() holds the message.
 */
#ifndef SMT_LINEAR_H
#define SMT_LINEAR_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_LINEAR_MAX_M 16
#define SMT_LINEAR_MAX_OUT 3
#define SMT_LINEAR_KSPLIT 8       /* fp32 partials combined per output element, in a fixed order */

typedef struct {
    const void* w;                /* [N][ldw] of the call's dtype */
    int64_t ldw;
    void* y;                      /* [M][ldy] of the call's dtype */
    int64_t ldy;
    int32_t N;
    int32_t reserved;
} SmtSkinnyOut;

#define SMT_SKINNY_PLAIN 0        /* y_i = x * W_i^T for each of n_out (1..3) outputs: one launch reads x once */
#define SMT_SKINNY_SWIGLU 1       /* n_out == 2, equal N: outs[0].y = swiglu(x * W_0^T, x * W_1^T); outs[1].y unused.
                                     Gate and up are each rounded to the dtype first, then the arithmetic of the
                                     SwiGLU forward of smt_model_ops.h, dtype(silu(g)) * u: bit for bit the chain of
                                     two PLAIN calls and that kernel. */

const char* smt_linear_last_error(void);

/* Bytes of workspace for smt_linear_skinny with these sizes (0 today); -1 if they are invalid. */
int64_t smt_linear_skinny_workspace(int32_t M, int32_t K, const SmtSkinnyOut* outs, int32_t n_out, int32_t epilogue);

/* x: [M][ldx] of `dtype` (SMT_DTYPE_BF16 / SMT_DTYPE_FP16 of smt_hip.h). outs: HOST array of n_out entries. */
int smt_linear_skinny(const void* x, int64_t ldx, int32_t M, int32_t K, int32_t dtype, const SmtSkinnyOut* outs,
                      int32_t n_out, int32_t epilogue, void* workspace, hipStream_t stream);

/*
 * smt_linear_skinny with a bias per output (the q, k and v projections of a Qwen2 model):
 *
 *     y[m][n] = RN_out( acc[m][n] + (float)b[n] ),
 *
 * acc the sum of the SMT_LINEAR_KSPLIT partials in wave order, as above; the add is one fp32 add in wave 0 and
 * the store's rounding is the only rounding to the dtype.
 * biases: HOST array of n_out device pointers. biases[i] is NULL (output i has no bias: its y is bit for bit
 * smt_linear_skinny's) or points to b [N_i] of the call's dtype, 16-byte aligned, unit stride. A workgroup reads
 * the 16 features of its tile once (32 bytes, wave 0, default cache policy).
 * SMT_SKINNY_PLAIN only: SMT_SKINNY_SWIGLU with any non-NULL entry returns -1. With every entry NULL the call
 * is smt_linear_skinny's launch, either epilogue.
 * Everything else is smt_linear_skinny's contract: a row's output is a function of that row of x, of W and of
 * b alone; rows >= M of x are never read; nothing of y is written outside [0, M) x [0, N); no synchronisation
 * between workgroups, workspace 0 (smt_linear_skinny_workspace answers for this call too); one launch, no
 * allocation, launch parameters from shapes and pointers only, so a captured call replays; the same return
 * codes, with -1 for a NULL `biases` and -2 for a misaligned bias, before any HIP call.
 */
int smt_linear_skinny_bias(const void* x, int64_t ldx, int32_t M, int32_t K, int32_t dtype, const SmtSkinnyOut* outs,
                           const void* const* biases, int32_t n_out, int32_t epilogue, void* workspace,
                           hipStream_t stream);

/*
 * The same stream on e4m3 operands (the fp8 path's frozen linears): x8 [M][ldx] e4m3fn bytes with one fp32
 * scale per row, sx [M]; each of the 1..3 outputs w8 [N][ldw] e4m3fn bytes with one fp32 scale per output
 * feature, sw [N]: exactly what smt_quant_rows_e4m3 (smt_fp8.h) writes. y is bf16 or fp16 (`out_dtype`).
 *
 *     y[m][n] = RN_out( RN32( acc[m][n] * RN32(sx[m] * sw[n]) ) ),
 *     acc[m][n] = sum_k dec(x8[m][k]) * dec(w8[n][k])  in fp32
 *
 * The order of the two scale multiplications is part of the contract: first the two scales, rounded to fp32,
 * then the accumulator times that product, rounded to fp32, then one rounding to the output dtype.
 *
 * A step is 64 K-elements of a 16-feature tile: one non-temporal 16-byte load per lane of w8, one default-
 * policy 16-byte load of x8, and two v_mfma_f32_16x16x32_fp8_fp8 (bytes 0..7 and 8..15 of the two loads; the
 * instruction pairs slot j of a lane's A bytes with slot j of the same lane group's B bytes, so any
 * assignment of bytes to K positions is right when both operands use the same one). The block-scaled
 * 16x16x128 form would take 32 bytes per lane and operand and force K % 128; at these shapes the kernel waits
 * for memory, not for the matrix core, so its higher rate buys nothing.
 *
 * Sizes and alignment: K % 64 == 0, N % 16 == 0; ldx, ldw multiples of 16 (bytes) with ldx >= K, ldw >= K;
 * ldy a multiple of 8 elements, ldy >= N; x8, w8, sw and y 16-byte aligned (sx: 4-byte).
 * Everything else is smt_linear_skinny's contract: SMT_LINEAR_KSPLIT contiguous K-slices (of the K / 64
 * steps) added in wave order, no atomics, bit-reproducible; a row's output is a function of that row of x8,
 * its sx and of the weights alone; rows >= M of x8 and sx are never read; nothing of y is written outside
 * [0, M) x [0, N); no synchronisation between workgroups, so the workspace query returns 0; one launch, no
 * allocation, launch parameters from shapes and pointers only; the same return codes.
 *
 * SMT_SKINNY_PLAIN: n_out 1..3, each output with its own sw; x8 is read once. SMT_SKINNY_SWIGLU: n_out == 2,
 * equal N; the scaled gate and up are each rounded to the dtype first, then the SwiGLU forward of
 * smt_model_ops.h: bit for bit the chain of two PLAIN calls and that kernel.
 */
typedef struct {
    const void* w8;               /* [N][ldw] e4m3fn bytes */
    const float* sw;              /* [N] */
    int64_t ldw;
    void* y;                      /* [M][ldy] of out_dtype */
    int64_t ldy;
    int32_t N;
    int32_t reserved;
} SmtSkinnyFp8Out;

/* Bytes of workspace for smt_linear_skinny_fp8 with these sizes (0 today); -1 if they are invalid. */
int64_t smt_linear_skinny_fp8_workspace(int32_t M, int32_t K, const SmtSkinnyFp8Out* outs, int32_t n_out,
                                        int32_t epilogue);

/* out_dtype: SMT_DTYPE_BF16 / SMT_DTYPE_FP16. outs: HOST array of n_out entries. */
int smt_linear_skinny_fp8(const void* x8, int64_t ldx, const float* sx, int32_t M, int32_t K, int32_t out_dtype,
                          const SmtSkinnyFp8Out* outs, int32_t n_out, int32_t epilogue, void* workspace,
                          hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMT_LINEAR_H */
