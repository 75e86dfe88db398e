/*
 * smt_beam.h — C-ABI of the beam-search scoring step (csrc/beam_kernels.hip, same library
 * libsmt_hip.so): steps b and c of transformers' GenerationMixin._beam_search for one token --
 * logits.float() -> log_softmax -> RepetitionPenaltyLogitsProcessor -> MinLength / MinNewTokensLength
 * suppression -> + running beam scores -> reshape [N, nb*V] -> topk(K) -- as one call that reads the
 * logits in their own format and writes K candidates per sample. No [R, V] fp32 tensor exists anywhere.
 *
 * Row r = n*nb + beam of `logits` belongs to beam `beam` of sample n. In fp32, for token v of a row:
 *   lp    = x_v - lse_row                      lse_row = log(sum_v exp(x_v)) of the row's V values
 *   lp    = lp < 0 ? lp * penalty : lp / penalty      if v occurs in sequences[row][0 .. cur_len)
 *   lp    = -inf                                       if v is one of the n_suppressed ids
 *   score = lp + beam_scores[row]
 * top_scores[n][0 .. K) are the K largest scores of sample n's nb*V candidates in descending order,
 * top_index[n][j] their flat index beam*V + v. Equal scores are ordered by lower flat index.
 *
 * Deterministic: no atomics, a fixed reduction order, bit-reproducible results. A row's lse is a
 * function of its V values and of V alone (not of the row index, N or nb): the row is cut into chunks
 * of SMT_BEAM_CHUNK elements, each reduced by one workgroup in a fixed order, and the chunk partials
 * are combined in a fixed order.
 *
 * Memory safety for any contents: a history id outside [0, V) is ignored and never forms an address;
 * columns >= V of a row are never read; a NaN logit may make that sample's result unspecified, but
 * every index written lies in [0, nb*V).
 *
 * Three launches on `stream`, no host synchronisation, no allocation: `workspace` (16-byte aligned,
 * smt_beam_topk_workspace bytes) holds the per-chunk partials (max and sum of exponentials, and the
 * chunk's K best candidates).
 * Return 0, -1 (invalid argument, before any HIP call), -2 (misaligned pointer or row), -4 (launch
 * failure); smt_beam_last_error() holds the message.
 */
#ifndef SMT_BEAM_H
#define SMT_BEAM_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_BEAM_CHUNK 2048        /* elements of a row one workgroup reduces */
#define SMT_BEAM_MAX_K 32
#define SMT_BEAM_MAX_SUPPRESSED 8

const char* smt_beam_last_error(void);

/* Bytes of workspace for smt_beam_topk with these sizes; -1 if they are invalid. */
int64_t smt_beam_topk_workspace(int32_t N, int32_t nb, int64_t V, int32_t K);

/* logits: [N*nb][ld] of `dtype` (SMT_DTYPE_BF16 / _FP32 / _FP16 of smt_hip.h), ld >= V, 16-byte aligned
 * rows. beam_scores: fp32 [N*nb]. sequences: int64 [N*nb][seq_ld], entries [0, cur_len) the row's token
 * history (may be NULL when cur_len == 0). penalty > 0. suppressed: HOST array of n_suppressed <= 8 ids.
 * 1 <= K <= 32, K <= nb*V, nb*V < 2^31. top_scores: fp32 [N][K]; top_index: int32 [N][K]. */
int smt_beam_topk(const void* logits, int64_t ld, int32_t dtype, int32_t N, int32_t nb, int64_t V,
                  const float* beam_scores, const int64_t* sequences, int64_t seq_ld, int32_t cur_len,
                  float penalty, const int64_t* suppressed, int32_t n_suppressed, int32_t K,
                  float* top_scores, int32_t* top_index, void* workspace, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMT_BEAM_H */
