/*
 * smt_sample.h — C-ABI of token selection for num_beams == 1 (csrc/sample_kernels.hip, same library
 * libsmt_hip.so): what transformers' GenerationMixin._sample does between the model's logits and the
 * next token -- logits.float() -> RepetitionPenaltyLogitsProcessor -> MinLength / MinNewTokensLength
 * suppression -> TemperatureLogitsWarper -> TopK / TopP / MinP warpers -> softmax -> multinomial (or
 * argmax) -- as one deterministic call that reads the logits in their own format. No whole-vocabulary
 * sort, no [R, V] tensor outside `workspace`, launch count and time independent of top_k.
 *
 * Per row r the values below are fp32 and every operation is one correctly rounded fp32 operation
 * (the library is built without fast-math):
 *   1. y_v = x_v;  y_v = x_v < 0 ? x_v * penalty : x_v / penalty  if v occurs in sequences[r][0 .. cur_len)
 *      (the penalty acts on the logits, as in _sample, not on log-probabilities);  y_v = -inf if v is one
 *      of the n_suppressed ids.
 *   2. z_v = y_v / temperature, a true division, and -0 becomes +0. This is what torch computes on the
 *      CPU for `scores / temperature`. Whether torch's device kernel multiplies by a reciprocal instead
 *      has not been checked: nothing here is pinned to torch's device chain.
 *   3. top-k (top_k <= 0 or >= V: off): t_k is the k-th largest z; v survives iff z_v >= t_k. Exact;
 *      ties at t_k all survive, as transformers' `scores < kth` keeps them.
 *   4. top-p (top_p >= 1: off), in real arithmetic over the survivors of 3: w_v = exp(z_v - M), M the
 *      row's maximum, W = sum w, c(v) = sum_{j: z_j <= z_v} w_j / W. v is removed iff c(v) <= thr with
 *      thr = (float)(1.0 - (double)top_p), computed on the host; every v with z_v == M is kept. Equal
 *      values are kept or removed together. transformers cuts inside a group of equal values wherever
 *      its unstable sort put the members, so this set is a superset of transformers' and the difference
 *      lies inside the one tie group at the threshold.
 *   5. min-p (min_p <= 0: off), on what is left: v is removed iff z_v - M < log(min_p) (the device
 *      compares fl(z_v - M) with (float)log((double)min_p)). The maximum always stays.
 *   6. All three are value thresholds: the kept set is {v : z_v >= threshold[r]}. threshold[r] is the
 *      smallest kept z as its exact fp32 value, kept[r] the size of the set.
 *   7. mode 0 (greedy): token[r] = argmax_v z_v, the lowest id among equal values. Exact.
 *   8. mode 1 (sample): the Gumbel-max draw. token[r] = argmax over the kept set of fl(z_v + g_v), the
 *      lowest id among equal values, with
 *        g_v     = -logf(-logf(u_v))
 *        u_v     = min(fl(fl((float)(word >> 8) + 0.5f) * 2^-24), 1 - 2^-24)      (so 0 < u_v < 1)
 *        word    = mix(row_key ^ (v * 0x9E3779B1))
 *        row_key = mix((mix(seed_lo + (row0 + r) * 0x9E3779B9) ^ seed_hi) + step * 0x85EBCA6B)
 *        mix(x):   x ^= x >> 16; x *= 0x21F0AAAD; x ^= x >> 15; x *= 0x735A2D97; x ^= x >> 15
 *      on uint32 with wrap-around (mix is that of smt_attention.h; seed_lo / seed_hi are the halves of
 *      `seed`). The draw is part of the contract: a pure function of (seed, step, row0 + r, v) and z.
 *      Parity unpinned: it is not torch's Philox stream, so a sampled run equals torch.multinomial's in
 *      distribution only.
 *
 * The device evaluates 4 as  mass{j : z_j > z_v} < (1 - thr) * W  on 64-bit fixed-point masses
 * round(expf(fl(z_j - M)) * 2^40), added as integers: the sums do not depend on the order, and the
 * rounding is at most 2^-41 per term against W >= 1.
 *
 * Deterministic: no atomics on floats, a fixed reduction order, bit-reproducible results. threshold[r],
 * kept[r] and token[r] are a function of row r's data and (seed, step, row0 + r): not of R or of what
 * the other rows hold.
 *
 * Memory safety for any contents: a history id outside [0, V) is ignored and never forms an address;
 * columns >= V of a row are never read; every token written lies in [0, V), even for NaN input, for
 * which the result is otherwise unspecified.
 *
 * Two launches on `stream`, no host synchronisation, no allocation: `workspace` (16-byte aligned,
 * smt_sample_workspace bytes) holds z, the candidate list of the selection and the chunk maxima.
 * Return 0, -1 (invalid argument, before any HIP call), -2 (misaligned pointer or row), -4 (launch
 * failure); smt_sample_last_error() holds the message.
 */
#ifndef SMT_SAMPLE_H
#define SMT_SAMPLE_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_SAMPLE_CHUNK 2048        /* elements of a row one workgroup of the first launch handles */
#define SMT_SAMPLE_MAX_SUPPRESSED 8
#define SMT_SAMPLE_GREEDY 0
#define SMT_SAMPLE_DRAW 1

const char* smt_sample_last_error(void);

/* Bytes of workspace for smt_sample_token with these sizes; -1 if they are invalid. */
int64_t smt_sample_workspace(int32_t R, int64_t V);

/* logits: [R][ld] of `dtype` (SMT_DTYPE_BF16 / _FP32 / _FP16 of smt_hip.h), ld >= V, 16-byte aligned
 * rows, V < 2^31. sequences: int64 [R][seq_ld], entries [0, cur_len) the row's token history (may be NULL
 * when cur_len == 0). penalty > 0. suppressed: HOST array of n_suppressed <= 8 ids. temperature > 0,
 * top_p > 0, min_p <= 1. mode: SMT_SAMPLE_GREEDY or SMT_SAMPLE_DRAW. token: int32 [R]; threshold: fp32 [R];
 * kept: int32 [R]. */
int smt_sample_token(const void* logits, int64_t ld, int32_t dtype, int32_t R, int64_t V,
                     const int64_t* sequences, int64_t seq_ld, int32_t cur_len, float penalty,
                     const int64_t* suppressed, int32_t n_suppressed, float temperature, int32_t top_k,
                     float top_p, float min_p, int32_t mode, uint64_t seed, uint32_t step, uint32_t row0,
                     int32_t* token, float* threshold, int32_t* kept, void* workspace, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMT_SAMPLE_H */
