/*
 * smt_attention.h — C-ABI of the gfx950 causal flash attention (forward + backward) used by the SMT
 * training step, and of the split-KV cached forward that serves generation from a KV cache on the
 * same model (smt_attn_fwd_cached, at the end) (csrc/attn_kernels.hip, same library libsmt_hip.so).
 *
 * Auxiliary to the SMT hot path (smt_hip.h): it replaces the attention of the HF transformers LLaMA
 * decoder that carries the SMT modules (the reference trains that model through
 * AutoModelForCausalLM, deepspeed/fine_tune.py:150-155; transformers' sdpa attention dispatches to
 * aotriton on this torch build). Causal, grouped-query (Hq = G * Hkv), head_dim 128, 16-bit in / out
 * (shape->dtype: SMT_DTYPE_BF16 or, since ABI v13, SMT_DTYPE_FP16 -- the reference's --dtype,
 * fine_tune.py:955-959), fp32 softmax statistics; P and dS are rounded to that format for their
 * products.
 *
 * Tensors are addressed by element strides (d-stride 1, rows 16-byte aligned):
 *   q, o, dq, do   element (b, h, s, d) at base + b*sb + h*sh + s*ss + d,  h < Hq
 *   k, v, dk, dv   element (b, h, s, d) at base + b*sb + h*sh + s*ss + d,  h < Hkv
 *   lse, delta     fp32 [B][Hq][S]; lse in log2 units of the scaled scores:
 *                  lse = log2(sum_j exp2(scale*log2(e) * q.k_j))
 * Returns 0 or a negative code; smt_attn_last_error() holds the message.
 */
#ifndef SMT_ATTENTION_H
#define SMT_ATTENTION_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_ATTN_HEAD_DIM 128

typedef struct smt_attn_tensor {
    void* ptr;
    int64_t sb, sh, ss;             /* element strides of batch, head, sequence */
} smt_attn_tensor;

typedef struct smt_attn_shape {
    int32_t B, Hq, Hkv, S;
    float scale;                    /* softmax scale, usually 1/sqrt(128) */
    int32_t dtype;                  /* ABI v13 (was padding, 0): SMT_DTYPE_BF16 (0) or SMT_DTYPE_FP16 (2) */
} smt_attn_shape;

const char* smt_attn_last_error(void);

/* o = softmax(scale * q k^T + causal mask) v ; lse as above. */
int smt_attn_fwd(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                 const smt_attn_tensor* o, float* lse, const smt_attn_shape* shape, hipStream_t stream);

/*
 * Gradients of smt_attn_fwd. delta_ws: fp32 [B][Hq][S] workspace (delta = rowsum(do * o)).
 * dk / dv sum the G query heads that share a key/value head (no atomics; deterministic).
 */
int smt_attn_bwd(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                 const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                 const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                 const smt_attn_shape* shape, hipStream_t stream);

/*
 * The same with a key mask (ABI v8): the attention of a padded batch, as transformers builds it from
 * the 2-D attention_mask the reference's collator passes (input_ids != pad_token_id,
 * deepspeed/helpers/helper.py:194-204), combined with the causal mask. key_mask: device uint64
 * [B][key_mask_ld], key_mask_ld >= ceil(S / 64); bit (j & 63) of word b*key_mask_ld + (j >> 6) set =
 * key j of batch b takes part. The mask may have holes anywhere (a pad id can occur inside a
 * sequence). A query row whose visible keys are all masked gets o = 0, lse = +inf and zero
 * gradients (torch's safe softmax). key_mask NULL = smt_attn_fwd / smt_attn_bwd.
 */
int smt_attn_fwd_kmask(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                       const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                       const smt_attn_shape* shape, hipStream_t stream);
int smt_attn_bwd_kmask(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                       const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                       const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                       const uint64_t* key_mask, int64_t key_mask_ld, const smt_attn_shape* shape,
                       hipStream_t stream);

/*
 * Attention dropout (additive entry points; the ABI version is unchanged). The probabilities are
 * dropped after the softmax: o = (softmax(...) o M) r v, with M the keep mask and r = 1 / (1 - p_eff).
 * lse is that of the undropped probabilities; a row whose visible keys were all dropped gets o = 0 and
 * a finite lse. The backward applies the same M: dS = P o (M o dP r - delta), dV = (P o M r)^T dO.
 *
 * The keep function is part of the contract. Whether probability (b, h, q, key) survives is a pure
 * function of a 64-bit seed (seed_lo / seed_hi its halves) and those four indices, on uint32 with
 * wrap-around -- never of S, the key mask, the dtype, the strides or which kernel asks:
 *
 *   mix(x):   x ^= x >> 16; x *= 0x21F0AAAD; x ^= x >> 15; x *= 0x735A2D97; x ^= x >> 15
 *   head_key = mix(seed_lo + (b*Hq + h) * 0x9E3779B9) ^ seed_hi
 *   row_key  = mix(head_key + q * 0x85EBCA6B)
 *   word     = mix(row_key ^ ((key >> 2) * 0x9E3779B1))
 *   byte     = (word >> (8 * (key & 3))) & 0xFF
 *   keep     = byte >= t            with t = clamp(floor(p*256 + 0.5), 0, 255)
 *
 * The effective drop rate is p_eff = t / 256 and kept probabilities are scaled by 1 / (1 - p_eff).
 * t == 0 is no dropout: the calls forward to smt_attn_fwd_kmask / smt_attn_bwd_kmask and seed may be
 * NULL. seed: one uint64 in device memory, read by the kernels (no host synchronisation; a graph
 * replay or a recompute that passes the same buffer sees the same masks). The masks are not torch's
 * Philox stream: a run is not mask-for-mask comparable with torch's dropout.
 *
 * p outside [0, 1) or NaN, and a NULL seed with t > 0, return -1 before any HIP call.
 */
int smt_attn_dropout_threshold(float p);      /* t as above, or -1 for p outside [0, 1) or NaN */

int smt_attn_fwd_dropout(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                         const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                         float p, const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream);
int smt_attn_bwd_dropout(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                         const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                         const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                         const uint64_t* key_mask, int64_t key_mask_ld, float p, const uint64_t* seed,
                         const smt_attn_shape* shape, hipStream_t stream);

/*
 * The keep mask itself: keep[((b*Hq + h)*S + q)*S + key] = 1 (kept) or 0 (dropped) for every
 * (b, h, q, key) of a device uint8 [B][Hq][S][S] buffer, from the same device function the three
 * kernels call (only B, Hq and S of the shape are used). A test oracle's input and a debugging aid,
 * not part of the training path.
 */
int smt_attn_dropout_mask(uint8_t* keep, float p, const uint64_t* seed, const smt_attn_shape* shape,
                          hipStream_t stream);

/*
 * Packed sequences (additive entry points; the ABI version is unchanged): several samples concatenated
 * into one row, block-diagonal causal attention. doc_start, doc_end: device int32 [B][S];
 * doc_start[b][i] is the index of the first token of token i's document, doc_end[b][i] one past its
 * last token. Query q sees key j iff doc_start[q] <= j <= q. The forward and the dQ kernel test that
 * rule; the dK / dV kernel, which owns keys, tests q < doc_end[j], the same set when the two arrays
 * describe one partition of the row into documents.
 *
 * The kernels are memory-safe for any array contents: doc_start[i] is read clamped to [0, i] and
 * doc_end[i] clamped to [i + 1, S], and the values only skip K/V tiles or query slices of the plain
 * causal sweep and mask scores inside it. Inconsistent arrays give an unspecified result, never an
 * access outside the tensors. Every row sees at least itself, so this path has no lse = +inf case.
 *
 * There is no key mask here: padding in a packed row is a trailing document of its own (whose labels
 * the loss ignores). p, seed: as in smt_attn_*_dropout (the keep function does not depend on the
 * documents; t == 0 is no dropout and seed may then be NULL). Both arrays NULL: the calls forward to
 * smt_attn_fwd_dropout / smt_attn_bwd_dropout without a key mask. Exactly one array NULL returns -1
 * before any HIP call.
 */
int smt_attn_fwd_docs(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                      const smt_attn_tensor* o, float* lse, const int32_t* doc_start, const int32_t* doc_end,
                      float p, const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream);
int smt_attn_bwd_docs(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                      const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                      const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                      const int32_t* doc_start, const int32_t* doc_end, float p, const uint64_t* seed,
                      const smt_attn_shape* shape, hipStream_t stream);

/*
 * Any sequence length (additive entry points; the ABI version is unchanged): the general form of the
 * chain above, with a row stride of their own for lse and delta. lse and delta_ws are fp32
 * [B][Hq][lse_ld] with lse_ld >= S, lse_ld % 4 == 0 and 16-byte aligned base pointers; S >= 1 is
 * otherwise free (the dK / dV kernel fetches lse and delta in 16-byte groups, so it is their rows that
 * need the alignment, not S). The forward writes entries [0, S) of each row and does not touch
 * [S, lse_ld). The backward's results do not depend on what [S, lse_ld) holds in lse or in delta_ws:
 * any bit pattern, NaN and Inf included (those entries are never fetched: the buffer descriptor of the
 * dK / dV kernel's 16-byte fetch ends at entry S of the row, its range check is per dword, and the
 * entries past S land as zeros). key_mask, doc_start / doc_end, p and seed mean what they mean above: key_mask NULL = no key
 * mask, both doc arrays NULL = no documents, t == 0 = no dropout (seed may then be NULL); the keep
 * function does not depend on S or lse_ld. Every entry point above is this one with lse_ld = S (so
 * smt_attn_bwd* still returns -2 for S % 4 != 0).
 *
 * Returns -1 before any HIP call for lse_ld < S, lse_ld % 4 != 0, exactly one doc array NULL, a key
 * mask together with documents, p outside [0, 1), a NULL seed with t > 0, and the null or malformed
 * arguments the entry points above refuse; -2 for misaligned lse / delta_ws pointers (backward).
 */
int smt_attn_fwd_ld(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                    const smt_attn_tensor* o, float* lse, int64_t lse_ld, const uint64_t* key_mask, int64_t key_mask_ld,
                    const int32_t* doc_start, const int32_t* doc_end, float p, const uint64_t* seed,
                    const smt_attn_shape* shape, hipStream_t stream);
int smt_attn_bwd_ld(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                    const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                    int64_t lse_ld, const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                    const uint64_t* key_mask, int64_t key_mask_ld, const int32_t* doc_start, const int32_t* doc_end,
                    float p, const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream);

/*
 * Cached (KV-cache) forward for inference (additive entry points; the ABI version is unchanged; no
 * backward). Sq query positions against Skv = shape->S key slots:
 *   q, o     element (b, h, i, d), h < Hq, i < Sq; k, v element (b, h, j, d), h < Hkv, j < Skv, any
 *            element strides (a slice of a larger cache buffer, a [B, S, H, D]-ordered cache)
 *   lse      fp32 [B][Hq][Sq] in the log2 units above, or NULL
 *   key_mask over the Skv keys, key_mask_ld >= ceil(Skv / 64), or NULL
 * Query i sits at absolute position q_offset + i and sees key j iff j <= q_offset + i, j < Skv and key
 * j's mask bit is set. Skv is arbitrary (no % 4, no % 64); q_offset + Sq <= Skv, and Skv may be larger
 * (a pre-allocated cache): K / V rows at j >= q_offset + Sq are never read, whatever they hold. Rows a
 * column does not see leave by selection, so an Inf or NaN in a key-masked row does not reach o. A
 * query whose visible keys are all masked gets o = 0 and lse = +inf, as in smt_attn_fwd_kmask.
 *
 * The kernel packs the (query position, query head of one KV head) pairs into the 32 columns of its
 * matrix products, so the G = Hq / Hkv heads of a group share ONE read of that head's K / V; Sq * G >
 * 32 takes further column blocks (correct for any Sq, fast for Sq * G <= 32). The keys [0, q_offset +
 * Sq) are cut into num_splits contiguous ranges of 64-key tiles, one workgroup each per (column block,
 * b, kv head); with num_splits > 1 each writes fp32 partials (unnormalised O, running max, running
 * sum) to `workspace` and a second kernel combines them in split order: no atomics, and for a given
 * num_splits the result is bit-reproducible. A split without a visible key contributes nothing.
 * num_splits == 1 writes o directly and needs no workspace. num_splits == 0 takes
 * smt_attn_cached_splits(shape, Sq), a pure host function of (B, Hkv, G, Sq, Skv): >= 1, at most the
 * number of 64-key tiles of Skv, 1 for Skv <= 64. smt_attn_cached_workspace: the bytes of `workspace`
 * (16-byte aligned device memory) for num_splits (0 = the default count); 0 when none is needed.
 * Both return -1 for a bad shape, Sq < 1 or num_splits < 0.
 *
 * Returns -1 before any HIP call for a null shape / tensor, Sq < 1, q_offset < 0, q_offset + Sq > Skv
 * (a query with no key slot of its own), num_splits < 0, a null workspace when one is needed, a dtype
 * that is not a 16-bit format, Hq % Hkv != 0.
 */
int     smt_attn_cached_splits(const smt_attn_shape* shape /* S = Skv */, int32_t Sq);
int64_t smt_attn_cached_workspace(const smt_attn_shape* shape, int32_t Sq, int32_t num_splits);
int     smt_attn_fwd_cached(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                            const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                            int32_t Sq, int32_t q_offset, int32_t num_splits, void* workspace,
                            const smt_attn_shape* shape, hipStream_t stream);

/*
 * The same call with the position on the device (additive; the ABI version is unchanged): for a
 * pre-allocated ("static") cache whose fill level the host does not know, and for capturing the call
 * in a HIP graph: no launch parameter depends on the position.
 *   positions         int64 device memory, 8-byte aligned; row b's first query sits at
 *                     p = positions[b * positions_stride], read by the kernel (never by the host)
 *   positions_stride  0: one position for the whole batch; 1: one per batch row
 *   shape->S = Skv    the CAPACITY of the K / V buffers; key_mask covers the capacity
 * Query i of row b sees key j iff j <= p + i and key j's mask bit is set; the keys any query of the row
 * sees are [0, p + Sq), and K / V rows at p + Sq and later are never read, whatever they hold. The
 * kernel derives from p what smt_attn_fwd_cached derives from q_offset on the host, the tile partition
 * included (tiles = ceil((p + Sq) / 64), ceil(tiles / num_splits) per split, per batch row): for a
 * given num_splits the result is bit-identical to smt_attn_fwd_cached with q_offset = p on the same
 * tensors. The grid, num_splits == 0 (smt_attn_cached_splits) and the workspace
 * (smt_attn_cached_workspace) are sized from the capacity; a split that ends up without tiles
 * contributes nothing, so a cache far from full runs more, emptier splits than the host-offset call.
 *
 * A position the host would have refused cannot be refused here: the kernel SATURATES p into
 * [0, Skv - Sq] before it forms any address, and computes the result of that position. No read or
 * write outside the tensors depends on the values in `positions`.
 *
 * Returns before any HIP call: -1 for what smt_attn_fwd_cached refuses (q_offset apart), null
 * positions, positions_stride other than 0 or 1, Sq > Skv; -2 for positions that are not 8-byte aligned
 * and when Skv rows of K or V span 2 GiB or more.
 */
int     smt_attn_fwd_cached_pos(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                                const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                                int32_t Sq, const int64_t* positions, int32_t positions_stride, int32_t num_splits,
                                void* workspace, const smt_attn_shape* shape, hipStream_t stream);

/*
 * Beam-shared cache (additive entry points; the ABI version is unchanged; forward only): one decode
 * position of beam search against a cache that is never reordered and never concatenated. shape->B = N
 * samples (shape->S is not used), nb beams each; row r = n * nb + beam.
 *   q, o               [N * nb][Hq][1][128]: smt_attn_tensor with sb the row stride (ss is not used)
 *   lse                fp32 [N * nb][Hq] in the log2 units above, or NULL
 *   k_prompt, v_prompt [N][Hkv][P_cap][128]: the prompt's keys, ONE copy per sample (the beams of a
 *                      sample hold identical prompt rows); P <= P_cap of them are valid. With P == 0
 *                      the two tensors are never touched and their ptr may be null.
 *   prompt_mask        uint64 [N][prompt_mask_ld] over the prompt keys (bit as in smt_attn_fwd_kmask),
 *                      prompt_mask_ld >= ceil(P / 64), or NULL; bits at j >= P are ignored
 *   k_gen, v_gen       [N * nb][Hkv][T_cap][128]: physical slot s of sample n is row n * nb + s, and
 *                      the key a slot wrote at step j is its row j; T <= T_cap steps are valid
 *   anc                uint8 [N * nb][anc_ld], anc_ld >= T: anc[r][j] is the physical slot (0..nb-1)
 *                      that holds the step-j key of row r's hypothesis
 * Row r of sample n sees prompt key j < P iff its mask bit is set, and generated entry (slot s, step
 * j < T) iff anc[r][j] == s; the result is the softmax over that set: smt_attn_fwd_cached with Sq = 1
 * on the row's gathered cache, up to the order of summation. Generated entries have no mask of their
 * own. A row with no visible key gets o = 0 and lse = +inf.
 *
 * The 32 columns of the kernel's products are (beam, query head of one KV head) pairs of one (sample,
 * KV head), col = beam * G + g; nb * G > 32 takes further column blocks (correct for any nb, fast for
 * nb * G <= 32). The tile list of a (sample, KV head) is the prompt's 64-key tiles, then every slot's
 * generated tiles: each physical K / V row is fetched once per sample, not once per beam, and nothing
 * is gathered. Rows at j >= P of the prompt buffers and j >= T of the generated buffers are never
 * read, whatever they hold; a row that no column of a block sees (a dead hypothesis, a masked key)
 * does not reach o, whatever it holds, an Inf or NaN included. num_splits, workspace: as in
 * smt_attn_fwd_cached, over contiguous ranges of that tile list (fp32 partials, combined in split
 * order, no atomics, bit-reproducible for a given num_splits; 1 writes o directly; 0 takes
 * smt_attn_beams_splits(shape, nb, P, T), a pure host function, >= 1). smt_attn_beams_workspace: the
 * bytes of `workspace` (16-byte aligned device memory) for num_splits (0 = the default); 0 when none
 * is needed. Both return -1 for a bad shape, nb < 1, P < 0, T < 1 or num_splits < 0.
 *
 * The kernel is memory-safe for any contents of anc: a value only ever enters the comparison
 * anc[r][j] == s against the slot counter s of the tile being swept (it masks a score or zeroes a V
 * row in LDS); no address depends on it, and a value >= nb matches no slot (that key is then invisible to row r). The bytes read are rows
 * [n * nb, n * nb + nb) x [0, T) of anc, nothing else.
 *
 * Returns -1 before any HIP call for a null shape / tensor / anc, nb < 1, P < 0, T < 1 (the current
 * token's key is already in the cache), P > P_cap, T > T_cap, anc_ld < T, prompt_mask_ld <
 * ceil(P / 64), Hq % Hkv != 0, a dtype that is not a 16-bit format, num_splits < 0 and a null
 * workspace when one is needed; -2 for misaligned rows, and when the P rows (T rows) of one head of
 * the prompt (generated) buffers, rounded up to whole tiles, span 2 GiB or more.
 */
int     smt_attn_beams_splits(const smt_attn_shape* shape /* B = N */, int32_t nb, int32_t P, int32_t T);
int64_t smt_attn_beams_workspace(const smt_attn_shape* shape, int32_t nb, int32_t P, int32_t T, int32_t num_splits);
int     smt_attn_fwd_beams(const smt_attn_tensor* q, const smt_attn_tensor* k_prompt, const smt_attn_tensor* v_prompt,
                           const smt_attn_tensor* k_gen, const smt_attn_tensor* v_gen, const smt_attn_tensor* o,
                           float* lse, const uint64_t* prompt_mask, int64_t prompt_mask_ld, const uint8_t* anc,
                           int64_t anc_ld, int32_t nb, int32_t P, int32_t P_cap, int32_t T, int32_t T_cap,
                           int32_t num_splits, void* workspace, const smt_attn_shape* shape, hipStream_t stream);

/*
 * The same call with the number of generated positions on the device (additive; the ABI version is
 * unchanged): for capturing a beam-search decode step in a HIP graph: no launch parameter depends on
 * the step.
 *   steps   int32 device memory, 4-byte aligned, ONE counter for the whole call: the number of
 *           generated positions, the current token's included; read by the kernel (never by the host)
 *   anc_ld  >= T_cap
 * The kernel SATURATES T = clamp(*steps, 1, T_cap) before it forms any address, and derives from T what
 * smt_attn_fwd_beams derives from its T on the host: ceil(T / 64) tiles per slot, the tile list (the
 * prompt's tiles, then every slot's), ceil(tiles / num_splits) tiles per split, the buffer descriptors
 * that end at row T - 1 and the j < T test on the ancestry bytes. For a given num_splits the result is
 * BIT-IDENTICAL to smt_attn_fwd_beams with T = clamp(*steps, 1, T_cap) on the same tensors. The grid,
 * num_splits == 0 (smt_attn_beams_splits(shape, nb, P, T_cap)) and the workspace
 * (smt_attn_beams_workspace(shape, nb, P, T_cap, num_splits)) are sized from the capacity; a split that
 * ends up without tiles writes the empty partial, so a cache far from full runs more, emptier splits
 * than the host-T call. No read or write outside the tensors depends on *steps or on a value in anc.
 *
 * Returns before any HIP call: -1 for what smt_attn_fwd_beams refuses with T read as T_cap, for null
 * steps and for anc_ld < T_cap; -2 for steps that are not 4-byte aligned, and for the 2 GiB extents
 * taken at T_cap.
 */
int     smt_attn_fwd_beams_pos(const smt_attn_tensor* q, const smt_attn_tensor* k_prompt, const smt_attn_tensor* v_prompt,
                               const smt_attn_tensor* k_gen, const smt_attn_tensor* v_gen, const smt_attn_tensor* o,
                               float* lse, const uint64_t* prompt_mask, int64_t prompt_mask_ld, const uint8_t* anc,
                               int64_t anc_ld, int32_t nb, int32_t P, int32_t P_cap, const int32_t* steps, int32_t T_cap,
                               int32_t num_splits, void* workspace, const smt_attn_shape* shape, hipStream_t stream);

/*
 * One step's K and V into the generated buffers, with the same counter and the same saturation: k_new,
 * v_new [rows][Hkv][1][128] (any sb / sh, d-stride 1, 16-byte aligned rows; ss is not used) are written
 * to row clamp(*steps, 1, T_cap) - 1 of k_gen, v_gen [rows][Hkv][T_cap][128], both in one launch, with
 * 16-byte stores; no other row is touched, and the row cannot leave the buffers whatever *steps holds.
 * dtype: SMT_DTYPE_BF16 or SMT_DTYPE_FP16 (the elements are copied as 16-bit words).
 * Returns before any HIP call: -1 for a null tensor or steps, a dtype that is not a 16-bit format,
 * rows / Hkv / T_cap < 1; -2 for misaligned rows and for steps that are not 4-byte aligned.
 */
int     smt_attn_kv_append_pos(const smt_attn_tensor* k_new, const smt_attn_tensor* v_new, const smt_attn_tensor* k_gen,
                               const smt_attn_tensor* v_gen, const int32_t* steps, int32_t rows, int32_t Hkv,
                               int32_t T_cap, int32_t dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMT_ATTENTION_H */
