// Causal grouped-query flash attention for gfx950 (CDNA4), head_dim 128, bf16 or fp16 I/O (the model's
// dtype, smt_attn_shape.dtype; ABI v13), fp32 softmax, optional attention dropout inside the three
// kernels (DROP instances, smt_attn_*_dropout), optional document mask of packed rows (DOC instances,
// smt_attn_*_docs); and the forward-only split-KV kernel of calls against a KV cache (attn_decode_kernel,
// smt_attn_fwd_cached; smt_attn_fwd_cached_pos with the query position read on the device, for a
// pre-allocated cache; attn_beams_kernel, smt_attn_fwd_beams, one decode position of beam search against
// a beam-shared cache that is never reordered; smt_attn_fwd_beams_pos with the number of generated
// positions read on the device and smt_attn_kv_append_pos, which writes a step's K / V at that
// position, for a decode step that is captured in a graph). Any sequence length S >= 1, forward and backward: lse and delta are
// [B][Hq][lse_ld] with a row stride lse_ld % 4 == 0 of their own (smt_attn_fwd_ld / smt_attn_bwd_ld),
// which is all the 16-byte lse / delta fetch of the dK/dV kernel needs; the other entry points are
// these with lse_ld = S.
// C ABI: include/smt_attention.h. Replaces transformers' sdpa attention (aotriton on this torch
// build) in the LLaMA decoder that carries the SMT modules.
//
// MFMA v_mfma_f32_32x32x16_bf16 lane maps (verified on gfx950):
//   A[m][k]: lane l holds m = l&31, k = 8*(l>>5) + j (j = 0..7)     B[k][n]: n = l&31, same k
//   C[m][n]: lane l holds n = l&31, m = (i&3) + 8*(i>>2) + 4*(l>>5) (i = 0..15)
// All products are arranged so that a softmax row lives on ONE lane pair (l, l^32):
//   forward   S^T[key][q] = K Q^T,  O^T[d][q] += V^T P^T          (q on the lane)
//   dQ        S^T, dP^T = V dO^T,   dQ^T[d][q] += K^T dS^T          (q on the lane)
//   dK, dV    S[q][key] = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS   (key on the lane)
// so row statistics are per-lane scalars and the probability tile, packed to bf16 and exchanged
// once between the two wave halves (v_permlane32_swap), IS the next product's B operand.
// LDS images are [row][128 d] bf16 rows of 256 B, swizzled by 16-B chunk:
//   chunk' = chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))
// which is conflict-free both for ds_read_b128 row reads (16 consecutive rows, same chunk) and for
// ds_read_b64_tr_b16 transposed reads (4 consecutive rows land in 4 different 64-B quarters).
//
// Shared code is kept only where scripts/diag/isa_compare.py shows every kernel's instructions unchanged
// (DESIGN §4a). Found to change code, so written out where they stand: a helper for the C-layout key
// index of the mask loops; a shared workgroup -> (b, h, hk, q block) mapping of the forward / dQ
// kernels; frag_or_zero in dQ and the decode kernel; store_row for dK / dV (as two row stores or per
// 8-byte group) and for the decode output; the dQ first issue without its `nt > 0` test.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "smt_attention.h"
#include "smt_hip.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "%s: %s", what, hipGetErrorString(e));
    return 0;
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;

constexpr int kD = 128;
constexpr int kRowB = 256;                 // one [d] row in LDS
constexpr float kNegInf = -__builtin_huge_valf();

struct Tns {
    const uint16_t* p;
    int64_t sb, sh, ss;
};

__device__ __forceinline__ uint32_t swz(uint32_t row) { return ((row & 3u) << 2) | ((row >> 2) & 3u); }
__device__ __forceinline__ uint32_t lds_off(uint32_t row, uint32_t byte) { return row * kRowB + (byte ^ (swz(row) << 4)); }

// 8 consecutive d of one row (ds_read_b128): A[m=row][k] or B[k][n=row] fragments of row-major data.
__device__ __forceinline__ bf16x8_t row_frag(const uint8_t* img, uint32_t row, uint32_t byte) {
    return *reinterpret_cast<const bf16x8_t*>(img + lds_off(row, byte));
}

// Transposed fragment (two ds_read_b64_tr_b16): lane l gets column (col0 + l&31) at rows
// row0 + 8*(l>>5) + 0..7, i.e. the A[m=col][k=row] operand of row-major data.
struct TrLane {
    uint32_t krow, feat_byte;
};
__device__ __forceinline__ TrLane tr_lane(int lane) {
    const int gi = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    return TrLane{8u * (gi >> 1) + q, 2u * (16u * (gi & 1) + 4u * p)};
}
__device__ __forceinline__ bf16x8_t tr_frag(const uint8_t* img, TrLane tl, uint32_t row0, uint32_t col0) {
    const uint32_t r = row0 + tl.krow, byte = 2u * col0 + tl.feat_byte;
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(img + lds_off(r, byte)));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(img + lds_off(r + 4, byte)));
    const s16x8_t both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, both);
}

// Fragments travel as bf16x8_t bit containers whatever the format; F = SMT_DTYPE_BF16 (0) or
// SMT_DTYPE_FP16 (2) picks the MFMA (v_mfma_f32_32x32x16_bf16 / _f16, the same lane maps) and the
// roundings of P, dS and the outputs.
template <int F>
__device__ __forceinline__ f32x16_t mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    if constexpr (F == SMT_DTYPE_FP16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c,
                                                      0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Two-lane fp32 arithmetic of the softmax. PK: packed (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32,
// one issue per pair); otherwise two scalar VALU ops per pair (the packed forms cost more than two
// scalar ones when issued beside MFMAs, MI355X_MICROARCH issue-cost table). Results are bit-identical
// either way (the same IEEE operations). The forward measured faster scalar, dQ and dK/dV packed
// (profiles/r04_e_attn_pk_ab.jsonl).
constexpr bool kPkFwd = false, kPkDq = true, kPkDkv = true;
template <bool PK>
__device__ __forceinline__ f32x2_t fma2(f32x2_t a, f32x2_t b, f32x2_t c) {
    if (PK) return __builtin_elementwise_fma(a, b, c);
    return f32x2_t{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)};
}
template <bool PK>
__device__ __forceinline__ f32x2_t submul2(f32x2_t a, f32x2_t d, f32x2_t p) {     // (a - d) * p
    if (PK) return (a - d) * p;
    return f32x2_t{(a.x - d.x) * p.x, (a.y - d.y) * p.y};
}
template <bool PK>
__device__ __forceinline__ f32x2_t add2(f32x2_t a, f32x2_t b) {
    if (PK) return a + b;
    return f32x2_t{a.x + b.x, a.y + b.y};
}

template <int F>
__device__ __forceinline__ uint32_t pk16(float a, float b) {        // two fp32 -> two 16-bit values (RNE)
    f32x2_t v = {a, b};
    if constexpr (F == SMT_DTYPE_FP16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
template <int F>
__device__ __forceinline__ float lo16(uint32_t w) {                  // the low / high 16-bit value of a word
    if constexpr (F == SMT_DTYPE_FP16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
    else return __uint_as_float(w << 16);
}
template <int F>
__device__ __forceinline__ float hi16(uint32_t w) {
    if constexpr (F == SMT_DTYPE_FP16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    else return __uint_as_float(w & 0xffff0000u);
}

__device__ __forceinline__ float other_half_max(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float halves_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// C-layout probabilities of one 32-column tile (16 fp32 per lane: column = lane's n, rows
// (i&3)+8(i>>2)+4hi) -> two B fragments for k-steps of 16 rows, rows 8hi..8hi+7 per lane.
template <int F>
__device__ __forceinline__ void pack_b_frags(const float (&p)[16], bf16x8_t& f0, bf16x8_t& f1) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = pk16<F>(p[2 * i], p[2 * i + 1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        auto a = __builtin_amdgcn_permlane32_swap(w[4 * h + 0], w[4 * h + 2], false, false);
        auto b = __builtin_amdgcn_permlane32_swap(w[4 * h + 1], w[4 * h + 3], false, false);
        u32x4_t v = {a[0], b[0], a[1], b[1]};
        if (h == 0) f0 = __builtin_bit_cast(bf16x8_t, v);
        else f1 = __builtin_bit_cast(bf16x8_t, v);
    }
}

// 8 consecutive d of one global row as a fragment; zeros for a row outside the tensor (never read).
__device__ __forceinline__ bf16x8_t frag_or_zero(bool valid, const uint16_t* p) {
    if (valid) return *reinterpret_cast<const bf16x8_t*>(p);
    return __builtin_bit_cast(bf16x8_t, u32x4_t{0u, 0u, 0u, 0u});
}

// One row of a C-layout accumulator (4 tiles of 32 d; the lane holds d = 32 dt + 8 g + 4 hi + 0..3),
// scaled and rounded to the 16-bit format, as 8-byte stores.
template <int F>
__device__ __forceinline__ void store_row(uint16_t* row, const f32x16_t (&acc)[4], float s, int hi) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 w;
            w.x = pk16<F>(acc[dt][4 * g] * s, acc[dt][4 * g + 1] * s);
            w.y = pk16<F>(acc[dt][4 * g + 2] * s, acc[dt][4 * g + 3] * s);
            const int d = 32 * dt + 8 * g + 4 * hi;
            *reinterpret_cast<uint2*>(row + d) = w;
        }
}

// The lane constants of the explicit LDS reads (rowx / trx): row l32's 16-B chunk hi, and the
// transposed reads' rows krow and krow + 4.
__device__ __forceinline__ void lane_lds(int lane, int l32, int hi, uint32_t& lo_row, uint32_t& lo_t0, uint32_t& lo_t4) {
    const uint32_t r = (uint32_t)l32;
    lo_row = r * kRowB + ((16u * hi) ^ (swz(r) << 4));
    const TrLane tl = tr_lane(lane);
    lo_t0 = tl.krow * kRowB + (tl.feat_byte ^ (swz(tl.krow) << 4));
    lo_t4 = (tl.krow + 4) * kRowB + (tl.feat_byte ^ (swz(tl.krow + 4) << 4));
}

// XCD-aware bijective remap (workgroups are dealt round-robin over the 8 XCDs): consecutive logical
// ids run on one XCD, so workgroups that share K/V (or Q/dO) share that XCD's L2.
__device__ __forceinline__ int xcd_logical(int bid, int total) {
    const int q8 = total >> 3, r8 = total & 7, xcd = bid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Explicit LDS addressing for compile-time image offsets. A swizzled row read (lds_off) of row r,
// 16-B chunk (ks, hi) is (r*256 + (16hi ^ swz(r)<<4)) ^ (ks<<5), and a transposed read at rows
// 16kq + krow (+4) and column block dt is 4096kq + ((r*256 + (feat_byte ^ swz<<4)) ^ (dt<<6)): one
// lane constant per read family, one v_xor per read, the image base in the instruction's offset.
// The lane constants are re-materialised per slice (an opaque copy), so hipcc cannot hoist the 8-16
// derived addresses out of the loop and spill them.
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <int IMG>
__device__ __forceinline__ bf16x8_t rowx(const uint8_t* lds, uint32_t lo, int ks) {
    return *reinterpret_cast<const bf16x8_t*>(lds + IMG + (lo ^ (uint32_t)(ks << 5)));
}
template <int IMG>
__device__ __forceinline__ bf16x8_t trx(const uint8_t* lds, uint32_t t0, uint32_t t4, int kq, int dt) {
    const uint32_t x = (uint32_t)(dt << 6);
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(lds + IMG + 4096 * kq + (t0 ^ x)));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(lds + IMG + 4096 * kq + (t4 ^ x)));
    const s16x8_t both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, both);
}

// LDS-DMA: lane l's 16 B from rsrc + voff land at LDS byte lds_base + 16*l (buffer_load ... lds).
// Inline asm so that hipcc does not treat it as an LDS write aliasing every ds_read (it then drains
// vmcnt before each read); completion is waited for explicitly (s_waitcnt vmcnt(0) + barrier).
// M0 is saved / restored inside the statement. Out-of-range offsets read as zeros.
typedef __attribute__((address_space(3))) uint8_t lds_u8_t;
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, uint32_t lds_base, int voff) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_base) : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const uint8_t* p) { return (uint32_t)(uintptr_t)(const lds_u8_t*)p; }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, int64_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const int n = __builtin_amdgcn_readfirstlane((int)bytes);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}
__device__ __forceinline__ void vm_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// The same wait as a builtin the compiler's waitcnt pass understands: after it, the pass knows that
// the register loads issued before the loop (Q / dO / K fragments) have landed. Without it the pass
// still counts them as pending at the loop header and puts a vmcnt(0) in front of their first use
// INSIDE the loop, which also waits for the next tile's LDS-DMA issued just before it (the prefetch
// then never overlaps compute). gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15.
__device__ __forceinline__ void vm_wait_all_known() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// Wait until at most n (wave-uniform) of this wave's vector-memory operations are outstanding,
// rounded down to an encodable immediate (waiting for more than needed is always safe).
__device__ __forceinline__ void vm_wait_upto(int n) {
    if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One wave copies `pieces` x 4 rows [row0, row0 + 4*pieces) of a [rows][128] bf16 operand (row stride
// ss elements, rows counted from the rsrc base) into a swizzled LDS image at img (image row = row - img_row0).
__device__ __forceinline__ void dma_rows(__amdgpu_buffer_rsrc_t rsrc, int64_t ss, uint32_t img, int img_row0,
                                         int row0, int pieces, int lane) {
#pragma unroll 4
    for (int i = 0; i < pieces; ++i) {
        const int r = row0 + 4 * i + (lane >> 4);             // source row of this lane
        const uint32_t ir = (uint32_t)(r - img_row0);          // image row
        const uint32_t ch = (uint32_t)(lane & 15) ^ swz(ir);   // logical chunk stored at this lane's slot
        const uint32_t base = __builtin_amdgcn_readfirstlane(img + (uint32_t)(r - (lane >> 4) - img_row0) * kRowB);
        dma16(rsrc, base, (int)((int64_t)r * ss * 2 + ch * 16));
    }
}

// ------------------------------------------------------------------------------------------------
// Forward: a workgroup = 4 waves x 32 query rows of one (b, q head); K/V tiles of 64 keys staged
// through registers into a double-buffered LDS ring (issue-early / write-late), one barrier per tile.
// ------------------------------------------------------------------------------------------------
// Waves (x 32 query rows) per workgroup of the forward / dQ kernels: 4, two workgroups per CU. Every
// workgroup stages its own K/V tiles, so 8 waves (256 query rows, one workgroup per CU) would halve
// the LDS-fill bytes per MFMA; measured at B16 Hq32 Hkv8 S2048 (profiles/r02_attn_waves.jsonl) the
// 8-wave forward ran 7 % slower (0.89 vs 0.83 ms) and the 8-wave dQ the same: these loops are not
// bound by the K/V fill. The forward reads its K / V fragments two MFMAs ahead (FwdLean::compute:
// 0.80 -> 0.76 ms at the bench shape, profiles/r04_f_attn_pref_ab.jsonl); the same read-ahead in dQ
// measured no faster and is not used.
constexpr int kFwdQW = 32, kFwdWaves = 4, kFwdQB = kFwdQW * kFwdWaves, kKV = 64;
constexpr int kDqWaves = 4, kDqQB = kFwdQW * kDqWaves;
constexpr int kTileB = kKV * kRowB;        // 16 KiB per operand tile

// Key mask (optional, smt_attn_*_kmask): bit (j & 63) of kmask[b * kmask_ld + (j >> 6)] set = key j
// of batch b takes part (transformers' 2-D attention_mask of a padded batch, e.g. the reference's
// collator mask input_ids != pad, deepspeed/helpers/helper.py:194-204). A query row whose every
// visible key is masked gets a zero output, lse = +inf and zero gradients (torch's safe softmax).
__device__ __forceinline__ bool key_bit(uint64_t w, int key) { return (w >> (key & 63)) & 1ull; }

// Document mask (optional, DOC instances, smt_attn_*_docs): several samples packed into one row, query
// q sees key j iff doc_start[q] <= j <= q. The forward and dQ lanes hold one q, so they test
// key < doc_start[q]; a dK/dV lane holds one key and tests q >= doc_end[key], the same set for
// consistent arrays. Every value is clamped where it is read (doc_start[i] to [0, i], doc_end[i] to
// [i + 1, S]) and only ever gates compute or selects a tile inside the sweep of the plain kernels, so no
// array content can move an access outside the tensors.
constexpr int kIntMax = 0x7fffffff;
__device__ __forceinline__ int doc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int wave_min(int v) {           // wave-uniform (an SGPR)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
// The smallest clamped doc_start of rows [q0, q0 + rows) of one batch row, from every wave alike
// (workgroup-uniform without a barrier): the K/V sweep of a forward / dQ workgroup starts at its tile.
__device__ __forceinline__ int doc_block_min(const int32_t* ds, int q0, int rows, int S, int lane) {
    int g = kIntMax;
    for (int r = q0 + lane; r < min(q0 + rows, S); r += 64) g = min(g, doc_clamp(ds[r], 0, r));
    return wave_min(g);
}

// Attention dropout (DROP instances, smt_attn_*_dropout; the keep function is documented in
// include/smt_attention.h and is part of the contract). One 32-bit word decides 4 consecutive keys of
// one query row, one byte each: keep = byte >= t. The forward and dQ lanes hold one q and runs of 4
// consecutive keys (one drop_word per 4 elements, row_key once per lane); a dK/dV lane holds one key
// and 16 rows per slice (DkvLean: the slice's 32 row keys once per workgroup, each word once per
// 4-lane group). The export kernel and the three attention kernels call these same functions.
struct DropArgs {
    const uint64_t* seed;                  // one value in device memory
    uint32_t t;                            // threshold, 1..255
    float r;                               // 1 / (1 - t/256)
};
__device__ __forceinline__ uint32_t drop_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x21F0AAADu; x ^= x >> 15; x *= 0x735A2D97u; x ^= x >> 15;
    return x;
}
__device__ __forceinline__ uint32_t drop_head_key(uint64_t seed, uint32_t bh) {       // bh = b*Hq + h
    return drop_mix((uint32_t)seed + bh * 0x9E3779B9u) ^ (uint32_t)(seed >> 32);
}
__device__ __forceinline__ uint32_t drop_row_key(uint32_t head_key, uint32_t q) {
    return drop_mix(head_key + q * 0x85EBCA6Bu);
}
constexpr uint32_t kDropKeyMul = 0x9E3779B1u;
// key_term = (key >> 2) * kDropKeyMul (callers with compile-time key offsets add their multiples)
__device__ __forceinline__ uint32_t drop_word(uint32_t row_key, uint32_t key_term) { return drop_mix(row_key ^ key_term); }
__device__ __forceinline__ bool drop_keep(uint32_t word, uint32_t key_lo2, uint32_t t) {
    return ((word >> (8u * key_lo2)) & 0xFFu) >= t;
}

struct FwdArgs {
    Tns q, k, v;
    uint16_t* o;
    int64_t o_sb, o_sh, o_ss;
    float* lse;
    int lse_ld;                            // row stride of lse: >= S, % 4 == 0
    const uint64_t* kmask;
    int64_t kmask_ld;
    int B, Hq, Hkv, S;
    float sl2;                             // scale * log2(e)
    DropArgs drop;                         // read by the DROP instances only
    const int32_t* doc_start;              // [B][S], read by the DOC instances only
};

// Causal balance: a workgroup takes the query blocks qb and nqb-1-qb (equal total work per workgroup).
struct PairTask {
    int b, hk, hh, blk[2], n;
};
__device__ __forceinline__ PairTask pair_task(int L, int nblk, int G, int Hkv) {
    const int npair = (nblk + 1) / 2;
    const int per_group = G * npair;
    const int grp = L / per_group;
    const int rem = L - grp * per_group;
    const int p = rem / G;
    PairTask t;
    t.b = grp / Hkv;
    t.hk = grp % Hkv;
    t.hh = rem % G;
    t.blk[0] = nblk - 1 - p;
    t.blk[1] = p;
    t.n = (t.blk[1] == t.blk[0]) ? 1 : 2;
    return t;
}

constexpr float kFwdThr = 8.f;


// v_max3_f32 as one instruction: fmaxf on MFMA results makes hipcc canonicalise both inputs first
// (an extra v_max per operand; cdna_hip_programming Appendix B, attention pitfalls)
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// ------------------------------------------------------------------------------------------------
// Forward (FwdLean): two workgroups per CU, i.e. two waves per SIMD whose MFMA and VALU phases
// overlap each other; Q in registers; a 2-slot K/V ring, one barrier per 64-key tile; the per-tile
// VALU cut to what the softmax needs: tiles in pairs so the LDS slot is a compile-time offset (no
// per-read address adds), the scores' first MFMA on a zero accumulator (no per-tile zeroing), the row
// max by v_max3 without canonicalisation, row max / sum as trees, a deferred running max (a row's max
// moves only when a tile's max exceeds it by more than kFwdThr, log2 units, so P <= 2^kFwdThr and the
// O rescale is rare; cdna_hip_programming T13) and the causal mask only on the wave's diagonal tile.
// Measured and removed (git history): a software-pipelined one-workgroup-per-CU forward,
// one wave per SIMD over 64 rows (two builds), all slower.
// ------------------------------------------------------------------------------------------------

// DOC: the sweep starts at the tile of the workgroup's smallest doc_start (an odd first tile runs once
// through tile<1>, so the ring slot stays a compile-time parity); a wave skips the compute, never the
// DMA, wait or barrier, of tiles wholly before its own rows' smallest doc_start, tests key <
// doc_start[q] on the tiles below its rows' largest doc_start, and runs the plain body on the rest.
// The sweep is written once: in the plain instances its first tile t0 is the constant 0 and folds away.
template <bool KMASK, int F, bool DROP, bool DOC = false>
struct FwdLean {
    const FwdArgs& a;
    uint8_t* lds;
    __amdgpu_buffer_rsrc_t rk, rv;
    uint32_t lds0;
    const uint64_t* km;
    bf16x8_t qf[8];
    f32x16_t o[4];
    float m_run, l_run;
    int qw, qrow, hi, l32, wave, lane, nt, last;
    uint32_t drop_rk;                      // DROP: the lane's row key
    int doc_ds, doc_wmax, doc_t0;          // DOC: the lane's doc_start, the wave's largest, the wave's first tile
    TrLane tl;

    __device__ __forceinline__ FwdLean(const FwdArgs& a_, uint8_t* lds_) : a(a_), lds(lds_) {}

    __device__ __forceinline__ void issue(int t) {            // K(t), V(t) into slot t & 1
        const uint32_t slot = lds0 + (uint32_t)((t & 1) * 2 * kTileB);
        dma_rows(rk, a.k.ss, slot, t * kKV, t * kKV + 16 * wave, 4, lane);
        dma_rows(rv, a.v.ss, slot + kTileB, t * kKV, t * kKV + 16 * wave, 4, lane);
    }

    template <int SLOT, bool DIAG_>
    __device__ __forceinline__ void compute(int t, bool DIAG) {
        const uint8_t* K = lds + SLOT * 2 * kTileB;
        const uint8_t* V = K + kTileB;
        const int k0 = t * kKV;
        f32x16_t sc[2];
        // K fragments read two k-steps ahead of their MFMAs (a 3-deep register ring, fenced so hipcc
        // keeps the order): without it each MFMA waited lgkmcnt(0) on a read issued one MFMA earlier
        bf16x8_t kf[3][2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) kf[p][j] = row_frag(K, 32 * j + l32, 32 * p + 16 * hi);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks + 2 < 8) {
#pragma unroll
                for (int j = 0; j < 2; ++j) kf[(ks + 2) % 3][j] = row_frag(K, 32 * j + l32, 32 * (ks + 2) + 16 * hi);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 2; ++j) sc[j] = mfma<F>(kf[ks % 3][j], qf[ks], ks ? sc[j] : f32x16_t{});
            __builtin_amdgcn_sched_barrier(0);
        }
        // the first two V fragments of the PV product, in flight during the softmax
        bf16x8_t vf[3];
        vf[0] = tr_frag(V, tl, 0, 0);
        vf[1] = tr_frag(V, tl, 16, 0);
        float x[32];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) x[16 * j + i] = sc[j][i];
        if (DIAG) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                if (key > qrow) x[i] = kNegInf;
            }
        }
        if (KMASK) {
            const uint64_t w = km[k0 >> 6];                    // workgroup-uniform
            if (~w != 0ull) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                    if (!key_bit(w, key)) x[i] = kNegInf;
                }
            }
        }
        if constexpr (DOC) {
            if (k0 < doc_wmax) {                               // a document of this wave starts past k0
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                    if (key < doc_ds) x[i] = kNegInf;
                }
            }
        }
        float mx[11];
#pragma unroll
        for (int i = 0; i < 10; ++i) mx[i] = max3f(x[3 * i], x[3 * i + 1], x[3 * i + 2]);
        mx[10] = max3f(x[30], x[31], mx[0]);
        mx[0] = max3f(mx[0], mx[1], mx[2]);
        mx[3] = max3f(mx[3], mx[4], mx[5]);
        mx[6] = max3f(mx[6], mx[7], mx[8]);
        mx[9] = max3f(mx[9], mx[10], mx[0]);
        const float m_tile = other_half_max(max3f(mx[3], mx[6], mx[9])) * a.sl2;
        const bool move = m_tile > m_run + kFwdThr;
        const float m_new = move ? m_tile : m_run;
        const float alpha = move ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.f;
        const float m_use = ((KMASK || DOC) && m_new == kNegInf) ? 0.f : m_new;
        // packed fp32 (v_pk_fma_f32 / v_pk_add_f32: two lanes' worth per VALU issue)
        const f32x2_t sl2v = {a.sl2, a.sl2}, mv = {-m_use, -m_use};
        f32x2_t sm[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const f32x2_t e = fma2<kPkFwd>(f32x2_t{x[2 * i], x[2 * i + 1]}, sl2v, mv);
            x[2 * i] = __builtin_amdgcn_exp2f(e.x);
            x[2 * i + 1] = __builtin_amdgcn_exp2f(e.y);
            sm[i] = f32x2_t{x[2 * i], x[2 * i + 1]};
        }
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
            for (int i = 0; i < w; ++i) sm[i] = add2<kPkFwd>(sm[i], sm[i + w]);
        l_run = l_run * alpha + (sm[0].x + sm[0].y);
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(move) != 0) {          // rare (deferred max)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
        }
        if constexpr (DROP) {
            // only the P tile of the PV product is dropped: the running max and sum above are those
            // of the undropped probabilities (r folds into the final 1 / l)
            const uint32_t kt0 = ((uint32_t)(k0 >> 2) + (uint32_t)hi) * kDropKeyMul;
#pragma unroll
            for (int w = 0; w < 8; ++w) {                      // keys k0 + 32 (w>>2) + 8 (w&3) + 4 hi + 0..3
                const uint32_t word = drop_word(drop_rk, kt0 + (uint32_t)(8 * (w >> 2) + 2 * (w & 3)) * kDropKeyMul);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (!drop_keep(word, c, a.drop.t)) x[4 * w + c] = 0.f;
            }
        }
        bf16x8_t pf[4];
        pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&x[0]), pf[0], pf[1]);
        pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&x[16]), pf[2], pf[3]);
        // V^T fragments two MFMAs ahead (n = 4 dt + kst)
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            if (n + 2 < 16) vf[(n + 2) % 3] = tr_frag(V, tl, 16 * ((n + 2) & 3), 32 * ((n + 2) >> 2));
            __builtin_amdgcn_sched_barrier(0);
            o[n >> 2] = mfma<F>(vf[n % 3], pf[n & 3], o[n >> 2]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // tile t (t & 1 == SLOT): fetch tile t+1 into the other slot, compute, wait, barrier
    template <int SLOT>
    __device__ __forceinline__ void tile(int t) {
        if (t + 1 < nt) issue(t + 1);
        if (t <= last && (!DOC || t >= doc_t0)) compute<SLOT, true>(t, t == last);
        vm_wait_all();
        __syncthreads();
    }

    __device__ __forceinline__ void run(int b, int h, int hk, int qb) {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        hi = lane >> 5;
        l32 = lane & 31;
        const int q0 = qb * kFwdQB;
        qw = q0 + wave * kFwdQW;
        qrow = qw + l32;
        const uint16_t* qp = a.q.p + b * a.q.sb + h * a.q.sh;
        const uint16_t* kp = a.k.p + b * a.k.sb + hk * a.k.sh;
        const uint16_t* vp = a.v.p + b * a.v.sb + hk * a.v.sh;
        km = KMASK ? a.kmask + (int64_t)b * a.kmask_ld : nullptr;
        if constexpr (DROP) drop_rk = drop_row_key(drop_head_key(*a.drop.seed, (uint32_t)(b * a.Hq + h)), (uint32_t)qrow);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            qf[ks] = frag_or_zero(qrow < a.S, qp + qrow * a.q.ss + 16 * ks + 8 * hi);
        }
        const int kv_end = min(a.S, q0 + kFwdQB);
        nt = (kv_end + kKV - 1) / kKV;
        last = min(nt - 1, qw / kKV);
        rk = uniform_rsrc(kp, (int64_t)a.S * a.k.ss * 2);
        rv = uniform_rsrc(vp, (int64_t)a.S * a.v.ss * 2);
        lds0 = lds_addr(lds);
        tl = tr_lane(lane);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
        m_run = kNegInf;
        l_run = 0.f;
        int t0 = 0;                                            // the first tile of the sweep
        if constexpr (DOC) {
            const int32_t* ds = a.doc_start + (int64_t)b * a.S;
            const bool qvalid = qrow < a.S;
            doc_ds = qvalid ? doc_clamp(ds[qrow], 0, qrow) : 0;
            doc_wmax = wave_max(doc_ds);
            doc_t0 = wave_min(qvalid ? doc_ds : kIntMax) / kKV;        // a wave without a valid row: no tile
            t0 = doc_block_min(ds, q0, kFwdQB, a.S, lane) / kKV;       // <= q0 / kKV < nt (row q0 is valid)
        }
        issue(t0);
        vm_wait_all();
        vm_wait_all_known();                                   // the Q fragments too (compiler-visible)
        __syncthreads();
        if (t0 & 1) {                                          // an odd first tile (DOC only): once through slot 1
            tile<1>(t0);
            ++t0;
        }
        for (int t = t0; t < nt; t += 2) {
            tile<0>(t);
            if (t + 1 < nt) tile<1>(t + 1);
        }
        const float l_tot = halves_sum(l_run);
        if (qrow < a.S) {
            float inv = (KMASK && !(l_tot > 0.f)) ? 0.f : 1.f / l_tot;
            if constexpr (DROP) inv *= a.drop.r;
            store_row<F>(a.o + b * a.o_sb + h * a.o_sh + (int64_t)qrow * a.o_ss, o, inv, hi);
            if (hi == 0)
                a.lse[((int64_t)b * a.Hq + h) * a.lse_ld + qrow] =
                    (KMASK && !(l_tot > 0.f)) ? __builtin_huge_valf() : m_run + __log2f(l_tot);
        }
    }
};

template <bool KMASK, int F, bool DROP, bool DOC = false>
__global__ __launch_bounds__(64 * kFwdWaves, 2)
void attn_fwd_kernel(FwdArgs a) {
    static_assert(!(KMASK && DOC), "no key mask beside documents");
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * kTileB];      // K/V ring: 2 x 32 KiB
    const int nqb = (a.S + kFwdQB - 1) / kFwdQB;
    const int G = a.Hq / a.Hkv;
    const int total = nqb * a.Hq * a.B;
    // consecutive ids: the G heads of one (b, kv head) at one q block, heaviest (longest causal row)
    // q blocks first (pairing q blocks measured 1-2 % slower here than this order)
    const int L = xcd_logical(blockIdx.x, total);
    const int per_group = G * nqb;
    const int grp = L / per_group;
    const int rem = L - grp * per_group;
    const int hk = grp % a.Hkv;
    FwdLean<KMASK, F, DROP, DOC> fl(a, lds);
    fl.run(grp / a.Hkv, hk * G + rem % G, hk, nqb - 1 - rem / G);
}

// ------------------------------------------------------------------------------------------------
// dQ: a workgroup = 4 waves x 32 query rows of one (b, q head), sweeping the K/V tiles up to the
// diagonal (staged as in the forward). Per tile: S^T = K Q^T, dP^T = V dO^T, P = exp2(S*c - lse),
// dS = P (dP - delta), dQ^T += K^T dS^T.
// ------------------------------------------------------------------------------------------------
// The dQ kernel also computes delta = rowsum(dO * O) of its own rows from the dO fragments it holds
// anyway (one O read) and writes it for the dK/dV kernel (no separate pass).

struct DqArgs {
    Tns q, k, v, dout, o;
    uint16_t* dq;
    int64_t dq_sb, dq_sh, dq_ss;
    const float* lse;
    float* delta;
    int lse_ld;                            // row stride of lse and delta
    const uint64_t* kmask;
    int64_t kmask_ld;
    int B, Hq, Hkv, S;
    float sl2, scale;
    DropArgs drop;                         // read by the DROP instances only
    const int32_t* doc_start;              // [B][S], read by the DOC instances only
};

// dQ (DqLean): a workgroup = 4 waves x 32 query rows of one (b, q head) sweeping the K/V tiles up to
// the diagonal; tiles in pairs (compile-time ring slot), explicit LDS addresses from two lane
// constants, S and dP from zero accumulators, p = exp2(c s - lse) and ds = p (dp - delta) in packed
// fp32, the causal test only on the wave's diagonal tile, scheduling fences that bound the fragment
// reads hoisted ahead. Measured and removed (git history): one wave per SIMD with AGPR
// accumulators, and dQ as a GEMM over a materialised dS, both slower.
// DOC: as in the forward (FwdLean).
template <bool KMASK, int F, bool DROP, bool DOC = false>
struct DqLean {
    const DqArgs& a;
    uint8_t* lds;
    bf16x8_t qf[8], df[8];
    f32x16_t dq[4];
    float lse, dlt;
    const uint64_t* km;
    __amdgpu_buffer_rsrc_t rk, rv;
    uint32_t lds0, lo_row, lo_t0, lo_t4;
    uint32_t drop_rk;                      // DROP: the lane's row key
    int doc_ds, doc_wmax, doc_t0;          // DOC: the lane's doc_start, the wave's largest, the wave's first tile
    int lane, wave, hi, l32, qw, qrow, nt, last;

    __device__ __forceinline__ DqLean(const DqArgs& a_, uint8_t* lds_) : a(a_), lds(lds_) {}

    __device__ __forceinline__ void issue(int t) {            // K(t), V(t) into slot t & 1
        const uint32_t slot = lds0 + (uint32_t)((t & 1) * 2 * kTileB);
        constexpr int rows_w = kKV / kDqWaves;
        dma_rows(rk, a.k.ss, slot, t * kKV, t * kKV + rows_w * wave, rows_w / 4, lane);
        dma_rows(rv, a.v.ss, slot + kTileB, t * kKV, t * kKV + rows_w * wave, rows_w / 4, lane);
    }

    template <int SLOT>
    __device__ __forceinline__ void compute(int t, bool diag) {
        constexpr int KI = SLOT * 2 * kTileB, VI = KI + kTileB;
        const int k0 = t * kKV;
        const uint32_t lr = opaque(lo_row);
        constexpr int KH = KI + 32 * kRowB, VH = VI + 32 * kRowB;     // keys 32..63 of the tile
        f32x16_t s[2], dp[2];
        s[0] = mfma<F>(rowx<KI>(lds, lr, 0), qf[0], f32x16_t{});
        s[1] = mfma<F>(rowx<KH>(lds, lr, 0), qf[0], f32x16_t{});
        dp[0] = mfma<F>(rowx<VI>(lds, lr, 0), df[0], f32x16_t{});
        dp[1] = mfma<F>(rowx<VH>(lds, lr, 0), df[0], f32x16_t{});
#pragma unroll
        for (int ks = 1; ks < 8; ++ks) {
            s[0] = mfma<F>(rowx<KI>(lds, lr, ks), qf[ks], s[0]);
            s[1] = mfma<F>(rowx<KH>(lds, lr, ks), qf[ks], s[1]);
            dp[0] = mfma<F>(rowx<VI>(lds, lr, ks), df[ks], dp[0]);
            dp[1] = mfma<F>(rowx<VH>(lds, lr, ks), df[ks], dp[1]);
            if (ks & 1) __builtin_amdgcn_sched_barrier(0);
        }
        float pr[32];
        const f32x2_t sl2v = {a.sl2, a.sl2}, lv = {-lse, -lse}, dv = {dlt, dlt};
#pragma unroll
        for (int i = 0; i < 32; i += 2) {
            const int j = i >> 4, ii = i & 15;
            const f32x2_t e = fma2<kPkDq>(f32x2_t{s[j][ii], s[j][ii + 1]}, sl2v, lv);
            pr[i] = __builtin_amdgcn_exp2f(e.x);
            pr[i + 1] = __builtin_amdgcn_exp2f(e.y);
        }
        if (diag) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                if (key > qrow) pr[i] = 0.f;
            }
        }
        if (KMASK) {
            const uint64_t w = km[k0 >> 6];                    // workgroup-uniform
            if (~w != 0ull) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                    if (!key_bit(w, key)) pr[i] = 0.f;
                }
            }
        }
        if constexpr (DOC) {
            if (k0 < doc_wmax) {                               // a document of this wave starts past k0
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
                    if (key < doc_ds) pr[i] = 0.f;
                }
            }
        }
        if constexpr (DROP) {                                  // dS = P (M dP r - delta)
            const uint32_t kt0 = ((uint32_t)(k0 >> 2) + (uint32_t)hi) * kDropKeyMul;
#pragma unroll
            for (int w = 0; w < 8; ++w) {                      // keys k0 + 32 (w>>2) + 8 (w&3) + 4 hi + 0..3
                const uint32_t word = drop_word(drop_rk, kt0 + (uint32_t)(8 * (w >> 2) + 2 * (w & 3)) * kDropKeyMul);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    dp[w >> 2][4 * (w & 3) + c] = drop_keep(word, c, a.drop.t) ? dp[w >> 2][4 * (w & 3) + c] * a.drop.r : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 32; i += 2) {
            const int j = i >> 4, ii = i & 15;
            const f32x2_t r = submul2<kPkDq>(f32x2_t{dp[j][ii], dp[j][ii + 1]}, dv, f32x2_t{pr[i], pr[i + 1]});
            pr[i] = r.x;
            pr[i + 1] = r.y;
        }
        bf16x8_t sf[4];
        pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&pr[0]), sf[0], sf[1]);
        pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&pr[16]), sf[2], sf[3]);
        const uint32_t t0 = opaque(lo_t0), t4 = opaque(lo_t4);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
            for (int kst = 0; kst < 4; ++kst) dq[dt] = mfma<F>(trx<KI>(lds, t0, t4, kst, dt), sf[kst], dq[dt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    template <int SLOT>
    __device__ __forceinline__ void tile(int t) {
        if (t + 1 < nt) issue(t + 1);
        if (t <= last && (!DOC || t >= doc_t0)) compute<SLOT>(t, t == last);
        vm_wait_all();
        __syncthreads();
    }

    __device__ __forceinline__ void run(int b, int h, int hk, int qb) {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        hi = lane >> 5;
        l32 = lane & 31;
        const int q0 = qb * kDqQB;
        qw = q0 + wave * kFwdQW;
        qrow = qw + l32;
        const bool qvalid = qrow < a.S;
        const uint16_t* qp = a.q.p + b * a.q.sb + h * a.q.sh;
        const uint16_t* dop = a.dout.p + b * a.dout.sb + h * a.dout.sh;
        const uint16_t* kp = a.k.p + b * a.k.sb + hk * a.k.sh;
        const uint16_t* vp = a.v.p + b * a.v.sb + hk * a.v.sh;
        km = KMASK ? a.kmask + (int64_t)b * a.kmask_ld : nullptr;
        if constexpr (DROP) drop_rk = drop_row_key(drop_head_key(*a.drop.seed, (uint32_t)(b * a.Hq + h)), (uint32_t)qrow);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (qvalid) {
                qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + qrow * a.q.ss + 16 * ks + 8 * hi);
                df[ks] = *reinterpret_cast<const bf16x8_t*>(dop + qrow * a.dout.ss + 16 * ks + 8 * hi);
            } else {
                qf[ks] = __builtin_bit_cast(bf16x8_t, u32x4_t{0u, 0u, 0u, 0u});
                df[ks] = qf[ks];
            }
        }
        const int64_t srow = ((int64_t)b * a.Hq + h) * a.lse_ld + (qvalid ? qrow : 0);
        lse = qvalid ? a.lse[srow] : 0.f;
        {
            const uint16_t* op = a.o.p + b * a.o.sb + h * a.o.sh;
            float part = 0.f;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const u32x4_t ov = qvalid ? *reinterpret_cast<const u32x4_t*>(op + qrow * a.o.ss + 16 * ks + 8 * hi)
                                          : u32x4_t{0u, 0u, 0u, 0u};
                const u32x4_t dv = __builtin_bit_cast(u32x4_t, df[ks]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    part += lo16<F>(ov[j]) * lo16<F>(dv[j]);
                    part += hi16<F>(ov[j]) * hi16<F>(dv[j]);
                }
            }
            dlt = halves_sum(part);
            if (qvalid && hi == 0) a.delta[srow] = dlt;
        }
        const int kv_end = min(a.S, q0 + kDqQB);
        nt = (kv_end + kKV - 1) / kKV;
        last = min(nt - 1, qw / kKV);
        rk = uniform_rsrc(kp, (int64_t)a.S * a.k.ss * 2);
        rv = uniform_rsrc(vp, (int64_t)a.S * a.v.ss * 2);
        lds0 = lds_addr(lds);
        lane_lds(lane, l32, hi, lo_row, lo_t0, lo_t4);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;
        int t0 = 0;                                            // the first tile of the sweep
        if constexpr (DOC) {
            const int32_t* ds = a.doc_start + (int64_t)b * a.S;
            doc_ds = qvalid ? doc_clamp(ds[qrow], 0, qrow) : 0;
            doc_wmax = wave_max(doc_ds);
            doc_t0 = wave_min(qvalid ? doc_ds : kIntMax) / kKV;        // a wave without a valid row: no tile
            t0 = doc_block_min(ds, q0, kDqQB, a.S, lane) / kKV;        // <= q0 / kKV < nt (row q0 is valid)
        }
        if (DOC || nt > 0) issue(t0);                          // nt > 0 always holds; the plain instances keep the test (header)
        vm_wait_all();
        vm_wait_all_known();
        __syncthreads();
        if (t0 & 1) {                                          // an odd first tile (DOC only): once through slot 1
            tile<1>(t0);
            ++t0;
        }
        for (int t = t0; t < nt; t += 2) {
            tile<0>(t);
            if (t + 1 < nt) tile<1>(t + 1);
        }
        if (qvalid) store_row<F>(a.dq + b * a.dq_sb + h * a.dq_sh + (int64_t)qrow * a.dq_ss, dq, a.scale, hi);
    }
};

template <bool KMASK, int F, bool DROP, bool DOC = false>
__global__ __launch_bounds__(64 * kDqWaves, 8 / kDqWaves)
void attn_dq_kernel(DqArgs a) {
    static_assert(!(KMASK && DOC), "no key mask beside documents");
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * kTileB];      // 64 KiB
    const int nqb = (a.S + kDqQB - 1) / kDqQB;
    const int G = a.Hq / a.Hkv;
    const int total = nqb * a.Hq * a.B;
    // consecutive ids: the G heads of one (b, kv head) at one q block, heaviest (longest causal row)
    // q blocks first (pairing q blocks measured 1-2 % slower here than this order)
    const int L = xcd_logical(blockIdx.x, total);
    const int per_group = G * nqb;
    const int grp = L / per_group;
    const int rem = L - grp * per_group;
    const int hk = grp % a.Hkv;
    DqLean<KMASK, F, DROP, DOC> dl(a, lds);
    dl.run(grp / a.Hkv, hk * G + rem % G, hk, nqb - 1 - rem / G);
}

// ------------------------------------------------------------------------------------------------
// dK, dV: a workgroup = 8 waves x 32 keys (256 keys) of one (b, kv head); it sweeps the G query
// heads x 32-row query slices from the block's first key to S, so the G heads' contributions are
// summed in registers (no atomics). K fragments live in registers, V rows in LDS (64 KiB); the
// Q / dO slices (+ their lse / delta) arrive by LDS-DMA into a kDkvLeanRing-deep ring (slices it+1 ..
// it+kDkvLeanRing-1 in flight while slice it is computed; the end-of-slice wait is a counted vmcnt).
// Per slice and wave: S = Q K^T and dP = dO V^T with the row constants (-lse/c, -delta) as the
// initial accumulators, P = exp2(c S'), dS = P dP', dV^T += dO^T P, dK^T += Q^T dS.
// Measured alternatives (profiles/r01_attn_variants.jsonl): V fragments in registers instead of the
// LDS image, and one wave per SIMD with 64 keys per wave (AGPR accumulators), both ran slower: at
// 256 VGPRs the kernel already spills ~30 registers, and every extra live value adds scratch reloads
// (each one a vmcnt wait) to the loop.
// ------------------------------------------------------------------------------------------------
// 256 keys per dK/dV workgroup (8 waves); 128-key workgroups of 4 waves (two per CU, independent
// barriers) measured the same (profiles/r03_attn_dkv128_ab.jsonl)
constexpr int kKB = 256, kKW = 32, kDkvWaves = kKB / kKW, kSlice = 32;
constexpr int kSliceB = kSlice * kRowB;            // 8 KiB per operand slice
constexpr int kSliceBuf = 2 * kSliceB + 256;       // Q, dO, 32 lse + 32 delta
constexpr int kVImg = kKB * kRowB;                 // 64 KiB

struct DkvArgs {
    Tns q, k, v, dout;
    uint16_t* dk;
    int64_t dk_sb, dk_sh, dk_ss;
    uint16_t* dv;
    int64_t dv_sb, dv_sh, dv_ss;
    const float* lse;
    const float* delta;
    int lse_ld;                            // row stride of lse and delta: >= S, % 4 == 0
    const uint64_t* kmask;
    int64_t kmask_ld;
    int B, Hq, Hkv, S;
    float sl2, scale;
    DropArgs drop;                         // read by the DROP instances only
    const int32_t* doc_end;                // [B][S], read by the DOC instances only
};

// dK / dV (DkvLean): the slice loop unrolled by two so that the ring slot is a compile-time LDS offset (the ring now sits in front of the V
// image, within the ds_read immediate range), S and dP started from zero accumulators and the row
// constants applied afterwards in packed fp32 (p = exp2(c s - lse), ds = p (dp - delta): v_pk_fma /
// v_pk_add / v_pk_mul), the causal test only on diagonal slices. Round 2's loop spilled ~30 VGPRs
// (the per-lane addresses of the runtime slot), and each scratch reload inside the loop carried a
// vmcnt wait that also drained the slice prefetch.
// Measured and removed (git history): one wave per SIMD x 64 keys with the accumulators in
// AGPRs (two builds), slower.
// slices in the ring (slices it+1 .. it+R-1 in flight while slice it is computed; rings of 2, 3 and 4
// measured 2.17, 2.21, 2.21 ms for the whole backward: profiles/r03_attn_bwd_variants.jsonl)
constexpr int kDkvLeanRing = 2;
static_assert(kDkvLeanRing >= 2 && kDkvLeanRing * kSliceBuf + kVImg <= 160 * 1024, "dK/dV lean ring");
// DROP: the 32 row keys of each ring slot's slice (one workgroup-wide copy, written by issue() under the
// ring's own barriers), after the V image so that the other LDS offsets are those of the plain kernels
constexpr int kDropRkOff = kDkvLeanRing * kSliceBuf + kVImg, kDropRkB = kSlice * 4;
static_assert(kDropRkOff + kDkvLeanRing * kDropRkB <= 160 * 1024, "dK/dV row keys");
// the word of 4-lane group member c, for all 4 lanes of the group (v_mov_b32 quad_perm:[c,c,c,c])
template <int C>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, C * 0x55, 0xf, 0xf, true);
}
// DOC: key on the lane, so the test is q >= doc_end[key] with the lane's own clamped doc_end (no
// per-slice data to stage). The sweep ends at doc_end of the block's last valid key instead of S
// (workgroup-uniform: it sizes n_sl, hence every issue, wait and barrier); a wave skips the compute
// of slices at or past its keys' largest doc_end and tests only slices that reach past their smallest.
template <bool KMASK, int F, bool DROP, bool DOC = false>
struct DkvLean {
    const DkvArgs& a;
    uint8_t* lds;
    bf16x8_t kf[8];
    f32x16_t dvt[4], dkt[4];
    int G, lane, wave, hi, l32, k0, kw, key, n_sl, n_it, b, hk, per_slice;
    bool kvalid;
    uint32_t lds0;
    uint32_t lo_row, lo_v, lo_t0, lo_t4;      // lane constants of the row / V-row / transposed reads
    uint64_t drop_seed;                       // DROP: the seed, the lane's (key >> 2) term and key & 3
    uint32_t drop_kt, drop_klo;
    int doc_de, doc_wmin, doc_wmax;           // DOC: the lane's doc_end, the wave's smallest and largest

    __device__ __forceinline__ DkvLean(const DkvArgs& a_, uint8_t* lds_) : a(a_), lds(lds_) {}

    __device__ __forceinline__ void issue(int it) {
        const int hh = it / n_sl, sl = n_sl - 1 - (it - hh * n_sl);
        const int h = hk * G + hh;
        const int s0 = k0 + sl * kSlice;
        const uint32_t buf = lds0 + (uint32_t)((it % kDkvLeanRing) * kSliceBuf);
        if (kDkvWaves == 8) {                              // waves 0-3: Q rows 8w.., waves 4-7: dO rows
            const bool is_q = wave < 4;
            const Tns& src = is_q ? a.q : a.dout;
            const uint16_t* base = src.p + b * src.sb + h * src.sh;
            dma_rows(uniform_rsrc(base, (int64_t)a.S * src.ss * 2), src.ss, buf + (is_q ? 0u : (uint32_t)kSliceB), s0,
                     s0 + 8 * (wave & 3), 2, lane);
        } else {                                           // 4 waves: Q and dO rows 8w .. 8w+7 each
            const uint16_t* qb = a.q.p + b * a.q.sb + h * a.q.sh;
            const uint16_t* db = a.dout.p + b * a.dout.sb + h * a.dout.sh;
            dma_rows(uniform_rsrc(qb, (int64_t)a.S * a.q.ss * 2), a.q.ss, buf, s0, s0 + 8 * wave, 2, lane);
            dma_rows(uniform_rsrc(db, (int64_t)a.S * a.dout.ss * 2), a.dout.ss, buf + (uint32_t)kSliceB, s0,
                     s0 + 8 * wave, 2, lane);
        }
        if (wave < 2 && lane < 8) {
            // Rows of lse_ld floats are 16-byte aligned for any S; the descriptor ends at entry S, so the
            // pad [S, lse_ld) is never fetched, whatever it holds. The range check of buffer_load_dwordx4
            // is per dword, also with the LDS destination: of the group that straddles S the entries
            // below S land and the others land as zeros, as every entry of a group past S does
            // (tests/test_gpu_attention_anylen.py::test_results_do_not_depend_on_the_pad holds NaN there).
            const float* row = (wave == 0 ? a.lse : a.delta) + ((int64_t)b * a.Hq + h) * a.lse_ld;
            dma16(uniform_rsrc(row, (int64_t)a.S * 4), __builtin_amdgcn_readfirstlane(buf + 2 * kSliceB + 128 * wave),
                  (s0 + 4 * lane) * 4);
        }
        if constexpr (DROP) {
            if (wave == 2 && lane < kSlice) {
                uint32_t* rkeys = reinterpret_cast<uint32_t*>(lds + kDropRkOff + (it % kDkvLeanRing) * kDropRkB);
                rkeys[lane] = drop_row_key(drop_head_key(drop_seed, (uint32_t)(b * a.Hq + h)), (uint32_t)(s0 + lane));
            }
        }
    }

    // the slice's s0, or -1 when no q of the slice sees a key of the wave (both phases skip it)
    __device__ __forceinline__ int slice_s0(int it) const {
        const int sl = n_sl - 1 - it % n_sl;               // descending q: the longest causal rows first
        const int s0 = k0 + sl * kSlice;
        if (DOC && s0 >= doc_wmax) return -1;
        return (s0 + kSlice - 1 < kw) ? -1 : s0;
    }

    // phase 1 of a slice (ring slot SLOT): S = Q K^T and dP = dO V^T
    template <int SLOT>
    __device__ __forceinline__ void qk(f32x16_t& s, f32x16_t& dp) {
        // ring slot SLOT at [SLOT * kSliceBuf, ...): Q rows, dO rows, lse[32], delta[32]; V image after the ring
        constexpr int QI = SLOT * kSliceBuf, DI = QI + kSliceB;
        const uint32_t lr = opaque(lo_row), lv = opaque(lo_v);
        s = mfma<F>(rowx<QI>(lds, lr, 0), kf[0], f32x16_t{});
        dp = mfma<F>(rowx<DI>(lds, lr, 0), rowx<0>(lds, lv, 0), f32x16_t{});
#pragma unroll
        for (int ks = 1; ks < 8; ++ks) {
            s = mfma<F>(rowx<QI>(lds, lr, ks), kf[ks], s);
            dp = mfma<F>(rowx<DI>(lds, lr, ks), rowx<0>(lds, lv, ks), dp);
            if (ks & 1) __builtin_amdgcn_sched_barrier(0);    // bound the reads hoisted ahead (VGPRs)
        }
    }

    // phase 2: P, dS, dV^T += dO^T P, dK^T += Q^T dS
    template <int SLOT>
    __device__ __forceinline__ void pv(int s0, const f32x16_t& s, const f32x16_t& dp) {
        constexpr int QI = SLOT * kSliceBuf, DI = QI + kSliceB;
        const float* cst = reinterpret_cast<const float*>(lds + QI + 2 * kSliceB);
        // rows q = s0 + (i&3) + 8(i>>2) + 4hi of register i; their constants are cst[8(i>>2) + 4hi + (i&3)]
        float pr[16], dsv[16];
        const f32x2_t sl2v = {a.sl2, a.sl2};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 lz = *reinterpret_cast<const float4*>(cst + 8 * g + 4 * hi);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = 4 * g + 2 * h;
                const f32x2_t l2 = h ? f32x2_t{lz.z, lz.w} : f32x2_t{lz.x, lz.y};
                const f32x2_t e = fma2<kPkDkv>(f32x2_t{s[i], s[i + 1]}, sl2v, -l2);
                pr[i] = __builtin_amdgcn_exp2f(e.x);
                pr[i + 1] = __builtin_amdgcn_exp2f(e.y);
            }
        }
        if (s0 < kw + kKW - 1) {                           // the slice crosses this wave's diagonal
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = s0 + (i & 3) + 8 * (i >> 2) + 4 * hi;
                if (key > q) pr[i] = 0.f;
            }
        }
        if (KMASK && !kvalid) {
#pragma unroll
            for (int i = 0; i < 16; ++i) pr[i] = 0.f;
        }
        if constexpr (DOC) {
            if (s0 + kSlice > doc_wmin) {                  // a document of this wave ends inside or before the slice
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int q = s0 + (i & 3) + 8 * (i >> 2) + 4 * hi;
                    if (q >= doc_de) pr[i] = 0.f;
                }
            }
        }
        bool kp[16];                                       // DROP: element i is kept
        if constexpr (DROP) {
            // the lane's 16 rows x its key need 16 words, the same 16 for the 4 lanes that share
            // key >> 2: member c of the group hashes the rows with (i & 3) == c, and all four read them
            const uint32_t* rkeys = reinterpret_cast<const uint32_t*>(lds + kDropRkOff + SLOT * kDropRkB);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t wq = drop_word(rkeys[8 * g + 4 * hi + (lane & 3)], drop_kt);
                kp[4 * g + 0] = drop_keep(quad_bcast<0>(wq), drop_klo, a.drop.t);
                kp[4 * g + 1] = drop_keep(quad_bcast<1>(wq), drop_klo, a.drop.t);
                kp[4 * g + 2] = drop_keep(quad_bcast<2>(wq), drop_klo, a.drop.t);
                kp[4 * g + 3] = drop_keep(quad_bcast<3>(wq), drop_klo, a.drop.t);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 dz = *reinterpret_cast<const float4*>(cst + 32 + 8 * g + 4 * hi);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = 4 * g + 2 * h;
                const f32x2_t d2 = h ? f32x2_t{dz.z, dz.w} : f32x2_t{dz.x, dz.y};
                f32x2_t dpv = {dp[i], dp[i + 1]};
                if constexpr (DROP)                        // dS = P (M dP r - delta)
                    dpv = f32x2_t{kp[i] ? dp[i] * a.drop.r : 0.f, kp[i + 1] ? dp[i + 1] * a.drop.r : 0.f};
                const f32x2_t r = submul2<kPkDkv>(dpv, d2, f32x2_t{pr[i], pr[i + 1]});
                dsv[i] = r.x;
                dsv[i + 1] = r.y;
            }
        }
        if constexpr (DROP) {                              // dV^T += dO^T (P M); r at the end (run)
#pragma unroll
            for (int i = 0; i < 16; ++i) pr[i] = kp[i] ? pr[i] : 0.f;
        }
        bf16x8_t pf[2], sf[2];
        pack_b_frags<F>(pr, pf[0], pf[1]);
        pack_b_frags<F>(dsv, sf[0], sf[1]);
        const uint32_t t0 = opaque(lo_t0), t4 = opaque(lo_t4);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int kq = 0; kq < 2; ++kq) {
                dvt[dt] = mfma<F>(trx<DI>(lds, t0, t4, kq, dt), pf[kq], dvt[dt]);
                dkt[dt] = mfma<F>(trx<QI>(lds, t0, t4, kq, dt), sf[kq], dkt[dt]);
                if (kq) __builtin_amdgcn_sched_barrier(0);
            }
    }

    // Both phases of slice it in one barrier interval. (Tried: waves 4-7 lagging half a slice behind
    // their SIMD partners - phase 2 of slice it-1, then phase 1 of slice it - so that one wave's MFMA
    // chain meets its partner's softmax VALU: S / dP then stay live across the barrier, and at 256
    // VGPRs per wave hipcc spilled ~90 registers inside the loop.)
    template <int SLOT>
    __device__ __forceinline__ void step(int it) {
        constexpr int R = kDkvLeanRing;
        if (it + R - 1 < n_it) issue(it + R - 1);          // into the slot slice it-1 used
        const int s0 = slice_s0(it);
        if (s0 >= 0) {
            f32x16_t s, dp;
            qk<SLOT>(s, dp);
            pv<SLOT>(s0, s, dp);
        }
        // slice it+1 landed; it+2 .. it+R-1 (those issued) may stay in flight
        vm_wait_upto(per_slice * max(0, min(R - 2, n_it - 2 - it)));
        __syncthreads();
    }

    template <int SLOT>
    __device__ __forceinline__ void steps(int it0) {       // slices it0 .. it0+R-1, slot = compile-time
        if (it0 + SLOT < n_it) {
            step<SLOT>(it0 + SLOT);
            if constexpr (SLOT + 1 < kDkvLeanRing) steps<SLOT + 1>(it0);
        }
    }

    __device__ __forceinline__ void run(int b_, int hk_, int kb) {
        b = b_;
        hk = hk_;
        G = a.Hq / a.Hkv;
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        hi = lane >> 5;
        l32 = lane & 31;
        k0 = kb * kKB;
        kw = k0 + wave * kKW;
        key = kw + l32;
        kvalid = !KMASK || (key < a.S && key_bit(a.kmask[(int64_t)b * a.kmask_ld + (key >> 6)], key));
        if constexpr (DROP) {
            drop_seed = *a.drop.seed;
            drop_kt = (uint32_t)(key >> 2) * kDropKeyMul;
            drop_klo = (uint32_t)(key & 3);
        }
        const uint16_t* kp = a.k.p + b * a.k.sb + hk * a.k.sh;
        const uint16_t* vp = a.v.p + b * a.v.sb + hk * a.v.sh;
        lds0 = lds_addr(lds);
        dma_rows(uniform_rsrc(vp, (int64_t)a.S * a.v.ss * 2), a.v.ss, lds0 + kDkvLeanRing * kSliceBuf, k0, kw, kKW / 4, lane);
        lane_lds(lane, l32, hi, lo_row, lo_t0, lo_t4);
        // V rows wave*32 + l32 (same swizzle as row l32), image after the ring (past the ds offset range)
        lo_v = lo_row + (uint32_t)(kDkvLeanRing * kSliceBuf + wave * kKW * kRowB);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            kf[ks] = frag_or_zero(key < a.S, kp + (int64_t)key * a.k.ss + 16 * ks + 8 * hi);
        }
        int s_end = a.S;
        if constexpr (DOC) {
            const int32_t* de = a.doc_end + (int64_t)b * a.S;
            const bool valid = key < a.S;
            doc_de = valid ? doc_clamp(de[key], key + 1, a.S) : kIntMax;
            doc_wmin = wave_min(doc_de);
            doc_wmax = wave_max(valid ? doc_de : 0);       // a wave without a valid key: no slice
            const int lk = min(k0 + kKB, a.S) - 1;         // the block's last valid key (k0 < S)
            s_end = doc_clamp(__builtin_amdgcn_readfirstlane(de[lk]), lk + 1, a.S);
        }
        n_sl = (s_end - k0 + kSlice - 1) / kSlice;
        n_it = G * n_sl;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) { dvt[dt][i] = 0.f; dkt[dt][i] = 0.f; }
        per_slice = (kDkvWaves == 8 ? 2 : 4) + (wave < 2 ? 1 : 0);   // DMA instructions per slice (+ lse / delta)
#pragma unroll
        for (int i = 0; i < kDkvLeanRing - 1; ++i)
            if (i < n_it) issue(i);
        vm_wait_all();
        vm_wait_all_known();                               // the K fragments too (compiler-visible)
        __syncthreads();
        for (int it = 0; it < n_it; it += kDkvLeanRing) steps<0>(it);
        if constexpr (DROP) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) dvt[dt][i] *= a.drop.r;
        }
        if (key < a.S) {
            uint16_t* dkr = a.dk + b * a.dk_sb + hk * a.dk_sh + (int64_t)key * a.dk_ss;
            uint16_t* dvr = a.dv + b * a.dv_sb + hk * a.dv_sh + (int64_t)key * a.dv_ss;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = 32 * dt + 8 * g + 4 * hi;
                    uint2 w;
                    w.x = pk16<F>(dkt[dt][4 * g] * a.scale, dkt[dt][4 * g + 1] * a.scale);
                    w.y = pk16<F>(dkt[dt][4 * g + 2] * a.scale, dkt[dt][4 * g + 3] * a.scale);
                    *reinterpret_cast<uint2*>(dkr + d) = w;
                    w.x = pk16<F>(dvt[dt][4 * g], dvt[dt][4 * g + 1]);
                    w.y = pk16<F>(dvt[dt][4 * g + 2], dvt[dt][4 * g + 3]);
                    *reinterpret_cast<uint2*>(dvr + d) = w;
                }
        }
    }
};

template <bool KMASK, int F, bool DROP, bool DOC = false>
__global__ __launch_bounds__(kDkvWaves * 64, 2)
void attn_dkdv_kernel(DkvArgs a) {
    static_assert(!(KMASK && DOC), "no key mask beside documents");
    __shared__ __attribute__((aligned(16))) uint8_t lds[kVImg + kDkvLeanRing * (kSliceBuf + (DROP ? kDropRkB : 0))];
    const int nkb = (a.S + kKB - 1) / kKB;
    const int total = ((nkb + 1) / 2) * a.Hkv * a.B;
    // key blocks kb (long causal sweep) and nkb-1-kb (short) in one workgroup: equal work per
    // workgroup (1594 vs 1946 us unpaired at B16 Hq32 Hkv8 S2048)
    const PairTask t = pair_task(xcd_logical(blockIdx.x, total), nkb, 1, a.Hkv);
#pragma nounroll
    for (int i = 0; i < t.n; ++i) {
        if (i) __syncthreads();
        DkvLean<KMASK, F, DROP, DOC> dl(a, lds);
        dl.run(t.b, t.hk, t.blk[1 - i]);
    }
}

// The keep mask of every (b, h, q, key) as bytes (smt_attn_dropout_mask): one thread per 4-key word.
__global__ __launch_bounds__(256)
void attn_dropout_mask_kernel(uint8_t* keep, DropArgs drop, int S, int64_t n_words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    const int wpr = (S + 3) >> 2;                          // words per (b, h, q) row
    const int64_t row = i / wpr;                           // (b*Hq + h)*S + q
    const int kw = (int)(i - row * wpr);
    const uint32_t bh = (uint32_t)(row / S), q = (uint32_t)(row - (int64_t)bh * S);
    const uint32_t word = drop_word(drop_row_key(drop_head_key(*drop.seed, bh), q), (uint32_t)kw * kDropKeyMul);
    for (int c = 0; c < 4; ++c) {
        const int key = 4 * kw + c;
        if (key < S) keep[row * S + key] = drop_keep(word, (uint32_t)c, drop.t) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// Cached (KV-cache) forward, smt_attn_fwd_cached: Sq query positions at absolute positions
// q_offset + i against keys [0, Skv); query i sees key j iff j <= q_offset + i (and j's mask bit).
// Bound by reading K/V once, so the 32 MFMA columns of S^T[key][col] = K Q^T are (query position,
// head within the KV group) pairs, col = i * G + g: all G query heads of a KV head ride on one read of
// its K/V. A workgroup is ONE wave: column block x split x (b, kv head). It sweeps the split's
// contiguous range of 64-key tiles with the decode step below. K/V rows at or past the column block's
// last visible key + 1 are outside the buffer descriptors: never read, zeros in LDS. Hidden keys are
// those past the column's own position (key > qpos) and those the key mask clears.
// ------------------------------------------------------------------------------------------------
constexpr int kDecCols = 32;
constexpr int kDecPartial = kDecCols * (kD + 2);           // floats per (b*Hkv, column block, split)

struct DecArgs {
    Tns q, k, v;
    uint16_t* o;
    int64_t o_sb, o_sh, o_ss;
    float* lse;                            // [B][Hq][Sq] or null
    const uint64_t* kmask;
    int64_t kmask_ld;
    float* ws;
    int Hq, Hkv, G, Sq, q_offset, ncols, ncb, nsplit, tps;     // ncols = Sq * G; tps = tiles per split
    float sl2;
};
struct DecPosArgs : DecArgs {              // the device-position form (DecArgs itself keeps its size)
    const int64_t* pos;
    int pos_stride, cap;
};

__device__ __forceinline__ float* dec_ws_o(const DecArgs& a, int64_t slot, int col) {
    return a.ws + (slot * kDecCols + col) * kD;
}
__device__ __forceinline__ float* dec_ws_ml(const DecArgs& a, int64_t nslots, int64_t slot, int col) {
    return a.ws + nslots * kDecCols * kD + (slot * kDecCols + col) * 2;
}

// The decode step, written once for attn_decode_kernel and attn_beams_kernel. The kernels differ in where
// a tile's K / V come from, in the tile list and in which keys a column sees; the rest is here. Tiles go
// through the forward's 2-slot LDS ring (2 workgroups = 128 KiB of landing buffers per CU; the tile after
// the one being computed is in flight) with the forward's lane maps, swizzle and deferred running max: a
// lane holds column l32 and the key rows (i & 3) + 8 ((i & 15) >> 2) + 32 (i >> 4) + 4 hi of a tile. Per
// tile: dec_zero_unseen_v, dec_scores, the kernel's own selection of hidden keys (x = -inf), dec_softmax_pv.
// num_splits > 1: fp32 partials per (b*Hkv, column block, split), O [32 col][128 d] then {max, sum}
// [32 col][2]; attn_decode_combine_kernel merges them in split order (no atomics). A split without a
// visible key writes max = -inf, sum = 0 and no O (dec_empty_split, dec_finish); the combine selects
// such splits out.

// the eight Q fragments of a column (qp: its row), zero for an unused column
__device__ __forceinline__ void dec_load_q(bf16x8_t (&qf)[8], bool cvalid, const uint16_t* qp, int hi) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = frag_or_zero(cvalid, qp + 16 * ks + 8 * hi);
}

// w_any: the tile's rows whose V stays. lane = the tile's row; the others are zeroed in LDS, so nothing
// from a row no column sees reaches the P V product.
__device__ __forceinline__ void dec_zero_unseen_v(uint8_t* V, uint64_t w_any, int lane) {
    if (~w_any == 0ull) return;
    if (!key_bit(w_any, lane)) {
#pragma unroll
        for (int c = 0; c < 16; ++c) *reinterpret_cast<u32x4_t*>(V + lane * kRowB + 16 * c) = u32x4_t{0u, 0u, 0u, 0u};
    }
    __syncthreads();
}

// S^T[key][col] = K Q^T of one tile, in the lane's 32 scores
template <int F>
__device__ __forceinline__ void dec_scores(float (&x)[32], const uint8_t* K, const bf16x8_t (&qf)[8], int l32, int hi) {
    f32x16_t sc[2];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            sc[j] = mfma<F>(row_frag(K, 32 * j + l32, 32 * ks + 16 * hi), qf[ks], ks ? sc[j] : f32x16_t{});
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) x[16 * j + i] = sc[j][i];
}

// The online softmax over x (hidden keys at -inf) and O += P V. The running max moves only when the
// tile's exceeds it by more than kFwdThr, and o is rescaled only in a tile where some lane's moved.
template <int F>
__device__ __forceinline__ void dec_softmax_pv(float (&x)[32], const uint8_t* V, TrLane tl, float sl2, float& m_run,
                                               float& l_run, f32x16_t (&o)[4]) {
    float mx = x[0];
#pragma unroll
    for (int i = 1; i < 32; ++i) mx = fmaxf(mx, x[i]);
    const float m_tile = other_half_max(mx) * sl2;
    const bool move = m_tile > m_run + kFwdThr;
    const float m_new = move ? m_tile : m_run;
    const float alpha = move ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.f;
    const float m_use = (m_new == kNegInf) ? 0.f : m_new;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        x[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], sl2, -m_use));
        sum += x[i];
    }
    l_run = l_run * alpha + sum;
    m_run = m_new;
    if (__builtin_amdgcn_ballot_w64(move) != 0) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    }
    bf16x8_t pf[4];
    pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&x[0]), pf[0], pf[1]);
    pack_b_frags<F>(*reinterpret_cast<const float(*)[16]>(&x[16]), pf[2], pf[3]);
#pragma unroll
    for (int n = 0; n < 16; ++n) o[n >> 2] = mfma<F>(tr_frag(V, tl, 16 * (n & 3), 32 * (n >> 2)), pf[n & 3], o[n >> 2]);
}

// A split without a tile (never with DIRECT); slot of nslots: the workgroup's partial, in the [b * Hkv]
// [column block][split] order. The test on DIRECT, cvalid and hi stays with the caller: inside this
// function it changed how the beams kernel stores {max, sum} (scripts/diag/isa_compare.py).
__device__ __forceinline__ void dec_empty_split(const DecArgs& a, int64_t nslots, int64_t slot, int l32) {
    float* ml = dec_ws_ml(a, nslots, slot, l32);
    ml[0] = kNegInf;
    ml[1] = 0.f;
}

// DIRECT (one split): the normalised row to a.o + o_idx and, with a.lse, its log-sum-exp to a.lse[lse_idx].
// Otherwise the split's partial: O as it is, then {max, sum}; max = -inf and no O without a visible key.
template <int F, bool DIRECT>
__device__ __forceinline__ void dec_finish(const DecArgs& a, const f32x16_t (&o)[4], float m_run, float l_run,
                                           int64_t nslots, int64_t slot, bool cvalid, int l32, int hi, int64_t o_idx,
                                           int64_t lse_idx) {
    const float l_tot = halves_sum(l_run);
    if (!cvalid) return;
    if (DIRECT) {
        store_row<F>(a.o + o_idx, o, l_tot > 0.f ? 1.f / l_tot : 0.f, hi);
        if (a.lse && hi == 0) a.lse[lse_idx] = l_tot > 0.f ? m_run + __log2f(l_tot) : __builtin_huge_valf();
    } else {
        const bool any = l_tot > 0.f;
        if (any) {
            float* po = dec_ws_o(a, slot, l32);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(po + 32 * dt + 8 * g + 4 * hi) =
                        float4{o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
        }
        if (hi == 0) {
            float* ml = dec_ws_ml(a, nslots, slot, l32);
            ml[0] = any ? m_run : kNegInf;
            ml[1] = any ? l_tot : 0.f;
        }
    }
}

// Args = DecPosArgs (smt_attn_fwd_cached_pos): the position of row b's first query is
// a.pos[b * a.pos_stride], read here and saturated into [0, cap - Sq] (cap = the K / V buffers' row
// count; Sq <= cap is checked by the host) before anything is derived from it, so no address depends on
// an out-of-contract value.
// The tile partition is then the one the host computes for that q_offset, and the grid is sized from
// the capacity. With Args = DecArgs, a.q_offset and a.tps are taken as they are.
template <bool KMASK, int F, bool DIRECT, class Args>
__global__ __launch_bounds__(64)
void attn_decode_kernel(Args a) {
    constexpr bool POS = std::is_same<Args, DecPosArgs>::value;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * kTileB];      // K/V ring: 2 x 32 KiB
    const int cb = blockIdx.x, sp = blockIdx.y, bh = blockIdx.z;
    const int b = bh / a.Hkv, hk = bh - b * a.Hkv;
    int q_offset = a.q_offset, tps = a.tps;
    if constexpr (POS) {
        int64_t p = a.pos[(int64_t)b * a.pos_stride];          // workgroup-uniform
        const int64_t p_max = (int64_t)a.cap - a.Sq;
        p = p < 0 ? 0 : (p > p_max ? p_max : p);
        q_offset = __builtin_amdgcn_readfirstlane((int)p);
        const int tiles = (q_offset + a.Sq + kKV - 1) / kKV;
        tps = (tiles + a.nsplit - 1) / a.nsplit;
    }
    const int lane = threadIdx.x, hi = lane >> 5, l32 = lane & 31;
    const int col = cb * kDecCols + l32;
    const bool cvalid = col < a.ncols;
    const int qi = cvalid ? col / a.G : 0;
    const int h = hk * a.G + (cvalid ? col - qi * a.G : 0);
    const int qpos = cvalid ? q_offset + qi : -1;            // an unused column sees no key
    // keys this column block can see: [0, kv_end), kv_end <= Skv (checked by the host, or by the clamp)
    const int kv_end = q_offset + min(a.Sq - 1, (cb * kDecCols + kDecCols - 1) / a.G) + 1;
    const int t0 = sp * tps, t1 = min((kv_end + kKV - 1) / kKV, t0 + tps);
    const int64_t nslots = (int64_t)gridDim.z * a.ncb * a.nsplit;
    const int64_t slot = ((int64_t)bh * a.ncb + cb) * a.nsplit + sp;
    if (t0 >= t1) {
        if (!DIRECT && cvalid && hi == 0) dec_empty_split(a, nslots, slot, l32);
        return;
    }
    const uint16_t* kp = a.k.p + b * a.k.sb + hk * a.k.sh;
    const uint16_t* vp = a.v.p + b * a.v.sb + hk * a.v.sh;
    const uint64_t* km = KMASK ? a.kmask + (int64_t)b * a.kmask_ld : nullptr;
    bf16x8_t qf[8];
    dec_load_q(qf, cvalid, a.q.p + b * a.q.sb + h * a.q.sh + (int64_t)qi * a.q.ss, hi);
    // the descriptors end with row kv_end - 1: later rows are never read (they land as zeros)
    const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(kp, (int64_t)(kv_end - 1) * a.k.ss * 2 + kRowB);
    const __amdgpu_buffer_rsrc_t rv = uniform_rsrc(vp, (int64_t)(kv_end - 1) * a.v.ss * 2 + kRowB);
    const uint32_t lds0 = lds_addr(lds);
    const TrLane tl = tr_lane(lane);
    f32x16_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    float m_run = kNegInf, l_run = 0.f;

    auto issue = [&](int t) {                                  // K(t), V(t) into slot t & 1
        const uint32_t s = lds0 + (uint32_t)((t & 1) * 2 * kTileB);
        dma_rows(rk, a.k.ss, s, t * kKV, t * kKV, kKV / 4, lane);
        dma_rows(rv, a.v.ss, s + kTileB, t * kKV, t * kKV, kKV / 4, lane);
    };
    issue(t0);
    vm_wait_all();
    vm_wait_all_known();                                       // the Q fragments too (compiler-visible)
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) issue(t + 1);
        uint8_t* K = lds + (t & 1) * 2 * kTileB;
        uint8_t* V = K + kTileB;
        const int k0 = t * kKV;
        uint64_t w = ~0ull;
        if (KMASK) {
            w = km[t];                                         // workgroup-uniform
            dec_zero_unseen_v(V, w, lane);                     // the V rows of masked keys
        }
        float x[32];
        dec_scores<F>(x, K, qf, l32, hi);
        // hidden keys leave by selection: the causal edge (which covers the ragged end, qpos < kv_end)
        // and the key mask
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int key = k0 + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hi;
            if (key > qpos || (KMASK && !key_bit(w, key))) x[i] = kNegInf;
        }
        dec_softmax_pv<F>(x, V, tl, a.sl2, m_run, l_run, o);
        vm_wait_all();
        __syncthreads();
    }
    dec_finish<F, DIRECT>(a, o, m_run, l_run, nslots, slot, cvalid, l32, hi, b * a.o_sb + h * a.o_sh + (int64_t)qi * a.o_ss,
                          ((int64_t)b * a.Hq + h) * a.Sq + qi);
}

// One workgroup per (column, b*Hkv), one thread per d: the splits' partials in split order.
// ROWS (smt_attn_fwd_beams, where the "query position" qi is the beam): lse is [B * Sq][Hq], row b * Sq + qi.
template <int F, bool ROWS = false>
__global__ __launch_bounds__(kD)
void attn_decode_combine_kernel(DecArgs a) {
    const int col = blockIdx.x, bh = blockIdx.y, d = threadIdx.x;
    const int b = bh / a.Hkv, hk = bh - b * a.Hkv;
    const int cb = col / kDecCols, c = col - cb * kDecCols;
    const int qi = col / a.G, h = hk * a.G + (col - qi * a.G);
    const int64_t nslots = (int64_t)gridDim.y * a.ncb * a.nsplit;
    const int64_t slot0 = ((int64_t)bh * a.ncb + cb) * a.nsplit;
    float M = kNegInf;
    for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, dec_ws_ml(a, nslots, slot0 + s, c)[0]);
    float L = 0.f, acc = 0.f;
    for (int s = 0; s < a.nsplit; ++s) {
        const float* ml = dec_ws_ml(a, nslots, slot0 + s, c);
        if (ml[0] == kNegInf) continue;                        // no visible key in this split: its O was not written
        const float wgt = __builtin_amdgcn_exp2f(ml[0] - M);
        L = __builtin_fmaf(wgt, ml[1], L);
        acc = __builtin_fmaf(wgt, dec_ws_o(a, slot0 + s, c)[d], acc);
    }
    const bool any = L > 0.f;
    const uint32_t r = pk16<F>(any ? acc / L : 0.f, 0.f);
    a.o[b * a.o_sb + h * a.o_sh + (int64_t)qi * a.o_ss + d] = (uint16_t)(r & 0xffffu);
    if (a.lse && d == 0)
        a.lse[ROWS ? ((int64_t)b * a.Sq + qi) * a.Hq + h : ((int64_t)b * a.Hq + h) * a.Sq + qi] =
            any ? M + __log2f(L) : __builtin_huge_valf();
}

// ------------------------------------------------------------------------------------------------
// Beam-shared cache, smt_attn_fwd_beams: one query position of N samples x nb beams against a cache
// that is never reordered. The prompt's K / V is stored once per sample; the generated K / V of step
// j sits in row j of the physical slot that wrote it, and anc[row][j] names the slot that holds the
// step-j key of that row's hypothesis. The 32 columns of a workgroup are (beam, head within the KV
// group) pairs of ONE (sample, KV head), col = beam * G + g: the beam plays the part the query position
// plays in attn_decode_kernel, and the tiles go through the same decode step (above), partials and
// combine. The tile list of a workgroup's (sample, KV head) is the prompt's 64-key tiles, then
// every slot's generated tiles, slot by slot: each physical row is fetched once per sample, whatever
// the number of beams that see it, and nothing is gathered. Splits are contiguous ranges of that list.
// Visibility is one 64-bit word per (column, tile): the prompt mask word for a prompt tile; for a
// generated tile of slot s, bit j = (anc[row][64 g + j] == s), built with one byte load per beam of
// the block (lane = the tile's row) and a ballot. The bytes of the next tile are fetched before its
// K / V (the loop's own wait covers them). anc only ever enters that comparison: no address depends
// on a value in it, and a value >= nb matches no slot. Rows past P (prompt) and past T (generated)
// are outside the buffer descriptors; a row inside them that no column of the block sees (a dead
// hypothesis, a masked prompt key) has its V row zeroed in LDS, and its scores leave by selection.
// ------------------------------------------------------------------------------------------------
struct BeamArgs : DecArgs {                // DecArgs: q / o with sb = nb rows, ss = one row; k, v = the prompt; Sq = nb
    Tns kg, vg;                            // generated K / V: row n * nb + slot, head, step
    const uint8_t* anc;
    int64_t anc_ld;
    int nb, P, T, pt, gt;                  // pt / gt: 64-key tiles of the prompt / of one slot's generated rows
};
struct BeamPosArgs : BeamArgs {            // the device-counter form (BeamArgs itself keeps its size); T = T_cap here
    const int32_t* steps;
};

struct BeamTile {
    int s, g;                              // s: the slot, -1 = the prompt; g: the tile within that segment
};
__device__ __forceinline__ BeamTile beam_tile(int t, int pt, int gt) {
    if (t < pt) return BeamTile{-1, t};
    const int u = t - pt, s = u / gt;
    return BeamTile{s, u - s * gt};
}
__device__ __forceinline__ BeamTile beam_next(BeamTile c, int pt, int gt) {
    ++c.g;
    if (c.g == (c.s < 0 ? pt : gt)) {
        c.g = 0;
        ++c.s;
    }
    return c;
}
// the first `rem` bits set (rem >= 64: all, rem <= 0: none)
__device__ __forceinline__ uint64_t low_bits(int rem) { return rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : (1ull << rem) - 1ull); }

constexpr int kBeamPre = 8;                // beams of a column block whose ancestry bytes are fetched a tile ahead

// Args = BeamPosArgs (smt_attn_fwd_beams_pos): the number of generated positions is *a.steps, read
// here and saturated into [1, T_cap] (a.T holds the capacity) before anything is derived from it, so no
// address depends on an out-of-contract value. gt, the tile list and the tiles per split are then the
// ones the host computes for that T, and the grid is sized from the capacity. The body reads the three
// through gen_T() / gen_gt() / gen_tps(): the kernel's own values here, a.T, a.gt and a.tps as they are
// with Args = BeamArgs. Selections on the constant POS and not locals or lambdas: those changed the code
// of the BeamArgs instances, which read nothing from the device (scripts/diag/isa_compare.py).
template <bool KMASK, int F, bool DIRECT, class Args>
__global__ __launch_bounds__(64)
void attn_beams_kernel(Args a) {
    constexpr bool POS = std::is_same<Args, BeamPosArgs>::value;
    int T_dev = 0, gt_dev = 0, tps_dev = 0;
    if constexpr (POS) {
        int s = *a.steps;                                      // workgroup-uniform
        s = s < 1 ? 1 : (s > a.T ? a.T : s);
        T_dev = __builtin_amdgcn_readfirstlane(s);
        gt_dev = (T_dev + kKV - 1) / kKV;
        tps_dev = (a.pt + a.nb * gt_dev + a.nsplit - 1) / a.nsplit;
    }
#define gen_T() (POS ? T_dev : a.T)
#define gen_gt() (POS ? gt_dev : a.gt)
#define gen_tps() (POS ? tps_dev : a.tps)
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * kTileB];      // K/V ring: 2 x 32 KiB
    const int cb = blockIdx.x, sp = blockIdx.y, bh = blockIdx.z;
    const int n = bh / a.Hkv, hk = bh - n * a.Hkv;
    const int lane = threadIdx.x, hi = lane >> 5, l32 = lane & 31;
    const int col = cb * kDecCols + l32;
    const bool cvalid = col < a.ncols;
    const int beam = cvalid ? col / a.G : -1;                  // an unused column sees no key
    const int h = hk * a.G + (cvalid ? col - beam * a.G : 0);
    // the beams this column block holds (workgroup-uniform)
    const int b_lo = (cb * kDecCols) / a.G, b_hi = min(a.nb - 1, (cb * kDecCols + kDecCols - 1) / a.G);
    const int t0 = sp * gen_tps(), t1 = min(a.pt + a.nb * gen_gt(), t0 + gen_tps());
    const int64_t nslots = (int64_t)gridDim.z * a.ncb * a.nsplit;
    const int64_t slot = ((int64_t)bh * a.ncb + cb) * a.nsplit + sp;
    if (t0 >= t1) {
        if (!DIRECT && cvalid && hi == 0) dec_empty_split(a, nslots, slot, l32);
        return;
    }
    const int64_t row0 = (int64_t)n * a.nb;                    // the sample's first row / slot
    const uint64_t* km = KMASK ? a.kmask + (int64_t)n * a.kmask_ld : nullptr;
    bf16x8_t qf[8];
    dec_load_q(qf, cvalid, a.q.p + n * a.q.sb + h * a.q.sh + (int64_t)(cvalid ? beam : 0) * a.q.ss, hi);
    const uint32_t lds0 = lds_addr(lds);
    const TrLane tl = tr_lane(lane);
    f32x16_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    float m_run = kNegInf, l_run = 0.f;

    // K, V of tile bt into slot t & 1. The descriptors end with the segment's last row (P - 1 of the
    // prompt, T - 1 of a slot): later rows are never read (they land as zeros). The slot index comes
    // from the tile counter, never from anc.
    auto issue = [&](int t, BeamTile bt) {
        const uint32_t s = lds0 + (uint32_t)((t & 1) * 2 * kTileB);
        const bool pr = bt.s < 0;
        const uint16_t* kb = pr ? a.k.p + n * a.k.sb + hk * a.k.sh : a.kg.p + (row0 + bt.s) * a.kg.sb + hk * a.kg.sh;
        const uint16_t* vb = pr ? a.v.p + n * a.v.sb + hk * a.v.sh : a.vg.p + (row0 + bt.s) * a.vg.sb + hk * a.vg.sh;
        const int64_t kss = pr ? a.k.ss : a.kg.ss, vss = pr ? a.v.ss : a.vg.ss;
        const int rows = pr ? a.P : gen_T();
        const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(kb, (int64_t)(rows - 1) * kss * 2 + kRowB);
        const __amdgpu_buffer_rsrc_t rv = uniform_rsrc(vb, (int64_t)(rows - 1) * vss * 2 + kRowB);
        dma_rows(rk, kss, s, bt.g * kKV, bt.g * kKV, kKV / 4, lane);
        dma_rows(rv, vss, s + kTileB, bt.g * kKV, bt.g * kKV, kKV / 4, lane);
    };
    // anc[row of beam b_lo + kBeamPre * chunk + i][64 g + lane] of a generated tile, -1 where there is
    // no such beam, no such step (>= T) or the tile is the prompt's: -1 equals no slot
    auto load_anc = [&](BeamTile bt, int chunk, int (&v)[kBeamPre]) {
        const int j = bt.g * kKV + lane;
#pragma unroll
        for (int i = 0; i < kBeamPre; ++i) {
            const int bm = b_lo + chunk * kBeamPre + i;
            v[i] = (bt.s >= 0 && bm <= b_hi && j < gen_T()) ? (int)a.anc[(row0 + bm) * a.anc_ld + j] : -1;
        }
    };

    BeamTile cur = beam_tile(t0, a.pt, gen_gt());
    int pre[kBeamPre];
    load_anc(cur, 0, pre);
    issue(t0, cur);
    vm_wait_all();
    vm_wait_all_known();                                       // the Q fragments and pre too (compiler-visible)
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        // w_col: the keys of this tile this lane's column sees; w_any: the rows whose V stays (seen by a
        // column of the block, or outside the descriptor and zero already)
        uint64_t w_col, w_any;
        if (cur.s < 0) {
            const uint64_t in = low_bits(a.P - cur.g * kKV);
            const uint64_t w = (KMASK ? km[cur.g] : ~0ull) & in;   // workgroup-uniform
            w_col = cvalid ? w : 0ull;
            w_any = w | ~in;
        } else {
            w_col = 0ull;
            w_any = ~low_bits(gen_T() - cur.g * kKV);
            for (int c = 0; b_lo + c * kBeamPre <= b_hi; ++c) {
                if (c) load_anc(cur, c, pre);                  // more than kBeamPre beams in the block: fetched here
#pragma unroll
                for (int i = 0; i < kBeamPre; ++i) {
                    const uint64_t w = __builtin_amdgcn_ballot_w64(pre[i] == cur.s);
                    w_any |= w;
                    if (beam == b_lo + c * kBeamPre + i) w_col = w;
                }
            }
        }
        const BeamTile nxt = beam_next(cur, a.pt, gen_gt());
        if (t + 1 < t1) {
            load_anc(nxt, 0, pre);
            issue(t + 1, nxt);
        }
        uint8_t* K = lds + (t & 1) * 2 * kTileB;
        uint8_t* V = K + kTileB;
        dec_zero_unseen_v(V, w_any, lane);
        float x[32];
        dec_scores<F>(x, K, qf, l32, hi);
        // hidden keys leave by selection
        const uint64_t w_hi = w_col >> (4 * hi);
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int key = 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2);       // + 4 * hi, shifted in above
            if (!key_bit(w_hi, key)) x[i] = kNegInf;
        }
        dec_softmax_pv<F>(x, V, tl, a.sl2, m_run, l_run, o);
        vm_wait_all();
        vm_wait_all_known();                                   // pre of the next tile has landed (compiler-visible)
        __syncthreads();
        cur = nxt;
    }
    dec_finish<F, DIRECT>(a, o, m_run, l_run, nslots, slot, cvalid, l32, hi, n * a.o_sb + h * a.o_sh + (int64_t)beam * a.o_ss,
                          (row0 + beam) * a.Hq + h);
}
#undef gen_T
#undef gen_gt
#undef gen_tps

// smt_attn_kv_append_pos: one step's K and V, [R][Hkv][1][128] each, into row clamp(*steps, 1, cap) - 1 of
// the generated buffers [R][Hkv][cap][128]. One thread per 16-byte piece of a (tensor, row, head); the
// row index is the saturated counter, so no address depends on an out-of-contract value.
struct AppendArgs {
    Tns kn, vn, kg, vg;
    const int32_t* steps;
    int Hkv, cap, n;
};
__global__ __launch_bounds__(256)
void attn_kv_append_kernel(AppendArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int s = *a.steps;
    s = s < 1 ? 1 : (s > a.cap ? a.cap : s);
    const int piece = i & (kD / 8 - 1), rh = i / (kD / 8);
    const int isv = rh & 1, r_h = rh >> 1;
    const int r = r_h / a.Hkv, h = r_h - r * a.Hkv;
    const Tns& src = isv ? a.vn : a.kn;
    const Tns& dst = isv ? a.vg : a.kg;
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src.p + r * src.sb + h * src.sh + 8 * piece);
    *reinterpret_cast<u32x4_t*>(const_cast<uint16_t*>(dst.p) + r * dst.sb + h * dst.sh + (int64_t)(s - 1) * dst.ss + 8 * piece) = w;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_tensor(const smt_attn_tensor* t, const char* what, const char* fn) {
    if (!t || !t->ptr) return fail(-1, "%s: null %s", fn, what);
    if (!al16(t->ptr) || (t->sb & 7) || (t->sh & 7) || (t->ss & 7))
        return fail(-2, "%s: %s needs 16-byte aligned rows (strides %% 8 == 0)", fn, what);
    return 0;
}

int check_shape(const smt_attn_shape* s, const char* fn) {
    if (!s) return fail(-1, "%s: null shape", fn);
    if (s->B <= 0 || s->Hq <= 0 || s->Hkv <= 0 || s->S <= 0 || s->Hq % s->Hkv)
        return fail(-1, "%s: bad shape B=%d Hq=%d Hkv=%d S=%d", fn, s->B, s->Hq, s->Hkv, s->S);
    if (!(s->scale > 0.f)) return fail(-1, "%s: scale must be > 0", fn);
    if (s->dtype != SMT_DTYPE_BF16 && s->dtype != SMT_DTYPE_FP16)
        return fail(-1, "%s: dtype %d is not a 16-bit format (SMT_DTYPE_BF16 / SMT_DTYPE_FP16)", fn, (int)s->dtype);
    return 0;
}

// Picks a kernel instance: dispatch(dtype, fn, bools...) calls the generic lambda fn(f, c...) with the
// format as a std::integral_constant and each runtime bool as a std::bool_constant, so f() and c() are
// template arguments inside fn. A combination that has no instance (a key mask beside documents) is
// fenced off with if constexpr there, and is never instantiated.
template <class Fn>
void with_bools(Fn&& fn) { fn(); }
template <class Fn, class... Rest>
void with_bools(Fn&& fn, bool b, Rest... rest) {
    if (b) with_bools([&](auto... c) { fn(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { fn(std::false_type{}, c...); }, rest...);
}
template <class Fn, class... Bools>
void dispatch(int dtype, Fn&& fn, Bools... bools) {
    if (dtype == SMT_DTYPE_FP16)
        with_bools([&](auto... c) { fn(std::integral_constant<int, SMT_DTYPE_FP16>{}, c...); }, bools...);
    else with_bools([&](auto... c) { fn(std::integral_constant<int, SMT_DTYPE_BF16>{}, c...); }, bools...);
}

Tns tns(const smt_attn_tensor* t) { return Tns{static_cast<const uint16_t*>(t->ptr), t->sb, t->sh, t->ss}; }

// t of the keep function, or -1 for p outside [0, 1) or NaN
int drop_threshold(float p) {
    if (!(p >= 0.f && p < 1.f)) return -1;
    const int t = (int)(p * 256.f + 0.5f);
    return t > 255 ? 255 : t;
}

// p and seed of a *_dropout call -> DropArgs (t == 0: no dropout); validated before any HIP call
int check_drop(float p, const uint64_t* seed, const char* fn, DropArgs* d) {
    const int t = drop_threshold(p);
    if (t < 0) return fail(-1, "%s: dropout p = %g is outside [0, 1)", fn, (double)p);
    if (t > 0 && !seed) return fail(-1, "%s: null seed with dropout p = %g", fn, (double)p);
    d->seed = seed;
    d->t = (uint32_t)t;
    d->r = 256.f / (float)(256 - t);
    return 0;
}

// doc_start / doc_end of a *_docs call (both set, never with a key mask)
struct DocArgs {
    const int32_t* start;
    const int32_t* end;
};
constexpr DocArgs kNoDocs = {nullptr, nullptr};

// the row stride of a key mask against the keys it has to cover (keys_name: "S" / "Skv" of the message)
int check_kmask_ld(const char* fn, const uint64_t* key_mask, int64_t key_mask_ld, int keys, const char* keys_name) {
    if (key_mask && key_mask_ld < (keys + 63) / 64)
        return fail(-1, "%s: key_mask_ld %lld < ceil(%s / 64)", fn, (long long)key_mask_ld, keys_name);
    return 0;
}

// the fields that FwdArgs, DqArgs and DkvArgs share
template <class Args, class Lse>
void fill_common(Args& a, const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v, Lse* lse,
                 int64_t lse_ld, const uint64_t* key_mask, int64_t key_mask_ld, DropArgs drop,
                 const smt_attn_shape* shape) {
    a.q = tns(q); a.k = tns(k); a.v = tns(v);
    a.lse = lse; a.lse_ld = (int)lse_ld;
    a.kmask = key_mask; a.kmask_ld = key_mask_ld;
    a.B = shape->B; a.Hq = shape->Hq; a.Hkv = shape->Hkv; a.S = shape->S;
    a.sl2 = shape->scale * 1.4426950408889634f;
    a.drop = drop;
}

// fn: the entry point's name for messages; drop.t == 0: the plain instances; docs.start: the DOC instances
// (never beside a key mask: the *_docs entry points take none and check_ld refuses the pair)
int attn_fwd(const char* fn, const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
             const smt_attn_tensor* o, float* lse, int64_t lse_ld, const uint64_t* key_mask, int64_t key_mask_ld,
             DropArgs drop, DocArgs docs, const smt_attn_shape* shape, hipStream_t stream) {
    int rc;
    if ((rc = check_shape(shape, fn)) || (rc = check_tensor(q, "q", fn)) || (rc = check_tensor(k, "k", fn)) ||
        (rc = check_tensor(v, "v", fn)) || (rc = check_tensor(o, "o", fn)))
        return rc;
    if (!lse) return fail(-1, "%s: null lse", fn);
    if ((rc = check_kmask_ld(fn, key_mask, key_mask_ld, shape->S, "S"))) return rc;
    FwdArgs a;
    fill_common(a, q, k, v, lse, lse_ld, key_mask, key_mask_ld, drop, shape);
    a.o = static_cast<uint16_t*>(o->ptr); a.o_sb = o->sb; a.o_sh = o->sh; a.o_ss = o->ss;
    a.doc_start = docs.start;
    const int64_t nqb = (shape->S + kFwdQB - 1) / kFwdQB;
    const int64_t blocks = nqb * shape->Hq * shape->B;
    if (blocks > 0x7fffffffLL) return fail(-1, "%s: too many blocks", fn);
    dispatch(shape->dtype, [&](auto f, auto km, auto dr, auto doc) {
        if constexpr (!(km() && doc()))
            hipLaunchKernelGGL((attn_fwd_kernel<km(), f(), dr(), doc()>), dim3((unsigned)blocks), dim3(64 * kFwdWaves), 0,
                               stream, a);
    }, key_mask && !docs.start, drop.t != 0, docs.start != nullptr);
    return check_launch("attn_fwd_kernel");
}

int attn_bwd(const char* fn, const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
             const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws, int64_t lse_ld,
             const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
             const uint64_t* key_mask, int64_t key_mask_ld, DropArgs drop, DocArgs docs, const smt_attn_shape* shape,
             hipStream_t stream) {
    int rc;
    if ((rc = check_shape(shape, fn)) || (rc = check_tensor(q, "q", fn)) || (rc = check_tensor(k, "k", fn)) ||
        (rc = check_tensor(v, "v", fn)) || (rc = check_tensor(o, "o", fn)) || (rc = check_tensor(d_o, "do", fn)) ||
        (rc = check_tensor(dq, "dq", fn)) || (rc = check_tensor(dk, "dk", fn)) || (rc = check_tensor(dv, "dv", fn)))
        return rc;
    if (!lse || !delta_ws) return fail(-1, "%s: null lse / delta workspace", fn);
    // lse_ld == S from the entry points without a stride of their own (the *_ld ones refuse such a stride first)
    if (lse_ld & 3) return fail(-2, "%s: lse / delta need 16-byte rows (S %% 4 == 0; any S through smt_attn_bwd_ld)", fn);
    if (!al16(lse) || !al16(delta_ws)) return fail(-2, "%s: lse / delta need 16-byte aligned base pointers", fn);
    if ((rc = check_kmask_ld(fn, key_mask, key_mask_ld, shape->S, "S"))) return rc;
    const int B = shape->B, Hq = shape->Hq, Hkv = shape->Hkv, S = shape->S;
    const bool masked = key_mask && !docs.start, dropping = drop.t != 0, packed = docs.start != nullptr;

    DqArgs qa;
    fill_common(qa, q, k, v, lse, lse_ld, key_mask, key_mask_ld, drop, shape);
    qa.dout = tns(d_o); qa.o = tns(o);
    qa.dq = static_cast<uint16_t*>(dq->ptr); qa.dq_sb = dq->sb; qa.dq_sh = dq->sh; qa.dq_ss = dq->ss;
    qa.delta = delta_ws; qa.scale = shape->scale;
    qa.doc_start = docs.start;
    const int64_t nqb = (S + kDqQB - 1) / kDqQB;
    const dim3 qgrid((unsigned)(nqb * Hq * B)), qblock(64 * kDqWaves);
    dispatch(shape->dtype, [&](auto f, auto km, auto dr, auto doc) {
        if constexpr (!(km() && doc()))
            hipLaunchKernelGGL((attn_dq_kernel<km(), f(), dr(), doc()>), qgrid, qblock, 0, stream, qa);
    }, masked, dropping, packed);
    if ((rc = check_launch("attn_dq_kernel"))) return rc;

    DkvArgs ka;
    fill_common(ka, q, k, v, lse, lse_ld, key_mask, key_mask_ld, drop, shape);
    ka.dout = tns(d_o);
    ka.dk = static_cast<uint16_t*>(dk->ptr); ka.dk_sb = dk->sb; ka.dk_sh = dk->sh; ka.dk_ss = dk->ss;
    ka.dv = static_cast<uint16_t*>(dv->ptr); ka.dv_sb = dv->sb; ka.dv_sh = dv->sh; ka.dv_ss = dv->ss;
    ka.delta = delta_ws; ka.scale = shape->scale;
    ka.doc_end = docs.end;
    const int64_t nkb = (S + kKB - 1) / kKB;
    const dim3 grid((unsigned)(((nkb + 1) / 2) * Hkv * B));
    dispatch(shape->dtype, [&](auto f, auto km, auto dr, auto doc) {
        if constexpr (!(km() && doc()))
            hipLaunchKernelGGL((attn_dkdv_kernel<km(), f(), dr(), doc()>), grid, dim3(kDkvWaves * 64), 0, stream, ka);
    }, masked, dropping, packed);
    return check_launch("attn_dkdv_kernel");
}

constexpr DropArgs kNoDrop = {nullptr, 0u, 1.f};

// lse_ld of the entry points without a stride of their own: S (a null shape is refused by attn_fwd / attn_bwd)
int64_t own_ld(const smt_attn_shape* shape) { return shape ? shape->S : 0; }

// what only the *_ld entry points can get wrong: the stride, and documents beside a key mask (the
// shape itself is checked by attn_fwd / attn_bwd, a null one included)
int check_ld(const char* fn, int64_t lse_ld, const uint64_t* key_mask, const int32_t* doc_start, const int32_t* doc_end,
             const smt_attn_shape* shape) {
    if (shape && lse_ld < shape->S) return fail(-1, "%s: lse_ld %lld < S %d", fn, (long long)lse_ld, shape->S);
    if (lse_ld & 3) return fail(-1, "%s: lse_ld %lld is not a multiple of 4 (16-byte rows)", fn, (long long)lse_ld);
    if (lse_ld > 0x7fffffffLL) return fail(-1, "%s: lse_ld %lld is above 2^31 - 1", fn, (long long)lse_ld);
    if (!doc_start != !doc_end) return fail(-1, "%s: doc_start and doc_end come together (one is null)", fn);
    if (doc_start && key_mask) return fail(-1, "%s: a key mask and documents together are not supported", fn);
    return 0;
}

// Cached forward: column blocks of a call, and the default split count. Host arithmetic only.
int dec_col_blocks(const smt_attn_shape* s, int32_t Sq) {
    return (int)(((int64_t)Sq * (s->Hq / s->Hkv) + kDecCols - 1) / kDecCols);
}

// Workgroups are one wave with a 64 KiB ring, two per CU: 512 run at once on the 256 CUs. Split until
// the grid has that many, but never below kDecMinTiles tiles per split (a split's fixed cost: the Q
// load, a first tile nothing overlaps, its partials and their combine).
constexpr int kDecWgSlots = 512, kDecMinTiles = 2;
int default_splits(int64_t base_workgroups, int64_t tiles) {
    int64_t n = (kDecWgSlots + base_workgroups - 1) / base_workgroups;
    if (n > tiles / kDecMinTiles) n = tiles / kDecMinTiles;
    return n < 1 ? 1 : (int)n;
}
int dec_default_splits(const smt_attn_shape* s, int32_t Sq) {
    return default_splits((int64_t)s->B * s->Hkv * dec_col_blocks(s, Sq), ((int64_t)s->S + kKV - 1) / kKV);
}

int64_t dec_workspace(const smt_attn_shape* s, int32_t Sq, int32_t num_splits) {
    if (num_splits <= 1) return 0;
    return (int64_t)s->B * s->Hkv * dec_col_blocks(s, Sq) * num_splits * kDecPartial * (int64_t)sizeof(float);
}

// The split count of a call (num_splits, or fallback for 0) and the workspace it needs; ws_fn names the
// entry point that sizes the workspace.
int check_splits(const char* fn, int32_t num_splits, int fallback, const void* workspace, const char* ws_fn, int* nsplit) {
    if (num_splits < 0) return fail(-1, "%s: num_splits = %d is negative", fn, (int)num_splits);
    const int n = *nsplit = num_splits ? num_splits : fallback;
    if (n > 65535) return fail(-1, "%s: num_splits = %d is above 65535", fn, n);
    if (n > 1 && !workspace) return fail(-1, "%s: null workspace with %d splits (%s bytes)", fn, n, ws_fn);
    if (n > 1 && !al16(workspace)) return fail(-2, "%s: workspace needs 16-byte alignment", fn);
    return 0;
}

// the fields of DecArgs that both decode launchers fill alike; Sq: the query positions, or the beams
void fill_dec_common(DecArgs& a, const smt_attn_tensor* o, int64_t o_sb, int64_t o_ss, float* lse, void* workspace,
                     const smt_attn_shape* shape, int32_t Sq, int nsplit) {
    a.o = static_cast<uint16_t*>(o->ptr); a.o_sb = o_sb; a.o_sh = o->sh; a.o_ss = o_ss;
    a.lse = lse;
    a.ws = static_cast<float*>(workspace);
    a.Hq = shape->Hq; a.Hkv = shape->Hkv; a.G = shape->Hq / shape->Hkv;
    a.Sq = Sq; a.ncols = Sq * a.G; a.ncb = dec_col_blocks(shape, Sq); a.nsplit = nsplit;
    a.sl2 = shape->scale * 1.4426950408889634f;
}

// The kernel of an argument struct, and the launch both decode launchers end with: a (by_pos: ap, the
// device-position form of the same call) on the grid column block x split x (b, kv head), then the combine
// of the splits' partials. The beams' combine writes lse by rows (ROWS).
template <bool KMASK, int F, bool DIRECT, class Args>
constexpr auto decode_kernel() {
    if constexpr (std::is_base_of<BeamArgs, Args>::value) return attn_beams_kernel<KMASK, F, DIRECT, Args>;
    else return attn_decode_kernel<KMASK, F, DIRECT, Args>;
}
template <class Args, class PosArgs>
int launch_decode(const Args& a, const PosArgs& ap, bool by_pos, const smt_attn_shape* shape, hipStream_t stream) {
    constexpr bool ROWS = std::is_base_of<BeamArgs, Args>::value;
    const unsigned bh = (unsigned)(shape->B * shape->Hkv);
    const dim3 grid((unsigned)a.ncb, (unsigned)a.nsplit, bh);
    dispatch(shape->dtype, [&](auto f, auto km, auto direct, auto pos_form) {
        if constexpr (pos_form())
            hipLaunchKernelGGL((decode_kernel<km(), f(), direct(), PosArgs>()), grid, dim3(64), 0, stream, ap);
        else hipLaunchKernelGGL((decode_kernel<km(), f(), direct(), Args>()), grid, dim3(64), 0, stream, a);
    }, a.kmask != nullptr, a.nsplit == 1, by_pos);
    int rc;
    if ((rc = check_launch(ROWS ? "attn_beams_kernel" : "attn_decode_kernel")) || a.nsplit == 1) return rc;
    dispatch(shape->dtype, [&](auto f) {
        hipLaunchKernelGGL((attn_decode_combine_kernel<f(), ROWS>), dim3((unsigned)a.ncols, bh), dim3(kD), 0, stream,
                           static_cast<const DecArgs&>(a));
    });
    return check_launch("attn_decode_combine_kernel");
}

// smt_attn_fwd_cached (pos == nullptr: the position is q_offset) and smt_attn_fwd_cached_pos (the
// position is read by the kernel; q_offset is unused and the bounds are taken on the capacity Skv).
int attn_fwd_cached(const char* fn, const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                    const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld, int32_t Sq,
                    int32_t q_offset, const int64_t* pos, int32_t pos_stride, bool by_pos, int32_t num_splits,
                    void* workspace, const smt_attn_shape* shape, hipStream_t stream) {
    int rc;
    if ((rc = check_shape(shape, fn)) || (rc = check_tensor(q, "q", fn)) || (rc = check_tensor(k, "k", fn)) ||
        (rc = check_tensor(v, "v", fn)) || (rc = check_tensor(o, "o", fn)))
        return rc;
    const int Skv = shape->S;
    if (Sq < 1) return fail(-1, "%s: Sq = %d (at least one query position)", fn, (int)Sq);
    if (by_pos) {
        if (!pos) return fail(-1, "%s: null positions", fn);
        if (reinterpret_cast<uintptr_t>(pos) & 7u) return fail(-2, "%s: positions need 8-byte alignment (int64)", fn);
        if (pos_stride != 0 && pos_stride != 1)
            return fail(-1, "%s: positions_stride = %d (0: one position for the batch, 1: one per row)", fn, (int)pos_stride);
        if (Sq > Skv) return fail(-1, "%s: Sq %d > Skv %d (a query without a key slot of its own)", fn, (int)Sq, Skv);
    } else {
        if (q_offset < 0) return fail(-1, "%s: q_offset = %d is negative", fn, (int)q_offset);
        if ((int64_t)q_offset + Sq > Skv)
            return fail(-1, "%s: q_offset %d + Sq %d > Skv %d (a query without a key slot of its own)", fn, (int)q_offset,
                        (int)Sq, Skv);
    }
    int nsplit;
    if ((rc = check_kmask_ld(fn, key_mask, key_mask_ld, Skv, "Skv")) ||
        (rc = check_splits(fn, num_splits, dec_default_splits(shape, Sq), workspace, "smt_attn_cached_workspace", &nsplit)))
        return rc;
    // keys any query of the call sees: [0, kv_all); a device position can reach the whole capacity
    const int kv_all = by_pos ? Skv : q_offset + Sq;
    if ((int64_t)kv_all * k->ss * 2 >= 0x7fffffffLL || (int64_t)kv_all * v->ss * 2 >= 0x7fffffffLL)
        return fail(-2, "%s: the visible K / V rows of one head must span less than 2 GiB", fn);
    const int64_t ncols = (int64_t)Sq * (shape->Hq / shape->Hkv);
    const int64_t bh = (int64_t)shape->B * shape->Hkv;
    if (ncols > 0x7fffffffLL / 2 || bh > 65535) return fail(-1, "%s: B * Hkv must stay within 65535 and Sq * G below 2^30", fn);
    DecArgs a;
    fill_dec_common(a, o, o->sb, o->ss, lse, workspace, shape, Sq, nsplit);
    a.q = tns(q); a.k = tns(k); a.v = tns(v);
    a.kmask = key_mask; a.kmask_ld = key_mask_ld;
    a.q_offset = by_pos ? 0 : q_offset;
    const int tiles = (kv_all + kKV - 1) / kKV;
    a.tps = (tiles + nsplit - 1) / nsplit;                 // by_pos: the kernel's own, from its position
    DecPosArgs ap;                                         // the device-position form of the same call
    static_cast<DecArgs&>(ap) = a;
    ap.pos = pos; ap.pos_stride = pos_stride; ap.cap = Skv;
    return launch_decode(a, ap, by_pos, shape, stream);
}

// Beam-shared cache: the shape (S is not used), the beam count and the fill levels. Host arithmetic only.
int check_beams(const char* fn, const smt_attn_shape* s, int32_t nb, int32_t P, int32_t T) {
    if (!s) return fail(-1, "%s: null shape", fn);
    if (s->B <= 0 || s->Hq <= 0 || s->Hkv <= 0 || s->Hq % s->Hkv)
        return fail(-1, "%s: bad shape B=%d Hq=%d Hkv=%d (Hq %% Hkv must be 0)", fn, s->B, s->Hq, s->Hkv);
    if (!(s->scale > 0.f)) return fail(-1, "%s: scale must be > 0", fn);
    if (s->dtype != SMT_DTYPE_BF16 && s->dtype != SMT_DTYPE_FP16)
        return fail(-1, "%s: dtype %d is not a 16-bit format (SMT_DTYPE_BF16 / SMT_DTYPE_FP16)", fn, (int)s->dtype);
    if (nb < 1) return fail(-1, "%s: nb = %d (at least one beam)", fn, (int)nb);
    if (P < 0) return fail(-1, "%s: P = %d is negative", fn, (int)P);
    if (T < 1) return fail(-1, "%s: T = %d (the current token's key is already in the cache)", fn, (int)T);
    if ((int64_t)nb * (s->Hq / s->Hkv) > 0x7fffffffLL / 2 || (int64_t)s->B * s->Hkv > 65535 ||
        (int64_t)s->B * nb > 0x7fffffffLL)
        return fail(-1, "%s: B * Hkv must stay within 65535, nb * G below 2^30 and B * nb below 2^31", fn);
    if ((int64_t)P / kKV + (int64_t)nb * ((int64_t)T / kKV + 1) > 0x3fffffffLL)
        return fail(-1, "%s: P = %d, nb = %d, T = %d make more than 2^30 tiles", fn, (int)P, (int)nb, (int)T);
    return 0;
}
int beam_col_blocks(const smt_attn_shape* s, int32_t nb) { return dec_col_blocks(s, nb); }
int beam_tiles(int32_t nb, int32_t P, int32_t T) { return (P + kKV - 1) / kKV + nb * ((T + kKV - 1) / kKV); }
// as dec_default_splits, over the tile list of one (sample, KV head)
int beam_default_splits(const smt_attn_shape* s, int32_t nb, int32_t P, int32_t T) {
    return default_splits((int64_t)s->B * s->Hkv * beam_col_blocks(s, nb), beam_tiles(nb, P, T));
}

// smt_attn_fwd_beams (by_pos false: T is the host's) and smt_attn_fwd_beams_pos (the kernel reads *steps;
// T is the capacity T_cap here, and the bounds, the default split count and the grid are taken on it).
int attn_fwd_beams(const char* fn, const smt_attn_tensor* q, const smt_attn_tensor* kp, const smt_attn_tensor* vp,
                   const smt_attn_tensor* kg, const smt_attn_tensor* vg, const smt_attn_tensor* o, float* lse,
                   const uint64_t* prompt_mask, int64_t prompt_mask_ld, const uint8_t* anc, int64_t anc_ld, int32_t nb,
                   int32_t P, int32_t P_cap, int32_t T, int32_t T_cap, const int32_t* steps, bool by_pos,
                   int32_t num_splits, void* workspace, const smt_attn_shape* shape, hipStream_t stream) {
    int rc;
    if ((rc = check_beams(fn, shape, nb, P, T)) || (rc = check_tensor(q, "q", fn)) || (rc = check_tensor(kg, "k_gen", fn)) ||
        (rc = check_tensor(vg, "v_gen", fn)) || (rc = check_tensor(o, "o", fn)))
        return rc;
    // the prompt segment may be absent (P == 0: its tensors are never touched, their ptr may be null)
    if (!kp || !vp) return fail(-1, "%s: null %s", fn, !kp ? "k_prompt" : "v_prompt");
    if (P > 0 && ((rc = check_tensor(kp, "k_prompt", fn)) || (rc = check_tensor(vp, "v_prompt", fn)))) return rc;
    if (!anc) return fail(-1, "%s: null anc", fn);
    if (P > P_cap) return fail(-1, "%s: P %d > P_cap %d", fn, (int)P, (int)P_cap);
    if (T > T_cap) return fail(-1, "%s: T %d > T_cap %d", fn, (int)T, (int)T_cap);
    if (by_pos && !steps) return fail(-1, "%s: null steps", fn);
    if (by_pos && (reinterpret_cast<uintptr_t>(steps) & 3u)) return fail(-2, "%s: steps needs 4-byte alignment (int32)", fn);
    if (anc_ld < T) return fail(-1, "%s: anc_ld %lld < %s %d", fn, (long long)anc_ld, by_pos ? "T_cap" : "T", (int)T);
    int nsplit;
    if ((rc = check_kmask_ld(fn, prompt_mask, prompt_mask_ld, P, "P")) ||
        (rc = check_splits(fn, num_splits, beam_default_splits(shape, nb, P, T), workspace, "smt_attn_beams_workspace", &nsplit)))
        return rc;
    // a tile's 64 rows are addressed with 32-bit byte offsets from the head's first row
    const auto span = [](int rows, int64_t ss) { return ((int64_t)rows + kKV) * ss * 2 >= 0x7fffffffLL; };
    if (P > 0 && (span(P, kp->ss) || span(P, vp->ss)))
        return fail(-2, "%s: the P rows of k_prompt / v_prompt of one head must span less than 2 GiB", fn);
    if (span(T, kg->ss) || span(T, vg->ss))
        return fail(-2, "%s: the T rows of k_gen / v_gen of one head must span less than 2 GiB", fn);
    BeamArgs a;
    fill_dec_common(a, o, o->sb * nb, o->sb, lse, workspace, shape, nb, nsplit);
    a.q = tns(q); a.q.ss = q->sb; a.q.sb = q->sb * nb;         // the beam as the "query position" of sample n
    a.k = P > 0 ? tns(kp) : Tns{nullptr, 0, 0, 0}; a.v = P > 0 ? tns(vp) : Tns{nullptr, 0, 0, 0};
    a.kg = tns(kg); a.vg = tns(vg);
    a.kmask = P > 0 ? prompt_mask : nullptr; a.kmask_ld = prompt_mask_ld;
    a.q_offset = 0;
    a.anc = anc; a.anc_ld = anc_ld;
    a.nb = nb; a.P = P; a.T = T;
    a.pt = (P + kKV - 1) / kKV; a.gt = (T + kKV - 1) / kKV;
    a.tps = (beam_tiles(nb, P, T) + nsplit - 1) / nsplit;
    BeamPosArgs ap;                                        // the device-counter form of the same call
    static_cast<BeamArgs&>(ap) = a;
    ap.steps = steps;
    return launch_decode(a, ap, by_pos, shape, stream);
}

}  // namespace

extern "C" {

const char* smt_attn_last_error(void) { return g_err; }


int smt_attn_fwd_kmask(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                       const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                       const smt_attn_shape* shape, hipStream_t stream) {
    return attn_fwd(key_mask ? "smt_attn_fwd_kmask" : "smt_attn_fwd", q, k, v, o, lse, own_ld(shape), key_mask,
                    key_mask_ld, kNoDrop, kNoDocs, shape, stream);
}

int smt_attn_fwd(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                 const smt_attn_tensor* o, float* lse, const smt_attn_shape* shape, hipStream_t stream) {
    return smt_attn_fwd_kmask(q, k, v, o, lse, nullptr, 0, shape, stream);
}

int smt_attn_bwd_kmask(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                       const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                       const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                       const uint64_t* key_mask, int64_t key_mask_ld, const smt_attn_shape* shape,
                       hipStream_t stream) {
    return attn_bwd(key_mask ? "smt_attn_bwd_kmask" : "smt_attn_bwd", q, k, v, o, d_o, lse, delta_ws,
                    own_ld(shape), dq, dk, dv, key_mask, key_mask_ld, kNoDrop, kNoDocs, shape, stream);
}

int smt_attn_bwd(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                 const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                 const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                 const smt_attn_shape* shape, hipStream_t stream) {
    return smt_attn_bwd_kmask(q, k, v, o, d_o, lse, delta_ws, dq, dk, dv, nullptr, 0, shape, stream);
}

int smt_attn_dropout_threshold(float p) { return drop_threshold(p); }

int smt_attn_fwd_dropout(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                         const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                         float p, const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream) {
    DropArgs drop;
    int rc;
    if ((rc = check_drop(p, seed, "smt_attn_fwd_dropout", &drop))) return rc;
    if (drop.t == 0) return smt_attn_fwd_kmask(q, k, v, o, lse, key_mask, key_mask_ld, shape, stream);
    return attn_fwd("smt_attn_fwd_dropout", q, k, v, o, lse, own_ld(shape), key_mask, key_mask_ld, drop, kNoDocs,
                    shape, stream);
}

int smt_attn_bwd_dropout(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                         const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                         const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                         const uint64_t* key_mask, int64_t key_mask_ld, float p, const uint64_t* seed,
                         const smt_attn_shape* shape, hipStream_t stream) {
    DropArgs drop;
    int rc;
    if ((rc = check_drop(p, seed, "smt_attn_bwd_dropout", &drop))) return rc;
    if (drop.t == 0)
        return smt_attn_bwd_kmask(q, k, v, o, d_o, lse, delta_ws, dq, dk, dv, key_mask, key_mask_ld, shape, stream);
    return attn_bwd("smt_attn_bwd_dropout", q, k, v, o, d_o, lse, delta_ws, own_ld(shape), dq, dk, dv, key_mask,
                    key_mask_ld, drop, kNoDocs, shape, stream);
}

int smt_attn_fwd_docs(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                      const smt_attn_tensor* o, float* lse, const int32_t* doc_start, const int32_t* doc_end, float p,
                      const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream) {
    const char* fn = "smt_attn_fwd_docs";
    if (!doc_start != !doc_end) return fail(-1, "%s: doc_start and doc_end come together (one is null)", fn);
    if (!doc_start) return smt_attn_fwd_dropout(q, k, v, o, lse, nullptr, 0, p, seed, shape, stream);
    DropArgs drop;
    int rc;
    if ((rc = check_drop(p, seed, fn, &drop))) return rc;
    return attn_fwd(fn, q, k, v, o, lse, own_ld(shape), nullptr, 0, drop, DocArgs{doc_start, doc_end}, shape, stream);
}

int smt_attn_bwd_docs(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                      const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                      const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                      const int32_t* doc_start, const int32_t* doc_end, float p, const uint64_t* seed,
                      const smt_attn_shape* shape, hipStream_t stream) {
    const char* fn = "smt_attn_bwd_docs";
    if (!doc_start != !doc_end) return fail(-1, "%s: doc_start and doc_end come together (one is null)", fn);
    if (!doc_start)
        return smt_attn_bwd_dropout(q, k, v, o, d_o, lse, delta_ws, dq, dk, dv, nullptr, 0, p, seed, shape, stream);
    DropArgs drop;
    int rc;
    if ((rc = check_drop(p, seed, fn, &drop))) return rc;
    return attn_bwd(fn, q, k, v, o, d_o, lse, delta_ws, own_ld(shape), dq, dk, dv, nullptr, 0, drop,
                    DocArgs{doc_start, doc_end}, shape, stream);
}

int smt_attn_fwd_ld(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                    const smt_attn_tensor* o, float* lse, int64_t lse_ld, const uint64_t* key_mask, int64_t key_mask_ld,
                    const int32_t* doc_start, const int32_t* doc_end, float p, const uint64_t* seed,
                    const smt_attn_shape* shape, hipStream_t stream) {
    const char* fn = "smt_attn_fwd_ld";
    DropArgs drop;
    int rc;
    if ((rc = check_ld(fn, lse_ld, key_mask, doc_start, doc_end, shape)) || (rc = check_drop(p, seed, fn, &drop))) return rc;
    return attn_fwd(fn, q, k, v, o, lse, lse_ld, key_mask, key_mask_ld, drop, DocArgs{doc_start, doc_end}, shape, stream);
}

int smt_attn_bwd_ld(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                    const smt_attn_tensor* o, const smt_attn_tensor* d_o, const float* lse, float* delta_ws,
                    int64_t lse_ld, const smt_attn_tensor* dq, const smt_attn_tensor* dk, const smt_attn_tensor* dv,
                    const uint64_t* key_mask, int64_t key_mask_ld, const int32_t* doc_start, const int32_t* doc_end,
                    float p, const uint64_t* seed, const smt_attn_shape* shape, hipStream_t stream) {
    const char* fn = "smt_attn_bwd_ld";
    DropArgs drop;
    int rc;
    if ((rc = check_ld(fn, lse_ld, key_mask, doc_start, doc_end, shape)) || (rc = check_drop(p, seed, fn, &drop))) return rc;
    return attn_bwd(fn, q, k, v, o, d_o, lse, delta_ws, lse_ld, dq, dk, dv, key_mask, key_mask_ld, drop,
                    DocArgs{doc_start, doc_end}, shape, stream);
}

int smt_attn_dropout_mask(uint8_t* keep, float p, const uint64_t* seed, const smt_attn_shape* shape,
                          hipStream_t stream) {
    const char* fn = "smt_attn_dropout_mask";
    DropArgs drop;
    int rc;
    if ((rc = check_drop(p, seed, fn, &drop)) || (rc = check_shape(shape, fn))) return rc;
    if (!keep) return fail(-1, "%s: null keep buffer", fn);
    const int64_t rows = (int64_t)shape->B * shape->Hq * shape->S;
    if (rows > 0xffffffffLL) return fail(-1, "%s: B * Hq * S must stay below 2^32", fn);
    if (drop.t == 0) {                                     // no dropout: every element is kept
        if (hipMemsetAsync(keep, 1, (size_t)rows * shape->S, stream) != hipSuccess)
            return fail(-4, "%s: hipMemsetAsync failed", fn);
        return 0;
    }
    const int64_t n_words = rows * ((shape->S + 3) / 4);
    const int64_t blocks = (n_words + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(-1, "%s: too many blocks", fn);
    hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, keep, drop, shape->S, n_words);
    return check_launch("attn_dropout_mask_kernel");
}

int smt_attn_cached_splits(const smt_attn_shape* shape, int32_t Sq) {
    const char* fn = "smt_attn_cached_splits";
    int rc;
    if ((rc = check_shape(shape, fn))) return rc;
    if (Sq < 1) return fail(-1, "%s: Sq = %d", fn, (int)Sq);
    return dec_default_splits(shape, Sq);
}

int64_t smt_attn_cached_workspace(const smt_attn_shape* shape, int32_t Sq, int32_t num_splits) {
    const char* fn = "smt_attn_cached_workspace";
    int rc;
    if ((rc = check_shape(shape, fn))) return rc;
    if (Sq < 1 || num_splits < 0) return fail(-1, "%s: Sq = %d, num_splits = %d", fn, (int)Sq, (int)num_splits);
    return dec_workspace(shape, Sq, num_splits ? num_splits : dec_default_splits(shape, Sq));
}

int smt_attn_fwd_cached(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                        const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                        int32_t Sq, int32_t q_offset, int32_t num_splits, void* workspace,
                        const smt_attn_shape* shape, hipStream_t stream) {
    return attn_fwd_cached("smt_attn_fwd_cached", q, k, v, o, lse, key_mask, key_mask_ld, Sq, q_offset, nullptr, 0, false,
                           num_splits, workspace, shape, stream);
}

int smt_attn_fwd_cached_pos(const smt_attn_tensor* q, const smt_attn_tensor* k, const smt_attn_tensor* v,
                            const smt_attn_tensor* o, float* lse, const uint64_t* key_mask, int64_t key_mask_ld,
                            int32_t Sq, const int64_t* positions, int32_t positions_stride, int32_t num_splits,
                            void* workspace, const smt_attn_shape* shape, hipStream_t stream) {
    return attn_fwd_cached("smt_attn_fwd_cached_pos", q, k, v, o, lse, key_mask, key_mask_ld, Sq, 0, positions,
                           positions_stride, true, num_splits, workspace, shape, stream);
}

int smt_attn_beams_splits(const smt_attn_shape* shape, int32_t nb, int32_t P, int32_t T) {
    int rc;
    if ((rc = check_beams("smt_attn_beams_splits", shape, nb, P, T))) return rc;
    return beam_default_splits(shape, nb, P, T);
}

int64_t smt_attn_beams_workspace(const smt_attn_shape* shape, int32_t nb, int32_t P, int32_t T, int32_t num_splits) {
    const char* fn = "smt_attn_beams_workspace";
    int rc;
    if ((rc = check_beams(fn, shape, nb, P, T))) return rc;
    if (num_splits < 0) return fail(-1, "%s: num_splits = %d is negative", fn, (int)num_splits);
    return dec_workspace(shape, nb, num_splits ? num_splits : beam_default_splits(shape, nb, P, T));
}

int smt_attn_fwd_beams(const smt_attn_tensor* q, const smt_attn_tensor* k_prompt, const smt_attn_tensor* v_prompt,
                       const smt_attn_tensor* k_gen, const smt_attn_tensor* v_gen, const smt_attn_tensor* o, float* lse,
                       const uint64_t* prompt_mask, int64_t prompt_mask_ld, const uint8_t* anc, int64_t anc_ld,
                       int32_t nb, int32_t P, int32_t P_cap, int32_t T, int32_t T_cap, int32_t num_splits,
                       void* workspace, const smt_attn_shape* shape, hipStream_t stream) {
    return attn_fwd_beams("smt_attn_fwd_beams", q, k_prompt, v_prompt, k_gen, v_gen, o, lse, prompt_mask, prompt_mask_ld,
                          anc, anc_ld, nb, P, P_cap, T, T_cap, nullptr, false, num_splits, workspace, shape, stream);
}

int smt_attn_fwd_beams_pos(const smt_attn_tensor* q, const smt_attn_tensor* k_prompt, const smt_attn_tensor* v_prompt,
                           const smt_attn_tensor* k_gen, const smt_attn_tensor* v_gen, const smt_attn_tensor* o, float* lse,
                           const uint64_t* prompt_mask, int64_t prompt_mask_ld, const uint8_t* anc, int64_t anc_ld,
                           int32_t nb, int32_t P, int32_t P_cap, const int32_t* steps, int32_t T_cap, int32_t num_splits,
                           void* workspace, const smt_attn_shape* shape, hipStream_t stream) {
    return attn_fwd_beams("smt_attn_fwd_beams_pos", q, k_prompt, v_prompt, k_gen, v_gen, o, lse, prompt_mask,
                          prompt_mask_ld, anc, anc_ld, nb, P, P_cap, T_cap, T_cap, steps, true, num_splits, workspace, shape,
                          stream);
}

int smt_attn_kv_append_pos(const smt_attn_tensor* k_new, const smt_attn_tensor* v_new, const smt_attn_tensor* k_gen,
                           const smt_attn_tensor* v_gen, const int32_t* steps, int32_t rows, int32_t Hkv, int32_t T_cap,
                           int32_t dtype, hipStream_t stream) {
    const char* fn = "smt_attn_kv_append_pos";
    int rc;
    if ((rc = check_tensor(k_new, "k_new", fn)) || (rc = check_tensor(v_new, "v_new", fn)) ||
        (rc = check_tensor(k_gen, "k_gen", fn)) || (rc = check_tensor(v_gen, "v_gen", fn)))
        return rc;
    if (!steps) return fail(-1, "%s: null steps", fn);
    if (reinterpret_cast<uintptr_t>(steps) & 3u) return fail(-2, "%s: steps needs 4-byte alignment (int32)", fn);
    if (dtype != SMT_DTYPE_BF16 && dtype != SMT_DTYPE_FP16)
        return fail(-1, "%s: dtype %d is not a 16-bit format (SMT_DTYPE_BF16 / SMT_DTYPE_FP16)", fn, (int)dtype);
    if (rows < 1 || Hkv < 1 || T_cap < 1)
        return fail(-1, "%s: rows = %d, Hkv = %d, T_cap = %d (each at least 1)", fn, (int)rows, (int)Hkv, (int)T_cap);
    const int64_t n = (int64_t)rows * Hkv * 2 * (kD / 8);      // one 16-byte piece per thread
    if (n > 0x7fffffffLL) return fail(-1, "%s: rows * Hkv = %lld is too large", fn, (long long)rows * Hkv);
    AppendArgs a;
    a.kn = tns(k_new); a.vn = tns(v_new); a.kg = tns(k_gen); a.vg = tns(v_gen);
    a.steps = steps; a.Hkv = Hkv; a.cap = T_cap; a.n = (int)n;
    hipLaunchKernelGGL(attn_kv_append_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    return check_launch("attn_kv_append_kernel");
}

}  // extern "C"
