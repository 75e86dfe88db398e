"""Bit-exact references for the tile weight-gradient kernels of ``csrc/smt_kernels.hip``
(``wgrad_quarter_kernel``, ``wgrad_dma_kernel``, ``wgrad_partial_kernel``, ``wgrad_f32_kernel``, the slab
reduces, ``wgrad_mx_kernel`` / ``wgrad_mx_quarter_kernel``; tests/test_gpu_wgrad_exact.py,
tests/test_wgrad_ref_host.py). CPU only.

Why bits and not a norm
-----------------------
A tile is C[m][n] = sum_t g[t][256 r + m] x[t][256 c + n]. On random data the fp32 sums of the CPU and of
the MFMA differ in order, roundings flip, and a test can only bound a norm: a wrong rounding mode, a double
rounding or a few hundred wrong elements hide inside the 1.2e-3 of the 16-bit output rounding. On operands
that are whole multiples of one power of two (``UNIT``; 1 for bf16 and fp32, 1/8 for fp16) every product is a
whole multiple of ``UNIT^2`` and, as long as sum_t |g x| < 2^24 UNIT^2, so is every fp32 partial sum *in any
order*: nothing rounds before the kernel's own roundings, and the whole pipeline is predictable bit for bit.

    single rounding     (``single``)              RNE_out(sum over all T + base)
    reference rounding  (``reference_rounding``)  v = RNE_op(sum over samples of RNE_op(sum over the sample));
                                                  16-bit out: RNE_out(base + v), fp32 out: base + v
                                                  (``wgrad_reduce_tile``; smt.py:397-404 and autograd's add)

RNE_op is the identity for fp32 operands. Every reference asserts its precondition: sum_t |g x| (and
|base| on top of it) below 2^24 units, and no 16-bit value beyond the format's largest finite one.

The operands (``int_operands``)
-------------------------------
g and x are independent uniform integers in [-amp, amp] times ``UNIT``; g's row block 1 is scaled by 2 and
x's last column block by 4, so that no two tiles of a matrix are alike and a swapped or transposed block
cannot cancel. amp is 15 for bf16 and fp32 (8 significand bits: a sum rounds from 256 on). fp16 has 11
significand bits and overflows at 65504: whole numbers round from 2048 on, a window of 2^5 between "rounds"
and "overflows" that cannot hold the 8-fold spread of the tile scalings, the sqrt(B) growth of the sample
sum and the tail of the largest element at once. The rounding of a binary format does not depend on a
common power of two, so the fp16 operands are the integers of amp 63 times 1/8: a sum rounds from 32 on and
the window is 2^11 wide. With amp 3, what the older layout test uses, nothing ever rounds: the amplitude
matters.

Measured on the CPU (``python -m tests.wgrad_ref``), per (B, seq) of the reference-rounding cases on the
tiles ``TILES[3]`` (scalings 4, 2, 1): share of per-sample partials / of sample sums that are inexact before
their rounding, share of elements where "round once at the end" differs from the two roundings, largest
|value| relative to 65504 (fp16) or to 2^24 (bf16)

                bf16 (amp 15)                 fp16 (amp 63, unit 1/8)
    3 x 100     0.53 0.54 0.36  max 0.0014    0.71 0.58 0.38  max 0.11
    3 x 33      0.36 0.47 0.33  max 0.0009    0.58 0.55 0.37  max 0.06
    2 x 200     0.62 0.46 0.33  max 0.0021    0.77 0.49 0.35  max 0.11
    9 x 64      0.46 0.73 0.41  max 0.0021    0.66 0.81 0.41  max 0.14
    5 x 64      0.46 0.64 0.39  max 0.0015    0.66 0.71 0.40  max 0.10

tests/test_wgrad_ref_host.py asserts >= 0.30 for the first two shares at every case's own tiles. On these
inputs ``reference_rounding`` equals ``oracle.linearz_tile_grads`` bit for bit and ``single`` in fp64 equals
``oracle.tile_grads_fp64`` (the same file): the references here are the oracle's.

Mutations (``MUTATIONS``): smallest share of the elements of the output it touches that a planted error
changes, over every case of the GPU file that relies on it (``mutation_applies``), 16-bit out, with a base
(tests/test_wgrad_ref_host.py asserts >= 0.01 at each case, for both output dtypes, with and without a base):

    one rounding instead of two 0.13     round-half-away 0.04      truncation 0.26
    sample boundary shifted by a row 0.15   one row past T 1.00     last row dropped 0.83
    tile transposed 0.99   (r, c) swapped 0.50 (one of two tiles is (2, 2))   base dropped 0.99
    base before the final rounding 0.08     two tiles exchanged 1.00

A single-rounding case has no sample boundary and one rounding only, an fp32 output of a single-rounding
case rounds nothing, fp32 operands round nothing at all, sums over fewer than 31 rows are exact in 16 bits,
"base" needs ``accumulate`` and an exchange two tiles: ``mutation_applies`` says which case can see which
mutation, and the GPU file counts on a case for a mutation only there.

The MX pair (``mx_int_operands``)
---------------------------------
Integers in [-7, 7] with power-of-two scalings per 256-column block and per 32-row group: e4m3 with one
shared exponent per 32 rows holds them without loss, so the truth of ``tile_wgrad_mx`` is ``single`` on the
bf16 operands. A column block of g is scaled by 8: products reach 392 and the sums the thousands, so the
bf16 output rounding is exercised.

Random data (``random_operands``, ``random_bound``)
--------------------------------------------------
Integers leave the low significand bits of the operands zero. One tier runs Gaussian operands (g * 1e-2,
x * 1, a few bf16 subnormals) with fp32 out against the fp64 truth, every element inside

    |out - truth| <= (T + S) 2^-24 sum_t |g_t x_t| + half an fp32 step at the truth

the first-order bound of T round-to-nearest additions in any order plus S - 1 slab additions (S splits of
T, from the workspace-size functions) and the rounding of the result. The f32 MFMA is an fmaf chain (one
rounding per term) and is held to this bound as it stands. How the bf16 / f16 MFMA rounds its internal
sums is not documented; ``RANDOM_ALLOWANCE`` is the whole multiple of the bound a 16-bit kernel is held to.

Measured on an MI355X (tests/test_gpu_wgrad_exact.py with ``WGRAD_REF_REPORT=1`` and ``-s``): largest
|error| / bound over every element

                          bf16 operands   fp16 operands   fp32 operands (wgrad_f32_kernel)
    quarter, direct       0.005           0.005           0.018
    quarter, S = 3 slabs  0.001           0.001           0.002
    full tile, direct     0.006           0.006           0.017
    full tile, S = 3      0.001           0.001           0.002

The bound is the worst case of T roundings all of one sign; the errors of a sum of mixed signs grow like
sqrt(T), hence the small ratios. Every kernel is far inside, so no allowance was needed: all three are 1.
"""
from __future__ import annotations

from typing import Optional

import torch

BLOCK = 256
F64 = torch.float64
# operands are whole multiples of UNIT[dtype] (module docstring); a product of two, of UNIT^2
UNIT = {torch.bfloat16: 1.0, torch.float32: 1.0, torch.float16: 0.125}
AMP = {torch.bfloat16: 15, torch.float32: 15, torch.float16: 63}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}
POISON = 96.0                            # the rows after T of an operand buffer; exact in bf16 / fp16 / fp32
G_SCALED_BLOCK, G_SCALE, X_SCALE = 1, 2.0, 4.0

# ------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_wgrad_exact.py (shared with tests/test_wgrad_ref_host.py)
# ------------------------------------------------------------------------------------------------
OUT_F, IN_F = 1024, 768                  # g [T, 1024], x [T, 768]: 4 x 3 tiles
# tile lists per n, never in table order of the matrix; scalings of the first three: 4, 2, 1
TILES = {
    1: [(1, 2)],
    2: [(2, 2), (1, 0)],
    3: [(2, 2), (1, 0), (0, 1)],
    9: [(0, 2), (2, 0), (1, 1), (3, 2), (0, 0), (1, 2), (2, 1), (3, 1), (1, 0)],
}
# single rounding: id -> (n tiles, T)
SINGLE_CASES = {
    "quarter-direct": (3, 300),
    "quarter-slabs-S3": (2, 1100),
    "full-direct": (9, 300),
    "full-slabs-S3": (9, 1100),
}
EDGE_T = [1, 31, 33, 64, 65]             # stage edges of the 32- and 64-row pipelines, n = 1 and 9
# reference rounding: id -> (n tiles, B, seq)
SEQ_CASES = {
    "quarter-kps1-3x100": (3, 3, 100),
    "quarter-kps1-3x33": (3, 3, 33),
    "quarter-kps2-2x200": (1, 2, 200),
    "full-kps1-3x100": (9, 3, 100),
    "full-kps2-2x200": (9, 2, 200),
    "reduce-unroll-9x64": (3, 9, 64),
    "reduce-unroll-5x64": (3, 5, 64),
}
# the rows fp32 operands run on (wgrad_f32_kernel: one direct, one slab, one kps = 1, one kps = 2)
F32_SINGLE = ["quarter-direct", "quarter-slabs-S3"]
F32_SEQ = ["quarter-kps1-3x100", "quarter-kps2-2x200"]


def seed_of(*key) -> int:
    """A fixed seed per case (no ``hash``: it is salted per process)."""
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def int_operands(T: int, out_f: int, in_f: int, dtype: torch.dtype, seed: int, amp: Optional[int] = None):
    """``(g [T, out_f], x [T, in_f])`` in ``dtype``: independent uniform integers in [-amp, amp] times
    ``UNIT[dtype]``; g's row block 1 (columns 256..511 of g) times 2, x's last column block times 4."""
    amp = AMP[dtype] if amp is None else amp
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-amp, amp + 1, (T, out_f), generator=gen).to(F64)
    x = torch.randint(-amp, amp + 1, (T, in_f), generator=gen).to(F64)
    if out_f >= 2 * BLOCK:
        g[:, G_SCALED_BLOCK * BLOCK:(G_SCALED_BLOCK + 1) * BLOCK] *= G_SCALE
    x[:, in_f - BLOCK:] *= X_SCALE
    g, x = g * UNIT[dtype], x * UNIT[dtype]
    gd, xd = g.to(dtype), x.to(dtype)
    assert torch.equal(gd.to(F64), g) and torch.equal(xd.to(F64), x), "operands not exact in their dtype"
    return gd, xd


def int_base(n_tiles: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """An ``accumulate`` base [n * 256, 256]: 16 k units of a product, k uniform in [-127, 127]: exact in every
    dtype, and of the size of the sums, so that it moves their rounding."""
    gen = torch.Generator().manual_seed(seed + 7919)
    k = torch.randint(-127, 128, (n_tiles * BLOCK, BLOCK), generator=gen).to(F64)
    return k * 64.0 * UNIT[dtype] ** 2


def mx_int_operands(T: int, out_f: int, in_f: int, seed: int):
    """bf16 ``(g, x)`` that MX e4m3 (one e8m0 exponent per 32 rows of a column) holds without loss: integers in
    [-7, 7]; g's column block 1 times 8 (products to 392), its block 2 (if any) times 1/2, x's rows 32..63 of
    every 128 times 1/4."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-7, 8, (T, out_f), generator=gen).to(F64)
    x = torch.randint(-7, 8, (T, in_f), generator=gen).to(F64)
    g[:, BLOCK:2 * BLOCK] *= 8.0
    g[:, 2 * BLOCK:3 * BLOCK] *= 0.5
    rows = torch.arange(T)
    x[(rows % 128 >= 32) & (rows % 128 < 64)] *= 0.25
    gd, xd = g.bfloat16(), x.bfloat16()
    assert torch.equal(gd.to(F64), g) and torch.equal(xd.to(F64), x)
    return gd, xd


MX_UNIT2 = 0.5 * 0.25                    # the grid of an MX product


def random_operands(T: int, out_f: int, in_f: int, dtype: torch.dtype, seed: int):
    """Gaussian ``(g * 1e-2, x)`` in ``dtype`` with a few bf16 subnormals (1e-40 scale) planted in both."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(T, out_f, generator=gen) * 1e-2
    x = torch.randn(T, in_f, generator=gen)
    if dtype != torch.float16:           # below fp16's smallest subnormal
        for t, idx in ((g, 5), (x, 11)):
            flat = t.view(-1)
            flat[idx::997] = flat[idx::997].sign() * 3e-40
    return g.to(dtype), x.to(dtype)


def random_bound(g, x, tiles, T: int, S: int):
    """``(truth, bound)`` in fp64 for fp32 out: (T + S) 2^-24 sum_t |g x| + half an fp32 step at the truth."""
    truth = _exact(g.to(F64), x.to(F64), tiles)
    mag = _exact(g.to(F64).abs(), x.to(F64).abs(), tiles)
    _, e = torch.frexp(truth)
    half_step = torch.ldexp(torch.ones_like(truth), (e - 24).clamp(min=-149)) * 0.5
    return truth, (T + S) * 2.0 ** -24 * mag + half_step


RANDOM_ALLOWANCE = {torch.bfloat16: 1, torch.float16: 1, torch.float32: 1}


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _exact(g, x, tiles, swap_rc=False):
    """fp64 [n, 256, 256]: sum_t g[t, r-block]^T x[t, c-block] (exact on the grids above)."""
    out = torch.empty(len(tiles), BLOCK, BLOCK, dtype=F64)
    for i, (r, c) in enumerate(tiles):
        if swap_rc:
            r, c = c, r
        out[i] = g[:, r * BLOCK:(r + 1) * BLOCK].t() @ x[:, c * BLOCK:(c + 1) * BLOCK]
    return out + 0.0            # a sum starts from +0.0: a lone product -0.0 (T = 1) ends as +0.0, as in the kernels


def round_to(v: torch.Tensor, dtype: torch.dtype, mode: str = "even") -> torch.Tensor:
    """fp64 ``v`` rounded to the significand of ``dtype`` (normal range), ties to even / away, or truncated."""
    if dtype == F64:
        return v
    m, e = torch.frexp(v)                                          # v = m 2^e, |m| in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(v), e - SIG_BITS[dtype])
    q = v / ulp
    if mode == "even":
        q = torch.round(q)
    elif mode == "away":
        q = torch.sign(q) * torch.floor(q.abs() + 0.5)
    else:
        q = torch.trunc(q)
    return q * ulp


def _check_exact(mag: torch.Tensor, unit2: float, what: str):
    top = float(mag.max()) / unit2 if mag.numel() else 0.0
    assert top < 2.0 ** 24, f"{what}: sum |g x| reaches {top:.3g} units: not exact in fp32"


def _check_finite16(v: torch.Tensor, dtype: torch.dtype, what: str):
    if dtype in (torch.bfloat16, torch.float16) and v.numel():
        assert float(v.abs().max()) <= torch.finfo(dtype).max, f"{what}: overflows {dtype}"


def _unit2(dtype, unit2):
    return UNIT[dtype] ** 2 if unit2 is None else unit2


MUTATIONS = ("one_rounding", "half_away", "truncate", "boundary_shift", "row_past_T", "last_row_dropped",
             "transposed", "rc_swapped", "base_dropped", "base_before_rounding", "tiles_exchanged")


def _restate(g, x, T, seq, tiles, op_dtype, out_dtype, base, mutate, unit2):
    """The one restatement behind ``single`` (seq = 0) and ``reference_rounding``: fp64 [n * 256, 256] holding
    values of ``out_dtype``. ``g`` / ``x`` may be taller than T (the buffer's poison rows: ``row_past_T``)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    G, X = g.to(F64), x.to(F64)
    assert mutate != "row_past_T" or G.shape[0] > T
    t_end = T + 1 if mutate == "row_past_T" else T - 1 if mutate == "last_row_dropped" else T
    mode = {"half_away": "away", "truncate": "trunc"}.get(mutate, "even")
    unit2 = _unit2(op_dtype, unit2)
    _check_exact(_exact(G[:T].abs(), X[:T].abs(), tiles) + (0 if base is None else base.to(F64).abs().view(-1, BLOCK, BLOCK)),
                 unit2, "wgrad_ref")
    swap = mutate == "rc_swapped"
    b = None if base is None or mutate == "base_dropped" else base.to(F64).view(-1, BLOCK, BLOCK)
    if not seq:
        v = _exact(G[:t_end], X[:t_end], tiles, swap)
        if b is not None:
            v = v + b
        out = round_to(v, out_dtype, mode)
    else:
        assert T % seq == 0
        shift = 1 if mutate == "boundary_shift" else 0
        cuts = [0] + [k * seq + shift for k in range(1, T // seq)] + [t_end]
        total = torch.zeros(len(tiles), BLOCK, BLOCK, dtype=F64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = _exact(G[lo:hi], X[lo:hi], tiles, swap)
            if mutate != "one_rounding":
                part = round_to(part, op_dtype, mode)
                _check_finite16(part, op_dtype, "a per-sample partial")
            total += part                                          # exact: whole units below 2^24
        v = round_to(total, op_dtype, mode)
        _check_finite16(v, op_dtype, "the sample sum")
        if b is None:
            out = v
        elif out_dtype == torch.float32:
            out = v + b
        elif mutate == "base_before_rounding":
            out = round_to(total + b, out_dtype, mode)              # the sum's own rounding skipped
        else:
            out = round_to(v + b, out_dtype, mode)
    _check_finite16(out, out_dtype, "the output")
    if mutate == "transposed":
        out = out.transpose(1, 2).contiguous()
    if mutate == "tiles_exchanged":
        assert len(tiles) >= 2
        out = out[[1, 0] + list(range(2, len(tiles)))]
    return out.reshape(-1, BLOCK)


def single(g, x, tiles, out_dtype, base=None, mutate=None, T=None, unit2=None) -> torch.Tensor:
    """One rounding: RNE_out(the exact sum over all T rows + base). fp64 [n * 256, 256] of ``out_dtype`` values;
    ``out_dtype`` fp64: the exact sum itself."""
    T = g.shape[0] if T is None else T
    return _restate(g, x, T, 0, tiles, g.dtype, out_dtype, base, mutate, unit2)


def reference_rounding(g, x, seq, tiles, op_dtype, out_dtype, base=None, mutate=None, T=None) -> torch.Tensor:
    """The reference's rounding (smt.py:397-404, ``smt_tile_wgrad_batch_seq``): see the module docstring."""
    T = g.shape[0] if T is None else T
    assert g.dtype == op_dtype and x.dtype == op_dtype
    return _restate(g, x, T, seq, tiles, op_dtype, out_dtype, base, mutate, None)


def mutation_applies(mutation: str, seq: int, T: int, op_dtype, out_dtype, has_base: bool, n_tiles: int) -> bool:
    """Whether a case of the GPU file can see ``mutation`` at all (module docstring)."""
    op16, out16 = op_dtype != torch.float32, out_dtype != torch.float32
    if mutation in ("half_away", "truncate"):
        return op16 and (bool(seq) or out16) and T >= 31     # shorter sums are exact in 16 bits
    if mutation == "one_rounding":
        return op16 and bool(seq)
    if mutation == "boundary_shift":
        return op16 and bool(seq)                   # fp32 operands: nothing rounds at a boundary
    if mutation == "base_dropped":
        return has_base
    if mutation == "base_before_rounding":
        return has_base and bool(seq) and out16
    if mutation == "tiles_exchanged":
        return n_tiles >= 2
    return True


def to_dtype(ref64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """A reference (fp64 holding values of ``dtype``) as a ``dtype`` tensor; the conversion must be exact."""
    out = ref64.to(torch.float32).to(dtype)
    assert torch.equal(out.to(F64), ref64), "reference values are not values of " + str(dtype)
    return out


def pad_rows(t: torch.Tensor, extra: int = 64) -> torch.Tensor:
    """``t`` with ``extra`` poison rows below it (what the GPU file's operand buffers hold after T)."""
    return torch.cat([t, torch.full((extra, t.shape[1]), POISON, dtype=t.dtype)])


def inexact_share(v: torch.Tensor, dtype: torch.dtype) -> float:
    return float((round_to(v, dtype) != v).double().mean())


# ------------------------------------------------------------------------------------------------
# the measurements quoted above
# ------------------------------------------------------------------------------------------------
def seq_shares(B: int, seq: int, dtype, tiles=None):
    """(share of inexact per-sample partials, of inexact sample sums, of elements where one rounding differs
    from two, largest |value| / the format's largest finite one) on the case's operands."""
    tiles = TILES[3] if tiles is None else tiles
    T = B * seq
    g, x = int_operands(T, OUT_F, IN_F, dtype, seed_of("seq", B, seq, dtype))
    G, X = g.to(F64), x.to(F64)
    parts = torch.stack([_exact(G[b * seq:(b + 1) * seq], X[b * seq:(b + 1) * seq], tiles) for b in range(B)])
    sums = round_to(parts, dtype).sum(0)
    two = reference_rounding(g, x, seq, tiles, dtype, dtype)
    one = reference_rounding(g, x, seq, tiles, dtype, dtype, mutate="one_rounding")
    top = max(float(parts.abs().max()), float(sums.abs().max()))
    limit = torch.finfo(dtype).max if dtype == torch.float16 else 2.0 ** 24
    return inexact_share(parts, dtype), inexact_share(sums, dtype), float((one != two).double().mean()), top / limit


def mutation_share(mutation, g, x, T, seq, tiles, op_dtype, out_dtype, base) -> float:
    """Share of the touched output's elements that ``mutation`` changes (``g`` / ``x`` carry poison rows)."""
    if seq:
        good = reference_rounding(g, x, seq, tiles, op_dtype, out_dtype, base, T=T)
        bad = reference_rounding(g, x, seq, tiles, op_dtype, out_dtype, base, mutate=mutation, T=T)
    else:
        good = single(g, x, tiles, out_dtype, base, T=T)
        bad = single(g, x, tiles, out_dtype, base, mutate=mutation, T=T)
    if mutation == "tiles_exchanged":                              # it touches the first two tiles only
        good, bad = good[:2 * BLOCK], bad[:2 * BLOCK]
    return float((good != bad).double().mean())


def host_cases():
    """Every (id, seq, T, n) of the GPU file's integer cases."""
    for cid, (n, T) in SINGLE_CASES.items():
        yield cid, 0, T, n
    for T in EDGE_T:
        for n in (1, 9):
            yield f"edge-T{T}-n{n}", 0, T, n
    for cid, (n, B, seq) in SEQ_CASES.items():
        yield cid, seq, B * seq, n


def case_dtypes(cid: str):
    f32 = cid in F32_SINGLE or cid in F32_SEQ
    return [torch.bfloat16, torch.float16] + ([torch.float32] if f32 else [])


def _measure():
    for B, seq in dict.fromkeys((B, seq) for _, B, seq in SEQ_CASES.values()):
        row = []
        for dt in (torch.bfloat16, torch.float16):
            a, b, c, top = seq_shares(B, seq, dt)
            row.append(f"{str(dt)[6:]}: partials {a:.2f} sums {b:.2f} one-vs-two {c:.2f} max {top:.2g}")
        print(f"{B} x {seq}: " + "   ".join(row))
    worst = {}
    for cid, seq, T, n in host_cases():
        tiles = TILES[n][:3]
        for dt in case_dtypes(cid):
            g, x = int_operands(T, OUT_F, IN_F, dt, seed_of(cid, dt))
            gp, xp = pad_rows(g), pad_rows(x)
            base = int_base(len(tiles), dt, seed_of(cid, dt))
            for out_dt in (dt, torch.float32):
                for mut in MUTATIONS:
                    if out_dt == torch.float32 or not mutation_applies(mut, seq, T, dt, out_dt, True, len(tiles)):
                        continue
                    s = mutation_share(mut, gp, xp, T, seq, tiles, dt, out_dt, base)
                    if s < worst.get(mut, (2.0,))[0]:
                        worst[mut] = (s, cid, dt)
    for mut, (s, cid, dt) in worst.items():
        print(f"mutation {mut}: smallest share {s:.3f} ({cid}, {dt})")


if __name__ == "__main__":
    _measure()
