"""The e4m3 quantisation of the fp8 path restated on the CPU (tests/test_fp8_ref_host.py,
tests/test_gpu_fp8_exact.py), independent of torch's converter and of the device.

OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; subnormals step 2^-9; no infinity; the
all-ones code 0x7F / 0xFF is NaN, so the largest value is 0x7E = 448. Encoding rounds to nearest,
ties to even; whatever rounds above 448 becomes 0x7F (as torch does; the kernels clamp to +-448
first, so they never produce it from a finite row); the sign of zero is kept.

The contract of csrc/fp8_math.h, per row (or column) of bf16 values:

    scale = RN32(amax * fp32(1/448)), 1 when amax == 0
    byte  = e4m3_encode(RN32(x / scale))

Everything here is integer arithmetic on the bits, or fp64 arithmetic that is exact for fp32
operands (a product has 48 bits; a quotient rounded to fp64 and then to fp32 is the correctly
rounded fp32 quotient because 53 >= 2 * 24 + 2), rounded to fp32 once. ``RN32`` is numpy's
fp64 -> fp32 conversion, which rounds to nearest even and keeps subnormals (test_fp8_ref_host.py pins that).

The functions take and return numpy arrays: bf16 values as their uint16 bit patterns (``bf16_bits``
turns a torch bf16 tensor into them), bytes as uint8, scales as float32.

The second half of the file builds the inputs of tests/test_gpu_fp8_exact.py, so that
tests/test_fp8_ref_host.py can show on the very same inputs that a wrong quantiser would be seen.
"""
from __future__ import annotations

import functools

import numpy as np

E4M3_MAX = 448.0
INV_E4M3_MAX = np.float32(1.0 / 448.0)            # fp64 1/448 rounded once to fp32 == 1.f / 448.f


# ----------------------------------------------------------------------------- bits and formats

def bf16_bits(t) -> np.ndarray:
    """uint16 bit patterns of a torch bf16 tensor (CPU or device)."""
    import torch
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def bits_to_bf16(bits: np.ndarray):
    """torch bf16 tensor (CPU) with these uint16 bit patterns."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def e4m3_decode(codes) -> np.ndarray:
    """fp64 value of each e4m3fn byte (NaN for 0x7F / 0xFF)."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    sign = np.where(c & 0x80, -1.0, 1.0)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2((e - 10).astype(np.float64)))
    return np.where((c & 0x7F) == 0x7F, np.nan, sign * mag)


def e4m3_encode(v, rounding: str = "rne", subnormals: bool = True, zero_sign: bool = True) -> np.ndarray:
    """e4m3fn byte of each fp32 value. ``rounding``: "rne" (the format), or the mutants "rtz" (toward
    zero) and "away" (ties away from zero); ``subnormals=False`` flushes e4m3 subnormals to zero and
    ``zero_sign=False`` drops the sign of a zero result (mutants as well)."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    sign = ((bits >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint8)
    mag = (bits & np.uint32(0x7FFFFFFF)).astype(np.int64)
    e = mag >> 23
    sig = np.where(e > 0, (mag & 0x7FFFFF) | 0x800000, 0)           # fp32 subnormals are < 2^-126: zero
    # value = sig * 2^(e - 150). Normal e4m3 (e >= 121, value >= 2^-6): keep 4 significant bits, drop
    # 20; below, the step is 2^-9: drop 141 - e bits (everything once that exceeds 25)
    sh = np.clip(np.maximum(20, 141 - e), 20, 40)
    q = sig >> sh
    rem = sig & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    if rounding == "rne":
        up = (rem > half) | ((rem == half) & ((q & 1) == 1))
    elif rounding == "away":
        up = rem >= half
    elif rounding == "rtz":
        up = np.zeros_like(rem, dtype=bool)
    else:
        raise ValueError(rounding)
    code = (np.maximum(e - 121, 0) << 3) + q + up                  # a carry out of the mantissa lands in the exponent
    if not subnormals:
        code = np.where(code < 8, 0, code)
    code = np.where((code > 0x7E) | (e == 255), 0x7F, code).astype(np.uint8)
    if not zero_sign:
        sign = np.where(code == 0, np.uint8(0), sign)
    return code | sign


def rn32(v64) -> np.ndarray:
    """fp64 -> fp32, round to nearest even, subnormals kept."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v64, dtype=np.float64).astype(np.float32)


def row_scale(amax) -> np.ndarray:
    """RN32(amax * fp32(1/448)); 1 for amax == 0."""
    a = np.asarray(amax, dtype=np.float32).astype(np.float64)
    return np.where(a > 0, rn32(a * np.float64(INV_E4M3_MAX)), np.float32(1.0)).astype(np.float32)


def row_scale_true_division(amax) -> np.ndarray:
    """Mutant: RN32(amax / 448)."""
    a = np.asarray(amax, dtype=np.float32).astype(np.float64)
    return np.where(a > 0, rn32(a / 448.0), np.float32(1.0)).astype(np.float32)


def quotient(x, scale) -> np.ndarray:
    """The correctly rounded fp32 quotient x / scale (fp32 operands)."""
    with np.errstate(all="ignore"):
        return rn32(np.asarray(x, dtype=np.float32).astype(np.float64) /
                    np.asarray(scale, dtype=np.float32).astype(np.float64))


def quotient_uncorrected(x, scale) -> np.ndarray:
    """Mutant: RN32(x * RN32(1 / scale)), the reciprocal multiply without the Markstein step."""
    with np.errstate(all="ignore"):
        rs = rn32(1.0 / np.asarray(scale, dtype=np.float32).astype(np.float64))
        return rn32(np.asarray(x, dtype=np.float32).astype(np.float64) * rs.astype(np.float64))


def _abs_f32(bits: np.ndarray) -> np.ndarray:
    return bf16_to_f32(np.asarray(bits, dtype=np.uint16) & np.uint16(0x7FFF))


def quant_rows(x_bits, *, amax=None, encode=e4m3_encode, scale_of=row_scale, quot=quotient):
    """Per-row quantisation of bf16 ``[rows, cols]`` (bit patterns): ``(bytes uint8, scales float32)``.
    ``amax`` overrides the row maxima (the callers below; the mutants)."""
    x_bits = np.asarray(x_bits, dtype=np.uint16)
    if amax is None:
        amax = _abs_f32(x_bits).max(axis=1)
    scale = scale_of(amax)
    return encode(quot(bf16_to_f32(x_bits), scale[:, None])), scale


def quant_rows_cat(parts, *, skip_source=None, **kw):
    """Per-row quantisation of the concatenation of bf16 parts, one scale per row over all of them
    (``skip_source``: the mutant whose amax leaves that source out)."""
    parts = [np.asarray(p, dtype=np.uint16) for p in parts]
    amax = np.max([_abs_f32(p).max(axis=1) for k, p in enumerate(parts) if k != skip_source], axis=0)
    return quant_rows(np.concatenate(parts, axis=1), amax=amax, **kw)


def quant_cols_t(w_bits, *, skip_segment=None, **kw):
    """Per-column quantisation of bf16 ``[rows, cols]``, written transposed: ``(bytes [cols, rows],
    scales [cols])`` (``skip_segment``: the mutant whose amax leaves that 256-row segment out)."""
    w_bits = np.asarray(w_bits, dtype=np.uint16)
    a = _abs_f32(w_bits)
    if skip_segment is not None:
        a = a.copy()
        a[256 * skip_segment:256 * (skip_segment + 1)] = 0
    return quant_rows(np.ascontiguousarray(w_bits.T), amax=a.max(axis=0), **kw)


def dequant(q, s) -> np.ndarray:
    """fp64 ``decode(q) * s`` with one scale per row of q."""
    return e4m3_decode(q) * np.asarray(s, dtype=np.float32).astype(np.float64)[:, None]


# ----------------------------------------------------------------------------- the comparer

def compare_bits(got, want, what="bytes", x_bits=None, scales=None, limit=1):
    """``None`` when ``got`` and ``want`` agree on every bit, else the report: the number of differing
    elements and, for the first ones, position, input value, scale, got and want."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (got.shape, want.shape)
    itype = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    g, w = got.view(itype), want.view(itype)
    bad = np.argwhere(g != w)
    if len(bad) == 0:
        return None
    lines = [f"{what}: {len(bad)} of {g.size} elements differ"]
    for pos in bad[:limit]:
        pos = tuple(int(p) for p in pos)
        line = f"  at {pos}: got 0x{int(g[pos]):x} want 0x{int(w[pos]):x}"
        if got.dtype == np.float32:
            line += f" ({got[pos]!r} vs {want[pos]!r})"
        if x_bits is not None and x_bits.shape == got.shape:
            line += f", x = {float(bf16_to_f32(x_bits[pos])):.9g} (0x{int(x_bits[pos]):04x})"
        if scales is not None:
            line += f", scale = {float(np.asarray(scales)[pos[0]]):.9g}"
        lines.append(line)
    return "\n".join(lines)


# ----------------------------------------------------------------------------- inputs of the GPU tests

# Binades (exponent of the bf16 amax) of the value-domain test, 128 mantissas each, beside every
# bf16 subnormal: the smallest normal binade; either side of 2^-120 (scale = amax / 448 crosses
# 2^-128 there, below which 1 / scale overflows); either side of 2^-105 (above it the residual of
# the Markstein step is exact); 2^0; 2^8 (448 itself); the largest finite binade.
DOMAIN_BINADES = (-126, -121, -120, -106, -105, 0, 8, 127)
DOMAIN_DEPTH = 20                 # every |x| from amax * 2^-20 up to amax
DOMAIN_FAR = (24, 40, 100)        # and one value this many binades below amax
DOMAIN_PAIRS = 3_806_462          # (amax, x) pairs in all: 1151 amax values, up to 5130 x each


@functools.lru_cache(maxsize=None)
def domain_amax_bits() -> np.ndarray:
    normals = [np.arange(128, dtype=np.int64) + ((e + 127) << 7) for e in DOMAIN_BINADES]
    return np.concatenate([np.arange(1, 128, dtype=np.int64)] + normals).astype(np.uint16)


def domain_values(amax_bits: int) -> np.ndarray:
    """The bf16 inputs (bit patterns) paired with this amax, without +-amax itself: every magnitude
    from amax * 2^-20 (or the smallest subnormal) up to the one below amax in both signs, +-0, and a
    few magnitudes far below."""
    a = int(amax_bits)
    mags = list(range(max(1, a - 128 * DOMAIN_DEPTH), a)) + [a - 128 * k for k in DOMAIN_FAR if a - 128 * k > 0] + [0]
    mags = np.array(sorted(set(mags)), dtype=np.uint16)
    return np.concatenate([mags, mags | np.uint16(0x8000)])


def domain_positions(cols: int):
    """Columns the row's single amax element moves through: first and last lane of a wave's first
    pass, the first lane of each wave of a 256-thread workgroup, its last thread, the last chunk."""
    cand = [0, 7, 63 * 8 + 3, 64 * 8, 128 * 8 + 1, 192 * 8 + 5, 255 * 8 + 7, 256 * 8 + 2, cols - 8, cols - 1]
    return [c for c in cand if 0 <= c < cols]


@functools.lru_cache(maxsize=None)
def domain_rows(cols: int):
    """``(x_bits [rows, cols], row_amax_bits [rows])``: for each amax of ``domain_amax_bits`` at least
    two rows (the amax element positive in one, negative in the next, at a position that moves from
    row to row) that together hold every value of ``domain_values``; a row is padded by repeating its
    values. One more row when needed so that rows % 4 != 0 (a ragged last workgroup)."""
    pos = domain_positions(cols)
    rows, amaxes = [], []
    for a in domain_amax_bits():
        vals = domain_values(a)
        n = max(2, -(-len(vals) // (cols - 1)))
        per = -(-len(vals) // n)
        for k in range(n):
            chunk = vals[k * per:(k + 1) * per]
            if len(chunk) == 0:
                chunk = vals[:1]
            fill = np.resize(chunk, cols - 1)
            p = pos[(len(rows) // 2) % len(pos)]               # each position in both signs
            mine = np.uint16(a) | np.uint16(0x8000 if len(rows) % 2 else 0)
            rows.append(np.concatenate([fill[:p], [mine], fill[p:]]))
            amaxes.append(a)
    while len(rows) % 4 != 3:
        rows.append(rows[len(rows) % 7])
        amaxes.append(amaxes[(len(rows) - 1) % 7])
    x = np.stack(rows).astype(np.uint16)
    x.setflags(write=False)
    return x, np.array(amaxes, dtype=np.uint16)


def domain_pair_table(x_bits: np.ndarray, row_amax_bits: np.ndarray) -> np.ndarray:
    """bool ``[n_amax, 65536]``: which (amax, x) pairs the rows hold."""
    amaxes = domain_amax_bits()
    idx = np.searchsorted(amaxes, row_amax_bits)
    assert np.array_equal(amaxes[idx], row_amax_bits)
    table = np.zeros((len(amaxes), 65536), dtype=bool)
    table[np.broadcast_to(idx[:, None], x_bits.shape), x_bits] = True
    return table


@functools.lru_cache(maxsize=None)
def domain_expected_table() -> np.ndarray:
    amaxes = domain_amax_bits()
    table = np.zeros((len(amaxes), 65536), dtype=bool)
    for i, a in enumerate(amaxes):
        table[i, domain_values(a)] = True
        table[i, [int(a), int(a) | 0x8000]] = True
    return table


def random_bits(rng, rows, cols, log2_scale=0):
    """Random bf16 bit patterns: |N(0,1)| * 2^log2_scale in fp32, truncated to bf16 (subnormals where
    the scale puts them), random signs, and some +-0.0."""
    v = (rng.standard_normal((rows, cols)) * 2.0 ** log2_scale).astype(np.float32)
    bits = (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    z = rng.random((rows, cols))
    bits = np.where(z < 0.02, np.uint16(0x8000), bits)
    return np.where(z > 0.98, np.uint16(0), bits).astype(np.uint16)


CAT_CASES = ((512, 512), (8, 1016, 24), (8, 8, 8, 8), (4096, 4096, 1024), (4096, 4104, 1016), (14336, 14336),
             (14336, 8, 14336), (1024,))
CAT_ROWS = 5


def cat_case(widths):
    """bf16 parts ``[CAT_ROWS, w]`` for ``quant_rows_cat``: row r's maximum sits in source r % n alone;
    row 3 is tiny (amax below 2^-110), row 4 subnormal; +-0.0 sprinkled everywhere."""
    rng = np.random.default_rng(sum(widths) + len(widths))
    parts = []
    for k, w in enumerate(widths):
        p = random_bits(rng, CAT_ROWS, w)
        p[3] = random_bits(rng, 1, w, -118)[0]
        p[4] = random_bits(rng, 1, w, -130)[0]
        parts.append(p)
    for r in range(CAT_ROWS):
        k = r % len(widths)
        top = max(int((p[r] & 0x7FFF).max()) for p in parts)
        parts[k][r, (7 * r + 3) % widths[k]] = np.uint16(top + 37) | np.uint16(0x8000 if r & 1 else 0)
    return parts


COLS_T_CASES = ((64, 256), (320, 512), (576, 768))


def cols_t_case(rows, cols):
    """bf16 ``[rows, cols]`` for ``quant_cols_t``: column c's maximum sits in 256-row segment c % n_seg
    alone; column 5 is all zero; columns with c % 7 == 3 are tiny, c % 11 == 4 subnormal."""
    rng = np.random.default_rng(rows * 1000 + cols)
    w = random_bits(rng, rows, cols)
    c = np.arange(cols)
    w[:, c % 7 == 3] = random_bits(rng, rows, int((c % 7 == 3).sum()), -118)
    w[:, c % 11 == 4] = random_bits(rng, rows, int((c % 11 == 4).sum()), -130)
    nseg = -(-rows // 256)
    top = (w & 0x7FFF).max(axis=0).astype(np.int64)
    seg = c % nseg
    r = np.minimum(seg * 256 + (c * 5) % 256, rows - 1)
    r = np.where(r // 256 == seg, r, seg * 256)
    w[r, c] = (top + 21).astype(np.uint16) | np.where(c & 1, 0x8000, 0).astype(np.uint16)
    w[:, 5] = 0
    return w
