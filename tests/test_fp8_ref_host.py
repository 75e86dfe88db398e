"""tests/fp8_ref.py checked on the CPU: the format against torch's CPU converter, the quotient against
``torch.div``, the inputs of tests/test_gpu_fp8_exact.py against eight wrong quantisers (each must be
seen by the comparer on those very inputs), and an emulation of the Markstein quotient of
csrc/fp8_math.h that maps where it is exact."""
import numpy as np
import pytest
import torch

from tests import fp8_ref as R


def _torch_encode(v32: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_decode_all_bytes_against_torch():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    got = R.e4m3_decode(codes)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 2
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))         # -0.0 included
    assert got[0x7E] == 448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6


def test_encode_every_bf16_pattern_against_torch():
    v = R.bf16_to_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16))
    assert R.compare_bits(R.e4m3_encode(v), _torch_encode(v)) is None


def test_encode_midpoints_and_their_neighbours_against_torch():
    vals = R.e4m3_decode(np.arange(0x7F, dtype=np.uint8))                      # 0 .. 448, ascending
    mid = ((vals[:-1] + vals[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (vals[:-1] + vals[1:]) / 2)  # exact in fp32
    pts = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9))])
    pts = np.concatenate([pts, -pts])
    got = R.e4m3_encode(pts)
    assert R.compare_bits(got, _torch_encode(pts)) is None
    # ties go to the even code, the neighbours to their own side
    n = len(mid)
    lo = np.arange(n)
    assert np.array_equal(got[:n], np.where(lo & 1, lo + 1, lo))
    assert np.array_equal(got[n:2 * n], lo) and np.array_equal(got[2 * n:3 * n], lo + 1)


def test_encode_top_of_the_range_against_torch():
    top = np.array([448.0, 464.0, np.nextafter(np.float32(464.0), np.float32(1e9)), 480.0, 1e30, np.inf], np.float32)
    top = np.concatenate([top, -top])
    got = R.e4m3_encode(top)
    assert R.compare_bits(got, _torch_encode(top)) is None
    assert list(got[:6]) == [0x7E, 0x7E, 0x7F, 0x7F, 0x7F, 0x7F] and list(got[6:8]) == [0xFE, 0xFE]
    zeros = np.array([0.0, -0.0, 2.0 ** -11, -2.0 ** -11, 1e-45, -1e-45], np.float32)
    assert list(R.e4m3_encode(zeros)) == [0x00, 0x80, 0x00, 0x80, 0x00, 0x80]
    assert R.compare_bits(R.e4m3_encode(zeros), _torch_encode(zeros)) is None


def test_rn32_keeps_subnormals_and_rounds_to_even():
    v = np.array([2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149,
                  1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** 128 * (1 - 2.0 ** -25), 2.0 ** 128 * (1 - 2.0 ** -26)])
    want = np.array([2.0 ** -149, 0.0, 2.0 ** -149, 2.0 ** -148, 2.0 ** -148, 1.0, 1 + 2.0 ** -22,
                     np.inf, np.inf])
    assert np.array_equal(R.rn32(v).astype(np.float64), want)
    assert float(R.INV_E4M3_MAX) == float(np.float32(1.0) / np.float32(448.0))
    assert float(R.row_scale(np.float32(0))) == 1.0 and float(R.row_scale(np.float32(448))) == 1.0


def _tiny_rows():
    """The value-domain rows (width 1024) whose amax lies below 2^-104."""
    x, amax = R.domain_rows(1024)
    sel = amax < ((-104 + 127) << 7)
    return x[sel], amax[sel]


def test_quotient_against_torch_div_on_the_tiny_scale_set():
    x, _ = _tiny_rows()
    xf = R.bf16_to_f32(x)
    scale = R.row_scale(np.abs(xf).max(axis=1))
    assert 0 < scale.min() < 2.0 ** -140 and (scale < 2.0 ** -126).sum() > 500         # subnormal scales too
    want = torch.div(torch.from_numpy(xf), torch.from_numpy(scale)[:, None]).numpy()
    assert R.compare_bits(R.quotient(xf, scale[:, None]), want, "quotient") is None
    # and on the whole width-1024 domain
    x, _ = R.domain_rows(1024)
    xf = R.bf16_to_f32(x)
    scale = R.row_scale(np.abs(xf).max(axis=1))
    want = torch.div(torch.from_numpy(xf), torch.from_numpy(scale)[:, None]).numpy()
    assert R.compare_bits(R.quotient(xf, scale[:, None]), want, "quotient") is None


@pytest.mark.parametrize("cols", [1024, 4096, 16384, 16392])
def test_domain_rows_cover_the_stated_pairs(cols):
    x, amax = R.domain_rows(cols)
    assert x.shape[0] % 4 == 3 and x.shape[1] == cols
    assert len(R.domain_amax_bits()) == 127 + 8 * 128
    assert np.array_equal((x & 0x7FFF).max(axis=1), amax)                    # the row's amax is the intended one
    assert np.all(((x & 0x7FFF) == amax[:, None]).sum(axis=1) == 1)          # and it sits in one element only
    table = R.domain_pair_table(x, amax)
    assert np.array_equal(table, R.domain_expected_table())
    assert table.sum() == R.DOMAIN_PAIRS
    # the amax element visits every listed position, in both signs
    col = np.argmax((x & 0x7FFF) == amax[:, None], axis=1)
    neg = x[np.arange(len(x)), col] >> 15
    assert {(int(c), int(s)) for c, s in zip(col, neg)} == {(c, s) for c in R.domain_positions(cols) for s in (0, 1)}


# ----------------------------------------------------------------------------- mutants

@pytest.fixture(scope="module")
def domain_1024():
    x, _ = R.domain_rows(1024)
    return x, R.quant_rows(x)


@pytest.mark.parametrize("name,kw", [
    ("round toward zero", dict(encode=lambda v: R.e4m3_encode(v, rounding="rtz"))),
    ("ties away from zero", dict(encode=lambda v: R.e4m3_encode(v, rounding="away"))),
    ("subnormals flushed", dict(encode=lambda v: R.e4m3_encode(v, subnormals=False))),
    ("zero sign dropped", dict(encode=lambda v: R.e4m3_encode(v, zero_sign=False))),
    ("amax / 448", dict(scale_of=R.row_scale_true_division)),
    ("x * (1 / scale)", dict(quot=R.quotient_uncorrected)),
])
def test_value_domain_inputs_see_the_mutant(domain_1024, name, kw):
    x, (q, s) = domain_1024
    mq, ms = R.quant_rows(x, **kw)
    report = R.compare_bits(mq, q, "bytes", x, s) or R.compare_bits(ms, s, "scales")
    assert report is not None, name
    if "scale_of" in kw:
        assert R.compare_bits(ms, s, "scales") is not None
    else:
        assert R.compare_bits(ms, s, "scales") is None
        n = int((mq != q).sum())
        print(f"{name}: {n} bytes differ")
        assert n >= 100                                   # not a single lucky element


@pytest.mark.parametrize("widths", R.CAT_CASES)
def test_cat_inputs_see_a_source_left_out_of_the_amax(widths):
    parts = R.cat_case(widths)
    q, s = R.quant_rows_cat(parts)
    assert (s[3] < 2.0 ** -110 / 448 * 2 ** 4) and s[4] < 2.0 ** -128
    assert sum(int((p == 0x8000).sum()) for p in parts) > 0
    if len(widths) == 1:
        return
    for k in range(len(widths)):
        mq, ms = R.quant_rows_cat(parts, skip_source=k)
        assert R.compare_bits(ms, s, "scales") is not None and R.compare_bits(mq, q) is not None, k


@pytest.mark.parametrize("rows,cols", R.COLS_T_CASES)
def test_cols_t_inputs_see_a_segment_left_out_of_the_amax(rows, cols):
    w = R.cols_t_case(rows, cols)
    q, s = R.quant_cols_t(w)
    assert q.shape == (cols, rows) and s[5] == 1.0 and not q[5].any()
    assert (s < 2.0 ** -128).any() and (w == 0x8000).any()
    for seg in range(-(-rows // 256)):
        mq, ms = R.quant_cols_t(w, skip_segment=seg)
        assert R.compare_bits(ms, s, "scales") is not None and R.compare_bits(mq, q) is not None, seg


# ----------------------------------------------------------------------------- the Markstein quotient, emulated

def _fma32(a, b, c):
    """RN32(a * b + c) for fp32 operands. The product is exact in fp64; the sum is rounded to fp64 to
    odd (TwoSum gives the exact error of the fp64 addition; where it is not zero the result is the
    neighbour with an odd last bit), and 53 >= 24 + 2 bits then make the rounding to fp32 a single one."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return R.rn32(s)


def qv_plain(x, scale):
    """The quotient of csrc/fp8_math.h before the tiny-row lift, emulated operation by operation in
    fp32 with subnormals kept (hipcc's default for fp32 on gfx950): rs = RN(1 / scale),
    q0 = RN(x * rs), r = fma(-q0, scale, x), q = fma(r, rs, q0), a clamp to +-448 that ignores a NaN
    (v_med3_f32 returns the minimum of its operands when one is a NaN: -448)."""
    with np.errstate(all="ignore"):
        rs = R.rn32(1.0 / scale.astype(np.float64))
        q0 = R.rn32(x.astype(np.float64) * rs.astype(np.float64))
        r = _fma32(-q0, scale, x)
        q = _fma32(r, rs, q0)
        q = np.where(np.isnan(q), np.float32(-448.0), np.clip(q, np.float32(-448.0), np.float32(448.0)))
        return q.astype(np.float32)


def qv_lifted(x, scale):
    """The quotient of csrc/fp8_math.h as it is now: rows whose scale is below 2^-100 are lifted by 2^64
    (exact for x and scale), and the residual is taken as q0 * scale - x and subtracted, which keeps
    the sign of a zero x."""
    with np.errstate(all="ignore"):
        lift = np.where(scale < np.float32(2.0 ** -100), np.float32(2.0 ** 64), np.float32(1.0))
        x, scale = (x * lift).astype(np.float32), (scale * lift).astype(np.float32)
        rs = R.rn32(1.0 / scale.astype(np.float64))
        q0 = R.rn32(x.astype(np.float64) * rs.astype(np.float64))
        r = _fma32(q0, scale, -x)
        q = _fma32(-r, rs, q0)
        q = np.where(np.isnan(q), np.float32(-448.0), np.clip(q, np.float32(-448.0), np.float32(448.0)))
        return q.astype(np.float32)


def _all_pairs(amax_bits):
    """x (fp32) [n_amax, n_x] = every bf16 |x| <= the largest amax in both signs (+-0 too), scale
    [n_amax, 1], and the mask of pairs with |x| <= amax."""
    top = int(amax_bits.max())
    mags = np.arange(0, top + 1, dtype=np.uint16)
    xb = np.concatenate([mags, mags | np.uint16(0x8000)])
    x = np.broadcast_to(R.bf16_to_f32(xb), (len(amax_bits), len(xb)))
    valid = (xb & 0x7FFF)[None, :] <= amax_bits[:, None]
    scale = R.row_scale(R.bf16_to_f32(amax_bits))[:, None]
    return xb, np.ascontiguousarray(x), scale, valid


def _mismatches(qfn, amax_bits, step=256):
    xb, x, scale, valid = _all_pairs(amax_bits)
    bad = np.zeros(valid.shape, dtype=bool)
    for i in range(0, len(amax_bits), step):                       # in slices: the fp64 temporaries are large
        sl = slice(i, i + step)
        want = R.e4m3_encode(R.quotient(x[sl], scale[sl]))
        got = R.e4m3_encode(qfn(x[sl], np.broadcast_to(scale[sl], x[sl].shape).copy()))
        bad[sl] = (got != want) & valid[sl]
    return bad, xb


# What the emulation of the plain quotient counts over every positive bf16 amax below 2^-100 and every
# bf16 |x| <= amax in both signs, -0.0 aside (which differs at every amax): the wrong bytes, the amax
# values with at least one, and the wrong bytes per amax range (below 1.3e-36, up to 1e-33, above).
PLAIN_MISMATCHES = 979_476
PLAIN_FAILING_AMAX = 1_076
PLAIN_BY_RANGE = (973_378, 6_028, 70)


def test_markstein_emulation_disagreement_set():
    """Every positive bf16 amax below 2^-100 against every |x| <= amax, and full binades above: where
    the plain Markstein quotient leaves the contract, and that the lifted one never does.

    Below amax = 2^-120 * 1.75 (scale below 2^-128) 1 / scale overflows: q0 is infinite, the result a
    NaN, and every element of the row, zeros included, becomes -448. From there up to 2^-105 the
    residual x - q0 * scale falls below 2^-149 for some pairs and is rounded, which moves a few results
    across an e4m3 rounding boundary. Above, no bit differs but the sign of -0.0. The arithmetic above
    the tiny range depends on the mantissas alone (no operation underflows or overflows), so the binades
    2^-100, 2^0, 2^8, 2^28 and 2^127 stand for the rest; with the last four every x below 2^-100 is there
    too, whose quotient underflows fp32 (the byte is a zero with the sign of x)."""
    tiny = np.arange(1, ((-100 + 127) << 7), dtype=np.uint16)                  # every amax below 2^-100
    bad, xb = _mismatches(qv_plain, tiny)
    neg_zero = xb == 0x8000
    assert bad[:, neg_zero].all()                                              # -0.0 -> +0 at every scale
    bad_nz = bad & ~neg_zero[None, :]
    per_amax = bad_nz.sum(axis=1)
    amax = R.bf16_to_f32(tiny).astype(np.float64)
    failing = per_amax > 0
    print(f"plain Markstein: {int(bad_nz.sum())} mismatches over {int(failing.sum())} amax values; "
          f"largest failing amax {amax[failing].max():.4g}; "
          f"{int(bad_nz[amax < 1.3e-36].sum())} below 1.3e-36, "
          f"{int(bad_nz[(amax >= 1.3e-36) & (amax < 1e-33)].sum())} in [1.3e-36, 1e-33), "
          f"{int(bad_nz[amax >= 1e-33].sum())} above")
    # the predicted domain ("The bar on fp8 quantisation")
    assert amax[failing].max() < 2.0 ** -104
    inf_rs = np.isinf(R.rn32(1.0 / R.row_scale(R.bf16_to_f32(tiny)).astype(np.float64)))
    assert per_amax[inf_rs].min() > 0                                          # 1 / scale = inf: every such row fails
    assert amax[inf_rs].max() < 2.0 ** -119
    assert int(bad_nz.sum()) == PLAIN_MISMATCHES and int(failing.sum()) == PLAIN_FAILING_AMAX
    assert (int(bad_nz[amax < 1.3e-36].sum()), int(bad_nz[(amax >= 1.3e-36) & (amax < 1e-33)].sum()),
            int(bad_nz[amax >= 1e-33].sum())) == PLAIN_BY_RANGE
    assert 3.27e-32 < amax[failing].max() < 3.28e-32
    # the header's quotient (lift, residual subtracted) is exact on all of it, -0.0 included
    bad, _ = _mismatches(qv_lifted, tiny)
    assert not bad.any()
    # and both are exact on whole binades above (but for -0.0 in the plain one)
    for e in (-100, 0, 8, 28, 127):
        binade = (np.arange(128) + ((e + 127) << 7)).astype(np.uint16)
        for fn in (qv_plain, qv_lifted):
            xb2, x, scale, valid = _all_pairs(binade)
            lo = int(binade[0]) - 128 * 24                                     # 24 binades of x below, and +-0
            keep = ((xb2 & 0x7FFF) >= max(lo, 0)) | ((xb2 & 0x7FFF) == 0)
            if e >= 0:                                                         # and quotients that underflow fp32
                keep |= (xb2 & 0x7FFF) < ((-100 + 127) << 7)
            want = R.e4m3_encode(R.quotient(x[:, keep], scale))
            got = R.e4m3_encode(fn(x[:, keep], np.broadcast_to(scale, x[:, keep].shape).copy()))
            bad = (got != want) & valid[:, keep]
            if fn is qv_plain:
                bad &= (xb2[keep] != 0x8000)[None, :]
            assert not bad.any(), (e, fn.__name__)
