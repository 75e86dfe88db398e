"""The bit-exact tile weight-gradient references of tests/wgrad_ref.py against the oracle on the CPU, their
preconditions, the share of roundings their operands exercise, and planted errors (each one changes at least
1 % of the output it touches at every case of tests/test_gpu_wgrad_exact.py that relies on it). No GPU."""
import pytest
import torch

from oracle import smt_oracle as oracle
from tests import wgrad_ref as W

BF16, FP16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
HOST_CASES = [(cid, seq, T, n, dt) for cid, seq, T, n in W.host_cases() for dt in W.case_dtypes(cid)]


def _id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


def _case_id(c):
    return f"{c[0]}-{_id(c[4])}"


def _operands(cid, T, dt):
    return W.int_operands(T, W.OUT_F, W.IN_F, dt, W.seed_of(cid, dt))


@pytest.mark.parametrize("case", [c for c in HOST_CASES if c[1]], ids=_case_id)
def test_reference_rounding_is_the_oracle_bit_for_bit(case):
    cid, seq, T, n, dt = case
    g, x = _operands(cid, T, dt)
    tiles = W.TILES[n]
    want = oracle.linearz_tile_grads(g.view(T // seq, seq, -1), x.view(T // seq, seq, -1), tiles)
    got = W.to_dtype(W.reference_rounding(g, x, seq, tiles, dt, dt), dt)
    assert want.dtype == dt and torch.equal(got.view(torch.int32 if dt == F32 else torch.int16),
                                            want.view(torch.int32 if dt == F32 else torch.int16))
    # fp32 out is the same values widened
    wide = W.reference_rounding(g, x, seq, tiles, dt, F32)
    assert torch.equal(wide, got.to(F64))


@pytest.mark.parametrize("case", HOST_CASES, ids=_case_id)
def test_single_in_fp64_is_the_oracles_fp64_truth(case):
    cid, seq, T, n, dt = case
    g, x = _operands(cid, T, dt)
    tiles = W.TILES[n]
    truth = oracle.tile_grads_fp64(g.unsqueeze(0), x.unsqueeze(0), tiles)
    assert torch.equal(W.single(g, x, tiles, F64), truth)
    # one rounding of it is torch's own conversion (round to nearest even), and fp32 out holds the sum itself
    for out_dt in (dt, F32):
        assert torch.equal(W.single(g, x, tiles, out_dt), truth.float().to(out_dt).to(F64))


@pytest.mark.parametrize("dt", [BF16, FP16, F32], ids=_id)
def test_round_to_even_is_torchs_conversion_and_the_other_modes_are_not(dt):
    gen = torch.Generator().manual_seed(3)
    v = torch.randint(-(1 << 16), 1 << 16, (1 << 16,), generator=gen).to(F64) * 0.125
    if dt == FP16:
        v = v / 4
    even = W.round_to(v, dt)
    assert torch.equal(even, v.float().to(dt).to(F64))
    away, trunc = W.round_to(v, dt, "away"), W.round_to(v, dt, "trunc")
    if dt == F32:
        assert torch.equal(away, v) and torch.equal(trunc, v)
        return
    assert bool((trunc.abs() <= v.abs()).all()) and bool((trunc != even).any())
    tie = (away != even)
    assert bool(tie.any()) and bool(((even - v).abs()[tie] == (away - v).abs()[tie]).all())
    # hand-made ties: 257 and 259 lie half way between two bf16 values, 2049 and 2051 between two fp16 values
    t = torch.tensor([257.0, 259.0, -257.0] if dt == BF16 else [2049.0, 2051.0, -2049.0], dtype=F64)
    want_even = [256.0, 260.0, -256.0] if dt == BF16 else [2048.0, 2052.0, -2048.0]
    want_away = [258.0, 260.0, -258.0] if dt == BF16 else [2050.0, 2052.0, -2050.0]
    assert W.round_to(t, dt).tolist() == want_even and W.round_to(t, dt, "away").tolist() == want_away


@pytest.mark.parametrize("case", [c for c in HOST_CASES if c[1] and c[4] != F32], ids=_case_id)
def test_the_operands_exercise_the_roundings_and_do_not_overflow(case):
    """>= 30 % of the per-sample partials and of the sample sums are inexact before their rounding, at the
    case's own tiles, and nothing reaches the format's largest finite value."""
    cid, seq, T, n, dt = case
    partials, sums, one_vs_two, top = W.seq_shares(T // seq, seq, dt, W.TILES[n])
    print(f"{cid} {dt}: partials {partials:.2f} sums {sums:.2f} one rounding differs {one_vs_two:.2f} max {top:.2g}")
    assert partials >= 0.30 and sums >= 0.30, (partials, sums)
    assert one_vs_two >= 0.10, one_vs_two
    assert top < (1.0 if dt == FP16 else 2.0 ** -8), top


@pytest.mark.parametrize("case", [c for c in HOST_CASES if not c[1] and c[2] >= 300 and c[4] != F32], ids=_case_id)
def test_the_single_rounding_is_exercised(case):
    cid, seq, T, n, dt = case
    g, x = _operands(cid, T, dt)
    share = W.inexact_share(W.single(g, x, W.TILES[n], F64), dt)
    assert share >= 0.30, share
    base = W.int_base(n, dt, W.seed_of(cid, dt))
    moved = W.single(g, x, W.TILES[n], dt, base) != W.single(g, x, W.TILES[n], dt) + base
    assert float(moved.double().mean()) >= 0.10, "the base does not move the rounding"


@pytest.mark.parametrize("case", HOST_CASES, ids=_case_id)
def test_every_planted_error_changes_the_output_it_touches(case):
    """At every case, output dtype and ``accumulate`` setting of the GPU file for which ``mutation_applies``
    says the case can see the error. The tiles are the case's first three (the shapes decide, not the count)."""
    cid, seq, T, n, dt = case
    tiles = W.TILES[n][:3]
    g, x = _operands(cid, T, dt)
    gp, xp = W.pad_rows(g), W.pad_rows(x)
    seen = set()
    for out_dt in ([dt, F32] if dt != F32 else [F32]):
        for base in (None, W.int_base(len(tiles), dt, W.seed_of(cid, dt))):
            for mut in W.MUTATIONS:
                if not W.mutation_applies(mut, seq, T, dt, out_dt, base is not None, len(tiles)):
                    continue
                share = W.mutation_share(mut, gp, xp, T, seq, tiles, dt, out_dt, base)
                assert share >= 0.01, (mut, out_dt, base is not None, share)
                seen.add(mut)
    assert {"row_past_T", "last_row_dropped", "transposed", "rc_swapped", "base_dropped"} <= seen


def test_every_mutation_is_relied_on_somewhere():
    seen = set()
    for cid, seq, T, n, dt in HOST_CASES:
        for out_dt in (dt, F32):
            seen |= {m for m in W.MUTATIONS if W.mutation_applies(m, seq, T, dt, out_dt, True, n)}
    assert seen == set(W.MUTATIONS)


def test_the_preconditions_are_asserted():
    # sum |g x| beyond 2^24: an fp32 partial sum could round
    g, x = W.int_operands(300, 512, 512, F32, 1, amp=1000)
    with pytest.raises(AssertionError, match="not exact in fp32"):
        W.single(g, x, [(0, 0)], F32)
    # a base that lifts it over
    g, x = W.int_operands(64, 512, 512, F32, 1)
    W.single(g, x, [(0, 0)], F32)
    with pytest.raises(AssertionError, match="not exact in fp32"):
        W.single(g, x, [(0, 0)], F32, base=torch.full((256, 256), 2.0 ** 24, dtype=F64))
    # fp16 overflow: 300 products of 16 * 16 are exact in fp32 and beyond 65504
    g = torch.full((300, 512), 16.0, dtype=FP16)
    W.reference_rounding(g[:200], g[:200], 100, [(1, 1)], FP16, FP16)
    with pytest.raises(AssertionError, match="overflows"):
        W.reference_rounding(g, g, 300, [(1, 1)], FP16, FP16)
    # operands off the grid are refused where they are made
    with pytest.raises(AssertionError, match="not exact in their dtype"):
        W.int_operands(8, 512, 512, BF16, 1, amp=1000)


def test_mx_operands_are_lossless_in_mx_and_exercise_the_bf16_rounding():
    T = 300
    g, x = W.mx_int_operands(T, 1024, 768, 5)
    rbs, cbs = [0, 1, 2, 3], [0, 1, 2]
    qg, sg = oracle.mx_quant_cols(g, rbs)
    qx, sx = oracle.mx_quant_cols(x, cbs)
    assert torch.equal(oracle.mx_dequant(qg, sg)[:, :T].permute(1, 0, 2).reshape(T, -1), g.to(F64))
    assert torch.equal(oracle.mx_dequant(qx, sx)[:, :T].permute(1, 0, 2).reshape(T, -1), x.to(F64))
    tiles = W.TILES[9]
    truth = W.single(g, x, tiles, F64, unit2=W.MX_UNIT2)
    assert torch.equal(oracle.mx_tile_grads_fp64(qg, sg, qx, sx, tiles), truth)
    assert float(g.to(F64).abs().max() * x.to(F64).abs().max()) > 256
    assert W.inexact_share(truth, BF16) >= 0.30
    # several exponents are really in use
    assert len(set(sg.flatten().tolist())) >= 3 and len(set(sx.flatten().tolist())) >= 2


def test_random_bound_is_positive_and_holds_for_a_plain_fp32_sum():
    """The bound admits an fp32 evaluation in the plain order (a check of the bound's own arithmetic)."""
    T, tiles = 300, W.TILES[2]
    for dt in (BF16, FP16, F32):
        g, x = W.random_operands(T, W.OUT_F, W.IN_F, dt, 9)
        if dt != FP16:
            tiny = g.float().abs()
            assert bool(((tiny > 0) & (tiny < 1e-38)).any()), "no subnormal operand"
        truth, bound = W.random_bound(g, x, tiles, T, 1)
        assert bool((bound > 0).all())
        acc = torch.zeros(len(tiles), 256, 256)
        for t in range(T):
            for i, (r, c) in enumerate(tiles):
                acc[i] += torch.outer(g[t, r * 256:(r + 1) * 256].float(), x[t, c * 256:(c + 1) * 256].float())
        ratio = ((acc.to(F64) - truth).abs() / bound).max().item()
        assert ratio <= 1.0, ratio
