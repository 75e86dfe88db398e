"""Exact, framed tests of the kernels that decide what gets trained: ``block_score_kernel``,
``act_accumulate_kernel`` and ``channel_partial_kernel`` / ``channel_final_kernel`` of
``csrc/smt_kernels.hip``.

The scores are compared with ``torch.equal`` against expectations computed in int64: the inputs come
from ``move_ref.exact_grid`` (fp32 multiples of 2^-10 below 16, whose sums and whose fp32 squares' sums
are exact in fp64 in any order), so no tolerance is needed and a square taken in fp64 or fused into the
add shows. The harvest is compared bit for bit with the CPU's fp32 ``=`` / ``+=`` on the whole 16-bit
domain and on fp32 bit patterns, except that a NaN may differ in payload (the NaN rule of
``move_ref.nan_rule``). Outputs and workspaces sit in ``move_ref.Frame`` windows through the C ABI."""
import numpy as np
import pytest
import torch

from oracle import smt_oracle as ref
from sparse_matrix_tuning_amd import _hip
from tests import move_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = M.BLOCK
CODE = {"mean_abs": _hip.SCORE_MEAN_ABS, "abs_mean": _hip.SCORE_ABS_MEAN, "L1": _hip.SCORE_L1, "L2": _hip.SCORE_L2}
_INT = {2: torch.int16, 4: torch.int32}
_ITEM = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _lib():
    return _hip.load()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _ok(rc, what):
    assert rc == 0, f"{what}: status {rc}: {_lib().smt_last_error().decode(errors='replace')}"
    torch.cuda.synchronize()


def _frame(rows, cols, itemsize, pad=0):
    return M.Frame(rows, cols, itemsize, pad=pad, device=DEV)


def _bits64(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int64)


# ----------------------------------------------------------------------------- block scores
@pytest.fixture(scope="module")
def grads():
    """The three gradients on the device; the (2, 3) one a view with ld = 768 + 4 whose pad columns hold
    a value that is no multiple of 2^-10 (a kernel that read them would miss the integer sums)."""
    out = []
    for k, x, (d1, d2) in M.score_case():
        if (d1, d2) == (2, 3):
            wide = torch.full((d1 * B + 1, d2 * B + M.SCORE_LD_PAD), 0.3, dtype=torch.float32, device=DEV)
            g = wide[:d1 * B, :d2 * B]
            g.copy_(x)
            assert g.stride(0) == 768 + 4 and g.data_ptr() % 16 == 0
        else:
            g = x.to(DEV)
        out.append(g)
    return out


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_block_scores_equal_the_integer_sums(grads, strategy):
    from sparse_matrix_tuning_amd.smt import ranking
    from sparse_matrix_tuning_amd.smt.smt_helper import finalize_scores
    case = M.score_case()
    raws = _hip.block_scores(grads, M.SCORE_GRIDS, CODE[strategy])
    torch.cuda.synchronize()
    assert len(raws) == 3
    for raw, (k, x, (d1, d2)) in zip(raws, case):
        raw = raw.cpu()
        want = M.block_raw_exact(k, x, d1, d2, strategy)
        assert torch.equal(raw, want), (strategy, (d1, d2), raw, want)
        assert torch.equal(_bits64(raw), _bits64(want))                     # no -0.0 sum either
        # what the existing test keeps: the finalised value and the ranking's interval
        got = finalize_scores(raw.numpy(), strategy).reshape(d1, d2)
        assert (got == ref.block_stat_fp64(x, d1, d2, strategy).numpy()).all()
        _nom, lo, hi = ranking.block_intervals(raw.numpy(), strategy)
        lit = ref.block_stat(x, d1, d2, strategy).numpy().reshape(-1)
        assert np.all(lo <= lit) and np.all(lit <= hi)
        if (d1, d2) == (2, 3):
            assert lo[0] == hi[0] == 0.0 and raw[0, 0] == 0 and raw[0, 1] == 0      # the all-zero block


def test_block_scores_table_with_a_strategy_per_entry(grads):
    """One ABI launch over the three gradients, each entry with its own grid, row stride and strategy,
    the three outputs carved from one framed fp64 buffer with two sentinel doubles between them."""
    case = M.score_case()
    for strategies in (("L2", "mean_abs", "L1"), ("abs_mean", "L2", "mean_abs")):
        sizes = [2 * d1 * d2 for d1, d2 in M.SCORE_GRIDS]
        offs, at = [], 0
        for n in sizes:
            offs.append(at)
            at += n + 2
        out = _frame(1, at, 8)
        want = torch.full((at,), M.SENTINEL[8], dtype=torch.int64)
        entries, blk = [], 0
        for g, (k, x, (d1, d2)), s, off, n in zip(grads, case, strategies, offs, sizes):
            assert (out.ptr + 8 * off) % 16 == 0
            entries.append(_hip.ScoreEntry(g.data_ptr(), g.stride(0), d1, d2, blk, out.ptr + 8 * off, CODE[s], 0))
            blk += d1 * d2
            want[off:off + n] = _bits64(M.block_raw_exact(k, x, d1, d2, s)).reshape(-1)
        assert [e.block_begin for e in entries] == [0, 1, 7] and [e.ld for e in entries] == [256, 772, 256]
        table = _hip._device_table(entries, _hip.ScoreEntry, torch.device(DEV))
        _ok(_lib().smt_block_score(table.data_ptr(), 3, blk, _stream()), "smt_block_score")
        out.check_intact()
        assert torch.equal(out.whole(), out.expected_whole(want)), strategies


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_block_scores_non_finite_blocks_stay_local(grads, strategy):
    clean = [r.cpu() for r in _hip.block_scores(grads, M.SCORE_GRIDS, CODE[strategy])]
    wide = torch.full((2 * B + 1, 3 * B + M.SCORE_LD_PAD), 0.3, dtype=torch.float32, device=DEV)
    g = wide[:2 * B, :3 * B]
    g.copy_(grads[1])
    g[100, 2 * B + 200] = float("nan")                                      # block (0, 2) = 2
    g[B + 255, 0] = float("-inf")                                           # block (1, 0) = 3
    dirty = [grads[0], g, grads[2]]
    got =[r.cpu() for r in _hip.block_scores(dirty, M.SCORE_GRIDS, CODE[strategy])]
    torch.cuda.synchronize()
    assert torch.isnan(got[1][2]).all()
    assert not torch.isfinite(got[1][3]).any()
    assert got[1][3, 1] == float("inf")
    keep = [0, 1, 4, 5]
    assert torch.equal(_bits64(got[1][keep]), _bits64(clean[1][keep]))
    assert torch.equal(_bits64(got[0]), _bits64(clean[0])) and torch.equal(_bits64(got[2]), _bits64(clean[2]))


# ----------------------------------------------------------------------------- activation harvest
def _harvest_inputs(dtype, Bn, S, C):
    """Three x of [Bn, S, C]: bit patterns (the domain tile when they are 65,536), then twice
    Gaussian-times-log-normal data."""
    item = _ITEM[dtype]
    first = M.with_domain_prefix(M.random_bits((Bn, S, C), item, 900 + S), 901).view(dtype)
    rest = [M.accum_gaussian(Bn * S * C, dtype, 910 + 2 * i + S).view(Bn, S, C) for i in range(2)]
    return [first] + rest


@pytest.mark.parametrize("Bn,S,C", [(2, 32, 1024), (3, 5, 520)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_accumulate_sliced_input_framed_accumulator(dtype, Bn, S, C):
    item = _ITEM[dtype]
    off = 8 if item == 2 else 4
    assert (Bn * S * (C // 8)) % 256 != 0 or (Bn, S, C) == (2, 32, 1024)
    acc = _frame(Bn * S, C, 4)
    feat = {}
    xs = _harvest_inputs(dtype, Bn, S, C)
    if (Bn, S, C) == (2, 32, 1024):
        assert torch.equal(xs[0].view(_INT[item]).reshape(B, B), M.domain_tile(item, 901))
    for step, x in enumerate(xs):
        big = M.random_bits((Bn, S + 5, C + 16), item, 920 + step).to(DEV)
        xd = big.view(dtype)[:, 3:3 + S, off:off + C]
        xd.copy_(x.to(DEV))
        before = big.clone()
        assert xd.stride(0) != S * xd.stride(1) and xd.data_ptr() % 16 == 0
        _ok(_lib().smt_act_accumulate(xd.data_ptr(), _hip._DT[dtype], xd.stride(1), xd.stride(0), Bn, S, C, acc.ptr,
                                      int(step == 0), _stream()), "smt_act_accumulate")
        ref.channel_hook_accumulate(feat, "k", x)
        acc.check_intact()
        report = M.nan_rule(acc.view(torch.float32), feat["k"])
        assert report is None, f"{dtype} step {step}: {report}"
        assert torch.equal(big, before), "x was written"
    # once through the wrapper: the same three steps into a plain accumulator
    plain = torch.empty(Bn, S, C, dtype=torch.float32, device=DEV)
    for step, x in enumerate(xs):
        big = torch.zeros(Bn, S + 5, C + 16, dtype=dtype, device=DEV)
        xd = big[:, 3:3 + S, off:off + C]
        xd.copy_(x.to(DEV))
        _hip.act_accumulate(xd, plain, assign=step == 0)
    torch.cuda.synchronize()
    report = M.nan_rule(plain, feat["k"])
    assert report is None, f"_hip.act_accumulate, {dtype}: {report}"


# ----------------------------------------------------------------------------- channel scores
@pytest.mark.parametrize("S", M.CHANNEL_S)
@pytest.mark.parametrize("Bn", M.CHANNEL_B)
def test_channel_scores_equal_the_integer_sums(Bn, S):
    C = M.CHANNEL_C
    k, x = M.channel_case(Bn, S)
    acc = x.to(DEV)
    need = _lib().smt_channel_score_workspace_bytes(S, C)
    assert need == (S + 31) // 32 * C * 8
    for strategy in M.STRATEGIES:
        want = M.channel_raw_exact(k, strategy)
        assert torch.equal(want, ref.channel_raw_fp64(x, strategy))
        ws = _frame(1, need // 8, 8)
        out = _frame(1, C, 8)
        _ok(_lib().smt_channel_score(acc.data_ptr(), Bn, S, C, CODE[strategy], ws.ptr, need, out.ptr, _stream()),
            "smt_channel_score")
        ws.check_intact()                                                   # nothing past `need` bytes
        out.check_intact()
        got = out.view(torch.float64).cpu().reshape(-1)
        assert torch.equal(got, want), (strategy, Bn, S)
        assert torch.equal(out.whole(), out.expected_whole(_bits64(want)))
        assert not bool((ws.bits() == M.SENTINEL[8]).any()), "a partial was never written"
        assert torch.equal(_hip.channel_scores(acc, CODE[strategy]).cpu(), want)


def test_channel_scores_workspace_contract_and_empty_sequence():
    C, S, Bn = M.CHANNEL_C, 33, 3
    _, x = M.channel_case(Bn, S)
    acc = x.to(DEV)
    need = _lib().smt_channel_score_workspace_bytes(S, C)
    ws = _frame(1, need // 8, 8)
    out = _frame(1, C, 8)
    rc = _lib().smt_channel_score(acc.data_ptr(), Bn, S, C, _hip.SCORE_L2, ws.ptr, need - 1, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == -3, rc                                                     # SMT_E_WORKSPACE
    assert "smt_channel_score" in _lib().smt_last_error().decode()
    for f in (ws, out):
        f.check_intact()
        assert bool((f.whole() == M.SENTINEL[8]).all())
    assert _lib().smt_channel_score_workspace_bytes(0, C) == 0
    _ok(_lib().smt_channel_score(acc.data_ptr(), Bn, 0, C, _hip.SCORE_L1, None, 0, out.ptr, _stream()), "smt_channel_score, S = 0")
    out.check_intact()
    assert torch.equal(out.bits(), torch.zeros(1, C, dtype=torch.int64))


# ----------------------------------------------------------------------------- argument errors
def test_act_accumulate_rejects_a_width_that_is_no_multiple_of_8():
    x = torch.zeros(2, 4, 32, dtype=torch.bfloat16, device=DEV)
    acc = _frame(8, 32, 4)
    rc = _lib().smt_act_accumulate(x.data_ptr(), _hip.DTYPE_BF16, 32, 128, 2, 4, 12, acc.ptr, 1, _stream())
    torch.cuda.synchronize()
    assert rc < 0 and "smt_act_accumulate" in _lib().smt_last_error().decode()
    acc.check_intact()
    assert bool((acc.whole() == M.SENTINEL[4]).all())
