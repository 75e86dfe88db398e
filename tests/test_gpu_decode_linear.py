"""The decode-linear kernel (smt_linear_skinny, include/smt_linear.h) on the GPU, held to the contracts its
header states, with the two bars of tests/linear_ref.py: integer inputs must be torch.equal to the exact
product, normal inputs must lie inside the derived per-element bound of the fp64 product.

Every launch writes into a 16-row buffer wider than N that is pre-filled with a sentinel, and everything
outside [0, M) x [0, N) must still hold it afterwards. Out-of-range behaviour is tested only with such
poison values inside allocations the test owns."""
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_ref as lr
from tests.attn_ref import assert_within_bounds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 77.0

# (M, N, K, pad): pad elements added to ldx, ldw and ldy
SHAPES = [
    (1, 16, 32, 0), (16, 16, 32, 0),        # one step, most waves idle
    (3, 48, 96, 0),                          # fewer steps than waves
    (16, 64, 544, 0),                        # 17 steps: an uneven split and an unroll tail
    (2, 16, 4896, 0),                        # 153 steps, 20 a wave: two full batches and a partial one, 13 on the last wave
    (5, 256, 512, 0),                        # the small model's shape
    (16, 32, 14336, 0), (16, 1024, 4096, 0),  # full depth
    (7, 64, 160, 8),                         # ldx = K + 8, ldw = K + 8, ldy = N + 8
]


def launch(x, weights, epilogue=_hip.SKINNY_PLAIN, pad=0):
    """The kernel's outputs for x [M, K] (a device tensor, any row stride) and device weights, written into
    sentinel-filled [16, N + 8 + pad] buffers whose every element outside [0, M) x [0, N) is checked."""
    M = x.shape[0]
    n_y = 1 if epilogue == _hip.SKINNY_SWIGLU else len(weights)
    bufs = [torch.full((16, w.shape[0] + 8 + pad), SENTINEL, dtype=x.dtype, device=DEV) for w in weights[:n_y]]
    outs = [b[:M, :w.shape[0]] for b, w in zip(bufs, weights)]
    got = _hip.linear_skinny(x, list(weights), epilogue, outs)
    torch.cuda.synchronize()
    for b, w in zip(bufs, weights):
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[:M, :w.shape[0]] = False
        assert bool((b[outside] == SENTINEL).all()), "the kernel wrote outside [0, M) x [0, N)"
    return [g.clone() for g in got]


def dev(t):
    """A device copy with the row stride of ``t`` (a view of a wider buffer stays one)."""
    if t.stride(0) == t.shape[1]:
        return t.to(DEV)
    buf = torch.zeros(t.shape[0], t.stride(0), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M, N, K, pad", SHAPES)
def test_integer_inputs_are_exact_and_normal_inputs_inside_the_bound(M, N, K, pad, dtype):
    ld = K + pad if pad else None
    for scale in (False, True):
        x, w = lr.int_inputs(M, N, K, dtype, seed=M + N + K, row_scale=scale, ldx=ld, ldw=ld)
        got = launch(dev(x), [dev(w)], pad=pad)[0]
        want = lr.exact(x, w)
        wrong = (got.cpu() != want)
        assert not wrong.any(), (f"{int(wrong.sum())} of {wrong.numel()} elements differ from the exact product "
                                 f"(row scale {scale}), first at {wrong.nonzero()[0].tolist()}")
    x, w = lr.normal_inputs(M, N, K, dtype, seed=N + K, ldx=ld, ldw=ld)
    xd, wd = dev(x), dev(w)
    got = launch(xd, [wd], pad=pad)[0]
    ref, bound = lr.ref64_bound(x, w)
    worst = assert_within_bounds(f"decode linear {M}x{N}x{K}", got.cpu(), ref, bound, dims="sd")
    print(f"{dtype} {M}x{N}x{K}: worst err / bound {worst:.3f}")
    assert torch.equal(launch(xd, [wd], pad=pad)[0], got)                  # two launches, equal bits


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N, K", [(64, 544), (32, 14336)])
def test_a_row_depends_on_that_row_alone(N, K, dtype):
    x, w = lr.normal_inputs(16, N, K, dtype, seed=K)
    x, w = x.to(DEV), w.to(DEV)
    full = launch(x, [w])[0]
    perm = torch.tensor([5, 0, 15, 3, 9, 1, 14, 2, 8, 13, 4, 12, 7, 11, 6, 10], device=DEV)
    assert torch.equal(launch(x[perm].contiguous(), [w])[0], full[perm])
    assert torch.equal(launch(x[:1].contiguous(), [w])[0], full[:1])         # row 0 alone, M = 1
    assert torch.equal(launch(x[11:12].contiguous(), [w])[0], full[11:12])   # row 11 as row 0 of an M = 1 call
    for M in (1, 6, 13):
        # x as the first M rows of a 16-row buffer: NaN below gives the bits that zeros give
        zeros, nans = x.clone(), x.clone()
        zeros[M:] = 0
        nans[M:] = float("nan")
        a, b = launch(zeros[:M], [w])[0], launch(nans[:M], [w])[0]
        assert torch.equal(a, b) and torch.equal(a, full[:M]) and torch.isfinite(a).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_grouped_outputs_equal_the_single_calls(dtype):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 544, generator=g).to(dtype).to(DEV)
    ws = [torch.randn(n, 544, generator=g).to(dtype).to(DEV) for n in (64, 32, 32)]
    singles = [launch(x, [w])[0] for w in ws]
    for n_out in (3, 2):
        for got, want in zip(launch(x, ws[:n_out]), singles):
            assert torch.equal(got, want)
    for got, want in zip(launch(x, [ws[1], ws[0]]), (singles[1], singles[0])):      # the order is the caller's
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M, N, K, span", [(16, 64, 544, None), (4, 1024, 512, None), (16, 64, 544, 120.0)])
def test_swiglu_epilogue_equals_the_three_launch_chain(M, N, K, span, dtype):
    """decode_linear twice, then the existing fused SwiGLU forward: equal bits. ``span``: x is scaled so that the
    gate reaches about +-span, which is past smt_sigmoid's denormal guard (-87.3) and on its saturated side."""
    g = torch.Generator().manual_seed(K + N)
    x = torch.randn(M, K, generator=g)
    wg, wu = (torch.randn(N, K, generator=g).to(dtype).to(DEV) for _ in range(2))
    if span is not None:
        x = x * (span / (x.to(dtype).double() @ wg.cpu().double().t()).abs().max().item())
    x = x.to(dtype).to(DEV)
    with torch.no_grad():
        gate, up = fl.decode_linear(x, wg), fl.decode_linear(x, wu)
        want = fl.FusedSwiGLUFn.apply(gate, up)
        if span is not None:
            assert gate.min().item() < -90 and gate.max().item() > 90
        got = launch(x, [wg, wu], _hip.SKINNY_SWIGLU)[0]
        assert torch.equal(got, want)
        assert torch.equal(fl.decode_swiglu(x, wg, wu), want)


def test_wrappers_count_their_launches_and_refuse_what_does_not_qualify():
    x = torch.randn(2, 3, 64, device=DEV).bfloat16()
    ws = [torch.randn(n, 64, device=DEV).bfloat16() for n in (32, 16, 48)]
    fl.decode_linear_stats.reset()
    with torch.no_grad():
        y = fl.decode_linear(x, ws[0])
        assert y.shape == (2, 3, 32) and torch.equal(y.view(6, 32), launch(x.view(6, 64), [ws[0]])[0])
        q, k, v = fl.decode_linear_group(x, ws)
        assert q.shape == (2, 3, 32) and k.shape == (2, 3, 16) and v.shape == (2, 3, 48)
        assert torch.equal(q, y) and fl.decode_swiglu(x, ws[0], ws[0]).shape == (2, 3, 32)
        assert fl.decode_linear_stats.as_dict() == {"single": 1, "group": 1, "swiglu": 1}
        with pytest.raises(RuntimeError, match="17 rows"):
            fl.decode_linear(torch.zeros(17, 64, device=DEV).bfloat16(), ws[0])
    with pytest.raises(RuntimeError, match="gradients"):
        fl.decode_linear(x, ws[0])
    assert fl.decode_linear_stats.as_dict() == {"single": 1, "group": 1, "swiglu": 1}
