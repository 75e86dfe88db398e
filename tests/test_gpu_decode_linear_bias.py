"""The bias epilogue of the decode-linear kernel (smt_linear_skinny_bias, include/smt_linear.h) on the GPU, held
to the contract its header states with the two bars of tests/linear_bias_ref.py: integer inputs must be
torch.equal to the int64 sum rounded once (the planted 257 + 1 and 259 + 4 among them), normal inputs must lie
inside the derived per-element bound of the fp64 value.

The shapes are the smallest at which the epilogue or its indexing can go wrong: M 1, 5, 16; K 32 (one step, seven
idle waves) and 544 (17 steps in uneven slices); one tile, three tiles, and a group of 16 + 8 + 8 tiles with
three biases, with the middle one only and with none.

Every y is a view of a 16-row buffer wider than N that is pre-filled with a sentinel, and everything outside
[0, M) x [0, N) must still hold it afterwards; every bias is a view, at a 16-byte boundary, of a buffer whose
other elements are NaN, so a read outside [0, N) that reached an output would show in it."""
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_bias_ref as br
from tests.attn_ref import assert_within_bounds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 77.0
MS, KS = (1, 5, 16), (32, 544)
# (the outputs' N, which of them have a bias)
OUTPUTS = {"n16": ((16,), (True,)), "n48": ((48,), (True,)),
           "group_3_biases": ((256, 128, 128), (True, True, True)),
           "group_middle_bias": ((256, 128, 128), (False, True, False)),
           "group_no_bias": ((256, 128, 128), (False, False, False))}


def framed_bias(b):
    """A device copy of b [N] as elements [8, 8 + N) of a NaN-filled buffer (16-byte aligned, like the buffer)."""
    if b is None:
        return None
    buf = torch.full((b.shape[0] + 16,), float("nan"), dtype=b.dtype, device=DEV)
    buf[8:8 + b.shape[0]] = b
    return buf[8:8 + b.shape[0]]


def launch(x, weights, biases, epilogue=_hip.SKINNY_PLAIN):
    """The kernel's outputs for device x [M, K], device weights and framed device biases (None: the unbiased
    entry point), written into sentinel-filled [16, N + 8] buffers whose outside is checked."""
    M = x.shape[0]
    bufs = [torch.full((16, w.shape[0] + 8), SENTINEL, dtype=x.dtype, device=DEV) for w in weights]
    outs = [b[:M, :w.shape[0]] for b, w in zip(bufs, weights)]
    got = _hip.linear_skinny(x, list(weights), epilogue, outs, biases=biases)
    torch.cuda.synchronize()
    for b, w in zip(bufs, weights):
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[:M, :w.shape[0]] = False
        assert bool((b[outside] == SENTINEL).all()), "the kernel wrote outside [0, M) x [0, N)"
    return [g.clone() for g in got]


def to_dev(x, ws, bs):
    return x.to(DEV), [w.to(DEV) for w in ws], [framed_bias(b) for b in bs]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(OUTPUTS))
def test_integer_inputs_are_exact_and_normal_inputs_inside_the_bound(name, dtype):
    Ns, biased = OUTPUTS[name]
    for M in MS:
        for K in KS:
            x, ws, bs = br.int_inputs(M, Ns, K, dtype, seed=M + K + len(Ns), biased=biased)
            xd, wd, bd = to_dev(x, ws, bs)
            got = launch(xd, wd, bd)
            plain = launch(xd, wd, None)
            for i, (g, w, b) in enumerate(zip(got, ws, bs)):
                want = br.exact(x, w, b)
                wrong = g.cpu() != want
                assert not wrong.any(), (f"M {M} K {K} output {i}: {int(wrong.sum())} of {wrong.numel()} elements differ "
                                         f"from the exact sum, first at {wrong.nonzero()[0].tolist()}")
                if dtype == torch.bfloat16:                  # the planted elements, in so many words
                    assert g[M - 1, -1].item() == (258.0 if b is not None else 256.0)
                    assert g[M - 1, 0].item() == (264.0 if b is not None else 260.0)
                if b is None:                                # a NULL entry: smt_linear_skinny's bits
                    assert torch.equal(g, plain[i])
            x, ws, bs = br.normal_inputs(M, Ns, K, dtype, seed=K + M, biased=biased)
            xd, wd, bd = to_dev(x, ws, bs)
            got = launch(xd, wd, bd)
            plain = launch(xd, wd, None)
            for i, (g, w, b) in enumerate(zip(got, ws, bs)):
                ref, bound = br.ref64_bound(x, w, b)
                worst = assert_within_bounds(f"decode linear + bias {M}x{w.shape[0]}x{K} output {i}", g.cpu(), ref, bound, dims="sd")
                print(f"{dtype} {name} M {M} K {K} output {i}: worst err / bound {worst:.3f}")
                if b is None:
                    assert torch.equal(g, plain[i])
                else:
                    assert not torch.equal(g, plain[i])
            for a, b in zip(launch(xd, wd, bd), got):        # two launches, equal bits
                assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_grouped_outputs_equal_the_single_calls(dtype):
    x, ws, bs = br.normal_inputs(5, (256, 128, 128), 544, dtype, seed=3)
    xd, wd, bd = to_dev(x, ws, bs)
    singles = [launch(xd, [w], [b])[0] for w, b in zip(wd, bd)]
    for got, want in zip(launch(xd, wd, bd), singles):
        assert torch.equal(got, want)
    got = launch(xd, [wd[1], wd[0]], [bd[1], None])                                   # the order is the caller's
    assert torch.equal(got[0], singles[1]) and torch.equal(got[1], launch(xd, [wd[0]], None)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
def test_a_row_depends_on_that_row_alone(K, dtype):
    Ns, biased = (256, 128, 128), (True, False, True)
    x, ws, bs = br.normal_inputs(16, Ns, K, dtype, seed=K, biased=biased)
    xd, wd, bd = to_dev(x, ws, bs)
    full = launch(xd, wd, bd)
    perm = torch.tensor([5, 0, 15, 3, 9, 1, 14, 2, 8, 13, 4, 12, 7, 11, 6, 10], device=DEV)
    for got, want in zip(launch(xd[perm].contiguous(), wd, bd), full):
        assert torch.equal(got, want[perm])
    for got, want in zip(launch(xd[11:12].contiguous(), wd, bd), full):                # row 11 as row 0 of an M = 1 call
        assert torch.equal(got, want[11:12])
    for M in (1, 5, 13):
        zeros, nans = xd.clone(), xd.clone()
        zeros[M:] = 0
        nans[M:] = float("nan")
        for a, b, want in zip(launch(zeros[:M], wd, bd), launch(nans[:M], wd, bd), full):
            assert torch.equal(a, b) and torch.equal(a, want[:M]) and torch.isfinite(a).all()


def test_refusals_return_before_the_launch_with_a_message():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 64, generator=g).bfloat16().to(DEV)
    w = torch.randn(32, 64, generator=g).bfloat16().to(DEV)
    b = framed_bias(torch.randn(32, generator=g).bfloat16())
    with pytest.raises(RuntimeError, match=r"status -1.*PLAIN"):
        _hip.linear_skinny(x, [w, w], _hip.SKINNY_SWIGLU, biases=[b, None])
    odd = torch.zeros(40, dtype=torch.bfloat16, device=DEV)[1:33]
    with pytest.raises(RuntimeError, match=r"status -2.*align"):
        _hip.linear_skinny(x, [w], biases=[odd])
    with pytest.raises(RuntimeError, match="bias 0 must be"):
        _hip.linear_skinny(x, [w], biases=[b.float()])
    lib = _hip.load()
    y = torch.full((4, 32), SENTINEL, dtype=torch.bfloat16, device=DEV)
    desc = (_hip.SkinnyOut * 1)(_hip.SkinnyOut(w=w.data_ptr(), ldw=64, y=y.data_ptr(), ldy=32, N=32))
    rc = lib.smt_linear_skinny_bias(x.data_ptr(), 64, 4, 64, _hip.DTYPE_BF16, desc, None, 1, _hip.SKINNY_PLAIN, None,
                                    torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == -1 and "null biases" in lib.smt_linear_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                                                # nothing ran
    # SWIGLU with every entry NULL is smt_linear_skinny's launch
    with torch.no_grad():
        assert torch.equal(_hip.linear_skinny(x, [w, w], _hip.SKINNY_SWIGLU, biases=[None, None])[0],
                           _hip.linear_skinny(x, [w, w], _hip.SKINNY_SWIGLU)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_a_captured_call_replays_the_same_bits(dtype):
    x, ws, bs = br.normal_inputs(5, (256, 128, 128), 544, dtype, seed=9, biased=(True, False, True))
    xd, wd, bd = to_dev(x, ws, bs)
    want = launch(xd, wd, bd)
    x2 = torch.randn(5, 544, generator=torch.Generator().manual_seed(10)).to(dtype).to(DEV)
    want2 = launch(x2, wd, bd)
    static_x = xd.clone()
    outs = [torch.full((5, n), SENTINEL, dtype=dtype, device=DEV) for n in (256, 128, 128)]
    _hip.linear_skinny(static_x, wd, outs=outs, biases=bd)                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.linear_skinny(static_x, wd, outs=outs, biases=bd)
    for inp, expect in ((xd, want), (x2, want2), (xd, want)):
        static_x.copy_(inp)
        for o in outs:
            o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, expect):
            assert torch.equal(o, e)


def test_wrappers_count_biased_launches_and_refuse_what_does_not_qualify():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 64, generator=g).bfloat16().to(DEV)
    ws = [torch.randn(n, 64, generator=g).bfloat16().to(DEV) for n in (32, 16, 48)]
    bs = [torch.randn(n, generator=g).bfloat16().to(DEV) for n in (32, 16, 48)]
    fl.decode_linear_stats.reset()
    with torch.no_grad():
        y = fl.decode_linear(x, ws[0], bs[0])
        assert y.shape == (2, 3, 32) and torch.equal(y.view(6, 32), launch(x.view(6, 64), [ws[0]], [bs[0]])[0])
        assert (fl.decode_linear_stats.single, fl.decode_linear_stats.bias) == (1, 1)
        q, k, v = fl.decode_linear_group(x, ws, [bs[0], None, bs[2]])
        assert torch.equal(q, y) and torch.equal(k, fl.decode_linear_group(x, ws)[1])
        assert torch.equal(v, fl.decode_linear(x, ws[2], bs[2]))
        assert fl.decode_linear_stats.as_dict() == {"single": 2, "group": 2, "swiglu": 0} and fl.decode_linear_stats.bias == 3
        fl.decode_linear_group(x, ws, [None, None, None])                              # no bias: not counted as one
        assert fl.decode_linear_stats.bias == 3 and fl.decode_linear_stats.group == 3
        with pytest.raises(RuntimeError, match="bias stride or alignment"):
            fl.decode_linear(x, ws[0], torch.zeros(40, dtype=torch.bfloat16, device=DEV)[1:33])
        with pytest.raises(RuntimeError, match="bias torch.float32"):
            fl.decode_linear(x, ws[0], bs[0].float())
    with pytest.raises(RuntimeError, match="gradients"):
        fl.decode_linear(x, ws[0], bs[0])
    assert fl.decode_linear_stats.bias == 3
