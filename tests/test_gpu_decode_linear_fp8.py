"""The e4m3 decode-linear kernel (smt_linear_skinny_fp8, include/smt_linear.h) on the GPU, held to the contracts
its header states, with the two bars of tests/linear_fp8_ref.py: integer inputs with scales that are not powers
of two must be torch.equal to the exact reference (the order of the two scale multiplications included), inputs
quantised by fp8.quant_rows must lie inside the derived per-element bound of the fp64 product of the bytes and
scales the call used.

Every launch reads x8 and sx from 16-row buffers whose rows >= M hold the NaN byte 0x7F and NaN scales, and
writes into a 16-row buffer wider than N that is pre-filled with a sentinel; everything outside [0, M) x [0, N)
must still hold it afterwards. Out-of-range behaviour is tested only with such poison values inside
allocations the test owns."""
import numpy as np
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fp8 as f8
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_fp8_ref as fr
from tests.attn_ref import assert_within_bounds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 77.0
NAN_BYTE = 0x7F


def dev_bytes(a, rows=None, fill=0):
    """A device uint8 view [a.shape] with the row stride of the numpy / torch array ``a``, as the first rows
    of a ``rows``-row buffer filled with ``fill``."""
    a = torch.from_numpy(np.ascontiguousarray(a)).view(torch.uint8) if isinstance(a, np.ndarray) else a.view(torch.uint8)
    return _place(a, rows, fill)


def _place(a, rows, fill):
    ld = a.stride(0) if a.dim() == 2 and a.stride(0) > a.shape[1] else a.shape[-1]
    buf = torch.full((rows or a.shape[0], ld), fill, dtype=torch.uint8, device=DEV)
    buf[:a.shape[0], :a.shape[1]] = a.to(DEV)
    return buf[:a.shape[0], :a.shape[1]]


def strided(a: np.ndarray, ld):
    """numpy [r, c] as a torch CPU view with row stride ``ld``."""
    t = torch.zeros(a.shape[0], ld, dtype=torch.uint8)
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
    return t[:, :a.shape[1]]


def dev_scales(s, rows=None, fill=float("nan")):
    s = torch.as_tensor(np.asarray(s) if not isinstance(s, torch.Tensor) else s, dtype=torch.float32)
    buf = torch.full((rows or s.numel(),), fill, dtype=torch.float32, device=DEV)
    buf[:s.numel()] = s.to(DEV)
    return buf[:s.numel()]


def launch(x8, sx, weights, dtype, epilogue=_hip.SKINNY_PLAIN, pad=0, poison=True):
    """The kernel's outputs for host or device x8 [M, K] / sx [M] and (w8, sw) pairs. x8 and sx become the first
    M rows of 16-row device buffers whose other rows are NaN (``poison``) or zero; the outputs are written into
    sentinel-filled [16, N + 8 + pad] buffers whose every element outside [0, M) x [0, N) is checked."""
    M = x8.shape[0]
    xd = dev_bytes(x8, 16, NAN_BYTE if poison else 0)
    sd = dev_scales(sx, 16, float("nan") if poison else 0.0)
    wd = [(w8 if isinstance(w8, torch.Tensor) and w8.device.type == "cuda" else dev_bytes(w8),
           sw if isinstance(sw, torch.Tensor) and sw.device.type == "cuda" else dev_scales(sw)) for w8, sw in weights]
    n_y = 1 if epilogue == _hip.SKINNY_SWIGLU else len(wd)
    bufs = [torch.full((16, w8.shape[0] + 8 + pad), SENTINEL, dtype=dtype, device=DEV) for w8, _ in wd[:n_y]]
    outs = [b[:M, :w[0].shape[0]] for b, w in zip(bufs, wd)]
    got = _hip.linear_skinny_fp8(xd, sd, wd, dtype, epilogue, outs)
    torch.cuda.synchronize()
    for b, (w8, _) in zip(bufs, wd):
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[:M, :w8.shape[0]] = False
        assert bool((b[outside] == SENTINEL).all()), "the kernel wrote outside [0, M) x [0, N)"
    return [g.clone() for g in got]


def _np(a, ld):
    return strided(a, ld) if ld else a


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M, N, K, pad", fr.CASES)
def test_integer_inputs_are_exact_and_quantised_inputs_inside_the_bound(M, N, K, pad, dtype):
    ld = K + pad if pad else None
    x8, sx, w8, sw = fr.int_inputs(M, N, K, seed=M + N + K)
    got = launch(_np(x8, ld), sx, [(_np(w8, ld), sw)], dtype, pad=pad)[0]
    want = fr.exact(x8, sx, w8, sw, dtype)
    wrong = got.cpu() != want
    assert not wrong.any(), (f"{int(wrong.sum())} of {wrong.numel()} elements differ from the exact reference, first at "
                             f"{wrong.nonzero()[0].tolist()}")
    if dtype == torch.bfloat16:
        assert got[M - 1, N - 1].item() == 260.0                    # the planted tie rounds to even
    # normal data quantised on the device: the bytes and scales the call uses are the ones read back here
    x, w = fr.normal_bf16(M, N, K, seed=N + K)
    xq, sxq = f8.quant_rows(x.to(DEV))
    wq, swq = f8.quant_rows(w.to(DEV))
    xq, wq = xq.view(torch.uint8), wq.view(torch.uint8)
    if ld:
        xq, wq = _place(strided(xq.cpu().numpy(), ld), None, 0), _place(strided(wq.cpu().numpy(), ld), None, 0)
    got = launch(xq, sxq, [(wq, swq)], dtype, pad=pad)[0]
    ref, bound = fr.ref64_bound(xq.cpu().numpy(), sxq.cpu().numpy(), wq.cpu().numpy(), swq.cpu().numpy(), dtype)
    worst = assert_within_bounds(f"fp8 decode linear {M}x{N}x{K}", got.cpu(), ref, bound, dims="sd")
    print(f"{dtype} {M}x{N}x{K}: worst err / bound {worst:.3f}")
    assert torch.equal(launch(xq, sxq, [(wq, swq)], dtype, pad=pad)[0], got)         # two launches, equal bits


def _quantised(M, N, K, seed):
    x, w = fr.normal_bf16(M, N, K, seed)
    xq, sx = f8.quant_rows(x.to(DEV))
    wq, sw = f8.quant_rows(w.to(DEV))
    return xq.view(torch.uint8), sx, wq.view(torch.uint8), sw


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N, K", [(48, 576), (16, 4160)])
def test_a_row_depends_on_that_row_alone(N, K, dtype):
    x8, sx, w8, sw = _quantised(16, N, K, seed=K)
    W = [(w8, sw)]
    full = launch(x8, sx, W, dtype)[0]
    perm = torch.tensor([5, 0, 15, 3, 9, 1, 14, 2, 8, 13, 4, 12, 7, 11, 6, 10], device=DEV)
    assert torch.equal(launch(x8[perm].contiguous(), sx[perm].contiguous(), W, dtype)[0], full[perm])
    assert torch.equal(launch(x8[:1], sx[:1], W, dtype)[0], full[:1])                 # row 0 alone, M = 1
    assert torch.equal(launch(x8[11:12], sx[11:12], W, dtype)[0], full[11:12])        # row 11 as row 0 of an M = 1 call
    for M in (1, 6, 13):
        # NaN bytes and NaN scales in rows >= M give the bits that zeros give
        a = launch(x8[:M], sx[:M], W, dtype, poison=False)[0]
        b = launch(x8[:M], sx[:M], W, dtype, poison=True)[0]
        assert torch.equal(a, b) and torch.equal(a, full[:M]) and torch.isfinite(a.float()).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_grouped_outputs_equal_the_single_calls(dtype):
    x8, sx, _, _ = _quantised(9, 16, 576, seed=11)
    ws = []
    for i, n in enumerate((32, 16, 16)):                                              # distinct sw per output
        _, _, w8, sw = _quantised(1, n, 576, seed=20 + i)
        ws.append((w8, sw * (1.0 + 0.37 * i)))
    singles = [launch(x8, sx, [w], dtype)[0] for w in ws]
    assert not torch.equal(singles[1], singles[2])
    for n_out in (3, 2):
        for got, want in zip(launch(x8, sx, ws[:n_out], dtype), singles):
            assert torch.equal(got, want)
    for got, want in zip(launch(x8, sx, [ws[1], ws[0]], dtype), (singles[1], singles[0])):
        assert torch.equal(got, want)
    # the integer bar on the group: each output against its own scales
    x8i, sxi, _, _ = fr.int_inputs(5, 16, 576, seed=3)
    wi = [fr.int_inputs(5, n, 576, seed=40 + n + i)[2:] for i, n in enumerate((32, 16, 16))]
    for got, (w8, sw) in zip(launch(x8i, sxi, wi, dtype), wi):
        assert torch.equal(got.cpu(), fr.exact(x8i, sxi, w8, sw, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M, N, K, span", [(16, 48, 576, None), (4, 1024, 512, None), (16, 48, 576, 120.0)])
def test_swiglu_epilogue_equals_the_three_launch_chain(M, N, K, span, dtype):
    """Two PLAIN calls, then the existing fused SwiGLU forward: equal bits. ``span``: the gate's scales are set so
    that it reaches about +-span, past smt_sigmoid's denormal guard (-87.3) and on its saturated side (seed 628:
    the gate's extremes are -120 and +118 there)."""
    x8, sx, wg, swg = _quantised(M, N, K, seed=628 if span else K + N)
    _, _, wu, swu = _quantised(1, N, K, seed=K + N + 1)
    gate = launch(x8, sx, [(wg, swg)], dtype)[0]
    if span is not None:
        swg = swg * (span / gate.float().abs().max().item())
        gate = launch(x8, sx, [(wg, swg)], dtype)[0]
        assert gate.min().item() < -90 and gate.max().item() > 90
    up = launch(x8, sx, [(wu, swu)], dtype)[0]
    with torch.no_grad():
        want = fl.FusedSwiGLUFn.apply(gate.contiguous(), up.contiguous())
    got = launch(x8, sx, [(wg, swg), (wu, swu)], dtype, _hip.SKINNY_SWIGLU)[0]
    assert torch.equal(got, want)


def test_error_codes_come_before_any_launch():
    lib = _hip.load()
    x8, sx, w8, sw = _quantised(4, 32, 128, seed=1)
    y = torch.full((4, 32), SENTINEL, dtype=torch.bfloat16, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(M=4, K=128, N=32, x=None, ldx=128, ldw=128, ldy=32, w=None):
        out = (_hip.SkinnyFp8Out * 1)(_hip.SkinnyFp8Out(w8=w or w8.data_ptr(), sw=sw.data_ptr(), ldw=ldw, y=y.data_ptr(), ldy=ldy, N=N))
        rc = lib.smt_linear_skinny_fp8(x or x8.data_ptr(), ldx, sx.data_ptr(), M, K, _hip.DTYPE_BF16, out, 1, 0, None, stream)
        return rc, lib.smt_linear_last_error().decode()

    for kw in (dict(M=0), dict(M=17), dict(K=96), dict(K=0), dict(N=24), dict(N=0)):
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
    for kw in (dict(x=x8.data_ptr() + 8), dict(w=w8.data_ptr() + 4), dict(ldx=136), dict(ldw=136), dict(ldy=36)):
        rc, msg = call(**kw)
        assert rc == -2 and "align" in msg, kw
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                                  # no launch happened
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(y, launch(x8, sx, [(w8, sw)], torch.bfloat16)[0])


def test_a_captured_call_replays_on_new_bytes():
    x8, sx, w8, sw = _quantised(5, 48, 576, seed=2)
    xb, sb = x8.clone(), sx.clone()
    y = torch.empty(5, 48, dtype=torch.bfloat16, device=DEV)
    _hip.linear_skinny_fp8(xb, sb, [(w8, sw)], torch.bfloat16, outs=[y])              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _hip.linear_skinny_fp8(xb, sb, [(w8, sw)], torch.bfloat16, outs=[y])
    for seed in (7, 8):
        x2, s2, _, _ = _quantised(5, 48, 576, seed=seed)
        xb.copy_(x2)
        sb.copy_(s2)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, launch(x2, s2, [(w8, sw)], torch.bfloat16)[0])


def test_wrappers_read_the_cached_copy_and_count_their_launches():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 256, generator=g).bfloat16().to(DEV)
    fws = [f8.Fp8Weight((torch.randn(n, 256, generator=g) * 0.05).bfloat16().to(DEV)) for n in (256, 256, 512)]
    fl.decode_fp8_stats.reset()
    fl.decode_linear_stats.reset()
    with torch.no_grad():
        y = fl.decode_linear_fp8(x, fws[0])                                           # quantises x: one launch, cached on x
        x8, sx = f8.quant_rows_cached(x)
        assert y.shape == (2, 3, 256)
        assert torch.equal(y.view(6, 256), launch(x8.view(torch.uint8), sx, [(fws[0].w8.view(torch.uint8), fws[0].sw)], torch.bfloat16)[0])
        q, k, v = fl.decode_linear_group_fp8(x, fws)                                  # finds the copy
        assert torch.equal(q, y) and k.shape == (2, 3, 256) and v.shape == (2, 3, 512)
        h = fl.decode_swiglu_fp8(x, fws[0], fws[1])
        assert torch.equal(h, fl.FusedSwiGLUFn.apply(q, k))
        assert fl.decode_fp8_stats.as_dict() == {"single": 1, "group": 1, "swiglu": 1, "quant": 1}
        # the kernel reads fw.w8 / fw.sw as they are at the call, not a copy of its own
        fws[0].sw.mul_(2.0)
        assert torch.equal(fl.decode_linear_fp8(x, fws[0]), y * 2)
        # against today's route (quant_rows + torch._scaled_mm): the same operands, another summation order
        ref = f8.fp8_linear_forward(x, fws[2]).float()
        assert (v.float() - ref).norm() <= 2.0 ** -7 * ref.norm()
        with pytest.raises(RuntimeError, match="17 rows"):
            fl.decode_linear_fp8(torch.zeros(17, 256, device=DEV).bfloat16(), fws[0])
    with pytest.raises(RuntimeError, match="gradients"):
        fl.decode_linear_fp8(x, fws[0])
    assert fl.decode_linear_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0}
