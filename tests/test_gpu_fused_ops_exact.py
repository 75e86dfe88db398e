"""Every kernel of csrc/llama_kernels.hip (RMSNorm and its residual-add / weight-gradient variants, RoPE,
SwiGLU, cross entropy) against the chain references of tests/fused_ops_ref.py, element by element
(``assert_chain_close``: one output step plus the derived slack, no NaN, at most 1e-3 of the elements
different at all), through the C ABI so that leading dimensions, strided outputs and the per-row
statistics are reachable. Outputs are windows of NaN-prefilled buffers: a stray write, or an element
left unwritten, shows. Inputs are drawn on the CPU, where the references are computed once per shape."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import fused_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5


def _ids(v):
    return str(v).replace("torch.", "")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _code(t):
    return _hip.dtype_code16(t.dtype, "test")


def _call(name, *args):
    _hip._check(getattr(_hip.load(), name)(*args, _stream()), name)


def _win(rows, H, dt, ld=None, fill=None):
    return R.Sentinel(rows, H, dt, DEV, ld=ld, fill=fill)


def _in(t, ld):
    """An input on the device: contiguous, or (ld) a window of a NaN-filled buffer of that leading dimension."""
    return t.to(DEV) if ld is None else _win(t.shape[0], t.shape[1], t.dtype, ld, t.to(DEV)).win


# ------------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------------
class _NormCase:
    """Inputs drawn once per (dtype, rows, hidden); each reference computed on first use and kept."""

    def __init__(self, dt, rows, H):
        g = torch.Generator().manual_seed(rows * 10007 + H)
        self.dt, self.rows, self.H = dt, rows, H
        self.x = (torch.randn(rows, H, generator=g) * 2).to(dt)
        self.res = (torch.randn(rows, H, generator=g) * 3).to(dt)
        self.w = (torch.randn(H, generator=g) * 0.2 + 1.0).to(dt)
        self.dy = torch.randn(rows, H, generator=g).to(dt)
        self.dres = torch.randn(rows, H, generator=g).to(dt)

    @functools.cached_property
    def fwd(self):
        return R.rmsnorm_fwd(self.x, self.w, EPS)                     # (x, y, rstd)

    @functools.cached_property
    def fwd_add(self):
        return R.rmsnorm_fwd(self.x, self.w, EPS, self.res)           # (h, y, rstd)

    @functools.cached_property
    def rstd(self):
        ss = self.x.double().pow(2).sum(-1).float()                   # rmsnorm_fwd's rstd, without its y
        return 1.0 / torch.sqrt(ss / float(self.H) + torch.tensor(EPS, dtype=torch.float32))

    @functools.cached_property
    def dx(self):
        return R.rmsnorm_bwd(self.dy, self.x, self.w, self.rstd)

    @functools.cached_property
    def dx_add(self):
        return R.rmsnorm_bwd(self.dy, self.x, self.w, self.rstd, self.dres)

    @functools.cached_property
    def dw(self):
        return R.rmsnorm_dw(self.dy, self.x, self.rstd)


@functools.lru_cache(maxsize=None)
def _norm_ref(dt, rows, H):
    return _NormCase(dt, rows, H)


def _run_fwd(c, ld=None, add=False):
    x, w = _in(c.x, ld), c.w.to(DEV)
    y = _win(c.rows, c.H, c.dt, ld)
    rstd = torch.full((c.rows + 2,), float("nan"), device=DEV)
    if add:
        res, h = _in(c.res, ld), _win(c.rows, c.H, c.dt, ld)
        _call("smt_add_rmsnorm_fwd", x.data_ptr(), x.stride(0), res.data_ptr(), res.stride(0), w.data_ptr(),
              h.win.data_ptr(), h.ld, y.win.data_ptr(), y.ld, rstd.data_ptr(), c.rows, c.H, EPS, _code(x))
        h.check("add_rmsnorm h")
        assert torch.equal(h.win.cpu(), c.fwd_add[0]), "h = dt(x + residual)"
    else:
        _call("smt_rmsnorm_fwd", x.data_ptr(), x.stride(0), w.data_ptr(), y.win.data_ptr(), y.ld, rstd.data_ptr(),
              c.rows, c.H, EPS, _code(x))
    torch.cuda.synchronize()
    y.check("rmsnorm y")
    assert torch.isnan(rstd[c.rows:]).all(), "rstd written past its rows"
    _, y_ref, r_ref = c.fwd_add if add else c.fwd
    what = f"{'add_' if add else ''}rmsnorm_fwd {_ids(c.dt)} [{c.rows}, {c.H}] ld {ld}"
    R.assert_rows_close(rstd[:c.rows], r_ref, r_ref.slack, what + " rstd")
    R.assert_chain_close(y.win.cpu(), y_ref, y_ref.slack, what + " y")


def _run_bwd(c, ld=None, add=False, dw=False, check_dx=True):
    """One of smt_rmsnorm_bwd (dw or not), smt_rmsnorm_bwd_add, smt_rmsnorm_bwd_add_dw, on the
    reference's rstd; returns (dx, dw) on the device."""
    x, dy, w, rstd = _in(c.x, ld), _in(c.dy, ld), c.w.to(DEV), c.rstd.to(DEV)
    dx = _win(c.rows, c.H, c.dt, ld)
    lib = _hip.load()
    dwo = partial = None
    if dw:
        partial = torch.full((lib.smt_rmsnorm_bwd_waves(c.rows) + 1, c.H), float("nan"), device=DEV)
        dwo = _win(1, c.H, c.dt)
    pp, pw = (partial.data_ptr(), dwo.win.data_ptr()) if dw else (None, None)
    if add:
        dres = _in(c.dres, ld)
        head = (dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), w.data_ptr(), rstd.data_ptr(), dres.data_ptr(),
                dres.stride(0), dx.win.data_ptr(), dx.ld)
        if dw:
            _call("smt_rmsnorm_bwd_add_dw", *head, pp, pw, c.rows, c.H, _code(x))
        else:
            _call("smt_rmsnorm_bwd_add", *head, c.rows, c.H, _code(x))
    else:
        _call("smt_rmsnorm_bwd", dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), w.data_ptr(), rstd.data_ptr(),
              dx.win.data_ptr(), dx.ld, pp, pw, c.rows, c.H, _code(x))
    torch.cuda.synchronize()
    what = f"rmsnorm_bwd{'_add' if add else ''}{'_dw' if dw else ''} {_ids(c.dt)} [{c.rows}, {c.H}] ld {ld}"
    dx.check(what + " dx")
    if check_dx:
        ref = c.dx_add if add else c.dx
        R.assert_chain_close(dx.win.cpu(), ref, ref.slack, what + " dx")
    if dw:
        dwo.check(what + " dw")
        assert torch.isnan(partial[-1]).all(), what + ": dw_partial written past smt_rmsnorm_bwd_waves(rows) rows"
        R.assert_chain_close(dwo.win[0].cpu(), c.dw, c.dw.slack, what + " dw")
    return dx.win.clone(), (dwo.win[0].clone() if dw else None)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("k", range(1, 17))
def test_rmsnorm_register_resident_instances(dt, k):
    """Every rmsnorm_fwd_reg_kernel<CPL, ADD> and rmsnorm_bwd_reg_kernel<CPL, ADD>, CPL 1..16 (fp32 rows up
    to 8, packed rows above, one wave per SIMD above 10): 9 rows = two full workgroups and a one-wave
    tail. The weight gradient rides on the same dx kernels, bit for bit."""
    c = _norm_ref(dt, 9, 512 * k)
    _run_fwd(c)
    _run_fwd(c, add=True)
    dx, _ = _run_bwd(c)
    dxa, _ = _run_bwd(c, add=True)
    dx2, dw = _run_bwd(c, dw=True)
    dxa2, dwa = _run_bwd(c, add=True, dw=True)
    assert torch.equal(dx, dx2) and torch.equal(dxa, dxa2) and torch.equal(dw, dwa)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("H", [8, 72, 520, 640, 3200, 8200, 8704])
def test_rmsnorm_generic_kernels(dt, rows, H):
    """rmsnorm_fwd_kernel / rmsnorm_bwd_kernel (hidden % 512 != 0 or > 8192): one chunk, fewer chunks
    than lanes, 65 chunks (lane 0 takes two), and sizes beside the register-resident range; with the
    weight gradient (rmsnorm_dw_rows_kernel takes any hidden % 8 == 0) the same dx."""
    c = _norm_ref(dt, rows, H)
    _run_fwd(c)
    dx, _ = _run_bwd(c)
    dx2, _ = _run_bwd(c, dw=True)
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_rmsnorm_generic_backward_second_trip_of_the_row_loop(dt):
    """rows > 4096 = smt_rmsnorm_bwd_waves' cap: the first three waves take a second row."""
    assert _hip.load().smt_rmsnorm_bwd_waves(4099) == 4096
    _run_bwd(_norm_ref(dt, 4099, 72))


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("H", [512, 640, 5120])
@pytest.mark.parametrize("wide", [False, True], ids=["ld_H+8", "ld_2H"])
def test_rmsnorm_leading_dimensions(dt, H, wide):
    """Every input and output a column slice of a wider NaN-filled buffer (ld = H + 8 or 2 H)."""
    c = _norm_ref(dt, 9, H)
    ld = max(2 * H, H + 8) if wide else H + 8
    _run_fwd(c, ld)
    _run_bwd(c, ld)
    _run_bwd(c, ld, dw=True)
    if H % 512 == 0:
        _run_fwd(c, ld, add=True)
        _run_bwd(c, ld, add=True)
        _run_bwd(c, ld, add=True, dw=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("H", [512, 640, 1536])
@pytest.mark.parametrize("rows", [63, 64, 65, 4161])
def test_rmsnorm_weight_gradient_per_column(dt, rows, H):
    """dw per column against the fp64 sum of the rounded terms: one chunk of rows, the 64-row floor, two
    chunks, and 66 chunks (rows_per_chunk 64 with 4161 rows: the second stage crosses kDwChunk). 640:
    the generic dx kernel beside the same dw kernels."""
    c = _norm_ref(dt, rows, H)
    _, dw = _run_bwd(c, dw=True)
    if H % 512 == 0:
        _, dwa = _run_bwd(c, add=True, dw=True, check_dx=False)      # its dx: the tests above
        assert torch.equal(dw, dwa)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("k", [8, 9])
def test_rmsnorm_bwd_add_is_bwd_then_add(dt, k):
    """smt_rmsnorm_bwd_add = smt_rmsnorm_bwd followed by the model-dtype add, bit for bit: CPL 8 (the
    residual gradient preloaded) and CPL 9 (packed rows, loaded in the second pass)."""
    c = _norm_ref(dt, 9, 512 * k)
    dx, _ = _run_bwd(c)
    dxa, _ = _run_bwd(c, add=True)
    assert torch.equal(dxa, dx + c.dres.to(DEV))


# ------------------------------------------------------------------------------------------------
# RoPE
# ------------------------------------------------------------------------------------------------
HEADS = [(8, 8), (32, 8), (16, 8), (8, 2), (9, 3), (1, 1)]        # three for rope_hg_kernel, three for rope_kernel


@functools.lru_cache(maxsize=None)
def _rope_ref(dt, S, D, B=3, heads=40):
    g = torch.Generator().manual_seed(S * 1000 + D)
    c = SimpleNamespace(B=B, S=S, D=D)
    c.t = torch.randn(B, S, heads, D, generator=g).to(dt)            # storage [B, S, heads, D]
    # positions that differ per batch row, as from position_ids restarting inside packed rows
    pos = torch.stack([(torch.arange(S) + 11 * b) % max(S - 3 * b, 1) for b in range(B)]).float()
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    emb = torch.cat((pos[..., None] * inv,) * 2, dim=-1)
    c.cos, c.sin = emb.cos().to(dt), emb.sin().to(dt)
    v = c.t.transpose(1, 2)
    c.out = {False: R.rope(v, c.cos, c.sin), True: R.rope(v, c.cos, c.sin, bwd=True)}
    c.out1 = {False: R.rope(v, c.cos[:1], c.sin[:1]), True: R.rope(v, c.cos[:1], c.sin[:1], bwd=True)}
    return c


def _desc(inp, out):
    sb, sh, ss, sd = inp.stride()
    ob, oh, os_, od = out.stride()
    assert sd == 1 and od == 1
    return _hip.RopeTensor(inp.data_ptr(), out.data_ptr(), sb, sh, ss, ob, oh, os_, inp.shape[1], 0)


def _padded4(shape, dt):
    """A [B, heads, S, D] window (d offset 8) of a NaN-filled [B, heads, S + 1, D + 8] buffer."""
    B, Hh, S, D = shape
    buf = torch.full((B, Hh, S + 1, D + 8), R.PATTERN, dtype=torch.int16, device=DEV)
    return buf, buf.view(dt)[:, :, :S, 8:]


def _padded4_check(buf, what):
    b = buf.clone()
    b[:, :, :-1, 8:] = R.PATTERN
    assert bool((b == R.PATTERN).all()), what + ": wrote outside its window"


def _rope_call(bwd, q, qo, k, ko, cos, sin):
    B, _, S, D = q.shape
    if cos.shape[0] != B:
        cos, sin = cos.expand(B, -1, -1), sin.expand(B, -1, -1)
    dq, dk = _desc(q, qo), _desc(k, ko)
    _call("smt_rope_bwd" if bwd else "smt_rope_fwd", ctypes.byref(dq), ctypes.byref(dk), cos.data_ptr(), sin.data_ptr(),
          cos.stride(0), cos.stride(1), B, S, D, _hip.dtype_code16(q.dtype, "test"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", [16, 32, 48, 64, 128, 256])
@pytest.mark.parametrize("S", [1, 33, 97])
def test_rope_equals_reference(dt, S, D):
    """smt_rope_fwd / smt_rope_bwd, both kernels, bit for bit: S * D / 16 threads per head row is never a
    multiple of 256 (a partial last workgroup), cos / sin differ per batch row. Per head pair: q as the
    transposed [B, S, H, D] view written in its own layout, k contiguous [B, H, S, D] written into a
    NaN-padded buffer of other strides; then the [1, S, D] zero-stride cos / sin, and in place."""
    c = _rope_ref(dt, S, D)
    cos, sin = c.cos.to(DEV), c.sin.to(DEV)
    t = c.t.to(DEV)
    for Hq, Hk in HEADS:
        for bwd in (False, True):
            what = f"rope {'bwd' if bwd else 'fwd'} {_ids(dt)} S {S} D {D} heads ({Hq}, {Hk})"
            q = t[:, :, :Hq].transpose(1, 2)                          # [B, Hq, S, D] view of [B, S, Hq.., D]
            k = t[:, :, Hq:Hq + Hk].transpose(1, 2).contiguous()     # contiguous [B, Hk, S, D]
            rq, rk = c.out[bwd][:, :Hq].to(DEV), c.out[bwd][:, Hq:Hq + Hk].to(DEV)
            qo = torch.empty_strided(q.shape, q.stride(), dtype=dt, device=DEV)
            kbuf, ko = _padded4(k.shape, dt)
            _rope_call(bwd, q, qo, k, ko, cos, sin)
            assert torch.equal(qo, rq), what + " q"
            assert torch.equal(ko, rk), what + " k (strided output)"
            _padded4_check(kbuf, what)
            # one [1, S, D] table for the batch, batch stride 0; outputs contiguous from a transposed q
            qo1 = torch.empty(q.shape, dtype=dt, device=DEV)
            ko1 = torch.empty_like(k)
            _rope_call(bwd, q, qo1, k, ko1, cos[:1], sin[:1])
            assert torch.equal(qo1, c.out1[bwd][:, :Hq].to(DEV)), what + " q, shared cos / sin"
            assert torch.equal(ko1, c.out1[bwd][:, Hq:Hq + Hk].to(DEV)), what + " k, shared cos / sin"
            # in place
            qi, ki = q.clone(memory_format=torch.preserve_format), k.clone()
            _rope_call(bwd, qi, qi, ki, ki, cos, sin)
            assert torch.equal(qi, rq) and torch.equal(ki, rk), what + " in place"


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("Hq,Hk", [(16, 8), (9, 3)])
def test_fused_apply_rotary_pos_emb_equals_reference(dt, Hq, Hk):
    """The autograd wrapper (and _rope_launch's in_place) on per-row cos / sin, S 33, D 64."""
    c = _rope_ref(dt, 33, 64)
    cos, sin, t = c.cos.to(DEV), c.sin.to(DEV), c.t.to(DEV)
    q = t[:, :, :Hq].transpose(1, 2).detach().requires_grad_(True)
    k = t[:, :, Hq:Hq + Hk].transpose(1, 2).detach().requires_grad_(True)
    oq, ok = fl.fused_apply_rotary_pos_emb(q, k, cos, sin)
    assert torch.equal(oq, c.out[False][:, :Hq].to(DEV)) and torch.equal(ok, c.out[False][:, Hq:Hq + Hk].to(DEV))
    # the reference's backward of the same tensor as upstream gradient
    torch.autograd.backward([oq, ok], [q.detach(), k.detach()])
    assert torch.equal(q.grad, c.out[True][:, :Hq].to(DEV)) and torch.equal(k.grad, c.out[True][:, Hq:Hq + Hk].to(DEV))
    qi, ki = q.detach().clone(memory_format=torch.preserve_format), k.detach().clone(memory_format=torch.preserve_format)
    ro, ko = fl._rope_launch("smt_rope_fwd", qi, ki, cos, sin, in_place=True)
    assert ro.data_ptr() == qi.data_ptr() and torch.equal(qi, oq) and torch.equal(ki, ok)


# ------------------------------------------------------------------------------------------------
# SwiGLU
# ------------------------------------------------------------------------------------------------
def _swiglu_run(gate, up, dh, what):
    n = gate.numel()
    dt = gate.dtype
    g, u, d = (_win(1, n, dt, fill=t.to(DEV)[None]) for t in (gate, up, dh))
    h, dg, du = (_win(1, n, dt) for _ in range(3))
    _call("smt_swiglu_fwd", g.win.data_ptr(), u.win.data_ptr(), h.win.data_ptr(), n, _code(gate))
    _call("smt_swiglu_bwd", g.win.data_ptr(), u.win.data_ptr(), d.win.data_ptr(), dg.win.data_ptr(), du.win.data_ptr(), n,
          _code(gate))
    torch.cuda.synchronize()
    for o, name in ((h, "h"), (dg, "dg"), (du, "du")):
        o.check(f"{what} {name}")
    rh = R.swiglu_fwd(gate, up)
    rdg, rdu = R.swiglu_bwd(gate, up, dh)
    outs = (h.win[0].cpu(), dg.win[0].cpu(), du.win[0].cpu())
    for got, ref, name in zip(outs, (rh, rdg, rdu), ("h", "dg", "du")):
        R.assert_chain_close(got, ref, ref.slack, f"{what} {name}")
    return outs


def _distinct_values(dt, n, g):
    """n distinct values of dt with 2^-6 <= |v| < 16, in random order. (Normal draws repeat in bf16: 2048
    of them hit a few hundred values, and a gate whose silu lies on a rounding tie, such as 5.9375, then
    flips in every copy at once, which the cap on differing elements counts as so many.)"""
    pos = torch.arange(0, 1 << 15, dtype=torch.int32).to(torch.int16).view(dt)
    pos = pos[(pos.float() >= 2.0 ** -6) & (pos.float() < 16.0)]
    vals = torch.cat((pos, -pos))
    assert len(vals) >= n
    return vals[torch.randperm(len(vals), generator=g)[:n]]


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("n8", [1, 255, 256, 257])
def test_swiglu_against_reference(dt, n8):
    """smt_swiglu_fwd / _bwd at one chunk, one chunk short of a workgroup, exactly one, and one over
    (`if (i >= n8) return` fires in three of them); NaN sentinels past n."""
    g = torch.Generator().manual_seed(n8)
    up, dh = (torch.randn(8 * n8, generator=g).to(dt) for _ in range(2))
    _swiglu_run(_distinct_values(dt, 8 * n8, g), up, dh, f"swiglu {_ids(dt)} n {8 * n8}")


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_swiglu_edge_values(dt):
    """gate at +-0, +-2^-126, +-20, +-88, +-89, +-104 (exp overflows fp32 between 88 and 89, exp2's
    argument passes 128 and 150), +-1e4 and +-max, crossed with up and grad_out at +-1 and +-max. Where
    the sigmoid is below the fp32 normal range the reference's slack is absolute (2^-126 |gate| times
    the factor that follows). No output is NaN where the eager chain's is not."""
    big = torch.finfo(dt).max
    edge = [0.0, 2.0 ** -126, 20.0, 88.0, 89.0, 104.0, 1e4, big]
    gv = torch.tensor([s * v for v in edge for s in (1.0, -1.0)], dtype=torch.float64)
    ov = torch.tensor([1.0, -1.0, big, -big], dtype=torch.float64)
    gate = gv[:, None, None].expand(-1, 4, 4).reshape(-1).to(dt)
    up = ov[None, :, None].expand(len(gv), -1, 4).reshape(-1).to(dt)
    dh = ov[None, None, :].expand(len(gv), 4, -1).reshape(-1).to(dt)
    outs = _swiglu_run(gate, up, dh, f"swiglu edge values {_ids(dt)}")
    ge, ue = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    he = torch.nn.functional.silu(ge) * ue
    he.backward(dh)
    for got, eager, name in zip(outs, (he.detach(), ge.grad, ue.grad), ("h", "dg", "du")):
        extra = torch.isnan(got) & ~torch.isnan(eager)
        assert not extra.any(), (name, gate[extra].tolist(), up[extra].tolist(), dh[extra].tolist())


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
IGNORE = -100


@functools.lru_cache(maxsize=None)
def _ce_ref(dt, V):
    g = torch.Generator().manual_seed(V)
    c = SimpleNamespace(V=V, rows=5)
    x = torch.randn(5, V, generator=g) * 4
    x[0, 1::3] = float("-inf")                       # some logits at -inf (not the label's)
    x[2] = float("-inf")
    x[2, V - 8] = 1.5                                # a single finite logit, the label's
    c.logits = x.to(dt)
    # column 0; the last column; the first column of the last chunk; ignored; out of range
    c.labels = torch.tensor([0, V - 1, V - 8, IGNORE, V + 3])
    c.scale = torch.tensor([1.0 / 3.0], dtype=torch.float32)
    c.lse, c.loss = R.ce_fwd(c.logits, c.labels, IGNORE)
    c.d = R.ce_bwd(c.logits, c.labels, c.lse, c.scale.item(), IGNORE)
    return c


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("pad", [0, 64], ids=["ld_V", "ld_V+64"])
@pytest.mark.parametrize("V", [8, 2040, 2048, 2056, 6152, 8192, 8200])
def test_cross_entropy_per_row(dt, V, pad):
    """smt_ce_fwd / smt_ce_bwd per row. V / 8 = 1, 255, 256, 257 (the single-chunk loops: below, at and
    past one trip per thread; at 257 the 2x unrolled backward loop takes its first trip), 769 (the 4x
    unrolled forward loop's first trip, by thread 0 alone), 1024 (one full 4x trip) and 1025."""
    c = _ce_ref(dt, V)
    what = f"ce {_ids(dt)} V {V} ld {V + pad}"
    ld = V + pad if pad else None
    logits = _in(c.logits, ld)
    labels, scale = c.labels.to(DEV), c.scale.to(DEV)
    lse = torch.full((c.rows + 2,), float("nan"), device=DEV)
    loss = torch.full((c.rows + 2,), 7.0, device=DEV)
    _call("smt_ce_fwd", logits.data_ptr(), logits.stride(0), labels.data_ptr(), c.rows, V, IGNORE, lse.data_ptr(),
          loss.data_ptr(), _code(logits))
    torch.cuda.synchronize()
    assert torch.isnan(lse[c.rows:]).all() and (loss[c.rows:] == 7.0).all(), what + ": wrote past its rows"
    R.assert_rows_close(lse[:c.rows], c.lse, c.lse.bound, what + " lse")
    R.assert_rows_close(loss[:c.rows], c.loss, c.loss.bound, what + " loss")
    assert torch.isnan(loss[4]) and loss[3] == 0, loss

    ref_lse = c.lse.to(DEV)
    if pad:
        d = _win(c.rows, V, dt, V + pad)
        out, ldd = d.win, d.ld
    else:
        out = torch.full((c.rows + 1, V), float("nan"), dtype=dt, device=DEV)
        ldd = V
    _call("smt_ce_bwd", logits.data_ptr(), logits.stride(0), labels.data_ptr(), ref_lse.data_ptr(), scale.data_ptr(),
          c.rows, V, IGNORE, out.data_ptr(), ldd, _code(logits))
    torch.cuda.synchronize()
    if pad:
        d.check(what + " dlogits")
    else:
        assert torch.isnan(out[c.rows]).all(), what + ": dlogits written past its rows"
    got = out[:c.rows].clone()
    R.assert_chain_close(got.cpu(), c.d, c.d.slack, what + " dlogits")
    assert not got[3].any(), what + ": gradient on an ignored row"

    # in place (dlogits == logits, ld_d == ld): bit-identical to the out-of-place gradient
    inp = _win(c.rows, V, dt, V + 64, c.logits.to(DEV)) if pad else None
    buf = inp.win if pad else c.logits.to(DEV).clone()
    _call("smt_ce_bwd", buf.data_ptr(), buf.stride(0), labels.data_ptr(), ref_lse.data_ptr(), scale.data_ptr(),
          c.rows, V, IGNORE, buf.data_ptr(), buf.stride(0), _code(logits))
    torch.cuda.synchronize()
    if pad:
        inp.check(what + " in place")
    assert torch.equal(buf.view(torch.int16), got.view(torch.int16)), what + " in place"
