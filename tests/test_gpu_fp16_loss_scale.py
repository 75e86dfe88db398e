"""The fp16 fused ops at the gradient magnitudes a loss-scaled step hands them.

The native engine trains an fp16 model under a dynamic loss scale (engine.backward:
``(loss.float() * scale).backward()``, scale 2^16 down to 1). tests/test_gpu_fused_fp16.py feeds every
fused backward unit-magnitude gradients; here the upstream gradients sit at the two ends of what the
scale produces, where fp16's range (normal down to 6.1e-5, subnormal step 6e-8, inf above 65504)
decides the result, and an inf / nan is put in to see that an overflowed step stays visible to the
loss scaler (it reads inf / nan in the tile gradients).

The error bar is the one tests/test_gpu_cross_entropy.py uses for the fused head: the relative L2
error of the fused op against an fp64 truth computed from the same fp16 operands must stay within
1.5 x the error of transformers' eager fp16 chain on those operands, measured in the same test (both
printed). No error constant is written down in advance; the attention keeps the floor of its
existing test, ``max(8e-3, 1.5 x sdpa)`` against an fp32 reference. Shapes are the smallest at
which the effect is large (N = 4096 rows x V = 8192: a non-label ``dlogits`` entry of a unit
upstream gradient is p / N ~ 3e-8, below fp16's smallest subnormal)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from sparse_matrix_tuning_amd import fused_llama as fl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H16 = torch.float16
SMALL, LARGE = 2.0 ** -12, 2.0 ** 8           # upstream gradient magnitudes: the ends of a dynamic scale


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _ulp_close(a, b, max_ulp_frac=1e-3):
    """tests/test_gpu_fused_fp16.py's criterion: fp16 tensors equal except for a small fraction
    differing by more than one rounding step (11 bits)."""
    a, b = a.float(), b.float()
    bad = ((a - b).abs() > b.abs() * 2 ** -10 + 6e-8).float().mean().item()
    return bad <= max_ulp_frac, bad


def _step_close(a, b, max_frac=1e-3):
    """Within one fp16 step of the reference value's binade, subnormals included: 2^-24 below 2^-14,
    |b| 2^-10 above, and no absolute slack (a kernel that flushed subnormals to zero fails)."""
    a, b = a.float(), b.float()
    tol = torch.where(b.abs() < 2.0 ** -14, torch.full_like(b, 2.0 ** -24), b.abs() * 2.0 ** -10)
    bad = ((a - b).abs() > tol).float().mean().item()
    return bad <= max_frac, bad


def _same_finite(a, b):
    return torch.equal(torch.isfinite(a), torch.isfinite(b))


def _covers_nonfinite(fused, eager):
    """Every element that is inf / nan in eager is inf / nan in the fused result (and eager has some)."""
    lost = (~torch.isfinite(eager) & torch.isfinite(fused)).sum().item()
    return lost == 0 and not torch.isfinite(eager).all().item(), lost


def _poisoned(g, value, index):
    g = g.clone()
    g[index] = value
    return g


# ------------------------------------------------------------------------------------------------
# (a) the fused LM head + loss under a loss scale
# ------------------------------------------------------------------------------------------------
HEAD = dict(B=2, S=2048, H=256, V=8192)


class _Head:
    def __init__(self, w, wt):
        self.weight = w
        if wt is not None:
            w._smt_weight_t = wt


@functools.lru_cache(maxsize=None)
def _head_case():
    """Operands as tests/test_gpu_cross_entropy.py::_head_operands builds them, in fp16, and the fp64
    truth of d loss / d hidden and d loss / d W for a unit upstream gradient (a power-of-two loss
    scale multiplies it exactly). Computed once; nothing below writes to it."""
    B, S, H, V = HEAD["B"], HEAD["S"], HEAD["H"], HEAD["V"]
    g = torch.Generator(device=DEV).manual_seed(B * S + V)
    h = torch.randn(B, S, H, device=DEV, generator=g).to(H16)
    w = (torch.randn(V, H, device=DEV, generator=g) * H ** -0.5 * 2).to(H16)
    labels = torch.randint(0, V, (B, S), device=DEV, generator=g)
    labels[0, : S // 7] = -100
    labels[1, 1000:1009] = -100
    x64 = h.double().reshape(-1, H).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    shift = F.pad(labels, (0, 1), value=-100)[..., 1:].reshape(-1)
    F.cross_entropy(x64 @ w64.t(), shift, ignore_index=-100, reduction="mean").backward()
    return h, w, w.t().contiguous(), labels, x64.grad.view(B, S, H), w64.grad


@functools.lru_cache(maxsize=None)
def _head_eager(scale):
    """transformers' eager fp16 chain on the same operands: F.linear, ForCausalLMLoss, x scale."""
    from transformers.loss.loss_utils import ForCausalLMLoss
    h, w, _wt, labels, _dh, _dw = _head_case()
    x, w2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    loss = ForCausalLMLoss(F.linear(x, w2), labels, vocab_size=w.shape[0])
    (loss * scale).backward()
    return loss.detach(), x.grad, w2.grad


def _head_unfused(transposed, scale):
    """The pair ``patch_llama(model, lm_head_loss=False)`` runs: the engine's FrozenLinearFn (or
    F.linear without a transposed copy), then the fused cross entropy."""
    from sparse_matrix_tuning_amd.engine import FrozenLinearFn
    h, w, wt, labels, _dh, _dw = _head_case()
    x = h.clone().requires_grad_(True)
    logits = FrozenLinearFn.apply(x, w, wt, None) if transposed else F.linear(x, w)
    loss = fl.fused_causal_lm_loss(logits, labels, vocab_size=w.shape[0])
    (loss * scale).backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("scale", [2.0 ** 16, 2.0 ** 8, 1.0])
@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("chunk", [1024, 4096])
def test_lm_head_loss_fp16_under_loss_scale(chunk, transposed, scale):
    """dh of the fused head at upstream gradient ``scale`` against the fp64 truth, within 1.5 x eager
    fp16's error (at scale 1 eager itself underflows: the bar then says "no worse than eager").

    At scale 2^16 it also equals the unfused pair's dh up to single rounding steps: with N = 4096 the
    fused head's internal ``dlogits`` scale, 2^(ceil(log2(denom)) + 4) / denom, is the very number
    2^16 / denom the unfused pair folds in, so the two differ only through the GEMM kernel chosen for
    the chunk shape, as in bf16. At the smaller scales the unfused pair's own ``dlogits`` (256 x and
    65536 x smaller) lose their subnormal entries, and the near-zero elements of dh move by more than a
    step (measured: 1.0e-2 of the elements at 2^8, 4.7e-1 at 1): printed, and held by the bar above."""
    h, w, wt, labels, dh64, _dw64 = _head_case()
    truth = dh64 * scale
    loss_e, dh_e, _ = _head_eager(scale)
    x = h.clone().requires_grad_(True)
    loss = fl.fused_lm_head_loss(x, _Head(w.clone(), wt if transposed else None), labels, chunk_rows=chunk)
    (loss * scale).backward()
    e_fused, e_eager = _rel(x.grad, truth), _rel(dh_e, truth)
    loss_u, dh_u = _head_unfused(transposed, scale)
    ok, bad = _ulp_close(x.grad, dh_u)
    print(f"chunk {chunk} transposed {transposed} scale {scale:g}: dh vs fp64 fused {e_fused:.3e}, eager {e_eager:.3e}; "
          f"vs the unfused pair: bit-identical {torch.equal(x.grad, dh_u)}, off by more than a step {bad:.2e}")
    assert x.grad.dtype == H16 and abs(loss.item() - loss_e.item()) <= 1e-3 * abs(loss_e.item())
    assert abs(loss.item() - loss_u.item()) <= 1e-6 * abs(loss_u.item())
    assert e_fused <= 1.5 * e_eager, (e_fused, e_eager)
    if scale == 2.0 ** 16:
        assert ok, bad


def test_lm_head_loss_fp16_trainable_head_under_loss_scale(monkeypatch):
    """The warm-up's trainable head at scale 2^16: dW from the fp32 accumulator over four chunks, and
    dh, each within 1.5 x eager of the fp64 truth and a rounding step from the unfused pair's."""
    monkeypatch.setattr(fl, "LM_HEAD_DW_CHUNK_ROWS", 0)
    scale = 2.0 ** 16
    h, w, _wt, labels, dh64, dw64 = _head_case()
    _loss_e, dh_e, dw_e = _head_eager(scale)
    x0, w0 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (fl.fused_causal_lm_loss(F.linear(x0, w0), labels, vocab_size=w.shape[0]) * scale).backward()
    x1, w1 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (fl.fused_lm_head_loss(x1, _Head(w1, None), labels, chunk_rows=1024) * scale).backward()
    for name, mine, unfused, eager, truth in (("dh", x1.grad, x0.grad, dh_e, dh64 * scale),
                                              ("dW", w1.grad, w0.grad, dw_e, dw64 * scale)):
        e_fused, e_eager = _rel(mine, truth), _rel(eager, truth)
        ok, bad = _ulp_close(mine, unfused)
        print(f"trainable head, scale 2^16, {name} vs fp64: fused {e_fused:.3e}, eager {e_eager:.3e}; vs the "
              f"unfused pair: bit-identical {torch.equal(mine, unfused)}, off by more than a step {bad:.2e}")
        assert mine.dtype == H16 and e_fused <= 1.5 * e_eager, (name, e_fused, e_eager)
        assert ok, (name, bad)


# ------------------------------------------------------------------------------------------------
# (b) the unfused fp16 cross entropy at the same magnitudes
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ce_case():
    torch.manual_seed(9)
    N, V = 4096, 8192
    logits = (torch.randn(N, V, device=DEV) * 2).to(H16)
    labels = torch.randint(0, V, (N,), device=DEV)
    labels[::7] = -100
    return logits, labels


def _ce_pair(scale):
    """(loss, dlogits) of eager (F.cross_entropy on the fp32 copy) and of FusedCrossEntropyFn."""
    logits, labels = _ce_case()
    le = logits.clone().requires_grad_(True)
    loss_e = F.cross_entropy(le.float(), labels, ignore_index=-100)
    (loss_e * scale).backward()
    lf = logits.clone().requires_grad_(True)
    denom = (labels != -100).sum().to(torch.float32)
    loss_f = fl.FusedCrossEntropyFn.apply(lf, labels, -100, denom)
    (loss_f * scale).backward()
    return loss_e.detach(), le.grad, loss_f.detach(), lf.grad


@pytest.mark.parametrize("scale", [2.0 ** 16, 1.0])
def test_cross_entropy_fp16_rounds_to_nearest_into_subnormals(scale):
    """At scale 1 a non-label gradient is p / N ~ 3e-8 .. 1e-6: fp16 subnormals, or below the smallest
    one. Eager rounds the fp32 gradient to nearest, subnormals included; the kernel's fp16 store must
    do the same, to one step of the reference value's binade with no absolute slack."""
    loss_e, g_e, loss_f, g_f = _ce_pair(scale)
    zero = (g_e == 0).float().mean().item()
    sub = ((g_e != 0) & (g_e.abs().float() < 2.0 ** -14)).float().mean().item() / max(1.0 - zero, 1e-30)
    ok, bad = _step_close(g_f, g_e)
    print(f"scale {scale:g}: eager's dlogits {zero:.1%} zero, {sub:.1%} of the others subnormal; fused off by more "
          f"than one step of the binade {bad:.2e}; bit-identical {torch.equal(g_f, g_e)}")
    assert abs(loss_f.item() - loss_e.item()) <= 1e-5 * abs(loss_e.item())
    assert g_f.dtype == H16 and ok, bad
    if scale == 1.0:
        assert sub > 0.9 and zero < 0.9       # the case is about subnormals: the non-zero outputs are


# ------------------------------------------------------------------------------------------------
# (c) the other fused fp16 backwards at loss-scaled magnitudes; (d) inf / nan stay visible
# ------------------------------------------------------------------------------------------------
def _bar(name, fused, eager, truth, floor=0.0):
    e_fused, e_eager = _rel(fused, truth), _rel(eager, truth)
    print(f"{name}: fused {e_fused:.3e}, eager {e_eager:.3e}")
    assert e_fused <= max(floor, 1.5 * e_eager), (name, e_fused, e_eager)


def _rmsnorm64(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


@functools.lru_cache(maxsize=None)
def _rmsnorm_case(H):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    torch.manual_seed(H)
    norm = LlamaRMSNorm(H, eps=1e-5).to(DEV).to(H16)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(H) * 0.2 + 1.0)
    x = (torch.randn(3, 257, H, device=DEV) * 3).to(H16)
    dy = torch.randn(3, 257, H, device=DEV)
    return norm, x, dy


def _rmsnorm_run(norm, x, dy):
    """((y, dx, dw) of eager, the same of the fused op) for the fp16 upstream gradient dy."""
    out = []
    for fused in (False, True):
        norm.weight.grad = None
        xi = x.clone().requires_grad_(True)
        y = fl.FusedRMSNormFn.apply(xi, norm.weight, norm.variance_epsilon) if fused else norm(xi)
        y.backward(dy)
        out.append((y.detach(), xi.grad, norm.weight.grad.clone()))
    norm.weight.grad = None
    return out


@pytest.mark.parametrize("mag", [SMALL, LARGE])
@pytest.mark.parametrize("H", [512, 4096])
def test_rmsnorm_fp16_backward_at_loss_scaled_magnitudes(H, mag):
    norm, x, dy = _rmsnorm_case(H)
    dy = (dy * mag).to(H16)
    (_ye, dx_e, dw_e), (_yf, dx_f, dw_f) = _rmsnorm_run(norm, x, dy)
    x64, w64 = x.double().requires_grad_(True), norm.weight.detach().double().requires_grad_(True)
    _rmsnorm64(x64, w64, norm.variance_epsilon).backward(dy.double())
    _bar(f"rmsnorm H {H} dy x {mag:g} dx", dx_f, dx_e, x64.grad)
    _bar(f"rmsnorm H {H} dy x {mag:g} dw", dw_f, dw_e, w64.grad)
    if mag == LARGE:
        assert _same_finite(dx_f, dx_e) and _same_finite(dw_f, dw_e)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_rmsnorm_fp16_backward_keeps_inf_and_nan(value):
    norm, x, dy = _rmsnorm_case(512)
    dy = _poisoned(dy.to(H16), value, (1, 100, 37))
    (_ye, dx_e, dw_e), (_yf, dx_f, dw_f) = _rmsnorm_run(norm, x, dy)
    for name, f, e in (("dx", dx_f, dx_e), ("dw", dw_f, dw_e)):
        ok, lost = _covers_nonfinite(f, e)
        assert ok, (name, lost)
    assert torch.isfinite(dx_f[0]).all() and torch.isfinite(dx_f[1, :100]).all()      # other rows untouched


def test_rmsnorm_fp16_forward_overflows_to_inf_like_eager():
    """A weight that lifts y beyond 65504: inf where eager's fp16 product is inf, not a saturated 65504."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    torch.manual_seed(21)
    H = 512
    norm = LlamaRMSNorm(H, eps=1e-5).to(DEV).to(H16)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(H) * 0.2 + 1.0)
        norm.weight[::5] = 30000.0
        norm.weight[1::5] = -30000.0
    x = (torch.randn(2, 65, H, device=DEV) * 3).to(H16)
    with torch.no_grad():
        ye, yf = norm(x), fl.FusedRMSNormFn.apply(x, norm.weight, norm.variance_epsilon)
    assert torch.isinf(ye).sum().item() > 100
    assert torch.equal(torch.isinf(yf), torch.isinf(ye)) and torch.equal(yf[torch.isinf(ye)], ye[torch.isinf(ye)])
    ok, bad = _ulp_close(yf[torch.isfinite(ye)], ye[torch.isfinite(ye)])
    assert ok, bad


@functools.lru_cache(maxsize=None)
def _add_rmsnorm_case():
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    torch.manual_seed(5)
    H = 4096
    norm = LlamaRMSNorm(H, eps=1e-5).to(DEV).to(H16)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(H) * 0.2 + 1.0)
    x, r = (torch.randn(2, 133, H, device=DEV) * 2).to(H16), (torch.randn(2, 133, H, device=DEV) * 3).to(H16)
    return norm, x, r, torch.randn(2, 133, H, device=DEV), torch.randn(2, 133, H, device=DEV)


def _add_rmsnorm_run(norm, x, r, dh, dy, weight_grad):
    out = []
    norm.weight.requires_grad_(weight_grad)
    try:
        for fused in (False, True):
            norm.weight.grad = None
            xi, ri = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
            if fused:
                h, y = fl.FusedAddRMSNormFn.apply(xi, ri, norm.weight, norm.variance_epsilon)
            else:
                h = ri + xi
                y = norm(h)
            torch.autograd.backward([h, y], [dh, dy])
            out.append((h.detach(), xi.grad, ri.grad, norm.weight.grad.clone() if weight_grad else None))
    finally:
        norm.weight.grad = None
        norm.weight.requires_grad_(True)
    return out


@pytest.mark.parametrize("mag", [SMALL, LARGE])
@pytest.mark.parametrize("weight_grad", [False, True])
def test_add_rmsnorm_fp16_backward_at_loss_scaled_magnitudes(weight_grad, mag):
    """Truth: fp64 of the norm on the fp16 sum h both sides produce (bit-identical), plus dh."""
    norm, x, r, dh, dy = _add_rmsnorm_case()
    dh, dy = (dh * mag).to(H16), (dy * mag).to(H16)
    (h_e, dx_e, dr_e, dw_e), (h_f, dx_f, dr_f, dw_f) = _add_rmsnorm_run(norm, x, r, dh, dy, weight_grad)
    assert torch.equal(h_f, h_e)
    h64, w64 = h_e.double().requires_grad_(True), norm.weight.detach().double().requires_grad_(True)
    _rmsnorm64(h64, w64, norm.variance_epsilon).backward(dy.double())
    truth = h64.grad + dh.double()
    tag = f"add+rmsnorm weight_grad {weight_grad} grads x {mag:g}"
    _bar(tag + " dx", dx_f, dx_e, truth)
    _bar(tag + " dresidual", dr_f, dr_e, truth)
    if weight_grad:
        _bar(tag + " dw", dw_f, dw_e, w64.grad)
    if mag == LARGE:
        assert _same_finite(dx_f, dx_e) and _same_finite(dr_f, dr_e)
        assert not weight_grad or _same_finite(dw_f, dw_e)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("weight_grad", [False, True])
@pytest.mark.parametrize("into", ["dh", "dy"])
def test_add_rmsnorm_fp16_backward_keeps_inf_and_nan(into, weight_grad, value):
    norm, x, r, dh, dy = _add_rmsnorm_case()
    dh, dy = dh.to(H16), dy.to(H16)
    if into == "dh":
        dh = _poisoned(dh, value, (1, 7, 4000))
    else:
        dy = _poisoned(dy, value, (1, 7, 4000))
    (_he, dx_e, dr_e, dw_e), (_hf, dx_f, dr_f, dw_f) = _add_rmsnorm_run(norm, x, r, dh, dy, weight_grad)
    pairs = [("dx", dx_f, dx_e), ("dresidual", dr_f, dr_e)]
    if weight_grad and into == "dy":
        pairs.append(("dw", dw_f, dw_e))
    for name, f, e in pairs:
        ok, lost = _covers_nonfinite(f, e)
        assert ok, (name, lost)
    assert torch.isfinite(dx_f[0]).all()


@functools.lru_cache(maxsize=None)
def _swiglu_case():
    torch.manual_seed(2)
    g = (torch.randn(4, 100, 1536, device=DEV) * 3).to(H16)
    u = torch.randn(4, 100, 1536, device=DEV).to(H16)
    return g, u, torch.randn(4, 100, 1536, device=DEV)


def _swiglu_run(g, u, dh):
    out = []
    for fused in (False, True):
        gi, ui = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        h = fl.FusedSwiGLUFn.apply(gi, ui) if fused else F.silu(gi) * ui
        h.backward(dh)
        out.append((h.detach(), gi.grad, ui.grad))
    return out


@pytest.mark.parametrize("mag", [SMALL, LARGE])
def test_swiglu_fp16_backward_at_loss_scaled_magnitudes(mag):
    g, u, dh = _swiglu_case()
    dh = (dh * mag).to(H16)
    (_he, dg_e, du_e), (_hf, dg_f, du_f) = _swiglu_run(g, u, dh)
    g64, u64 = g.double().requires_grad_(True), u.double().requires_grad_(True)
    (F.silu(g64) * u64).backward(dh.double())
    _bar(f"swiglu dh x {mag:g} dgate", dg_f, dg_e, g64.grad)
    _bar(f"swiglu dh x {mag:g} dup", du_f, du_e, u64.grad)
    if mag == LARGE:
        assert _same_finite(dg_f, dg_e) and _same_finite(du_f, du_e)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_swiglu_fp16_backward_keeps_inf_and_nan(value):
    g, u, dh = _swiglu_case()
    dh = _poisoned(dh.to(H16), value, (2, 50, 777))
    (_he, dg_e, du_e), (_hf, dg_f, du_f) = _swiglu_run(g, u, dh)
    for name, f, e in (("dgate", dg_f, dg_e), ("dup", du_f, du_e)):
        ok, lost = _covers_nonfinite(f, e)
        assert ok, (name, lost)
        assert torch.isfinite(f).sum().item() == f.numel() - 1            # that element and no other


def test_swiglu_fp16_forward_overflows_to_inf_like_eager():
    """silu(gate) * up beyond 65504: +-inf where eager's fp16 product is, not a saturated 65504."""
    g, u, _dh = _swiglu_case()
    g, u = g.clone(), u.clone()
    g[0, 0, :64] = 300.0
    u[0, 0, :32] = 300.0
    u[0, 0, 32:64] = -300.0
    g[1, 1, :16], u[1, 1, :16] = 256.0, 255.75             # 65472: the largest products that stay finite
    with torch.no_grad():
        he, hf = F.silu(g) * u, fl.FusedSwiGLUFn.apply(g, u)
    assert torch.isinf(he).sum().item() == 64 and torch.isfinite(he[1, 1, :16]).all()
    assert torch.equal(torch.isinf(hf), torch.isinf(he)) and torch.equal(hf[0, 0, :64], he[0, 0, :64])
    ok, bad = _ulp_close(hf[torch.isfinite(he)], he[torch.isfinite(he)])
    assert ok, bad


@functools.lru_cache(maxsize=None)
def _rope_case():
    torch.manual_seed(1)
    B, S, D, Hq, Hk = 2, 96, 128, 8, 2
    q = torch.randn(B, S, Hq * D, device=DEV).to(H16).view(B, S, Hq, D).transpose(1, 2)
    k = torch.randn(B, S, Hk * D, device=DEV).to(H16).view(B, S, Hk, D).transpose(1, 2)
    pos = torch.arange(S, device=DEV, dtype=torch.float32)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2, device=DEV, dtype=torch.float32) / D))
    emb = torch.cat((torch.outer(pos, inv),) * 2, dim=-1)
    return q, k, emb.cos()[None].to(H16), emb.sin()[None].to(H16), torch.randn(B, Hq, S, D, device=DEV), \
        torch.randn(B, Hk, S, D, device=DEV)


def _rope_run(q, k, cos, sin, gq, gk):
    out = []
    for fn in (fl.eager_apply_rotary_pos_emb, fl.fused_apply_rotary_pos_emb):
        qi, ki = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        oq, ok_ = fn(qi, ki, cos, sin)
        torch.autograd.backward([oq, ok_], [gq, gk])
        out.append((qi.grad, ki.grad))
    return out


@pytest.mark.parametrize("mag", [SMALL, LARGE])
def test_rope_fp16_backward_bit_exact_at_loss_scaled_magnitudes(mag):
    """At 2^-12 the products g * cos, g * sin reach fp16's subnormals: still bit-identical to eager."""
    q, k, cos, sin, gq, gk = _rope_case()
    gq, gk = (gq * mag).to(H16), (gk * mag).to(H16)
    (dq_e, dk_e), (dq_f, dk_f) = _rope_run(q, k, cos, sin, gq, gk)
    assert torch.isfinite(dq_e).all() and torch.isfinite(dk_e).all()
    assert torch.equal(dq_f, dq_e) and torch.equal(dk_f, dk_e)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_rope_fp16_backward_keeps_inf_and_nan(value):
    q, k, cos, sin, gq, gk = _rope_case()
    gq, gk = _poisoned(gq.to(H16), value, (1, 3, 40, 10)), _poisoned(gk.to(H16), value, (0, 1, 90, 100))
    (dq_e, dk_e), (dq_f, dk_f) = _rope_run(q, k, cos, sin, gq, gk)
    for name, f, e in (("dq", dq_f, dq_e), ("dk", dk_f, dk_e)):
        ok, lost = _covers_nonfinite(f, e)
        assert ok, (name, lost)
    assert torch.isfinite(dq_f[0]).all() and torch.isfinite(dk_f[1]).all()


ATTN = dict(B=2, Hq=8, Hkv=2, S=256, D=128)


@functools.lru_cache(maxsize=None)
def _attn_case():
    torch.manual_seed(ATTN["S"] + ATTN["Hq"])
    B, Hq, Hkv, S, D = (ATTN[n] for n in ("B", "Hq", "Hkv", "S", "D"))
    mk = lambda heads: torch.randn(B, S, heads, D, device=DEV).to(H16).transpose(1, 2)
    return mk(Hq), mk(Hkv), mk(Hkv), torch.randn(B, S, Hq, D, device=DEV)


def _attn_run(q, k, v, g):
    """(dq, dk, dv) of torch's fp16 sdpa and of smt_flash for the fp16 upstream gradient g [B, S, Hq, D]."""
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    F.scaled_dot_product_attention(qs, ks, vs, is_causal=True, enable_gqa=True).transpose(1, 2).backward(g)
    qf, kf, vf = (t.clone().requires_grad_(True) for t in (q, k, v))
    fl.flash_attention(qf, kf, vf).backward(g)
    return (qs.grad, ks.grad, vs.grad), (qf.grad, kf.grad, vf.grad)


@pytest.mark.parametrize("mag", [SMALL, LARGE])
def test_flash_attention_fp16_backward_at_loss_scaled_magnitudes(mag):
    """The existing bar, max(8e-3, 1.5 x torch's fp16 sdpa) against an fp32 reference on the same
    fp16 inputs, with dO at 2^-12 (dS = P (dP - delta) reaches fp16's subnormals before the dQ / dK
    products) and at 2^8."""
    q, k, v, g = _attn_case()
    g = (g * mag).to(H16)
    G = ATTN["Hq"] // ATTN["Hkv"]
    sd, mine = _attn_run(q, k, v, g)
    q32, k32, v32 = (t.float().requires_grad_(True) for t in (q, k, v))
    ro = F.scaled_dot_product_attention(q32, k32.repeat_interleave(G, 1), v32.repeat_interleave(G, 1), is_causal=True,
                                        scale=ATTN["D"] ** -0.5)
    ro.transpose(1, 2).backward(g.float())
    for name, f, e, t in zip(("dq", "dk", "dv"), mine, sd, (q32.grad, k32.grad, v32.grad)):
        _bar(f"attention dO x {mag:g} {name}", f, e, t, floor=8e-3)
        if mag == LARGE:
            assert _same_finite(f, e), name


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_flash_attention_fp16_backward_keeps_inf_and_nan(value):
    """One inf / nan in dO (batch 1, head 5, row 100): the gradients of that batch x head (dq of head
    5, dk / dv of its kv head 1) are inf / nan wherever sdpa's are; the other batch stays finite."""
    q, k, v, g = _attn_case()
    g = _poisoned(g.to(H16), value, (1, 100, 5, 77))
    sd, mine = _attn_run(q, k, v, g)
    for name, f, e in zip(("dq", "dk", "dv"), mine, sd):
        ok, lost = _covers_nonfinite(f, e)
        assert ok, (name, lost)
        assert torch.isfinite(f[0]).all(), name
    assert not torch.isfinite(mine[0][1, 5, 100]).any()


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_cross_entropy_and_lm_head_loss_fp16_keep_inf_and_nan(value):
    """An inf / nan upstream gradient of the loss (what an overflowed scaled loss hands back): every
    gradient eager returns non-finite is non-finite from the fused cross entropy and the fused head."""
    _loss_e, g_e, _loss_f, g_f = _ce_pair(value)
    ok, lost = _covers_nonfinite(g_f, g_e)
    assert ok, lost
    h, w, wt, labels, _dh64, _dw64 = _head_case()
    _l, dh_e, _dw_e = _head_eager(value)
    for transposed in (True, False):
        x = h.clone().requires_grad_(True)
        loss = fl.fused_lm_head_loss(x, _Head(w.clone(), wt if transposed else None), labels, chunk_rows=1024)
        (loss * value).backward()
        ok, lost = _covers_nonfinite(x.grad, dh_e)
        assert ok, (transposed, lost)


# ------------------------------------------------------------------------------------------------
# (e) one step through the engine: its loss scale reaches the head
# ------------------------------------------------------------------------------------------------
def test_engine_fp16_step_hands_the_head_a_scaled_gradient():
    """A mini-LLaMA in fp16 under the engine's dynamic loss scale (the reference's fp16 block: scale
    2^16), N = 4096 rows x V = 4096. The gradient that leaves the fused head into the final norm,
    against 65536 x d loss / d hidden in fp64 from the captured hidden state, the head's weight and
    the shifted labels: within 1.5 x the error of eager fp16 (F.linear + ForCausalLMLoss, scaled) on
    that hidden state."""
    import bench
    from transformers.loss.loss_utils import ForCausalLMLoss
    from sparse_matrix_tuning_amd.engine import SMTFusedAdam, initialize
    from sparse_matrix_tuning_amd.smt import smt
    torch.manual_seed(3)
    model = bench.build_model("mini", DEV).to(H16)
    sel_mlp = {("gate_proj", 1): [(0, 0), (2, 1)], ("down_proj", 2): [(1, 0)]}
    sel_att = {("q_proj", 0): [(0, 1), (1, 0)], ("v_proj", 3): [(0, 0)]}
    ids = torch.randint(0, 4096, (2, 2048), generator=torch.Generator().manual_seed(5)).to(DEV)
    seen = {}

    def cap(_m, _inp, out):
        seen["hidden"] = out.detach().clone()
        out.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))

    counts = fl.patch_llama(model)
    try:
        assert counts["lm_head_loss"] == 1
        smt.freeze_unselected_matrix_layer(model, sel_mlp, sel_att)
        smt.convert_linear_layer_to_matrix_sparsity(model, sel_mlp, sel_att)
        opt = SMTFusedAdam(smt.get_optimizer_sparse_grouped_parameters(model, 0.0, 1e-4), lr=1e-4, betas=(0.9, 0.95))
        eng, *_ = initialize(model=model, optimizer=opt,
                             config={"gradient_clipping": 1.0, "fp16": {"enabled": True, "loss_scale_window": 100}})
        scale = eng.loss_scaler.scale
        assert scale == 2.0 ** 16
        hook = model.model.norm.register_forward_hook(cap)
        try:
            loss = eng(input_ids=ids, labels=ids, use_cache=False).loss
            eng.backward(loss)
            torch.cuda.synchronize()
        finally:
            hook.remove()
    finally:
        fl.unpatch_llama(model)
    hidden, got = seen["hidden"], seen["grad"]
    w = model.lm_head.weight.detach()
    V = w.shape[0]
    shift = F.pad(ids, (0, 1), value=-100)[..., 1:].reshape(-1)
    x64 = hidden.double().reshape(-1, hidden.shape[-1]).requires_grad_(True)
    truth_loss = F.cross_entropy(x64 @ w.double().t(), shift, ignore_index=-100, reduction="mean")
    (truth_loss * scale).backward()
    truth = x64.grad.view_as(hidden)
    xe = hidden.clone().requires_grad_(True)
    (ForCausalLMLoss(F.linear(xe, w), ids, vocab_size=V) * scale).backward()
    e_fused, e_eager = _rel(got, truth), _rel(xe.grad, truth)
    print(f"engine fp16 step, scale 2^16, N 4096 x V {V}: d loss / d hidden vs fp64 fused {e_fused:.3e}, "
          f"eager {e_eager:.3e}")
    assert got.dtype == H16 and abs(loss.item() - truth_loss.item()) <= 1e-3 * truth_loss.item()
    assert e_fused <= 1.5 * e_eager, (e_fused, e_eager)
