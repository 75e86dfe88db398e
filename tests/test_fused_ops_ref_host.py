"""The chain references of tests/fused_ops_ref.py against transformers on the CPU, and the checker
against planted faults (no GPU): every fault fails ``assert_chain_close`` / ``torch.equal``, and the
bar it replaces (``_ulp_close`` plus a whole-tensor norm ratio) is shown to pass some of them."""
import pytest
import torch

from tests import fused_ops_ref as R

DTYPES = [torch.bfloat16, torch.float16]


def _norm_case(dt, rows=9, H=1024, seed=0):
    g = torch.Generator().manual_seed(seed + H)
    x = (torch.randn(rows, H, generator=g) * 2).to(dt)
    w = (torch.randn(H, generator=g) * 0.2 + 1.0).to(dt)
    dy = torch.randn(rows, H, generator=g).to(dt)
    dres = torch.randn(rows, H, generator=g).to(dt)
    return x, w, dy, dres


def _rope_case(dt, B=3, heads=8, S=33, D=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, heads, D, generator=g).to(dt).transpose(1, 2)
    pos = torch.stack([(torch.arange(S) + 7 * b) % (S - 5 * b) for b in range(B)]).float()   # restarts per row
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    emb = torch.cat((pos[..., None] * inv,) * 2, dim=-1)
    return q, emb.cos().to(dt), emb.sin().to(dt)


def _ce_case(dt, rows=5, V=2056, seed=2):
    g = torch.Generator().manual_seed(seed + V)
    logits = (torch.randn(rows, V, generator=g) * 4).to(dt)
    labels = torch.tensor([0, V - 1, V - 8, -100, V // 2][:rows])
    return logits, labels


# ------------------------------------------------------------------------------------------------
# the references against transformers' eager chains
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_rope_reference_is_transformers_rope_bitwise(dt):
    from sparse_matrix_tuning_amd.fused_llama import eager_apply_rotary_pos_emb
    q, cos, sin = _rope_case(dt)
    k = q[:, :2].clone()
    qe, ke = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    oq, ok = eager_apply_rotary_pos_emb(qe, ke, cos, sin)
    assert torch.equal(oq, R.rope(q, cos, sin)) and torch.equal(ok, R.rope(k, cos, sin))
    gq, gk = torch.randn(oq.shape).to(dt), torch.randn(ok.shape).to(dt)
    torch.autograd.backward([oq, ok], [gq, gk])
    assert torch.equal(qe.grad, R.rope(gq, cos, sin, bwd=True)) and torch.equal(ke.grad, R.rope(gk, cos, sin, bwd=True))


@pytest.mark.parametrize("dt", DTYPES)
def test_swiglu_reference_is_eager_silu_times_up_bitwise(dt):
    g = torch.Generator().manual_seed(3)
    gate = (torch.randn(8 * 257, generator=g) * 3).to(dt)
    up = torch.randn(8 * 257, generator=g).to(dt)
    assert torch.equal(R.swiglu_fwd(gate, up), torch.nn.functional.silu(gate) * up)
    dh = torch.randn(8 * 257, generator=g).to(dt)
    ge, ue = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    (torch.nn.functional.silu(ge) * ue).backward(dh)
    dg, du = R.swiglu_bwd(gate, up, dh)
    R.assert_chain_close(ge.grad, dg, dg.slack, "eager dg")
    R.assert_chain_close(ue.grad, du, du.slack, "eager du")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [640, 1024])
def test_rmsnorm_reference_against_llama_rmsnorm(dt, H):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    x, w, dy, _ = _norm_case(dt, H=H)
    norm = LlamaRMSNorm(H, eps=1e-5).to(dt)
    with torch.no_grad():
        norm.weight.copy_(w)
    xe = x.clone().requires_grad_(True)
    ye = norm(xe)
    ye.backward(dy)
    _, y, rstd = R.rmsnorm_fwd(x, w, 1e-5)
    R.assert_chain_close(ye.detach(), y, y.slack, "eager y")
    dx = R.rmsnorm_bwd(dy, x, w, rstd)
    R.assert_chain_close(xe.grad, dx, dx.slack, "eager dx")
    dw = R.rmsnorm_dw(dy, x, rstd)
    R.assert_chain_close(norm.weight.grad, dw, dw.slack, "eager dw")


@pytest.mark.parametrize("dt", DTYPES)
def test_cross_entropy_reference_against_transformers_per_row(dt):
    from transformers.loss.loss_utils import ForCausalLMLoss
    logits, labels = _ce_case(dt)
    keep = labels != -100                      # the mean over an ignored row alone is 0 / 0
    logits, labels = logits[keep], labels[keep]
    V = logits.shape[1]
    x = logits.clone().requires_grad_(True)
    rows = torch.stack([ForCausalLMLoss(x[r:r + 1][None], None, V, shift_labels=labels[r:r + 1][None])
                        for r in range(len(labels))])
    rows.sum().backward()
    lse, loss = R.ce_fwd(logits, labels)
    R.assert_rows_close(rows.detach(), loss, loss.bound, "eager loss")
    d = R.ce_bwd(logits, labels, lse, 1.0)
    R.assert_chain_close(x.grad, d, d.slack, "eager dlogits")


# ------------------------------------------------------------------------------------------------
# planted faults
# ------------------------------------------------------------------------------------------------
def _nan_like(t):
    return torch.full(t.shape, R.PATTERN, dtype=torch.int16).view(t.dtype)


def _chunk_fault(t):
    t = t.clone()
    t[-2, 16:24] = t[-3, 16:24]
    return t


def _last_row_fault(t):
    t = t.clone()
    t[-1] = _nan_like(t[-1])
    return t


def _one_nan(t):
    t = t.clone()
    t.view(-1)[t.numel() // 3] = float("nan")
    return t


def _fails(actual, ref, what):
    with pytest.raises(AssertionError):
        R.assert_chain_close(actual, ref, ref.slack, what)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [640, 1024])
def test_checker_fails_planted_rmsnorm_faults(dt, H):
    x, w, dy, dres = _norm_case(dt, H=H)
    _, y, rstd = R.rmsnorm_fwd(x, w, 1e-5)
    dx = R.rmsnorm_bwd(dy, x, w, rstd)
    dxr = R.rmsnorm_bwd(dy, x, w, rstd, dres)
    for ref in (y, dx, dxr):
        R.assert_chain_close(ref.clone(), ref, ref.slack, "the reference itself")
        for fault in (_chunk_fault, _last_row_fault, _one_nan):
            _fails(fault(ref), ref, fault.__name__)
    # the inner rounding of w * dt(x * r) dropped
    _fails((w.float() * (x.float() * rstd[:, None])).to(dt), y, "inner rounding")
    # the mean taken over H + 8
    r8 = 1.0 / torch.sqrt(x.float().pow(2).sum(-1) / (H + 8) + 1e-5)
    _fails((w.float() * (x.float() * r8[:, None]).to(dt).float()).to(dt), y, "mean over H + 8")
    with pytest.raises(AssertionError):
        R.assert_rows_close(r8, rstd, rstd.slack, "rstd over H + 8")
    R.assert_rows_close(rstd.clone(), rstd, rstd.slack, "rstd")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [65, 4161])
def test_checker_fails_dw_missing_its_last_row(dt, rows):
    x, w, dy, _ = _norm_case(dt, rows=rows, H=512)
    _, _, rstd = R.rmsnorm_fwd(x, w, 1e-5)
    dw = R.rmsnorm_dw(dy, x, rstd)
    R.assert_chain_close(dw.clone(), dw, dw.slack, "the reference itself")
    _fails(R.rmsnorm_dw(dy[:-1], x[:-1], rstd[:-1]), dw, "dw without the last row")
    _fails(_one_nan(dw), dw, "one NaN")


@pytest.mark.parametrize("dt", DTYPES)
def test_planted_rope_faults_are_not_equal(dt):
    q, cos, sin = _rope_case(dt)
    for bwd in (False, True):
        ref = R.rope(q, cos, sin, bwd)
        # cos / sin of batch row 0 used for every batch row
        assert not torch.equal(R.rope(q, cos[:1], sin[:1], bwd), ref)
        # the sign of the sin term flipped in the last 8-pair chunk of the last position
        s2 = sin.clone()
        s2[:, -1, -8:] = -s2[:, -1, -8:]
        assert not torch.equal(R.rope(q, cos, s2, bwd), ref)
        assert torch.equal(R.rope(q.contiguous(), cos, sin, bwd), ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_checker_fails_planted_swiglu_faults(dt):
    g = torch.Generator().manual_seed(5)
    n = 8 * 257
    gate, up, dh = ((torch.randn(n, generator=g) * s).to(dt) for s in (3, 1, 1))
    h = R.swiglu_fwd(gate, up)
    dg, du = R.swiglu_bwd(gate, up, dh)
    for ref in (h, dg, du):
        R.assert_chain_close(ref.clone(), ref, ref.slack, "the reference itself")
        _fails(_one_nan(ref), ref, "one NaN")
        t = ref.clone()
        t[-8:] = t[-16:-8]
        _fails(t, ref, "last chunk from the one before")
    # du from the unrounded silu
    gf = gate.float()
    _fails((dh.float() * (gf * torch.sigmoid(gf))).to(dt), du, "du from the unrounded silu")


@pytest.mark.parametrize("dt", DTYPES)
def test_checker_fails_planted_cross_entropy_faults(dt):
    logits, labels = _ce_case(dt)
    lse, loss = R.ce_fwd(logits, labels)
    d = R.ce_bwd(logits, labels, lse, 0.25)
    R.assert_chain_close(d.clone(), d, d.slack, "the reference itself")
    # the label column moved by 8
    moved = torch.where(labels >= 8, labels - 8, torch.where(labels >= 0, labels + 8, labels))
    _fails(R.ce_bwd(logits, moved, lse, 0.25), d, "label column moved by 8")
    _fails(_chunk_fault(d), d, "chunk")
    _fails(_last_row_fault(d), d, "last row")
    _fails(_one_nan(d), d, "one NaN")
    assert loss[3] == 0 and not d[3].any()
    off = lse.clone()
    off[1] += 4 * R.step(lse[1].double(), torch.float32).float()
    with pytest.raises(AssertionError):
        R.assert_rows_close(off, lse, lse.bound, "lse four steps off")


# ------------------------------------------------------------------------------------------------
# what the bar before this one let through
# ------------------------------------------------------------------------------------------------
def _old_ulp_close(a, b, max_ulp_frac=1e-3):
    """tests/test_gpu_fused_llama.py's _ulp_close as it stood: a NaN difference is never > tol."""
    a, b = a.float(), b.float()
    diff = (a - b).abs()
    tol = b.abs() * 2 ** -7 + 1e-30
    bad = (diff > tol).float().mean().item()
    return bad <= max_ulp_frac


def _old_norm_ratio(a, b, bar=5e-3):
    return ((a.float() - b.float()).norm() / b.float().norm()).item() < bar


def test_the_old_bar_passed_faults_the_checker_fails():
    """At test_rmsnorm_forward_backward_vs_eager's shape, [3 * 257, 4096] bf16: ``_ulp_close`` (the bar
    on y) passes an 8-element chunk taken from the row above, one NaN, and a last row left at the NaN
    sentinel (1 / 771 of the elements, none of them counted); the norm ratio < 5e-3 (the bar on dx)
    passes the chunk. The checker fails all four."""
    dt = torch.bfloat16
    x, w, dy, _ = _norm_case(dt, rows=3 * 257, H=4096)
    _, y, rstd = R.rmsnorm_fwd(x, w, 1e-5)
    dx = R.rmsnorm_bwd(dy, x, w, rstd)
    for fault in (_chunk_fault, _one_nan, _last_row_fault):
        assert _old_ulp_close(fault(y), y), fault.__name__
        _fails(fault(y), y, fault.__name__)
    assert _old_norm_ratio(_chunk_fault(dx), dx)
    _fails(_chunk_fault(dx), dx, "chunk in dx")
