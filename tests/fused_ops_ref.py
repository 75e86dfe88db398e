"""Chain references and the per-element checker for the fused RMSNorm / RoPE / SwiGLU / cross-entropy
kernels of ``csrc/llama_kernels.hip`` (tests/test_gpu_fused_ops_exact.py, tests/test_fused_ops_ref_host.py).

A chain reference is the formula of the kernel's header comment (``llama_kernels.hip``,
``include/smt_model_ops.h``) written in torch with every intermediate rounding to the model dtype
(bf16 or fp16) kept per element. The only things a kernel may do differently are

* the order of an fp32 row reduction (RMSNorm's sum of squares, the backward's ``sum(dt(dy*w) * x)``, the
  cross entropy's sum of exponentials, the rows of the weight gradient), and
* ``v_exp_f32`` / ``v_rcp_f32`` in place of libm (``silu_math.h``, ``lse_chunk``, ``ce_grad8``).

Here the reductions are taken in fp64 and rounded to fp32 once. Beside each output a reference returns
``slack``: per element, the first-order effect of those two freedoms on that element. It is zero for an
element whose value cannot change: a value ``t`` that is rounded to the model dtype changes only if ``t``
lies within its own uncertainty ``tol`` of a rounding boundary (``_rounded``), and then by one step.

    y    = dt(w * n), n = dt(x * rstd): tol(x * rstd) = |x * rstd| * (RSTD_REL + 2^-24); where n can
           flip, y moves by |w| * step(n) and is rounded again (+ step(y) / 2).
    dx   = dt(r * gw - x * coef), coef = r^3 * dot / H: the difference cancels, so the uncertainty is
           that of its terms, |x| * tol(coef) + 2^-23 * (|r * gw| + |x * coef|), with tol(coef) from
           tol(dot) = RED_REL * sum |gw * x| -- not a fraction of |dx|.
    dx+dres = dt(dt(dx) + dres) flips only where dt(dx) does, by the step of dx (+ its own rounding).
    dw   = dt(sum_rows term): tol = RED_REL * sum_rows |term| (the terms themselves are exact, rstd is
           an input).
    silu = dt(g * sig(g)): tol = |g * sig| * SIG_REL(g), SIG_REL from 1 ulp for each of v_exp_f32 and
           v_rcp_f32, the rounding of the exponent's argument and of 1 + e, and the multiply (_sig_rel).
    lse  : RED_REL (a relative error of the sum is an absolute error of its logarithm) plus one fp32
           step of lse -- the bound, there is no model-dtype rounding.
    dlogits = dt((p - [label]) * scale), p = exp(x - lse): tol(p) = p * ln2 * 2^-24 * (|x| log2e +
           2 |lse| log2e) (the roundings of the exponent's argument) + 3 * 2^-24 * (p + [label]).

``assert_chain_close`` then judges every element: ``~(|actual - ref| <= step(ref) + slack)`` fails, so a
NaN or an Inf fails unless ref holds the same non-finite value; and at most 1e-3 of the elements (never
fewer than 2) may differ from ref at all.

Measured constants (CPU, ``python -m tests.fused_ops_ref``; printed by ``_measure`` below):

    fp32 ``torch.sum`` and a sequential fp32 ``cumsum`` against the fp64 sum of the same terms, as a
    fraction of sum |term|, the largest of 200 draws each:
        sum of squares  H 640: 1.36e-07   H 4096: 1.31e-07   (rstd off by 1.62 / 1.72 fp32 steps)
        signed terms    n 64: 2.5e-09   n 640: 8.1e-09   n 4161: 4.9e-09
    RED_REL = 2.8e-07, twice the largest of them. RSTD_REL = RED_REL / 2 + 3 * 2^-24 (rstd = (ss / H +
    eps)^-1/2 halves the relative error of ss; a division, an addition and a correctly rounded
    square root and reciprocal follow).

    Fraction of elements that differ from the reference at all when the reductions are taken in
    plain fp32 instead (the reference alone, no kernel), rows 64, H 640 and 4096:
        bf16  y, dx, dx+dres: 0
        fp16  y 2.3e-05 - 4.9e-05,  dx 0 - 1.1e-05,  dx+dres 0;  one step each
        dw (a sequential fp32 sum over 4161 rows): 0 in both
    and of transformers' eager chain on the CPU against the references (65536 elements; 64 x 8192):
        swiglu h, du: 0;  dg: 0 (bf16), 1.1e-04 (fp16);  ce dlogits: 5.9e-05 (bf16), 4.0e-05 (fp16)
    all below the cap of 1e-3, one step each, and none outside the per-element bound.
"""
from __future__ import annotations

import math

import torch

RED_REL = 2.8e-7
F32 = 2.0 ** -24                      # half an fp32 step, relative
RSTD_REL = RED_REL / 2 + 3 * F32
DIFFER_CAP = 1e-3
PATTERN = 0x7FC1                      # sentinel: a NaN in bf16 and in fp16, so an unwritten output shows
LOG2E = 1.4426950408889634
_MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
_EMIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}


def step(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """One step of ``dtype`` at ``ref`` (fp64): the spacing of the binade ``|ref|`` lies in."""
    _, e = torch.frexp(ref.double().abs())
    e = torch.clamp(e.to(torch.int64) - 1, min=_EMIN[dtype])
    e = torch.where(ref == 0, torch.full_like(e, _EMIN[dtype]), e)            # frexp(0) has exponent 0
    e = torch.where(torch.isfinite(ref.double()), e, torch.zeros_like(e))
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), (e - _MANT[dtype]).to(torch.int32))


def _rounded(t: torch.Tensor, tol: torch.Tensor, dtype: torch.dtype, ref: torch.Tensor = None):
    """``ref = dt(fp32(t))`` (or the given ref) and its slack: where ``t`` (fp64) lies within ``tol`` of
    a rounding boundary of ``dtype``, or ref is not fp64's own rounding, ``tol + step(ref)``; else 0."""
    near = t.float().to(dtype)
    if ref is None:
        ref = near
    n = near.double()
    inf = torch.full_like(near, float("inf"))
    up, dn = torch.nextafter(near, inf).double(), torch.nextafter(near, -inf).double()
    dist = torch.minimum(((n + up) / 2 - t).abs(), ((n + dn) / 2 - t).abs())
    flip = ~(dist > tol) | (ref != near)
    flip &= torch.isfinite(t)
    slack = torch.where(flip, tol + step(ref.double(), dtype), torch.zeros_like(t))
    return ref, torch.nan_to_num(slack, nan=0.0, posinf=0.0)


def _after(flip_slack: torch.Tensor, moved_by: torch.Tensor, out: torch.Tensor, dtype) -> torch.Tensor:
    """Slack of ``out = dt(f(n))`` where ``n`` may flip (flip_slack > 0) and that moves f by moved_by."""
    return torch.where(flip_slack > 0, moved_by + step(out.double(), dtype) / 2, torch.zeros_like(moved_by))


# ------------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, w, eps, residual=None):
    """``(h, y, rstd)`` and ``(slack_y, slack_rstd)`` as ``.slack`` attributes of y and rstd.
    h = dt(x + residual) (x itself without a residual); rstd = fp32((fp32(sum64(h^2)) / H + eps)^-1/2)."""
    dt = x.dtype
    h = x if residual is None else (x.float() + residual.float()).to(dt)
    H = h.shape[-1]
    ss = h.double().pow(2).sum(-1).float()
    rstd = 1.0 / torch.sqrt(ss / float(H) + torch.tensor(eps, dtype=torch.float32))
    t = h.double() * rstd.double()[..., None]
    n, sn = _rounded(t, t.abs() * (RSTD_REL + F32), dt)
    y = (w.float() * n.float()).to(dt)
    y.slack = _after(sn, w.double().abs() * step(n.double(), dt), y, dt)
    rstd.slack = rstd.double() * RSTD_REL
    return h, y, rstd


def rmsnorm_bwd(dy, x, w, rstd, dres=None):
    """dx = dt(r * gw - x * coef), gw = dt(dy * w), coef = fp32(r^3 * fp32(sum64(gw * x)) / H); with
    dres: dt(dt(dx) + dres). ``.slack`` on the result."""
    dt = x.dtype
    H = x.shape[-1]
    gw = (dy.float() * w.float()).to(dt)
    prod = gw.double() * x.double()
    dot, absdot = prod.sum(-1).float(), prod.abs().sum(-1)
    r = rstd.float()
    coef = r * r * r * dot / float(H)
    rd = r.double()
    tol_coef = rd.pow(3) / H * (RED_REL * absdot) + 4 * F32 * coef.double().abs()
    a, b = rd[..., None] * gw.double(), x.double() * coef.double()[..., None]
    t = a - b
    tol = x.double().abs() * tol_coef[..., None] + 2 * F32 * (a.abs() + b.abs())
    ref = (r[..., None] * gw.float() - x.float() * coef[..., None]).to(dt)
    dx, s = _rounded(t, tol, dt, ref)
    if dres is not None:
        out = (dx.float() + dres.float()).to(dt)
        out.slack = torch.where(s > 0, s + step(dx.double(), dt) / 2 + step(out.double(), dt) / 2, s)
        return out
    dx.slack = s
    return dx


def rmsnorm_dw(dy, x, rstd):
    """dw = dt(sum64_rows dt(dy * dt(x * rstd))); bound term RED_REL * sum |term| + the rounding flip."""
    dt = x.dtype
    n = (x.float() * rstd.float()[..., None]).to(dt)
    term = (dy.float() * n.float()).to(dt).double()
    t = term.sum(0)
    dw, s = _rounded(t, RED_REL * term.abs().sum(0), dt)
    dw.slack = s
    return dw


# ------------------------------------------------------------------------------------------------
# RoPE: no reduction, no transcendental -- compared with torch.equal
# ------------------------------------------------------------------------------------------------
def rope(t, cos, sin, bwd=False):
    """``t`` [B, heads, S, D], cos / sin [B or 1, S, D], every product and sum rounded to the dtype.
    forward:  lo' = dt(dt(lo*c_lo) + dt(-hi*s_lo)),  hi' = dt(dt(hi*c_hi) + dt(lo*s_hi))
    backward: dlo = dt(dt(dlo'*c_lo) + dt(dhi'*s_hi)), dhi = dt(dt(dhi'*c_hi) - dt(dlo'*s_lo))"""
    half = t.shape[-1] // 2
    c, s = cos.unsqueeze(1), sin.unsqueeze(1)
    lo, hi = t[..., :half], t[..., half:]
    c_lo, c_hi, s_lo, s_hi = c[..., :half], c[..., half:], s[..., :half], s[..., half:]
    if not bwd:
        return torch.cat((lo * c_lo + (-hi) * s_lo, hi * c_hi + lo * s_hi), dim=-1)
    return torch.cat((lo * c_lo + hi * s_hi, hi * c_hi - lo * s_lo), dim=-1)


# ------------------------------------------------------------------------------------------------
# SwiGLU
# ------------------------------------------------------------------------------------------------
def _sig_rel(x64: torch.Tensor, sig64: torch.Tensor) -> torch.Tensor:
    """Relative uncertainty of g * sigmoid(g) as silu_math.h computes it: e = exp2(-x * log2e) carries
    the two roundings of its argument (|x| log2e ln2 * 2 * 2^-24 relative on e) and 1 ulp of v_exp_f32;
    sig = 1 / (1 + e) takes (1 - sig) of e's relative error, half a step of the addition and 1 ulp of
    v_rcp_f32; the multiply by g half a step. libm's own chain (the reference) lies inside it too."""
    return (1 - sig64) * (2 * F32 + x64.abs() * 2 * F32) + F32 + 2 * F32 + F32


def _silu(g):
    dt = g.dtype
    xf = g.float()
    s32 = xf / (1.0 + torch.exp(-xf))              # transformers' eager silu, in fp32
    x64 = g.double()
    sig64 = torch.sigmoid(x64)
    t = x64 * sig64
    # a sigmoid below the fp32 normal range may be flushed to zero by the hardware: absolute
    tol = t.abs() * _sig_rel(x64, sig64) + torch.where(sig64 < 2.0 ** -125, x64.abs() * 2.0 ** -126, 0.0)
    s, slack = _rounded(t, tol, dt, s32.to(dt))
    return s, slack, sig64


def swiglu_fwd(g, u):
    """h = dt(dt(g * sigmoid(g)) * u), ``.slack``."""
    dt = g.dtype
    s, ss, _ = _silu(g)
    h = (s.float() * u.float()).to(dt)
    h.slack = _after(ss, u.double().abs() * ss, h, dt)
    h.silu = s
    return h


def swiglu_bwd(g, u, dh):
    """ds = dt(dh * u), du = dt(dh * s), dg = dt(ds * sig * (1 + g * (1 - sig))); ``(dg, du)`` with slack."""
    dt = g.dtype
    s, ss, sig = _silu(g)
    du = (dh.float() * s.float()).to(dt)
    du.slack = _after(ss, dh.double().abs() * ss, du, dt)
    ds = (dh.float() * u.float()).to(dt)
    x = g.double()
    e_sig = _sig_rel(x, sig)
    bf = 1 + x * (1 - sig)
    err_1ms = sig * e_sig + F32 * (1 - sig)
    err_bf = x.abs() * err_1ms + F32 * (x * (1 - sig)).abs() + F32 * bf.abs()
    t = ds.double() * sig * bf
    tol = ds.double().abs() * (sig * e_sig * bf.abs() + sig * err_bf) + 2 * F32 * t.abs()
    tol = tol + torch.where(sig < 2.0 ** -125, ds.double().abs() * bf.abs() * 2.0 ** -126, 0.0)
    xf = g.float()
    sig32 = 1.0 / (1.0 + torch.exp(-xf))
    ref = ((ds.float() * sig32) * (1.0 + xf * (1.0 - sig32))).to(dt)
    dg, sg = _rounded(t, torch.nan_to_num(tol, nan=0.0, posinf=0.0), dt, ref)
    dg.slack = sg
    return dg, du


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
def ce_fwd(logits, labels, ignore_index=-100):
    """Per row: lse = fp32(logsumexp64(logits)), loss = fp32(lse - logits[label]); 0 on an ignored
    row, NaN where the label is outside [0, V). ``.bound``: the whole per-row bound (fp32 outputs)."""
    V = logits.shape[-1]
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1).float()
    valid = (labels >= 0) & (labels < V)
    picked = logits.float().gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    loss = lse - picked
    loss = torch.where(valid, loss, torch.full_like(loss, float("nan")))
    loss = torch.where(labels == ignore_index, torch.zeros_like(loss), loss)
    lse.bound = RED_REL + step(lse.double(), torch.float32)
    loss.bound = lse.bound + step(torch.nan_to_num(loss.double()), torch.float32)
    return lse, loss


def ce_bwd(logits, labels, lse, scale, ignore_index=-100):
    """dlogits = dt((exp(x - lse) - [j == label]) * scale), zeros on an ignored row; ``.slack``."""
    dt = logits.dtype
    V = logits.shape[-1]
    x, l = logits.double(), lse.double()[:, None]
    w = torch.where(labels == ignore_index, 0.0, float(scale)).double()[:, None]
    p = torch.exp(x - l)
    hot = (torch.arange(V)[None, :].to(labels.device) == labels[:, None]).double()
    t = (p - hot) * w
    tol = w.abs() * (p * math.log(2.0) * F32 * LOG2E * (x.abs() + 2 * l.abs()) + 3 * F32 * (p + hot))
    d, s = _rounded(t, torch.nan_to_num(tol, nan=0.0, posinf=0.0), dt)
    d.slack = s
    return d


# ------------------------------------------------------------------------------------------------
# the checker and the sentinel
# ------------------------------------------------------------------------------------------------
def mismatches(actual, ref, slack):
    """(bad, differ): elements outside ``step(ref) + slack`` (any NaN / Inf that ref does not hold too
    among them), and elements that differ from ref at all."""
    dt = ref.dtype
    a, r = actual.detach().double().cpu(), ref.detach().double().cpu()
    same = (a == r) | (torch.isnan(a) & torch.isnan(r))
    bound = step(r, dt) + (slack.double().cpu() if torch.is_tensor(slack) else float(slack))
    bad = ~(same | ((a - r).abs() <= bound))
    return bad, ~same


def assert_chain_close(actual, ref, slack, what):
    assert actual.shape == ref.shape and actual.dtype == ref.dtype, (what, actual.shape, ref.shape, actual.dtype)
    bad, differ = mismatches(actual, ref, slack)
    n = ref.numel()
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {n} elements outside one step + slack; first at {i}: "
                             f"{actual[i].item()!r} vs {ref[i].item()!r}")
    cap = max(2, int(DIFFER_CAP * n))
    if int(differ.sum()) > cap:
        some = [(tuple(int(v) for v in i), actual[tuple(i)].item(), ref[tuple(i)].item()) for i in differ.nonzero()[:6]]
        raise AssertionError(f"{what}: {int(differ.sum())} of {n} elements differ from the reference (cap {cap}); "
                             f"(index, actual, ref): {some}")


def assert_rows_close(actual, ref, bound, what):
    """fp32 per-row statistics (rstd, lse, loss): every row inside ``bound``, NaN only where ref's is."""
    a, r = actual.detach().double().cpu(), ref.double().cpu()
    bad = ~(((a - r).abs() <= bound.double().cpu()) | (torch.isnan(a) & torch.isnan(r)) | (a == r))
    assert not bad.any(), f"{what}: rows {bad.nonzero().flatten().tolist()}: {a[bad].tolist()} vs {r[bad].tolist()}"


class Sentinel:
    """A [rows, H] window at row 1, column 8 of a wider buffer (leading dimension ``ld``, default H + 8)
    prefilled with a 16-bit pattern; ``check`` asserts every element outside the window unchanged."""

    def __init__(self, rows, H, dtype, device, ld=None, fill=None):
        self.rows, self.H, self.ld = rows, H, ld or H + 8
        assert self.ld >= H + 8 and self.ld % 8 == 0
        self.buf = torch.full((rows + 3, self.ld), PATTERN, dtype=torch.int16, device=device)
        self.win = self.buf.view(dtype)[1:1 + rows, 8:8 + H]
        if fill is not None:
            self.win.copy_(fill)

    def check(self, what):
        b = self.buf.clone()
        b[1:1 + self.rows, 8:8 + self.H] = PATTERN
        assert bool((b == PATTERN).all()), f"{what}: wrote outside its [{self.rows}, {self.H}] window"


# ------------------------------------------------------------------------------------------------
# the measurements quoted above
# ------------------------------------------------------------------------------------------------
def _measure():
    torch.manual_seed(0)
    print("fp32 reduction error / sum |term| (max of 200 draws), torch.sum and sequential cumsum")
    for H in (640, 4096):
        worst = ulps = 0.0
        for _ in range(200):
            x = (torch.randn(H) * 3).bfloat16().float()
            sq = x * x
            ex = sq.double().sum()
            for got in (sq.sum(), sq.cumsum(0)[-1]):
                worst = max(worst, abs(got.double() - ex).item() / ex.item())
            r32 = 1.0 / torch.sqrt(sq.sum() / H + 1e-5)
            r64 = 1.0 / torch.sqrt(ex / H + 1e-5)
            ulps = max(ulps, (abs(r32.double() - r64) / step(r64, torch.float32)).item())
        print(f"  sum of squares H {H}: {worst:.2e}, rstd {ulps:.2f} fp32 ulps")
    for n in (64, 640, 4161):
        worst = 0.0
        for _ in range(200):
            t = (torch.randn(n).bfloat16() * torch.randn(n).bfloat16()).float()
            ex, ab = t.double().sum(), t.double().abs().sum()
            for got in (t.sum(), t.cumsum(0)[-1]):
                worst = max(worst, abs(got.double() - ex).item() / ab.item())
        print(f"  signed terms n {n}: {worst:.2e}")
    print("reference alone: fp32-order reductions against the fp64-statistic reference")
    for dt in (torch.bfloat16, torch.float16):
        for H in (640, 4096):
            x = (torch.randn(64, H) * 2).to(dt)
            w = (torch.randn(H) * 0.2 + 1).to(dt)
            dy, dres = torch.randn(64, H).to(dt), torch.randn(64, H).to(dt)
            _, y, rstd = rmsnorm_fwd(x, w, 1e-5)
            r32 = 1.0 / torch.sqrt(x.float().pow(2).sum(-1) / H + 1e-5)
            y32 = (w.float() * (x.float() * r32[:, None]).to(dt).float()).to(dt)
            gw = (dy.float() * w.float()).to(dt)
            dot = (gw.float() * x.float()).sum(-1)
            coef = rstd * rstd * rstd * dot / H
            dx32 = (rstd[:, None] * gw.float() - x.float() * coef[:, None]).to(dt)
            dxr32 = (dx32.float() + dres.float()).to(dt)
            for name, got, ref in (("y", y32, y), ("dx", dx32, rmsnorm_bwd(dy, x, w, rstd)),
                                   ("dx+dres", dxr32, rmsnorm_bwd(dy, x, w, rstd, dres))):
                bad, differ = mismatches(got, ref, ref.slack)
                steps = ((got.double() - ref.double()).abs() / step(ref.double(), dt)).max().item()
                print(f"  {dt} H {H} {name}: differ {differ.float().mean().item():.2e}, "
                      f"worst {steps:.0f} steps, outside the bound {int(bad.sum())}")

        x = (torch.randn(4161, 512) * 2).to(dt)
        dy = torch.randn(4161, 512).to(dt)
        rstd = rmsnorm_fwd(x, torch.ones(512).to(dt), 1e-5)[2]
        dw = rmsnorm_dw(dy, x, rstd)
        term = (dy.float() * (x.float() * rstd[:, None]).to(dt).float()).to(dt).float()
        _report(dt, "dw (sequential fp32 sum, 4161 rows)", term.cumsum(0)[-1].to(dt), dw)
        g, u, dh = ((torch.randn(1 << 16) * s).to(dt) for s in (3, 1, 1))
        ge, ue = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        he = torch.nn.functional.silu(ge) * ue
        he.backward(dh)
        dg, du = swiglu_bwd(g, u, dh)
        for name, got, ref in (("h", he.detach(), swiglu_fwd(g, u)), ("dg", ge.grad, dg), ("du", ue.grad, du)):
            _report(dt, "swiglu " + name + " (eager)", got, ref)
        logits = (torch.randn(64, 8192) * 4).to(dt).requires_grad_(True)
        labels = torch.randint(0, 8192, (64,))
        torch.nn.functional.cross_entropy(logits.float(), labels, reduction="sum").backward()
        lse, _ = ce_fwd(logits.detach(), labels)
        _report(dt, "ce dlogits (eager)", logits.grad, ce_bwd(logits.detach(), labels, lse, 1.0))


def _report(dt, name, got, ref):
    bad, differ = mismatches(got, ref, ref.slack)
    steps = ((got.double() - ref.double()).abs() / step(ref.double(), dt)).max().item()
    print(f"  {dt} {name}: differ {differ.float().mean().item():.2e}, worst {steps:.0f} steps, "
          f"outside the bound {int(bad.sum())}")


if __name__ == "__main__":
    _measure()
