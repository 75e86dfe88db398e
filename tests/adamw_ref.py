"""One-step fp64 references and per-element bounds for the fused clip + AdamW kernels of
``csrc/smt_kernels.hip`` (``AdamStep::apply``, ``clip_scale``; tests/test_gpu_adamw_exact.py,
tests/test_adamw_ref_host.py), with the checker's non-finite semantics of tests/fused_ops_ref.py.

The reference
-------------
``reference(p, m, v, g, h, norm_sq)`` evaluates one step in fp64 from the fp32 state, the gradient
(already widened: a bf16 / fp16 gradient is exact in fp32) and the ``smt_adamw_args`` fields ``h``.
The fields are used as given; a test of the kernel passes ``h.f32()``, the values the kernel sees.
``1 - beta`` is formed in fp32 and widened, as ``1.f - b1`` is in the kernel. With ge = g * s:

    DeepSpeed  m' = b1 m + (1-b1) ge            torch  p1 = p (1 - lr wd)
               v' = b2 v + (1-b2) ge ge                m' = m + (1-b1) (ge - m)
               den = sqrt(v' / bc2) + eps              v' = v b2 + (1-b2) ge ge
               q = (m' / bc1) / den                    den = sqrt(v') / sqrt(bc2) + eps
               p' = p - lr (q + wd p)                  p' = p1 - (lr / bc1) (m' / den)

The two modes are one function up to rounding. The scale ``s`` (``clip_scale``): s = grad_scale;
with a norm and max_norm > 0, total = fp32(sqrt(norm_sq)), clip = (total + 1e-6f) / max_norm, and
s = grad_scale / clip only when clip > 1. The value of s is taken in fp64 from those fp32 fields;
the *decision* clip > 1 is a branch of the kernel, so it is taken on the fp32 value the kernel
compares (``np.float32`` arithmetic; the addition and the division are correctly rounded in both).

The bound
---------
Per element and output, first order in u = 2^-24 (half an fp32 step, relative), counting the
roundings of the kernel's expression tree; ``step(x)`` is one fp32 step at x and covers the rounding
of the result itself (half a step) with as much again to spare. FMA contraction is on for this code
and only removes roundings.

    ge = g s          : one rounding; each use of ge below carries u |ge|.
    m' (DeepSpeed)    : b1 m (1), ge (1), (1-b1) ge (1)           <= 4u (b1 |m| + (1-b1) |ge|) + step(m')
    m' (torch)        : ge (1), ge - m (1), the product (1)       <= 4u (|m| + (1-b1) (|ge| + |m|)) + step(m')
    v'                : ge twice (2), (1-b2) ge (1), * ge (1), b2 v (1) <= 5u (b2 v + (1-b2) ge^2) + step(v')
    den               : the quotient, the root(s) and the sum are at most 4 roundings of den; the
                        inherited error of v' is carried as an interval, not a derivative (v' -> 0
                        makes the derivative blow up):
                          den_lo = sqrt(max(v' - tol_v, 0) / bc2) + eps, den_hi = sqrt((v' + tol_v) / bc2) + eps
                          tol_den = max(den_hi - den, den - den_lo) + 4u den
    q = (m'/bc1)/den  : tol_q = (tol_m / bc1) / den_lo + |q| tol_den / den_lo + 3u |q|
                        (two quotients; torch mode: lr / bc1, m' / den and their product)
    p'                : tol_p = lr tol_q + 3u lr (|q| + wd |p|) + step(p')
                        (wd p, the sum, the product with lr); torch mode adds 2u |p| for lr wd,
                        1 - lr wd and p (1 - lr wd).
    clip active       : s = grad_scale / ((fp32(sqrt) + 1e-6f) / max_norm) carries four more roundings
                        (the cast of the root, the sum, two quotients), 4u relative on ge: the ge
                        term of tol_m gains 4u (1-b1) |ge|, the ge^2 term of tol_v 8u (1-b2) ge^2.

``sqrtf`` and the fp32 divisions are taken as correctly rounded (the library is built -O3 without
fast-math, and hipcc's default keeps fp32 divide and sqrt correctly rounded). No allowance for any
single operation was needed on the GPU: see the measured ratios.

A non-finite gradient makes the reference non-finite at that element in the same way as the kernel
(g = +-inf: m' = +-inf, v' = +inf, p' = NaN; g = NaN: all NaN); ``outside`` passes a NaN or an Inf only
where the reference holds the same value, and the bound there is taken as 0.

Measured: largest |error| / bound over every element of the input set (``inputs``), s = 0.37 by
``grad_scale``, step 3, betas (0.9, 0.95), eps 1e-8, lr 1e-3, wd 0 and 0.01
-------------------------------------------------------------------------------------------------
CPU, a plain op-by-op fp32 evaluation (``plain_fp32``; ``python -m tests.adamw_ref``, 2^18 elements):

    DeepSpeed  p 0.50  m 0.44  v 0.57          torch  p 0.54  m 0.52  v 0.57

Fraction of elements a mutation of the fp64 formula (``MUTATIONS``) puts outside the bound of the
output it touches (2^14 elements, wd 0.01, the same in both modes to 0.01):

    eps inside the root 0.51   eps dropped 0.43   eps / sqrt(bc2) 0.42   bc2 dropped 0.92   bc1 dropped 0.92
    weight decay dropped 0.50 (every p != 0)   m with b2 0.96   g^2 scaled by s once 0.66
    elements 2 and 3 of every eight swapped 0.25 (every touched element but equal zeros)

MI355X, the kernels (tests/test_gpu_adamw_exact.py with ``ADAMW_REF_REPORT=1`` and ``-s`` prints them):
the flat kernel over n in {1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 5}, the tiled kernel over 3 tiles, wd 0
and 0.01; (gradient dtype, parameter dtype); p / m / v

                          DeepSpeed           torch
    flat  fp32, bf16      0.50 0.41 0.50      0.52 0.41 0.50
    flat  fp32, fp16      0.50 0.41 0.50      0.52 0.41 0.50
    flat  fp32, fp32      0.50 0.41 0.50      0.52 0.41 0.50
    flat  bf16, bf16      0.50 0.38 0.51      0.52 0.40 0.51
    flat  fp16, fp16      0.50 0.39 0.48      0.50 0.44 0.48
    tiled fp32, bf16      0.50 0.44 0.58      0.52 0.45 0.58
    tiled fp32, fp16      0.50 0.44 0.58      0.52 0.45 0.58
    tiled fp32, fp32      0.50 0.44 0.58      0.52 0.45 0.58
    clip active, gs 1     0.50 0.35 0.40      0.41 0.40 0.40     (fp32, bf16; the widened ge terms)
    clip active, gs 2^-16 0.50 0.35 0.40      0.41 0.40 0.40     (fp32, fp16; a 2^16 loss-scaled gradient)

The kernels sit where the plain fp32 evaluation does (the tiled rows are 196608 elements against 6149, hence
the larger maxima): no operation needed an allowance of its own.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from tests.fused_ops_ref import step

U = 2.0 ** -24
DEEPSPEED, TORCH = 0, 1          # SMT_ADAM_DEEPSPEED / SMT_ADAM_TORCH
F32 = torch.float32


def _f(x) -> float:
    return float(np.float32(x))


class Hyper(NamedTuple):
    """The numeric fields of ``smt_adamw_args``."""
    lr: float
    beta1: float
    beta2: float
    eps: float
    weight_decay: float
    bc1: float
    bc2: float
    max_grad_norm: float
    grad_scale: float
    mode: int

    def f32(self) -> "Hyper":
        """The fields as the fp32 values the kernel sees."""
        return self._replace(**{k: _f(getattr(self, k)) for k in self._fields if k != "mode"})


def hyper(step_no=3, mode=DEEPSPEED, wd=0.01, max_grad_norm=0.0, grad_scale=1.0, lr=1e-3, betas=(0.9, 0.95),
          eps=1e-8) -> Hyper:
    return Hyper(lr, betas[0], betas[1], eps, wd, 1 - betas[0] ** step_no, 1 - betas[1] ** step_no, max_grad_norm,
                 grad_scale, mode)


def clip_scale(norm_sq: Optional[float], h: Hyper):
    """``(s, active, s32)``: the scale in fp64 from the fp32 fields, whether the clip applied (decided
    on the fp32 value of clip, as the kernel's branch is) and the kernel's own fp32 scale."""
    gs, gs32 = float(h.grad_scale), np.float32(h.grad_scale)
    if norm_sq is None or not np.float32(h.max_grad_norm) > 0:
        return gs, False, gs32
    total = np.float32(math.sqrt(norm_sq))
    clip32 = (total + np.float32(1e-6)) / np.float32(h.max_grad_norm)
    if not clip32 > 1:
        return gs, False, gs32
    clip = (float(total) + float(np.float32(1e-6))) / float(np.float32(h.max_grad_norm))
    return gs / clip, True, gs32 / clip32


def threshold_totals(max_norm: float):
    """``[(total, clip, active)]``: the fp32 norms for which ``(total + 1e-6f) / max_norm`` is exactly 1.0 (the
    clip does not apply) and the first fp32 value above 1 (it does); ``max_norm`` a power of two."""
    mn, e6, out = np.float32(max_norm), np.float32(1e-6), []
    for target, active in ((np.float32(1), False), (np.nextafter(np.float32(1), np.float32(2)), True)):
        t = np.float32(float(target) * float(mn) - 1e-6)
        for _ in range(64):
            c = (t + e6) / mn
            if c == target:
                break
            t = np.nextafter(t, np.float32(np.inf if c < target else -np.inf))
        else:
            raise AssertionError(f"no fp32 norm gives clip {target!r}")
        out.append((t, target, active))
    return out


# mutations of the fp64 formula that the bound must reject, and the output each one touches
MUTATIONS = {
    "eps_inside_sqrt": "p", "eps_dropped": "p", "eps_over_sqrt_bc2": "p", "bc2_dropped": "p", "bc1_dropped": "p",
    "weight_decay_dropped": "p", "m_with_beta2": "m", "g2_scaled_once": "v", "swap_adjacent_in_pack": "pmv",
}


class Ref(NamedTuple):
    p: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    tol_p: torch.Tensor
    tol_m: torch.Tensor
    tol_v: torch.Tensor
    s: float
    active: bool


def _formula(P, M, V, G, s, h: Hyper, mutate=None):
    """(p', m', v') in fp64; ``mutate`` plants one of ``MUTATIONS``."""
    b1, b2 = h.beta1, h.beta2
    omb1 = float(np.float32(1) - np.float32(b1))
    omb2 = float(np.float32(1) - np.float32(b2))
    ge = G * s
    ge2 = G * ge if mutate == "g2_scaled_once" else ge * ge
    bm = b2 if mutate == "m_with_beta2" else b1
    omm = omb2 if mutate == "m_with_beta2" else omb1
    wd = 0.0 if mutate == "weight_decay_dropped" else h.weight_decay
    bc1 = 1.0 if mutate == "bc1_dropped" else h.bc1
    bc2 = 1.0 if mutate == "bc2_dropped" else h.bc2
    if h.mode == DEEPSPEED:
        m1 = bm * M + omm * ge
        v1 = b2 * V + omb2 * ge2
    else:
        m1 = M + omm * (ge - M) if mutate != "m_with_beta2" else bm * M + omm * ge
        v1 = V * b2 + omb2 * ge2
    if mutate == "eps_inside_sqrt":
        den = torch.sqrt(v1 / bc2 + h.eps)
    elif mutate == "eps_dropped":
        den = torch.sqrt(v1 / bc2)
    elif mutate == "eps_over_sqrt_bc2":
        den = torch.sqrt(v1 / bc2) + h.eps / math.sqrt(bc2)
    elif h.mode == DEEPSPEED:
        den = torch.sqrt(v1 / bc2) + h.eps
    else:
        den = torch.sqrt(v1) / math.sqrt(bc2) + h.eps
    if h.mode == DEEPSPEED:
        p1 = P - h.lr * ((m1 / bc1) / den + wd * P)
    else:
        p1 = P * (1.0 - h.lr * wd) - (h.lr / bc1) * (m1 / den)
    if mutate == "swap_adjacent_in_pack":          # elements 2 and 3 of every eight-element group
        idx = torch.arange(P.numel())
        k = idx % 8
        idx = torch.where(k == 2, idx + 1, torch.where(k == 3, idx - 1, idx)).clamp_(max=P.numel() - 1)
        p1, m1, v1 = p1[idx], m1[idx], v1[idx]
    return p1, m1, v1


def _finite(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


def reference(p, m, v, g, h: Hyper, norm_sq: Optional[float] = None, mutate=None) -> Ref:
    """One step in fp64 and the per-element bounds (module docstring). ``p, m, v, g``: 1-D CPU tensors."""
    P, M, V, G = (t.detach().double().cpu() for t in (p, m, v, g))
    s, active, _ = clip_scale(norm_sq, h)
    p1, m1, v1 = _formula(P, M, V, G, s, h, mutate)
    b1, b2 = h.beta1, h.beta2
    omb1 = float(np.float32(1) - np.float32(b1))
    omb2 = float(np.float32(1) - np.float32(b2))
    age = (G * s).abs()
    extra = 4 * U if active else 0.0                                # the roundings of s itself
    if h.mode == DEEPSPEED:
        tol_m = 4 * U * (b1 * M.abs() + omb1 * age)
    else:
        tol_m = 4 * U * (M.abs() + omb1 * (age + M.abs()))
    tol_m = tol_m + extra * omb1 * age + step(m1, F32)
    tol_v = 5 * U * (b2 * V + omb2 * age * age) + 2 * extra * omb2 * age * age + step(v1, F32)
    # den and q of the unmutated formula at this element
    den = torch.sqrt(v1 / h.bc2) + h.eps
    den_lo = torch.sqrt(torch.clamp(v1 - tol_v, min=0.0) / h.bc2) + h.eps
    den_hi = torch.sqrt((v1 + tol_v) / h.bc2) + h.eps
    tol_den = torch.maximum(den_hi - den, den - den_lo) + 4 * U * den
    q = (m1 / h.bc1) / den
    tol_q = (tol_m / h.bc1) / den_lo + q.abs() * tol_den / den_lo + 3 * U * q.abs()
    tol_p = h.lr * tol_q + 3 * U * h.lr * (q.abs() + h.weight_decay * P.abs()) + step(p1, F32)
    if h.mode == TORCH:
        tol_p = tol_p + 2 * U * P.abs()
    return Ref(p1, m1, v1, _finite(tol_p), _finite(tol_m), _finite(tol_v), s, active)


def plain_fp32(p, m, v, g, h: Hyper, norm_sq: Optional[float] = None):
    """``AdamStep::apply`` op by op in fp32 on the CPU, every operation rounded (no FMA): (p', m', v')."""
    c = lambda x: torch.tensor(x, dtype=F32)
    lr, b1, b2, eps, wd, bc1, bc2 = (c(x) for x in (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.bc1, h.bc2))
    one = c(1.0)
    _, _, s32 = clip_scale(norm_sq, h)
    p, m, v = p.float().clone(), m.float().clone(), v.float().clone()
    ge = g.float() * c(float(s32))
    if h.mode == DEEPSPEED:
        m = b1 * m + (one - b1) * ge
        v = b2 * v + ((one - b2) * ge) * ge
        denom = torch.sqrt(v / bc2) + eps
        update = (m / bc1) / denom + wd * p
        p = p - lr * update
    else:
        p = p * (one - lr * wd)
        m = m + (one - b1) * (ge - m)
        v = v * b2 + ((one - b2) * ge) * ge
        denom = torch.sqrt(v) / torch.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v


def inputs(n: int, seed: int = 0, s: float = 1.0, g_mul: float = 1.0):
    """The input set ``(p, m, v, g)`` in fp32 (fixed seed, random signs):
    |g| log-uniform in [1e-9, 1e2] (raised so that |g s| >= 1e-12: g^2 stays a normal fp32 number), 10 % exact
    zeros, times ``g_mul`` (a loss scale); |p| log-uniform in [1e-6, 10], every fifth exactly 0 (there p' is
    -lr * update: the update itself is checked to a few u); |m| = 0.3 * log-uniform [1e-9, 1e2], 10 % zeros;
    v = the square of such a draw, 10 % zeros; every 37th element has g = m = v = p = 0 and must stay 0."""
    gen = torch.Generator().manual_seed(1000 + seed)

    def logu(lo, hi):
        r = torch.rand(n, generator=gen, dtype=torch.float64)
        return torch.exp(math.log(lo) + r * (math.log(hi) - math.log(lo)))

    def sign():
        return torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1

    def some_zero(t, frac=0.1):
        return torch.where(torch.rand(n, generator=gen) < frac, torch.zeros_like(t), t)

    g_lo = max(1e-9, 1.001e-12 / abs(s * g_mul)) if s else 1e-9
    g = some_zero(sign() * logu(g_lo, 1e2)) * g_mul
    p = sign() * logu(1e-6, 10.0)
    m = some_zero(sign() * 0.3 * logu(1e-9, 1e2))
    v = some_zero((0.3 * logu(1e-9, 1e2)) ** 2)
    i = torch.arange(n)
    p[i % 5 == 4] = 0.0
    dead = i % 37 == 36
    for t in (g, p, m, v):
        t[dead] = 0.0
    return p.float(), m.float(), v.float(), g.float()


# ------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------
def outside(actual, ref, tol):
    """Elements with ``~(|actual - ref| <= tol)``: a NaN or an Inf passes only where ref holds the same."""
    a = actual.detach().double().cpu()
    same = (a == ref) | (torch.isnan(a) & torch.isnan(ref))
    return ~(same | ((a - ref).abs() <= tol))


def ratio(actual, ref, tol) -> float:
    """Largest |actual - ref| / tol over the elements where ref is finite."""
    a = actual.detach().double().cpu()
    ok = torch.isfinite(ref) & torch.isfinite(a)
    return float(((a - ref).abs()[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0


def assert_within(actual, ref, tol, what):
    assert actual.shape == ref.shape, (what, actual.shape, ref.shape)
    bad = outside(actual, ref, tol)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements outside the bound; first at {i}: "
                             f"{actual[i].item()!r} vs {ref[i].item()!r} (bound {tol[i].item():.3e})")


def assert_step_within(got, r: Ref, what):
    """``got`` = (p', m', v') of a kernel or an evaluation against the reference ``r``; the ratios."""
    out = {}
    for name, a, x, t in (("p", got[0], r.p, r.tol_p), ("m", got[1], r.m, r.tol_m), ("v", got[2], r.v, r.tol_v)):
        assert_within(a, x, t, f"{what} {name}")
        out[name] = ratio(a, x, t)
    return out


# ------------------------------------------------------------------------------------------------
# the measurements quoted above
# ------------------------------------------------------------------------------------------------
def _measure():
    for mode, name in ((DEEPSPEED, "DeepSpeed"), (TORCH, "torch")):
        worst = {"p": 0.0, "m": 0.0, "v": 0.0}
        for wd in (0.0, 0.01):
            h = hyper(3, mode, wd, grad_scale=0.37).f32()
            p, m, v, g = inputs(1 << 18, 0, 0.37)
            r = reference(p, m, v, g, h)
            for k, x in assert_step_within(plain_fp32(p, m, v, g, h), r, name).items():
                worst[k] = max(worst[k], x)
        print(f"plain fp32 / bound, {name}: " + "  ".join(f"{k} {x:.2f}" for k, x in worst.items()))
    p, m, v, g = inputs(1 << 14, 1, 0.37)
    for mut, touches in MUTATIONS.items():
        fr = []
        for mode in (DEEPSPEED, TORCH):
            h = hyper(3, mode, 0.01, grad_scale=0.37).f32()
            r, x = reference(p, m, v, g, h), reference(p, m, v, g, h, mutate=mut)
            fr.append(max(float(outside(getattr(x, k), getattr(r, k), getattr(r, "tol_" + k)).double().mean())
                          for k in touches))
        print(f"mutation {mut}: outside the bound of {touches}: {fr[0]:.2f} (DeepSpeed) {fr[1]:.2f} (torch)")


if __name__ == "__main__":
    _measure()
