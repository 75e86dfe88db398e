"""The fp64 AdamW references of tests/adamw_ref.py against ``torch.optim.AdamW`` and the oracle's
DeepSpeed restatement on the CPU, and their per-element bound against a plain fp32 evaluation (inside,
every element) and against planted formula errors (each rejected). No GPU.

Largest error / bound of the plain fp32 evaluation over 2^18 elements, wd 0 and 0.01 (p / m / v):
DeepSpeed 0.50 / 0.44 / 0.57, torch 0.54 / 0.52 / 0.57; the planted errors put 25 % (two swapped lanes of
eight) to 96 % of the elements outside (the table in tests/adamw_ref.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import smt_oracle as oracle
from tests import adamw_ref as A

MODES = [A.DEEPSPEED, A.TORCH]
N = 1 << 14
S = 0.37


def _f32(x):
    return float(np.float32(x))


def _rel_err(got, want, terms=None):
    """Per element, relative to the reference value (0 where both are 0). Both sides are fp64 evaluations
    whose roundings (a handful of 2^-53) are relative to the ``terms`` of a sum, not to a result that cancels:
    p' = p - lr q loses |p| / |p'| where p is close to lr q, m' likewise where g opposes m. With ``terms`` an
    element is measured against max(|want|, terms / 100): the bar relative to the result itself wherever less
    than 100-fold cancels, and 100 times tighter than the bar relative to the terms elsewhere."""
    got, want = got.double(), want.double()
    scale = want.abs() if terms is None else torch.maximum(want.abs(), terms / 100)
    return torch.where(scale == 0, got.abs(), (got - want).abs() / scale).max().item()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_torch_mode_reference_is_torch_adamw_in_fp64(wd):
    """3 steps from zero state; betas, lr, eps and wd are fp32 values so that both sides see the same."""
    lr, b1, b2, eps, wd = _f32(1e-3), _f32(0.9), _f32(0.95), _f32(1e-8), _f32(wd)
    p0, _, _, _ = A.inputs(N, 0)
    param = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for step_no in (1, 2, 3):
        g = A.inputs(N, step_no)[3].double()
        param.grad = g.clone()
        opt.step()
        h = A.hyper(step_no, A.TORCH, wd, lr=lr, betas=(b1, b2), eps=eps)
        r = A.reference(p, m, v, g, h)
        terms_p, terms_m = p.abs() + (r.p - p).abs(), m.abs() + g.abs()
        p, m, v = r.p, r.m, r.v
        st = opt.state[param]
        assert _rel_err(p, param.detach(), terms_p) <= 1e-13, step_no
        assert _rel_err(m, st["exp_avg"], terms_m) <= 1e-13 and _rel_err(v, st["exp_avg_sq"]) <= 1e-13, step_no


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clipped", [False, True])
def test_deepspeed_mode_reference_is_the_oracle_in_fp64(wd, clipped):
    """``oracle.smt_oracle.fused_adam_step`` on fp64 tensors, ``clip_coef`` for the scale; the random state."""
    b1, b2 = _f32(0.9), _f32(0.95)
    p0, m0, v0, g = A.inputs(N, 2)
    coef = oracle.clip_coef([g], 1.0) if clipped else 1.0
    assert (coef < 0.1) == clipped
    p, m, v = p0.double().clone(), m0.double().clone(), v0.double().clone()
    oracle.fused_adam_step(p, g.double() * coef, m, v, 3, 1e-3, (b1, b2), 1e-8, wd)
    r = A.reference(p0, m0, v0, g, A.hyper(3, A.DEEPSPEED, wd, grad_scale=coef, betas=(b1, b2)))
    assert r.s == coef and not r.active
    terms_p, terms_m = p0.double().abs() + (r.p - p0.double()).abs(), m0.double().abs() + (g.double() * coef).abs()
    assert _rel_err(r.p, p, terms_p) <= 1e-13 and _rel_err(r.m, m, terms_m) <= 1e-13 and _rel_err(r.v, v) <= 1e-13
    if clipped:
        # the reference's own clip takes the norm's root and 1e-6 as the kernel's fp32 values, the oracle as
        # doubles: the two scales agree to the roundings of those two values
        norm_sq = math.fsum((g.double() ** 2).tolist())
        s, active, _ = A.clip_scale(norm_sq, A.hyper(3, max_grad_norm=1.0).f32())
        assert active and abs(s / coef - 1) <= 2 * A.U


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_plain_fp32_evaluation_is_inside_the_bound_everywhere(mode, wd):
    h = A.hyper(3, mode, wd, grad_scale=S).f32()
    p, m, v, g = A.inputs(1 << 18, 0, S)
    r = A.reference(p, m, v, g, h)
    ratios = A.assert_step_within(A.plain_fp32(p, m, v, g, h), r, f"plain fp32, mode {mode}")
    print(f"mode {mode} wd {wd}: error / bound " + " ".join(f"{k} {x:.2f}" for k, x in ratios.items()))
    assert max(ratios.values()) <= 1.0
    # the all-zero elements stay zero, and a bound is never empty
    dead = (g == 0) & (p == 0) & (m == 0) & (v == 0)
    assert dead.any() and all(bool((t[dead] == 0).all()) for t in (r.p, r.m, r.v))
    assert all(bool((t > 0).all()) for t in (r.tol_p, r.tol_m, r.tol_v))


@pytest.mark.parametrize("mode", MODES)
def test_plain_fp32_with_the_clip_active_is_inside_the_bound(mode):
    """s through the clip (four more roundings, the widened ge terms) and the fp16 unscale 2^-16."""
    for gs, g_mul in ((1.0, 1.0), (2.0 ** -16, 2.0 ** 16)):
        p, m, v, g = A.inputs(N, 3, S * gs, g_mul)
        norm_sq = math.fsum(((g.double() * gs) ** 2).tolist())
        h = A.hyper(3, mode, 0.01, max_grad_norm=S * math.sqrt(norm_sq), grad_scale=gs).f32()
        r = A.reference(p, m, v, g, h, norm_sq)
        assert r.active and abs(r.s / gs - S) < 1e-6
        A.assert_step_within(A.plain_fp32(p, m, v, g, h, norm_sq), r, f"clip active, mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mutation", sorted(A.MUTATIONS))
def test_the_bound_rejects_a_wrong_formula(mode, mutation):
    p, m, v, g = A.inputs(N, 1, S)
    h = A.hyper(3, mode, 0.01, grad_scale=S).f32()
    r, x = A.reference(p, m, v, g, h), A.reference(p, m, v, g, h, mutate=mutation)
    for k in A.MUTATIONS[mutation]:
        frac = A.outside(getattr(x, k), getattr(r, k), getattr(r, "tol_" + k)).double().mean().item()
        assert frac > 0.10, (mutation, k, frac)


def test_the_two_modes_are_one_function_up_to_rounding():
    """Not a mutation: each mode's fp64 value lies inside the other's bound."""
    p, m, v, g = A.inputs(N, 1, S)
    a = A.reference(p, m, v, g, A.hyper(3, A.DEEPSPEED, 0.01, grad_scale=S).f32())
    b = A.reference(p, m, v, g, A.hyper(3, A.TORCH, 0.01, grad_scale=S).f32())
    A.assert_step_within((b.p, b.m, b.v), a, "torch in DeepSpeed's bound")
    A.assert_step_within((a.p, a.m, a.v), b, "DeepSpeed in torch's bound")


def test_checker_semantics_for_non_finite_values():
    p, m, v, g = A.inputs(64, 4)
    g[3], g[9], g[20] = float("inf"), float("nan"), float("-inf")
    for mode in MODES:
        h = A.hyper(3, mode, 0.01).f32()
        r = A.reference(p, m, v, g, h)
        assert math.isinf(r.m[3]) and math.isinf(r.v[3]) and math.isnan(r.p[3])
        assert r.m[20] == float("-inf") and r.v[20] == float("inf") and math.isnan(r.p[20])
        assert all(math.isnan(t[9]) for t in (r.p, r.m, r.v))
        got = A.plain_fp32(p, m, v, g, h)
        A.assert_step_within(got, r, "non-finite")
        for bad in (0.0, float("inf")):                        # a finite value or another non-finite one fails
            q = got[0].clone()
            q[3] = bad
            assert A.outside(q, r.p, r.tol_p)[3]
        q = got[1].clone()
        q[5] = float("nan")                                    # a NaN where the reference is finite fails
        assert A.outside(q, r.m, r.tol_m)[5]


def test_clip_scale_follows_the_kernels_branch():
    h = A.hyper(3, max_grad_norm=2.0, grad_scale=0.5).f32()
    assert A.clip_scale(None, h)[:2] == (0.5, False)
    assert A.clip_scale(1e30, h._replace(max_grad_norm=0.0))[:2] == (0.5, False)
    assert A.clip_scale(1.0, h)[:2] == (0.5, False)            # clip = 0.5
    for total, clip, active in A.threshold_totals(2.0):
        s, act, s32 = A.clip_scale(float(total) ** 2, h)
        assert act == active and (np.float32(total) + np.float32(1e-6)) / np.float32(2.0) == np.float32(clip)
        if not active:
            assert s == 0.5
        else:
            assert clip == np.nextafter(np.float32(1), np.float32(2)) and 0.5 * (1 - 2.0 ** -22) < s < 0.5
