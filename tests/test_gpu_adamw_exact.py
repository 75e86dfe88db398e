"""Per-element tests of the optimizer step: ``smt_adamw_step`` (flat and tiled), ``smt_adamw_multi`` and
``smt_sq_norm`` against the fp64 references and derived bounds of tests/adamw_ref.py.

Every case is one launch from the random state of ``adamw_ref.inputs`` (step 3, betas (0.9, 0.95),
eps 1e-8, lr 1e-3, wd 0 and 0.01). ``master``, ``exp_avg`` and ``exp_avg_sq`` are judged element by
element, no element left out; ``param`` is ``master'`` rounded to the parameter dtype, bit for bit;
guard elements after ``n`` in all four written buffers keep their sentinel.
"""
import math
import os

import numpy as np
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from tests import adamw_ref as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MODES = [A.DEEPSPEED, A.TORCH]
PAIRS = [(torch.float32, torch.bfloat16), (torch.float32, torch.float16), (torch.float32, torch.float32),
         (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)]
FLAT_N = [1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 5]
S = 0.37
GUARD = 64
SENTINEL = -8192.0                       # exact in bf16, fp16 and fp32
TILE = 65536
REPORT = bool(os.environ.get("ADAMW_REF_REPORT"))


def _ids(v):
    if isinstance(v, tuple):
        return "-".join(_ids(t) for t in v)
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    return {A.DEEPSPEED: "deepspeed", A.TORCH: "torch"}[v]


def _args(h: A.Hyper):
    return _hip.AdamWArgs(lr=h.lr, beta1=h.beta1, beta2=h.beta2, eps=h.eps, weight_decay=h.weight_decay,
                          bias_correction1=h.bc1, bias_correction2=h.bc2, max_grad_norm=h.max_grad_norm,
                          grad_scale=h.grad_scale, mode=h.mode, grad_dtype=0)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class State:
    """Device copies of (g, p, m, v, param) with ``GUARD`` sentinel elements after the ``n`` in use."""

    def __init__(self, p, m, v, g, pdt, gdt=torch.float32):
        self.n, self.pdt = p.numel(), pdt
        self.g_host = g.to(gdt)                                        # the gradient the kernel reads
        self.host = (p, m, v)

        def guarded(t, dt):
            buf = torch.full((self.n + GUARD,), SENTINEL, dtype=dt, device=DEV)
            buf[:self.n] = t.to(dt).to(DEV)
            return buf
        self.bufs = [guarded(p, torch.float32), guarded(m, torch.float32), guarded(v, torch.float32), guarded(p, pdt)]
        self.g = self.g_host.to(DEV)

    def views(self):
        return [b[:self.n] for b in self.bufs]

    def step(self, h, norm_sq=None, tiles=None, n_tiles=0, g=None):
        norm = None if norm_sq is None else torch.tensor([norm_sq], dtype=torch.float64, device=DEV)
        _hip.adamw_step(self.g if g is None else g, *self.views(), _args(h), tiles=tiles, n_tiles=n_tiles,
                        grad_sq_norm=norm)
        torch.cuda.synchronize()
        return self

    def out(self):
        return [b[:self.n].cpu() for b in self.bufs]

    def check_guards(self, what):
        for name, b in zip(("master", "exp_avg", "exp_avg_sq", "param"), self.bufs):
            assert bool((b[self.n:] == SENTINEL).all()), f"{what}: wrote past n in {name}"

    def check_param(self, what):
        """param == master' rounded to the parameter dtype, bit for bit (any NaN for a NaN)."""
        master, _, _, param = self.out()
        want = master.to(self.pdt)
        nan = torch.isnan(master)
        assert bool(torch.isnan(param.float())[nan].all()), f"{what}: param is not NaN where master is"
        assert torch.equal(_bits(param)[~nan], _bits(want)[~nan]), f"{what}: param is not master' in {self.pdt}"


def _check(state: State, h, norm_sq, what, report=None):
    r = A.reference(*state.host, state.g_host.float(), h, norm_sq)
    out = state.out()
    ratios = A.assert_step_within(out[:3], r, what)
    state.check_param(what)
    state.check_guards(what)
    if report is not None:
        for k, x in ratios.items():
            report[k] = max(report.get(k, 0.0), x)
    return r


def _show(what, report):
    if REPORT:
        print(f"\nADAMW_RATIO {what}: " + " ".join(f"{k} {x:.2f}" for k, x in sorted(report.items())))


# ------------------------------------------------------------------------------------------------
# per element against the fp64 reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_flat_kernel_per_element(mode, pair):
    gdt, pdt = pair
    report = {}
    for n in FLAT_N:
        for wd in (0.0, 0.01):
            h = A.hyper(3, mode, wd, grad_scale=S).f32()
            p, m, v, g = A.inputs(n, n, S)
            st = State(p, m, v, g, pdt, gdt).step(h)
            _check(st, h, None, f"flat n={n} wd={wd}", report)
    _show(f"flat {_ids(mode)} {_ids(pair)}", report)


def _tile_entries(n_tiles):
    """One [512, 512] W, tiles in ascending flat order."""
    return [(1, 0), (0, 1), (1, 1), (0, 0)][:n_tiles]


@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("pdt", [torch.bfloat16, torch.float16, torch.float32], ids=_ids)
def test_tiled_kernel_per_element_and_equal_to_flat(mode, pdt):
    n_tiles = 3
    n = n_tiles * TILE
    report = {}
    for wd in (0.0, 0.01):
        h = A.hyper(3, mode, wd, grad_scale=S).f32()
        p, m, v, g = A.inputs(n, 7, S)
        W = torch.full((512, 512), SENTINEL, dtype=pdt, device=DEV)
        tiles = _tile_entries(n_tiles)
        descs = _hip.tile_descs([(W, r, c, i * TILE) for i, (r, c) in enumerate(tiles)], DEV, pdt)
        tiled = State(p, m, v, g, pdt).step(h, tiles=descs, n_tiles=n_tiles)
        _check(tiled, h, None, f"tiled wd={wd}", report)
        flat = State(p, m, v, g, pdt).step(h)
        for name, a, b in zip(("master", "exp_avg", "exp_avg_sq", "param"), tiled.out(), flat.out()):
            assert _same_bits(a, b), f"tiled != flat in {name}"
        param = tiled.out()[3].view(n_tiles, 256, 256)
        Wc = W.cpu()
        for i, (r, c) in enumerate(tiles):
            assert _same_bits(Wc[r * 256:(r + 1) * 256, c * 256:(c + 1) * 256], param[i]), f"W tile {(r, c)}"
        assert bool((Wc[:256, :256] == SENTINEL).all()), "the unselected tile of W changed"
    _show(f"tiled {_ids(mode)} float32-{_ids(pdt)}", report)


# ------------------------------------------------------------------------------------------------
# the clip
# ------------------------------------------------------------------------------------------------
def _clip_state(seed, pdt=torch.bfloat16):
    n = 3 * 2048 + 5
    return n, A.inputs(n, seed, S), pdt


@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_clip_cases_that_do_not_apply_equal_the_null_norm_launch(mode):
    """max_grad_norm = 0 with a norm, a norm with clip <= 1, and clip exactly 1.0: each within the bound for
    the reference's s = grad_scale and bit-identical to the launch without a norm."""
    n, (p, m, v, g), pdt = _clip_state(11)
    h0 = A.hyper(3, mode, 0.01, max_grad_norm=2.0, grad_scale=S).f32()
    null = State(p, m, v, g, pdt).step(h0)
    r0 = _check(null, h0, None, "NULL norm")
    assert not r0.active and r0.s == h0.grad_scale
    (t_one, clip_one, active_one), _ = A.threshold_totals(2.0)
    assert clip_one == 1 and not active_one
    cases = {"max_grad_norm = 0": (h0._replace(max_grad_norm=0.0), 1e30),
             "max_grad_norm < 0": (h0._replace(max_grad_norm=-1.0), 1e30),
             "clip <= 1": (h0, 1.5 ** 2),
             "clip == 1.0": (h0, float(t_one) ** 2)}
    for what, (h, norm_sq) in cases.items():
        st = State(p, m, v, g, pdt).step(h, norm_sq)
        r = _check(st, h, norm_sq, what)
        assert not r.active and r.s == h0.grad_scale, what
        for name, a, b in zip(("master", "exp_avg", "exp_avg_sq", "param"), st.out(), null.out()):
            assert _same_bits(a, b), f"{what}: {name} differs from the NULL-norm launch"


@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_clip_at_the_first_value_above_one_applies(mode):
    n, (p, m, v, g), pdt = _clip_state(12)
    h = A.hyper(3, mode, 0.01, max_grad_norm=2.0, grad_scale=S).f32()
    _, (t_above, clip_above, active) = A.threshold_totals(2.0)
    assert active and clip_above == np.nextafter(np.float32(1), np.float32(2))
    norm_sq = float(t_above) ** 2
    st = State(p, m, v, g, pdt).step(h, norm_sq)
    r = _check(st, h, norm_sq, "clip = 1 + 2^-23")
    assert r.active and r.s < h.grad_scale
    # the kernel's own fp32 scale is one step below grad_scale, so exp_avg_sq cannot equal the unclipped launch
    assert A.clip_scale(norm_sq, h)[2] != np.float32(h.grad_scale)
    null = State(p, m, v, g, pdt).step(h)
    assert not _same_bits(st.out()[2], null.out()[2])


@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("unscale", [False, True], ids=["gs1", "gs2^-16"])
def test_clip_active_per_element(mode, unscale):
    """The clip active on the true norm of the effective gradient, s ~ 0.37 of grad_scale; with
    grad_scale = 2^-16 on a loss-scaled gradient (the fp16 unscale composing with the clip)."""
    gs, g_mul = (2.0 ** -16, 2.0 ** 16) if unscale else (1.0, 1.0)
    n = 3 * 2048 + 5
    p, m, v, g = A.inputs(n, 13, S * gs, g_mul)
    norm_sq = math.fsum(((g.double() * gs) ** 2).tolist())
    report = {}
    for wd in (0.0, 0.01):
        h = A.hyper(3, mode, wd, max_grad_norm=S * math.sqrt(norm_sq), grad_scale=gs).f32()
        st = State(p, m, v, g, torch.float16 if unscale else torch.bfloat16).step(h, norm_sq)
        r = _check(st, h, norm_sq, f"clip active wd={wd}", report)
        assert r.active and abs(r.s / gs - S) < 1e-6
    _show(f"clip active {_ids(mode)} grad_scale {gs}", report)


# ------------------------------------------------------------------------------------------------
# tolerance-free identities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("gdt", [torch.bfloat16, torch.float16], ids=_ids)
def test_16_bit_gradient_equals_the_same_values_in_fp32(mode, gdt):
    n = 3 * 2048 + 5
    p, m, v, g = A.inputs(n, 21, S)
    h = A.hyper(3, mode, 0.01, grad_scale=S).f32()
    narrow = State(p, m, v, g, gdt, gdt).step(h)
    wide = State(p, m, v, g.to(gdt).float(), gdt).step(h)
    for name, a, b in zip(("master", "exp_avg", "exp_avg_sq", "param"), narrow.out(), wide.out()):
        assert _same_bits(a, b), name


@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_grad_scale_half_equals_halved_gradient(mode):
    n = 3 * 2048 + 5
    p, m, v, g = A.inputs(n, 22, 0.5)
    a = State(p, m, v, g, torch.bfloat16).step(A.hyper(3, mode, 0.01, grad_scale=0.5).f32())
    b = State(p, m, v, g * 0.5, torch.bfloat16).step(A.hyper(3, mode, 0.01, grad_scale=1.0).f32())
    for name, x, y in zip(("master", "exp_avg", "exp_avg_sq", "param"), a.out(), b.out()):
        assert _same_bits(x, y), name


@pytest.mark.parametrize("gdt", [torch.bfloat16, torch.float32], ids=_ids)
def test_multi_equals_per_tensor_steps_in_torch_mode_with_an_empty_tensor(gdt):
    """``smt_adamw_multi`` in SMT_ADAM_TORCH over ragged tensors with a zero-element tensor in the middle of
    the table: bit for bit the per-tensor ``smt_adamw_step``, the empty tensor a no-op for its neighbours."""
    sizes = [7, 2049, 0, 2048, 1, 3 * 2048 + 5]
    h = A.hyper(3, A.TORCH, 0.01, max_grad_norm=1.0, grad_scale=0.5).f32()
    norm = torch.tensor([4.0], dtype=torch.float64, device=DEV)
    multi, solo = [], []
    for k, n in enumerate(sizes):
        p, m, v, g = A.inputs(n, 30 + k, 0.25)
        multi.append(State(p, m, v, g, torch.bfloat16, gdt))
        solo.append(State(p, m, v, g, torch.bfloat16, gdt))
    _hip.adamw_multi([(s.g, *s.views()) for s in multi], _args(h), grad_sq_norm=norm)
    for s in solo:
        _hip.adamw_step(s.g, *s.views(), _args(h), grad_sq_norm=norm)
    torch.cuda.synchronize()
    for n, a, b in zip(sizes, multi, solo):
        for name, x, y in zip(("master", "exp_avg", "exp_avg_sq", "param"), a.out(), b.out()):
            assert _same_bits(x, y), (n, name)
        a.check_guards(f"multi n={n}")
        if n:
            r = A.reference(*a.host, a.g_host.float(), h, 4.0)
            assert r.active
            A.assert_step_within(a.out()[:3], r, f"multi n={n}")
            a.check_param(f"multi n={n}")


# ------------------------------------------------------------------------------------------------
# the tiled layout of the engine: several W, views, a permutation, a NULL weight
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdt", [torch.bfloat16, torch.float32], ids=_ids)
def test_tiled_layout_as_the_engine_uses_it(pdt):
    """One launch over two W with different leading dimensions, one a column-slice view of a wider matrix;
    flat offsets a non-monotonic permutation; one descriptor without a weight; one tile in the last row and
    column block of its W."""
    n_tiles = 4
    n = n_tiles * TILE
    h = A.hyper(3, A.DEEPSPEED, 0.01, grad_scale=S).f32()
    p, m, v, g = A.inputs(n, 41, S)
    W1 = torch.full((512, 768), SENTINEL, dtype=pdt, device=DEV)                 # ld 768
    base = torch.full((512, 536), SENTINEL, dtype=pdt, device=DEV)               # ld 536 > the view's 512 columns
    W2 = base[:, 8:8 + 512]
    assert W2.stride(0) == 536 and W2.data_ptr() % 16 == 0
    # (W, row block, column block, flat offset in tiles)
    entries = [(W1, 1, 2, 2), (W2, 0, 1, 0), (None, 1, 1, 3), (W2, 1, 1, 1)]
    descs = _hip.tile_descs([(w, r, c, k * TILE) for w, r, c, k in entries], DEV, pdt)
    before_param = p.to(pdt)
    st = State(p, m, v, g, pdt).step(h, tiles=descs, n_tiles=n_tiles)
    _check(st, h, None, "engine layout")
    flat = State(p, m, v, g, pdt).step(h)
    for name, a, b in zip(("master", "exp_avg", "exp_avg_sq", "param"), st.out(), flat.out()):
        assert _same_bits(a, b), f"tiled != flat in {name}"
    param = st.out()[3].view(n_tiles, 256, 256)
    want1 = torch.full((512, 768), SENTINEL, dtype=pdt)
    want2 = torch.full((512, 536), SENTINEL, dtype=pdt)
    want1[256:512, 512:768] = param[2]
    want2[0:256, 8 + 256:8 + 512] = param[0]
    want2[256:512, 8 + 256:8 + 512] = param[1]
    assert _same_bits(W1.cpu(), want1), "W1: a tile is not param, or something else changed"
    assert _same_bits(base.cpu(), want2), "W2: a tile is not param, or the view's padding / other tiles changed"
    # the tile without a weight is still stepped
    assert not _same_bits(param[3], before_param.view(n_tiles, 256, 256)[3])


# ------------------------------------------------------------------------------------------------
# non-finite gradients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_ids)
@pytest.mark.parametrize("gdt", [torch.float32, torch.float16], ids=_ids)
def test_non_finite_gradients_stay_in_their_elements(mode, gdt):
    """An inf and a NaN in separate eight-element groups and one in the scalar tail: the reference's
    non-finite values at exactly those elements, every other element within its bound."""
    n = 3 * 2048 + 5
    inf, nan = float("inf"), float("nan")
    for plant in ({10: inf, 2048 + 17: nan, n - 3: -inf}, {3: nan, 4096 + 100: -inf, n - 1: nan, n - 5: inf}):
        p, m, v, g = A.inputs(n, 51, S)
        for i, x in plant.items():
            g[i] = x
        h = A.hyper(3, mode, 0.01, grad_scale=S).f32()
        st = State(p, m, v, g, gdt, gdt).step(h)
        r = _check(st, h, None, f"non-finite {sorted(plant)}")
        bad = ~torch.isfinite(r.p)
        assert sorted(bad.nonzero().flatten().tolist()) == sorted(plant)
        master, em, ev, _ = st.out()
        for t in (master, em, ev):
            assert sorted((~torch.isfinite(t)).nonzero().flatten().tolist()) == sorted(plant)


# ------------------------------------------------------------------------------------------------
# smt_sq_norm
# ------------------------------------------------------------------------------------------------
SQ_N = [0, 1, 3, 4, 5, 1023, 262147]


def _sq_buffers():
    """For each n: (aligned view, view offset by one element (the unaligned path), fsum of the fp64 squares)."""
    gen = torch.Generator().manual_seed(77)
    out = {}
    for n in SQ_N:
        mag = torch.exp(math.log(1e-20) + torch.rand(n + 1, generator=gen, dtype=torch.float64) * math.log(1e39))
        x = (mag * (torch.randint(0, 2, (n + 1,), generator=gen).double() * 2 - 1)).float()
        base = x.to(DEV)
        views = (base[:n], base[1:1 + n])
        assert views[0].data_ptr() % 16 == 0 and (n == 0 or views[1].data_ptr() % 16 == 4)
        out[n] = [(w, math.fsum((w.double().cpu() ** 2).tolist())) for w in views]
    return out


@pytest.fixture(scope="module")
def sq_buffers():
    return _sq_buffers()


@pytest.mark.parametrize("n_partials", [1, 7, 1024])
def test_sq_norm_against_fsum(sq_buffers, n_partials):
    for n in SQ_N:
        for path, (x, want) in zip(("aligned", "unaligned"), sq_buffers[n]):
            got = _hip.sq_norm(x, n_partials=n_partials).item()
            again = _hip.sq_norm(x, n_partials=n_partials).item()
            what = f"n={n} {path} n_partials={n_partials}"
            assert got == want if n == 0 else math.isclose(got, want, rel_tol=1e-12), (what, got, want)
            assert np.float64(got).tobytes() == np.float64(again).tobytes(), f"{what}: two calls differ"


@pytest.mark.parametrize("n_partials", [1, 1024])
def test_sq_norm_of_values_whose_fp32_square_overflows(n_partials):
    n = 1023
    x = torch.full((n + 1,), 3e38)
    x[::2] = -3e38
    base = x.to(DEV)
    for view in (base[:n], base[1:1 + n]):
        want = math.fsum((view.double().cpu() ** 2).tolist())
        got = _hip.sq_norm(view, n_partials=n_partials).item()
        assert math.isfinite(got) and math.isclose(got, want, rel_tol=1e-12), (got, want)


@pytest.mark.parametrize("n,n_partials", [(1023, 7), (262147, 1024)])
def test_sq_norm_propagates_a_single_non_finite_value(sq_buffers, n, n_partials):
    """One +inf, -inf or NaN first, in the middle or in the last n % 4 elements, on the aligned and on the
    unaligned path: +inf for an inf, NaN for a NaN, and ``torch.isfinite`` false (what engine.step reads)."""
    assert n % 4 == 3
    for path, (x, _) in zip(("aligned", "unaligned"), sq_buffers[n]):
        for pos in (0, n // 2, n - 1, n - 3):
            for val in (float("inf"), float("-inf"), float("nan")):
                y = x.clone() if path == "aligned" else torch.cat([x[:1], x])[1:]
                assert (y.data_ptr() % 16 == 0) == (path == "aligned")
                y[pos] = val
                out = _hip.sq_norm(y, n_partials=n_partials)
                assert not bool(torch.isfinite(out).any()), (path, pos, val)
                got = out.item()
                assert math.isnan(got) if math.isnan(val) else got == float("inf"), (path, pos, val, got)
