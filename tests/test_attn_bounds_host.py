"""The per-element bar on attention (tests/attn_ref.py: ref64_bounds, assert_within_bounds), tested without
a GPU ("The bar on attention").

A torch emulation of the kernels' rounding chain (csrc/attn_kernels.hip: fp32 scores of the 16-bit inputs,
64-key tiles, P against a running max that moves only when a tile's max beats it by more than kFwdThr = 8,
P rounded to the dtype for an fp32 PV product, the 1 / l scale and the 16-bit store; delta from the 16-bit
O, P = exp2(c s - lse), dS rounded to the dtype, the 16-bit stores of dq, dk, dv) must stay inside every
bound; the same emulation with one planted fault must fail the bar; and the file shows which of those
faults the bar of the GPU tests before it (relative Frobenius error <= 8e-3 per tensor, lse within 2e-3)
lets through."""
import pytest
import torch

from tests.attn_ref import (LOG2E, D, allowed_cached, allowed_causal, allowed_docs, assert_within_bounds, inputs, ref32,
                            ref64_bounds, rel)

CPU = torch.device("cpu")
DTYPES = [torch.bfloat16, torch.float16]
B, HQ, HKV = 1, 4, 2
SCALE = D ** -0.5
NAMES = ("o", "dq", "dk", "dv", "lse2")
BOUND = {"o": "b_o", "dq": "b_dq", "dk": "b_dk", "dv": "b_dv", "lse2": "b_lse"}
DIMS = {"o": "bshd", "dq": "bhsd", "dk": "bhsd", "dv": "bhsd", "lse2": "bhs"}


def emulate(q, k, v, g, scale, allowed, M=None, r=1.0, no_rescale=None, delta_from_next=None, dk_without=None,
            allowed_bwd=None):
    """The kernels' chain in torch, fp32 where they are fp32 and rounded to q's dtype where they round.
    Returns o [B, S, Hq, D], dq, dk, dv (the dtype) and lse2 (fp32). The three optional arguments plant a
    fault: ``no_rescale`` (b, h, row): that row's O is not rescaled when its running max moves;
    ``delta_from_next`` (b, h, row): the row takes the next row's delta; ``dk_without`` (b, h, keys):
    head h's term is missing from dk at those key rows; ``allowed_bwd``: the mask of the dQ and dK/dV
    kernels where it is not the forward's."""
    dtype = q.dtype
    Bq, Hq, S, Dh = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    qf, gf = q.detach().float(), g.detach().float().transpose(1, 2)
    kx, vx = k.detach().float().repeat_interleave(G, 1), v.detach().float().repeat_interleave(G, 1)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    al = allowed.expand(Bq, Hq, S, Skv)
    Mu = None if M is None else M.expand(Bq, Hq, S, Skv)
    x = qf @ kx.transpose(-1, -2)
    ninf = float("-inf")
    m_run = torch.full((Bq, Hq, S), ninf)
    l_run = torch.zeros(Bq, Hq, S)
    acc = torch.zeros(Bq, Hq, S, Dh)
    for t0 in range(0, Skv, 64):
        sl = slice(t0, min(t0 + 64, Skv))
        xt = x[..., sl].masked_fill(~al[..., sl], ninf)
        m_tile = xt.amax(-1) * sl2
        move = m_tile > m_run + 8.0
        m_new = torch.where(move, m_tile, m_run)
        alpha = torch.where(move, torch.exp2(m_run - m_new), torch.ones_like(m_run))
        m_use = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
        p = torch.exp2(xt * sl2 - m_use[..., None])
        l_run = l_run * alpha + p.sum(-1)
        m_run = m_new
        a_o = alpha.clone()
        if no_rescale is not None:
            a_o[no_rescale] = 1.0
        acc = acc * a_o[..., None]
        if Mu is not None:
            p = p * Mu[..., sl]
        acc = acc + p.to(dtype).float() @ vx[..., sl, :]
    some = l_run > 0
    inv = torch.where(some, 1.0 / l_run, torch.zeros_like(l_run)) * r
    o16 = (acc * inv[..., None]).to(dtype)
    lse = torch.where(some, m_run + torch.log2(l_run), torch.full_like(l_run, float("inf")))

    delta = (gf * o16.float()).sum(-1)
    if delta_from_next is not None:
        b_, h_, i_ = delta_from_next
        delta[b_, h_, i_] = delta[b_, h_, i_ + 1]
    if allowed_bwd is not None:
        al = allowed_bwd.expand(Bq, Hq, S, Skv)
    P = torch.exp2(x * sl2 - lse[..., None]).masked_fill(~al, 0.0)
    dP = gf @ vx.transpose(-1, -2)
    if Mu is not None:
        dP = torch.where(Mu, dP * r, torch.zeros_like(dP))
    dS16 = (P * (dP - delta[..., None])).to(dtype).float()
    dq = ((dS16 @ kx) * scale).to(dtype)
    dkh = dS16.transpose(-1, -2) @ qf
    if dk_without is not None:
        b_, h_, keys = dk_without
        dkh[b_, h_, keys] = 0.0
    dk = (dkh.view(Bq, Hkv, G, Skv, Dh).sum(2) * scale).to(dtype)
    P16 = (P if Mu is None else P * Mu).to(dtype).float()
    dv = ((P16.transpose(-1, -2) @ gf).view(Bq, Hkv, G, Skv, Dh).sum(2) * r).to(dtype)
    return {"o": o16.transpose(1, 2), "dq": dq, "dk": dk, "dv": dv, "lse2": lse}


def dead_masks(R):
    """The elements each output must hold exactly (0, or +inf for lse): rows without a visible key, keys
    no query of their group sees."""
    dead_row = ~R.visible
    return {"o": dead_row.transpose(1, 2)[..., None], "dq": dead_row[..., None], "dk": ~R.key_live[..., None],
            "dv": ~R.key_live[..., None], "lse2": dead_row}


def judge(got, R):
    """name -> worst err / bound, or the AssertionError that assert_within_bounds raised."""
    dead = dead_masks(R)
    out = {}
    for name in NAMES:
        try:
            out[name] = assert_within_bounds(name, got[name], getattr(R, name), getattr(R, BOUND[name]),
                                             dead=dead[name], dims=DIMS[name],
                                             dead_value=float("inf") if name == "lse2" else 0.0)
        except AssertionError as e:
            out[name] = e
    return out


def old_bar_accepts(got, R):
    """The bar of tests/test_gpu_attention*.py before this file: relative Frobenius error <= 8e-3 on o, dq,
    dk and dv, lse within 2e-3 on the rows with a visible key (and finite values throughout)."""
    for name in ("o", "dq", "dk", "dv"):
        if not torch.isfinite(got[name].float()).all() or not rel(got[name], getattr(R, name)) <= 8e-3:
            return False
    vis = R.visible
    return bool(((got["lse2"].double()[vis] - R.lse2[vis]).abs().max() < 2e-3).item()) if vis.any() else True


def make_inputs(S, dtype, kind, seed=0):
    q, k, v, g = (t.detach() for t in inputs(B, HQ, HKV, S, "hf", dtype, 1000 + S + seed, device=CPU))
    if kind == "flat":
        q = (q.float() * 0.25).to(dtype)
    elif kind == "peaked":
        # every query shares a positive direction and key 200 lies along it: its score beats every earlier
        # one by ~24 log2 units, so the rows from 200 on move their deferred max in the fourth tile
        q = (q.float() * 0.25 + 0.5).to(dtype)
        k = k.clone()
        k[:, :, min(200, S - 1)] = 3.0
    return q, k, v, g


def keep_mask(S):
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[0, :3] = False                         # leading masked keys: rows 0-2 see nothing
    keep[0, 70] = keep[0, 129] = False          # holes
    keep[0, S - S // 5:] = False                # right padding
    return keep


DOC_ROWS = {320: [[70, 1, 59, 100, 90]], 333: [[70, 1, 59, 100, 103]]}       # boundaries off the 64 grid, a length-1 document


def variant(name, S):
    """allowed, M, r of a variant. The dropout mask is a seeded Bernoulli one here (the kernels' keep
    function runs on the GPU only; the bound does not depend on which mask it is)."""
    gen = torch.Generator().manual_seed(S)
    M = r = None
    if "drop" in name:
        M, r = torch.rand(B, HQ, S, S, generator=gen) >= 26 / 256, 1.0 / (1.0 - 26 / 256)
    if name.startswith("kmask"):
        al = allowed_causal(S, keep_mask(S), device=CPU)
    elif name.startswith("docs"):
        al = allowed_docs(DOC_ROWS[S], S, device=CPU)
    else:
        al = allowed_causal(S, device=CPU)
    return al, M, (r or 1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("S", [320, 333])
@pytest.mark.parametrize("name,kind", [("plain", "normal"), ("plain", "flat"), ("plain", "peaked"), ("kmask", "normal"),
                                       ("docs", "normal"), ("drop", "normal"), ("kmask+drop", "flat"),
                                       ("docs+drop", "normal")])
def test_emulation_is_inside_every_bound(name, kind, S, dtype):
    q, k, v, g = make_inputs(S, dtype, kind)
    al, M, r = variant(name, S)
    R = ref64_bounds(q, k, v, g, SCALE, al, M, r)
    res = judge(emulate(q, k, v, g, SCALE, al, M, r), R)
    print(f"{name} {kind} S={S} {dtype}: worst err/bound",
          ", ".join(f"{n} {res[n]:.3f}" if isinstance(res[n], float) else f"{n} FAILS" for n in NAMES))
    for n in NAMES:
        assert isinstance(res[n], float), res[n]


# ---- planted faults ---------------------------------------------------------------------------------------
S_F = 333
LATE = 301                                      # a late row: tile 4, q block 2, wave 1


def _edge(al, extra, row=LATE):
    al = al.expand(B, HQ, S_F, S_F).clone()
    if extra:
        al[0, 1, row, row + 1] = True           # the row sees key q + 1
    else:
        al[0, 1, row, row] = False              # the row does not see key q
    return al


def _quiet_row(R, q, k):
    """The late row (the last q block) of head 1 whose key q + 1 is the heaviest stray key that the old lse
    bar still cannot see: the lse of a row that gains a key of weight w (relative to the row's sum) moves
    by log2(1 + w), and the old bar accepts less than 2e-3."""
    s2 = (q[0, 1].double() @ k[0, 0].double().T) * (SCALE * LOG2E)
    rows = torch.arange(256, S_F - 1)
    shift = torch.log2(1.0 + torch.exp2(s2[rows, rows + 1] - R.lse2[0, 1, rows]))
    shift = torch.where(shift < 2e-3, shift, torch.zeros_like(shift))
    return int(rows[shift.argmax()])


def _tile_skipped(al):
    al = al.expand(B, HQ, S_F, S_F).clone()
    al[0, 2, S_F - 20:, 128:192] = False        # one 64-key tile, the last 20 rows, one head
    return al


def _chunk(o):
    o = o.clone()
    o[0, LATE, 1, 16:24] = o[0, LATE, 1, 8:16]
    return o


def _stale(o):
    o = o.clone()
    o[0, LATE, 1] = o[0, LATE - 128, 1]          # what an earlier launch left there
    return o


def _nan(t):
    t = t.clone()
    t[0, 1, LATE, 77] = float("nan")
    return t


# name -> (inputs, variant, what to do): "mask" replaces the mask the emulation runs under ("mask_bwd": its
# backward only, which leaves o and lse as they were), "kw" hands emulate
# a fault argument, "post" rewrites one output afterwards, "M" replaces the dropout mask the emulation applies
FAULTS = {
    "edge: key q+1 visible": ("flat", "plain", ("mask", lambda al, *_: _edge(al, True))),
    "edge: key q invisible": ("flat", "plain", ("mask", lambda al, *_: _edge(al, False))),
    "edge: key q+1 visible, the heaviest one the old lse bar accepts":
        ("normal", "plain", ("mask", lambda al, R, q, k: _edge(al, True, _quiet_row(R, q, k)))),
    "edge: key q+1 visible in dQ and dK/dV only": ("flat", "plain", ("mask_bwd", lambda al, *_: _edge(al, True))),
    "a tile skipped for 20 rows of one head": ("flat", "plain", ("mask", lambda al, *_: _tile_skipped(al))),
    "a GQA head missing from dk at four keys": ("normal", "plain", ("kw", {"dk_without": (0, 3, slice(40, 44))})),
    "a misplaced 8-element chunk": ("normal", "plain", ("post", "o", _chunk)),
    "a stale row": ("normal", "plain", ("post", "o", _stale)),
    "delta from the next row": ("normal", "plain", ("kw", {"delta_from_next": (0, 1, LATE)})),
    "O not rescaled when the max moves": ("peaked", "plain", ("kw", {"no_rescale": (0, 1, LATE)})),
    "one NaN": ("normal", "plain", ("post", "dq", _nan)),
    "dropout mask shifted by one key": ("flat", "drop", ("M", lambda M: M.roll(1, -1))),
}


def _faulted(fault, dtype):
    kind, var, what = FAULTS[fault]
    q, k, v, g = make_inputs(S_F, dtype, kind)
    al, M, r = variant(var, S_F)
    R = ref64_bounds(q, k, v, g, SCALE, al, M, r)
    clean = emulate(q, k, v, g, SCALE, al, M, r)
    if what[0] == "mask":
        got = emulate(q, k, v, g, SCALE, what[1](al, R, q, k), M, r)
    elif what[0] == "mask_bwd":
        got = emulate(q, k, v, g, SCALE, al, M, r, allowed_bwd=what[1](al, R, q, k))
    elif what[0] == "M":
        got = emulate(q, k, v, g, SCALE, al, what[1](M), r)
    elif what[0] == "kw":
        got = emulate(q, k, v, g, SCALE, al, M, r, **what[1])
    else:
        got = dict(clean)
        got[what[1]] = what[2](clean[what[1]])
    return clean, got, R


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_fails_the_bar(fault, dtype):
    clean, got, R = _faulted(fault, dtype)
    base = judge(clean, R)
    assert all(isinstance(x, float) for x in base.values()), base      # the unfaulted run is inside every bound
    res = judge(got, R)
    caught = [n for n in NAMES if not isinstance(res[n], float)]
    print(f"{fault} {dtype}: fails on {caught}; the old bar {'accepts' if old_bar_accepts(got, R) else 'refuses'} it")
    for n in caught:
        print("   ", res[n])
    assert caught, f"{fault}: inside every bound: {res}"


def test_the_old_bar_accepts_faults_the_new_one_refuses():
    """Which planted faults pass `rel <= 8e-3` per tensor and `|lse error| < 2e-3`, though every one of them
    fails assert_within_bounds (the test above). The off-by-one causal edge passes every Frobenius bar in both
    dtypes; the old lse bar sees it in the forward only where the stray key weighs more than 2e-3 ln 2 of the
    row's sum, and never in the backward kernels, which write no lse."""
    accepted = []
    for dtype in DTYPES:
        for fault in FAULTS:
            clean, got, R = _faulted(fault, dtype)
            assert old_bar_accepts(clean, R)
            if old_bar_accepts(got, R):
                accepted.append((fault, dtype))
    print("the old bar accepts:", accepted)
    for dtype in DTYPES:
        assert ("edge: key q+1 visible, the heaviest one the old lse bar accepts", dtype) in accepted
        assert ("edge: key q+1 visible in dQ and dK/dV only", dtype) in accepted


# ---- the reference itself ------------------------------------------------------------------------------------
def _masks():
    S = 77
    keep = torch.ones(2, S, dtype=torch.bool)
    keep[0, :2] = False
    keep[1, 40] = False
    keep[1, 60:] = False
    yield "causal", S, S, allowed_causal(S, device=CPU)
    yield "causal + key mask", S, S, allowed_causal(S, keep, device=CPU)
    yield "documents", S, S, allowed_docs([[30, 1, 46], [77]], S, device=CPU)
    yield "cached", 5, S, allowed_cached(2, 5, S, 40, device=CPU)
    yield "cached + key mask, a position per row", 5, S, allowed_cached(2, 5, S, torch.tensor([72, 0]), keep, device=CPU)


@pytest.mark.parametrize("case", list(_masks()), ids=lambda c: c[0])
def test_ref64_agrees_with_ref32(case):
    """ref32 is the same attention in fp32: it must sit inside the bounds of the model at u = 2^-24 (an
    fp32 P, dS and store), on every mask builder of attn_ref."""
    _, Sq, Skv, al = case
    torch.manual_seed(3)
    q = torch.randn(2, 4, Sq, D).bfloat16()
    k, v = torch.randn(2, 2, Skv, D).bfloat16(), torch.randn(2, 2, Skv, D).bfloat16()
    g = torch.randn(2, Sq, 4, D).bfloat16()
    o, dq, dk, dv, lse2, vis = ref32(q, k, v, g, SCALE, al)
    R = ref64_bounds(q, k, v, g, SCALE, al, dtype=torch.float32)
    assert torch.equal(vis, R.visible)
    lse2 = lse2.masked_fill(~vis, float("inf"))          # ref32 leaves logsumexp's -inf on a row without a key
    res = judge({"o": o, "dq": dq, "dk": dk, "dv": dv, "lse2": lse2}, R)
    print({n: (f"{x:.3f}" if isinstance(x, float) else "FAIL") for n, x in res.items()})
    for n in NAMES:
        assert isinstance(res[n], float), res[n]


def test_assert_within_bounds_excuses_nothing():
    want = torch.zeros(1, 2, 300, 8, dtype=torch.float64)
    bound = torch.full_like(want, 1e-3)
    got = want.clone()
    assert assert_within_bounds("x", got, want, bound) == 0.0
    got[0, 1, 200, 3] = 1.0001e-3                # one element of 4800, by 0.01 %
    with pytest.raises(AssertionError, match=r"1 of 4800 .*row 200: tile 3, q block 1 wave 2.*head 1"):
        assert_within_bounds("x", got, want, bound)
    got[0, 1, 200, 3] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_within_bounds("x", got, want, bound)
    dead = torch.zeros(1, 2, 300, 1, dtype=torch.bool)
    dead[0, 0, 5] = True
    got = want.clone()
    got[0, 0, 5, 0] = 1e-30                      # inside the bound, but a dead row holds exact zeros
    with pytest.raises(AssertionError, match="dead"):
        assert_within_bounds("x", got, want, bound, dead=dead)
    lse = torch.tensor([[[float("inf"), 1.0]]], dtype=torch.float64)
    d = torch.tensor([[[True, False]]])
    assert assert_within_bounds("lse", lse, lse.clone(), torch.full_like(lse, 1e-6), dead=d, dead_value=float("inf")) == 0.0
    with pytest.raises(AssertionError, match="dead"):
        assert_within_bounds("lse", torch.tensor([[[50.0, 1.0]]]), lse, torch.full_like(lse, 1e-6), dead=d,
                             dead_value=float("inf"))
