"""The one fp32 reference of the flash-attention GPU tests (tests/test_gpu_attention*.py): attention under
an explicit boolean mask ``allowed`` [B, 1 or Hq, Sq, Skv] (True = query i sees key j), the 16-bit eager
attention under the same mask that sets the tests' error bar, the builders of the three masks the kernels
implement (causal with an optional key mask, block-diagonal causal from document lengths, a call against
a KV cache at ``q_offset``), the error measure and the seeded inputs. Below them, the per-element bar
(tests/test_gpu_attention_bounds.py, tests/test_attn_bounds_host.py): ``ref64_bounds``, the same attention
in fp64 with a derived error bound for every element of every output, and ``assert_within_bounds``. The
builders and ``inputs`` take a ``device`` (default: the GPU) so that the host tests can run them.

Conventions, those of the kernels (include/smt_attention.h): q [B, Hq, Sq, D], k / v [B, Hkv, Skv, D],
o and its gradient g [B, Sq, Hq, D]; lse in log2 units of the scaled scores, that of the undropped
probabilities; a row without a visible key has a zero output, zero gradients and lse = +inf. Dropout is
the keep mask M [B, Hq, Sq, Skv] times r = 1 / (1 - p_eff) on the probabilities of the PV product."""
import math

import torch

DEV = torch.device("cuda", 0)
D = 128


def rel(a, b):
    """Relative Frobenius error of a against b."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def allowed_causal(S, keep=None, device=None):
    """[1 or B, 1, S, S]: causal, and key j kept by ``keep`` [B, S] (bool) where one is given."""
    causal = torch.ones(S, S, dtype=torch.bool, device=device or DEV).tril()[None, None]
    return causal if keep is None else causal & keep[:, None, None, :]


def allowed_docs(rows, S, device=None):
    """The block-diagonal causal mask [B, 1, S, S], written out from the document lengths of each row."""
    m = torch.zeros(len(rows), 1, S, S, dtype=torch.bool)
    for b, lens in enumerate(rows):
        assert sum(lens) == S
        at = 0
        for n in lens:
            m[b, 0, at:at + n, at:at + n] = torch.ones(n, n, dtype=torch.bool).tril()
            at += n
    return m.to(device or DEV)


def allowed_cached(B, Sq, Skv, q_offset, keep=None, device=None):
    """[B, 1, Sq, Skv]: query i sits at position q_offset + i (an int, or one position per batch row as a
    [B] tensor) and sees key j <= its position, and kept by ``keep`` [B, Skv] where one is given."""
    dev = device or DEV
    pos = torch.as_tensor(q_offset, device=dev).reshape(-1, 1) + torch.arange(Sq, device=dev)[None]      # [1 or B, Sq]
    a = (torch.arange(Skv, device=dev)[None, None, :] <= pos[:, :, None]).expand(B, Sq, Skv)
    return (a & keep[:, None, :] if keep is not None else a)[:, None]


def _masked_scores(qx, kx, scale, allowed):
    G = qx.shape[1] // kx.shape[1]
    s = (qx @ kx.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    return s.masked_fill(~allowed, float("-inf")), allowed.any(-1, keepdim=True)


def ref32(q, k, v, g, scale, allowed, M=None, r=1.0):
    """fp32 attention of the 16-bit inputs under ``allowed``, gradients by autograd of g (None: forward
    only, the gradients are None). Returns o [B, Sq, Hq, D], dq, dk, dv, lse2 [B, Hq, Sq] and the rows
    with a visible key (bool, lse2's shape)."""
    qf, kf, vf = (t.detach().float().requires_grad_(g is not None) for t in (q, k, v))
    s, any_key = _masked_scores(qf, kf, scale, allowed)
    p = torch.softmax(s.masked_fill(~any_key, 0.0), -1) * any_key
    if M is not None:
        p = p * (M.float() * r)
    o = p @ vf.repeat_interleave(q.shape[1] // k.shape[1], 1)
    if g is not None:
        o.transpose(1, 2).backward(g.float())
    lse2 = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    return o.transpose(1, 2).detach(), qf.grad, kf.grad, vf.grad, lse2, any_key.squeeze(-1).expand_as(lse2)


def eager16(q, k, v, g, scale, allowed, M=None, r=1.0):
    """16-bit eager attention under the same mask, in transformers' eager_attention_forward order: scores
    in the dtype, fp32 softmax cast to the dtype, times M r, the PV matmul in the dtype."""
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s, any_key = _masked_scores(qs, ks, scale, allowed)
    p = (torch.softmax(s.masked_fill(~any_key, 0.0), -1, dtype=torch.float32) * any_key).to(q.dtype)
    if M is not None:
        p = p * (M.to(q.dtype) * r)
    o = p @ vs.repeat_interleave(q.shape[1] // k.shape[1], 1)
    o.transpose(1, 2).backward(g)
    return o.transpose(1, 2).detach(), qs.grad, ks.grad, vs.grad


def inputs(B, Hq, Hkv, S, layout, dtype, seed, device=None):
    """Seeded leaves q, k, v and the output gradient g, drawn in that order."""
    torch.manual_seed(seed)
    dev = device or DEV
    if layout == "hf":      # [B, S, H, D] storage viewed as [B, H, S, D], as transformers hands them over
        mk = lambda H: torch.randn(B, S, H, D, device=dev).to(dtype).transpose(1, 2).requires_grad_(True)
    else:
        mk = lambda H: torch.randn(B, H, S, D, device=dev).to(dtype).requires_grad_(True)
    return mk(Hq), mk(Hkv), mk(Hkv), torch.randn(B, S, Hq, D, device=dev).to(dtype)


# ---- the per-element bar: an fp64 reference with a derived elementwise error bound -------------------------
# DESIGN.md, "The bar on attention", derives every constant below; none is fitted to what a GPU returns.
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
F32 = 2.0 ** -24                    # unit roundoff of one fp32 operation rounded to nearest
ULP32 = 2.0 ** -23                  # one ulp, relative: v_exp_f32 and v_log_f32 are 1-ulp instructions
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: F32}     # fp32: ref32 against this model
KEY_TILE = 64                       # keys per tile of the forward, dQ and decode sweeps
FWD_THR = 8.0                       # kFwdThr: the running max lags the true one by at most this, log2 units
SECOND_ORDER = 4.0                  # (1 + u)^3 <= 1 + 4u: operand rounding, fp32 error and the final store compound
TILE_OPS = 72.0                     # fp32 roundings per 64-key tile on a row's running sum and accumulator


def _acc(n):
    """Relative error, on the sum of magnitudes, of an MFMA chain that accumulates n products: n adds
    inside the 16-wide steps and n / 16 adds onto the accumulator, each one rounding of at most one ulp
    (the ISA does not promise round-to-nearest inside the MFMA adder)."""
    return (n + n / 16.0) * ULP32


class Ref64:
    """What :func:`ref64_bounds` returns: o [B, Sq, Hq, D], dq [B, Hq, Sq, D], dk / dv [B, Hkv, Skv, D],
    lse2 [B, Hq, Sq] (fp64), a bound of the same shape for each (b_o, b_dq, b_dk, b_dv, b_lse), the rows
    with a visible key (``visible``, lse2's shape) and the keys some query of their group sees
    (``key_live`` [B, Hkv, Skv]); ``delta`` = rowsum(dO * O) [B, Hq, Sq], the backward's workspace, and its
    bound. The gradients, delta and their bounds are None when g is None."""
    __slots__ = ("o", "dq", "dk", "dv", "lse2", "b_o", "b_dq", "b_dk", "b_dv", "b_lse", "visible", "key_live", "delta",
                 "b_delta")


def ref64_bounds(q, k, v, g, scale, allowed, M=None, r=1.0, dtype=None, tiles=None):
    """fp64 attention of the 16-bit inputs under ``allowed`` (ref32's conventions: a row without a visible
    key has zero output, zero gradients and lse = +inf; dropout is M r on the probabilities of the PV
    product and dS = P (M r dP - delta)), and for every element of o, dq, dk, dv and lse2 a bound on the
    error of the kernels of csrc/attn_kernels.hip for ``dtype`` (default: q's): a first-order forward
    error analysis, in fp64 from this reference's own intermediates, of the roundings those kernels make
    (P and dS to 16 bit as MFMA operands, delta from the 16-bit O, the 16-bit stores, and the fp32
    operations in between). ``tiles``: the number of 64-key tiles a row's sweep can cross (default
    ceil(Skv / 64); the beam kernel's tile list is longer)."""
    dtype = dtype or q.dtype
    u = UNIT[dtype]
    # fp16 only: a value below 2^-14 is rounded to a multiple of 2^-24, an absolute error of up to 2^-25
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    B, Hq, Sq, Dh = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    nt = float(tiles if tiles is not None else -(-Skv // KEY_TILE))
    so = 1.0 + SECOND_ORDER * u
    qd, kd, vd = (t.detach().double() for t in (q, k, v))
    kx, vx = kd.repeat_interleave(G, 1), vd.repeat_interleave(G, 1)
    absQ, absK, absV = qd.abs(), kx.abs(), vx.abs()
    sl2 = float(scale) * LOG2E
    al = allowed.expand(B, Hq, Sq, Skv)
    ald = al.double()
    s2 = (qd @ kx.transpose(-1, -2)) * sl2                              # scores in log2 units
    A = (absQ @ absK.transpose(-1, -2)) * sl2                           # their sums of magnitudes
    vis = al.any(-1)
    s2m = s2.masked_fill(~al, float("-inf"))
    m = torch.where(vis, s2m.amax(-1), torch.zeros_like(s2m[..., 0]))
    e = torch.exp2(s2m - m[..., None])
    l = e.sum(-1)
    lse2 = torch.where(vis, m + torch.log2(l.clamp_min(1e-300)), torch.full_like(l, float("inf")))
    P = e / l.clamp_min(1e-300)[..., None]
    n = ald.sum(-1)                                                     # visible keys per row
    keep = ald if M is None else ald * M.expand(B, Hq, Sq, Skv).double()
    keepr = None if M is None else M.expand(B, Hq, Sq, Skv).double() * r
    PM = P if M is None else P * keepr
    o = PM @ vx                                                         # [B, Hq, Sq, D]

    # fp32: a score (Dh products; scale -> fp32, the log2(e) constant and their product are 3 roundings),
    # the exp2 argument (one fma rounding of s2 - m_run, |m_run| <= |m| + FWD_THR), one ulp of v_exp_f32
    e_s = (_acc(Dh) + 3 * F32) * A
    abs_s2 = s2.abs().masked_fill(~al, 0.0)
    eps_f = ((LN2 * (e_s + F32 * (abs_s2 + m.abs()[..., None] + FWD_THR)) + ULP32) * ald)
    l_rel = (P * eps_f).sum(-1) + (TILE_OPS * nt + 1) * F32            # relative error of the row sum
    lse_fin = torch.where(vis, lse2, torch.zeros_like(lse2))
    b_lse = so * (l_rel / LN2 + ULP32 * (torch.log2(n.clamp_min(1.0)) + FWD_THR) + F32 * lse_fin.abs())
    PV = PM @ absV
    b_o = so * (u * (o.abs() + PV) + (PM * eps_f) @ absV + (_acc(n)[..., None] + TILE_OPS * nt * F32) * PV
                + (l_rel[..., None] + 3 * F32) * o.abs()) + tiny * (1.0 + r * (keep @ absV))

    R = Ref64()
    R.o, R.b_o, R.lse2, R.b_lse, R.visible = o.transpose(1, 2), b_o.transpose(1, 2), lse2, b_lse * vis, vis
    grp = lambda t: t.reshape(B, Hkv, G, *t.shape[2:]).sum(2)
    cnt = grp(ald.sum(-2))                                              # query rows summed into key j, all G heads
    R.key_live = cnt > 0
    R.dq = R.dk = R.dv = R.b_dq = R.b_dk = R.b_dv = R.delta = R.b_delta = None
    if g is None:
        return R
    gd = g.detach().double().transpose(1, 2)                            # [B, Hq, Sq, D]
    absG = gd.abs()
    dP = gd @ vx.transpose(-1, -2)
    delta = (gd * o).sum(-1)
    # delta = rowsum(dO * O) from the kernel's 16-bit O. O is linear in the rounded probabilities, so their
    # relative errors reach delta through sum_j P_ij dP_ij, not through sum_d |dO_d| (P |V|)_d; the 16-bit
    # store of O costs u E_i with E_i = sum_d |dO_d| |o_d|; the rest are the fp32 terms of b_o and the sum itself
    E = (absG * o.abs()).sum(-1)
    b_delta = (so * (u * E + (PM * (u + eps_f) * dP.abs()).sum(-1) + (l_rel + 3 * F32) * E
                     + (_acc(n) + TILE_OPS * nt * F32) * (absG * PV).sum(-1))
               + tiny * (absG.sum(-1) + r * (keep * dP.abs()).sum(-1)) + (Dh + 1) * F32 * E)
    dPm = dP if M is None else dP * keepr
    dS = P * (dPm - delta[..., None])
    eps_b = (LN2 * (e_s + b_lse[..., None] + F32 * (abs_s2 + lse_fin.abs()[..., None])) + ULP32) * ald
    e_dp = (_acc(Dh) + F32) * (absG @ absV.transpose(-1, -2))
    if M is not None:
        e_dp = e_dp * keepr
    W = u * dS.abs() + tiny * ald + dS.abs() * (eps_b + 2 * F32) + P * (e_dp + b_delta[..., None])
    sc = float(scale)
    R.delta, R.b_delta = delta, b_delta
    R.dq = sc * (dS @ kx)
    R.b_dq = so * (u * R.dq.abs() + sc * (W @ absK) + (_acc(n)[..., None] + 2 * F32) * sc * (dS.abs() @ absK)) + tiny
    dSt, Wt, PMt = dS.transpose(-1, -2), W.transpose(-1, -2), PM.transpose(-1, -2)
    accj = _acc(cnt)[..., None] + 2 * F32
    R.dk = grp(sc * (dSt @ qd))
    R.b_dk = so * (u * R.dk.abs() + grp(sc * (Wt @ absQ)) + accj * grp(sc * (dSt.abs() @ absQ))) + tiny
    R.dv = grp(PMt @ gd)
    R.b_dv = (so * (u * R.dv.abs() + grp((PM * (u + eps_b)).transpose(-1, -2) @ absG) + accj * grp(PMt @ absG))
              + tiny * (1.0 + r * grp(keep.transpose(-1, -2) @ absG)))
    return R


def _where(idx, dims):
    """The position of a worst element in the kernels' units: head, row, and the row's 64-key tile,
    128-row q block, 32-row wave and 256-key dK/dV block."""
    at = dict(zip(dims, idx))
    out = [f"{c}={at[c]}" for c in dims]
    if "s" in at:
        s = at["s"]
        out.append(f"[row {s}: tile {s // 64}, q block {s // 128} wave {s % 128 // 32}, key block {s // 256}"
                   + (f", head {at['h']}" if "h" in at else "") + "]")
    return " ".join(out)


def assert_within_bounds(name, got, want, bound, dead=None, dims=None, dead_value=0.0):
    """Every element of ``got`` within ``bound`` of ``want``: no share of elements is excused, and NaN or
    Inf fails. ``dead`` (bool, broadcastable): the elements the mask makes dead, which must equal
    ``dead_value`` exactly (0, or +inf for lse). ``dims``: one letter per axis out of b, h, s, d, for the
    report of the worst element. Returns the worst err / bound."""
    got = got.detach().double()
    want, bound = want.to(got.device), bound.to(got.device)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    dims = dims or "bhsd"[:got.dim()]
    dead = torch.zeros_like(got, dtype=torch.bool) if dead is None else dead.to(got.device).expand_as(got)
    problems = []
    bad_dead = dead & ~(got == dead_value)
    if bad_dead.any():
        i = tuple(bad_dead.nonzero()[0].tolist())
        problems.append(f"{int(bad_dead.sum())} dead elements are not {dead_value}, first {got[i].item()} at {_where(i, dims)}")
    live = ~dead
    nonfinite = live & ~torch.isfinite(got)
    if nonfinite.any():
        i = tuple(nonfinite.nonzero()[0].tolist())
        problems.append(f"{int(nonfinite.sum())} non-finite elements, first {got[i].item()} at {_where(i, dims)}")
    err = torch.where(live & ~nonfinite, (got - want).abs(), torch.zeros_like(got))
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if worst > 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        problems.append(f"{int((ratio > 1.0).sum())} of {ratio.numel()} elements outside their bound; worst err/bound "
                        f"{worst:.3f}: got {got[i].item():.6g}, want {want[i].item():.6g}, bound {bound[i].item():.3g} "
                        f"at {_where(i, dims)}")
    assert not problems, f"{name}: " + "; ".join(problems)
    return worst


_BOUND = {"o": "b_o", "dq": "b_dq", "dk": "b_dk", "dv": "b_dv", "lse2": "b_lse"}
_DIMS = {"o": "bshd", "dq": "bhsd", "dk": "bhsd", "dv": "bhsd", "lse2": "bhs"}


def check_outputs(what, got, R):
    """assert_within_bounds on each output in ``got`` (a dict over o, dq, dk, dv, lse2, in the layouts of
    :class:`Ref64`), with the rows and keys the mask makes dead held to exact zeros (lse: +inf); prints and
    returns the worst err / bound of each."""
    dead_row = ~R.visible
    dead = {"o": dead_row.transpose(1, 2)[..., None], "dq": dead_row[..., None], "dk": ~R.key_live[..., None],
            "dv": ~R.key_live[..., None], "lse2": dead_row}
    worst = {}
    for name, t in got.items():
        worst[name] = assert_within_bounds(f"{what}: {name}", t, getattr(R, name), getattr(R, _BOUND[name]), dead=dead[name],
                                           dims=_DIMS[name], dead_value=float("inf") if name == "lse2" else 0.0)
    print(f"{what}: worst err/bound " + ", ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    return worst
