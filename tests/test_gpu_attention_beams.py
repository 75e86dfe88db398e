"""Beam-shared cache attention, smt_attn_fwd_beams / flash_attention_beams: one decode position of N
samples x nb beams against a prompt segment stored once per sample and generated buffers that are
never reordered, judged against an fp32 masked softmax on the per-row cache a DynamicCache would hold
(gathered here through the ancestry table). The bar is the project's own (tests/test_gpu_attention.py):
relative norm error of o <= max(8e-3, 1.5 x the error of torch's 16-bit sdpa on the same gathered
tensors), lse (log2 units) within 2e-3 abs. Rows without a visible key: o == 0, lse == +inf. N = 2
throughout; the shapes are the smallest that reach each branch (no prompt, one tile, a ragged tile,
several tiles per segment, several splits, empty splits, exactly 32 columns, two column blocks)."""
import pytest
import torch
import torch.nn.functional as F

from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
from sparse_matrix_tuning_amd.fused_llama import (KeyMask, flash_attention_beams, smt_flash_attention_forward,
                                                  smt_flash_mask)
from tests.attn_ref import D, DEV, ref32, rel as _rel

pytestmark = pytest.mark.gpu
N = 2


def _genealogy(nb, T, T_cap, seed):
    """uint8 [N * nb, T_cap] after T steps of a simulated beam search: every step is written at the row's
    own slot, and before each further step a random within-sample beam_idx is applied the way
    BeamSharedCache.reorder_cache applies it."""
    g = torch.Generator().manual_seed(seed)
    R = N * nb
    anc = (torch.arange(R) % nb).to(torch.uint8)[:, None].repeat(1, T_cap)
    base = torch.arange(R) // nb * nb
    for t in range(1, T):
        beam_idx = base + torch.randint(0, nb, (R,), generator=g)
        anc[:, :t] = anc[beam_idx][:, :t]
    return anc.to(DEV)


def _case(Hq, Hkv, nb, P, T, dtype=torch.bfloat16, P_cap=None, T_cap=None, seed=0):
    P_cap = max(P, 1) + 3 if P_cap is None else P_cap
    T_cap = T + 2 if T_cap is None else T_cap
    torch.manual_seed(100000 * nb + 1000 * P + 10 * T + Hq + seed)
    R = N * nb
    q = torch.randn(R, 1, Hq, D, device=DEV).to(dtype).transpose(1, 2)            # transformers' layout
    kp = torch.randn(N, Hkv, P_cap, D, device=DEV).to(dtype)
    vp = torch.randn(N, Hkv, P_cap, D, device=DEV).to(dtype)
    kg = torch.randn(R, Hkv, T_cap, D, device=DEV).to(dtype)
    vg = torch.randn(R, Hkv, T_cap, D, device=DEV).to(dtype)
    return q, kp, vp, kg, vg, _genealogy(nb, T, T_cap, seed + 7 * T + nb)


def _gather(kp, vp, kg, vg, anc, nb, P, T):
    """The per-row [N * nb, Hkv, P + T, D] K / V: the prompt of the row's sample, then step j from the slot
    anc[r, j] of that sample (a value >= nb is clamped here; such keys are masked out by _keep)."""
    R = kg.shape[0]
    first = torch.arange(R, device=DEV) // nb * nb
    src = first[:, None] + anc[:, :T].long().clamp(max=nb - 1)
    step = torch.arange(T, device=DEV)[None, :]
    out = []
    for prompt, gen in ((kp, kg), (vp, vg)):
        g = gen[src, :, step].permute(0, 2, 1, 3)
        out.append(torch.cat([prompt[:, :, :P].repeat_interleave(nb, 0), g], dim=2))
    return out


def _keep(anc, nb, P, T, prompt_keep=None):
    """bool [N * nb, P + T]: the keys row r sees."""
    R = anc.shape[0]
    pk = torch.ones(N, P, dtype=torch.bool, device=DEV) if prompt_keep is None else prompt_keep[:, :P]
    return torch.cat([pk.repeat_interleave(nb, 0), anc[:, :T] < nb], dim=1)


# torch's own 16-bit sdpa under the boolean mask (the bar of this file's header)
def _sdpa16(q, k, v, scale, allowed):
    G = q.shape[1] // k.shape[1]
    o = F.scaled_dot_product_attention(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), attn_mask=allowed,
                                       scale=scale)
    return o.transpose(1, 2)


def _judge(o, lse, q, kp, vp, kg, vg, anc, nb, P, T, prompt_keep=None, what=""):
    """o [R, 1, Hq, D] and lse [R, Hq] of a beam call against the fp32 reference on the gathered cache."""
    R, Hq = q.shape[0], q.shape[1]
    scale = D ** -0.5
    k, v = _gather(kp, vp, kg, vg, anc, nb, P, T)
    keep = _keep(anc, nb, P, T, prompt_keep)
    clean = lambda t: torch.where(keep[:, None, :, None], t, torch.zeros_like(t))
    k, v = clean(k), clean(v)
    allowed = keep[:, None, None, :]
    ro, _, _, _, rlse, visible = ref32(q, k, v, None, scale, allowed)               # [R, 1, Hq, D], [R, Hq, 1]
    vis_o = visible.transpose(1, 2)[..., None].expand(R, 1, Hq, D)
    assert o.shape == ro.shape and o.dtype == q.dtype, what
    assert torch.isfinite(o.float()).all(), what
    assert (o.float()[~vis_o] == 0).all(), what
    so = _sdpa16(q, k, v, scale, allowed).float().masked_fill(~vis_o, 0.0)
    e, es = _rel(o.float(), ro), _rel(so, ro)
    print(f"{what}: rel err {e:.3e} (sdpa {es:.3e})")
    assert e <= max(8e-3, 1.5 * es), (what, e, es)
    if lse is not None:
        assert lse.shape == (R, Hq) and lse.dtype == torch.float32, what
        vis, rl = visible[..., 0], rlse[..., 0]
        if vis.any():
            assert (lse[vis] - rl[vis]).abs().max().item() < 2e-3, what
        assert torch.isinf(lse[~vis]).all() and (lse[~vis] > 0).all(), what
    return e


def _run(c, nb, P, T, **kw):
    q, kp, vp, kg, vg, anc = c
    return flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, return_lse=True, **kw)


@pytest.mark.parametrize("Hq,Hkv,nb", [(4, 4, 1), (4, 4, 4), (8, 2, 4), (8, 1, 4), (8, 1, 5)])
@pytest.mark.parametrize("P,T", [(1, 1), (63, 2), (64, 64), (65, 65), (130, 130), (0, 3)])
def test_beams_against_the_gathered_cache(P, T, Hq, Hkv, nb):
    c = _case(Hq, Hkv, nb, P, T)
    o, lse = _run(c, nb, P, T)
    _judge(o, lse, *c, nb, P, T, what=f"P {P} T {T} Hq {Hq} Hkv {Hkv} nb {nb}")


def test_beams_fp16():
    c = _case(8, 2, 4, 130, 65, dtype=torch.float16)
    o, lse = _run(c, 4, 130, 65)
    _judge(o, lse, *c, 4, 130, 65, what="fp16")


@pytest.mark.parametrize("nb,P,T", [(4, 65, 65), (5, 130, 130)])
def test_forced_splits(nb, P, T):
    """1 and 3 splits and one more than the tile count (empty splits) each meet the bar, and a second
    run with the same split count is bit-identical."""
    c = _case(8, 1, nb, P, T)
    tiles = -(-P // 64) + nb * -(-T // 64)
    for ns in (1, 3, tiles + 3):
        o, lse = _run(c, nb, P, T, num_splits=ns)
        _judge(o, lse, *c, nb, P, T, what=f"nb {nb} P {P} T {T} splits {ns}")
        o2, lse2 = _run(c, nb, P, T, num_splits=ns)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), ns


@pytest.mark.parametrize("splits", [None, 1, 3])
def test_left_padded_prompt_with_a_hole(splits):
    nb, P, T = 4, 130, 5
    c = _case(8, 2, nb, P, T)
    q, kp, vp, kg, vg, anc = c
    keep = torch.ones(N, P, dtype=torch.bool, device=DEV)
    keep[1, :70] = False                                    # left padding: 0 keys in sample 0, 70 in sample 1
    keep[0, 40] = keep[1, 100] = False                      # holes inside the visible range
    # a NaN / Inf in a masked prompt row must not reach o
    kp[1, :, 3] = float("nan")
    vp[1, :, 5] = float("nan")
    vp[0, :, 40] = float("inf")
    o, lse = _run(c, nb, P, T, prompt_key_mask=KeyMask.from_padding_mask(keep), num_splits=splits)
    _judge(o, lse, *c, nb, P, T, prompt_keep=keep, what=f"left padding splits {splits}")
    # the mask as the transformers route hands it over: rows [::nb] of the expanded batch's words, a view
    full = KeyMask.from_padding_mask(torch.cat([keep.repeat_interleave(nb, 0),
                                                torch.ones(N * nb, T, dtype=torch.bool, device=DEV)], 1))
    view = KeyMask(full.bits[::nb, :-(-P // 64)], P)
    o2, lse2 = _run(c, nb, P, T, prompt_key_mask=view, num_splits=splits)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("splits", [1, 3])
def test_rows_with_one_and_with_no_visible_key(splits):
    """Sample 1's prompt is fully masked and T = 1: its rows see their own key only (finite). Row 2's
    ancestry holds a value >= nb, which matches no slot: o == 0 and lse == +inf there."""
    nb, P, T = 4, 70, 1
    c = _case(4, 2, nb, P, T)
    q, kp, vp, kg, vg, anc = c
    keep = torch.ones(N, P, dtype=torch.bool, device=DEV)
    keep[1] = False
    dead = nb + 2                                           # row 6 of 8: sample 1, beam 2
    anc[dead, 0] = nb
    anc[1, 0] = 255                                         # sample 0: the prompt is still visible
    o, lse = _run(c, nb, P, T, prompt_key_mask=KeyMask.from_padding_mask(keep), num_splits=splits)
    assert (o[dead].float() == 0).all() and torch.isinf(lse[dead]).all() and (lse[dead] > 0).all()
    others = [r for r in range(N * nb) if r != dead]
    assert torch.isfinite(lse[others]).all()
    _judge(o, lse, *c, nb, P, T, prompt_keep=keep, what=f"one / no visible key splits {splits}")


@pytest.mark.parametrize("Hq,Hkv,nb", [(8, 2, 4), (8, 1, 5)])
@pytest.mark.parametrize("splits", [None, 1, 3])
def test_garbage_is_never_read(splits, Hq, Hkv, nb):
    """Prompt rows >= P, generated rows >= T and every generated entry no row's ancestry points to hold
    NaN: bit for bit the result of the same call with zeros there."""
    P, T = 70, 67
    c = _case(Hq, Hkv, nb, P, T, P_cap=130, T_cap=140)
    q, kp, vp, kg, vg, anc = c
    used = torch.zeros(N * nb, 140, dtype=torch.bool, device=DEV)                # [slot row, step]
    first = torch.arange(N * nb, device=DEV) // nb * nb
    src = first[:, None] + anc[:, :T].long()
    used[src, torch.arange(T, device=DEV)[None, :].expand_as(src)] = True
    assert (~used[:, :T]).any()                                                   # dead hypotheses exist
    outs = []
    for fill in (float("nan"), 0.0):
        kp2, vp2, kg2, vg2 = (t.clone() for t in (kp, vp, kg, vg))
        kp2[:, :, P:] = fill
        vp2[:, :, P:] = fill
        for g in (kg2, vg2):
            g.masked_fill_(~used[:, None, :, None], fill)
        outs.append(flash_attention_beams(q, kp2, vp2, kg2, vg2, anc, nb, P, T, num_splits=splits, return_lse=True))
    (o, lse), (o0, lse0) = outs
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    _judge(o, lse, *c, nb, P, T, what=f"garbage nb {nb} splits {splits}")


def test_strides():
    Hq, Hkv, nb, P, T = 8, 2, 4, 100, 70
    R = N * nb
    torch.manual_seed(5)
    # generated buffers: the [:, :, :96] slice of larger allocations; the prompt: a [N, S, H, D]-ordered store
    kgb = torch.randn(R, Hkv, 256, D, device=DEV).bfloat16()
    vgb = torch.randn(R, Hkv, 256, D, device=DEV).bfloat16()
    kg, vg = kgb[:, :, :96], vgb[:, :, :96]
    kp = torch.randn(N, 128, Hkv, D, device=DEV).bfloat16().transpose(1, 2)
    vp = torch.randn(N, 128, Hkv, D, device=DEV).bfloat16().transpose(1, 2)
    # q: a slice of a joint q|k|v projection output; the ancestry: a slice of a wider table
    joint = torch.randn(R, 1, (Hq + 2 * Hkv) * D, device=DEV).bfloat16()
    q = joint[:, :, :Hq * D].view(R, 1, Hq, D).transpose(1, 2)
    anc = torch.full((R, 200), 9, dtype=torch.uint8, device=DEV)
    anc[:, :96] = _genealogy(nb, T, 96, 3)
    anc = anc[:, :96]
    assert not kg.is_contiguous() and not kp.is_contiguous() and not q.is_contiguous() and not anc.is_contiguous()
    o, lse = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, return_lse=True)
    _judge(o, lse, q, kp, vp, kg, vg, anc, nb, P, T, what="strided buffers")
    o2, lse2 = flash_attention_beams(q.contiguous(), kp.contiguous(), vp.contiguous(), kg.contiguous(), vg.contiguous(),
                                     anc.contiguous(), nb, P, T, return_lse=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


class _Cfg:
    num_hidden_layers = 1


def test_transformers_interface_dispatch():
    """smt_flash_attention_forward sends the K / V that a BeamSharedCache's decode update returns to the
    beam kernel: the result of flash_attention_beams on the cache's buffers, bit for bit."""
    Hq, Hkv, nb, P = 8, 2, 4, 37
    R = N * nb
    torch.manual_seed(11)
    cache = BeamSharedCache(_Cfg(), nb, 8)
    k0 = torch.randn(N, Hkv, P, D, device=DEV).bfloat16().repeat_interleave(nb, 0)
    v0 = torch.randn(N, Hkv, P, D, device=DEV).bfloat16().repeat_interleave(nb, 0)
    cache.update(k0, v0, 0)
    am = torch.ones(R, P, dtype=torch.int64, device=DEV)
    am[nb:, :9] = 0                                         # sample 1 is left-padded
    base = torch.arange(R, device=DEV) // nb * nb
    for t in range(3):
        cache.reorder_cache(base + torch.randint(0, nb, (R,), device=DEV))
        k1 = torch.randn(R, Hkv, 1, D, device=DEV).bfloat16()
        v1 = torch.randn(R, Hkv, 1, D, device=DEV).bfloat16()
        q = torch.randn(R, 1, Hq, D, device=DEV).bfloat16().transpose(1, 2)
        am = torch.cat([am, am.new_ones(R, 1)], 1)
        cm = smt_flash_mask(R, 1, P + t + 1, q_offset=cache.get_seq_length(), attention_mask=am)
        k, v = cache.update(k1, v1, 0)
        o, _ = smt_flash_attention_forward(None, q, k, v, cm)
        ly = cache.layers[0]
        keep = am[::nb, :P].bool()
        ref = flash_attention_beams(q, ly.k_prompt, ly.v_prompt, ly.k_gen, ly.v_gen, cache.ancestors, nb, P, t + 1,
                                    prompt_key_mask=KeyMask.from_padding_mask(keep))
        assert torch.equal(o, ref), t
        _judge(o, None, q, ly.k_prompt, ly.v_prompt, ly.k_gen, ly.v_gen, cache.ancestors, nb, P, t + 1, prompt_keep=keep,
               what=f"interface step {t}")
    with pytest.raises(NotImplementedError):
        smt_flash_attention_forward(None, q, k, v, cm, dropout=0.1)


def test_decode_step_does_not_synchronise():
    """reorder_cache, the decode update, smt_flash_mask and smt_flash_attention_forward of one step on a
    BeamSharedCache under torch's sync debug mode, where the build supports it."""
    Hq, Hkv, nb, P = 8, 2, 4, 37
    R = N * nb
    torch.manual_seed(12)
    cache = BeamSharedCache(_Cfg(), nb, 4)
    k0 = torch.randn(N, Hkv, P, D, device=DEV).bfloat16().repeat_interleave(nb, 0)
    cache.update(k0, k0.clone(), 0)
    k1 = torch.randn(R, Hkv, 1, D, device=DEV).bfloat16()
    q = torch.randn(R, 1, Hq, D, device=DEV).bfloat16().transpose(1, 2)
    cache.update(k1, k1.clone(), 0)                                    # step 0, so that the reorder below has work
    beam_idx = torch.arange(R, device=DEV) // nb * nb + torch.randint(0, nb, (R,), device=DEV)
    am = torch.ones(R, P + 2, dtype=torch.int64, device=DEV)
    am[nb:, :9] = 0
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        guarded = True
    except Exception:
        guarded = False
    try:
        cache.reorder_cache(beam_idx)
        cm = smt_flash_mask(R, 1, P + 2, q_offset=cache.get_seq_length(), attention_mask=am)
        k, v = cache.update(k1, k1.clone(), 0)
        o, _ = smt_flash_attention_forward(None, q, k, v, cm)
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode:", "on" if guarded else "not available")
    ly = cache.layers[0]
    _judge(o, None, q, ly.k_prompt, ly.v_prompt, ly.k_gen, ly.v_gen, cache.ancestors, nb, P, 2, prompt_keep=am[::nb, :P].bool(),
           what="no-sync step")


def test_rejections():
    nb, P, T = 2, 20, 3
    c = _case(4, 2, nb, P, T)
    q, kp, vp, kg, vg, anc = c
    with pytest.raises(NotImplementedError):
        flash_attention_beams(q.detach().requires_grad_(True), kp, vp, kg, vg, anc, nb, P, T)
    with pytest.raises(NotImplementedError):
        flash_attention_beams(q, kp, vp, kg.detach().requires_grad_(True), vg, anc, nb, P, T)
    with torch.no_grad():
        flash_attention_beams(q.detach().requires_grad_(True), kp, vp, kg, vg, anc, nb, P, T)    # no gradient asked: fine
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, 0)                  # the current token's key is in the cache
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, kg.shape[2] + 1)
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc, nb, kp.shape[2] + 1, T)
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc.long(), nb, P, T)           # uint8 only
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc[:, :T - 1], nb, P, T)
    with pytest.raises(ValueError):
        flash_attention_beams(q, kp, vp, kg, vg, anc, 3, P, T)                   # 4 rows, 3 beams
