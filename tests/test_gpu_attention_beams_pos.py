"""The beam kernel with the number of generated positions on the device, smt_attn_fwd_beams_pos
(flash_attention_beams with a tensor gen_len), and smt_attn_kv_append_pos (kv_append).

The contract is bit identity: for a given num_splits the device-counter call equals
flash_attention_beams with the integer T = clamp(counter, 1, T_cap) on the same tensors, o and lse,
torch.equal. The integer call is held to the fp32 reference by tests/test_gpu_attention_beams.py; one
call per column configuration is judged against that reference here as well (same bar: relative norm
error of o <= max(8e-3, 1.5 x torch's 16-bit sdpa), lse within 2e-3), which guards this file's wiring.
N = 2 and head_dim 128 throughout; the shapes are the smallest that reach each branch: no prompt, a
ragged and a full prompt tile, one / two / three generated tiles per slot, T on both sides of a tile
edge, one and several splits, more splits than tiles (empty splits), two column blocks."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
from sparse_matrix_tuning_amd.fused_llama import (KeyMask, flash_attention_beams, kv_append, smt_flash_attention_forward,
                                                  smt_flash_mask)
from tests.attn_ref import D, DEV
from tests.test_gpu_attention_beams import N, _case, _judge

pytestmark = pytest.mark.gpu
CONFIGS = [(4, 4, 1), (8, 2, 4), (8, 1, 5)]              # (Hq, Hkv, nb); the last is two column blocks


def _cnt(value):
    return torch.tensor([value], dtype=torch.int32, device=DEV)


def _prompt_keep(P):
    """A left-padded prompt mask with a hole for the ragged prompts, None (no mask) for the others."""
    if P not in (13, 70):
        return None
    keep = torch.ones(N, P, dtype=torch.bool, device=DEV)
    keep[1, :5] = False
    keep[0, 7] = keep[1, 9] = False
    return keep


def _both(c, nb, P, T, counter, splits, keep=None):
    """(the device-counter call's (o, lse), the integer call's) for one split count."""
    q, kp, vp, kg, vg, anc = c
    pm = KeyMask.from_padding_mask(keep) if keep is not None else None
    dev = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, _cnt(counter), prompt_key_mask=pm, num_splits=splits,
                                return_lse=True)
    ref = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, prompt_key_mask=pm, num_splits=splits, return_lse=True)
    return dev, ref


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), what
    assert torch.equal(a[1], b[1]), what


def _default_splits(Hq, Hkv, nb, P, T_cap, dtype=torch.bfloat16):
    shape = _hip.AttnShape(N, Hq, Hkv, P + T_cap, D ** -0.5, _hip.dtype_code16(dtype, "test"))
    return _hip.load().smt_attn_beams_splits(ctypes.byref(shape), nb, P, T_cap)


@pytest.mark.parametrize("T_cap", [65, 130])
@pytest.mark.parametrize("Hq,Hkv,nb", CONFIGS)
def test_bit_identity_with_the_integer_call(Hq, Hkv, nb, T_cap):
    for P in (0, 13, 64, 70):
        c = _case(Hq, Hkv, nb, P, T_cap, T_cap=T_cap)
        keep = _prompt_keep(P)
        tiles_cap = -(-P // 64) + nb * -(-T_cap // 64)
        for T in sorted({1, 63, 64, 65, T_cap}):
            for ns in (1, 3, tiles_cap + 3):
                dev, ref = _both(c, nb, P, T, T, ns, keep)
                _same(dev, ref, (P, T, ns))
            # the default split count is the capacity's
            q, kp, vp, kg, vg, anc = c
            pm = KeyMask.from_padding_mask(keep) if keep is not None else None
            dev = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, _cnt(T), prompt_key_mask=pm, return_lse=True)
            ref = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, prompt_key_mask=pm, return_lse=True,
                                        num_splits=_default_splits(Hq, Hkv, nb, P, T_cap))
            _same(dev, ref, (P, T, "default"))


def test_bit_identity_fp16():
    nb, P, T_cap = 4, 70, 130
    c = _case(8, 2, nb, P, T_cap, dtype=torch.float16, T_cap=T_cap)
    for T in (1, 65, T_cap):
        for ns in (1, 3):
            dev, ref = _both(c, nb, P, T, T, ns, _prompt_keep(P))
            _same(dev, ref, (T, ns))
            assert dev[0].dtype == torch.float16


@pytest.mark.parametrize("Hq,Hkv,nb", CONFIGS)
def test_the_counter_saturates(Hq, Hkv, nb):
    P, T_cap = 70, 65
    c = _case(Hq, Hkv, nb, P, T_cap, T_cap=T_cap)
    for counter, T in ((0, 1), (-7, 1), (T_cap + 9, T_cap)):
        for ns in (1, 3):
            dev, ref = _both(c, nb, P, T, counter, ns, _prompt_keep(P))
            _same(dev, ref, (counter, ns))
            assert torch.isfinite(dev[0].float()).all()


@pytest.mark.parametrize("Hq,Hkv,nb", CONFIGS)
@pytest.mark.parametrize("T", [1, 64, 67])
def test_nothing_past_the_counter_is_read(T, Hq, Hkv, nb):
    """Rows >= T of the generated buffers hold NaN and the ancestry bytes at j >= T hold 255: bit for bit
    the clean run's result."""
    P, T_cap = 13, 130
    q, kp, vp, kg, vg, anc = _case(Hq, Hkv, nb, P, T_cap, T_cap=T_cap)
    kg2, vg2, anc2 = kg.clone(), vg.clone(), anc.clone()
    kg2[:, :, T:] = float("nan")
    vg2[:, :, T:] = float("nan")
    anc2[:, T:] = 255
    for ns in (None, 1, 3):
        clean = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, _cnt(T), num_splits=ns, return_lse=True)
        dirty = flash_attention_beams(q, kp, vp, kg2, vg2, anc2, nb, P, _cnt(T), num_splits=ns, return_lse=True)
        assert torch.isfinite(dirty[0].float()).all() and torch.isfinite(dirty[1]).all()
        _same(dirty, clean, (T, ns))


SENTINEL = 0x7A5C                                          # a bit pattern no randn value rounds to


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("counter,row", [(1, 0), (64, 63), (65, 64), (130, 129), (0, 0), (133, 129)])
def test_append_writes_exactly_one_row(counter, row, dtype):
    R, Hkv, T_cap = 6, 2, 130
    torch.manual_seed(counter + 1000)
    kg = torch.empty(R, Hkv, T_cap, D, dtype=dtype, device=DEV)
    vg = torch.empty_like(kg)
    _bits(kg).fill_(SENTINEL)
    _bits(vg).fill_(SENTINEL + 1)
    # the model's layout: [R, 1, Hkv, D] transposed, here a slice of a wider projection output; v as a
    # plain contiguous [R, Hkv, 1, D]
    joint = torch.randn(R, 1, (Hkv + 1) * D, device=DEV).to(dtype)
    kn = joint[:, :, :Hkv * D].view(R, 1, Hkv, D).transpose(1, 2)
    vn = torch.randn(R, Hkv, 1, D, device=DEV).to(dtype)
    assert kn.shape == (R, Hkv, 1, D) and not kn.is_contiguous()
    kv_append(kn, vn, kg, vg, _cnt(counter))
    for gen, new, fill in ((kg, kn, SENTINEL), (vg, vn, SENTINEL + 1)):
        assert torch.equal(_bits(gen[:, :, row]), _bits(new[:, :, 0].contiguous()))
        rest = torch.ones(T_cap, dtype=torch.bool, device=DEV)
        rest[row] = False
        assert (_bits(gen)[:, :, rest] == fill).all()


def test_append_rejections():
    kg = torch.zeros(4, 2, 8, D, dtype=torch.bfloat16, device=DEV)
    kn = torch.zeros(4, 2, 1, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        kv_append(kn, kn, kg, kg.clone(), torch.zeros(1, dtype=torch.int64, device=DEV))     # int32 only
    with pytest.raises(ValueError):
        kv_append(kn[:3], kn[:3], kg, kg.clone(), _cnt(1))
    with pytest.raises(ValueError):
        flash_attention_beams(kn.transpose(1, 2).reshape(4, 2, 1, D), kg[:1, :, :1], kg[:1, :, :1], kg, kg,
                              torch.zeros(4, 7, dtype=torch.uint8, device=DEV), 4, 0, _cnt(1))  # ancestors < T_cap


def test_graph_replay_follows_the_device_tensors():
    """Append + attention captured once (3 splits, a prompt mask), replayed at T = 1..5 after the
    counter, the new K / V, q and the ancestry table changed in place: each replay equals the eager
    integer-T call on the same buffers bit for bit."""
    Hq, Hkv, nb, P, T_cap, ns = 8, 2, 4, 70, 8, 3
    R = N * nb
    q, kp, vp, kg, vg, anc = _case(Hq, Hkv, nb, P, 1, T_cap=T_cap)
    q = q.contiguous()
    pm = KeyMask.from_padding_mask(_prompt_keep(P))
    kn = torch.randn(R, 1, Hkv, D, device=DEV).bfloat16().transpose(1, 2)
    vn = torch.randn(R, 1, Hkv, D, device=DEV).bfloat16().transpose(1, 2)
    cnt = _cnt(1)
    kg0, vg0 = kg.clone(), vg.clone()
    kv_append(kn, vn, kg, vg, cnt)                                                        # warm-up
    flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, cnt, prompt_key_mask=pm, num_splits=ns, return_lse=True)
    kg.copy_(kg0)
    vg.copy_(vg0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                             # one stream, a linear chain
        kv_append(kn, vn, kg, vg, cnt)
        o, lse = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, cnt, prompt_key_mask=pm, num_splits=ns,
                                       return_lse=True)
    gen = torch.Generator(device=DEV).manual_seed(13)
    base = torch.arange(R, device=DEV) // nb * nb
    for T in range(1, 6):
        cnt.fill_(T)
        for t in (q, kn, vn):
            t.copy_(torch.randn(t.shape, device=DEV, generator=gen).bfloat16())
        if T > 1:                                                                         # reorder_cache's update
            beam_idx = base + torch.randint(0, nb, (R,), device=DEV, generator=gen)
            anc[:, :T - 1] = anc.index_select(0, beam_idx)[:, :T - 1]
        g.replay()
        assert torch.equal(kg[:, :, T - 1], kn[:, :, 0]) and torch.equal(vg[:, :, T - 1], vn[:, :, 0])
        ref = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, prompt_key_mask=pm, num_splits=ns, return_lse=True)
        _same((o, lse), ref, ("replay", T))
        assert torch.isfinite(lse).all()
    _judge(o, lse, q, kp, vp, kg, vg, anc, nb, P, 5, prompt_keep=_prompt_keep(P), what="last replay")


class _Cfg:
    num_hidden_layers = 1


def test_device_steps_decode_step_does_not_synchronise():
    """reorder_cache, smt_flash_mask, the device_steps update and smt_flash_attention_forward of two
    decode steps (the first builds the prompt mask words) under torch's sync debug mode, where the
    build supports it; each equals the integer call on the cache's buffers bit for bit."""
    Hq, Hkv, nb, P = 8, 2, 4, 37
    R = N * nb
    torch.manual_seed(12)
    cache = BeamSharedCache(_Cfg(), nb, 4, device_steps=True)
    k0 = torch.randn(N, Hkv, P, D, device=DEV).bfloat16().repeat_interleave(nb, 0)
    cache.update(k0, k0.clone(), 0)
    ks = [torch.randn(R, 1, Hkv, D, device=DEV).bfloat16().transpose(1, 2) for _ in range(2)]
    qs = [torch.randn(R, 1, Hkv * 4, D, device=DEV).bfloat16().transpose(1, 2) for _ in range(2)]
    beam_idx = torch.arange(R, device=DEV) // nb * nb + torch.randint(0, nb, (R,), device=DEV)
    ams = [torch.ones(R, P + 1 + t, dtype=torch.int64, device=DEV) for t in range(2)]
    for am in ams:
        am[nb:, :9] = 0
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        guarded = True
    except Exception:
        guarded = False
    outs = []
    try:
        for t in range(2):
            cache.reorder_cache(beam_idx)
            cm = smt_flash_mask(R, 1, P + t + 1, q_offset=cache.get_seq_length(), attention_mask=ams[t])
            k, v = cache.update(ks[t], ks[t].clone(), 0)
            outs.append(smt_flash_attention_forward(None, qs[t], k, v, cm)[0].clone())
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode:", "on" if guarded else "not available")
    ly = cache.layers[0]
    assert k.shape == ly.k_gen.shape and int(cache.steps_tensor) == 2 == ly.steps
    keep = ams[0][::nb, :P].bool()
    ref = flash_attention_beams(qs[1], ly.k_prompt, ly.v_prompt, ly.k_gen, ly.v_gen, cache.ancestors, nb, P, 2,
                                prompt_key_mask=KeyMask.from_padding_mask(keep),
                                num_splits=_default_splits(Hq, Hkv, nb, P, 4))
    assert torch.equal(outs[1], ref)
    _judge(outs[1], None, qs[1], ly.k_prompt, ly.v_prompt, ly.k_gen, ly.v_gen, cache.ancestors, nb, P, 2, prompt_keep=keep,
           what="no-sync device-steps step")


@pytest.mark.parametrize("Hq,Hkv,nb", CONFIGS)
def test_quality_bar_against_the_gathered_cache(Hq, Hkv, nb):
    P, T, T_cap = 70, 67, 130
    c = _case(Hq, Hkv, nb, P, T, T_cap=T_cap)
    q, kp, vp, kg, vg, anc = c
    keep = _prompt_keep(P)
    o, lse = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, _cnt(T), prompt_key_mask=KeyMask.from_padding_mask(keep),
                                   return_lse=True)
    _judge(o, lse, *c, nb, P, T, prompt_keep=keep, what=f"device counter Hq {Hq} Hkv {Hkv} nb {nb}")
