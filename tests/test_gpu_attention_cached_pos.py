"""Cached attention with the position on the device (smt_attn_fwd_cached_pos, flash_attention_cached with
a tensor q_offset) against the host-offset call of the same library on the same tensors: for a given
split count the two are bit-identical (the kernel derives the causal edge, the descriptor ends and the
tile partition from the position it reads, exactly as the host does from q_offset). One leg is judged
independently, against an fp32 masked softmax with the project's bar (tests/test_gpu_attention_cached.py:
relative norm error of o <= max(8e-3, 1.5 x torch's 16-bit sdpa), lse within 2e-3 abs). The graph
replays and the sync-debug leg are the ones that show the host reads nothing. B = 2 or 3, head_dim 128."""
import pytest
import torch
import torch.nn.functional as F

from sparse_matrix_tuning_amd.fused_llama import (CacheMask, KeyMask, flash_attention_cached, smt_flash_attention_forward,
                                                  smt_flash_mask)
from tests.attn_ref import D, DEV, allowed_cached, ref32, rel as _rel

pytestmark = pytest.mark.gpu
ENDS = (1, 63, 64, 65, 128, 129)                          # p + Sq: one tile, the ragged tile, the tile boundary
SPLITS = (1, 2, 3, 7)                                     # 7 splits over 1-3 tiles: empty splits; 1: direct store


def _buffers(B, Hq, Hkv, Sq, cap, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(1000 * cap + 10 * Hq + Sq + seed)
    q = torch.randn(B, Sq, Hq, D, device=DEV).to(dtype).transpose(1, 2)
    k = torch.randn(B, Hkv, cap, D, device=DEV).to(dtype)
    v = torch.randn(B, Hkv, cap, D, device=DEV).to(dtype)
    return q, k, v


def _pos(p, dtype=torch.int64, shape=()):
    return torch.full(shape, p, dtype=dtype, device=DEV)


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), ("o", what)
    assert torch.equal(a[1], b[1]), ("lse", what)


@pytest.mark.parametrize("cap", [129, 200])
@pytest.mark.parametrize("Sq", [1, 5, 9])
def test_bit_identical_to_the_host_offset_call(cap, Sq):
    q, k, v = _buffers(2, 8, 2, Sq, cap)
    for end in ENDS:
        p = end - Sq
        if p < 0:
            continue
        for n in SPLITS:
            ref = flash_attention_cached(q, k, v, q_offset=p, num_splits=n, return_lse=True)
            got = flash_attention_cached(q, k, v, q_offset=_pos(p), num_splits=n, return_lse=True)
            _same(got, ref, (cap, Sq, p, n))
    # the default split count follows the capacity in both calls
    _same(flash_attention_cached(q, k, v, q_offset=_pos(64 - Sq), return_lse=True),
          flash_attention_cached(q, k, v, q_offset=64 - Sq, return_lse=True), "default splits")


def test_bit_identical_fp16_and_int32_positions():
    q, k, v = _buffers(2, 8, 2, 5, 200, dtype=torch.float16)
    for end in ENDS[1:]:
        for n in (1, 3):
            ref = flash_attention_cached(q, k, v, q_offset=end - 5, num_splits=n, return_lse=True)
            _same(flash_attention_cached(q, k, v, q_offset=_pos(end - 5), num_splits=n, return_lse=True), ref, ("fp16", end, n))
    q, k, v = _buffers(2, 8, 2, 1, 129)
    for end in ENDS:
        for n in SPLITS:
            ref = flash_attention_cached(q, k, v, q_offset=end - 1, num_splits=n, return_lse=True)
            for shape in ((), (1,), (2,)):
                got = flash_attention_cached(q, k, v, q_offset=_pos(end - 1, torch.int32, shape), num_splits=n, return_lse=True)
                _same(got, ref, ("int32", shape, end, n))
    _same(flash_attention_cached(q, k, v, q_offset=_pos(77, shape=(1,)), num_splits=2, return_lse=True),
          flash_attention_cached(q, k, v, q_offset=77, num_splits=2, return_lse=True), "int64 [1]")


@pytest.mark.parametrize("Sq", [1, 5])
def test_one_position_per_batch_row(Sq):
    """Rows at 0, 64 and 130 in one call: each has its own partition (row 0 one tile, so two of three
    splits are empty there and none in row 2) and equals its own host-offset call."""
    B, cap, rows = 3, 200, (0, 64, 130)
    q, k, v = _buffers(B, 8, 2, Sq, cap)
    pos = torch.tensor(rows, dtype=torch.int64, device=DEV)
    for n in (1, 3, 7):
        o, lse = flash_attention_cached(q, k, v, q_offset=pos, num_splits=n, return_lse=True)
        for b, p in enumerate(rows):
            ro, rlse = flash_attention_cached(q[b:b + 1], k[b:b + 1], v[b:b + 1], q_offset=p, num_splits=n, return_lse=True)
            assert torch.equal(o[b:b + 1], ro) and torch.equal(lse[b:b + 1], rlse), (Sq, n, b, p)
    # a strided [B] tensor and an int32 one
    wide = torch.zeros(B, 2, dtype=torch.int64, device=DEV)
    wide[:, 0] = pos
    ref = flash_attention_cached(q, k, v, q_offset=pos, num_splits=3, return_lse=True)
    _same(flash_attention_cached(q, k, v, q_offset=wide[:, 0], num_splits=3, return_lse=True), ref, "strided positions")
    _same(flash_attention_cached(q, k, v, q_offset=pos.int(), num_splits=3, return_lse=True), ref, "int32 [B]")


@pytest.mark.parametrize("splits", [1, 3])
def test_key_mask_against_the_fp32_softmax(splits):
    """Independent of the host-offset call. Capacity 200, rows at 129 and 150, Sq 2: row 0 has a hole,
    row 1 left padding that covers every key its queries can see (o == 0, lse == +inf there)."""
    B, Hq, Hkv, Sq, cap = 2, 8, 2, 2, 200
    rows = (129, 150)
    q, k, v = _buffers(B, Hq, Hkv, Sq, cap)
    keep = torch.ones(B, cap, dtype=torch.bool, device=DEV)
    keep[0, :70] = False
    keep[0, 100] = False
    keep[1, :160] = False
    k, v = k.clone(), v.clone()
    k[0, :, 3] = float("nan")                               # masked rows may hold anything
    v[0, :, 100] = float("inf")
    pos = torch.tensor(rows, dtype=torch.int64, device=DEV)
    o, lse = flash_attention_cached(q, k, v, key_mask=KeyMask.from_padding_mask(keep), q_offset=pos, num_splits=splits,
                                    return_lse=True)
    G, scale = Hq // Hkv, D ** -0.5
    allowed = allowed_cached(B, Sq, cap, pos, keep)                                         # [B, 1, Sq, cap]
    clean = lambda t: torch.where(keep[:, None, :, None], t, torch.zeros_like(t))
    kc, vc = clean(k), clean(v)
    ro, _, _, _, rlse, visible = ref32(q, kc, vc, None, scale, allowed)
    vis_o = visible.transpose(1, 2)[..., None].expand(B, Sq, Hq, D)
    # torch's own 16-bit sdpa under the same mask: the bar, so written here and not in tests/attn_ref.py
    so = F.scaled_dot_product_attention(q, kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1),
                                        attn_mask=allowed, scale=scale).transpose(1, 2).float()
    so = so.masked_fill(~vis_o, 0.0)
    assert torch.isfinite(o.float()).all()
    assert (o[1].float() == 0).all() and torch.isinf(lse[1]).all() and (lse[1] > 0).all()
    assert torch.isfinite(lse[0]).all()
    e, es = _rel(o.float(), ro), _rel(so, ro)
    print(f"splits {splits}: rel err {e:.3e} (sdpa {es:.3e}), lse err {(lse[0] - rlse[0]).abs().max().item():.3e}")
    assert e <= max(8e-3, 1.5 * es), (e, es)
    assert (lse[0] - rlse[0]).abs().max().item() < 2e-3


@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_garbage_tail_is_never_read(fill):
    cap, Sq, p = 200, 2, 68
    q, k, v = _buffers(2, 8, 2, Sq, cap)
    for n in (1, 2, 4):
        ref = flash_attention_cached(q, k, v, q_offset=_pos(p), num_splits=n, return_lse=True)
        kg, vg = k.clone(), v.clone()
        kg[:, :, p + Sq:] = fill
        vg[:, :, p + Sq:] = fill
        got = flash_attention_cached(q, kg, vg, q_offset=_pos(p), num_splits=n, return_lse=True)
        _same(got, ref, (fill, n))
        assert torch.isfinite(got[0].float()).all() and torch.isfinite(got[1]).all()


def test_strided_caches():
    B, Hq, Hkv, cap = 2, 8, 2, 136
    torch.manual_seed(5)
    kb = torch.randn(B, Hkv, 256, D, device=DEV).bfloat16()
    vb = torch.randn(B, Hkv, 256, D, device=DEV).bfloat16()
    q = torch.randn(B, 1, Hq, D, device=DEV).bfloat16().transpose(1, 2)
    k, v = kb[:, :, :cap], vb[:, :, :cap]                                 # a slice of a larger buffer
    k2 = k.transpose(1, 2).contiguous().transpose(1, 2)                    # a [B, S, H, D]-ordered cache
    v2 = v.transpose(1, 2).contiguous().transpose(1, 2)
    assert not k.is_contiguous() and k2.stride(2) == Hkv * D
    for p in (0, 99, 135):
        for n in (1, 3):
            ref = flash_attention_cached(q, k.contiguous(), v.contiguous(), q_offset=p, num_splits=n, return_lse=True)
            _same(flash_attention_cached(q, k, v, q_offset=_pos(p), num_splits=n, return_lse=True), ref, ("slice", p, n))
            _same(flash_attention_cached(q, k2, v2, q_offset=_pos(p), num_splits=n, return_lse=True), ref, ("bshd", p, n))


def test_out_of_contract_positions_saturate():
    """The defined clamp into [0, Skv - Sq]. K / V are the leading slots of larger allocations."""
    B, cap, Sq = 2, 136, 3
    q, kb, vb = _buffers(B, 8, 2, Sq, 256)
    k, v = kb[:, :, :cap], vb[:, :, :cap]
    for n in (1, 3):
        top = flash_attention_cached(q, k, v, q_offset=cap - Sq, num_splits=n, return_lse=True)
        low = flash_attention_cached(q, k, v, q_offset=0, num_splits=n, return_lse=True)
        for p in (cap - Sq + 1, cap, 10 ** 6, 2 ** 31 + 5, 2 ** 62):
            _same(flash_attention_cached(q, k, v, q_offset=_pos(p), num_splits=n, return_lse=True), top, (p, n))
        for p in (-1, -2 ** 40):
            _same(flash_attention_cached(q, k, v, q_offset=_pos(p), num_splits=n, return_lse=True), low, (p, n))
        mixed = torch.tensor([-7, cap + 9], dtype=torch.int64, device=DEV)
        o, lse = flash_attention_cached(q, k, v, q_offset=mixed, num_splits=n, return_lse=True)
        assert torch.equal(o[0], low[0][0]) and torch.equal(o[1], top[0][1])
        assert torch.equal(lse[0], low[1][0]) and torch.equal(lse[1], top[1][1])


def test_graph_replay_follows_the_device_tensors():
    """One captured call (Sq 1, 4 splits, key mask), replayed after the position, q and the mask bits
    changed in place: each replay equals the eager call on the same values bit for bit."""
    B, Hq, Hkv, cap, n = 2, 8, 2, 200, 4
    q, k, v = _buffers(B, Hq, Hkv, 1, cap)
    q = q.contiguous()
    pos = _pos(10)
    km = KeyMask(torch.full((B, 4), -1, dtype=torch.int64, device=DEV), cap)
    flash_attention_cached(q, k, v, key_mask=km, q_offset=pos, num_splits=n, return_lse=True)      # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                              # one stream, a linear chain of two kernels
        o, lse = flash_attention_cached(q, k, v, key_mask=km, q_offset=pos, num_splits=n, return_lse=True)
    gen = torch.Generator(device=DEV).manual_seed(11)
    for p in (0, 64, 199):
        pos.fill_(p)
        q.copy_(torch.randn(q.shape, device=DEV, generator=gen).bfloat16())
        keep = torch.rand(B, cap, device=DEV, generator=gen) > 0.2
        keep[:, p] = True
        km.bits.copy_(KeyMask.from_padding_mask(keep).bits)
        g.replay()
        ref = flash_attention_cached(q, k, v, key_mask=km, q_offset=p, num_splits=n, return_lse=True)
        _same((o, lse), ref, ("replay", p))
        assert torch.isfinite(lse).all()


def test_decode_step_does_not_synchronise():
    """smt_flash_mask + smt_flash_attention_forward of a decode step on a static cache (tensor offset,
    short mask) under torch's sync debug mode, where the build supports it; the result equals the
    integer call's."""
    B, Hq, Hkv, cap, p = 2, 8, 2, 200, 77
    q, k, v = _buffers(B, Hq, Hkv, 1, cap)
    am = torch.ones(B, p + 1, dtype=torch.bool, device=DEV)
    am[1, :9] = False
    level = _pos(p)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        guarded = True
    except Exception:
        guarded = False
    try:
        cm = smt_flash_mask(B, 1, cap, q_offset=level, attention_mask=am)
        level.add_(1)                                                      # the cache's update, before attention
        o, _ = smt_flash_attention_forward(None, q, k, v, cm)
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode:", "on" if guarded else "not available")
    assert isinstance(cm, CacheMask) and isinstance(cm.q_offset, torch.Tensor)
    full = torch.zeros(B, cap, dtype=torch.bool, device=DEV)
    full[:, :p + 1] = am
    ref = flash_attention_cached(q, k, v, key_mask=KeyMask.from_padding_mask(full), q_offset=p)
    assert torch.equal(o, ref)


def test_static_prefill_runs_the_same_length_forward():
    """The first forward on a static cache: 13 queries, 21 slots, a left-padded batch. The result is the
    training forward's on the first 13 slots, whatever the other slots hold."""
    from sparse_matrix_tuning_amd.fused_llama import flash_attention
    B, Sq, cap = 2, 13, 21
    q, k, v = _buffers(B, 8, 2, Sq, cap)
    k[:, :, Sq:] = float("nan")
    v[:, :, Sq:] = float("nan")
    am = torch.ones(B, Sq, dtype=torch.bool, device=DEV)
    am[1, :6] = False
    cm = smt_flash_mask(B, Sq, cap, q_offset=0, attention_mask=am)
    with torch.no_grad():
        o, _ = smt_flash_attention_forward(None, q, k, v, cm)
        ref = flash_attention(q, k[:, :, :Sq], v[:, :, :Sq], key_mask=KeyMask.from_padding_mask(am), any_length=True)
    assert torch.equal(o, ref) and torch.isfinite(o.float()).all()


def test_rejections():
    q, k, v = _buffers(2, 8, 2, 1, 64)
    with pytest.raises(ValueError):
        flash_attention_cached(q, k, v, q_offset=torch.tensor(3))                       # on the host
    with pytest.raises(ValueError):
        flash_attention_cached(q, k, v, q_offset=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        flash_attention_cached(q, k, v, q_offset=torch.zeros((), device=DEV))
    q9 = torch.randn(2, 8, 65, D, device=DEV).bfloat16()
    with pytest.raises(ValueError):
        flash_attention_cached(q9, k, v, q_offset=_pos(0))                              # Sq > capacity
