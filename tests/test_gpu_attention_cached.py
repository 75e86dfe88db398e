"""Cached (KV-cache) attention, smt_attn_fwd_cached / flash_attention_cached: the split-KV decode
kernel against an fp32 masked softmax on the same 16-bit inputs. The bar is the project's own
(tests/test_gpu_attention.py): relative norm error of o <= max(8e-3, 1.5 x the error of torch's 16-bit
sdpa with the same boolean mask), lse (log2 units) within 2e-3 abs. Rows without a visible key:
o == 0, lse == +inf. B = 2 throughout; the shapes are the smallest that reach each branch (one tile,
a ragged tile, several tiles, several splits, empty splits, two column blocks)."""
import pytest
import torch
import torch.nn.functional as F

from sparse_matrix_tuning_amd.fused_llama import (CacheMask, DocMask, KeyMask, flash_attention, flash_attention_cached,
                                                  smt_flash_attention_forward, smt_flash_mask)
from tests.attn_ref import D, DEV, allowed_cached, ref32, rel as _rel

pytestmark = pytest.mark.gpu
B = 2


def _allowed(Sq, Skv, q_offset, keep):
    """bool [B, 1, Sq, Skv]: query i (at position q_offset + i) sees key j."""
    return allowed_cached(B, Sq, Skv, q_offset, keep)


def _ref_masked(q, k, v, scale, allowed):
    """The fp32 reference, forward only: o [B, Sq, Hq, D], lse in log2 units and visible, both [B, Hq, Sq]."""
    o, _, _, _, lse2, visible = ref32(q, k, v, None, scale, allowed)
    return o, lse2, visible


# torch's own 16-bit sdpa under the boolean mask (the bar of this file's header), so not in tests/attn_ref.py
def _sdpa16(q, k, v, scale, allowed):
    G = q.shape[1] // k.shape[1]
    o = F.scaled_dot_product_attention(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1),
                                       attn_mask=allowed, scale=scale)
    return o.transpose(1, 2)


def _judge(o, lse, q, k, v, q_offset, keep=None, what=""):
    """o [B, Sq, Hq, D] and lse [B, Hq, Sq] of a cached call on (q, k, v) against the fp32 reference."""
    Sq, Skv = q.shape[2], k.shape[2]
    scale = D ** -0.5
    allowed = _allowed(Sq, Skv, q_offset, keep)
    ro, rlse, visible = _ref_masked(q, k, v, scale, allowed)
    vis_o = visible.transpose(1, 2)[..., None].expand(B, Sq, q.shape[1], D)       # [B, Sq, Hq, D]
    assert o.shape == ro.shape and o.dtype == q.dtype, what
    assert torch.isfinite(o.float()).all(), what
    assert (o.float()[~vis_o] == 0).all(), what
    so = _sdpa16(q, k, v, scale, allowed).float().masked_fill(~vis_o, 0.0)       # sdpa: NaN rows where nothing is visible
    e, es = _rel(o.float(), ro), _rel(so, ro)
    print(f"{what}: rel err {e:.3e} (sdpa {es:.3e})")
    assert e <= max(8e-3, 1.5 * es), (what, e, es)
    if lse is not None:
        vis = visible.expand_as(rlse)
        assert (lse[vis] - rlse[vis]).abs().max().item() < 2e-3, what
        assert torch.isinf(lse[~vis]).all() and (lse[~vis] > 0).all(), what
    return e


def _qkv(Hq, Hkv, Sq, Skv, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(1000 * Skv + 10 * Hq + Sq + seed)
    q = torch.randn(B, Sq, Hq, D, device=DEV).to(dtype).transpose(1, 2)           # transformers' layout
    k = torch.randn(B, Hkv, Skv, D, device=DEV).to(dtype)
    v = torch.randn(B, Hkv, Skv, D, device=DEV).to(dtype)
    return q, k, v


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("Skv", [1, 63, 64, 65, 130, 1000])
def test_decode_one_query(Skv, Hq, Hkv):
    q, k, v = _qkv(Hq, Hkv, 1, Skv)
    o, lse = flash_attention_cached(q, k, v, return_lse=True)
    _judge(o, lse, q, k, v, Skv - 1, what=f"Skv {Skv} Hq {Hq} Hkv {Hkv}")


def test_decode_fp16():
    q, k, v = _qkv(8, 2, 1, 130, dtype=torch.float16)
    o, lse = flash_attention_cached(q, k, v, return_lse=True)
    _judge(o, lse, q, k, v, 129, what="fp16")


@pytest.mark.parametrize("Skv", [65, 1000])
def test_forced_splits(Skv):
    """1, 2 and 7 splits (at Skv 65 there are two tiles: five of seven splits are empty) each meet the
    bar, and a second run with the same split count is bit-identical."""
    q, k, v = _qkv(8, 2, 1, Skv)
    for ns in (1, 2, 7):
        o, lse = flash_attention_cached(q, k, v, num_splits=ns, return_lse=True)
        _judge(o, lse, q, k, v, Skv - 1, what=f"Skv {Skv} splits {ns}")
        o2, lse2 = flash_attention_cached(q, k, v, num_splits=ns, return_lse=True)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), ns


@pytest.mark.parametrize("Sq,q_offset,Skv,splits", [
    (5, 60, 65, None),          # the causal edge crosses a tile boundary inside the call
    (5, 60, 65, 2),
    (9, 121, 130, None),        # 36 columns at G = 4: two column blocks
    (9, 121, 130, 3),
    (40, 0, 40, None),          # a same-length call through the cached kernel
])
def test_several_query_positions(Sq, q_offset, Skv, splits):
    q, k, v = _qkv(8, 2, Sq, Skv)
    o, lse = flash_attention_cached(q, k, v, q_offset=q_offset, num_splits=splits, return_lse=True)
    _judge(o, lse, q, k, v, q_offset, what=f"Sq {Sq} offset {q_offset} Skv {Skv} splits {splits}")


@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("splits", [None, 1, 3])
def test_key_mask_left_padding_and_hole(Sq, splits):
    Skv = 130
    q, k, v = _qkv(8, 2, Sq, Skv)
    keep = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
    keep[1, :70] = False                                    # left padding: 0 keys in row 0, 70 in row 1
    keep[0, 40] = keep[1, 100] = False                      # holes inside the visible range
    cm = smt_flash_mask(B, Sq, Skv, q_offset=Skv - Sq, attention_mask=keep.long())
    assert isinstance(cm, CacheMask) and cm.q_offset == Skv - Sq
    # a NaN in a masked row must not reach o
    k, v = k.clone(), v.clone()
    k[1, :, 3] = float("nan")
    v[1, :, 5] = float("nan")
    v[0, :, 40] = float("inf")
    o, lse = flash_attention_cached(q, k, v, key_mask=cm.key_mask, q_offset=cm.q_offset, num_splits=splits,
                                    return_lse=True)
    clean = lambda t: torch.where(keep[:, None, :, None], t, torch.zeros_like(t))
    _judge(o, lse, q, clean(k), clean(v), Skv - Sq, keep, what=f"kmask Sq {Sq} splits {splits}")


@pytest.mark.parametrize("splits", [1, 3])
def test_key_mask_row_without_a_visible_key(splits):
    """Row 1's visible keys are all masked: o == 0, lse == +inf there, finite everywhere else."""
    Skv, Sq = 130, 2
    q, k, v = _qkv(4, 2, Sq, Skv)
    keep = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
    keep[1] = False
    keep[0, :5] = False
    o, lse = flash_attention_cached(q, k, v, key_mask=KeyMask.from_padding_mask(keep), num_splits=splits, return_lse=True)
    assert (o[1].float() == 0).all() and torch.isinf(lse[1]).all() and (lse[1] > 0).all()
    assert torch.isfinite(lse[0]).all()
    _judge(o, lse, q, k, v, Skv - Sq, keep, what=f"dead row splits {splits}")


def test_strides():
    Hq, Hkv, Skv = 8, 2, 100
    torch.manual_seed(5)
    # k / v: the [:, :, :Skv] slice of a pre-allocated [B, Hkv, 256, 128] buffer
    kb = torch.randn(B, Hkv, 256, D, device=DEV).bfloat16()
    vb = torch.randn(B, Hkv, 256, D, device=DEV).bfloat16()
    # q: a slice of a joint q|k|v projection output [B, 1, (Hq + 2 Hkv) * D]
    joint = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=DEV).bfloat16()
    q = joint[:, :, :Hq * D].view(B, 1, Hq, D).transpose(1, 2)
    k, v = kb[:, :, :Skv], vb[:, :, :Skv]
    assert not k.is_contiguous() and not q.is_contiguous()
    o, lse = flash_attention_cached(q, k, v, return_lse=True)
    _judge(o, lse, q, k, v, Skv - 1, what="buffer slice")
    # k / v: transposed views of a [B, Skv, Hkv, 128]-ordered cache
    k2 = k.transpose(1, 2).contiguous().transpose(1, 2)
    v2 = v.transpose(1, 2).contiguous().transpose(1, 2)
    assert k2.stride(2) == Hkv * D
    o2, lse2 = flash_attention_cached(q, k2, v2, return_lse=True)
    _judge(o2, lse2, q, k2, v2, Skv - 1, what="[B, S, H, D] cache")
    assert torch.equal(o, o2)


@pytest.mark.parametrize("splits", [None, 1, 2])
def test_garbage_tail_is_never_read(splits):
    """A fixed-size cache: Skv 192 slots, the queries end at position 69, rows 70..191 hold NaN."""
    Skv, Sq, q_offset = 192, 2, 68
    q, k, v = _qkv(8, 2, Sq, Skv)
    k[:, :, 70:] = float("nan")
    v[:, :, 70:] = float("nan")
    o, lse = flash_attention_cached(q, k, v, q_offset=q_offset, num_splits=splits, return_lse=True)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    _judge(o, lse, q, k[:, :, :70], v[:, :, :70], q_offset, what=f"garbage tail splits {splits}")


def test_agrees_with_the_training_forward():
    """Row p of the training kernel's causal forward at S 128 and the cached call with q_offset = p,
    Skv = p + 1: each judged against the fp32 reference."""
    S, Hq, Hkv = 128, 8, 2
    q, k, v = _qkv(Hq, Hkv, S, S)
    with torch.no_grad():
        full = flash_attention(q, k, v)                                         # [B, S, Hq, D]
    allowed = _allowed(S, S, 0, None)
    ro, _, _ = _ref_masked(q, k, v, D ** -0.5, allowed)
    so = _sdpa16(q, k, v, D ** -0.5, allowed).float()
    for p in (0, 63, 64, 127):
        qp = q[:, :, p:p + 1]
        o, lse = flash_attention_cached(qp, k[:, :, :p + 1], v[:, :, :p + 1], q_offset=p, return_lse=True)
        _judge(o, lse, qp, k[:, :, :p + 1], v[:, :, :p + 1], p, what=f"row {p} cached")
        e, es = _rel(full[:, p].float(), ro[:, p]), _rel(so[:, p], ro[:, p])
        assert e <= max(8e-3, 1.5 * es), ("training forward", p, e, es)


def test_transformers_interface_dispatch():
    """smt_flash_attention_forward sends a CacheMask, Sq != Skv and a no-grad S % 4 != 0 same-length
    call to the cached kernel."""
    q, k, v = _qkv(8, 2, 1, 37)
    cm = smt_flash_mask(B, 1, 37, q_offset=36)
    o, _ = smt_flash_attention_forward(None, q, k, v, cm)
    _judge(o, None, q, k, v, 36, what="interface decode")
    o, _ = smt_flash_attention_forward(None, q, k, v, None)
    _judge(o, None, q, k, v, 36, what="interface Sq != Skv")
    q, k, v = _qkv(8, 2, 13, 13)
    keep = torch.ones(B, 13, dtype=torch.bool, device=DEV)
    keep[1, :6] = False
    km = smt_flash_mask(B, 13, 13, attention_mask=keep.long())
    assert isinstance(km, KeyMask)
    with torch.no_grad():
        o, _ = smt_flash_attention_forward(None, q, k, v, km)
    _judge(o, None, q, k, v, 0, keep, what="interface odd prefill")


def test_rejections():
    q, k, v = _qkv(4, 2, 1, 20)
    with pytest.raises(NotImplementedError):
        flash_attention_cached(q.detach().requires_grad_(True), k, v)
    with torch.no_grad():
        flash_attention_cached(q.detach().requires_grad_(True), k, v)           # no gradient asked: fine
    cm = smt_flash_mask(B, 1, 20, q_offset=19)
    with pytest.raises(NotImplementedError):
        smt_flash_attention_forward(None, q, k, v, cm, dropout=0.1)
    docs = DocMask.from_sequence_ids(torch.zeros(B, 20, dtype=torch.int64, device=DEV))
    with pytest.raises(NotImplementedError):
        smt_flash_attention_forward(None, q, k, v, docs)
    with pytest.raises(ValueError):
        flash_attention_cached(q, k, v, q_offset=20)                            # no key slot of its own
