"""Host side of the device-position cached attention: smt_attn_fwd_cached_pos refuses bad arguments
before any HIP call, and smt_flash_mask takes a static cache's tensor-valued q_offset (kept as a tensor
at q_length == 1, read once at q_length > 1) and its short padding mask. No device needed."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.fused_llama import CacheMask, KeyMask, smt_flash_mask

TAB = ctypes.c_void_p(1 << 20)                         # aligned, never dereferenced: validation fails first


def _call(lib, shape, Sq=1, pos=TAB, stride=0, num_splits=1, ws=None, q=TAB, k=TAB, o=TAB, ss=128):
    mk = lambda p: ctypes.byref(_hip.AttnTensor(p, 1024, 128, ss)) if p is not None else None
    return lib.smt_attn_fwd_cached_pos(mk(q), mk(k), mk(TAB), mk(o), None, None, 0, Sq, pos, stride, num_splits, ws,
                                       ctypes.byref(shape), None)


def test_bad_arguments_return_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    assert "smt_attn_fwd_cached_pos" in _hip.ABI_FUNCTIONS
    good = _hip.AttnShape(2, 8, 2, 100, 0.088, _hip.DTYPE_BF16)
    cases = {
        "null q": (dict(q=None), -1),
        "null k": (dict(k=None), -1),
        "null o": (dict(o=None), -1),
        "Sq": (dict(Sq=0), -1),
        "null positions": (dict(pos=None), -1),
        "8-byte alignment": (dict(pos=ctypes.c_void_p((1 << 20) + 4)), -2),
        "positions_stride": (dict(stride=2), -1),
        "key slot": (dict(Sq=101), -1),
        "num_splits": (dict(num_splits=-1), -1),
        "null workspace": (dict(num_splits=2, ws=None), -1),
    }
    for word, (kw, code) in cases.items():
        assert _call(lib, good, **kw) == code, word
        err = lib.smt_attn_last_error()
        assert err.startswith(b"smt_attn_fwd_cached_pos: ") and word.encode() in err, (word, err)
    assert _call(lib, good, stride=-1) == -1 and b"positions_stride" in lib.smt_attn_last_error()
    # the default split count follows the capacity and needs a workspace
    big = _hip.AttnShape(2, 8, 2, 4096, 0.088, _hip.DTYPE_BF16)
    assert lib.smt_attn_cached_splits(ctypes.byref(big), 1) > 1
    assert _call(lib, big, num_splits=0, ws=None) == -1 and b"null workspace" in lib.smt_attn_last_error()
    # the 2 GiB bound is taken on the capacity: 2^15 slots x 2^15 elements x 2 bytes
    wide = _hip.AttnShape(1, 8, 2, 1 << 15, 0.088, _hip.DTYPE_BF16)
    assert _call(lib, wide, ss=1 << 15) == -2 and b"2 GiB" in lib.smt_attn_last_error()
    for bad in (_hip.DTYPE_FP32, 7):
        assert _call(lib, _hip.AttnShape(2, 8, 2, 100, 0.088, bad)) == -1
        assert b"not a 16-bit format" in lib.smt_attn_last_error()
    assert _call(lib, _hip.AttnShape(2, 8, 3, 100, 0.088, _hip.DTYPE_BF16)) == -1 and b"bad shape" in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_cached_pos(None, None, None, None, None, None, 0, 1, None, 0, 1, None, None, None) == -1


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_mask_builder_keeps_a_tensor_offset_at_one_query(dtype):
    off = torch.tensor(36, dtype=dtype)
    cm = smt_flash_mask(2, 1, 64, q_offset=off)
    assert isinstance(cm, CacheMask) and cm.kv_length == 64 and cm.key_mask is None and cm.prefill is None
    assert isinstance(cm.q_offset, torch.Tensor) and cm.q_offset.dtype == dtype and cm.q_offset.item() == 36
    # the cache advances its counter in place before the attention runs: the mask holds its own copy
    off.add_(1)
    assert cm.q_offset.item() == 36
    # zero is a position like any other (nothing asks the tensor whether it is zero)
    cm = smt_flash_mask(2, 1, 64, q_offset=torch.tensor(0, dtype=dtype))
    assert isinstance(cm, CacheMask) and isinstance(cm.q_offset, torch.Tensor)
    cm = smt_flash_mask(2, 1, 1, q_offset=torch.tensor(0, dtype=dtype))
    assert isinstance(cm, CacheMask) and isinstance(cm.q_offset, torch.Tensor)


def test_mask_builder_reads_a_tensor_offset_once_for_several_queries():
    cm = smt_flash_mask(2, 3, 64, q_offset=torch.tensor(27))
    assert isinstance(cm, CacheMask) and cm.q_offset == 27 and isinstance(cm.q_offset, int) and cm.prefill is None
    cm = smt_flash_mask(2, 3, 64, q_offset=torch.tensor([5], dtype=torch.int32))
    assert cm.q_offset == 5 and isinstance(cm.q_offset, int)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 3, 64, q_offset=torch.tensor(62))              # queries [62, 65) of 64 slots


def test_short_mask_is_extended():
    am = torch.ones(2, 37, dtype=torch.bool)
    am[1, :9] = False                                     # a left-padded batch, 37 keys written, 64 slots
    cm = smt_flash_mask(2, 1, 64, q_offset=torch.tensor(36), attention_mask=am)
    full = torch.zeros(2, 64, dtype=torch.bool)
    full[:, :37] = am
    assert isinstance(cm.key_mask, KeyMask) and cm.key_mask.S == 64 and cm.kv_length == 64
    assert torch.equal(cm.key_mask.bits, KeyMask.from_padding_mask(full).bits)
    # an integer offset (a static cache before its first update reports 0) takes the short mask too
    cm = smt_flash_mask(2, 1, 64, q_offset=36, attention_mask=am)
    assert cm.q_offset == 36 and torch.equal(cm.key_mask.bits, KeyMask.from_padding_mask(full).bits)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=37, attention_mask=am)          # the query's own key is not covered


def test_static_prefill_carries_the_same_length_mask():
    am = torch.ones(2, 13, dtype=torch.bool)
    am[1, :6] = False
    for off in (0, torch.tensor(0)):
        cm = smt_flash_mask(2, 13, 21, q_offset=off, attention_mask=am)
        assert isinstance(cm, CacheMask) and cm.q_offset == 0 and cm.kv_length == 21
        (pm,) = cm.prefill
        assert isinstance(pm, KeyMask) and pm.S == 13 and torch.equal(pm.bits, KeyMask.from_padding_mask(am).bits)
        assert cm.key_mask.S == 21
    (pm,) = smt_flash_mask(2, 13, 21, q_offset=0, attention_mask=torch.ones(2, 13, dtype=torch.bool)).prefill
    assert pm is None                                     # every key valid: plain causal
    assert smt_flash_mask(2, 13, 21, q_offset=torch.tensor(0)).prefill == (None,)
    # a cache call of today (integer offset, no mask or a full-length one) is no static prefill
    assert smt_flash_mask(2, 4, 37, q_offset=0).prefill is None
    assert smt_flash_mask(2, 4, 37, q_offset=0, attention_mask=torch.ones(2, 37, dtype=torch.bool)).prefill is None


def test_tensor_kv_offset_and_bad_offsets_still_raise():
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=torch.tensor(36), kv_offset=torch.tensor(0))
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=36, kv_offset=torch.tensor(0))
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=torch.tensor(36), kv_offset=1)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=torch.tensor([3, 4]))           # one fill level per cache
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 64, q_offset=torch.tensor(3.0))
