"""Host side of the cached (KV-cache) attention: argument validation of smt_attn_fwd_cached before any
HIP call, the split heuristic and workspace size (pure host functions), and what smt_flash_mask
returns for cache-shaped and training-shaped calls. No device needed."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.fused_llama import CacheMask, DocMask, KeyMask, smt_flash_mask

TAB = ctypes.c_void_p(1 << 20)                         # 16-byte aligned, never dereferenced: validation fails first


def _call(lib, shape, Sq=1, q_offset=None, num_splits=1, ws=None, q=TAB, k=TAB, o=TAB):
    mk = lambda p: ctypes.byref(_hip.AttnTensor(p, 1024, 128, 128)) if p is not None else None
    q_offset = shape.S - Sq if q_offset is None else q_offset
    return lib.smt_attn_fwd_cached(mk(q), mk(k), mk(TAB), mk(o), None, None, 0, Sq, q_offset, num_splits, ws,
                                   ctypes.byref(shape), None)


def test_bad_arguments_return_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    good = _hip.AttnShape(2, 8, 2, 100, 0.088, _hip.DTYPE_BF16)
    cases = {
        "null q": dict(q=None),
        "null k": dict(k=None),
        "null o": dict(o=None),
        "Sq": dict(Sq=0),
        "q_offset": dict(q_offset=-1),
        "key slot": dict(Sq=2, q_offset=99),
        "num_splits": dict(num_splits=-1),
        "null workspace": dict(num_splits=2, ws=None),
    }
    for word, kw in cases.items():
        assert _call(lib, good, **kw) == -1, word
        assert word.encode() in lib.smt_attn_last_error(), (word, lib.smt_attn_last_error())
    # the default split count of this shape needs a workspace too
    big = _hip.AttnShape(2, 8, 2, 4096, 0.088, _hip.DTYPE_BF16)
    assert lib.smt_attn_cached_splits(ctypes.byref(big), 1) > 1
    assert _call(lib, big, num_splits=0, ws=None) == -1
    assert b"null workspace" in lib.smt_attn_last_error()
    for bad in (_hip.DTYPE_FP32, 7):
        assert _call(lib, _hip.AttnShape(2, 8, 2, 100, 0.088, bad)) == -1
        assert b"not a 16-bit format" in lib.smt_attn_last_error()
    assert _call(lib, _hip.AttnShape(2, 8, 3, 100, 0.088, _hip.DTYPE_BF16)) == -1          # Hq % Hkv
    assert b"bad shape" in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_cached(None, None, None, None, None, None, 0, 1, 0, 1, None, None, None) == -1


def test_split_heuristic_and_workspace():
    lib = _hip.load(build_if_missing=True)
    for Bn, Hq, Hkv in ((1, 8, 2), (2, 4, 4), (16, 32, 8), (64, 32, 8), (1, 32, 32)):
        for Skv in (1, 63, 64, 65, 128, 129, 512, 2048, 8192, 100000):
            for Sq in (1, 5, 9, 100):
                if Sq > Skv:
                    continue
                shape = _hip.AttnShape(Bn, Hq, Hkv, Skv, 0.088, _hip.DTYPE_BF16)
                n = lib.smt_attn_cached_splits(ctypes.byref(shape), Sq)
                tiles = -(-Skv // 64)
                assert 1 <= n <= tiles, (Bn, Hq, Hkv, Skv, Sq, n)
                if Skv <= 64:
                    assert n == 1
                assert lib.smt_attn_cached_workspace(ctypes.byref(shape), Sq, 1) == 0
                ncb = -(-(Sq * (Hq // Hkv)) // 32)
                for ns in (0, 2, 7):
                    eff = ns or n
                    ws = lib.smt_attn_cached_workspace(ctypes.byref(shape), Sq, ns)
                    # per (b, kv head, column block, split): 32 columns of 128 fp32 O values, a max and a sum
                    need = Bn * Hkv * ncb * eff * 32 * (128 + 2) * 4
                    assert (ws == 0 and eff == 1) or ws >= need, (Bn, Hq, Hkv, Skv, Sq, ns, ws, need)
    # the evaluation shape is split (128 (b, kv head) pairs alone would leave half the CUs idle)
    shape = _hip.AttnShape(16, 32, 8, 2048, 0.088, _hip.DTYPE_BF16)
    assert lib.smt_attn_cached_splits(ctypes.byref(shape), 1) > 1
    assert lib.smt_attn_cached_splits(ctypes.byref(shape), 0) == -1
    assert lib.smt_attn_cached_workspace(ctypes.byref(shape), 1, -1) == -1


def test_mask_builder_with_a_cache():
    am = torch.ones(2, 37, dtype=torch.int64)
    am[1, :9] = 0                                         # a left-padded batch
    cm = smt_flash_mask(2, 1, 37, q_offset=36, attention_mask=am)
    assert isinstance(cm, CacheMask) and cm.q_offset == 36 and cm.kv_length == 37
    assert isinstance(cm.key_mask, KeyMask) and cm.key_mask.S == 37
    assert torch.equal(cm.key_mask.bits, KeyMask.from_padding_mask(am).bits)
    # no mask: nothing to build; a longer mask is cut to the cache length
    cm = smt_flash_mask(2, 1, 37, q_offset=36)
    assert isinstance(cm, CacheMask) and cm.key_mask is None
    cm = smt_flash_mask(2, 3, 30, q_offset=27, attention_mask=am)
    assert cm.q_offset == 27 and torch.equal(cm.key_mask.bits, KeyMask.from_padding_mask(am[:, :30]).bits)
    # a chunked prefill: q_offset 0 but fewer queries than keys is a cache call as well
    assert isinstance(smt_flash_mask(2, 4, 37, q_offset=0), CacheMask)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 37, q_offset=36, kv_offset=1, attention_mask=am)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 37, 37, kv_offset=1)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 37, q_offset=36, mask_function=lambda b, h, q, k: q >= k)


def test_packed_ids_with_a_cache_raise():
    from transformers.masking_utils import and_masks, causal_mask_function, packed_sequence_mask_function
    ids = torch.zeros(2, 37, dtype=torch.int64)
    fn = and_masks(causal_mask_function, packed_sequence_mask_function(ids))
    assert isinstance(smt_flash_mask(2, 37, 37, mask_function=fn), DocMask)      # the training call still works
    with pytest.raises(NotImplementedError):
        smt_flash_mask(2, 1, 37, q_offset=36, mask_function=fn)


def test_training_shaped_calls_are_unchanged():
    from transformers.masking_utils import and_masks, causal_mask_function, packed_sequence_mask_function
    assert smt_flash_mask(2, 16, 16) is None
    assert smt_flash_mask(2, 16, 16, mask_function=causal_mask_function) is None
    assert smt_flash_mask(2, 16, 16, attention_mask=torch.ones(2, 16, dtype=torch.int64)) is None
    am = torch.ones(2, 16, dtype=torch.int64)
    am[0, 12:] = 0
    km = smt_flash_mask(2, 16, 16, attention_mask=am)
    assert isinstance(km, KeyMask) and torch.equal(km.bits, KeyMask.from_padding_mask(am).bits)
    ids = torch.tensor([[0] * 10 + [1] * 6, [0] * 16])
    dm = smt_flash_mask(2, 16, 16, mask_function=and_masks(causal_mask_function, packed_sequence_mask_function(ids)))
    assert isinstance(dm, DocMask)
    ref = DocMask.from_sequence_ids(ids)
    assert torch.equal(dm.start, ref.start) and torch.equal(dm.end, ref.end)
