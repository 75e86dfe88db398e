"""Packed sequences on the host: the document mask of the gfx950 flash attention
(fused_llama.DocMask, include/smt_attention.h ``smt_attn_*_docs``) and its transformers hook.

The three DocMask constructors (position ids, sequence ids, cumulative lengths) agree with each other
and with a Python loop over the document lengths. ``smt_flash_mask`` turns the mask function that
transformers' ``create_causal_mask`` really builds for a packed batch (restarting ``position_ids``, no
``attention_mask``) into a DocMask, recognised by its closures, and still refuses every other
non-causal mask function. No GPU is needed: the constructors are tensor ops."""
import pytest
import torch

from sparse_matrix_tuning_amd import fused_llama as fl
from sparse_matrix_tuning_amd.fused_llama import DocMask, KeyMask, flash_attention, smt_flash_mask

# rows of document lengths; every row of a layout sums to the same S
LAYOUTS = {
    "lengths_1_and_tile_edges": [[1, 63, 64, 130, 62, 256]],
    "one_document_per_row": [[40], [40]],
    "all_length_1": [[1] * 12],
    "rows_differ": [[5, 1, 1, 9], [16], [1, 15], [8, 8]],
    "length_1_last": [[7, 1]],
}


def _brute(rows):
    S = sum(rows[0])
    start = torch.empty(len(rows), S, dtype=torch.int32)
    end = torch.empty(len(rows), S, dtype=torch.int32)
    for b, lens in enumerate(rows):
        assert sum(lens) == S
        at = 0
        for n in lens:
            for i in range(at, at + n):
                start[b, i], end[b, i] = at, at + n
            at += n
    return start, end


def _position_ids(rows, first=0):
    return torch.tensor([[first + i for n in lens for i in range(n)] for lens in rows])


def _sequence_ids(rows):
    return torch.tensor([[7 * d + 3 for d, n in enumerate(lens) for _ in range(n)] for lens in rows])


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _check(dm, rows):
    start, end = _brute(rows)
    assert dm.S == start.shape[1]
    assert dm.start.dtype == torch.int32 and dm.end.dtype == torch.int32
    assert dm.start.is_contiguous() and dm.end.is_contiguous()
    assert torch.equal(dm.start, start), (dm.start, start)
    assert torch.equal(dm.end, end), (dm.end, end)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_constructors_agree_with_a_python_loop(name):
    rows = LAYOUTS[name]
    B, S = len(rows), sum(rows[0])
    _check(DocMask.from_position_ids(_position_ids(rows)), rows)
    _check(DocMask.from_sequence_ids(_sequence_ids(rows)), rows)
    _check(DocMask.from_cu_seqlens([_cu(lens) for lens in rows], B, S), rows)
    _check(DocMask.from_cu_seqlens([torch.tensor(_cu(lens)) for lens in rows], B, S), rows)
    if B == 1:
        _check(DocMask.from_cu_seqlens(_cu(rows[0]), 1, S), rows)
        _check(DocMask.from_cu_seqlens(torch.tensor(_cu(rows[0]), dtype=torch.int32), 1, S), rows)


def test_position_ids_that_restart_at_a_nonzero_position():
    # transformers' rule: a document starts wherever the difference to the previous position is not 1
    rows = [[4, 3, 1, 8]]
    pos = torch.tensor([[0, 1, 2, 3, 5, 6, 7, 2, 10, 11, 12, 13, 14, 15, 16, 17]])
    _check(DocMask.from_position_ids(pos), rows)
    _check(DocMask.from_position_ids(_position_ids(rows, first=3)), rows)
    # equal neighbours and a step of 2 both open a document
    _check(DocMask.from_position_ids(torch.tensor([[0, 0, 1, 3]])), [[1, 2, 1]])


def test_constructors_match_transformers_packed_indices():
    from transformers.masking_utils import find_packed_sequence_indices
    rows = LAYOUTS["rows_differ"]
    pos = _position_ids(rows)
    ids = find_packed_sequence_indices(pos)
    a, b = DocMask.from_position_ids(pos), DocMask.from_sequence_ids(ids)
    assert torch.equal(a.start, b.start) and torch.equal(a.end, b.end)


def _tiny_config():
    from transformers import LlamaConfig
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=64, num_hidden_layers=1,
                      num_attention_heads=2, num_key_value_heads=1, head_dim=128, max_position_embeddings=64)
    cfg._attn_implementation = fl.register_attention()
    return cfg


def _create(position_ids, **kw):
    from transformers.masking_utils import create_causal_mask
    B, S = position_ids.shape
    args = dict(config=_tiny_config(), inputs_embeds=torch.zeros(B, S, 256), attention_mask=None, past_key_values=None,
                position_ids=position_ids)
    args.update(kw)
    try:
        return create_causal_mask(**args)
    except TypeError:                                    # older transformers also ask for cache_position
        return create_causal_mask(cache_position=torch.arange(S), **args)


def test_smt_flash_mask_builds_a_doc_mask_from_what_transformers_hands_over():
    rows = LAYOUTS["rows_differ"]
    pos = _position_ids(rows)
    got = _create(pos)
    assert isinstance(got, DocMask)
    want = DocMask.from_position_ids(pos)
    assert torch.equal(got.start, want.start) and torch.equal(got.end, want.end) and got.S == want.S
    _check(got, rows)
    # an unpacked batch is still the plain causal path
    assert _create(_position_ids([[16], [16]])) is None


def test_smt_flash_mask_still_refuses_other_mask_functions():
    from transformers.masking_utils import (and_masks, causal_mask_function, packed_sequence_mask_function,
                                            sliding_window_causal_mask_function)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(1, 16, 16, mask_function=sliding_window_causal_mask_function(8))

    def mine(batch_idx, head_idx, q_idx, kv_idx):
        return kv_idx % 2 == 0
    with pytest.raises(NotImplementedError):
        smt_flash_mask(1, 16, 16, mask_function=and_masks(causal_mask_function, mine))
    pos = _position_ids([[5, 11]])
    with pytest.raises(NotImplementedError):             # the same through create_causal_mask, packing on top
        _create(pos, and_mask_function=mine)
    ids = torch.tensor([[0] * 5 + [1] * 11])
    packed = and_masks(causal_mask_function, packed_sequence_mask_function(ids))
    assert isinstance(smt_flash_mask(1, 16, 16, mask_function=packed), DocMask)
    with pytest.raises(NotImplementedError):             # packing with a KV offset (a cache)
        smt_flash_mask(1, 16, 16, kv_offset=4, mask_function=packed)
    with pytest.raises(NotImplementedError):
        smt_flash_mask(1, 16, 16, q_offset=4, mask_function=packed)
    with pytest.raises(NotImplementedError):             # the packed function without the causal one
        smt_flash_mask(1, 16, 16, mask_function=packed_sequence_mask_function(ids))
    with pytest.raises(NotImplementedError):
        smt_flash_mask(1, 16, 16, mask_function=and_masks(packed_sequence_mask_function(ids), causal_mask_function, mine))


def test_key_mask_together_with_doc_mask_raises():
    q = torch.zeros(1, 2, 16, 128, dtype=torch.bfloat16)
    k = v = torch.zeros(1, 1, 16, 128, dtype=torch.bfloat16)
    dm = DocMask.from_cu_seqlens([0, 5, 16], 1, 16)
    km = KeyMask.from_padding_mask(torch.ones(1, 16, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="trailing document"):
        flash_attention(q, k, v, key_mask=km, doc_mask=dm)
    ids = torch.tensor([[0] * 5 + [1] * 11])
    from transformers.masking_utils import and_masks, causal_mask_function, packed_sequence_mask_function
    with pytest.raises(NotImplementedError, match="trailing document"):
        smt_flash_mask(1, 16, 16, mask_function=and_masks(causal_mask_function, packed_sequence_mask_function(ids)),
                       attention_mask=torch.ones(1, 16, dtype=torch.bool))


def test_c_entry_points_validate_before_any_hip_call():
    import ctypes

    from sparse_matrix_tuning_amd import _hip
    lib = _hip.load()
    sp = ctypes.byref(_hip.AttnShape(1, 2, 1, 64, 0.125, _hip.DTYPE_BF16))
    arr = (ctypes.c_int32 * 64)()
    one = ctypes.cast(arr, ctypes.c_void_p)
    seed_p = ctypes.cast((ctypes.c_uint64 * 1)(7), ctypes.c_void_p)
    # exactly one array: refused, whatever else is passed
    for ds, de in ((one, None), (None, one)):
        assert lib.smt_attn_fwd_docs(None, None, None, None, None, ds, de, 0.0, None, sp, None) == -1
        assert b"smt_attn_fwd_docs" in lib.smt_attn_last_error() and b"doc_start and doc_end" in lib.smt_attn_last_error()
        assert lib.smt_attn_bwd_docs(None, None, None, None, None, None, None, None, None, None, ds, de, 0.0, None, sp,
                                     None) == -1
        assert b"smt_attn_bwd_docs" in lib.smt_attn_last_error() and b"doc_start and doc_end" in lib.smt_attn_last_error()
    # both NULL: the dropout / plain entry points answer
    assert lib.smt_attn_fwd_docs(None, None, None, None, None, None, None, 0.0, None, sp, None) == -1
    assert b"smt_attn_fwd: null q" in lib.smt_attn_last_error()
    assert lib.smt_attn_bwd_docs(None, None, None, None, None, None, None, None, None, None, None, None, 0.1, seed_p, sp,
                                 None) == -1
    assert b"smt_attn_bwd_dropout: null q" in lib.smt_attn_last_error()
    # both set: p and seed as in the dropout calls, then the tensors
    assert lib.smt_attn_fwd_docs(None, None, None, None, None, one, one, 1.0, seed_p, sp, None) == -1
    assert b" p " in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_docs(None, None, None, None, None, one, one, 0.1, None, sp, None) == -1
    assert b"seed" in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_docs(None, None, None, None, None, one, one, 0.0, None, sp, None) == -1
    assert b"smt_attn_fwd_docs: null q" in lib.smt_attn_last_error()
    assert lib.smt_attn_bwd_docs(None, None, None, None, None, None, None, None, None, None, one, one, 0.1, seed_p, sp,
                                 None) == -1
    assert b"smt_attn_bwd_docs: null q" in lib.smt_attn_last_error()
