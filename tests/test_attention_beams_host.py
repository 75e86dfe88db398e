"""Host side of the beam-shared cache: the ABI symbols, argument validation of smt_attn_fwd_beams before
any HIP call, the split / workspace helpers (pure host functions), and the bookkeeping of
BeamSharedCache on CPU tensors against transformers' DynamicCache. No device needed."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache

TAB = ctypes.c_void_p(1 << 20)                         # 16-byte aligned, never dereferenced: validation fails first
ROW = 1024                                             # element stride of a q / o row and of a K / V head


def _call(lib, shape, nb=4, P=100, P_cap=None, T=5, T_cap=None, anc=TAB, anc_ld=None, num_splits=1, ws=None,
          pm=None, pm_ld=0, q=TAB, kp=TAB, vp=TAB, kg=TAB, vg=TAB, o=TAB, ss=128):
    mk = lambda p, s=128: ctypes.byref(_hip.AttnTensor(p, 1 << 24, ROW, s)) if p is not None else None
    P_cap = P if P_cap is None else P_cap
    T_cap = T if T_cap is None else T_cap
    anc_ld = T if anc_ld is None else anc_ld
    return lib.smt_attn_fwd_beams(mk(q), mk(kp, ss), mk(vp, ss), mk(kg, ss), mk(vg, ss), mk(o), None, pm, pm_ld, anc,
                                  anc_ld, nb, P, P_cap, T, T_cap, num_splits, ws, ctypes.byref(shape), None)


def test_symbols_are_declared_and_exported():
    lib = _hip.load(build_if_missing=True)
    for name in ("smt_attn_beams_splits", "smt_attn_beams_workspace", "smt_attn_fwd_beams"):
        assert name in _hip.ABI_FUNCTIONS
        assert hasattr(lib, name)


def test_bad_arguments_return_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    good = _hip.AttnShape(2, 8, 2, 0, 0.088, _hip.DTYPE_BF16)
    cases = {
        "null q": dict(q=None),
        "null k_prompt": dict(kp=None),
        "null v_prompt": dict(vp=None),
        "null k_gen": dict(kg=None),
        "null v_gen": dict(vg=None),
        "null o": dict(o=None),
        "null anc": dict(anc=None),
        "nb =": dict(nb=0),
        "P =": dict(P=-1, P_cap=4),
        "T =": dict(T=0, T_cap=4),
        "P_cap": dict(P=100, P_cap=99),
        "T_cap": dict(T=5, T_cap=4),
        "anc_ld": dict(T=5, anc_ld=4),
        "key_mask_ld": dict(P=129, pm=TAB, pm_ld=2),
        "num_splits": dict(num_splits=-1),
        "null workspace": dict(num_splits=2, ws=None),
    }
    for word, kw in cases.items():
        assert _call(lib, good, **kw) == -1, word
        err = lib.smt_attn_last_error()
        assert b"smt_attn_fwd_beams" in err and word.encode() in err, (word, err)
    # the default split count of a long cache needs a workspace too
    assert lib.smt_attn_beams_splits(ctypes.byref(good), 4, 2048, 256) > 1
    assert _call(lib, good, P=2048, T=256, num_splits=0, ws=None) == -1
    assert b"null workspace" in lib.smt_attn_last_error()
    for bad in (_hip.DTYPE_FP32, 7):
        assert _call(lib, _hip.AttnShape(2, 8, 2, 0, 0.088, bad)) == -1
        assert b"smt_attn_fwd_beams" in lib.smt_attn_last_error() and b"not a 16-bit format" in lib.smt_attn_last_error()
    assert _call(lib, _hip.AttnShape(2, 8, 3, 0, 0.088, _hip.DTYPE_BF16)) == -1          # Hq % Hkv
    assert b"smt_attn_fwd_beams" in lib.smt_attn_last_error() and b"Hq % Hkv" in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_beams(None, None, None, None, None, None, None, None, 0, None, 0, 4, 1, 1, 1, 1, 1, None,
                                  None, None) == -1
    assert b"null shape" in lib.smt_attn_last_error()
    # extents of 2 GiB and more: the rows of one head are addressed with 32-bit byte offsets
    assert _call(lib, good, P=1 << 20, ss=1024) == -2
    assert b"k_prompt" in lib.smt_attn_last_error() and b"2 GiB" in lib.smt_attn_last_error()
    assert _call(lib, good, P=0, T=1 << 20, ss=1024) == -2
    assert b"k_gen" in lib.smt_attn_last_error() and b"2 GiB" in lib.smt_attn_last_error()
    # an absent prompt segment (P == 0) does not need its tensors' pointers; misaligned rows are -2
    assert _call(lib, good, P=3, kp=ctypes.c_void_p((1 << 20) + 2)) == -2


def test_split_heuristic_and_workspace():
    lib = _hip.load(build_if_missing=True)
    for Bn, Hq, Hkv in ((1, 8, 2), (2, 4, 4), (4, 32, 8), (16, 32, 8), (1, 32, 32)):
        for nb in (1, 4, 5, 40):
            for P in (0, 1, 63, 64, 65, 512, 4096):
                for T in (1, 64, 65, 256):
                    shape = _hip.AttnShape(Bn, Hq, Hkv, 0, 0.088, _hip.DTYPE_BF16)
                    n = lib.smt_attn_beams_splits(ctypes.byref(shape), nb, P, T)
                    tiles = -(-P // 64) + nb * -(-T // 64)
                    assert 1 <= n <= tiles, (Bn, Hq, Hkv, nb, P, T, n)
                    assert lib.smt_attn_beams_workspace(ctypes.byref(shape), nb, P, T, 1) == 0
                    ncb = -(-(nb * (Hq // Hkv)) // 32)
                    for ns in (0, 2, 7):
                        eff = ns or n
                        ws = lib.smt_attn_beams_workspace(ctypes.byref(shape), nb, P, T, ns)
                        # per (sample, kv head, column block, split): 32 columns of 128 fp32 O values, a max and a sum
                        need = Bn * Hkv * ncb * eff * 32 * (128 + 2) * 4
                        assert (ws == 0 and eff == 1) or ws >= need, (Bn, Hq, Hkv, nb, P, T, ns, ws, need)
    shape = _hip.AttnShape(4, 32, 8, 0, 0.088, _hip.DTYPE_BF16)          # the evaluation shape is split
    assert lib.smt_attn_beams_splits(ctypes.byref(shape), 4, 1024, 128) > 1
    for bad in (dict(nb=0), dict(P=-1), dict(T=0)):
        kw = dict(nb=4, P=10, T=1)
        kw.update(bad)
        assert lib.smt_attn_beams_splits(ctypes.byref(shape), kw["nb"], kw["P"], kw["T"]) == -1
        assert b"smt_attn_beams_splits" in lib.smt_attn_last_error()
        assert lib.smt_attn_beams_workspace(ctypes.byref(shape), kw["nb"], kw["P"], kw["T"], 2) == -1
    assert lib.smt_attn_beams_workspace(ctypes.byref(shape), 4, 10, 1, -1) == -1
    assert lib.smt_attn_beams_splits(ctypes.byref(_hip.AttnShape(4, 32, 5, 0, 0.088, _hip.DTYPE_BF16)), 4, 10, 1) == -1
    assert lib.smt_attn_beams_splits(None, 4, 10, 1) == -1


class _Cfg:
    num_hidden_layers = 2


# beam_idx after each forward (the first follows the prefill), 2 samples x 3 beams, within-sample.
# Step 3 lets hypothesis 1 of sample 0 (and 5 of sample 1) take over all beams: the other slots' earlier
# entries are dead from then on.
SCRIPT = [
    [0, 1, 2, 3, 4, 5],
    [1, 0, 0, 5, 5, 3],
    [2, 1, 0, 3, 4, 5],
    [1, 1, 1, 5, 5, 5],
    [0, 2, 1, 4, 3, 3],
    [2, 2, 0, 3, 5, 4],
    [0, 0, 1, 4, 4, 4],
    [1, 2, 0, 5, 3, 4],
]


def test_cache_bookkeeping_matches_dynamic_cache_bit_for_bit():
    from transformers import DynamicCache
    N, nb, L, P, steps, Hkv, D = 2, 3, 2, 5, 7, 2, 128
    torch.manual_seed(0)
    beam = BeamSharedCache(_Cfg(), nb, steps)
    dyn = DynamicCache()
    assert beam.get_seq_length() == 0 and beam.get_mask_sizes(P, 0) == (P, 0)
    # the prefill: generate() hands every layer the nb-times expanded rows
    for l in range(L):
        k = torch.randn(N, Hkv, P, D).to(torch.bfloat16).repeat_interleave(nb, 0)
        v = torch.randn(N, Hkv, P, D).to(torch.bfloat16).repeat_interleave(nb, 0)
        rk, rv = beam.update(k, v, l)
        assert rk is k and rv is v                                     # the prefill attention is unchanged
        dyn.update(k, v, l)
    ptrs = [(ly.k_gen.data_ptr(), ly.v_gen.data_ptr(), ly.k_prompt.data_ptr()) for ly in beam.layers]
    assert beam.layers[0].k_prompt.shape == (N, Hkv, P, D) and beam.layers[0].k_gen.shape == (N * nb, Hkv, steps, D)
    for step in range(steps + 1):
        idx = torch.tensor(SCRIPT[step])
        beam.reorder_cache(idx)
        dyn.reorder_cache(idx)
        assert beam.ancestry_updates == step + 1                       # once per token, not once per layer
        for l in range(L):
            gk, gv = beam.gather(l)
            assert torch.equal(gk, dyn.layers[l].keys) and torch.equal(gv, dyn.layers[l].values), (step, l)
        if step == steps:
            break
        assert beam.get_seq_length() == dyn.get_seq_length() == P + step
        assert beam.get_mask_sizes(1, 0) == dyn.get_mask_sizes(1, 0)
        for l in range(L):
            k = torch.randn(N * nb, Hkv, 1, D).to(torch.bfloat16)
            v = torch.randn(N * nb, Hkv, 1, D).to(torch.bfloat16)
            rk, rv = beam.update(k, v, l)
            assert rk._smt_beam is beam.layers[l] and rv._smt_beam is beam.layers[l]
            assert rk.shape == (N * nb, Hkv, step + 1, D) and rk.data_ptr() == ptrs[l][0]
            dk, dv = dyn.update(k, v, l)
            gk, gv = beam.gather(l)                                    # before the reorder: the own slots
            assert torch.equal(gk, dk) and torch.equal(gv, dv), (step, l)
        assert [(ly.k_gen.data_ptr(), ly.v_gen.data_ptr(), ly.k_prompt.data_ptr()) for ly in beam.layers] == ptrs
    # dead slots exist: after the take-over of step 3 no row of sample 0 points at slots 0 and 2 for steps 0..2
    anc = beam.ancestors
    assert anc.dtype == torch.uint8 and anc.shape == (N * nb, steps)
    assert len(set(anc[:3, 0].tolist())) == 1 and len(set(anc[3:, 0].tolist())) == 1
    assert int(anc.max()) < nb
    # the buffers are full
    with pytest.raises(RuntimeError):
        beam.update(torch.zeros(N * nb, Hkv, 1, D, dtype=torch.bfloat16), torch.zeros(N * nb, Hkv, 1, D, dtype=torch.bfloat16), 0)


def test_generate_drives_the_cache_as_it_drives_a_dynamic_cache():
    """generate(num_beams=3) on a small fp32 eager LLaMA on the CPU. The beam kernel needs a device, so
    the layers here hand the model gather() in place of the tagged buffers: what is checked is the
    bookkeeping under generate() itself (expanded prefill, one reorder per token, mask sizes), and since
    gather() is bit-equal to a DynamicCache's tensors the tokens are identical."""
    from transformers import DynamicCache, LlamaConfig, LlamaForCausalLM
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedLayer

    class GatheredLayer(BeamSharedLayer):
        def update(self, k, v, *args, **kwargs):
            prefill = not self.is_initialized
            out = super().update(k, v, *args, **kwargs)
            return out if prefill else self.gather()

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=16, vocab_size=97, max_position_embeddings=64, pad_token_id=0,
                      bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    ids = torch.randint(3, 97, (2, 9))
    mask = torch.ones(2, 9, dtype=torch.int64)
    ids[1, :4] = 0
    mask[1, :4] = 0
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=8, min_new_tokens=8, do_sample=False, num_beams=3)
    cache = BeamSharedCache(cfg, 3, 8)
    assert len(cache.layers) == 2
    cache.layers = [GatheredLayer(cache.state) for _ in cache.layers]
    forwards = []
    hook = model.register_forward_pre_hook(lambda m, a: forwards.append(1))
    with torch.no_grad():
        out = model.generate(**kw, past_key_values=cache)
        hook.remove()
        ref = model.generate(**kw, past_key_values=DynamicCache(config=cfg))
    assert out.shape == (2, 17) and torch.equal(out, ref)
    assert len(forwards) == 8 and cache.ancestry_updates == 8           # once per token, not once per layer
    assert [ly.steps for ly in cache.layers] == [7, 7]
    assert cache.layers[0].k_prompt.shape == (2, 2, 9, 16) and cache.layers[0].k_gen.shape == (6, 2, 8, 16)


def test_unsupported_cache_operations_raise():
    nb, Hkv, D = 2, 1, 128
    beam = BeamSharedCache(_Cfg(), nb, 4)
    k = torch.zeros(4, Hkv, 3, D, dtype=torch.bfloat16)
    for l in range(2):
        beam.update(k, k, l)
    with pytest.raises(NotImplementedError):
        beam.update(k[:, :, :2], k[:, :, :2], 0)                      # Sq > 1 after the prefill
    for call in (lambda: beam.crop(-1), lambda: beam.batch_repeat_interleave(2),
                 lambda: beam.batch_select_indices(torch.tensor([0]))):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        BeamSharedCache(_Cfg(), 3, 4).update(k, k, 0)                  # 4 rows, 3 beams
    with pytest.raises(ValueError):
        BeamSharedCache(_Cfg(), 0, 4)
