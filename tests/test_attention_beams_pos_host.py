"""Host side of the device-counter beam entry points: the ABI symbols, argument validation of
smt_attn_fwd_beams_pos and smt_attn_kv_append_pos before any HIP call (the pointers here are never
dereferenced: validation fails first), and the bookkeeping of BeamSharedCache(device_steps=True) on CPU
tensors against the host-counter cache, through the teacher-forced script of
tests/test_attention_beams_host.py. No device needed."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
from tests.test_attention_beams_host import SCRIPT

TAB = ctypes.c_void_p(1 << 20)                         # 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 2)
ROW = 1024


def _mk(p, s=128):
    return ctypes.byref(_hip.AttnTensor(p, 1 << 24, ROW, s)) if p is not None else None


def _call(lib, shape, nb=4, P=100, P_cap=None, T_cap=5, anc=TAB, anc_ld=None, steps=TAB, num_splits=1, ws=None,
          pm=None, pm_ld=0, q=TAB, kp=TAB, vp=TAB, kg=TAB, vg=TAB, o=TAB, ss=128):
    P_cap = P if P_cap is None else P_cap
    anc_ld = T_cap if anc_ld is None else anc_ld
    return lib.smt_attn_fwd_beams_pos(_mk(q), _mk(kp, ss), _mk(vp, ss), _mk(kg, ss), _mk(vg, ss), _mk(o), None, pm, pm_ld,
                                      anc, anc_ld, nb, P, P_cap, steps, T_cap, num_splits, ws, ctypes.byref(shape), None)


def _append(lib, kn=TAB, vn=TAB, kg=TAB, vg=TAB, steps=TAB, rows=8, Hkv=2, T_cap=5, dtype=_hip.DTYPE_BF16):
    return lib.smt_attn_kv_append_pos(_mk(kn), _mk(vn), _mk(kg), _mk(vg), steps, rows, Hkv, T_cap, dtype, None)


def test_symbols_are_declared_and_exported():
    lib = _hip.load(build_if_missing=True)
    for name in ("smt_attn_fwd_beams_pos", "smt_attn_kv_append_pos"):
        assert name in _hip.ABI_FUNCTIONS
        assert hasattr(lib, name)
    assert lib.smt_abi_version() == 13


def test_beams_pos_bad_arguments_return_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    good = _hip.AttnShape(2, 8, 2, 0, 0.088, _hip.DTYPE_BF16)
    cases = {                                              # what smt_attn_fwd_beams refuses, with T read as T_cap
        "null q": dict(q=None),
        "null k_prompt": dict(kp=None),
        "null v_prompt": dict(vp=None),
        "null k_gen": dict(kg=None),
        "null v_gen": dict(vg=None),
        "null o": dict(o=None),
        "null anc": dict(anc=None),
        "null steps": dict(steps=None),
        "nb =": dict(nb=0),
        "P =": dict(P=-1, P_cap=4),
        "T =": dict(T_cap=0),
        "P_cap": dict(P=100, P_cap=99),
        "anc_ld": dict(T_cap=5, anc_ld=4),
        "key_mask_ld": dict(P=129, pm=TAB, pm_ld=2),
        "num_splits": dict(num_splits=-1),
        "null workspace": dict(num_splits=2, ws=None),
    }
    for word, kw in cases.items():
        assert _call(lib, good, **kw) == -1, word
        err = lib.smt_attn_last_error()
        assert b"smt_attn_fwd_beams_pos" in err and word.encode() in err, (word, err)
    assert _call(lib, good, anc_ld=4) == -1 and b"T_cap" in lib.smt_attn_last_error()
    # the default split count is the capacity's: a long cache needs a workspace whatever the counter holds
    assert lib.smt_attn_beams_splits(ctypes.byref(good), 4, 2048, 256) > 1
    assert _call(lib, good, P=2048, T_cap=256, num_splits=0, ws=None) == -1
    assert b"null workspace" in lib.smt_attn_last_error()
    for bad in (_hip.DTYPE_FP32, 7):
        assert _call(lib, _hip.AttnShape(2, 8, 2, 0, 0.088, bad)) == -1
        assert b"smt_attn_fwd_beams_pos" in lib.smt_attn_last_error() and b"not a 16-bit format" in lib.smt_attn_last_error()
    assert _call(lib, _hip.AttnShape(2, 8, 3, 0, 0.088, _hip.DTYPE_BF16)) == -1          # Hq % Hkv
    assert b"Hq % Hkv" in lib.smt_attn_last_error()
    assert lib.smt_attn_fwd_beams_pos(None, None, None, None, None, None, None, None, 0, None, 0, 4, 1, 1, None, 1, 1,
                                      None, None, None) == -1
    assert b"null shape" in lib.smt_attn_last_error()
    # -2: a misaligned counter, misaligned rows, and the 2 GiB extents taken at the capacity
    assert _call(lib, good, steps=ODD) == -2
    err = lib.smt_attn_last_error()
    assert b"smt_attn_fwd_beams_pos" in err and b"steps" in err and b"4-byte" in err
    assert _call(lib, good, P=3, kp=ODD) == -2
    assert _call(lib, good, P=1 << 20, ss=1024) == -2
    assert b"k_prompt" in lib.smt_attn_last_error() and b"2 GiB" in lib.smt_attn_last_error()
    assert _call(lib, good, P=0, T_cap=1 << 20, ss=1024) == -2
    assert b"k_gen" in lib.smt_attn_last_error() and b"2 GiB" in lib.smt_attn_last_error()


def test_kv_append_bad_arguments_return_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    fn = b"smt_attn_kv_append_pos"
    for word, kw in {"null k_new": dict(kn=None), "null v_new": dict(vn=None), "null k_gen": dict(kg=None),
                     "null v_gen": dict(vg=None), "null steps": dict(steps=None), "rows =": dict(rows=0),
                     "Hkv =": dict(Hkv=0), "T_cap =": dict(T_cap=0)}.items():
        assert _append(lib, **kw) == -1, word
        err = lib.smt_attn_last_error()
        assert fn in err and word.encode() in err, (word, err)
    for bad in (_hip.DTYPE_FP32, 7):
        assert _append(lib, dtype=bad) == -1
        assert fn in lib.smt_attn_last_error() and b"not a 16-bit format" in lib.smt_attn_last_error()
    for word, kw in {"k_new": dict(kn=ODD), "v_new": dict(vn=ODD), "k_gen": dict(kg=ODD), "v_gen": dict(vg=ODD),
                     "steps": dict(steps=ODD)}.items():
        assert _append(lib, **kw) == -2, word
        err = lib.smt_attn_last_error()
        assert fn in err and word.encode() in err, (word, err)


class _Cfg:
    num_hidden_layers = 2


def test_device_steps_bookkeeping_matches_the_host_counter_cache_bit_for_bit():
    """The teacher-forced script of test_cache_bookkeeping_matches_dynamic_cache_bit_for_bit through a
    host-counter cache (itself bit-equal to a DynamicCache there) and a device_steps one."""
    N, nb, L, P, steps, Hkv, D = 2, 3, 2, 5, 7, 2, 128
    torch.manual_seed(0)
    host = BeamSharedCache(_Cfg(), nb, steps)
    dev = BeamSharedCache(_Cfg(), nb, steps, device_steps=True)
    assert dev.device_steps and not dev.graph and not host.device_steps and host.steps_tensor is None
    assert dev.steps_tensor is None                                    # allocated with the ancestry table
    for l in range(L):
        k = torch.randn(N, Hkv, P, D).to(torch.bfloat16).repeat_interleave(nb, 0)
        v = torch.randn(N, Hkv, P, D).to(torch.bfloat16).repeat_interleave(nb, 0)
        rk, rv = dev.update(k, v, l)
        assert rk is k and rv is v
        host.update(k, v, l)
    cnt = dev.steps_tensor
    assert cnt.dtype == torch.int32 and cnt.shape == (1,) and int(cnt) == 0
    ptrs = [(ly.k_gen.data_ptr(), ly.v_gen.data_ptr()) for ly in dev.layers]
    for step in range(steps + 1):
        idx = torch.tensor(SCRIPT[step])
        dev.reorder_cache(idx)
        host.reorder_cache(idx)
        assert dev.ancestry_updates == step + 1 and torch.equal(dev.ancestors, host.ancestors)
        for l in range(L):
            (gk, gv), (hk, hv) = dev.gather(l), host.gather(l)
            assert torch.equal(gk, hk) and torch.equal(gv, hv), (step, l)
        if step == steps:
            break
        assert dev.get_seq_length() == host.get_seq_length() == P + step
        assert dev.get_mask_sizes(1, 0) == host.get_mask_sizes(1, 0)
        for l in range(L):
            k = torch.randn(N * nb, 1, Hkv, D).to(torch.bfloat16).transpose(1, 2)      # the model's transposed view
            v = torch.randn(N * nb, 1, Hkv, D).to(torch.bfloat16).transpose(1, 2)
            rk, rv = dev.update(k, v, l)
            host.update(k, v, l)
            # the whole buffers, tagged; the counter moved once for both layers
            assert rk._smt_beam is dev.layers[l] and rv._smt_beam is dev.layers[l]
            assert rk.shape == (N * nb, Hkv, steps, D) and rv.shape == rk.shape
            assert (rk.data_ptr(), rv.data_ptr()) == ptrs[l]
            assert int(cnt) == step + 1 == dev.layers[l].steps
            (gk, gv), (hk, hv) = dev.gather(l), host.gather(l)
            assert torch.equal(gk, hk) and torch.equal(gv, hv), (step, l)
        assert dev.steps_tensor is cnt
    # the buffers are full: the step raises before anything changes
    z = torch.zeros(N * nb, Hkv, 1, D, dtype=torch.bfloat16)
    before = [ly.k_gen.clone() for ly in dev.layers]
    with pytest.raises(RuntimeError):
        dev.update(z, z, 0)
    assert int(cnt) == steps and [ly.steps for ly in dev.layers] == [steps] * L
    assert all(torch.equal(b, ly.k_gen) for b, ly in zip(before, dev.layers))
    dev.reset()
    assert int(cnt) == 0 and dev.steps_tensor is None and all(ly.steps == 0 for ly in dev.layers)
    assert dev.get_seq_length() == 0 and dev.ancestors is None


def test_the_device_counter_saturates_on_cpu_tensors_as_in_the_kernel():
    """The CPU update clamps the counter into [1, capacity] as smt_attn_kv_append_pos does: an
    out-of-contract counter cannot send the write outside the buffers."""
    nb, Hkv, D, cap = 2, 1, 128, 3
    c = BeamSharedCache(_Cfg(), nb, cap, device_steps=True)
    k0 = torch.zeros(2, Hkv, 4, D, dtype=torch.bfloat16)
    c.update(k0, k0, 0)
    c.layers[0].k_gen.zero_()
    c.layers[0].v_gen.zero_()
    one = torch.ones(2, Hkv, 1, D, dtype=torch.bfloat16)
    c.steps_tensor.fill_(40)                                           # + 1 by layer 0, then clamped to cap
    c.update(one, 2 * one, 0)
    ly = c.layers[0]
    assert (ly.k_gen[:, :, cap - 1] == 1).all() and (ly.v_gen[:, :, cap - 1] == 2).all()
    assert (ly.k_gen[:, :, :cap - 1] == 0).all()
    c.steps_tensor.fill_(-9)
    c.update(3 * one, 3 * one, 0)
    assert (ly.k_gen[:, :, 0] == 3).all() and (ly.k_gen[:, :, 1] == 0).all()


def test_the_default_constructor_behaves_as_before():
    nb, Hkv, D = 2, 1, 128
    c = BeamSharedCache(_Cfg(), nb, 4)
    assert not c.device_steps and not c.graph and c.graph_captures == 0 and c.graph_replays == 0
    k0 = torch.randn(2, Hkv, 3, D).to(torch.bfloat16)
    for l in range(2):
        c.update(k0, k0, l)
    assert c.steps_tensor is None
    for t in range(2):
        k1 = torch.randn(2, Hkv, 1, D).to(torch.bfloat16)
        rk, rv = c.update(k1, k1, 0)
        assert rk.shape == (2, Hkv, t + 1, D) and rk.data_ptr() == c.layers[0].k_gen.data_ptr()
        assert torch.equal(rk[:, :, t:], k1) and rk._smt_beam is c.layers[0]
    assert BeamSharedCache(_Cfg(), nb, 4, graph=True).device_steps     # graph implies device_steps
