"""smt_attn_fwd_ld / smt_attn_bwd_ld (include/smt_attention.h, any sequence length): what they refuse,
they refuse with -1 and a message before any HIP call, so this runs without a device (the pattern of
test_abi.py: pointers that are never dereferenced)."""
import ctypes

from sparse_matrix_tuning_amd import _hip

TAB = ctypes.c_void_p(16)                                   # 16-byte aligned, never dereferenced


def _calls(S=66, dtype=_hip.DTYPE_BF16):
    lib = _hip.load()
    shape = _hip.AttnShape(1, 4, 2, S, 0.088, dtype)
    t = _hip.AttnTensor(TAB, 0, 0, 8)
    T, sh = ctypes.byref(t), ctypes.byref(shape)

    def fwd(lse=TAB, lse_ld=68, km=None, ds=None, de=None, p=0.0, seed=None):
        return lib.smt_attn_fwd_ld(T, T, T, T, lse, lse_ld, km, 2 if km else 0, ds, de, p, seed, sh, None)

    def bwd(lse=TAB, delta=TAB, lse_ld=68, km=None, ds=None, de=None, p=0.0, seed=None):
        return lib.smt_attn_bwd_ld(T, T, T, T, T, lse, delta, lse_ld, T, T, T, km, 2 if km else 0, ds, de, p, seed, sh,
                                   None)

    return lib, fwd, bwd, (T, sh)


def test_ld_entry_points_refuse_bad_arguments_before_any_hip_call():
    lib, fwd, bwd, _ = _calls()
    err = lib.smt_attn_last_error
    for name, call in (("smt_attn_fwd_ld", fwd), ("smt_attn_bwd_ld", bwd)):
        who = name.encode()
        assert call(lse_ld=64) == -1                        # lse_ld < S
        assert err().startswith(who) and b"lse_ld" in err() and b"< S" in err(), err()
        assert call(lse_ld=66) == -1 and call(lse_ld=70) == -1     # not a multiple of 4 (66 == S)
        assert err().startswith(who) and b"multiple of 4" in err(), err()
        assert call(lse=None) == -1                         # a null lse
        assert err().startswith(who) and b"null lse" in err(), err()
        assert call(ds=TAB) == -1 and call(de=TAB) == -1    # exactly one doc array
        assert err().startswith(who) and b"come together" in err(), err()
        assert call(km=TAB, ds=TAB, de=TAB) == -1           # a key mask together with documents
        assert err().startswith(who) and b"key mask" in err(), err()
        assert call(p=1.0, seed=TAB) == -1                  # p outside [0, 1)
        assert err().startswith(who) and b"outside [0, 1)" in err(), err()
        assert call(p=float("nan"), seed=TAB) == -1
        assert call(p=0.5) == -1                            # dropout without a seed
        assert err().startswith(who) and b"null seed" in err(), err()
    assert bwd(delta=None) == -1
    assert b"null lse / delta" in err()
    # misaligned lse / delta pointers are -2, as in the entry points without a stride
    assert bwd(lse=ctypes.c_void_p(20)) == -2
    assert b"16-byte aligned base pointers" in err()
    assert bwd(delta=ctypes.c_void_p(24)) == -2


def test_ld_entry_points_refuse_a_bad_shape_and_dtype():
    lib, fwd, bwd, _ = _calls(dtype=_hip.DTYPE_FP32)
    assert fwd() == -1 and b"not a 16-bit format" in lib.smt_attn_last_error()
    assert bwd() == -1 and b"not a 16-bit format" in lib.smt_attn_last_error()
    lib, fwd, bwd, _ = _calls(S=0)
    assert fwd(lse_ld=0) == -1 and b"bad shape" in lib.smt_attn_last_error()
    assert bwd(lse_ld=0) == -1 and b"bad shape" in lib.smt_attn_last_error()


def test_entry_points_without_a_stride_keep_their_contract():
    """lse_ld = S there: the backward at S = 66 is still -2 (16-byte rows), never a launch."""
    lib, _, _, (T, sh) = _calls(S=66)
    assert lib.smt_attn_bwd(T, T, T, T, T, TAB, TAB, T, T, T, sh, None) == -2
    assert b"16-byte rows" in lib.smt_attn_last_error()
    assert lib.smt_attn_bwd_kmask(T, T, T, T, T, TAB, TAB, T, T, T, TAB, 2, sh, None) == -2
    assert lib.smt_attn_bwd_dropout(T, T, T, T, T, TAB, TAB, T, T, T, None, 0, 0.5, TAB, sh, None) == -2
    assert lib.smt_attn_bwd_docs(T, T, T, T, T, TAB, TAB, T, T, T, TAB, TAB, 0.0, None, sh, None) == -2
