"""Attention dropout without a GPU: the threshold and the argument validation of the C ABI
(include/smt_attention.h, ``smt_attn_*_dropout``), and the statistics of the keep function, measured on
its numpy restatement (tests/dropout_keep_ref.py).

Statistics, over the causal region (key <= q) of every (seed, p, shape) below, against the binomial
with the effective rate p_eff = t / 256: aggregates (keep counts overall and per head, lag-1 agreement
along key and along q, agreement between every pair of (batch, head) slices, agreement between seed and
seed + 1) within 5 sigma; row and column keep counts with >= 64 visible elements within 6 sigma.
"""
import ctypes

import numpy as np
import pytest

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd.fused_llama import dropout_effective_p
from tests.dropout_keep_ref import keep_mask, threshold

SEEDS = (0, 1, 12345, 2 ** 63 - 1, 0x5DEECE66D1234ABC & (2 ** 63 - 1))
RATES = (0.02, 0.1, 0.5)
SHAPES = ((2, 4, 256), (1, 2, 200), (1, 8, 512))


def test_threshold():
    lib = _hip.load()
    for p, t in ((0.0, 0), (0.1, 26), (0.5, 128), (0.999, 255), (-0.1, -1), (1.0, -1), (float("nan"), -1)):
        assert lib.smt_attn_dropout_threshold(p) == t, p
    for p in (0.0, 0.001, 0.002, 0.02, 0.1, 0.25, 0.5, 0.9, 0.999):
        assert lib.smt_attn_dropout_threshold(p) == threshold(p), p
    assert dropout_effective_p(0.1) == 26 / 256
    assert dropout_effective_p(0.0) == 0.0
    with pytest.raises(ValueError, match="outside"):
        dropout_effective_p(1.0)


def test_validation_errors_without_gpu():
    lib = _hip.load()
    shape = _hip.AttnShape(1, 2, 1, 64, 0.125, _hip.DTYPE_BF16)
    sp = ctypes.byref(shape)
    seed = (ctypes.c_uint64 * 1)(7)                        # a host address: never dereferenced by these calls
    seed_p = ctypes.cast(seed, ctypes.c_void_p)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert lib.smt_attn_fwd_dropout(None, None, None, None, None, None, 0, bad, seed_p, sp, None) == -1
        assert b" p " in lib.smt_attn_last_error() and b"smt_attn_fwd_dropout" in lib.smt_attn_last_error()
        assert lib.smt_attn_bwd_dropout(None, None, None, None, None, None, None, None, None, None, None, 0, bad,
                                        seed_p, sp, None) == -1
        assert b" p " in lib.smt_attn_last_error() and b"smt_attn_bwd_dropout" in lib.smt_attn_last_error()
        assert lib.smt_attn_dropout_mask(None, bad, seed_p, sp, None) == -1
        assert b" p " in lib.smt_attn_last_error() and b"smt_attn_dropout_mask" in lib.smt_attn_last_error()
    # a null seed with t > 0
    assert lib.smt_attn_fwd_dropout(None, None, None, None, None, None, 0, 0.1, None, sp, None) == -1
    assert b"seed" in lib.smt_attn_last_error()
    assert lib.smt_attn_bwd_dropout(None, None, None, None, None, None, None, None, None, None, None, 0, 0.1, None,
                                    sp, None) == -1
    assert b"seed" in lib.smt_attn_last_error()
    assert lib.smt_attn_dropout_mask(None, 0.1, None, sp, None) == -1
    assert b"seed" in lib.smt_attn_last_error()
    # t == 0 forwards to the plain functions (seed may be null): their own validation answers
    assert lib.smt_attn_fwd_dropout(None, None, None, None, None, None, 0, 0.0, None, sp, None) == -1
    assert b"smt_attn_fwd: null q" in lib.smt_attn_last_error()
    assert lib.smt_attn_bwd_dropout(None, None, None, None, None, None, None, None, None, None, None, 0, 0.001, None,
                                    sp, None) == -1
    assert b"smt_attn_bwd: null q" in lib.smt_attn_last_error()
    # valid p and seed: the remaining arguments are checked as before, still without a HIP call
    assert lib.smt_attn_fwd_dropout(None, None, None, None, None, None, 0, 0.1, seed_p, sp, None) == -1
    assert b"smt_attn_fwd_dropout: null q" in lib.smt_attn_last_error()
    assert lib.smt_attn_dropout_mask(None, 0.1, seed_p, sp, None) == -1
    assert b"null keep" in lib.smt_attn_last_error()
    assert lib.smt_attn_dropout_mask(None, 0.1, seed_p, None, None) == -1
    assert b"null shape" in lib.smt_attn_last_error()


def _sigmas(count, n, prob):                               # scalars or arrays
    return np.abs(count - n * prob) / np.sqrt(n * prob * (1.0 - prob))


@pytest.mark.parametrize("B,H,S", SHAPES)
@pytest.mark.parametrize("p", RATES)
def test_keep_function_statistics(B, H, S, p):
    pe = threshold(p) / 256.0
    keep_p = 1.0 - pe
    agree_p = keep_p * keep_p + pe * pe                    # two independent elements agree
    causal = np.tril(np.ones((S, S), dtype=bool))
    n_vis = int(causal.sum())
    lag_k = causal[:, 1:] & causal[:, :-1]                 # (q, key) and (q, key + 1) both visible
    lag_q = causal[1:, :] & causal[:-1, :]
    row_n = np.arange(1, S + 1)                            # visible keys of row q
    col_n = np.arange(S, 0, -1)                            # visible rows of column key
    worst_agg, worst_marg = 0.0, 0.0
    for seed in SEEDS:
        m = keep_mask(B, H, S, p, seed).reshape(B * H, S, S)
        m1 = keep_mask(B, H, S, p, seed + 1).reshape(B * H, S, S)
        agg = [_sigmas(int((m & causal).sum()), B * H * n_vis, keep_p)]
        agg += [_sigmas(int((m[i] & causal).sum()), n_vis, keep_p) for i in range(B * H)]
        agg.append(_sigmas(int(((m[:, :, 1:] == m[:, :, :-1]) & lag_k).sum()), B * H * int(lag_k.sum()), agree_p))
        agg.append(_sigmas(int(((m[:, 1:, :] == m[:, :-1, :]) & lag_q).sum()), B * H * int(lag_q.sum()), agree_p))
        for i in range(B * H):
            for j in range(i + 1, B * H):
                agg.append(_sigmas(int(((m[i] == m[j]) & causal).sum()), n_vis, agree_p))
        agg.append(_sigmas(int(((m == m1) & causal).sum()), B * H * n_vis, agree_p))
        rows = (m & causal).sum(-1)                        # [BH, S] kept per row
        cols = (m & causal).sum(-2)
        marg = [_sigmas(rows[:, row_n >= 64], row_n[row_n >= 64][None, :], keep_p).max(),
                _sigmas(cols[:, col_n >= 64], col_n[col_n >= 64][None, :], keep_p).max()]
        print(f"seed {seed:#x} p {p} shape {(B, H, S)}: aggregates <= {max(agg):.2f} sigma, "
              f"marginals <= {max(marg):.2f} sigma")
        worst_agg, worst_marg = max(worst_agg, max(agg)), max(worst_marg, max(marg))
    assert worst_agg <= 5.0
    assert worst_marg <= 6.0


def test_keep_function_depends_on_nothing_else():
    # the same (seed, b, h, q, key) gives the same answer whatever S and B are
    a = keep_mask(1, 4, 64, 0.5, 99)
    b = keep_mask(2, 4, 200, 0.5, 99)
    assert np.array_equal(a[0], b[0, :, :64, :64])
    # the halves of the seed both matter, and a 64-bit seed is not truncated
    assert not np.array_equal(keep_mask(1, 1, 64, 0.5, 5), keep_mask(1, 1, 64, 0.5, 5 + 2 ** 32))
    assert not np.array_equal(keep_mask(1, 1, 64, 0.5, 5), keep_mask(1, 1, 64, 0.5, 6))
    # the threshold orders the masks: what p = 0.1 keeps ... p = 0.5 may drop, never the reverse
    lo, hi = keep_mask(1, 2, 128, 0.1, 3), keep_mask(1, 2, 128, 0.5, 3)
    assert not (hi & ~lo).any()
    assert keep_mask(1, 2, 128, 0.0, 3).all()
