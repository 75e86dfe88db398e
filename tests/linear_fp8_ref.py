"""References for the e4m3 decode-linear kernel (smt_linear_skinny_fp8, include/smt_linear.h): helpers only.

The contract, per element:

    y[m][n] = RN_out( RN32( acc[m][n] * RN32(sx[m] * sw[n]) ) ),   acc = sum_k dec(x8[m][k]) * dec(w8[n][k])  in fp32

Bytes are decoded with tests/fp8_ref.py's e4m3_decode and built with its e4m3_encode, never with torch's
converter. Two bars, neither fitted to what a GPU returns.

The integer bar. x8 and w8 hold integers in [-4, 4] (all of them e4m3 values). Every product and every partial
sum is an integer of magnitude at most 14336 * 16 = 229,376 < 2^24, and the products inside one instruction
span 2^0 .. 2^4, far inside the 13 bits the e4m3 MFMA keeps below its largest product, so acc is
exact in ANY order. The scales are not powers of two, so the two scale multiplications do round: the reference
makes them in numpy float32 in the order of the contract and rounds once to the dtype, and the kernel must be
torch.equal to it. One element, (M - 1, N - 1), is linear_ref's planted tie: its rows are zero except 16
products 4 * 4 and one 3 * 1, the sum 259, with sx[M - 1] = sw[N - 1] = 1; in bf16 that is a tie between 258
and 260 that round-to-nearest-even (260) and truncation (258) resolve differently.

The bound. For inputs quantised from random normal data, per element against the fp64 product of the decoded
bytes and the scales, three terms:

    UNIT[dtype] * |ref|
  + (1 + UNIT[dtype]) * (_acc(K) + (KSPLIT + 2) * F32) * sx sw sum_k |a_k b_k|      (linear_ref's, with two more
                                                                                      fp32 operations: the scales)
  + (1 + UNIT[dtype]) * sx sw sum_k [p_k < 2^(emax - 6)] min(p_k, 2^(emax - 13))    (as
                                                                                      tests/test_gpu_fp8_exact.py
                                                                                      takes it)
  + the smallest subnormal of the dtype

where p_k = |a_k b_k| and emax = floor(log2 max_k p_k): inside one instruction the products are aligned to the
largest one and what lies below 2^(e - 13) is dropped; a product of two 4-bit significands has at most 7
significant bits, so only one more than 6 binades below the largest can lose anything.
"""
import numpy as np
import torch

from tests import fp8_ref as R
from tests.attn_ref import F32, UNIT, _acc
from tests.linear_ref import KSPLIT, TINY, truncate

KSTEP = 64                          # K-elements of one step (two 16x16x32 instructions)
ALIGN_BITS = 13                     # tests/test_gpu_fp8_exact.py's ALIGN_BITS

KS = (64, 512, 576, 4160)           # one step and seven idle waves; one step a wave; uneven slices with the trailing
                                    # waves empty; a full batch plus a partial one in wave 0's slice
NS = (16, 48)
MS = (1, 5, 16)
K_LONG = 14336                      # at N = 16 only: the longest chain, the integer ceiling
# (M, N, K, pad): pad bytes added to ldx and ldw, pad elements to ldy
CASES = [(M, N, K, 0) for K in KS for N in NS for M in MS] + [(M, 16, K_LONG, 0) for M in MS] + \
        [(5, 48, 576, 16), (16, 16, 64, 32)]


def _strided(a: np.ndarray, ld):
    """``a`` as a view of a zero-filled buffer with row stride ``ld``."""
    if ld is None:
        return a
    buf = np.zeros((a.shape[0], ld), dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


def _scales(n, rng, last_one=True):
    """fp32 scales that are not powers of two, between 2^-7 and 2^-1; the last one is 1 (the planted element's)."""
    s = (rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-7, -1, n))).astype(np.float32)
    if last_one:
        s[-1] = 1.0
    return s


def int_inputs(M, N, K, seed, ldx=None, ldw=None):
    """``(x8 [M, K] uint8, sx [M] float32, w8 [N, K] uint8, sw [N] float32)`` as numpy arrays: integer values
    in [-4, 4] encoded as e4m3, the planted element at (M - 1, N - 1), scales that are not powers of two."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (M, K)).astype(np.float32)
    w = rng.integers(-4, 5, (N, K)).astype(np.float32)
    x[M - 1] = 0
    w[N - 1] = 0
    x[M - 1, :16] = 4
    w[N - 1, :16] = 4
    x[M - 1, 16] = 3
    w[N - 1, 16] = 1
    x8, w8 = R.e4m3_encode(x), R.e4m3_encode(w)
    assert np.array_equal(R.e4m3_decode(x8), x) and np.array_equal(R.e4m3_decode(w8), w)
    return _strided(x8, ldx), _scales(M, rng), _strided(w8, ldw), _scales(N, rng)


def normal_bf16(M, N, K, seed):
    """bf16 ``(x [M, K], W [N, K])`` (CPU) of random normal data, the rows at different magnitudes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.arange(M) % 5 - 2.0)[:, None]
    w = torch.randn(N, K, generator=g) * 0.05
    return x.bfloat16(), w.bfloat16()


def quant_host(t: torch.Tensor, ld=None):
    """``(bytes, scales)`` of the bf16 rows of ``t`` by the CPU restatement of smt_quant_rows_e4m3
    (tests/fp8_ref.py), which tests/test_gpu_fp8_exact.py holds the kernel to, bit for bit."""
    q, s = R.quant_rows(R.bf16_bits(t))
    return _strided(q, ld), s


def exact(x8, sx, w8, sw, dtype):
    """The integer bar: int64 product of the decoded values, then the contract's two float32 multiplications
    in numpy float32, then one rounding to the dtype."""
    a, b = R.e4m3_decode(x8), R.e4m3_decode(w8)
    assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))
    acc = a.astype(np.int64) @ b.astype(np.int64).T
    assert int(np.abs(acc).max()) < 2 ** 24
    s = np.asarray(sx, dtype=np.float32)[:, None] * np.asarray(sw, dtype=np.float32)[None, :]
    assert s.dtype == np.float32
    v = acc.astype(np.float32) * s
    assert v.dtype == np.float32
    return torch.from_numpy(v).to(dtype)


def ref64_bound(x8, sx, w8, sw, dtype):
    """(fp64 reference, per-element bound) as torch tensors; see the module docstring."""
    a, b = R.e4m3_decode(x8), R.e4m3_decode(w8)
    K = a.shape[1]
    ss = np.asarray(sx, dtype=np.float64)[:, None] * np.asarray(sw, dtype=np.float64)[None, :]
    ref = (a @ b.T) * ss
    mag = (np.abs(a) @ np.abs(b).T) * ss
    align = np.empty_like(ref)
    for i in range(a.shape[0]):
        p = np.abs(a[i][None, :] * b)                                           # [N, K], exact
        emax = np.floor(np.log2(np.maximum(p.max(axis=1, keepdims=True), 2.0 ** -60)))
        cut = np.exp2(emax - ALIGN_BITS)
        lossy = p < np.exp2(emax - ALIGN_BITS + 7)
        align[i] = (np.minimum(p, cut) * lossy).sum(axis=1)
    u = UNIT[dtype]
    bound = u * np.abs(ref) + (1.0 + u) * ((_acc(K) + (KSPLIT + 2) * F32) * mag + align * ss) + TINY[dtype]
    return torch.from_numpy(ref), torch.from_numpy(bound)


def emulate(x8, sx, w8, sw, dtype, drop=None, wrong_sx=False, wrong_sw=False, scale_after_round=False, trunc=False,
            swap_rows=False, ksplit=KSPLIT):
    """An fp32 numpy emulation of the kernel: the K / 64 steps are cut into ``ksplit`` contiguous slices of
    ceil(steps / ksplit) steps, each slice accumulates its products in k order in fp32, the partials are added
    in slice order, and the sum is multiplied by RN32(sx * sw) and rounded once. The mutants: ``drop`` =
    (m, n, k) leaves that product out; ``wrong_sx`` / ``wrong_sw`` index the scales by the next row / feature;
    ``scale_after_round`` rounds the accumulator to the dtype before the scales and again after; ``trunc``
    truncates at the store; ``swap_rows`` exchanges rows 0 and M - 1 of the result."""
    a = R.e4m3_decode(x8).astype(np.float32)
    b = R.e4m3_decode(w8).astype(np.float32)
    M, K = a.shape
    N = b.shape[0]
    steps = K // KSTEP
    per = -(-steps // ksplit)
    total = np.zeros((M, N), dtype=np.float32)
    for s in range(ksplit):
        k0, k1 = min(K, s * per * KSTEP), min(K, (s + 1) * per * KSTEP)
        if k0 == k1:
            continue
        p = a[:, None, k0:k1] * b[None, :, k0:k1]                                # exact: two 4-bit significands
        if drop is not None and k0 <= drop[2] < k1:
            p[drop[0], drop[1], drop[2] - k0] = 0.0
        total = total + np.cumsum(p, axis=2, dtype=np.float32)[:, :, -1]         # sequential fp32 adds in k order
    sx, sw = np.asarray(sx, dtype=np.float32), np.asarray(sw, dtype=np.float32)
    if wrong_sx:
        sx = np.roll(sx, -1)
    if wrong_sw:
        sw = np.roll(sw, -1)
    if scale_after_round:
        total = torch.from_numpy(total).to(dtype).float().numpy()
    v = torch.from_numpy(total * (sx[:, None] * sw[None, :]))
    y = truncate(v, dtype) if trunc else v.to(dtype)
    if swap_rows:
        y = y.clone()
        y[[0, M - 1]] = y[[M - 1, 0]]
    return y


MUTANTS = ({"drop": "planted"}, {"wrong_sx": True}, {"wrong_sw": True}, {"scale_after_round": True}, {"trunc": True},
           {"swap_rows": True})


def mutant_kwargs(mut: dict, M, N):
    """The keyword arguments of :func:`emulate` for a mutant; the dropped product is the planted element's 3 * 1."""
    return {k: ((M - 1, N - 1, 16) if v == "planted" else v) for k, v in mut.items()}


def within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> bool:
    return bool(((got.double() - ref).abs() <= bound).all()) and bool(torch.isfinite(got.float()).all())
