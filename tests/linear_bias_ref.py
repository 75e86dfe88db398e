"""References for the bias epilogue of the decode-linear kernel (smt_linear_skinny_bias, include/smt_linear.h):
helpers only, no tests. They extend tests/linear_ref.py, whose two bars they keep.

The integer bar. x, W and b hold integers, x and W in [-4, 4], b in [-9, 9] apart from the planted ones, so
|acc + b| <= 14336 * 16 + 9 < 2^24: every partial sum, the sum of the partials and the sum with the bias are exact
in fp32 in any order, the store's rounding is the only one, and the kernel must be torch.equal to the int64 sum
converted once to the dtype. Row M - 1 of x is 4 in its first 16 places, 1 in the 17th and 0 elsewhere, and two
rows of every W are planted against it:

  - feature N - 1: 16 products 4 * 4 and one 1 * 1, acc = 257, with b = 1. One rounding gives 258 in bf16.
    Rounding acc first gives 256 (the tie 257 goes to the even neighbour), then 256 + 1 = 257 rounds to 256
    again: a kernel that rounds before it adds the bias returns 256.
  - feature 0: 16 products 4 * 4 and one 1 * 3, acc = 259, with b = 4: 263 is in bf16 a tie between 262 and 264
    whose lower neighbour is odd, so rounding to nearest even (264) and truncation (262) differ.

An output without a bias keeps b = None and its planted elements are 257 -> 256 and 259 -> 260.

The bound. For normal data, per element against the fp64 value x . w + b of the 16-bit inputs:

    UNIT * |ref| + (1 + UNIT) * (_acc(K) + (KSPLIT + 1) * F32) * (sum_k |x_k * w_k| + |b|) + smallest subnormal

linear_ref's bound with one more fp32 operation, the bias add, whose result is bounded by the magnitude sum
with |b| added.
"""
import torch

from tests import linear_ref as lr
from tests.attn_ref import F32, UNIT, _acc

KSPLIT = lr.KSPLIT
BIAS_SPAN = 9


def int_inputs(M, Ns, K, dtype, seed, biased=None):
    """(x [M, K], [W_i [N_i, K]], [b_i [N_i] or None]) of ``dtype`` on the CPU with integer values and the
    planted elements. ``biased``: per output, whether it has a bias (default: all)."""
    assert K >= 32 and all(N >= 16 for N in Ns)
    biased = [True] * len(Ns) if biased is None else list(biased)
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    x[M - 1] = 0
    x[M - 1, :16] = 4
    x[M - 1, 16] = 1
    ws, bs = [], []
    for N, has in zip(Ns, biased):
        w = torch.randint(-4, 5, (N, K), generator=g).double()
        b = torch.randint(-BIAS_SPAN, BIAS_SPAN + 1, (N,), generator=g).double()
        for n, last, bias in ((N - 1, 1, 1), (0, 3, 4)):
            w[n] = 0
            w[n, :16] = 4
            w[n, 16] = last
            b[n] = bias
        ws.append(w.to(dtype))
        bs.append(b.to(dtype) if has else None)
    return x.to(dtype), ws, bs


def normal_inputs(M, Ns, K, dtype, seed, biased=None):
    biased = [True] * len(Ns) if biased is None else list(biased)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    ws = [torch.randn(N, K, generator=g).to(dtype) for N in Ns]
    bs = [(4.0 * torch.randn(N, generator=g)).to(dtype) if has else None for N, has in zip(Ns, biased)]
    return x, ws, bs


def exact(x, w, b=None, dtype=None):
    """The exact value of integer inputs, int64 arithmetic, converted once to the dtype (round to nearest even)."""
    dtype = dtype or x.dtype
    for t in (x, w) + (() if b is None else (b,)):
        assert torch.equal(t.double(), t.double().round())
    total = x.double().long() @ w.double().long().t()
    if b is not None:
        total = total + b.double().long()[None, :]
    assert int(total.abs().max()) < 2 ** 24
    return total.double().to(dtype)


def ref64_bound(x, w, b=None, dtype=None):
    """(fp64 reference, per-element bound) for 16-bit x [M, K], W [N, K] and b [N] or None."""
    if b is None:
        return lr.ref64_bound(x, w, dtype)
    dtype = dtype or x.dtype
    K = x.shape[1]
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = xd @ wd.t() + bd[None, :]
    mag = xd.abs() @ wd.abs().t() + bd.abs()[None, :]
    bound = UNIT[dtype] * ref.abs() + (1.0 + UNIT[dtype]) * (_acc(K) + (KSPLIT + 1) * F32) * mag + lr.TINY[dtype]
    return ref, bound


def emulate(x, w, b=None, dtype=None, mutant=None, other=None):
    """An fp32 emulation of the kernel: linear_ref's 8-way split summed in slice order, one fp32 add of
    ``(float) b[n]``, one rounding to the dtype. ``mutant`` builds a wrong kernel instead:

      "dropped"         the bias is left out
      "other"           ``other``'s first N entries are added in place of b (another output's bias)
      "by_row"          b is indexed by the row, b[m % N]
      "after_rounding"  the accumulator is rounded to the dtype first, the bias added then, and the sum rounded again
      "truncate"        the store truncates
    """
    dtype = dtype or x.dtype
    acc = lr.emulate(x, w, dtype=torch.float32)             # the fp32 sum of the partials, unrounded
    if b is None:
        return lr.truncate(acc, dtype) if mutant == "truncate" else acc.to(dtype)
    M, N = acc.shape
    bf = b.float()
    if mutant == "dropped":
        return acc.to(dtype)
    if mutant == "other":
        return (acc + other.float()[:N][None, :]).to(dtype)
    if mutant == "by_row":
        return (acc + bf[torch.arange(M) % N][:, None]).to(dtype)
    if mutant == "after_rounding":
        return (acc.to(dtype).float() + bf[None, :]).to(dtype)
    total = acc + bf[None, :]
    if mutant == "truncate":
        return lr.truncate(total, dtype)
    assert mutant is None, mutant
    return total.to(dtype)
