"""References for the decode-linear kernel (include/smt_linear.h): helpers only, no tests.

Two bars, neither fitted to what a GPU returns.

The integer bar. x and W hold integers in [-4, 4] (x optionally scaled per row by a power of two, which
commutes with every operation). Every product and every partial sum is then an integer of magnitude at most
14336 * 16 = 229,376 < 2^24, hence exact in fp32 in ANY order, so the only rounding is the store's and the
kernel must be torch.equal to the int64 product converted to the dtype (round to nearest even). One element,
(M - 1, N - 1), is planted: its row of x and row of W are zero except 16 products 4 * 4 and one 3 * 1, the
sum 259. In bf16 that is a tie between 258 and 260 whose lower neighbour is odd, so rounding to nearest
even (260) and truncation (258) differ at every K.

The bound. For random normal data, per element against the fp64 product of the 16-bit inputs:

    UNIT[dtype] * |ref| + (1 + UNIT[dtype]) * (_acc(K) + KSPLIT * F32) * sum_k |x_k * w_k| + smallest subnormal

with the constants of tests/attn_ref.py: the store's rounding, an MFMA chain of K products (_acc), and the
KSPLIT fp32 additions that combine the K-slices (SMT_LINEAR_KSPLIT of the header), each of which rounds a
partial sum bounded by the sum of magnitudes.
"""
import numpy as np
import torch

from tests.attn_ref import F32, UNIT, _acc

KSPLIT = 8                          # SMT_LINEAR_KSPLIT (tests/test_decode_linear_host.py compares it with the header)
TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}        # smallest subnormal of the format


def int_inputs(M, N, K, dtype, seed, row_scale=False, ldx=None, ldw=None):
    """(x [M, K], W [N, K]) of ``dtype`` on the CPU with integer values in [-4, 4] and the planted element.
    ``row_scale``: row m of x is multiplied by 2^((m % 5) - 2). ``ldx`` / ``ldw``: return views of wider
    buffers with these row strides."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    w = torch.randint(-4, 5, (N, K), generator=g).double()
    x[M - 1] = 0
    w[N - 1] = 0
    x[M - 1, :16] = 4
    w[N - 1, :16] = 4
    x[M - 1, 16] = 3
    w[N - 1, 16] = 1
    if row_scale:
        x = x * (2.0 ** ((torch.arange(M) % 5) - 2).double())[:, None]
    return _strided(x.to(dtype), ldx), _strided(w.to(dtype), ldw)


def normal_inputs(M, N, K, dtype, seed, ldx=None, ldw=None):
    g = torch.Generator().manual_seed(seed)
    return (_strided(torch.randn(M, K, generator=g).to(dtype), ldx), _strided(torch.randn(N, K, generator=g).to(dtype), ldw))


def _strided(t, ld):
    if ld is None:
        return t
    buf = torch.zeros(t.shape[0], ld, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def exact(x, w, dtype=None):
    """The exact product of integer-valued inputs, converted once to the dtype (round to nearest even):
    int64 arithmetic on the values scaled to integers, so no floating-point sum is involved."""
    dtype = dtype or x.dtype
    xs = x.double() * 4.0                                   # the row scales are >= 2^-2: integers again
    assert torch.equal(xs, xs.round()) and torch.equal(w.double(), w.double().round())
    prod = xs.long() @ w.double().long().t()
    assert int(prod.abs().max()) < 2 ** 26
    return (prod.double() / 4.0).to(dtype)                  # exact in fp64 and in fp32: one rounding


def ref64_bound(x, w, dtype=None):
    """(fp64 reference, per-element bound) for 16-bit inputs x [M, K], W [N, K]."""
    dtype = dtype or x.dtype
    K = x.shape[1]
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    bound = UNIT[dtype] * ref.abs() + (1.0 + UNIT[dtype]) * (_acc(K) + KSPLIT * F32) * mag + TINY[dtype]
    return ref, bound


def truncate(y32, dtype):
    """fp32 -> dtype rounding toward zero (the wrong store the integer bar must catch)."""
    y = y32.to(dtype)
    over = y.float().abs() > y32.abs()
    bits = y.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)


def emulate(x, w, dtype=None, drop=None, trunc=False, ksplit=KSPLIT):
    """An fp32 numpy emulation of the kernel's reduction: the K / 32 steps are cut into ``ksplit``
    contiguous slices of ceil(steps / ksplit) steps, each slice accumulates its products in k order in
    fp32, and the slices' partials are added in slice order; one rounding to the dtype. ``drop`` =
    (m, n, k) leaves that product out; ``trunc`` truncates at the store."""
    dtype = dtype or x.dtype
    xf, wf = x.float().numpy(), w.float().numpy()
    M, K = xf.shape
    N = wf.shape[0]
    steps = K // 32
    per = -(-steps // ksplit)
    total = np.zeros((M, N), dtype=np.float32)
    for s in range(ksplit):
        part = np.zeros((M, N), dtype=np.float32)
        for k in range(min(K, s * per * 32), min(K, (s + 1) * per * 32)):
            p = xf[:, k, None] * wf[None, :, k]
            if drop is not None and drop[2] == k:
                p[drop[0], drop[1]] = 0.0
            part = part + p
        total = total + part
    y32 = torch.from_numpy(total)
    return truncate(y32, dtype) if trunc else y32.to(dtype)
