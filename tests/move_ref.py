"""Helpers of the exact tests for the movers, the accumulators and the selection scores
(``tests/test_move_ref_host.py``, ``tests/test_gpu_movers_exact.py``, ``tests/test_gpu_scores_exact.py``).

Three things live here, none of them a test:

* ``Frame``: an output window inside a sentinel-filled buffer, so that a write outside the window shows;
* the inputs: the whole 16-bit value domain as one 256x256 tile, fp32 bit patterns with the special
  values planted, and ``exact_grid``: fp32 values whose block and channel sums are exact in fp64 in
  any order, so that the expected scores are integers;
* independent references: plain indexing and int64 arithmetic, no call into the code under test.

Pure movers are compared on the integer view of the data (``torch.equal`` on int16 / int32), never as
floats: a float comparison cannot see a NaN payload or the sign of a zero.
"""
from __future__ import annotations

import functools

import torch

BLOCK = 256
TILE = BLOCK * BLOCK

_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
# finite as bf16 / fp16 / fp32 / fp64, not a repeated byte, never produced by a zero fill
SENTINEL = {2: 0x5A5B, 4: 0x5A5B5C5D, 8: 0x5A5B5C5D5E5F6061}
STRATEGIES = ("mean_abs", "abs_mean", "L1", "L2")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
class Frame:
    """A window of ``rows x cols`` elements of ``itemsize`` bytes inside a buffer filled with
    ``SENTINEL[itemsize]``: ``pad`` columns after each row, ``before`` / ``after`` guard rows and 16
    guard elements at both ends. The window's first byte is 16-byte aligned and so is every row
    (``ld * itemsize % 16 == 0``). With ``pad == 0`` the window is contiguous."""

    REGIONS = ("head", "rows before", "row padding", "rows after", "tail")

    def __init__(self, rows, cols, itemsize, pad=8, before=2, after=2, device="cpu"):
        self.rows, self.cols, self.itemsize, self.pad = int(rows), int(cols), itemsize, int(pad)
        self.before, self.after = before, after
        self.ld = self.cols + self.pad
        assert self.ld * itemsize % 16 == 0, f"row stride {self.ld} x {itemsize} B is not a multiple of 16 B"
        self.total = (before + self.rows + after) * self.ld
        self.off = 16
        self.flat = torch.full((self.total + 32,), SENTINEL[itemsize], dtype=_INT[itemsize], device=device)
        self.ints = self.flat[self.off:self.off + self.total].view(-1, self.ld)[before:before + self.rows, :self.cols]
        self.ptr = self.ints.data_ptr() if self.rows and self.cols else self.flat.data_ptr() + (
            self.off + before * self.ld) * itemsize
        assert self.ptr % 16 == 0

    def view(self, dtype: torch.dtype) -> torch.Tensor:
        """The window as a ``[rows, cols]`` tensor of a dtype of the same width (row stride ``ld``)."""
        assert torch.empty(0, dtype=dtype).element_size() == self.itemsize
        typed = self.flat.view(dtype)
        return typed[self.off:self.off + self.total].view(-1, self.ld)[self.before:self.before + self.rows, :self.cols]

    def fill(self, bits: torch.Tensor) -> "Frame":
        self.ints.copy_(bits.reshape(self.rows, self.cols).to(_INT[self.itemsize]))
        return self

    def bits(self) -> torch.Tensor:
        return self.ints.cpu().clone()

    def whole(self) -> torch.Tensor:
        """Every element of the buffer, guards included, on the CPU."""
        return self.flat.cpu().clone()

    def expected_whole(self, bits: torch.Tensor) -> torch.Tensor:
        """The buffer as it must look when the window holds ``bits`` and nothing else was written."""
        exp = torch.full((self.total + 32,), SENTINEL[self.itemsize], dtype=_INT[self.itemsize])
        win = exp[self.off:self.off + self.total].view(-1, self.ld)[self.before:self.before + self.rows, :self.cols]
        win.copy_(bits.reshape(self.rows, self.cols).to(_INT[self.itemsize]))
        return exp

    def region_of(self, i: int) -> str:
        if i < self.off:
            return "head"
        if i >= self.off + self.total:
            return "tail"
        r, c = divmod(i - self.off, self.ld)
        if r < self.before:
            return "rows before"
        if r >= self.before + self.rows:
            return "rows after"
        return "row padding" if c >= self.cols else "window"

    def damage(self):
        """None if every guard element still holds the sentinel, else a description of the first that
        does not."""
        flat = self.whole()
        win = flat[self.off:self.off + self.total].view(-1, self.ld)[self.before:self.before + self.rows, :self.cols]
        win.fill_(SENTINEL[self.itemsize])
        bad = (flat != SENTINEL[self.itemsize]).nonzero().flatten()
        if bad.numel() == 0:
            return None
        i = int(bad[0])
        return (f"{bad.numel()} guard element(s) overwritten; first at flat index {i} ({self.region_of(i)}): "
                f"{int(flat[i]):#x}")

    def check_intact(self) -> None:
        report = self.damage()
        assert report is None, report


def carve(sizes, itemsize, shift=0, guard=16):
    """Element offsets of ``len(sizes)`` windows inside one flat buffer: each 16-byte aligned plus
    ``shift`` elements, ``guard`` or more sentinel elements between neighbours and at both ends.
    Returns ``(offsets, total)``."""
    align = 16 // itemsize
    offs, at = [], guard
    for n in sizes:
        at = (at + align - 1) // align * align
        offs.append(at + shift)
        at += shift + int(n) + guard
    return offs, at + guard


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _domain16(seed: int) -> torch.Tensor:
    return (torch.randperm(65536, generator=_gen(seed)) - 32768).to(torch.int16).view(BLOCK, BLOCK)


def domain16(seed: int) -> torch.Tensor:
    """[256, 256] int16: every 16-bit pattern exactly once, in a seeded permutation. Viewed as bf16 or
    fp16 it is the whole value domain in one tile."""
    return _domain16(int(seed)).clone()


# +0, -0, +Inf, -Inf, a quiet and a signalling NaN with payload (both signs), the smallest and the
# largest subnormal (both signs), the largest finite value (both signs), the smallest normal, 1.0
SPECIALS32 = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC12345, 0x7F812345, 0xFF812345,
              0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x3F800000)


def _to_i32(v: int) -> int:
    return v - (1 << 32) if v >= (1 << 31) else v


def random_bits(shape, itemsize: int, seed: int) -> torch.Tensor:
    bits = 8 * itemsize
    return torch.randint(-(1 << (bits - 1)), 1 << (bits - 1), tuple(shape), generator=_gen(seed),
                         dtype=torch.int64).to(_INT[itemsize])


def patterns32(seed: int) -> torch.Tensor:
    """[256, 256] int32 of seeded random bit patterns with ``SPECIALS32`` planted at the start of the
    rows 0, 85, 170 and 255 (at a different phase of a 16-byte chunk in each)."""
    t = random_bits((BLOCK, BLOCK), 4, seed)
    sp = torch.tensor([_to_i32(v) for v in SPECIALS32], dtype=torch.int32)
    for i, r in enumerate((0, 85, 170, 255)):
        t[r, i:i + sp.numel()] = sp
    return t


def domain_tile(itemsize: int, seed: int) -> torch.Tensor:
    return domain16(seed) if itemsize == 2 else patterns32(seed)


def with_domain_prefix(bits: torch.Tensor, seed: int) -> torch.Tensor:
    """``bits`` with its first elements (row-major) replaced by the domain tile, as many as fit."""
    flat = bits.reshape(-1)
    dom = domain_tile(bits.element_size(), seed).reshape(-1)
    m = min(flat.numel(), dom.numel())
    flat[:m] = dom[:m]
    return bits


def weight_bits(rows: int, cols: int, itemsize: int, seed: int, domain_block=None) -> torch.Tensor:
    """[rows, cols] random bit patterns, the block ``domain_block = (r, c)`` holding the domain tile."""
    w = random_bits((rows, cols), itemsize, seed)
    if domain_block is not None:
        r, c = domain_block
        w[r * BLOCK:(r + 1) * BLOCK, c * BLOCK:(c + 1) * BLOCK] = domain_tile(itemsize, seed + 1)
    return w


def pick_columns(n_in: int, n_cols: int, seed: int) -> list:
    """``n_cols`` distinct columns of ``[0, n_in)`` in a seeded order, the first and the last column of
    x among them when there is room."""
    perm = torch.randperm(n_in, generator=_gen(seed))[:n_cols].tolist()
    for pos, must in ((0, n_in - 1), (n_cols - 1, 0)):
        if n_cols > pos >= 0 and must not in perm:
            perm[pos] = must
    assert len(set(perm)) == len(perm) and all(0 <= c < n_in for c in perm)
    return perm


def from_k(k: torch.Tensor) -> torch.Tensor:
    """fp32 ``k * 2^-10`` for int64 ``|k| < 2^14``, with the promises the exact sums rest on: the
    value is exact, and its fp32 square is a multiple of 2^-20 below 2^8."""
    assert k.dtype == torch.int64 and int(k.abs().max() if k.numel() else 0) < (1 << 14)
    x = (k.double() * 2.0 ** -10).float()
    assert torch.equal(x.double() * 1024.0, k.double())
    sq = (x * x).double() * 2.0 ** 20
    assert torch.equal(sq, sq.floor()) and (not sq.numel() or float(sq.max()) < 2.0 ** 28)
    return x


def exact_grid(shape, seed: int):
    """``(k, x)``: int64 ``k`` with ``|k| < 2^14`` and fp32 ``x = k * 2^-10``. Every term ``g`` or
    ``|g|`` is a multiple of 2^-10 below 16, so a sum of 65,536 of them needs at most 30 bits; the fp32
    square is a multiple of 2^-20 below 2^8, so such a sum needs at most 44 bits. Both are exact in
    fp64 whatever the order of the additions."""
    k = torch.randint(-(1 << 14) + 1, 1 << 14, tuple(shape), generator=_gen(seed), dtype=torch.int64)
    return k, from_k(k)


def l2_units(x: torch.Tensor) -> torch.Tensor:
    """int64 ``fp32(x * x) * 2^20``: the L2 term of the reference (``g.abs() ** 2`` in fp32)."""
    x = x.float()
    return ((x * x).double() * 2.0 ** 20).long()


def plant_blocks(k: torch.Tensor, zero=None, negative=None, corners=None) -> torch.Tensor:
    """In place on ``k [d1*256, d2*256]``: an all-zero block, an all-negative block, and a block that is
    zero except its elements (0, 0) and (255, 255)."""
    def blk(rc):
        r, c = rc
        return k[r * BLOCK:(r + 1) * BLOCK, c * BLOCK:(c + 1) * BLOCK]
    if zero is not None:
        blk(zero).zero_()
    if negative is not None:
        b = blk(negative)
        b.copy_(-b.abs() - 1)
        b.clamp_(min=-(1 << 14) + 1)
    if corners is not None:
        b = blk(corners)
        a, z = int(b[0, 0]) or 5, int(b[255, 255]) or -7
        b.zero_()
        b[0, 0], b[255, 255] = a, z
    return k


# ------------------------------------------------------------------------------------------------
# references: movers (any dtype, used on the integer views)
# ------------------------------------------------------------------------------------------------
def tiles_of(W: torch.Tensor, tiles) -> torch.Tensor:
    """[n*256, 256]: tile i is ``W[r_i*256 : +256, c_i*256 : +256]``."""
    out = torch.empty(len(tiles) * BLOCK, BLOCK, dtype=W.dtype)
    for i, (r, c) in enumerate(tiles):
        for m in range(BLOCK):
            out[i * BLOCK + m] = W[r * BLOCK + m, c * BLOCK:c * BLOCK + BLOCK]
    return out


def scatter_tiles(W: torch.Tensor, tiles, new: torch.Tensor) -> torch.Tensor:
    """A copy of W with ``W[r_i*256 : +256, c_i*256 : +256] = new[i*256 : +256]``."""
    W = W.clone()
    for i, (r, c) in enumerate(tiles):
        for m in range(BLOCK):
            W[r * BLOCK + m, c * BLOCK:c * BLOCK + BLOCK] = new[i * BLOCK + m]
    return W


def rows_of(W: torch.Tensor, index, n_cols: int) -> torch.Tensor:
    out = torch.empty(len(index), n_cols, dtype=W.dtype)
    for i, r in enumerate(index):
        out[i] = W[r, :n_cols]
    return out


def scatter_rows(W: torch.Tensor, index, rows: torch.Tensor, n_cols: int) -> torch.Tensor:
    W = W.clone()
    for i, r in enumerate(index):
        W[r, :n_cols] = rows[i, :n_cols]
    return W


def columns_of(x: torch.Tensor, cols, ld_out: int) -> torch.Tensor:
    """[T, ld_out]: ``out[:, j] = x[:, cols[j]]``, zero bits in the columns ``[len(cols), ld_out)``."""
    out = torch.zeros(x.shape[0], ld_out, dtype=x.dtype)
    for j, c in enumerate(cols):
        out[:, j] = x[:, c]
    return out


def colblocks_of(x: torch.Tensor, blocks) -> torch.Tensor:
    """[n_cb, T, 256]: ``out[j, t, k] = x[t, blocks[j]*256 + k]``."""
    out = torch.empty(len(blocks), x.shape[0], BLOCK, dtype=x.dtype)
    for j, b in enumerate(blocks):
        out[j] = x[:, b * BLOCK:(b + 1) * BLOCK]
    return out


def scatter_tiles_t(Wt: torch.Tensor, descs, flat: torch.Tensor) -> torch.Tensor:
    """A copy of ``Wt = W^T`` with ``Wt[c*256 + j, r*256 + k] = flat[flat_offset + k*256 + j]`` for every
    descriptor ``(live, r, c, flat_offset)`` that is live."""
    Wt = Wt.clone()
    for live, r, c, off in descs:
        if not live:
            continue
        tile = flat[off:off + TILE].view(BLOCK, BLOCK)
        for j in range(BLOCK):
            Wt[c * BLOCK + j, r * BLOCK:(r + 1) * BLOCK] = tile[:, j]
    return Wt


# ------------------------------------------------------------------------------------------------
# references: the two arithmetic kernels (torch CPU fp32 `=` / `+=`) and the NaN rule
# ------------------------------------------------------------------------------------------------
def accumulate(dst: torch.Tensor, src: torch.Tensor, assign: bool) -> torch.Tensor:
    """In place on the CPU fp32 ``dst``: ``dst = float(src)`` or ``dst += float(src)``."""
    assert dst.dtype == torch.float32 and dst.device.type == "cpu" and src.device.type == "cpu"
    if assign:
        dst.copy_(src.to(torch.float32))
    else:
        dst += src.to(torch.float32)
    return dst


def harvest(acc: torch.Tensor, x: torch.Tensor, assign: bool) -> torch.Tensor:
    """In place on the CPU fp32 ``acc``: ``acc = float(|x|)`` or ``acc += float(|x|)``."""
    return accumulate(acc, x.abs(), assign)


def nan_rule(got: torch.Tensor, want: torch.Tensor):
    """The comparison of the two arithmetic kernels: fp32 ``got`` equals ``want`` bit for bit wherever
    ``want`` is not a NaN, and is a NaN (any payload: an fp32 add may quiet a signalling NaN that the
    CPU's assignment keeps) wherever it is. Returns None, or a description of the first difference."""
    got, want = got.reshape(-1).float().cpu(), want.reshape(-1).float().cpu()
    assert got.shape == want.shape
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
    if bad.numel() == 0:
        return None
    i = int(bad[0])
    return (f"{bad.numel()} of {got.numel()} elements differ; first at {i}: got "
            f"{int(got.view(torch.int32)[i]) & 0xFFFFFFFF:#010x}, want {int(want.view(torch.int32)[i]) & 0xFFFFFFFF:#010x}")


# ------------------------------------------------------------------------------------------------
# references: scores in integer arithmetic
# ------------------------------------------------------------------------------------------------
def block_raw_exact(k: torch.Tensor, x: torch.Tensor, d1: int, d2: int, strategy: str) -> torch.Tensor:
    """fp64 ``[d1*d2, 2]``: per 256x256 block (row-major) the sum of the strategy's terms and the sum of
    their magnitudes, from int64 sums scaled once at the end."""
    if strategy == "mean_abs":
        t, m, scale = k, k.abs(), 2.0 ** -10
    elif strategy in ("abs_mean", "L1"):
        t, m, scale = k.abs(), k.abs(), 2.0 ** -10
    elif strategy == "L2":
        t = m = l2_units(x)
        scale = 2.0 ** -20
    else:
        raise ValueError(strategy)
    out = torch.empty(d1 * d2, 2, dtype=torch.float64)
    for bi in range(d1):
        for bj in range(d2):
            sl = (slice(bi * BLOCK, (bi + 1) * BLOCK), slice(bj * BLOCK, (bj + 1) * BLOCK))
            st, sm = int(t[sl].sum()), int(m[sl].sum())
            assert abs(st) < (1 << 53) and sm < (1 << 53)
            out[bi * d2 + bj, 0] = st * scale
            out[bi * d2 + bj, 1] = sm * scale
    return out


def channel_raw_exact(k: torch.Tensor, strategy: str) -> torch.Tensor:
    """fp64 ``[C]`` for an accumulator ``[B, S, C] = k * 2^-10``: ``sum_s A_s`` (``sum_s A_s^2`` for L2)
    with ``A_s = sum_b |k|``, in int64."""
    assert strategy in STRATEGIES
    A = k.abs().sum(0)
    tot, scale = ((A * A).sum(0), 2.0 ** -20) if strategy == "L2" else (A.sum(0), 2.0 ** -10)
    assert not tot.numel() or int(tot.max()) < (1 << 53)
    return tot.double() * scale


def find_entry(begins, blk: int, strict: bool = False) -> int:
    """The table lookup of the multi-tensor kernels: the last entry whose exclusive prefix is ``<= blk``
    (``strict``: ``< blk``, the mutation)."""
    lo, hi = 0, len(begins) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if (begins[mid] < blk) if strict else (begins[mid] <= blk):
            lo = mid
        else:
            hi = mid - 1
    return lo


# ------------------------------------------------------------------------------------------------
# the cases of the GPU tests (the host test proves on the same inputs that a wrong kernel shows)
# ------------------------------------------------------------------------------------------------
TILE_W = (512, 768)                                   # 2 x 3 blocks
TILE_LIST = [(1, 2), (0, 0), (1, 0), (0, 2)]
TILE_DOMAIN_BLOCK = (1, 2)
TILE_PAD = {2: 8, 4: 4}

ROW_COUNT = 6
ROW_INDEX = [5, 0, 3]
ROW_WIDTHS = {2: [8, 2048, 2056], 4: [4, 1024, 1028]}          # 16 B, 4096 B, 4112 B
ROW_PADS = {2: (8, 16), 4: (4, 8)}                             # (W pad, rows pad): ld_weight != ld_rows != n_cols
ROW_DOMAIN_WIDTH = 32768                                       # 16-bit: the rows 5 and 0 hold the whole domain

# (T, n_in, n_cols, ld_out)
COLUMN_CASES = [(5, 8192, 13, 256), (5, 8200, 13, 256), (3, 16384, 9, 256), (3, 16392, 9, 256), (4, 512, 0, 256),
                (1, 264, 264, 512),
                (256, 256, 256, 256)]                          # x is the domain tile, every column moved
COLUMN_CASES_FP32 = [(5, 1000, 37, 256), (3, 4100, 8, 256)]

# (T, in_f, blocks); the last one moves the whole domain (block 2 of x is the domain tile)
COLBLOCK_CASES = [(1, 768, [2]), (9, 768, [2, 0, 1]), (3, 1024, [3, 0, 3]), (256, 768, [2, 0, 1])]

# descriptors (live, r, c, flat_offset) of the transposed scatter: W [512, 768], W^T [768, 512]
SCATTER_T_DESCS = [(True, 1, 2, 2 * TILE), (False, 0, 1, 0), (True, 0, 0, 3 * TILE), (True, 1, 0, 1 * TILE)]

ACCUM_SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 65536]
ACCUM_SIZES_MID = [1, 7, 8, 9, 2047, 0, 2048, 2049, 4095, 4096, 4097, 65536]      # the empty entry in the middle
ACCUM_MISALIGNED = [9, 2049, 4097]

SCORE_GRIDS = [(1, 1), (2, 3), (3, 1)]
SCORE_LD_PAD = 4                                      # the (2, 3) gradient is a view with ld = 768 + 4
CHANNEL_B, CHANNEL_S, CHANNEL_C = (1, 3), (1, 32, 33, 70), 264


def tile_case(itemsize: int):
    return weight_bits(TILE_W[0], TILE_W[1], itemsize, 100 + itemsize, TILE_DOMAIN_BLOCK)


def row_case(itemsize: int, n_cols: int):
    w = random_bits((ROW_COUNT, n_cols), itemsize, 200 + itemsize)
    if n_cols == ROW_DOMAIN_WIDTH and itemsize == 2:
        dom = domain16(201).reshape(2, ROW_DOMAIN_WIDTH)
        w[5], w[0] = dom[0], dom[1]
    else:
        with_domain_prefix(w, 201)
    return w


def column_case(T: int, n_in: int, n_cols: int, itemsize: int = 2):
    x = with_domain_prefix(random_bits((T, n_in), itemsize, 300 + n_in), 301)
    return x, pick_columns(n_in, n_cols, 302 + n_in)


def colblock_case(T: int, in_f: int):
    x = random_bits((T, in_f), 2, 400 + T)
    if T == BLOCK:
        x[:, 2 * BLOCK:3 * BLOCK] = domain16(401)
    else:
        with_domain_prefix(x, 401)
    return x


def scatter_t_case():
    """(Wt bits [768, 512], flat source [4 * 65536]); the first descriptor's tile is the domain tile."""
    Wt = random_bits((TILE_W[1], TILE_W[0]), 2, 500)
    flat = random_bits((4 * TILE,), 2, 501)
    flat[2 * TILE:3 * TILE] = domain16(502).reshape(-1)
    return Wt, flat


def accum_source(n: int, itemsize: int, launch: int) -> torch.Tensor:
    """Source bits of one entry for launch 0 (assign), 1 and 2 (add): the 65,536-element entry is the
    domain tile in the first two launches; everything else, and the third launch, is Gaussian data
    (so that the additions also meet ordinary roundings), as bits of the source format."""
    if n == TILE and launch < 2:
        return domain_tile(itemsize, 600 + launch).reshape(-1)
    return random_bits((n,), itemsize, 610 + 7 * launch + n % 1000)


def accum_gaussian(n: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    g = torch.randn(n, generator=_gen(seed)) * torch.exp(2.0 * torch.randn(n, generator=_gen(seed + 1)))
    return g.to(dtype)


def score_case(seed: int = 700):
    """The three gradients of the block-score tests as ``[(k, x, (d1, d2)), ...]``, with the planted
    blocks: in the (2, 3) one an all-zero block (0, 0), an all-negative block (0, 1) and a block (1, 2)
    that is zero except two corners; one -0.0 in the (3, 1) one."""
    out = []
    for i, (d1, d2) in enumerate(SCORE_GRIDS):
        k, _ = exact_grid((d1 * BLOCK, d2 * BLOCK), seed + i)
        if (d1, d2) == (2, 3):
            plant_blocks(k, zero=(0, 0), negative=(0, 1), corners=(1, 2))
        x = from_k(k)
        if (d1, d2) == (3, 1):
            k[300, 17] = 0
            x = from_k(k)
            x[300, 17] = -0.0
        out.append((k, x, (d1, d2)))
    return out


def channel_case(B: int, S: int, C: int = CHANNEL_C):
    return exact_grid((B, S, C), 800 + 10 * B + S)
