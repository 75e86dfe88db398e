"""Bit-exact, framed tests of the kernels that move weights and activations and of the warm-up
accumulation: ``tile_copy_kernel``, ``row_copy_kernel``, ``column_gather_kernel`` /
``column_gather_dma_kernel``, ``colblock_gather_kernel``, ``tile_scatter_t_kernel`` and
``grad_accumulate_kernel`` of ``csrc/smt_kernels.hip``.

Every call goes through the C ABI with ctypes, so that each output sits in a ``move_ref.Frame``: a
window of a sentinel-filled buffer whose every other element must still hold the sentinel afterwards.
The data are bit patterns (the whole 16-bit domain, fp32 patterns with NaN payloads, -0.0, infinities
and subnormals) and are compared as integers. Each kernel is also called once through its ``_hip``
wrapper. The shapes are the smallest that reach each dispatch edge; ``tests/test_move_ref_host.py``
shows on the CPU that these inputs see a wrong kernel."""
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from tests import move_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = M.BLOCK
_INT = {2: torch.int16, 4: torch.int32}
_ITEM = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _lib():
    return _hip.load()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _ok(rc, what):
    assert rc == 0, f"{what}: status {rc}: {_lib().smt_last_error().decode(errors='replace')}"
    torch.cuda.synchronize()


def _frame(rows, cols, itemsize, pad):
    return M.Frame(rows, cols, itemsize, pad=pad, device=DEV)


def _same(got: torch.Tensor, want: torch.Tensor, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; first at {i}: "
                             f"got {int(got[i]):#x}, want {int(want[i]):#x}")


def _framed(frame: M.Frame, want_bits: torch.Tensor, what: str):
    """Every element of the framed buffer: the window equals ``want_bits`` and the guards are intact."""
    frame.check_intact()
    _same(frame.whole(), frame.expected_whole(want_bits), what)


# ----------------------------------------------------------------------------- tile gather / scatter
@pytest.mark.parametrize("n_tiles", [4, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_gather_and_scatter(dtype, n_tiles):
    item = _ITEM[dtype]
    tiles = M.TILE_LIST[:n_tiles]
    Wb = M.tile_case(item)
    W = _frame(M.TILE_W[0], M.TILE_W[1], item, M.TILE_PAD[item]).fill(Wb.to(DEV))
    assert W.ld != M.TILE_W[1]
    rc_tab = _hip.tile_table(tiles, torch.device(DEV))
    out = _frame(n_tiles * B, B, item, 0)
    before = W.whole()
    _ok(_lib().smt_tile_gather(W.ptr, W.ld, item, rc_tab.data_ptr(), n_tiles, out.ptr, _stream()), "smt_tile_gather")
    _framed(out, M.tiles_of(Wb, tiles), "gathered tiles")
    _same(W.whole(), before, "W after a gather")

    new = M.random_bits((n_tiles * B, B), item, 31)
    new[:B] = M.domain_tile(item, 32)
    src = _frame(n_tiles * B, B, item, 0).fill(new.to(DEV))
    _ok(_lib().smt_tile_scatter(W.ptr, W.ld, item, rc_tab.data_ptr(), n_tiles, src.ptr, _stream()), "smt_tile_scatter")
    _framed(W, M.scatter_tiles(Wb, tiles, new), "W after a scatter (unselected blocks and pads included)")
    _framed(src, new, "source tiles after a scatter")

    # once through the wrappers, on the same strided W
    got = _hip.tile_gather(W.view(dtype), rc_tab, torch.empty(n_tiles * B, B, dtype=dtype, device=DEV))
    _same(got.view(_INT[item]).cpu(), new, "_hip.tile_gather of the scattered tiles")
    back = M.tiles_of(Wb, tiles)
    _hip.tile_scatter(W.view(dtype), rc_tab, back.to(DEV).view(dtype))
    torch.cuda.synchronize()
    _framed(W, Wb, "W after _hip.tile_scatter of its first tiles")


# ----------------------------------------------------------------------------- row gather / scatter
def _row_widths():
    cases = [(dt, n) for dt in DTYPES for n in M.ROW_WIDTHS[_ITEM[dt]]]
    return cases + [(torch.bfloat16, M.ROW_DOMAIN_WIDTH)]


@pytest.mark.parametrize("dtype,n_cols", _row_widths())
def test_row_gather_and_scatter(dtype, n_cols):
    item = _ITEM[dtype]
    pad_w, pad_r = M.ROW_PADS[item]
    Wb = M.row_case(item, n_cols)
    W = _frame(M.ROW_COUNT, n_cols, item, pad_w).fill(Wb.to(DEV))
    rows = _frame(len(M.ROW_INDEX), n_cols, item, pad_r)
    assert len({W.ld, rows.ld, n_cols}) == 3
    idx = _hip.index_table(M.ROW_INDEX, torch.device(DEV))
    n = len(M.ROW_INDEX)
    _ok(_lib().smt_row_gather(W.ptr, W.ld, item, n_cols, idx.data_ptr(), n, rows.ptr, rows.ld, _stream()), "smt_row_gather")
    _framed(rows, M.rows_of(Wb, M.ROW_INDEX, n_cols), "gathered rows")
    _framed(W, Wb, "W after a row gather")

    new = M.with_domain_prefix(M.random_bits((n, n_cols), item, 33), 34)
    rows.fill(new.to(DEV))
    _ok(_lib().smt_row_scatter(W.ptr, W.ld, item, n_cols, idx.data_ptr(), n, rows.ptr, rows.ld, _stream()), "smt_row_scatter")
    want = M.scatter_rows(Wb, M.ROW_INDEX, new, n_cols)
    _framed(W, want, "W after a row scatter")
    _framed(rows, new, "rows after a row scatter")

    got = _hip.row_gather(W.view(dtype), idx, torch.empty(n, n_cols, dtype=dtype, device=DEV))
    _same(got.view(_INT[item]).cpu(), new, "_hip.row_gather")
    _hip.row_scatter(W.view(dtype), idx, M.rows_of(Wb, M.ROW_INDEX, n_cols).to(DEV).view(dtype))
    torch.cuda.synchronize()
    _framed(W, Wb, "W after _hip.row_scatter of its first rows")


# ----------------------------------------------------------------------------- column gather
@pytest.mark.parametrize("T,n_in,n_cols,ld_out", M.COLUMN_CASES)
def test_column_gather_16bit(T, n_in, n_cols, ld_out):
    xb, cols = M.column_case(T, n_in, n_cols)
    x = _frame(T, n_in, 2, 8).fill(xb.to(DEV))
    out = _frame(T, ld_out, 2, 0)                                 # the kernel owns all ld_out columns of a row
    tab = _hip.index_table(cols, torch.device(DEV)) if n_cols else None
    _ok(_lib().smt_column_gather(x.ptr, x.ld, n_in, T, tab.data_ptr() if n_cols else None, n_cols, out.ptr, ld_out,
                                 _stream()), "smt_column_gather")
    want = M.columns_of(xb, cols, ld_out)
    assert not want[:, n_cols:].any()
    _framed(out, want, f"gathered columns ({n_cols} of {n_in}, zero padding to {ld_out})")
    _framed(x, xb, "x after a column gather")
    if n_cols:
        got = _hip.column_gather(x.view(torch.float16), tab, n_cols, ld_out)
        _same(got.view(torch.int16).cpu(), want, "_hip.column_gather")


@pytest.mark.parametrize("T,n_in,n_cols,ld_out", M.COLUMN_CASES_FP32)
def test_column_gather_fp32_route(T, n_in, n_cols, ld_out):
    """fp32 columns as the 16-bit column pairs (2c, 2c + 1): only ``_hip.column_gather`` builds them."""
    xb, cols = M.column_case(T, n_in, n_cols, itemsize=4)
    sp = torch.tensor([M._to_i32(v) for v in M.SPECIALS32], dtype=torch.int32)
    xb[T - 1, cols[:sp.numel()]] = sp[:min(n_cols, sp.numel())]          # the special values in gathered columns
    x = _frame(T, n_in, 4, 4).fill(xb.to(DEV))
    tab = _hip.index_table(cols, torch.device(DEV))
    got = _hip.column_gather(x.view(torch.float32), tab, n_cols, ld_out)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, ld_out)
    _same(got.view(torch.int32).cpu(), M.columns_of(xb, cols, ld_out), "fp32 column gather")
    _framed(x, xb, "x after an fp32 column gather")


# ----------------------------------------------------------------------------- column-block gather
@pytest.mark.parametrize("T,in_f,blocks", M.COLBLOCK_CASES)
def test_colblock_gather(T, in_f, blocks):
    xb = M.colblock_case(T, in_f)
    x = _frame(T, in_f, 2, 8).fill(xb.to(DEV))
    assert x.ld == in_f + 8
    out = _frame(len(blocks) * T, B, 2, 0)
    tab = _hip.index_table(blocks, torch.device(DEV))
    _ok(_lib().smt_colblock_gather(x.ptr, x.ld, T, tab.data_ptr(), len(blocks), out.ptr, _stream()), "smt_colblock_gather")
    want = M.colblocks_of(xb, blocks)
    _framed(out, want, "gathered column blocks [n_cb, T, 256]")
    _framed(x, xb, "x after a column-block gather")
    got = _hip.colblock_gather(x.view(torch.bfloat16), tab)
    assert tuple(got.shape) == (len(blocks), T, B)
    _same(got.view(torch.int16).cpu(), want, "_hip.colblock_gather")


# ----------------------------------------------------------------------------- transposed tile scatter
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_tile_scatter_transposed(dtype):
    Wtb, flatb = M.scatter_t_case()
    Wt = _frame(M.TILE_W[1], M.TILE_W[0], 2, 8).fill(Wtb.to(DEV))
    assert Wt.ld == 520
    flat = _frame(1, 4 * M.TILE, 2, 0).fill(flatb.to(DEV))
    entries = [(Wt.view(dtype) if live else None, r, c, off) for live, r, c, off in M.SCATTER_T_DESCS]
    assert entries[1][0] is None and [e[3] // M.TILE for e in entries] == [2, 0, 3, 1]
    descs = _hip.tile_descs(entries, torch.device(DEV), dtype)
    _ok(_lib().smt_tile_scatter_t(descs.data_ptr(), len(entries), flat.ptr, _stream()), "smt_tile_scatter_t")
    want = M.scatter_tiles_t(Wtb, M.SCATTER_T_DESCS, flatb)
    _framed(Wt, want, "W^T after the transposed scatter (the NULL-weight descriptor skipped)")
    _framed(flat, flatb, "the flat source after the transposed scatter")

    Wt.fill(Wtb.to(DEV))                                          # and through the wrapper
    _hip.tile_scatter_t(descs, len(entries), flat.view(dtype).reshape(-1))
    torch.cuda.synchronize()
    _framed(Wt, want, "W^T after _hip.tile_scatter_t")


# ----------------------------------------------------------------------------- warm-up accumulation
_CODE = {torch.bfloat16: _hip.DTYPE_BF16, torch.float16: _hip.DTYPE_FP16, torch.float32: _hip.DTYPE_FP32}


class _Pool:
    """Windows carved from one flat sentinel-filled device buffer, with its CPU mirror."""

    def __init__(self, sizes, itemsize, shift=0):
        self.sizes, self.itemsize = list(sizes), itemsize
        self.offs, total = M.carve(sizes, itemsize, shift)
        self.host = torch.full((total,), M.SENTINEL[itemsize], dtype=_INT[itemsize])
        self.dev = self.host.to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def put(self, i, bits):
        self.host[self.offs[i]:self.offs[i] + self.sizes[i]] = bits
        self.dev[self.offs[i]:self.offs[i] + self.sizes[i]] = bits.to(DEV)

    def win(self, i):
        return self.host[self.offs[i]:self.offs[i] + self.sizes[i]]

    def ptr(self, i):
        return self.dev.data_ptr() + self.offs[i] * self.itemsize


def _launch_accumulate(dst: _Pool, srcs, assigns):
    """One launch: entry i adds (or assigns) ``srcs[i] = (pool, index, dtype)`` into window i of dst."""
    entries, chunk = [], 0
    for i, ((pool, j, dtype), assign) in enumerate(zip(srcs, assigns)):
        n = dst.sizes[i]
        assert pool.sizes[j] == n
        entries.append(_hip.AccumEntry(pool.ptr(j), dst.ptr(i), n, chunk, _CODE[dtype], int(assign)))
        chunk += (n + _hip.ACC_CHUNK - 1) // _hip.ACC_CHUNK
    table = _hip._device_table(entries, _hip.AccumEntry, torch.device(DEV))
    _ok(_lib().smt_grad_accumulate(table.data_ptr(), len(entries), chunk, _stream()), "smt_grad_accumulate")
    for i, ((pool, j, dtype), assign) in enumerate(zip(srcs, assigns)):        # the CPU `=` / `+=`
        M.accumulate(dst.win(i).view(torch.float32), pool.win(j).view(dtype), bool(assign))


def _check_pool(dst: _Pool, what):
    """Guards bit for bit, windows under the NaN rule."""
    got = dst.dev.cpu()
    mask = torch.ones_like(got, dtype=torch.bool)
    for i, n in enumerate(dst.sizes):
        mask[dst.offs[i]:dst.offs[i] + n] = False
        report = M.nan_rule(got[dst.offs[i]:dst.offs[i] + n].view(torch.float32), dst.win(i).view(torch.float32))
        assert report is None, f"{what}: entry {i} (n = {n}): {report}"
    assert bool((got[mask] == M.SENTINEL[4]).all()), f"{what}: a guard element between the accumulators was written"


def _sources(sizes, dtype, launch, shift=0):
    item = _ITEM[dtype]
    pool = _Pool(sizes, item, shift)
    for i, n in enumerate(sizes):
        if launch < 2 or n == 0:
            pool.put(i, M.accum_source(n, item, launch))
        else:
            pool.put(i, M.accum_gaussian(n, dtype, 620 + n % 1000).view(_INT[item]))
    return pool


@pytest.mark.parametrize("sizes", [M.ACCUM_SIZES, M.ACCUM_SIZES_MID], ids=["empty-first", "empty-middle"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_accumulate_sizes_and_domain(dtype, sizes):
    dst = _Pool(sizes, 4)
    for launch, assign in enumerate((1, 0, 0)):
        src = _sources(sizes, dtype, launch)
        before = src.dev.clone()
        _launch_accumulate(dst, [(src, i, dtype) for i in range(len(sizes))], [assign] * len(sizes))
        _check_pool(dst, f"{dtype} launch {launch} ({'assign' if assign else 'add'})")
        assert torch.equal(src.dev, before), "a source was written"


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_accumulate_misaligned_equals_aligned(dtype):
    sizes = M.ACCUM_MISALIGNED
    results = {}
    for name, (s_shift, d_shift) in {"aligned": (0, 0), "src+1": (1, 0), "dst+1": (0, 1), "both+1": (1, 1)}.items():
        dst = _Pool(sizes, 4, d_shift)
        for launch, assign in enumerate((1, 0, 0)):
            src = _sources(sizes, dtype, launch, s_shift)
            assert all((src.ptr(i) % 16 != 0) == bool(s_shift) and (dst.ptr(i) % 16 != 0) == bool(d_shift)
                       for i in range(len(sizes)))
            _launch_accumulate(dst, [(src, i, dtype) for i in range(len(sizes))], [assign] * len(sizes))
            _check_pool(dst, f"{dtype} {name} launch {launch}")
        got = dst.dev.cpu()
        results[name] = [got[o:o + n].clone() for o, n in zip(dst.offs, sizes)]
    for name, wins in results.items():
        for i, w in enumerate(wins):
            _same(w, results["aligned"][i], f"{name} against the aligned run, n = {sizes[i]}")


def test_grad_accumulate_mixed_dtypes_and_assign_flags():
    sizes = [2049, 9, 0, 4097, 65536, 8, 4096]
    dtypes = [torch.float16, torch.float32, torch.bfloat16, torch.bfloat16, torch.float16, torch.float32, torch.bfloat16]
    assigns = [1, 0, 1, 0, 0, 1, 0]
    dst = _Pool(sizes, 4)
    for i, n in enumerate(sizes):                                 # the accumulators start from data, not zeros
        dst.put(i, M.accum_gaussian(n, torch.float32, 640 + i).view(torch.int32))
    pools = {dt: _sources(sizes, dt, 1) for dt in set(dtypes)}
    _launch_accumulate(dst, [(pools[dt], i, dt) for i, dt in enumerate(dtypes)], assigns)
    _check_pool(dst, "mixed table")
    _launch_accumulate(dst, [(pools[dt], i, dt) for i, dt in enumerate(dtypes)], [1 - a for a in assigns])
    _check_pool(dst, "mixed table, flags flipped")


def test_grad_accumulate_wrapper():
    sizes = [n for n in M.ACCUM_SIZES if n]
    accs = [torch.empty(n, dtype=torch.float32, device=DEV) for n in sizes]
    want = [torch.empty(n) for n in sizes]
    for launch, dtype in enumerate(DTYPES):
        srcs = [M.accum_source(n, _ITEM[dtype], 1).view(dtype) for n in sizes]
        _hip.grad_accumulate([(a, s.to(DEV)) for a, s in zip(accs, srcs)], assign=launch == 0)
        torch.cuda.synchronize()
        for a, w, s in zip(accs, want, srcs):
            M.accumulate(w, s, launch == 0)
            report = M.nan_rule(a, w)
            assert report is None, f"_hip.grad_accumulate, {dtype}, n = {w.numel()}: {report}"


# ----------------------------------------------------------------------------- argument errors
def _rejected(rc, fn, frames):
    assert rc < 0, f"{fn} accepted the call"
    msg = _lib().smt_last_error().decode(errors="replace")
    assert fn in msg, msg
    torch.cuda.synchronize()
    for f in frames:
        f.check_intact()
        assert bool((f.whole() == M.SENTINEL[f.itemsize]).all()), f"{fn} wrote its output before failing"


def test_rejected_arguments_write_nothing():
    """Only what the launchers refuse before any launch; every buffer is large enough for the call as
    stated, so nothing here could read or write outside an allocation."""
    lib, dev = _lib(), torch.device(DEV)
    idx = _hip.index_table([1, 0], dev)
    W = _frame(4, 16, 2, 8)
    rows = _frame(2, 16, 2, 8)
    for fn in ("smt_row_gather", "smt_row_scatter"):             # 12-column rows: 24 bytes
        _rejected(getattr(lib, fn)(W.ptr, W.ld, 2, 12, idx.data_ptr(), 2, rows.ptr, rows.ld, _stream()), fn, [W, rows])
        _rejected(getattr(lib, fn)(W.ptr, W.ld, 3, 16, idx.data_ptr(), 2, rows.ptr, rows.ld, _stream()), fn, [W, rows])
    x = _frame(2, 64, 2, 8)
    out = _frame(2, 32, 2, 0)
    cols = _hip.index_table([3, 1, 2, 0], dev)
    # ld_out = 20 (not a multiple of 8), then n_in = 80 > ld_x = 72
    _rejected(lib.smt_column_gather(x.ptr, x.ld, 64, 2, cols.data_ptr(), 4, out.ptr, 20, _stream()), "smt_column_gather", [x, out])
    _rejected(lib.smt_column_gather(x.ptr, x.ld, 80, 2, cols.data_ptr(), 4, out.ptr, out.ld, _stream()), "smt_column_gather",
              [x, out])
    Wt = _frame(B, B, 2, 8)
    tiles = _frame(B, B, 2, 0)
    tab = _hip.tile_table([(0, 0)], dev)
    _rejected(lib.smt_tile_gather(Wt.ptr, Wt.ld, 3, tab.data_ptr(), 1, tiles.ptr, _stream()), "smt_tile_gather", [Wt, tiles])
    _rejected(lib.smt_tile_scatter(Wt.ptr, Wt.ld, 3, tab.data_ptr(), 1, tiles.ptr, _stream()), "smt_tile_scatter", [Wt, tiles])
