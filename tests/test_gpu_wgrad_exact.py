"""Bit-exact per-element tests of the tile weight-gradient kernels: ``tile_wgrad``, ``tile_wgrad_batch`` (with
and without ``seq_len``), ``tile_wgrad_mx`` and ``tile_wgrad_mx_batch`` against the restatements of
tests/wgrad_ref.py on operands whose every fp32 partial sum is exact in any order.

Every case compares every element of every tile on its bits, in an output that lies between two sentinel
tiles (intact afterwards), from operands that are row views of buffers 64 poison rows taller, and asserts
from the workspace-size functions that it reached the branch it is named for: S splits (0 bytes: the direct
store), kps pieces per sample, and the quarter-tile kernels up to 8 tiles. One small tier runs Gaussian
operands against the fp64 truth under the first-order bound of tests/wgrad_ref.py.
"""
import os

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from tests import wgrad_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16, FP16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
SENTINEL = -8192.0                       # exact in bf16, fp16 and fp32
GARBAGE = 3.0                            # what a non-accumulating launch finds in its output
SLAB = 256 * 256 * 4                     # bytes of one fp32 partial slab
QUARTER_MAX = 8                          # the quarter-tile kernels take launches of at most 8 tiles
REPORT = bool(os.environ.get("WGRAD_REF_REPORT"))


def _id(v):
    if isinstance(v, tuple):
        return "-".join(str(_id(t)) for t in v)
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else v


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _rows_view(t):
    """``t`` on the device as the first rows of a buffer 64 poison rows taller."""
    buf = torch.full((t.shape[0] + 64, t.shape[1]), W.POISON, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


class Out:
    """An [n * 256, 256] output between two sentinel tiles, holding ``base`` or garbage."""

    def __init__(self, n, dtype, base=None):
        self.buf = torch.full(((n + 2) * 256, 256), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[256:(n + 1) * 256]
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
        if base is None:
            self.view.fill_(GARBAGE)
        else:
            self.view.copy_(W.to_dtype(base, dtype))

    def result(self):
        torch.cuda.synchronize()
        return self.view.cpu()

    def check(self, want64, what):
        got = self.result()
        want = W.to_dtype(want64, got.dtype)
        same = _bits(got) == _bits(want)
        if not bool(same.all()):
            bad = (~same).nonzero()
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, in tiles "
                                 f"{sorted(set((bad[:, 0] // 256).tolist()))}; first at tile {i // 256} "
                                 f"({i % 256}, {j}): {got[i, j].item()!r} vs {want[i, j].item()!r}")
        ends = torch.cat([self.buf[:256], self.buf[-256:]])
        assert bool((ends == SENTINEL).all()), f"{what}: wrote outside the output"
        return got


def _splits_single(T, n):
    """S of a launch without ``seq_len`` from ``smt_wgrad_workspace_bytes`` (0 bytes: S == 1, direct store)."""
    ws = _hip.wgrad_workspace_bytes(T, n)
    assert ws == int(_hip.load().smt_wgrad_batch_workspace_bytes(T, n)) and ws % (n * SLAB) == 0
    return ws // (n * SLAB) or 1


def _kps_seq(T, seq, n):
    ws = int(_hip.load().smt_wgrad_seq_workspace_bytes(T, seq, n))
    assert ws > 0 and ws % (n * SLAB * (T // seq)) == 0
    return ws // (n * SLAB * (T // seq))


def _splits_mx(ldq, n):
    ws = int(_hip.load().smt_wgrad_mx_workspace_bytes(ldq, n))
    assert ws % (n * SLAB) == 0
    return ws // (n * SLAB) or 1


def _order(n, seed):
    """A random schedule permutation (never the identity for n > 1)."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    if n > 1 and torch.equal(perm, torch.arange(n)):
        perm = perm.flip(0)
    return perm.to(torch.int32).to(DEV)


def _reference(g, x, tiles, seq, dt, out_dt, base):
    if seq:
        return W.reference_rounding(g, x, seq, tiles, dt, out_dt, base)
    return W.single(g, x, tiles, out_dt, base)


def _run_case(what, g, x, tiles, dt, seq, gd=None, xd=None):
    """Every output dtype, with and without ``accumulate`` (the accumulating launch under a random ``order``);
    returns {out dtype: the result without a base}."""
    n = len(tiles)
    gd = _rows_view(g) if gd is None else gd
    xd = _rows_view(x) if xd is None else xd
    rc = _hip.tile_table(tiles, DEV)
    plain = {}
    for out_dt in ([dt, F32] if dt != F32 else [F32]):
        for acc in (False, True):
            base = W.int_base(n, dt, W.seed_of(what)) if acc else None
            out = Out(n, out_dt, base)
            _hip.tile_wgrad(gd, xd, rc, out.view, accumulate=acc, order=_order(n, 5) if acc else None,
                            seq_len=seq or None)
            got = out.check(_reference(g, x, tiles, seq, dt, out_dt, base),
                            f"{what} out {_id(out_dt)} accumulate {acc}")
            if not acc:
                plain[out_dt] = got
    if dt != F32:
        if seq:      # the value is rounded to the operand dtype before it is stored: fp32 out is it widened
            assert torch.equal(_bits(plain[F32]), _bits(plain[dt].float())), f"{what}: fp32 out != 16-bit out widened"
        else:        # fp32 out is the exact sum, 16-bit out its one rounding
            assert torch.equal(_bits(plain[F32].to(dt)), _bits(plain[dt])), f"{what}: 16-bit out != RNE(fp32 out)"
    return plain


# ------------------------------------------------------------------------------------------------
# single rounding
# ------------------------------------------------------------------------------------------------
SINGLE_PARAMS = [(cid, dt) for cid in W.SINGLE_CASES for dt in W.case_dtypes(cid)]
SINGLE_S = {"quarter-direct": 1, "quarter-slabs-S3": 3, "full-direct": 1, "full-slabs-S3": 3}


@pytest.mark.parametrize("cid,dt", SINGLE_PARAMS, ids=_id)
def test_single_rounding(cid, dt):
    n, T = W.SINGLE_CASES[cid]
    assert (n <= QUARTER_MAX) == cid.startswith("quarter") and _splits_single(T, n) == SINGLE_S[cid]
    assert T % 64 and T % 32                                           # a ragged last stage in both pipelines
    g, x = W.int_operands(T, W.OUT_F, W.IN_F, dt, W.seed_of(cid, dt))
    _run_case(f"{cid} {_id(dt)}", g, x, W.TILES[n], dt, 0)


@pytest.mark.parametrize("dt", [BF16, FP16], ids=_id)
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("T", W.EDGE_T)
def test_single_rounding_at_the_stage_edges(T, n, dt):
    assert _splits_single(T, n) == 1
    cid = f"edge-T{T}-n{n}"
    g, x = W.int_operands(T, W.OUT_F, W.IN_F, dt, W.seed_of(cid, dt))
    _run_case(f"{cid} {_id(dt)}", g, x, W.TILES[n], dt, 0)


# ------------------------------------------------------------------------------------------------
# reference rounding
# ------------------------------------------------------------------------------------------------
SEQ_PARAMS = [(cid, dt) for cid in W.SEQ_CASES for dt in W.case_dtypes(cid)]
SEQ_KPS = {"quarter-kps1-3x100": 1, "quarter-kps1-3x33": 1, "quarter-kps2-2x200": 2, "full-kps1-3x100": 1,
           "full-kps2-2x200": 2, "reduce-unroll-9x64": 1, "reduce-unroll-5x64": 1}


@pytest.mark.parametrize("cid,dt", SEQ_PARAMS, ids=_id)
def test_reference_rounding(cid, dt):
    n, B, seq = W.SEQ_CASES[cid]
    T = B * seq
    assert (n <= QUARTER_MAX) == (not cid.startswith("full")) and _kps_seq(T, seq, n) == SEQ_KPS[cid]
    if cid.startswith("reduce-unroll"):
        assert B % 8 and B > 4                                         # the 8-fold unrolled sample loop's remainder
    g, x = W.int_operands(T, W.OUT_F, W.IN_F, dt, W.seed_of(cid, dt))
    _run_case(f"{cid} {_id(dt)}", g, x, W.TILES[n], dt, seq)


# ------------------------------------------------------------------------------------------------
# the register-staged kernel: a leading dimension whose split no longer fits 32-bit buffer offsets
# ------------------------------------------------------------------------------------------------
BIG_LD = 1 << 23
STAGED_TILES = {9: [(3, 1), (0, 0), (1, 1), (4, 0), (2, 1), (0, 1), (3, 0), (1, 0), (4, 1)],
                3: [(1, 1), (4, 0), (2, 1)]}


@pytest.mark.parametrize("n,seq", [(9, 0), (3, 0), (3, 100)], ids=["n9-direct", "n3-direct", "n3-3x100"])
def test_register_staged_kernel_equals_the_dma_kernels_and_the_restatement(n, seq):
    """x is a 512-column view of an (uninitialised) [T + 64, 2^23] buffer: chunk * ld * 2 >= 2^31, so the launch
    takes ``wgrad_partial_kernel`` (no quarter tiles, no 16-bit slabs); the same operands in a contiguous
    tensor take the LDS-DMA kernels. Both bit-identical to the restatement and so to each other."""
    T, dt = 300, BF16
    rows = -(-seq // 32) * 32 if seq else -(-T // _splits_single(T, n))   # a lower bound of the split's rows
    assert rows * BIG_LD * 2 >= 1 << 31 and rows * 1024 * 2 < 1 << 31
    g, x = W.int_operands(T, 1280, 512, dt, W.seed_of("staged", n, seq))
    what = f"register-staged n={n} seq={seq}"
    big = torch.empty((T + 64, BIG_LD), dtype=dt, device=DEV)
    try:
        big[:T, :512] = x.to(DEV)
        big[T:, :512] = W.POISON
        xv = big[:T, :512]
        assert xv.stride(0) == BIG_LD and xv.data_ptr() % 16 == 0
        staged = _run_case(what, g, x, STAGED_TILES[n], dt, seq, xd=xv)
    finally:
        del big
        xv = None
        torch.cuda.empty_cache()
    dma = _run_case(what + " (contiguous)", g, x, STAGED_TILES[n], dt, seq)
    for out_dt in staged:
        assert torch.equal(_bits(staged[out_dt]), _bits(dma[out_dt]))


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
BATCH_WIDTHS = [(512, 768), (768, 1024), (1024, 512)]          # (out, in) of the three modules
BATCH_TILES = {
    8: [[(1, 2), (0, 0), (1, 1)], [(2, 3), (0, 1)], [(3, 1), (1, 0), (0, 1)]],
    11: [[(1, 2), (0, 0), (1, 1), (0, 2)], [(2, 3), (0, 1), (1, 0)], [(3, 1), (1, 0), (0, 1), (2, 0)]],
}
BLOCK_MAJOR_COLS = [1, 0]                                       # module 2's x: its column blocks in this order


@pytest.mark.parametrize("dt", [BF16, FP16, F32], ids=_id)
@pytest.mark.parametrize("T,seq", [(300, 0), (1100, 0), (300, 100)], ids=["direct", "slabs", "seq-3x100"])
@pytest.mark.parametrize("total", [8, 11])
def test_batch_of_three_modules(total, T, seq, dt):
    """One launch over three modules of different widths: module 1 accumulates, module 2 reads the block-major
    copy of ``colblock_gather`` (fp32 operands, which it does not take: the same copy by indexing), the tile
    indices are a non-identity permutation of table order, the table rows are shuffled over the modules and
    ``order`` is a random permutation. Bit-identical without ``order``. fp32 operands (``wgrad_f32_kernel``
    on table rows of every module) give fp32 tiles only."""
    module_tiles = BATCH_TILES[total]
    assert sum(len(t) for t in module_tiles) == total and (total <= QUARTER_MAX) == (total == 8)
    if seq:
        assert _kps_seq(T, seq, total) == 1
    else:
        assert (_splits_single(T, total) > 1) == (T == 1100)
    mods = []
    for m, ((out_f, in_f), tiles) in enumerate(zip(BATCH_WIDTHS, module_tiles)):
        g, x = W.int_operands(T, out_f, in_f, dt, W.seed_of("batch", m, total, T, dt))
        slot = torch.randperm(len(tiles), generator=torch.Generator().manual_seed(40 + m)).tolist()
        if slot == sorted(slot):
            slot = slot[::-1]
        xd = _rows_view(x)
        if m == 2 and dt == F32:
            xd = torch.stack([xd[:, 256 * c:256 * (c + 1)] for c in BLOCK_MAJOR_COLS]).contiguous()
        elif m == 2:
            xd = _hip.colblock_gather(xd, torch.tensor(BLOCK_MAJOR_COLS, dtype=torch.int32, device=DEV))
        if m == 2:
            assert xd.shape == (len(BLOCK_MAJOR_COLS), T, 256) and xd.is_contiguous()
        mods.append(dict(g=g, x=x, gd=_rows_view(g), xd=xd, tiles=tiles, slot=slot, acc=(m == 1)))
    rows = []
    for m, md in enumerate(mods):
        for i, (r, c) in enumerate(md["tiles"]):
            rows.append((m, r, BLOCK_MAJOR_COLS.index(c) if m == 2 else c, md["slot"][i]))
    shuffle = torch.randperm(total, generator=torch.Generator().manual_seed(total)).tolist()
    tab = torch.tensor([rows[i] for i in shuffle], dtype=torch.int32, device=DEV)
    for out_dt in ((dt, F32) if dt != F32 else (F32,)):
        results = []
        for order in (_order(total, 9), None):
            outs = []
            for m, md in enumerate(mods):
                base = W.int_base(len(md["tiles"]), dt, W.seed_of("batch", m)) if md["acc"] else None
                outs.append((Out(len(md["tiles"]), out_dt, base), base))
            _hip.tile_wgrad_batch([(md["gd"], md["xd"], o.view, md["acc"]) for md, (o, _) in zip(mods, outs)], tab,
                                  order, seq_len=seq or None)
            got = []
            for m, (md, (o, base)) in enumerate(zip(mods, outs)):
                by_slot = [md["tiles"][md["slot"].index(k)] for k in range(len(md["tiles"]))]
                want = _reference(md["g"], md["x"], by_slot, seq, dt, out_dt, base)
                got.append(o.check(want, f"batch {total} module {m} out {_id(out_dt)} order {order is not None}"))
            results.append(got)
        for a, b in zip(*results):
            assert torch.equal(_bits(a), _bits(b)), "order changed the result"


# ------------------------------------------------------------------------------------------------
# MX
# ------------------------------------------------------------------------------------------------
MX_RBS, MX_CBS = [2, 0, 3, 1], [1, 2, 0]                        # the quantised blocks, not in matrix order


def _mx_first_slab_T(n):
    """The smallest ldq at which an n-tile MX launch splits, by asking the size function; T ragged below it."""
    ldq = next(l for l in range(64, 8192, 64) if _splits_mx(l, n) > 1)
    return ldq - 28, ldq


def _mx_module(T, seed):
    g, x = W.mx_int_operands(T, W.OUT_F, W.IN_F, seed)
    qg = _hip.mx_quant_cols(_rows_view(g), torch.tensor(MX_RBS, dtype=torch.int32, device=DEV))
    qx = _hip.mx_quant_cols(_rows_view(x), torch.tensor(MX_CBS, dtype=torch.int32, device=DEV))
    return g, x, qg, qx


def _mx_packed(tiles):
    return [(MX_RBS.index(r), MX_CBS.index(c)) for r, c in tiles]


@pytest.mark.parametrize("n,kind", [(9, "direct-320"), (9, "ragged-300"), (2, "ragged-300"), (2, "slabs"), (9, "slabs")],
                         ids=_id)
def test_mx_against_the_single_rounding_of_the_bf16_operands(n, kind):
    if kind == "slabs":
        T, ldq = _mx_first_slab_T(n)
        assert _splits_mx(ldq, n) > 1 and _splits_mx(ldq - 64, n) == 1 and _hip.mx_ld(T) == ldq
    else:
        T = int(kind.split("-")[1])
        assert _splits_mx(_hip.mx_ld(T), n) == 1
    tiles = W.TILES[n]
    g, x, qg, qx = _mx_module(T, W.seed_of("mx", n, kind))
    table = _hip.tile_table(_mx_packed(tiles), DEV)
    for out_dt in (BF16, F32):
        for acc in (False, True):
            base = W.int_base(n, BF16, W.seed_of("mx", n, kind)) if acc else None
            out = Out(n, out_dt, base)
            _hip.tile_wgrad_mx(qg, qx, table, out.view, accumulate=acc, order=_order(n, 3) if acc else None)
            out.check(W.single(g, x, tiles, out_dt, base, unit2=W.MX_UNIT2),
                      f"mx n={n} {kind} out {_id(out_dt)} accumulate {acc}")


@pytest.mark.parametrize("total", [2, 9])
def test_mx_batch_of_two_modules_with_slabs(total):
    """Two modules in one launch at the first T that splits (``wgrad_reduce_batch_kernel`` on the MX modules), module 1
    accumulating, tile indices reversed, the table rows interleaved, a random ``order``."""
    T, ldq = _mx_first_slab_T(total)
    assert _splits_mx(ldq, total) > 1
    module_tiles = [W.TILES[9][:total - total // 2], W.TILES[9][::-1][:total // 2]]
    mods = [_mx_module(T, W.seed_of("mx-batch", m, total)) for m in range(2)]
    rows = []
    for m, tiles in enumerate(module_tiles):
        rows.extend((m, r, c, len(tiles) - 1 - i) for i, (r, c) in enumerate(_mx_packed(tiles)))
    rows = rows[::2] + rows[1::2]
    tab = torch.tensor(rows, dtype=torch.int32, device=DEV)
    for out_dt in (BF16, F32):
        outs = []
        for m, tiles in enumerate(module_tiles):
            base = W.int_base(len(tiles), BF16, W.seed_of("mx-batch", m)) if m == 1 else None
            outs.append((Out(len(tiles), out_dt, base), base))
        _hip.tile_wgrad_mx_batch([(qg, qx, o.view, m == 1) for m, ((_, _, qg, qx), (o, _)) in enumerate(zip(mods, outs))],
                                 tab, _order(total, 4))
        for m, ((g, x, _, _), (o, base), tiles) in enumerate(zip(mods, outs, module_tiles)):
            o.check(W.single(g, x, tiles[::-1], out_dt, base, unit2=W.MX_UNIT2),
                    f"mx batch {total} module {m} out {_id(out_dt)}")


# ------------------------------------------------------------------------------------------------
# random data: every element inside the first-order bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, FP16, F32], ids=_id)
@pytest.mark.parametrize("cid", list(W.SINGLE_CASES))
def test_random_operands_inside_the_first_order_bound(cid, dt):
    n, T = W.SINGLE_CASES[cid]
    S = _splits_single(T, n)
    assert S == SINGLE_S[cid]
    tiles = W.TILES[n]
    g, x = W.random_operands(T, W.OUT_F, W.IN_F, dt, W.seed_of("random", cid, dt))
    out = Out(n, F32)
    _hip.tile_wgrad(_rows_view(g), _rows_view(x), _hip.tile_table(tiles, DEV), out.view)
    got = out.result().to(F64).view(n, 256, 256)
    assert bool((out.buf[:256] == SENTINEL).all()) and bool((out.buf[-256:] == SENTINEL).all())
    truth, bound = W.random_bound(g, x, tiles, T, S)
    ratio = ((got - truth).abs() / bound).max().item()
    if REPORT:
        print(f"\nWGRAD_RATIO {cid} {_id(dt)}: {ratio:.3f}")
    allowed = W.RANDOM_ALLOWANCE[dt]
    bad = (got - truth).abs() > allowed * bound
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements outside {allowed} x the bound; largest ratio {ratio:.3f}"
