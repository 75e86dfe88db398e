"""CPU checks of ``tests/move_ref.py``: the references agree with the oracle where it has one,
``exact_grid`` keeps its promises, the frame sees one flipped guard element anywhere, and a wrong
kernel (thirteen of them, restated in Python) fails the check of the GPU tests on the very inputs those
tests use."""
import pytest
import torch

from oracle import smt_oracle as ref
from tests import move_ref as M

B = M.BLOCK


# ----------------------------------------------------------------------------- inputs
def test_domain16_is_every_pattern_once():
    d = M.domain16(3)
    assert d.shape == (256, 256) and d.dtype == torch.int16
    assert torch.equal(d.reshape(-1).long().sort().values, torch.arange(-32768, 32768))
    assert not torch.equal(d, M.domain16(4)) and torch.equal(d, M.domain16(3))
    for dt in (torch.bfloat16, torch.float16):                   # NaNs, infinities, zeros of both signs, subnormals
        v = d.view(dt)
        assert torch.isnan(v).any() and torch.isinf(v).any() and (v == 0).sum() == 2


def test_patterns32_holds_the_special_values():
    p = M.patterns32(5)
    have = set((p.reshape(-1).long() & 0xFFFFFFFF).tolist())
    assert set(M.SPECIALS32) <= have
    f = p.view(torch.float32)
    assert torch.isnan(f).any() and torch.isinf(f).any()


@pytest.mark.parametrize("itemsize", [2, 4])
def test_cases_hold_the_domain(itemsize):
    r, c = M.TILE_DOMAIN_BLOCK
    assert torch.equal(M.tile_case(itemsize)[r * B:(r + 1) * B, c * B:(c + 1) * B], M.domain_tile(itemsize, 101 + itemsize))
    if itemsize == 2:
        w = M.row_case(2, M.ROW_DOMAIN_WIDTH)
        moved = M.rows_of(w, M.ROW_INDEX, M.ROW_DOMAIN_WIDTH).reshape(-1).long()
        assert moved.unique().numel() == 65536
        x, cols = M.column_case(256, 256, 256)
        assert M.columns_of(x, cols, 256).reshape(-1).long().unique().numel() == 65536
        assert M.colblocks_of(M.colblock_case(256, 768), [2, 0, 1])[0].reshape(-1).long().unique().numel() == 65536
        _, flat = M.scatter_t_case()
        assert flat[2 * M.TILE:3 * M.TILE].long().unique().numel() == 65536


# ----------------------------------------------------------------------------- references against the oracle
@pytest.mark.parametrize("itemsize", [2, 4])
def test_tile_references_agree_with_the_oracle(itemsize):
    W = M.tile_case(itemsize)
    for tiles in (M.TILE_LIST, M.TILE_LIST[:1]):
        got = M.tiles_of(W, tiles)
        assert torch.equal(got, ref.gather_tiles(W, tiles))
        new = M.random_bits(got.shape, itemsize, 9)
        W2 = W.clone()
        ref.writeback_tiles(W2, new, tiles)
        assert torch.equal(M.scatter_tiles(W, tiles, new), W2)


@pytest.mark.parametrize("itemsize", [2, 4])
def test_row_references_agree_with_the_oracle(itemsize):
    for n_cols in M.ROW_WIDTHS[itemsize]:
        W = M.row_case(itemsize, n_cols)
        got = M.rows_of(W, M.ROW_INDEX, n_cols)
        assert torch.equal(got, ref.gather_rows(W, M.ROW_INDEX))
        new = M.random_bits(got.shape, itemsize, 10)
        W2 = W.clone()
        for i, r in enumerate(M.ROW_INDEX):
            W2[r] = new[i]
        assert torch.equal(M.scatter_rows(W, M.ROW_INDEX, new, n_cols), W2)


def test_transposed_scatter_is_the_transpose_of_the_write_back():
    Wt, flat = M.scatter_t_case()
    live = [(r, c, off) for on, r, c, off in M.SCATTER_T_DESCS if on]
    W = Wt.t().contiguous()
    ref.writeback_tiles(W, torch.cat([flat[off:off + M.TILE].view(B, B) for _, _, off in live]), [(r, c) for r, c, _ in live])
    assert torch.equal(M.scatter_tiles_t(Wt, M.SCATTER_T_DESCS, flat), W.t())


def test_column_references():
    x, cols = M.column_case(5, 8192, 13)
    out = M.columns_of(x, cols, 256)
    assert torch.equal(out[:, :13], x[:, cols]) and not out[:, 13:].any()
    xb = M.colblock_case(9, 768)
    assert torch.equal(M.colblocks_of(xb, [2, 0, 1]), torch.stack([xb[:, 512:768], xb[:, 0:256], xb[:, 256:512]]))


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_block_raw_exact_is_the_oracle_bit_for_bit(strategy):
    for k, x, (d1, d2) in M.score_case():
        assert torch.equal(M.block_raw_exact(k, x, d1, d2, strategy), ref.block_raw_fp64(x, d1, d2, strategy))


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_channel_raw_exact_is_the_oracle_bit_for_bit(strategy):
    for Bn in M.CHANNEL_B:
        for S in M.CHANNEL_S:
            k, x = M.channel_case(Bn, S)
            assert torch.equal(M.channel_raw_exact(k, strategy), ref.channel_raw_fp64(x, strategy))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_harvest_agrees_with_the_oracle_hook(dtype):
    feat, acc = {}, torch.empty(3, 5, 520)
    for step in range(3):
        x = M.accum_gaussian(3 * 5 * 520, dtype, 40 + step).view(3, 5, 520)
        ref.channel_hook_accumulate(feat, "k", x)
        M.harvest(acc, x, assign=step == 0)
        assert M.nan_rule(acc, feat["k"]) is None
        assert torch.equal(acc, feat["k"])


# ----------------------------------------------------------------------------- exact_grid keeps its promises
def test_exact_grid_sums_do_not_depend_on_the_order():
    k, x = M.exact_grid((256, 256), 11)
    assert int(k.abs().max()) < (1 << 14) and x.dtype == torch.float32
    terms = {"mean_abs": x.double(), "abs_mean": x.abs().double(), "L2": (x * x).double()}
    for name, t in terms.items():
        want = M.block_raw_exact(k, x, 1, 1, name)[0, 0].item()
        flat = t.reshape(-1)
        for seed in (1, 2):
            p = flat[torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))]
            seq = 0.0
            for chunk in p.view(256, 256):                       # a different association as well
                seq = seq + chunk.sum().item()
            assert p.sum().item() == want and seq == want and p.flip(0).cumsum(0)[-1].item() == want


def test_exact_grid_has_inexact_squares():
    k, x = M.exact_grid((256, 256), 11)
    share = (M.l2_units(x) != k * k).double().mean().item()
    assert share > 0.25, share                                  # 41.7 % on random 14-bit k
    with pytest.raises(AssertionError):
        M.from_k(torch.tensor([1 << 14]))


# ----------------------------------------------------------------------------- the frame
@pytest.mark.parametrize("itemsize", [2, 4, 8])
def test_frame_reports_one_flipped_guard_element_in_each_region(itemsize):
    def frame():
        return M.Frame(3, 8, itemsize, pad=8, before=2, after=2)
    f = frame()
    f.check_intact()
    assert f.ptr % 16 == 0 and f.ld == 16 and f.view({2: torch.bfloat16, 4: torch.float32, 8: torch.float64}[itemsize]).shape == (3, 8)
    f.fill(torch.arange(24))
    f.check_intact()                                            # the window itself is free
    assert torch.equal(f.whole(), f.expected_whole(torch.arange(24)))
    spots = {"head": [0, 15], "rows before": [16, 16 + 2 * 16 - 1], "row padding": [16 + 2 * 16 + 8, 16 + 5 * 16 - 1],
             "rows after": [16 + 5 * 16, 16 + 7 * 16 - 1], "tail": [16 + 7 * 16, 16 + 7 * 16 + 15]}
    assert set(spots) == set(M.Frame.REGIONS)
    for region, where in spots.items():
        for i in where:
            f = frame()
            f.flat[i] ^= 1
            report = f.damage()
            assert report is not None and f"({region})" in report and "1 guard element" in report, (region, i, report)
            with pytest.raises(AssertionError):
                f.check_intact()


def test_carve_keeps_guards_and_alignment():
    for itemsize in (2, 4):
        for shift in (0, 1):
            offs, total = M.carve(M.ACCUM_SIZES, itemsize, shift)
            end = 0
            for o, n in zip(offs, M.ACCUM_SIZES):
                assert (o - shift) * itemsize % 16 == 0 and o - end >= 16
                end = o + n
            assert total - end >= 16


# ----------------------------------------------------------------------------- the inputs see a wrong kernel
def _framed(frame_bits, want):
    """The check of the GPU tests on a framed output: every bit, guards included."""
    return torch.equal(frame_bits, want)


@pytest.mark.parametrize("itemsize", [2, 4])
@pytest.mark.parametrize("n_tiles", [4, 1])
def test_mutation_tile_row_and_column_swapped(itemsize, n_tiles):
    W, tiles = M.tile_case(itemsize), M.TILE_LIST[:n_tiles]
    swapped = [(c % 2, r % 3) for r, c in tiles]                 # (r, c) exchanged, folded into the 2 x 3 grid
    assert not torch.equal(M.tiles_of(W, swapped), M.tiles_of(W, tiles))
    new = M.random_bits((n_tiles * B, B), itemsize, 9)
    assert not torch.equal(M.scatter_tiles(W, swapped, new), M.scatter_tiles(W, tiles, new))


def test_mutation_transposed_scatter_without_the_transpose():
    Wt, flat = M.scatter_t_case()
    wrong = Wt.clone()
    for live, r, c, off in M.SCATTER_T_DESCS:
        if live:
            wrong[c * B:(c + 1) * B, r * B:(r + 1) * B] = flat[off:off + M.TILE].view(B, B)
    assert not torch.equal(wrong, M.scatter_tiles_t(Wt, M.SCATTER_T_DESCS, flat))
    # a kernel that does not skip the NULL-weight descriptor, or takes the tiles in table order
    alive = [(True, r, c, off) for _, r, c, off in M.SCATTER_T_DESCS]
    assert not torch.equal(M.scatter_tiles_t(Wt, alive, flat), M.scatter_tiles_t(Wt, M.SCATTER_T_DESCS, flat))
    in_order = [(live, r, c, i * M.TILE) for i, (live, r, c, _) in enumerate(M.SCATTER_T_DESCS)]
    assert not torch.equal(M.scatter_tiles_t(Wt, in_order, flat), M.scatter_tiles_t(Wt, M.SCATTER_T_DESCS, flat))


@pytest.mark.parametrize("itemsize", [2, 4])
def test_mutation_chunk_dropped_at_the_slice_boundary(itemsize):
    per16 = 16 // itemsize
    for n_cols, lo_byte in ((M.ROW_WIDTHS[itemsize][2], 4096), (M.ROW_WIDTHS[itemsize][1], 4080),
                            (M.ROW_WIDTHS[itemsize][2], 4080), (M.ROW_WIDTHS[itemsize][0], 0)):
        W = M.row_case(itemsize, n_cols)
        want = M.rows_of(W, M.ROW_INDEX, n_cols)
        wrong = want.clone()
        lo = lo_byte // itemsize
        wrong[:, lo:lo + per16] = M.SENTINEL[itemsize]           # the destination keeps what it held
        assert not torch.equal(wrong, want)
        new = M.random_bits(want.shape, itemsize, 10)
        good = M.scatter_rows(W, M.ROW_INDEX, new, n_cols)
        bad = good.clone()
        for r in M.ROW_INDEX:
            bad[r, lo:lo + per16] = W[r, lo:lo + per16]
        assert not torch.equal(bad, good)
    # one chunk too many: it lands in the row padding, which only the frame sees
    f = M.Frame(3, M.ROW_WIDTHS[itemsize][2], itemsize, pad=M.ROW_PADS[itemsize][1])
    f.view({2: torch.int16, 4: torch.int32}[itemsize])            # same width
    f.flat[f.off + f.before * f.ld + f.cols] = 0
    assert f.damage() is not None and "(row padding)" in f.damage()


@pytest.mark.parametrize("itemsize", [2, 4])
def test_mutation_row_index_off_by_one(itemsize):
    for n_cols in M.ROW_WIDTHS[itemsize]:
        W = M.row_case(itemsize, n_cols)
        off = [(r + 1) % M.ROW_COUNT for r in M.ROW_INDEX]
        assert not torch.equal(M.rows_of(W, off, n_cols), M.rows_of(W, M.ROW_INDEX, n_cols))
        shifted = M.ROW_INDEX[1:] + M.ROW_INDEX[:1]               # the table read one entry on
        assert not torch.equal(M.rows_of(W, shifted, n_cols), M.rows_of(W, M.ROW_INDEX, n_cols))


def test_mutation_stale_padding_and_shifted_columns():
    for T, n_in, n_cols, ld_out in M.COLUMN_CASES:
        x, cols = M.column_case(T, n_in, n_cols)
        want = M.columns_of(x, cols, ld_out)
        if ld_out > n_cols:
            stale = torch.full_like(want, M.SENTINEL[2])         # a buffer that was never zeroed
            stale[:, :n_cols] = want[:, :n_cols]
            assert not torch.equal(stale, want)
        if n_cols:
            assert not torch.equal(M.columns_of(x, cols[1:] + cols[:1], ld_out), want)
            if T > 1:                                            # rows of another workgroup slot
                assert not torch.equal(M.columns_of(x.roll(1, 0), cols, ld_out), want)
    for T, in_f, blocks in M.COLBLOCK_CASES:
        x = M.colblock_case(T, in_f)
        want = M.colblocks_of(x, blocks)
        row_major = torch.cat([x[:, b * B:(b + 1) * B] for b in blocks], 1).reshape(want.shape)   # the layout before ABI v5
        if T > 1 and len(blocks) > 1:
            assert not torch.equal(row_major, want)
        assert not torch.equal(M.colblocks_of(x, [(b + 1) % (in_f // B) for b in blocks]), want)


def test_mutation_l2_squared_in_fp64():
    for k, x, (d1, d2) in M.score_case():
        want = M.block_raw_exact(k, x, d1, d2, "L2")
        fused = torch.stack([(x.double() ** 2).reshape(d1, B, d2, B).sum(dim=(1, 3)).reshape(-1)] * 2, 1)
        assert not torch.equal(fused, want)
        ok = (x * x).double().reshape(d1, B, d2, B).sum(dim=(1, 3)).reshape(-1)
        assert torch.equal(ok, want[:, 0])


def test_mutation_mean_abs_summing_magnitudes():
    for k, x, (d1, d2) in M.score_case():
        want = M.block_raw_exact(k, x, d1, d2, "mean_abs")
        wrong = M.block_raw_exact(k, x, d1, d2, "abs_mean")
        assert not torch.equal(wrong[:, 0], want[:, 0]) and torch.equal(wrong[:, 1], want[:, 1])
    k, x, _ = M.score_case()[1]
    raw = M.block_raw_exact(k, x, 2, 3, "mean_abs")
    assert raw[0, 0] == 0 and raw[0, 1] == 0                     # the all-zero block
    assert raw[1, 0] == -raw[1, 1] and raw[1, 0] < 0             # the all-negative block
    assert raw[5, 1] == (abs(int(k[256, 512])) + abs(int(k[511, 767]))) * 2.0 ** -10     # the two corners


def test_mutation_block_coordinates_from_d1():
    k, x, (d1, d2) = M.score_case()[1]
    for strategy in M.STRATEGIES:
        want = M.block_raw_exact(k, x, d1, d2, strategy)
        per_block = want.view(d1, d2, 2)
        # local blocks 0..3 stay inside the gradient with the wrong divisor (4 and 5 would leave it)
        wrong = torch.stack([per_block[local // d1, local % d1] for local in range(4)])
        assert not torch.equal(wrong, want[:4])
        assert not torch.equal(wrong[2], want[2]) and not torch.equal(wrong[3], want[3])


def _walk_table(grids, strict):
    """Which (entry, local block) each launched block writes, with the lookup of the kernel."""
    begins, n = [], 0
    for d1, d2 in grids:
        begins.append(n)
        n += d1 * d2
    written = set()
    for blk in range(n):
        e = M.find_entry(begins, blk, strict)
        written.add((e, blk - begins[e]))
    return written, {(e, l) for e, (d1, d2) in enumerate(grids) for l in range(d1 * d2)}


def test_mutation_entry_lookup_strict_at_a_block_begin():
    written, wanted = _walk_table(M.SCORE_GRIDS, strict=False)
    assert written == wanted
    written, wanted = _walk_table(M.SCORE_GRIDS, strict=True)
    # the first block of the second and third gradient is never written (its sentinel stays), and a
    # block past the end of the first and second one is: both show in the framed output
    assert {(1, 0), (2, 0)} <= wanted - written and written - wanted
    # the same lookup over the chunk prefixes of the accumulation tables, empty entries included
    for sizes in (M.ACCUM_SIZES, M.ACCUM_SIZES_MID):
        begins, n = [], 0
        for s in sizes:
            begins.append(n)
            n += (s + 4095) // 4096
        for strict in (False, True):
            seen = {}
            for chunk in range(n):
                e = M.find_entry(begins, chunk, strict)
                seen.setdefault(e, []).append(chunk - begins[e])
            good = all(seen.get(e, []) == list(range((s + 4095) // 4096)) for e, s in enumerate(sizes))
            assert good != strict


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_mutation_last_channel_partial_dropped(strategy):
    for Bn in M.CHANNEL_B:
        for S in M.CHANNEL_S:
            k, _ = M.channel_case(Bn, S)
            want = M.channel_raw_exact(k, strategy)
            kept = (S - 1) // 32 * 32
            wrong = M.channel_raw_exact(k[:, :kept], strategy) if kept else torch.zeros_like(want)
            assert not torch.equal(wrong, want)
            if S > 1:                                           # and a partial that stops one row early
                assert not torch.equal(M.channel_raw_exact(k[:, :S - 1], strategy), want)


def test_mutation_channel_square_per_element():
    for S in M.CHANNEL_S:
        k, _ = M.channel_case(3, S)
        wrong = (k * k).sum(dim=(0, 1)).double() * 2.0 ** -20
        assert not torch.equal(wrong, M.channel_raw_exact(k, "L2"))
        # the batch sum taken without the magnitudes
        A = k.sum(0)
        assert not torch.equal((A * A).sum(0).double() * 2.0 ** -20, M.channel_raw_exact(k, "L2"))
        assert not torch.equal(A.sum(0).double() * 2.0 ** -10, M.channel_raw_exact(k, "L1"))


_DT = {2: (torch.bfloat16, torch.float16), 4: (torch.float32,)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_mutation_accumulate_assigns_and_wrong_widening(dtype):
    itemsize = torch.empty(0, dtype=dtype).element_size()
    for n in [s for s in M.ACCUM_SIZES if s]:
        s0 = M.accum_source(n, itemsize, 0).view(dtype)
        s1 = M.accum_source(n, itemsize, 1).view(dtype)
        want = M.accumulate(M.accumulate(torch.empty(n), s0, True), s1, False)
        assigned = M.accumulate(M.accumulate(torch.empty(n), s0, True), s1, True)
        assert M.nan_rule(assigned, want) is not None, n
        if n == M.TILE:                                          # an assign done as `0 + x` loses the -0.0
            added = M.accumulate(torch.zeros(n), s0, False)
            assert M.nan_rule(added, M.accumulate(torch.empty(n), s0, True)) is not None
        if itemsize == 2:
            other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
            widened = M.accumulate(torch.empty(n), M.accum_source(n, 2, 0).view(other), True)
            assert M.nan_rule(widened, M.accumulate(torch.empty(n), s0, True)) is not None, n


def test_nan_rule_excuses_only_nan_positions():
    want = torch.tensor([1.0, float("nan"), -0.0, float("inf")])
    assert M.nan_rule(want.clone(), want) is None
    quiet = want.clone()
    quiet.view(torch.int32)[1] = 0x7FC00001
    assert M.nan_rule(quiet, want) is None
    for i, v in ((1, 2.0), (2, 0.0), (0, float("nan")), (3, float("nan"))):
        got = want.clone()
        got[i] = v
        assert M.nan_rule(got, want) is not None, i
