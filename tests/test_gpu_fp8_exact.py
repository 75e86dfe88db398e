"""The e4m3 quantisers (csrc/fp8_kernels.hip, the QUANT RMSNorm kernels of csrc/llama_kernels.hip)
against tests/fp8_ref.py, bit for bit, on their whole value domain and at every dispatch edge; and the
fp8 GEMM seams against the fp64 product of the operands they used, element by element.

Expected bytes and scales are computed on the CPU from the input's bits (integer and fp64 arithmetic;
tests/test_fp8_ref_host.py checks that reference and shows that these inputs see a wrong quantiser).
Every output lies inside a larger buffer filled with a sentinel (pad columns, rows before and after,
unselected blocks), which must be intact afterwards. No element is excused.

GEMM seam bound, per element v = sa_i * sb_j * sum_k a_ik b_jk (the decoded operands of the call), the
sum of three terms ("The bar on fp8 quantisation", has the measurements behind the last two
and the worst err / bound seen on the MI355X):

* one bf16 rounding of the result: half a step of an 8-bit significand, 2^(floor(log2 |v|) - 8). That is
  2^-9 |v| only at the top of a binade and 2^-8 |v| at its bottom, so 2^-9 |v| alone is not a bound.
* the fp32 chain over the partial sums and the two scale multiplies, (K + 4) * 2^-24 * sa_i * sb_j *
  sum_k |a_ik b_jk|.
* the alignment inside one MFMA instruction: the library's kernel adds the e4m3 products of an
  instruction after aligning them to the largest one, 2^e with e the sum of its operands' exponents,
  and drops what lies below 2^(e - 13) (scripts/diag/fp8_gemm_accum_probe.py: beside +-448 * 448 =
  +-1.53 * 2^17 (e = 16) a product of 2^3 survives and 2^2 is lost; beside +-2^8 it is 2^-5 and 2^-6,
  beside +-2^-2 2^-15 and 2^-16; across instructions the sum is an exact fp32 chain). The product of
  two 4-bit significands has at most 7 significant bits, so it loses something only if its exponent
  is more than 6 below the cut's 13, and then less than min(|p|, 2^(e - 13)). Here e is replaced by
  emax = floor(log2 max_k |p_k|) >= e over the whole dot product, which bounds every instruction's own.
"""
import functools

import numpy as np
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fp8 as f8
from tests import fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}
_SENT = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Frame:
    """An output of ``rows x cols`` elements inside a device buffer filled with a sentinel: ``pad``
    columns after each row, ``before`` / ``after`` rows around it, and 16 elements at either end."""

    def __init__(self, rows, cols, itemsize, pad=8, before=2, after=2, ptr_mod16=None):
        self.rows, self.cols, self.before, self.itemsize = rows, cols, before, itemsize
        self.ld = cols + pad
        self.total = (before + rows + after) * self.ld
        self.sent = _NP[itemsize](_SENT[itemsize])
        fill = int(np.array(self.sent).view({1: np.uint8, 2: np.int16, 4: np.int32}[itemsize]))
        self.flat = torch.full((self.total + 32,), fill, dtype=_TORCH[itemsize], device=DEV)
        self.off = 16
        if ptr_mod16 is not None:               # place the output's first byte at this offset from a 16-byte boundary
            base = self.flat.data_ptr() + (self.off + before * self.ld) * itemsize
            self.off += ((ptr_mod16 - base) % 16) // itemsize
        self.view = self.flat[self.off:self.off + self.total].view(-1, self.ld)[before:before + rows, :cols]
        self.ptr = self.view.data_ptr()
        assert ptr_mod16 is None or self.ptr % 16 == ptr_mod16

    def got(self) -> np.ndarray:
        return self.view.cpu().numpy().view(_NP[self.itemsize])

    def check(self, want, what, **info):
        """Every bit of the output equals ``want`` (rows of ``want`` equal to the sentinel: untouched),
        and the sentinel around it is intact."""
        want = np.ascontiguousarray(want).view(_NP[self.itemsize]).reshape(self.rows, self.cols)
        report = R.compare_bits(self.got(), want, what, **info)
        assert report is None, report
        flat = self.flat.cpu().numpy().view(_NP[self.itemsize])
        exp = np.full_like(flat, self.sent)
        exp[self.off:self.off + self.total].reshape(-1, self.ld)[self.before:self.before + self.rows, :self.cols] = want
        report = R.compare_bits(flat, exp, what + " (sentinel around the output)")
        assert report is None, report


def _scales_frame(rows):
    return Frame(rows, 1, 4, pad=0)


def _bf16_in(bits: np.ndarray, pad=0, junk=0x7F7F) -> torch.Tensor:
    """The bf16 matrix with these bits on the device, as a column slice of a buffer ``pad`` columns
    wider whose other columns hold a huge finite value (an amax that read them would show)."""
    rows, cols = bits.shape
    big = np.full((rows, cols + pad), junk, dtype=np.uint16)
    big[:, :cols] = bits
    return R.bits_to_bf16(big).to(DEV)[:, :cols]


def _dev_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ----------------------------------------------------------------------------- quant_rows: the value domain

@functools.lru_cache(maxsize=None)
def _domain_reference(cols):
    x, amax = R.domain_rows(cols)
    return x, amax, R.quant_rows(x)


@pytest.mark.parametrize("cols", [1024, 4096, 16384, 16392])       # reg<2>, reg<8>, wg<8>, two-pass
def test_quant_rows_value_domain(cols):
    """Every bf16 amax of eight binades and every subnormal one, against every bf16 x within 2^-20 of
    it in both signs, +-0 and a few far smaller values; the amax element alone in its row, moving
    through the lanes and waves, negative in every other row."""
    x, amax, (q, s) = _domain_reference(cols)
    assert x.shape[0] % 4 == 3                                       # a ragged last workgroup of four rows
    table = R.domain_pair_table(x, amax)
    assert np.array_equal(table, R.domain_expected_table()) and int(table.sum()) == R.DOMAIN_PAIRS
    out, sc = Frame(x.shape[0], cols, 1), _scales_frame(x.shape[0])
    f8.quant_rows(_bf16_in(x), out=out.view, scales=sc.view[:, 0])
    torch.cuda.synchronize()
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=x, scales=s)


# ----------------------------------------------------------------------------- quant_rows: geometry

def _mixed_rows(rows, cols, seed):
    """Rows of very different magnitude (tiny and subnormal ones too), +-0.0 inside, row 4 all zero."""
    rng = np.random.default_rng(seed)
    exps = (0, -3, 6, -118, 0, -131, 100, -20, -112)
    x = np.stack([R.random_bits(rng, 1, cols, exps[r % len(exps)] - (r // len(exps)) % 5)[0] for r in range(rows)])
    x[4 % rows] = 0
    return x


def _quant_rows_abi(xd, rows, cols, out, sc, blocks=None):
    rc = _hip.load().smt_quant_rows_e4m3(xd.data_ptr(), xd.stride(0), rows, cols,
                                         None if blocks is None else blocks.data_ptr(),
                                         0 if blocks is None else blocks.numel(), out.ptr, out.ld, sc.ptr, _stream())
    _hip._check(rc, "smt_quant_rows_e4m3")
    torch.cuda.synchronize()


@pytest.mark.parametrize("cols", [8, 1016, 1024, 1032, 4096, 4104, 16384, 16392])   # either side of each kernel switch
def test_quant_rows_geometry(cols):
    rows = 9
    x = _mixed_rows(rows, cols, cols)
    q, s = R.quant_rows(x)
    assert s[4] == 1.0 and not q[4].any()                            # an all-zero row: scale 1, bytes 0
    xd = _bf16_in(x, pad=8)
    assert xd.stride(0) == cols + 8
    out, sc = Frame(rows, cols, 1, pad=8, ptr_mod16=8), _scales_frame(rows)
    _quant_rows_abi(xd, rows, cols, out, sc)
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=x, scales=s)


@pytest.mark.parametrize("cols", [520, 1032, 4104, 16392])          # one width per kernel
def test_quant_rows_selected_blocks(cols):
    """row_blocks = [2, 0] of 600 rows: block 2 is ragged (88 rows), block 1 stays untouched."""
    rows = 600
    x = _mixed_rows(rows, cols, cols + 1)
    q, s = R.quant_rows(x)
    out, sc = Frame(rows, cols, 1), _scales_frame(rows)
    q[256:512] = out.sent
    s = s.view(np.uint32).copy()
    s[256:512] = sc.sent
    blocks = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    _quant_rows_abi(_bf16_in(x, pad=8), rows, cols, out, sc, blocks)
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=x)


# ----------------------------------------------------------------------------- quant_rows_cat

@pytest.mark.parametrize("widths", R.CAT_CASES)
def test_quant_rows_cat(widths):
    parts = R.cat_case(widths)
    q, s = R.quant_rows_cat(parts)
    rows, total = R.CAT_ROWS, sum(widths)
    srcs_d = [_bf16_in(p, pad=8 + 8 * k) for k, p in enumerate(parts)]            # each ld > cols
    srcs = (_hip.QuantSrc * len(parts))(*[_hip.QuantSrc(t.data_ptr(), t.stride(0), t.shape[1], 0) for t in srcs_d])
    out, sc = Frame(rows, total, 1, ptr_mod16=8), _scales_frame(rows)
    rc = _hip.load().smt_quant_rows_cat_e4m3(srcs, len(parts), rows, out.ptr, out.ld, sc.ptr, _stream())
    _hip._check(rc, "smt_quant_rows_cat_e4m3")
    torch.cuda.synchronize()
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=np.concatenate(parts, axis=1), scales=s)


# ----------------------------------------------------------------------------- quant_cols_t

@pytest.mark.parametrize("rows,cols", R.COLS_T_CASES)
@pytest.mark.parametrize("select", [False, True])
def test_quant_cols_t(rows, cols, select):
    w = R.cols_t_case(rows, cols)
    q, s = R.quant_cols_t(w)
    assert s[5] == 1.0 and not q[5].any()
    nb = cols // 256
    sel = ([2, 0] if nb == 3 else [nb - 1]) if select else None      # [2, 0]: block 1 untouched
    out, sc = Frame(cols, rows, 1, pad=16), _scales_frame(cols)
    s = s.view(np.uint32).copy()
    if sel is not None:
        for b in set(range(nb)) - set(sel):
            q[256 * b:256 * (b + 1)] = out.sent
            s[256 * b:256 * (b + 1)] = sc.sent
    wd = _bf16_in(w, pad=8)
    blocks = None if sel is None else torch.tensor(sel, dtype=torch.int32, device=DEV)
    assert out.ptr % 16 == 0 and out.ld % 16 == 0 and out.ld > rows and wd.stride(0) > cols
    rc = _hip.load().smt_quant_cols_t_e4m3(wd.data_ptr(), wd.stride(0), rows, cols,
                                           None if blocks is None else blocks.data_ptr(),
                                           0 if blocks is None else blocks.numel(), out.ptr, out.ld, sc.ptr, _stream())
    _hip._check(rc, "smt_quant_cols_t_e4m3")
    torch.cuda.synchronize()
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=np.ascontiguousarray(w.T))


# ----------------------------------------------------------------------------- fused producers

def _cpu_quant_of(frame_or_bits):
    bits = frame_or_bits.got() if isinstance(frame_or_bits, Frame) else frame_or_bits
    return bits, R.quant_rows(bits)


@pytest.mark.parametrize("cols", [8, 8192, 8200, 16384])            # CPT 2 up to 8192, CPT 4 up to 16384
def test_swiglu_fwd_quant(cols):
    rows = 3
    rng = np.random.default_rng(cols)
    g = R.random_bits(rng, rows, cols, 1)
    u = R.random_bits(rng, rows, cols)
    u[1] = R.random_bits(rng, 1, cols, -126)[0]                      # a tiny up: the row's amax is below 2^-119
    gd, ud = _bf16_in(g), _bf16_in(u)
    lib = _hip.load()
    h_ref = torch.empty_like(gd)
    assert lib.smt_swiglu_fwd(gd.data_ptr(), ud.data_ptr(), h_ref.data_ptr(), gd.numel(), _hip.DTYPE_BF16,
                              _stream()) == 0
    h_bits, (q, s) = _cpu_quant_of(_dev_bits(h_ref))
    assert 0 < s[1] * 448 < 2.0 ** -119.5                           # 1 / scale overflows fp32
    out, sc, h = Frame(rows, cols, 1), _scales_frame(rows), Frame(rows, cols, 2, pad=0)
    _hip._check(lib.smt_swiglu_fwd_quant_e4m3(gd.data_ptr(), ud.data_ptr(), rows, cols, out.ptr, out.ld, sc.ptr,
                                              h.ptr, _stream()), "smt_swiglu_fwd_quant_e4m3")
    torch.cuda.synchronize()
    h.check(h_bits, "h (bf16) against smt_swiglu_fwd")
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=h_bits, scales=s)
    out2, sc2 = Frame(rows, cols, 1), _scales_frame(rows)            # the bf16 output not requested
    _hip._check(lib.smt_swiglu_fwd_quant_e4m3(gd.data_ptr(), ud.data_ptr(), rows, cols, out2.ptr, out2.ld, sc2.ptr,
                                              None, _stream()), "smt_swiglu_fwd_quant_e4m3")
    torch.cuda.synchronize()
    sc2.check(s, "scales (no h)")
    out2.check(q, "bytes (no h)", x_bits=h_bits, scales=s)


def _swiglu_bwd_inputs(rows, cols):
    rng = np.random.default_rng(cols + 7)
    g = R.random_bits(rng, rows, cols, 1)
    u = R.random_bits(rng, rows, cols)
    dh = R.random_bits(rng, rows, cols, -9)
    dh[1] = R.random_bits(rng, 1, cols, -128)[0]                     # a tiny dh: the row's amax is below 2^-119
    gd, ud, dhd = _bf16_in(g), _bf16_in(u), _bf16_in(dh)
    dg, du = torch.empty_like(gd), torch.empty_like(ud)
    assert _hip.load().smt_swiglu_bwd(gd.data_ptr(), ud.data_ptr(), dhd.data_ptr(), dg.data_ptr(), du.data_ptr(),
                                      gd.numel(), _hip.DTYPE_BF16, _stream()) == 0
    dg, du = _dev_bits(dg), _dev_bits(du)
    q, s = R.quant_rows_cat([dg, du])
    assert 0 < s[1] * 448 < 2.0 ** -119.5
    return gd, ud, dhd, dg, du, q, s


@pytest.mark.parametrize("cols", [8, 8192, 8200, 16384])
def test_swiglu_bwd_quant(cols):
    rows = 3
    gd, ud, dhd, dg, du, q, s = _swiglu_bwd_inputs(rows, cols)
    both = np.concatenate([dg, du], axis=1)
    for want_g, want_u in ((True, True), (True, False), (False, True), (False, False)):
        out, sc = Frame(rows, 2 * cols, 1), _scales_frame(rows)
        fg, fu = Frame(rows, cols, 2, pad=0), Frame(rows, cols, 2, pad=0)
        rc = _hip.load().smt_swiglu_bwd_quant_e4m3(gd.data_ptr(), ud.data_ptr(), dhd.data_ptr(), rows, cols, out.ptr,
                                                   out.ld, sc.ptr, fg.ptr if want_g else None,
                                                   fu.ptr if want_u else None, _stream())
        _hip._check(rc, "smt_swiglu_bwd_quant_e4m3")
        torch.cuda.synchronize()
        tag = f" (grad_gate {want_g}, grad_up {want_u})"
        fg.check(dg if want_g else np.full_like(dg, fg.sent), "grad_gate (bf16) against smt_swiglu_bwd" + tag)
        fu.check(du if want_u else np.full_like(du, fu.sent), "grad_up (bf16) against smt_swiglu_bwd" + tag)
        sc.check(s, "scales" + tag)
        out.check(q, "bytes" + tag, x_bits=both, scales=s)


@pytest.mark.parametrize("cols", [256, 8192, 16384])
def test_swiglu_bwd_quant_packed(cols):
    """A position map that reorders and skips 256-column blocks: only the mapped blocks are written,
    where the map says; the e4m3 rows do not change."""
    rows = 3
    gd, ud, dhd, dg, du, q, s = _swiglu_bwd_inputs(rows, cols)
    nb = cols // 256
    gpos = np.full(nb, -1, dtype=np.int32)
    gpos[nb - 1] = 0                                                 # the last block first,
    if nb > 1:
        gpos[0], gpos[nb // 2] = 2, 1                                # then a middle one, then the first
    upos = np.full(nb, -1, dtype=np.int32)
    upos[nb // 3] = 0
    out, sc = Frame(rows, 2 * cols, 1), _scales_frame(rows)
    ng = int((gpos >= 0).sum())
    fg, fu = Frame(rows, 256 * ng, 2, pad=8), Frame(rows, 256, 2, pad=8)
    gp, up = torch.from_numpy(gpos).to(DEV), torch.from_numpy(upos).to(DEV)
    rc = _hip.load().smt_swiglu_bwd_quant_e4m3_packed(gd.data_ptr(), ud.data_ptr(), dhd.data_ptr(), rows, cols, out.ptr,
                                                      out.ld, sc.ptr, fg.ptr, gp.data_ptr(), fg.ld, fu.ptr,
                                                      up.data_ptr(), fu.ld, _stream())
    _hip._check(rc, "smt_swiglu_bwd_quant_e4m3_packed")
    torch.cuda.synchronize()
    want_g = np.empty((rows, 256 * ng), dtype=np.uint16)
    for b in range(nb):
        if gpos[b] >= 0:
            want_g[:, 256 * gpos[b]:256 * (gpos[b] + 1)] = dg[:, 256 * b:256 * (b + 1)]
    b = nb // 3
    fg.check(want_g, "packed grad_gate")
    fu.check(du[:, 256 * b:256 * (b + 1)], "packed grad_up")
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=np.concatenate([dg, du], axis=1), scales=s)


@pytest.mark.parametrize("tiny_w", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("H", [1024, 2048, 4096, 8192])              # CPL 2, 4, 8, 16
def test_rmsnorm_quant(H, residual, tiny_w):
    rows, eps = 5, 1e-5
    rng = np.random.default_rng(H + residual)
    x = R.random_bits(rng, rows, H, 1)
    w = R.random_bits(rng, 1, H, -126 if tiny_w else 0)              # a tiny w: every row's amax is below 2^-119
    xd, wd = _bf16_in(x, pad=8), _bf16_in(w)                         # a row-strided x
    rd = _bf16_in(R.random_bits(rng, rows, H)) if residual else None
    lib, st = _hip.load(), _stream()
    y_ref = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    h_ref = torch.empty_like(y_ref)
    rstd_ref = torch.empty(rows, device=DEV)
    if residual:
        assert lib.smt_add_rmsnorm_fwd(xd.data_ptr(), xd.stride(0), rd.data_ptr(), H, wd.data_ptr(), h_ref.data_ptr(),
                                       H, y_ref.data_ptr(), H, rstd_ref.data_ptr(), rows, H, eps, _hip.DTYPE_BF16,
                                       st) == 0
    else:
        assert lib.smt_rmsnorm_fwd(xd.data_ptr(), xd.stride(0), wd.data_ptr(), y_ref.data_ptr(), H, rstd_ref.data_ptr(),
                                   rows, H, eps, _hip.DTYPE_BF16, st) == 0
    y_bits, (q, s) = _cpu_quant_of(_dev_bits(y_ref))
    if tiny_w:
        assert 0 < (s * 448).max() < 2.0 ** -119.5
    rstd_bits = rstd_ref.cpu().numpy()
    for need_y in (True, False):
        out, sc, fr = Frame(rows, H, 1), _scales_frame(rows), _scales_frame(rows)
        fy, fh = Frame(rows, H, 2), Frame(rows, H, 2)
        rc = lib.smt_rmsnorm_fwd_quant_e4m3(xd.data_ptr(), xd.stride(0), rd.data_ptr() if residual else None,
                                            H if residual else 0, wd.data_ptr(), fh.ptr if residual else None, fh.ld,
                                            fy.ptr if need_y else None, fy.ld, fr.ptr, out.ptr, out.ld, sc.ptr, rows, H,
                                            eps, st)
        _hip._check(rc, "smt_rmsnorm_fwd_quant_e4m3")
        torch.cuda.synchronize()
        tag = f" (need_y {need_y})"
        fr.check(rstd_bits, "rstd" + tag)
        fy.check(y_bits if need_y else np.full_like(y_bits, fy.sent), "y (bf16) against the unfused norm" + tag)
        fh.check(_dev_bits(h_ref) if residual else np.full_like(y_bits, fh.sent), "h (bf16)" + tag)
        sc.check(s, "scales" + tag)
        out.check(q, "bytes" + tag, x_bits=y_bits, scales=s)


@pytest.mark.parametrize("H", [1024, 2048, 4096, 8192])
def test_rmsnorm_bwd_add_quant(H):
    rows = 5
    rng = np.random.default_rng(H + 11)
    x, w = R.random_bits(rng, rows, H, 1), R.random_bits(rng, 1, H)
    dy, dres = R.random_bits(rng, rows, H), R.random_bits(rng, rows, H)
    for r in (1, 3):                                                 # tiny dy and dres: the rows' amax is below 2^-119
        dy[r], dres[r] = R.random_bits(rng, 1, H, -126)[0], R.random_bits(rng, 1, H, -126)[0]
    xd, wd, dyd, drd = _bf16_in(x, pad=8), _bf16_in(w), _bf16_in(dy, pad=16), _bf16_in(dres, pad=8)
    rstd = (torch.rand(rows, generator=torch.Generator().manual_seed(H)) + 0.5).to(DEV)
    lib, st = _hip.load(), _stream()
    dx_ref = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    assert lib.smt_rmsnorm_bwd_add(dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), wd.data_ptr(),
                                   rstd.data_ptr(), drd.data_ptr(), drd.stride(0), dx_ref.data_ptr(), H, rows, H,
                                   _hip.DTYPE_BF16, st) == 0
    dx_bits, (q, s) = _cpu_quant_of(_dev_bits(dx_ref))
    assert 0 < (s[[1, 3]] * 448).max() < 2.0 ** -119.5
    out, sc, fdx = Frame(rows, H, 1), _scales_frame(rows), Frame(rows, H, 2)
    rc = lib.smt_rmsnorm_bwd_add_quant_e4m3(dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), wd.data_ptr(),
                                            rstd.data_ptr(), drd.data_ptr(), drd.stride(0), fdx.ptr, fdx.ld, out.ptr,
                                            out.ld, sc.ptr, rows, H, st)
    _hip._check(rc, "smt_rmsnorm_bwd_add_quant_e4m3")
    torch.cuda.synchronize()
    fdx.check(dx_bits, "dx (bf16) against smt_rmsnorm_bwd_add")
    sc.check(s, "scales")
    out.check(q, "bytes", x_bits=dx_bits, scales=s)


# ----------------------------------------------------------------------------- GEMM seams

def _u8(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.uint8).cpu().numpy()


ALIGN_BITS = 13          # an instruction keeps the bits of its products down to 2^(emax - 13) (see the header)


def _seam(name, y, a8, sa, b8, sb):
    """Every element of the bf16 result ``y [M, N]`` against the fp64 product of the operands the call
    used (``a8 [M, K]``, ``b8 [N, K]`` e4m3 with their scales), within the derived bound."""
    a8, b8 = _u8(a8), _u8(b8)
    sa, sb = sa.cpu().numpy().astype(np.float64).reshape(-1), sb.cpu().numpy().astype(np.float64).reshape(-1)
    A, B = R.e4m3_decode(a8), R.e4m3_decode(b8)
    K = A.shape[1]
    ss = sa[:, None] * sb[None, :]
    v = (A @ B.T) * ss
    got = y.double().cpu().numpy().reshape(v.shape)
    err = np.abs(got - v)
    # one bf16 rounding: half a step of the 8-bit significand in the binade of the result
    big = np.maximum(np.maximum(np.abs(v), np.abs(got)), 2.0 ** -126)
    t_bf16 = np.exp2(np.floor(np.log2(big)) - 8)
    # the fp32 chain over the instructions' partial sums and the two scale multiplies
    t_fp32 = (K + 4) * 2.0 ** -24 * ss * (np.abs(A) @ np.abs(B).T)
    # inside an instruction: a product (7 significant bits) loses what lies below 2^(emax - ALIGN_BITS)
    t_align = np.empty_like(v)
    for i in range(A.shape[0]):
        p = np.abs(A[i][None, :] * B).astype(np.float32)                    # [N, K], exact
        pmax = np.maximum(p.max(axis=1, keepdims=True), np.float32(2.0 ** -60))
        emax = np.floor(np.log2(pmax))
        cut = np.exp2(emax - ALIGN_BITS)
        lossy = p < np.exp2(emax - ALIGN_BITS + 7)                          # its last bit lies below the cut
        t_align[i] = (np.minimum(p, cut) * lossy).sum(axis=1, dtype=np.float64)
    t_align *= ss
    bound = t_bf16 + t_fp32 + t_align
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    past = np.maximum(err - t_bf16, 0) / np.where(t_fp32 + t_align > 0, t_fp32 + t_align, 1)
    i2, j2 = np.unravel_index(np.argmax(past), past.shape)
    print(f"seam {name}: worst err / bound = {ratio[i, j]:.3f} at ({i}, {j}): v = {v[i, j]:.6g}, "
          f"err = {err[i, j]:.3g}, "
          f"bound = {t_bf16[i, j]:.3g} (bf16) + {t_fp32[i, j]:.3g} (fp32 chain) + {t_align[i, j]:.3g} (alignment); "
          f"worst (err - bf16 term) / (fp32 chain + alignment) = {past[i2, j2]:.3f} at ({i2}, {j2}); "
          f"against the issue's 2^-9 |v| + fp32 chain: {(err / (2.0 ** -9 * np.abs(v) + t_fp32 + 1e-300)).max():.3f}")
    bad = np.argwhere(~(err <= bound))
    assert len(bad) == 0, f"{name}: {len(bad)} elements outside the bound, first {tuple(bad[0])}"
    return float(ratio[i, j])


def _seam_operands(M=96, K=512, outs=(256,), seed=0, w_row=None, w_col=None):
    """x [M, K] and W_i [out_i, K]. Row 7 of x and one row (``w_row``: the forward's per-row scales) or
    one column (``w_col``: the data gradient's per-column scales) of each W are 2^10 larger than their
    neighbours, so a scale vector paired with the wrong row or column shows at once."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[7] *= 1024
    ws = []
    for o in outs:
        w = torch.randn(o, K, generator=g) * 0.05
        if w_row is not None:
            w[w_row] *= 1024
        if w_col is not None:
            w[:, w_col] *= 1024
        ws.append(w.bfloat16().to(DEV))
    return x.bfloat16().to(DEV), ws


def test_seam_linear_forward_and_dgrad():
    x, (W,) = _seam_operands(w_row=11)
    fw = f8.Fp8Weight(W)
    y = f8.fp8_linear_forward(x, fw)
    _v, x8, sx = x._smt_q8                                            # the rows the call quantised and used
    assert sx[7] > 256 * sx[6] and fw.sw[11] > 256 * fw.sw[10]
    _seam("forward", y, x8, sx, fw.w8, fw.sw)
    _x, (W,) = _seam_operands(seed=1, w_col=13)
    fw = f8.Fp8Weight(W)
    dy = torch.randn(96, 256, generator=torch.Generator().manual_seed(1))
    dy[5] *= 1024
    dy = dy.bfloat16().to(DEV)
    gi = f8.fp8_linear_dgrad(dy, fw)
    _v, g8, sg = dy._smt_q8
    assert sg[5] > 256 * sg[4] and fw.swt[13] > 256 * fw.swt[12]
    _seam("dgrad", gi, g8, sg, fw.wt8, fw.swt)


def _spy(monkeypatch, name):
    calls, real = [], getattr(f8, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        calls.append(out)
        return out
    monkeypatch.setattr(f8, name, wrapped)
    return calls


def test_seam_group_joint_dgrad_from_quant_rows_cat(monkeypatch):
    x, ws = _seam_operands(outs=(256, 128, 128), seed=2, w_col=13)              # a q/k/v-shaped group
    grp = f8.Fp8Group(ws)
    fws = [f8.Fp8Weight(w, grp, i) for i, w in enumerate(ws)]
    xr = x.view(1, 96, 512).clone().requires_grad_()
    ys = [f8.Fp8LinearFn.apply(xr, w, fw, None) for w, fw in zip(ws, fws)]
    gen = torch.Generator().manual_seed(3)
    dys = []
    for y in ys:
        d = torch.randn(y.shape, generator=gen)
        d[0, 5] *= 1024
        dys.append(d.bfloat16().to(DEV))
    calls = _spy(monkeypatch, "quant_rows_cat")
    torch.autograd.backward(ys, dys)
    assert len(calls) == 1                                           # ONE joint GEMM on the concatenated rows
    q, sq = calls[0]
    assert q.shape == (96, 512) and grp.swt[13] > 256 * grp.swt[12]
    _seam("group dgrad (quant_rows_cat)", xr.grad, q, sq, grp.wt8, grp.swt)


def test_seam_group_joint_dgrad_from_swiglu_rows(monkeypatch):
    from sparse_matrix_tuning_amd.fused_llama import FusedSwiGLUFn
    x, ws = _seam_operands(outs=(512, 512), seed=4, w_col=13)                  # a gate/up-shaped group
    grp = f8.Fp8Group(ws)
    fws = [f8.Fp8Weight(w, grp, i) for i, w in enumerate(ws)]
    xr = x.view(1, 96, 512).clone().requires_grad_()
    dh = torch.randn(1, 96, 512, generator=torch.Generator().manual_seed(5))
    dh[0, 5] *= 1024
    dh = dh.bfloat16().to(DEV)
    calls = _spy(monkeypatch, "swiglu_bwd_quant")
    assert f8.FUSED_SWIGLU_QUANT
    with f8.sole_swiglu_consumer():
        gate = f8.Fp8LinearFn.apply(xr, ws[0], fws[0], None)
        up = f8.Fp8LinearFn.apply(xr, ws[1], fws[1], None)
    assert f8.swiglu_group(gate, up) is not None
    FusedSwiGLUFn.apply(gate, up).backward(dh)
    assert len(calls) == 1                                           # the SwiGLU backward's own e4m3 rows
    q, sq = calls[0][0], calls[0][1]
    assert q.shape == (96, 1024) and grp.swt[13] > 256 * grp.swt[12]
    _seam("group dgrad (SwiGLU rows)", xr.grad, q, sq, grp.wt8, grp.swt)
