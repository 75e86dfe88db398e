"""The per-element bar on the smt_flash attention kernels ("The bar on attention"): every element
of o, dq, dk, dv and lse against tests/attn_ref.py::ref64_bounds, an fp64 reference that carries a derived
elementwise error bound, through assert_within_bounds, which excuses no element and holds the rows and keys
a mask makes dead to exact zeros (lse: +inf). Everything goes through the public entry points
(flash_attention, flash_attention_cached with a host or a device position, flash_attention_beams), and once
through the C ABI with output windows of the test's own.

The shapes are the smallest that reach each structural edge of csrc/attn_kernels.hip: q blocks of 128 rows
as 4 waves x 32, 64-key tiles in ring-slot pairs, the paired q blocks (nblk - 1 - p, p) of dQ, dK/dV key
blocks of 256 as 8 waves x 32, 32-row Q / dO slices in a ring of 2, 16-byte lse / delta groups. S = 320 is 5
tiles, 3 q blocks (a pair and a single) and 2 key blocks, the second ragged; 333 adds S % 4 != 0 and a
ragged last wave. Each test prints its worst err / bound per output (DESIGN.md records them; they are no
thresholds)."""
import ctypes

import pytest
import torch

from sparse_matrix_tuning_amd import _hip, fused_llama as fl
from sparse_matrix_tuning_amd.fused_llama import (DocMask, KeyMask, dropout_effective_p, flash_attention,
                                                  flash_attention_beams, flash_attention_cached, flash_dropout_mask)
from tests.attn_ref import (D, DEV, allowed_cached, allowed_causal, allowed_docs, check_outputs, inputs, ref64_bounds)

pytestmark = pytest.mark.gpu
SCALE = D ** -0.5
BF16, FP16 = torch.bfloat16, torch.float16
P_DROP, SEED = 0.1, 2 ** 40 + 17


def _inputs(B, Hq, Hkv, S, layout, dtype, kind):
    q, k, v, g = inputs(B, Hq, Hkv, S, layout, dtype, 7 * S + Hq)
    if kind == "flat":                      # a stray or a missing key carries weight
        q = (q.detach().float() * 0.25).to(dtype).requires_grad_(True)
    elif kind == "peaked":
        # every query shares a positive direction and one late key lies along it: its score beats every
        # earlier one by ~24 log2 units (> kFwdThr), so the rows past it move their deferred max after
        # the first tiles
        q = (q.detach().float() * 0.25 + 0.5).to(dtype).requires_grad_(True)
        k = k.detach().clone()
        k[:, :, min(200, S - 1)] = 3.0
        k.requires_grad_(True)
    return q, k, v, g


def _keep(B, S):
    """Right padding, holes, and leading masked keys (row 0's first queries see nothing)."""
    keep = torch.ones(B, S, dtype=torch.bool, device=DEV)
    keep[0, :min(3, S - 1)] = False
    keep[0, S - S // 3:] = False
    for j in (5, 64, 100, 257):
        if j < S:
            keep[B - 1, j] = False
    keep[B - 1, S // 2 + 7:] = False
    return keep


# Document lengths per batch row. Row 0: boundaries off the 64 grid, a length-1 document, waves whose rows
# straddle two documents (rows 64..95 around 70). Row 1 at S >= 320: every row of q block 1 (and the first
# rows of q block 2) belongs to the document that starts at 100, so those workgroups' first visible tile is
# tile 1, an odd one (the `t0 & 1` path).
DOCS = {65: [[64, 1], [30, 35]], 130: [[70, 1, 59], [100, 30]], 320: [[70, 1, 59, 100, 90], [100, 160, 60]],
        333: [[70, 1, 59, 100, 103], [100, 160, 73]]}


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _variant(name, B, Hq, S):
    """flash_attention's keyword arguments and the reference's allowed, M, r."""
    kw, M, r = {}, None, 1.0
    if "kmask" in name:
        keep = _keep(B, S)
        kw["key_mask"] = KeyMask.from_padding_mask(keep)
        allowed = allowed_causal(S, keep)
    elif "docs" in name:
        rows = [DOCS[S][b % 2] for b in range(B)]
        kw["doc_mask"] = DocMask.from_cu_seqlens([torch.tensor(_cu(r_), device=DEV) for r_ in rows], B, S)
        allowed = allowed_docs(rows, S)
    else:
        allowed = allowed_causal(S)
    if "drop" in name:
        kw.update(dropout_p=P_DROP, seed=SEED)
        M = flash_dropout_mask(B, Hq, S, P_DROP, SEED, DEV)
        r = 1.0 / (1.0 - dropout_effective_p(P_DROP))
    return kw, allowed, M, r


def _train(q, k, v, g, **kw):
    S = q.shape[2]
    o = flash_attention(q, k, v, any_length=True, **kw)
    lse = o.grad_fn.saved_tensors[4][:, :, :S].clone()
    o.backward(g)
    return {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "lse2": lse}


def _case(what, B, Hq, Hkv, S, layout, dtype, kind, name):
    q, k, v, g = _inputs(B, Hq, Hkv, S, layout, dtype, kind)
    kw, allowed, M, r = _variant(name, B, Hq, S)
    got = _train(q, k, v, g, **kw)
    R = ref64_bounds(q, k, v, g, SCALE, allowed, M, r)
    return check_outputs(f"{what} {name} {kind} B{B} Hq{Hq} Hkv{Hkv} S{S} {layout} {str(dtype)[6:]}", got, R)


# ---- training: forward, dQ, dK/dV -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S", [1, 4, 63, 64, 65, 130, 320, 333])
def test_plain(S, dtype):
    _case("train", 2, 4, 2, S, "hf", dtype, "normal", "plain")


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Hq,Hkv,S,layout", [(1, 8, 1, 320, "hf"), (1, 2, 2, 333, "hf"), (2, 4, 2, 333, "contig")],
                         ids=["G8", "G1", "contig"])
def test_head_shapes_and_layout(B, Hq, Hkv, S, layout, dtype):
    _case("train", B, Hq, Hkv, S, layout, dtype, "normal", "plain")


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S", [320, 333])
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_flat_and_peaked_inputs(kind, S, dtype):
    _case("train", 2, 4, 2, S, "hf", dtype, kind, "plain")


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S", [65, 130, 320, 333])
@pytest.mark.parametrize("name,kind", [("kmask", "flat"), ("docs", "flat"), ("drop", "normal"), ("kmask+drop", "flat"),
                                       ("docs+drop", "flat")])
def test_masks_and_dropout(name, kind, S, dtype):
    _case("train", 2, 4, 2, S, "hf", dtype, kind, name)


def test_peaked_under_a_key_mask_and_documents():
    """The deferred max moves inside a masked sweep and inside a document."""
    _case("train", 2, 4, 2, 320, "hf", BF16, "peaked", "kmask")
    _case("train", 2, 4, 2, 333, "hf", FP16, "peaked", "docs")


def test_joint_gradient_buffer():
    """joint=True: dq, dk, dv as slices of one buffer are the separate buffers' bits, and carry the bounds."""
    B, Hq, Hkv, S = 2, 4, 2, 320
    q, k, v, g = _inputs(B, Hq, Hkv, S, "hf", BF16, "normal")
    sep = _train(q, k, v, g)
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    joint = _train(q2, k2, v2, g, joint=True)
    for n in ("o", "dq", "dk", "dv", "lse2"):
        assert torch.equal(sep[n], joint[n]), n
    check_outputs("train joint", joint, ref64_bounds(q, k, v, g, SCALE, allowed_causal(S)))


def test_c_abi_output_windows():
    """smt_attn_fwd_ld / smt_attn_bwd_ld with o, dq, dk, dv as strided windows of NaN-filled buffers and
    lse_ld > S: inside the windows every element is within its bound; outside them, and in [S, lse_ld) of
    lse and delta, nothing is written."""
    B, Hq, Hkv, S = 2, 4, 2, 333
    lse_ld = ((S + 3) & ~3) + 8
    q, k, v, g = (t.detach() for t in _inputs(B, Hq, Hkv, S, "hf", BF16, "normal"))
    nan = float("nan")

    def window(H):
        """A [B, H, S, D] window with a margin on every axis of a NaN-filled [B, S + 2, H + 1, D + 16] buffer."""
        big = torch.full((B, S + 2, H + 1, D + 16), nan, dtype=BF16, device=DEV)
        inside = torch.zeros_like(big, dtype=torch.bool)
        inside[:, 1:S + 1, :H, 8:8 + D] = True
        return big, inside, big[:, 1:S + 1, :H, 8:8 + D].transpose(1, 2)

    (bo, io, o), (bq, iq, dq), (bk, ik, dk), (bv, iv, dv) = window(Hq), window(Hq), window(Hkv), window(Hkv)
    lse = torch.full((B, Hq, lse_ld), nan, dtype=torch.float32, device=DEV)
    delta = torch.full_like(lse, nan)
    lib, T = _hip.load(), lambda t: ctypes.byref(fl._attn_tensor(t))
    shape = _hip.AttnShape(B, Hq, Hkv, S, SCALE, _hip.DTYPE_BF16)
    rc = lib.smt_attn_fwd_ld(T(q), T(k), T(v), T(o), lse.data_ptr(), lse_ld, None, 0, None, None, 0.0, None,
                             ctypes.byref(shape), fl._stream(q))
    _hip._check(rc, "smt_attn_fwd_ld")
    rc = lib.smt_attn_bwd_ld(T(q), T(k), T(v), T(o), T(g.transpose(1, 2)), lse.data_ptr(), delta.data_ptr(), lse_ld,
                             T(dq), T(dk), T(dv), None, 0, None, None, 0.0, None, ctypes.byref(shape), fl._stream(q))
    _hip._check(rc, "smt_attn_bwd_ld")
    for name, big, inside in (("o", bo, io), ("dq", bq, iq), ("dk", bk, ik), ("dv", bv, iv)):
        assert torch.isnan(big[~inside]).all(), f"{name}: written outside its window"
    assert torch.isnan(lse[:, :, S:]).all() and torch.isnan(delta[:, :, S:]).all(), "written into the pad [S, lse_ld)"
    R = ref64_bounds(q, k, v, g, SCALE, allowed_causal(S))
    check_outputs("C ABI windows", {"o": o.transpose(1, 2), "dq": dq, "dk": dk, "dv": dv, "lse2": lse[:, :, :S]}, R)
    # delta = rowsum(dO * O): the workspace the dK/dV kernel reads, within the bound the model gives it
    assert ((delta[:, :, :S].double() - R.delta).abs() <= R.b_delta).all()


# ---- decode: the split-KV kernel and its combine ----------------------------------------------------------
def _cache(B, Hq, Hkv, Sq, Skv, dtype, seed):
    torch.manual_seed(seed)
    mk = lambda H, S: torch.randn(B, S, H, D, device=DEV).to(dtype).transpose(1, 2)
    return mk(Hq, Sq), mk(Hkv, Skv), mk(Hkv, Skv)


def _cache_keep(B, Skv):
    """Holes, and the whole second 128 keys (Skv = 65: the second tile) of row 0 masked, so that a split of
    the forced counts sees no key through the mask."""
    keep = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
    keep[0, 5] = False
    if Skv > 256:
        keep[0, 128:256] = False
    else:
        keep[0, 64:] = False
        keep[0, 30] = False
    keep[B - 1, 0:2] = False
    keep[B - 1, Skv // 2] = False
    return keep


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("Sq", [1, 3, 40])
@pytest.mark.parametrize("Skv", [65, 333])
def test_cached(Skv, Sq, G, dtype):
    """Sq * G below, at and above the 32 columns of a block; 1, 2 and 5 splits (at Skv = 65 two tiles, so 5
    splits leave three without a key; at 333 six tiles in pairs, so two of 5); with and without a key mask."""
    B, Hkv = 2, 2
    q, k, v = _cache(B, Hkv * G, Hkv, Sq, Skv, dtype, 1000 * Skv + 10 * Sq + G)
    if Sq == 40 and Skv == 65:
        keep = _cache_keep(B, Skv)
        keep[0, 64:] = True                  # q_offset = 25: the queries' own keys stay (no row without a key here)
        keep[0, 26:64] = False               # ... and the first tile's tail goes instead
    else:
        keep = _cache_keep(B, Skv)
    for masked in (False, True):
        al = allowed_cached(B, Sq, Skv, Skv - Sq, keep if masked else None)
        R = ref64_bounds(q, k, v, None, SCALE, al)
        km = KeyMask.from_padding_mask(keep) if masked else None
        for ns in (1, 2, 5):
            o, lse = flash_attention_cached(q, k, v, key_mask=km, num_splits=ns, return_lse=True)
            check_outputs(f"cached Skv{Skv} Sq{Sq} G{G} {str(dtype)[6:]} mask {masked} splits {ns}", {"o": o, "lse2": lse}, R)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_cached_rows_without_a_key(dtype):
    """A key mask that hides every key a row's first queries see: o == 0 and lse == +inf there, whatever
    the split count."""
    B, Hq, Hkv, Sq, Skv = 2, 8, 2, 3, 130
    q, k, v = _cache(B, Hq, Hkv, Sq, Skv, dtype, 5)
    keep = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
    keep[1, :Skv - 1] = False                # row 1: queries 0 and 1 see nothing, query 2 its own key only
    al = allowed_cached(B, Sq, Skv, Skv - Sq, keep)
    R = ref64_bounds(q, k, v, None, SCALE, al)
    assert not R.visible[1, :, :2].any() and R.visible[1, :, 2].all() and R.visible[0].all()
    for ns in (1, 2, 5):
        o, lse = flash_attention_cached(q, k, v, key_mask=KeyMask.from_padding_mask(keep), num_splits=ns, return_lse=True)
        check_outputs(f"cached dead rows {str(dtype)[6:]} splits {ns}", {"o": o, "lse2": lse}, R)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_cached_device_positions(dtype):
    """The device-position form with a different position per batch row, in a cache of capacity 333."""
    B, Hq, Hkv, Sq, cap = 2, 8, 2, 3, 333
    q, k, v = _cache(B, Hq, Hkv, Sq, cap, dtype, 6)
    pos = torch.tensor([100, cap - Sq], dtype=torch.int64, device=DEV)
    keep = _cache_keep(B, cap)
    for masked in (False, True):
        R = ref64_bounds(q, k, v, None, SCALE, allowed_cached(B, Sq, cap, pos, keep if masked else None))
        km = KeyMask.from_padding_mask(keep) if masked else None
        for ns in (1, 2, 5):
            o, lse = flash_attention_cached(q, k, v, key_mask=km, q_offset=pos, num_splits=ns, return_lse=True)
            check_outputs(f"cached device positions {str(dtype)[6:]} mask {masked} splits {ns}", {"o": o, "lse2": lse}, R)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_beams(dtype):
    """nb = 3, a prompt of 70, 5 generated steps with a random ancestry, against the gathered cache under
    the mask tests/test_gpu_attention_beams.py builds; with and without a left-padded prompt mask."""
    from tests.test_gpu_attention_beams import N, _case as beam_case, _gather, _keep as beam_keep
    Hq, Hkv, nb, P, T = 8, 2, 3, 70, 5
    q, kp, vp, kg, vg, anc = beam_case(Hq, Hkv, nb, P, T, dtype=dtype)
    k, v = _gather(kp, vp, kg, vg, anc, nb, P, T)
    pk = torch.ones(N, P, dtype=torch.bool, device=DEV)
    pk[1, :9] = False                        # sample 1 is left-padded
    pk[0, 40] = pk[1, 66] = False
    tiles = -(-P // 64) + nb * -(-T // 64)
    for prompt_keep in (None, pk):
        keep = beam_keep(anc, nb, P, T, prompt_keep)
        R = ref64_bounds(q, k, v, None, SCALE, keep[:, None, None, :], tiles=tiles)
        km = KeyMask.from_padding_mask(prompt_keep) if prompt_keep is not None else None
        for ns in (None, 1, 3):
            o, lse = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, prompt_key_mask=km, num_splits=ns,
                                           return_lse=True)
            check_outputs(f"beams {str(dtype)[6:]} mask {prompt_keep is not None} splits {ns}",
                          {"o": o, "lse2": lse[..., None]}, R)
