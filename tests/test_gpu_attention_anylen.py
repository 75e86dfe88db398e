"""Any sequence length in the gfx950 flash attention: fused_llama.flash_attention(any_length=True), C ABI
include/smt_attention.h ``smt_attn_fwd_ld`` / ``smt_attn_bwd_ld`` (lse and delta with a row stride of
their own), and what a ``patch_llama``'d model does with the reference collator's batches, whose length
is the longest sample's (deepspeed/helpers/helper.py:191-205).

Lengths: the smallest at which each structure of the kernels first meets a length that is not a multiple
of 4. 1, 3: shorter than one 16-byte lse group; 33: one row into the second 32-row dK/dV slice and the
forward's second wave; 66: one 64-key tile plus two; 130: two rows into a second 128-row query block; 259:
three keys into a second 256-key dK/dV block (paired with block 0); 517: three key blocks, S % 4 == 1.

References and bars are those of the tests of the S % 4 == 0 paths: tests/test_gpu_attention.py (plain and
key mask), tests/test_gpu_attention_dropout.py, tests/test_gpu_attention_packed.py,
tests/test_gpu_fused_llama.py::test_patched_mini_llama_matches_eager and tests/test_gpu_parity.py's
end-to-end mini LLaMA."""
import ctypes
from collections import defaultdict

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from sparse_matrix_tuning_amd.fused_llama import (DocMask, KeyMask, dropout_effective_p, flash_attention,
                                                  flash_dropout_mask, smt_flash_attention_forward, smt_flash_mask)
from tests import test_gpu_attention as plain
from tests import test_gpu_attention_packed as pref
from tests.attn_ref import (D, DEV, allowed_causal, allowed_docs, check_outputs, eager16, inputs, ref32, ref64_bounds,
                            rel as _rel)

pytestmark = pytest.mark.gpu
LENGTHS = [1, 3, 33, 66, 130, 259, 517]


def _inputs(B, Hq, Hkv, S, layout="hf", dtype=torch.bfloat16, seed=0):
    return inputs(B, Hq, Hkv, S, layout, dtype, seed + S + Hq)


def _per_element(what, o, lse, dq, dk, dv, R):
    """Beside the Frobenius bars: every element within its derived bound (DESIGN, "The bar on attention")."""
    check_outputs(what, {"o": o, "dq": dq, "dk": dk, "dv": dv, "lse2": lse}, R)


def _run(q, k, v, g, **kw):
    """(o, lse[:, :, :S], dq, dk, dv) of flash_attention on fresh leaves."""
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    if q.stride(1) != qs.stride(1):                      # clone() of a transposed view keeps its strides; be sure
        raise AssertionError("layout lost")
    o = flash_attention(qs, ks, vs, **kw)
    lse = o.grad_fn.saved_tensors[4]
    S = q.shape[2]
    assert lse.shape == (q.shape[0], q.shape[1], (S + 3) & ~3)
    lse = lse[:, :, :S].clone()
    o.backward(g)
    assert qs.grad.stride() == qs.stride() and ks.grad.stride() == ks.stride()
    return o.detach(), lse, qs.grad, ks.grad, vs.grad


@pytest.mark.parametrize("B,Hq,Hkv,S,layout,dtype",
                         [(2, 4, 2, S, lay, torch.bfloat16) for S in LENGTHS for lay in ("contig", "hf")]
                         + [(1, 8, 1, 259, "contig", torch.bfloat16), (1, 8, 1, 259, "hf", torch.bfloat16),
                            (2, 4, 2, 130, "hf", torch.float16)])
def test_any_length_matches_fp32_reference(B, Hq, Hkv, S, layout, dtype):
    q, k, v, g = _inputs(B, Hq, Hkv, S, layout, dtype)
    o, lse, dq, dk, dv = _run(q, k, v, g, any_length=True)
    assert o.shape == (B, S, Hq, D) and o.dtype == dtype
    ro, rdq, rdk, rdv, rlse = plain._ref(q, k, v, g, D ** -0.5)
    so, sdq, sdk, sdv = plain._sdpa_bf16(q, k, v, g)
    for name, mine, sdpa, ref in (("o", o, so, ro), ("dq", dq, sdq, rdq), ("dk", dk, sdk, rdk), ("dv", dv, sdv, rdv)):
        e, es = _rel(mine, ref), _rel(sdpa, ref)
        print(f"S {S} {name}: rel err {e:.3e} (sdpa {es:.3e})")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= max(8e-3, 1.5 * es), (name, e, es)
    assert (lse - rlse).abs().max().item() < 2e-3
    _per_element(f"S {S} {layout}", o, lse, dq, dk, dv, ref64_bounds(q, k, v, g, D ** -0.5, allowed_causal(S)))


@pytest.mark.parametrize("S", [66, 259])
def test_any_length_key_mask(S):
    """Holes, right padding and a fully masked prefix (rows without a key: o = 0, zero gradients)."""
    B, Hq, Hkv = 2, 4, 2
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=1)
    keep = torch.ones(B, S, dtype=torch.bool, device=DEV)
    keep[0, S - S // 3:] = False                        # right padding
    keep[0, 5] = keep[0, 40] = False                    # holes
    keep[1, 0:3] = False                                # queries 0-2 see no key
    keep[1, S - 1] = False                              # the very last key
    km = smt_flash_mask(B, S, S, attention_mask=keep.long())
    assert isinstance(km, KeyMask)
    o, lse, dq, dk, dv = _run(q, k, v, g, key_mask=km, any_length=True)
    ro, rdq, rdk, rdv, rlse, visible = ref32(q, k, v, g, D ** -0.5, allowed_causal(S, keep))
    for name, mine, ref in (("o", o, ro), ("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        e = _rel(mine, ref)
        print(f"S {S} {name}: rel err {e:.3e}")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= 8e-3, (name, e)
    vis = visible.expand_as(rlse)
    assert (lse[vis] - rlse[vis]).abs().max().item() < 2e-3
    assert torch.isinf(lse[~vis]).all() and (lse[~vis] > 0).all()
    assert not vis[1, :, :3].any() and (o[1, :3].float() == 0).all() and (dq[1, :, :3].float() == 0).all()
    dead = ~keep[:, None, :, None].expand(B, Hkv, S, D)
    assert (dk.float()[dead] == 0).all() and (dv.float()[dead] == 0).all()
    _per_element(f"S {S} key mask", o, lse, dq, dk, dv, ref64_bounds(q, k, v, g, D ** -0.5, allowed_causal(S, keep)))


@pytest.mark.parametrize("S", [66, 259])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_any_length_dropout(S, p):
    B, Hq, Hkv = 2, 4, 2
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=2)
    seed = (S << 33) + 17 * Hq + 3
    o, lse, dq, dk, dv = _run(q, k, v, g, dropout_p=p, seed=seed, any_length=True)
    M = flash_dropout_mask(B, Hq, S, p, seed, DEV)
    r = 1.0 / (1.0 - dropout_effective_p(p))
    ro, rdq, rdk, rdv, rlse, vis = ref32(q, k, v, g, D ** -0.5, allowed_causal(S), M, r)
    eo, edq, edk, edv = eager16(q, k, v, g, D ** -0.5, allowed_causal(S), M, r)
    for name, mine, eager, ref in (("o", o, eo, ro), ("dq", dq, edq, rdq), ("dk", dk, edk, rdk), ("dv", dv, edv, rdv)):
        e, es = _rel(mine, ref), _rel(eager, ref)
        print(f"S {S} p {p} {name}: rel err {e:.3e} (16-bit eager {es:.3e})")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= max(8e-3, 1.5 * es), (name, e, es)
    assert (lse - rlse).abs().max().item() < 2e-3       # lse is untouched by dropout
    _per_element(f"S {S} p {p}", o, lse, dq, dk, dv, ref64_bounds(q, k, v, g, D ** -0.5, allowed_causal(S), M, r))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_does_not_depend_on_the_length(p):
    seed = 2 ** 35 + 77
    a = flash_dropout_mask(2, 4, 66, p, seed, DEV)
    b = flash_dropout_mask(2, 4, 68, p, seed, DEV)
    assert torch.equal(a, b[:, :, :66, :66])


@pytest.mark.parametrize("S,rows", [(66, [[7, 59]]), (259, [[100, 158, 1]])])
def test_any_length_documents(S, rows):
    B, Hq, Hkv = len(rows), 4, 2
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=3)
    dm = pref._doc_mask(rows, S)
    assert isinstance(dm, DocMask)
    o, lse, dq, dk, dv = _run(q, k, v, g, doc_mask=dm, any_length=True)
    allowed = allowed_docs(rows, S)
    ro, rdq, rdk, rdv, rlse, _ = ref32(q, k, v, g, D ** -0.5, allowed)
    eo, edq, edk, edv = eager16(q, k, v, g, D ** -0.5, allowed)
    for name, mine, eager, ref in (("o", o, eo, ro), ("dq", dq, edq, rdq), ("dk", dk, edk, rdk), ("dv", dv, edv, rdv)):
        e, es = _rel(mine, ref), _rel(eager, ref)
        print(f"S {S} {name}: rel err {e:.3e} (16-bit eager {es:.3e})")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= max(8e-3, 1.5 * es), (name, e, es)
    assert torch.isfinite(lse).all()
    _per_element(f"S {S} documents", o, lse, dq, dk, dv, ref64_bounds(q, k, v, g, D ** -0.5, allowed))
    assert (lse - rlse).abs().max().item() < 2e-3


def test_joint_buffer_is_bit_equal_at_an_odd_length():
    q, k, v, g = _inputs(2, 4, 2, 66, seed=4)
    a = _run(q, k, v, g, any_length=True)
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(qs, ks, vs, joint=True, any_length=True)
    o.backward(g)
    assert torch.equal(o, a[0])
    assert torch.equal(qs.grad, a[2]) and torch.equal(ks.grad, a[3]) and torch.equal(vs.grad, a[4])


def test_any_length_is_the_default_call_at_a_multiple_of_four():
    q, k, v, g = _inputs(2, 4, 2, 68, seed=5)
    strict, relaxed = _run(q, k, v, g), _run(q, k, v, g, any_length=True)
    assert all(torch.equal(a, b) for a, b in zip(strict, relaxed))
    with pytest.raises(NotImplementedError):            # the default still refuses S % 4 != 0
        flash_attention(q[:, :, :66], k[:, :, :66], v[:, :, :66])


# ---- C ABI: the pad [S, lse_ld) of lse and delta -----------------------------------------------------
SENTINEL = -12345.0


def _abi(S, lse_ld, fills, masked, p):
    """smt_attn_fwd_ld, then smt_attn_bwd_ld once per fill of the pads; returns the (dq, dk, dv) of each."""
    B, Hq, Hkv = 2, 4, 2
    q, k, v, g = (t.detach() for t in _inputs(B, Hq, Hkv, S, seed=6))
    lib, T = _hip.load(), fl._attn_tensor
    shape = _hip.AttnShape(B, Hq, Hkv, S, D ** -0.5, _hip.DTYPE_BF16)
    km = None
    if masked:
        keep = torch.ones(B, S, dtype=torch.bool, device=DEV)
        keep[0, S - S // 3:] = False
        keep[1, 0:3] = False
        keep[1, 20] = False
        km = KeyMask.from_padding_mask(keep).bits
    seed = torch.tensor([2 ** 40 + 5], dtype=torch.int64, device=DEV) if p else None
    kmp, kml = (km.data_ptr(), km.shape[1]) if masked else (None, 0)
    o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=DEV)
    lse = torch.full((B, Hq, lse_ld), SENTINEL, dtype=torch.float32, device=DEV)
    rc = lib.smt_attn_fwd_ld(ctypes.byref(T(q)), ctypes.byref(T(k)), ctypes.byref(T(v)),
                             ctypes.byref(T(o.transpose(1, 2))), lse.data_ptr(), lse_ld, kmp, kml, None, None, p,
                             seed.data_ptr() if p else None, ctypes.byref(shape), fl._stream(q))
    _hip._check(rc, "smt_attn_fwd_ld")
    assert (lse[:, :, S:] == SENTINEL).all(), "the forward wrote into the pad"
    assert not (lse[:, :, :S] == SENTINEL).any()
    outs = []
    for fill in fills:
        lse_f = lse.clone()
        lse_f[:, :, S:] = fill
        delta = torch.full_like(lse, fill)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        rc = lib.smt_attn_bwd_ld(ctypes.byref(T(q)), ctypes.byref(T(k)), ctypes.byref(T(v)),
                                 ctypes.byref(T(o.transpose(1, 2))), ctypes.byref(T(g.transpose(1, 2))),
                                 lse_f.data_ptr(), delta.data_ptr(), lse_ld, ctypes.byref(T(dq)), ctypes.byref(T(dk)),
                                 ctypes.byref(T(dv)), kmp, kml, None, None, p, seed.data_ptr() if p else None,
                                 ctypes.byref(shape), fl._stream(q))
        _hip._check(rc, "smt_attn_bwd_ld")
        assert (delta[:, :, S:] == fill).all() or fill != fill, "the backward wrote into delta's pad"
        outs.append((o.clone(), dq, dk, dv))
    return outs


@pytest.mark.parametrize("S", [33, 259])
@pytest.mark.parametrize("masked,p", [(False, 0.0), (True, 0.0), (False, 0.5)])
def test_results_do_not_depend_on_the_pad(S, masked, p):
    ld0 = (S + 3) & ~3
    fills = (0.0, float("nan"), float("inf"))
    runs = _abi(S, ld0, fills, masked, p) + _abi(S, ld0 + 8, fills, masked, p)
    for r in runs:
        for name, t in zip(("o", "dq", "dk", "dv"), r):
            assert torch.isfinite(t.float()).all(), name
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    if not masked and not p:                             # and they are the autograd path's bits
        q, k, v, g = _inputs(2, 4, 2, S, seed=6)
        o, _, dq, dk, dv = _run(q, k, v, g, any_length=True)
        assert all(torch.equal(a, b) for a, b in zip(runs[0], (o, dq, dk, dv)))


# ---- the transformers interface -------------------------------------------------------------------------
def test_interface_with_grad_at_an_odd_length():
    B, Hq, Hkv, S = 2, 4, 2, 37
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=7)
    keep = torch.ones(B, S, dtype=torch.bool, device=DEV)
    keep[1, 21:] = False
    km = smt_flash_mask(B, S, S, attention_mask=keep.long())
    assert isinstance(km, KeyMask)
    o, _ = smt_flash_attention_forward(None, q, k, v, km)
    o.backward(g)
    ro, rdq, rdk, rdv, _, _ = ref32(q, k, v, g, D ** -0.5, allowed_causal(S, keep))
    for name, mine, ref in (("o", o, ro), ("dq", q.grad, rdq), ("dk", k.grad, rdk), ("dv", v.grad, rdv)):
        assert _rel(mine, ref) <= 8e-3, (name, _rel(mine, ref))
    # packed rows
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=8)
    rows = [[10, 27], [37]]
    o, _ = smt_flash_attention_forward(None, q, k, v, pref._doc_mask(rows, S))
    o.backward(g)
    allowed = allowed_docs(rows, S)
    ro, rdq, rdk, rdv, _, _ = ref32(q, k, v, g, D ** -0.5, allowed)
    eo, edq, edk, edv = eager16(q, k, v, g, D ** -0.5, allowed)
    for name, mine, eager, ref in (("o", o, eo, ro), ("dq", q.grad, edq, rdq), ("dk", k.grad, edk, rdk),
                                   ("dv", v.grad, edv, rdv)):
        e, es = _rel(mine, ref), _rel(eager, ref)
        assert e <= max(8e-3, 1.5 * es), (name, e, es)


def test_interface_without_grad_at_an_odd_length():
    B, Hq, Hkv, S = 2, 8, 2, 13
    q, k, v, g = _inputs(B, Hq, Hkv, S, seed=9)
    with torch.no_grad():
        o, _ = smt_flash_attention_forward(None, q, k, v, None)
    assert o.shape == (B, S, Hq, D)
    ro = plain._ref(q, k, v, g, D ** -0.5)[0]
    so = plain._sdpa_bf16(q, k, v, g)[0]
    e, es = _rel(o, ro), _rel(so, ro)
    assert e <= max(8e-3, 1.5 * es), (e, es)


# ---- whole models on the reference collator's batches -------------------------------------------------------
PAD, IGNORE_INDEX = 0, -100


def _collate(lengths, vocab, seed=3):
    """helper.py:191-205 on synthetic samples: pad to the longest with the pad id, labels with IGNORE_INDEX,
    attention_mask = ids != pad."""
    gen = torch.Generator().manual_seed(seed)
    S = max(lengths)
    ids = torch.full((len(lengths), S), PAD, dtype=torch.int64)
    labels = torch.full((len(lengths), S), IGNORE_INDEX, dtype=torch.int64)
    for b, n in enumerate(lengths):
        seq = torch.randint(1, vocab, (n,), generator=gen)
        ids[b, :n] = seq
        labels[b, :n] = seq
    return ids, labels, ids.ne(PAD)


@pytest.mark.parametrize("S", [40, 37, 38, 39])
def test_patched_mini_llama_on_collated_batches(S):
    """The patched model against the unpatched one (sdpa), as test_patched_mini_llama_matches_eager, on a
    batch padded to its longest sample. S = 40 is the control: it ran before any-length support."""
    import bench
    torch.manual_seed(3)
    model = bench.build_model("mini", DEV)
    ids, labels, mask = (t.to(DEV) for t in _collate((S, 21), 4096))
    out_e = model(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
    out_e.loss.backward()
    ge = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    try:
        fl.patch_llama(model)
        out_f = model(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
        out_f.loss.backward()
        with torch.no_grad():                            # the reference's evaluation(): labels, no gradient
            out_n = model(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
    finally:
        fl.unpatch_llama(model)
    rel = abs(out_f.loss.item() - out_e.loss.item()) / abs(out_e.loss.item())
    rel_n = abs(out_n.loss.item() - out_e.loss.item()) / abs(out_e.loss.item())
    worst = max(((p.grad.float() - ge[n].float()).norm() / ge[n].float().norm()).item()
                for n, p in model.named_parameters() if p.grad is not None)
    print(f"S {S}: loss rel {rel:.2e} (no-grad forward {rel_n:.2e}), worst parameter gradient rel {worst:.2e}")
    assert rel < 1e-3 and rel_n < 1e-3, (out_f.loss.item(), out_n.loss.item(), out_e.loss.item())
    assert worst < 5e-2, worst


def test_smt_mini_llama_on_a_collated_batch_of_odd_length():
    """tests/test_gpu_parity.py's end-to-end mini LLaMA (SMT modules, CPU restatement of the reference
    modules) through patch_llama on a collated batch of lengths (37, 21): loss <= 1e-3, tile gradients
    against the fp64 truth of their own operands <= max(1e-3, 1.1 x the reference algorithm's error)."""
    from oracle import smt_oracle as ref
    from sparse_matrix_tuning_amd.smt import smt
    from tests.test_gpu_parity import _mini_llama
    import bench
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(10)
    model = _mini_llama(2)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sel_mlp = defaultdict(list, {('up_proj', 1): [(2, 1), (0, 0)], ('down_proj', 0): [(1, 0)]})
    sel_att = defaultdict(list, {('v_proj', 1): [(0, 1)], ('q_proj', 0): [(1, 1)]})
    smt.freeze_unselected_matrix_layer(model, sel_mlp, sel_att)
    smt.convert_linear_layer_to_matrix_sparsity(model, sel_mlp, sel_att)
    gpu_mods = {n: m for n, m in model.named_modules() if isinstance(m, smt.LinearLayer_MatrixSparsity)}
    seen_x, seen_g = {}, {}

    def capture(name):
        def hook(_m, inp, out):
            seen_x[name] = inp[0].detach().clone()
            out.register_hook(lambda g: seen_g.__setitem__(name, g.detach().clone()))
        return hook
    handles = [m.register_forward_hook(capture(n)) for n, m in gpu_mods.items()]
    ids, labels, mask = _collate((37, 21), 4096, seed=0)
    fl.patch_llama(model)
    try:
        out = model(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=labels.to(DEV), use_cache=False)
        out.loss.backward()
        torch.cuda.synchronize()
    finally:
        fl.unpatch_llama(model)
        for h in handles:
            h.remove()

    cfg = dict(bench.MODELS["mini"])
    cfg["num_hidden_layers"] = 2
    cpu_cfg = LlamaConfig(**cfg)
    cpu_cfg._attn_implementation = "eager"               # applies the 2-D mask, as tests/test_gpu_padded_batch.py
    cpu = LlamaForCausalLM(cpu_cfg).to(torch.bfloat16)
    cpu.load_state_dict(sd)
    smt.freeze_unselected_matrix_layer(cpu, sel_mlp, sel_att)
    ref.ref_convert(cpu, sel_mlp, sel_att)
    out_ref = cpu(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
    rel = abs(out.loss.item() - out_ref.loss.item()) / abs(out_ref.loss.item())
    print(f"\nloss: MI355X {out.loss.item():.6f}, reference restatement {out_ref.loss.item():.6f}, rel {rel:.2e}")
    assert rel <= 1e-3, (out.loss.item(), out_ref.loss.item())
    assert sorted(seen_g) == sorted(gpu_mods)
    for n, m in gpu_mods.items():
        x, g = seen_x[n].cpu(), seen_g[n].cpu()
        truth = ref.tile_grads_fp64(g, x, m.index_list)
        _gi, ref_gw = ref.linearz_backward(g, x, m.weight.detach().cpu(), m.index_list)
        err, ref_err = _rel(m.selected_weight.grad.cpu(), truth), _rel(ref_gw, truth)
        print(f"{n}: tile grads vs fp64 {err:.2e} (reference {ref_err:.2e})")
        assert err <= max(1e-3, 1.1 * ref_err), (n, err, ref_err)
