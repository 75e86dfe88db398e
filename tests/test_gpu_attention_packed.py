"""Packed sequences (document mask) in the gfx950 flash attention: fused_llama.flash_attention(doc_mask=...),
C ABI include/smt_attention.h ``smt_attn_*_docs``.

1. Numerics, with the structure and bound of tests/test_gpu_attention_dropout.py: against an fp32
   reference under the block-diagonal causal mask built explicitly ([B, 1, S, S]) from the document
   lengths, the relative Frobenius error of o, dq, dk, dv is at most max(8e-3, 1.5 x es), es the error
   of a 16-bit eager attention (transformers' eager_attention_forward order) under the same mask; lse
   within 2e-3 (log2 units).
2. No leakage: changing k / v of one document leaves o and lse of every other document bit-identical,
   and with dO zero outside one document dk / dv outside it are exactly 0.
3. Bit-identity with the plain kernels: documents of whole 256-key blocks equal flash_attention on
   each document's slice alone, and a one-document mask equals doc_mask=None.
4. A two-layer LLaMA on one packed row (restarting position_ids, no attention_mask) through
   patch_llama and smt_flash_mask: loss and input-embedding gradient against transformers' eager
   attention on the same packed input and against the three documents run on their own.
"""
import pytest
import torch

from sparse_matrix_tuning_amd import fused_llama as fl
from sparse_matrix_tuning_amd.fused_llama import (DocMask, dropout_effective_p, flash_attention, flash_dropout_mask)
from tests.attn_ref import D, DEV, allowed_docs as _allowed, eager16, inputs, ref32, rel as _rel

pytestmark = pytest.mark.gpu

DOCS_576 = [[1, 63, 64, 130, 62, 256],      # a length-1 document; boundaries on and off the 64 / 128 tile edges; ends at S
            [300, 276],                     # a boundary inside a 256-key block; a document longer than a block
            [576]]                          # no packing


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _doc_mask(rows, S):
    return DocMask.from_cu_seqlens([torch.tensor(_cu(r), device=DEV) for r in rows], len(rows), S)


def _inputs(B, Hq, Hkv, S, dtype, seed):
    return inputs(B, Hq, Hkv, S, "hf", dtype, seed)


CASES = [
    # Hq, Hkv, S, documents per row, dtype, joint, dropout p
    (4, 2, 576, DOCS_576, torch.bfloat16, False, 0.0),
    (8, 1, 200, [[7, 193]], torch.bfloat16, False, 0.0),            # G = 8 and a ragged last tile
    (2, 2, 4, [[1, 3]], torch.bfloat16, False, 0.0),
    (4, 2, 576, DOCS_576, torch.float16, False, 0.0),
    (4, 2, 576, DOCS_576, torch.bfloat16, True, 0.0),               # joint gradient buffer: bit-identical
    (4, 2, 576, DOCS_576, torch.bfloat16, False, 0.25),             # dropout, a seed above 2^32
]


@pytest.mark.parametrize("Hq,Hkv,S,rows,dtype,joint,p", CASES)
def test_packed_rows_match_fp32_reference(Hq, Hkv, S, rows, dtype, joint, p):
    B = len(rows)
    q, k, v, g = _inputs(B, Hq, Hkv, S, dtype, S + Hq)
    scale = D ** -0.5
    seed = (S << 33) + 17 * Hq + 3
    dm = _doc_mask(rows, S)
    o = flash_attention(q, k, v, joint=joint, dropout_p=p, seed=seed, doc_mask=dm)
    assert o.shape == (B, S, Hq, D) and o.dtype == dtype
    lse = o.grad_fn.saved_tensors[4].clone()             # log2 units of the scaled scores
    o.backward(g)
    allowed = _allowed(rows, S)
    M = flash_dropout_mask(B, Hq, S, p, seed, DEV) if p else None
    r = 1.0 / (1.0 - dropout_effective_p(p)) if p else 1.0
    ro, rdq, rdk, rdv, rlse, _ = ref32(q, k, v, g, scale, allowed, M, r)
    eo, edq, edk, edv = eager16(q, k, v, g, scale, allowed, M, r)
    for name, mine, eager, ref in (("o", o, eo, ro), ("dq", q.grad, edq, rdq), ("dk", k.grad, edk, rdk),
                                   ("dv", v.grad, edv, rdv)):
        e, es = _rel(mine, ref), _rel(eager, ref)
        print(f"{name}: rel err {e:.3e} (16-bit eager {es:.3e})")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= max(8e-3, 1.5 * es), (name, e, es)
    assert torch.isfinite(lse).all()                     # every row sees itself: no +inf case here
    assert (lse - rlse).abs().max().item() < 2e-3
    if joint:
        q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o2 = flash_attention(q2, k2, v2, dropout_p=p, seed=seed, doc_mask=dm)
        o2.backward(g)
        assert torch.equal(o, o2)
        assert torch.equal(q.grad, q2.grad) and torch.equal(k.grad, k2.grad) and torch.equal(v.grad, v2.grad)


def _run(q, k, v, g, **kw):
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(qs, ks, vs, **kw)
    lse = o.grad_fn.saved_tensors[4].clone()
    o.backward(g)
    return o.detach(), lse, qs.grad, ks.grad, vs.grad


def test_no_leakage_between_documents():
    Hq, Hkv, S = 4, 2, 576
    B = len(DOCS_576)
    q, k, v, g = _inputs(B, Hq, Hkv, S, torch.bfloat16, 21)
    dm = _doc_mask(DOCS_576, S)
    base = _run(q, k, v, g, doc_mask=dm)
    # (row, first token, one past the last) of the perturbed document: an off-edge one, and the second of row 1
    for b, lo, hi in ((0, 128, 258), (1, 300, 576), (0, 0, 1)):
        k2, v2 = k.detach().clone(), v.detach().clone()
        k2[b, :, lo:hi] += 1.5
        v2[b, :, lo:hi] = -3.0 * v2[b, :, lo:hi] + 0.25
        o2, lse2, _, _, _ = _run(q, k2, v2, g, doc_mask=dm)
        other = torch.ones(B, S, dtype=torch.bool, device=DEV)
        other[b, lo:hi] = False
        assert torch.equal(o2[other], base[0][other]), (b, lo, hi)
        assert torch.equal(lse2.transpose(1, 2)[other], base[1].transpose(1, 2)[other]), (b, lo, hi)
        assert not torch.equal(o2[~other], base[0][~other])
        # dO zero outside the document: dk / dv outside it are exactly 0
        g2 = torch.zeros_like(g)
        g2[b, lo:hi] = g[b, lo:hi]
        _, _, dq, dk, dv = _run(q, k, v, g2, doc_mask=dm)
        assert (dk.transpose(1, 2)[other].float() == 0).all(), (b, lo, hi)
        assert (dv.transpose(1, 2)[other].float() == 0).all(), (b, lo, hi)
        assert (dq.transpose(1, 2)[other].float() == 0).all(), (b, lo, hi)
        assert dv.transpose(1, 2)[~other].float().abs().sum() > 0
        if hi - lo > 1:                                  # a length-1 document: P = 1, dS = 0, so dk = 0
            assert dk.transpose(1, 2)[~other].float().abs().sum() > 0


def test_block_aligned_documents_equal_the_plain_kernels_on_each_slice():
    Hq, Hkv, S = 4, 2, 768
    q, k, v, g = _inputs(1, Hq, Hkv, S, torch.bfloat16, 33)
    o, lse, dq, dk, dv = _run(q, k, v, g, doc_mask=_doc_mask([[256, 256, 256]], S))
    for d in range(3):
        sl = slice(256 * d, 256 * (d + 1))
        po, plse, pdq, pdk, pdv = _run(q[:, :, sl], k[:, :, sl], v[:, :, sl], g[:, sl])
        assert torch.equal(o[:, sl], po), d
        assert torch.equal(lse[:, :, sl], plse), d
        assert torch.equal(dq[:, :, sl], pdq) and torch.equal(dk[:, :, sl], pdk) and torch.equal(dv[:, :, sl], pdv), d


def test_one_document_equals_no_doc_mask():
    Hq, Hkv, S = 4, 2, 320
    q, k, v, g = _inputs(2, Hq, Hkv, S, torch.bfloat16, 34)
    a = _run(q, k, v, g, doc_mask=_doc_mask([[S], [S]], S))
    b = _run(q, k, v, g)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = _run(q, k, v, g, doc_mask=_doc_mask([[S], [S]], S), dropout_p=0.1, seed=2 ** 35 + 9)
    b = _run(q, k, v, g, dropout_p=0.1, seed=2 ** 35 + 9)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the kernels clamp what they read: doc_start to [0, i], doc_end to [i + 1, S]. Out-of-range values
    # that clamp to one document per row are again the plain result.
    wild = DocMask(torch.full((2, S), -5, dtype=torch.int32, device=DEV),
                   torch.full((2, S), 2 ** 30, dtype=torch.int32, device=DEV), S)
    wild.start[1, ::3] = -2 ** 31
    wild.end[0, ::2] = 2 ** 31 - 1
    assert all(torch.equal(x, y) for x, y in zip(_run(q, k, v, g, doc_mask=wild), _run(q, k, v, g)))


# ---- model level ------------------------------------------------------------------------------------
MODEL_DOCS = [100, 156, 128]


def _llama(dtype, attn):
    from transformers import LlamaConfig, LlamaForCausalLM
    # 2 heads x head_dim 128 over 1 kv head; hidden 512, the smallest the fused RMSNorm takes (a multiple
    # of 512), with head_dim given on its own (as tests/test_gpu_attention_dropout.py)
    cfg = LlamaConfig(vocab_size=512, hidden_size=512, intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1, head_dim=128, max_position_embeddings=512)
    cfg._attn_implementation = attn
    torch.manual_seed(5)
    return LlamaForCausalLM(cfg).to(dtype).to(DEV)


def _packed_batch():
    S = sum(MODEL_DOCS)
    ids = torch.randint(1, 512, (1, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    pos = torch.cat([torch.arange(n, device=DEV) for n in MODEL_DOCS])[None]
    labels = ids.clone()
    for at in _cu(MODEL_DOCS)[:-1]:
        labels[0, at] = -100                              # no document predicts its own first token ...
    return ids, pos, labels


def _loss_and_embed_grad(model, ids, pos, labels):
    model.zero_grad(set_to_none=True)
    emb = model.get_input_embeddings()(ids).detach().requires_grad_(True)
    loss = model(inputs_embeds=emb, position_ids=pos, labels=labels, use_cache=False).loss
    loss.backward()
    return loss.detach().float(), emb.grad.detach().float()


def test_llama_on_a_packed_row():
    ids, pos, labels = _packed_batch()
    S = ids.shape[1]
    model = _llama(torch.bfloat16, "sdpa")
    seen = []
    fl.patch_llama(model)
    try:
        h = model.model.layers[0].self_attn.register_forward_pre_hook(
            lambda _m, a, kw: seen.append(kw.get("attention_mask")), with_kwargs=True)
        loss, dx = _loss_and_embed_grad(model, ids, pos, labels)
        h.remove()
        assert seen and isinstance(seen[0], DocMask)      # through smt_flash_mask, no NotImplementedError
        want = DocMask.from_cu_seqlens(_cu(MODEL_DOCS), 1, S)
        assert torch.equal(seen[0].start.cpu(), want.start) and torch.equal(seen[0].end.cpu(), want.end)
        # the three documents as separate unpadded batches; the packed loss is their token-weighted mean
        # (labels shift inside the model: a document's last token predicts the next document's first
        # token, whose label is -100, so each document counts n - 1 targets in both runs)
        parts, dxs = [], []
        for at, n in zip(_cu(MODEL_DOCS), MODEL_DOCS):
            sl = slice(at, at + n)
            l, d = _loss_and_embed_grad(model, ids[:, sl], pos[:, sl], labels[:, sl])
            parts.append((l, n - 1))
            dxs.append(d * (n - 1))
    finally:
        fl.unpatch_llama(model)
    total = sum(n for _, n in parts)
    split_loss = sum(l * n for l, n in parts) / total
    split_dx = torch.cat(dxs, dim=1) / total

    eager = _llama(torch.bfloat16, "eager")
    eager.load_state_dict(model.state_dict())
    eloss, edx = _loss_and_embed_grad(eager, ids, pos, labels)
    truth = _llama(torch.float32, "eager")
    truth.load_state_dict({n: t.float() for n, t in model.state_dict().items()})
    tloss, tdx = _loss_and_embed_grad(truth, ids, pos, labels)

    rel = lambda a, b: abs(a.item() - b.item()) / abs(b.item())
    print(f"\npacked loss {loss.item():.6f}, eager {eloss.item():.6f} (rel {rel(loss, eloss):.2e}), documents on their own "
          f"{split_loss.item():.6f} (rel {rel(loss, split_loss):.2e}), fp32 {tloss.item():.6f}")
    err, ref_err, direct, split = _rel(dx, tdx), _rel(edx, tdx), _rel(dx, edx), _rel(dx, split_dx)
    print(f"embedding gradient vs fp32 {err:.2e} (eager {ref_err:.2e}), vs eager {direct:.2e}, vs the documents on "
          f"their own {split:.2e}")
    # the bars of tests/test_gpu_padded_batch.py: loss relative <= 1e-3; a gradient against the truth
    # <= max(1e-3, 1.1 x the reference path's error), against the reference path <= max(1e-3, 1.5 x it)
    assert rel(loss, eloss) <= 1e-3 and rel(loss, split_loss) <= 1e-3
    assert err <= max(1e-3, 1.1 * ref_err), (err, ref_err)
    assert direct <= max(1e-3, 1.5 * ref_err), (direct, ref_err)
    assert split <= max(1e-3, 1.5 * ref_err), (split, ref_err)
