"""Attention dropout inside the gfx950 flash attention (fused_llama.flash_attention(dropout_p=...),
C ABI include/smt_attention.h ``smt_attn_*_dropout``).

Mask: ``flash_dropout_mask`` (the kernels' own keep function, exported) equals the numpy restatement
of the documented definition (tests/dropout_keep_ref.py) bit for bit.

Numerics: against an fp32 reference that uses the exported mask M, o = (softmax(causal [& key mask])
o M r) V with r = 1 / (1 - p_eff), gradients by autograd. Relative Frobenius error of o, dq, dk, dv
<= max(8e-3, 1.5 x es), es the error of a 16-bit eager attention with the same mask in the order of
transformers' eager_attention_forward (scores in the dtype, fp32 softmax cast to the dtype, times
M r, the PV matmul in the dtype) -- the bound of tests/test_gpu_attention.py with dropout on both
sides. lse is that of the undropped probabilities: within 2e-3 (log2 units) of the undropped reference.
"""
import numpy as np
import pytest
import torch

from sparse_matrix_tuning_amd import fused_llama as fl
from sparse_matrix_tuning_amd.fused_llama import (KeyMask, dropout_effective_p, flash_attention, flash_dropout_mask,
                                                  smt_flash_mask)
from tests.attn_ref import D, DEV, allowed_causal, eager16, inputs as _inputs, ref32, rel as _rel
from tests.dropout_keep_ref import keep_mask

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,S", [(2, 4, 200), (1, 8, 512)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [12345, (0xA5A5 << 32) | 0x1234567])
def test_exported_mask_is_the_documented_function(B, H, S, p, seed):
    got = flash_dropout_mask(B, H, S, p, seed, DEV)
    assert got.shape == (B, H, S, S) and got.dtype == torch.bool
    assert np.array_equal(got.cpu().numpy(), keep_mask(B, H, S, p, seed))
    # the seed as a device tensor is the same seed
    st = torch.tensor([seed], dtype=torch.int64, device=DEV)
    assert torch.equal(flash_dropout_mask(B, H, S, p, st, DEV), got)


def test_exported_mask_without_dropout_keeps_everything():
    assert flash_dropout_mask(1, 2, 64, 0.0, None, DEV).all()
    assert flash_dropout_mask(1, 2, 64, 0.001, 7, DEV).all()             # t == 0


def _key_mask(B, S):
    keep = torch.ones(B, S, dtype=torch.bool, device=DEV)
    keep[0, S - S // 3:] = False                        # right padding
    keep[0, 5] = keep[0, 64] = keep[0, 100] = False      # holes
    keep[1, 0:3] = False                                 # a fully masked prefix: queries 0-2 see no key
    keep[1, 77] = False
    return keep


CASES = [
    # B, Hq, Hkv, S, p, layout, dtype, key mask, joint
    (2, 8, 2, 256, 0.1, "hf", torch.bfloat16, False, False),          # one dK/dV key block
    (1, 4, 4, 200, 0.5, "hf", torch.bfloat16, False, False),          # ragged; rows whose only key is dropped
    (1, 8, 1, 384, 0.1, "contig", torch.bfloat16, False, False),      # G = 8
    (1, 4, 2, 640, 0.1, "hf", torch.bfloat16, False, False),          # 5 query blocks, 2.5 key blocks (a causal pair)
    (1, 2, 2, 4, 0.5, "hf", torch.bfloat16, False, False),
    (2, 4, 2, 320, 0.25, "hf", torch.bfloat16, True, False),          # key mask with holes + a masked prefix
    (1, 4, 2, 256, 0.1, "hf", torch.float16, False, False),
    (1, 4, 2, 256, 0.1, "hf", torch.bfloat16, False, True),           # joint gradient buffer
]


@pytest.mark.parametrize("B,Hq,Hkv,S,p,layout,dtype,masked,joint", CASES)
def test_dropout_matches_fp32_reference_with_the_exported_mask(B, Hq, Hkv, S, p, layout, dtype, masked, joint):
    q, k, v, g = _inputs(B, Hq, Hkv, S, layout, dtype, S + Hq)
    scale = D ** -0.5
    seed = (S << 33) + 17 * Hq + 3                       # some above 2^32
    keep = _key_mask(B, S) if masked else None
    km = smt_flash_mask(B, S, S, attention_mask=keep.long()) if masked else None
    assert km is None or isinstance(km, KeyMask)
    o = flash_attention(q, k, v, key_mask=km, joint=joint, dropout_p=p, seed=seed)
    assert o.shape == (B, S, Hq, D) and o.dtype == dtype
    lse = o.grad_fn.saved_tensors[4].clone()             # log2 units of the scaled scores
    o.backward(g)
    M = flash_dropout_mask(B, Hq, S, p, seed, DEV)
    r = 1.0 / (1.0 - dropout_effective_p(p))
    allowed = allowed_causal(S, keep)
    ro, rdq, rdk, rdv, rlse, vis = ref32(q, k, v, g, scale, allowed, M, r)
    eo, edq, edk, edv = eager16(q, k, v, g, scale, allowed, M, r)
    for name, mine, eager, ref in (("o", o, eo, ro), ("dq", q.grad, edq, rdq), ("dk", k.grad, edk, rdk),
                                   ("dv", v.grad, edv, rdv)):
        e, es = _rel(mine, ref), _rel(eager, ref)
        print(f"{name}: rel err {e:.3e} (16-bit eager {es:.3e})")
        assert torch.isfinite(mine.float()).all(), name
        assert e <= max(8e-3, 1.5 * es), (name, e, es)
    # lse is untouched by dropout
    assert (lse[vis] - rlse[vis]).abs().max().item() < 2e-3
    if masked:
        assert torch.isinf(lse[~vis]).all() and (lse[~vis] > 0).all()
        dead = ~keep[:, None, :, None].expand(B, Hkv, S, D)
        assert (k.grad.float()[dead] == 0).all() and (v.grad.float()[dead] == 0).all()
    # a row all of whose visible keys were dropped: o = 0 exactly, a finite lse, a zero dq row
    gone = vis & ~(M & allowed).any(-1)                       # [B, Hq, S]
    if (S, p) == (200, 0.5):
        assert gone[:, :, 0].any() and not gone[:, :, 0].all()          # q = 0 sees key 0 only: dropped for some heads
    assert torch.isfinite(lse[gone]).all()
    assert (o.transpose(1, 2).float()[gone] == 0).all()
    assert (q.grad.float()[gone] == 0).all()
    if joint:
        q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o2 = flash_attention(q2, k2, v2, key_mask=km, dropout_p=p, seed=seed)
        o2.backward(g)
        assert torch.equal(o, o2)
        assert torch.equal(q.grad, q2.grad) and torch.equal(k.grad, k2.grad) and torch.equal(v.grad, v2.grad)


def test_dropout_is_a_function_of_the_seed():
    B, Hq, Hkv, S = 1, 4, 2, 256
    q, k, v, g = _inputs(B, Hq, Hkv, S, "hf", torch.bfloat16, 5)

    def run(**kw):
        qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o = flash_attention(qs, ks, vs, **kw)
        o.backward(g)
        return o.detach(), qs.grad, ks.grad, vs.grad

    a = run(dropout_p=0.1, seed=2 ** 40 + 1)
    b = run(dropout_p=0.1, seed=2 ** 40 + 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = run(dropout_p=0.1, seed=2 ** 40 + 2)
    assert not torch.equal(a[0], c[0])
    # a seed tensor is read on the device, and is the same seed
    d = run(dropout_p=0.1, seed=torch.tensor([2 ** 40 + 1], dtype=torch.int64, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(a, d))
    # no seed: drawn from the device generator, so torch.manual_seed pins it
    torch.manual_seed(77)
    e = run(dropout_p=0.1)
    torch.manual_seed(77)
    f = run(dropout_p=0.1)
    assert all(torch.equal(x, y) for x, y in zip(e, f))
    assert not torch.equal(e[0], run(dropout_p=0.1)[0])
    # dropout_p = 0 through the new arguments is today's call
    plain = run()
    zero = run(dropout_p=0.0, seed=9)
    assert all(torch.equal(x, y) for x, y in zip(plain, zero))
    with pytest.raises(ValueError, match="outside"):
        run(dropout_p=1.0)


def _llama(attention_dropout):
    from transformers import LlamaConfig, LlamaForCausalLM
    # 2 heads x head_dim 128 over 1 kv head; hidden 512, the smallest the fused RMSNorm takes (a multiple
    # of 512), with head_dim given on its own
    cfg = LlamaConfig(vocab_size=512, hidden_size=512, intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1, head_dim=128, max_position_embeddings=256,
                      attention_dropout=attention_dropout)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(5)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(DEV)


def _step(model, ids, seed, checkpoint=False, train=True):
    """(loss, gradients) of one forward + backward of the patched model after torch.manual_seed(seed);
    in eval mode (logits, {})."""
    model.zero_grad(set_to_none=True)
    model.train(train)
    fl.patch_llama(model)
    try:
        if checkpoint:
            model.gradient_checkpointing_enable()
        torch.manual_seed(seed)
        if not train:
            with torch.no_grad():
                return model(input_ids=ids, use_cache=False).logits, {}
        loss = model(input_ids=ids, labels=ids, use_cache=False).loss
        loss.backward()
    finally:
        if checkpoint:
            model.gradient_checkpointing_disable()
        fl.unpatch_llama(model)                          # the RoPE patch is process-global
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    return torch.equal(a[0], b[0]) and sorted(a[1]) == sorted(b[1]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_llama_trains_with_attention_dropout():
    ids = torch.randint(1, 512, (2, 128), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    drop, plain = _llama(0.1), _llama(0.0)
    a = _step(drop, ids, 11)
    ref = _step(plain, ids, 11)
    assert torch.isfinite(a[0]) and all(torch.isfinite(g.float()).all() for g in a[1].values())
    assert not torch.equal(a[0], ref[0])                                 # the dropout is applied
    assert _same(a, _step(drop, ids, 11))                                # the same seed: the same step
    assert not torch.equal(a[0], _step(drop, ids, 12)[0])
    # per-layer recompute replays the masks; the same equality without dropout tells which side broke
    assert _same(ref, _step(plain, ids, 11, checkpoint=True)), "attention_dropout=0"
    assert _same(a, _step(drop, ids, 11, checkpoint=True)), "attention_dropout=0.1"
    # eval: transformers passes dropout 0.0
    assert torch.equal(_step(drop, ids, 11, train=False)[0], _step(plain, ids, 11, train=False)[0])
