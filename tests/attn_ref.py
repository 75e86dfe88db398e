"""The one fp32 reference of the flash-attention GPU tests (tests/test_gpu_attention*.py): attention under
an explicit boolean mask ``allowed`` [B, 1 or Hq, Sq, Skv] (True = query i sees key j), the 16-bit eager
attention under the same mask that sets the tests' error bar, the builders of the three masks the kernels
implement (causal with an optional key mask, block-diagonal causal from document lengths, a call against
a KV cache at ``q_offset``), the error measure and the seeded inputs.

Conventions, those of the kernels (include/smt_attention.h): q [B, Hq, Sq, D], k / v [B, Hkv, Skv, D],
o and its gradient g [B, Sq, Hq, D]; lse in log2 units of the scaled scores, that of the undropped
probabilities; a row without a visible key has a zero output, zero gradients and lse = +inf. Dropout is
the keep mask M [B, Hq, Sq, Skv] times r = 1 / (1 - p_eff) on the probabilities of the PV product."""
import math

import torch

DEV = torch.device("cuda", 0)
D = 128


def rel(a, b):
    """Relative Frobenius error of a against b."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def allowed_causal(S, keep=None):
    """[1 or B, 1, S, S]: causal, and key j kept by ``keep`` [B, S] (bool) where one is given."""
    causal = torch.ones(S, S, dtype=torch.bool, device=DEV).tril()[None, None]
    return causal if keep is None else causal & keep[:, None, None, :]


def allowed_docs(rows, S):
    """The block-diagonal causal mask [B, 1, S, S], written out from the document lengths of each row."""
    m = torch.zeros(len(rows), 1, S, S, dtype=torch.bool)
    for b, lens in enumerate(rows):
        assert sum(lens) == S
        at = 0
        for n in lens:
            m[b, 0, at:at + n, at:at + n] = torch.ones(n, n, dtype=torch.bool).tril()
            at += n
    return m.to(DEV)


def allowed_cached(B, Sq, Skv, q_offset, keep=None):
    """[B, 1, Sq, Skv]: query i sits at position q_offset + i (an int, or one position per batch row as a
    [B] tensor) and sees key j <= its position, and kept by ``keep`` [B, Skv] where one is given."""
    pos = torch.as_tensor(q_offset, device=DEV).reshape(-1, 1) + torch.arange(Sq, device=DEV)[None]      # [1 or B, Sq]
    a = (torch.arange(Skv, device=DEV)[None, None, :] <= pos[:, :, None]).expand(B, Sq, Skv)
    return (a & keep[:, None, :] if keep is not None else a)[:, None]


def _masked_scores(qx, kx, scale, allowed):
    G = qx.shape[1] // kx.shape[1]
    s = (qx @ kx.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    return s.masked_fill(~allowed, float("-inf")), allowed.any(-1, keepdim=True)


def ref32(q, k, v, g, scale, allowed, M=None, r=1.0):
    """fp32 attention of the 16-bit inputs under ``allowed``, gradients by autograd of g (None: forward
    only, the gradients are None). Returns o [B, Sq, Hq, D], dq, dk, dv, lse2 [B, Hq, Sq] and the rows
    with a visible key (bool, lse2's shape)."""
    qf, kf, vf = (t.detach().float().requires_grad_(g is not None) for t in (q, k, v))
    s, any_key = _masked_scores(qf, kf, scale, allowed)
    p = torch.softmax(s.masked_fill(~any_key, 0.0), -1) * any_key
    if M is not None:
        p = p * (M.float() * r)
    o = p @ vf.repeat_interleave(q.shape[1] // k.shape[1], 1)
    if g is not None:
        o.transpose(1, 2).backward(g.float())
    lse2 = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    return o.transpose(1, 2).detach(), qf.grad, kf.grad, vf.grad, lse2, any_key.squeeze(-1).expand_as(lse2)


def eager16(q, k, v, g, scale, allowed, M=None, r=1.0):
    """16-bit eager attention under the same mask, in transformers' eager_attention_forward order: scores
    in the dtype, fp32 softmax cast to the dtype, times M r, the PV matmul in the dtype."""
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s, any_key = _masked_scores(qs, ks, scale, allowed)
    p = (torch.softmax(s.masked_fill(~any_key, 0.0), -1, dtype=torch.float32) * any_key).to(q.dtype)
    if M is not None:
        p = p * (M.to(q.dtype) * r)
    o = p @ vs.repeat_interleave(q.shape[1] // k.shape[1], 1)
    o.transpose(1, 2).backward(g)
    return o.transpose(1, 2).detach(), qs.grad, ks.grad, vs.grad


def inputs(B, Hq, Hkv, S, layout, dtype, seed):
    """Seeded leaves q, k, v and the output gradient g, drawn in that order."""
    torch.manual_seed(seed)
    if layout == "hf":      # [B, S, H, D] storage viewed as [B, H, S, D], as transformers hands them over
        mk = lambda H: torch.randn(B, S, H, D, device=DEV).to(dtype).transpose(1, 2).requires_grad_(True)
    else:
        mk = lambda H: torch.randn(B, H, S, D, device=DEV).to(dtype).requires_grad_(True)
    return mk(Hq), mk(Hkv), mk(Hkv), torch.randn(B, S, Hq, D, device=DEV).to(dtype)
