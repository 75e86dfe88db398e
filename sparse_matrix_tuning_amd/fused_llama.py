"""Fused gfx950 replacements for the eager elementwise chains of the HF LLaMA decoder.

The SMT step trains ``transformers`` ``LlamaForCausalLM`` (the reference loads it through
``AutoModelForCausalLM``, ``fine_tune.py:150-155``). In eager mode its RMSNorm, rotary embedding and
SwiGLU each run as chains of 4-8 elementwise kernels, several in fp32; on MI355X those chains are
27 % of an SMT step (profiles/r01_bench_step_breakdown.txt). :func:`patch_llama` swaps them for
one-pass HIP kernels (``csrc/llama_kernels.hip``, C ABI ``include/smt_model_ops.h``) wrapped in
autograd Functions. Every intermediate 16-bit rounding of the eager chain is reproduced, so results
match the eager model up to reduction order / exp ulps (tests/test_gpu_fused_llama.py).

It also routes the decoder's attention to a gfx950 causal flash attention (forward + backward,
``csrc/attn_kernels.hip``, C ABI ``include/smt_attention.h``), registered with transformers'
``AttentionInterface`` as ``"smt_flash"``; sdpa on this torch build runs aotriton at 25-27 % of the
step. Tolerances vs an fp32 reference are in tests/test_gpu_attention.py. Calls against a KV cache
(``generate()`` on the patched model) run a split-KV decode kernel, forward only
(:func:`flash_attention_cached`, tests/test_gpu_attention_cached.py, tests/test_gpu_generate.py).

The causal-LM loss (transformers ``ForCausalLMLoss``: ``logits.float()`` then cross entropy) becomes
two row kernels over the bf16 logits (``smt_ce_fwd`` / ``smt_ce_bwd``), so the 16.8 GB fp32 logits
copy, its log-softmax and its fp32 gradient are never materialised (tests/test_gpu_cross_entropy.py).

``patch_llama(decode_linears=True)`` (opt-in) routes the dense linears of a decode step (at most 16 rows,
gradients off) to a weight-streaming kernel (``csrc/linear_kernels.hip``, C ABI ``include/smt_linear.h``;
:func:`decode_linear`, :func:`decode_linear_group`, :func:`decode_swiglu`) at the sizes where it measured
faster than hipBLASLt (tests/test_gpu_decode_linear.py, tests/test_gpu_generate_decode_linears.py). With
``decode_fp8=True`` as well, the frozen linears of an fp8 model (``engine.attach_fp8_weights``) first try the
same stream on their e4m3 bytes (``smt_linear_skinny_fp8``; :func:`decode_linear_fp8`,
:func:`decode_linear_group_fp8`, :func:`decode_swiglu_fp8`) at the sizes where it measured faster than
``quant_rows`` + ``torch._scaled_mm`` (tests/test_gpu_decode_linear_fp8.py, tests/test_gpu_generate_decode_fp8.py).

:func:`patch_model` / :func:`unpatch_model` are :func:`patch_llama` / :func:`unpatch_llama` for any family of
:data:`FAMILIES`, LLaMA and Qwen2 (the reference's other family, the DeepSeek-R1 distills): the family is read from
the model's classes and the same body runs over its table entry. Qwen2's biased q, k and v go through the
decode-linear kernel's bias epilogue (``smt_linear_skinny_bias``; tests/test_gpu_decode_linear_bias.py,
tests/test_gpu_qwen2.py).

The model's dtype is bf16 or, since ABI v13, fp16 (the reference's ``--dtype fp16``,
``fine_tune.py:955-959``): every kernel is one template body for both formats, rounding where the eager
chain rounds to the model's dtype (tests/test_gpu_fused_fp16.py). fp32 models and mixed dtypes raise
(no silent fallback); the fp8 producer fusions stay bf16-only.
"""
from __future__ import annotations

import ctypes
import gc
import os
import weakref

import torch
from torch import nn

from . import _hip


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need(t: torch.Tensor, what: str, like: torch.Tensor = None):
    """A ROCm tensor of the model's 16-bit dtype: bf16, or fp16 (the reference's --dtype fp16,
    fine_tune.py:955-959; ABI v13) -- and, with ``like``, the same dtype as it."""
    if t.device.type != "cuda" or t.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"fused {what}: bf16 / fp16 ROCm tensors only (got {t.dtype} on {t.device})")
    if like is not None and t.dtype != like.dtype:
        raise RuntimeError(f"fused {what}: {t.dtype} beside {like.dtype} (one model dtype)")


def _dt(t: torch.Tensor) -> int:
    """SMT_DTYPE_* of a 16-bit tensor, the kernels' format argument."""
    return _hip.dtype_code16(t.dtype, "fused op")


def _tag(out, op, a2d, b2d=None, w=None, rstd=None):
    """Under the "selective" activation policy, let an SMT linear consuming ``out`` rebuild its column
    blocks from these operands in the backward instead of keeping them (smt.tag_recompute)."""
    from .smt.smt import tag_recompute
    return tag_recompute(out, op, a2d, b2d, w, rstd)


def _rows2d(t: torch.Tensor):
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(-1) != 1 or t2.stride(0) % 8 or t2.data_ptr() % 16:
        t2 = t2.contiguous()
    return t2


# ------------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------------
class FusedRMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        _need(x, "rmsnorm")
        _need(weight, "rmsnorm", like=x)
        x2 = _rows2d(x)
        rows, H = x2.shape
        y = torch.empty((rows, H), dtype=x.dtype, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w = weight.contiguous()
        rc = _hip.load().smt_rmsnorm_fwd(x2.data_ptr(), x2.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0),
                                         rstd.data_ptr(), rows, H, float(eps), _dt(x), _stream(x))
        _hip._check(rc, "smt_rmsnorm_fwd")
        ctx.save_for_backward(x2, w, rstd)
        ctx.shape = x.shape
        return _tag(y.view(x.shape), _hip.RECOMPUTE_RMSNORM, x2, None, w, rstd)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rstd = ctx.saved_tensors
        dx, dw = _rmsnorm_bwd(x2, w, rstd, dy, ctx.needs_input_grad[1])
        return dx.view(ctx.shape), dw, None


def _reg_hidden(H: int) -> bool:
    """The register-resident norm kernels (a row of 512 * k values per wave, k <= 16) take this hidden
    size; every other hidden % 8 == 0 runs the generic kernels, which have no fused residual add."""
    return H % 512 == 0 and H <= 8192


def _rmsnorm_bwd(x2, w, rstd, dy, need_dw: bool, dres=None):
    """dx (+ ``dres``, the gradient reaching the same input by the residual path) and, with
    ``need_dw``, the weight gradient. With both (the full fine-tuning warm-up) one
    ``smt_rmsnorm_bwd_add_dw`` pass; returns ``(dx 2-D, dw or None)``."""
    rows, H = x2.shape
    dy2 = _rows2d(dy)
    dx = torch.empty_like(x2)
    lib = _hip.load()
    dw = partial = None
    if need_dw:
        waves = lib.smt_rmsnorm_bwd_waves(rows)
        partial = torch.empty(waves, H, dtype=torch.float32, device=x2.device)
        dw = torch.empty(H, dtype=w.dtype, device=w.device)
    if dres is not None and need_dw and _reg_hidden(H):
        dr2 = _rows2d(dres)
        rc = lib.smt_rmsnorm_bwd_add_dw(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(),
                                        rstd.data_ptr(), dr2.data_ptr(), dr2.stride(0), dx.data_ptr(), dx.stride(0),
                                        partial.data_ptr(), dw.data_ptr(), rows, H, _dt(x2), _stream(x2))
        _hip._check(rc, "smt_rmsnorm_bwd_add_dw")
        return dx, dw
    rc = lib.smt_rmsnorm_bwd(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(),
                             rstd.data_ptr(), dx.data_ptr(), dx.stride(0),
                             None if partial is None else partial.data_ptr(),
                             None if dw is None else dw.data_ptr(), rows, H, _dt(x2), _stream(x2))
    _hip._check(rc, "smt_rmsnorm_bwd")
    if dres is not None:
        dx = dx + _rows2d(dres)
    return dx, dw


def fused_rmsnorm_forward(self, hidden_states):
    """Drop-in for ``LlamaRMSNorm.forward``."""
    return FusedRMSNormFn.apply(hidden_states, self.weight, self.variance_epsilon)


class FusedRMSNormResFn(torch.autograd.Function):
    """``LlamaDecoderLayer``'s ``residual = x; y = input_layernorm(x)`` as one node returning
    ``(y, residual)`` (the residual an alias of ``x``), so that the backward receives both gradients
    of ``x`` and sums them inside the norm's backward kernel (``smt_rmsnorm_bwd_add``) instead of an
    autograd add."""

    @staticmethod
    def forward(ctx, x, weight, eps, quant=False, need_y=True):
        if not quant:
            y = FusedRMSNormFn.forward(ctx, x, weight, eps)
            return y, x.view_as(x)
        # fp8 consumers (q/k/v): the norm also emits their e4m3 input (fp8.quant_rows_cached finds it)
        from .fp8 import rmsnorm_quant
        _need(x, "rmsnorm")
        x2, w = _rows2d(x), weight.contiguous()
        _h, y, rstd, q, sq = rmsnorm_quant(x2, None, w, eps, need_y)
        ctx.save_for_backward(x2, w, rstd)
        ctx.shape = x.shape
        ctx.quant_grad = True             # fp8 model: the input gradient feeds the previous down_proj
        y = y.view(x.shape) if y is not None else x.new_zeros(()).expand(x.shape)
        y._smt_q8 = (y._version, q, sq)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x2, w, rstd = ctx.saved_tensors              # unpacked once (activation checkpointing)
        if dres is None or ctx.needs_input_grad[1] or x2.shape[1] % 512 or x2.shape[1] > 8192:
            dx, dw = _rmsnorm_bwd(x2, w, rstd, dy, ctx.needs_input_grad[1], dres)
            return dx.view(ctx.shape), dw, None, None, None
        rows, H = x2.shape
        dy2, dr2 = _rows2d(dy), _rows2d(dres)
        if getattr(ctx, "quant_grad", False):
            from .fp8 import rmsnorm_bwd_add_quant
            dx, q, sq = rmsnorm_bwd_add_quant(dy2, x2, w, rstd, dr2)
            dx = dx.view(ctx.shape)
            dx._smt_q8 = (dx._version, q, sq)
            return dx, None, None, None, None
        dx = torch.empty_like(x2)
        rc = _hip.load().smt_rmsnorm_bwd_add(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(),
                                             rstd.data_ptr(), dr2.data_ptr(), dr2.stride(0), dx.data_ptr(), H, rows, H,
                                             _dt(x2), _stream(x2))
        _hip._check(rc, "smt_rmsnorm_bwd_add")
        return dx.view(ctx.shape), None, None, None, None


class FusedAddRMSNormFn(torch.autograd.Function):
    """``h = x + residual`` and ``y = RMSNorm(h)`` (LlamaDecoderLayer's attention residual feeding
    ``post_attention_layernorm``) in one pass; the backward adds the gradient that reaches ``h`` by
    the residual path inside the norm's backward. Returns ``(h, y)``."""

    @staticmethod
    def forward(ctx, x, residual, weight, eps, quant=False, need_y=True):
        for t, n in ((x, "x"), (residual, "residual"), (weight, "weight")):
            _need(t, "add+rmsnorm " + n, like=x)
        x2, r2 = _rows2d(x), _rows2d(residual)
        rows, H = x2.shape
        if quant:
            # fp8 consumers (gate/up): the norm also emits their e4m3 input
            from .fp8 import rmsnorm_quant
            w = weight.contiguous()
            h, y, rstd, q, sq = rmsnorm_quant(x2, r2, w, eps, need_y)
            ctx.save_for_backward(h, w, rstd)
            ctx.shape = x.shape
            ctx.quant_grad = True         # fp8 model: the gradient of h feeds o_proj
            y = y.view(x.shape) if y is not None else x.new_zeros(()).expand(x.shape)
            y._smt_q8 = (y._version, q, sq)
            return h.view(x.shape), y
        y = torch.empty((rows, H), dtype=x.dtype, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w = weight.contiguous()
        if _reg_hidden(H):
            h = torch.empty((rows, H), dtype=x.dtype, device=x.device)
            rc = _hip.load().smt_add_rmsnorm_fwd(x2.data_ptr(), x2.stride(0), r2.data_ptr(), r2.stride(0), w.data_ptr(),
                                                 h.data_ptr(), H, y.data_ptr(), H, rstd.data_ptr(), rows, H, float(eps),
                                                 _dt(x), _stream(x))
            _hip._check(rc, "smt_add_rmsnorm_fwd")
        else:
            # the one-pass kernel holds a row in registers (hidden = 512 * k); any other hidden % 8 == 0:
            # the model-dtype add, then the generic norm kernel over h (the same values)
            h = (x2 + r2).contiguous()
            rc = _hip.load().smt_rmsnorm_fwd(h.data_ptr(), H, w.data_ptr(), y.data_ptr(), H, rstd.data_ptr(), rows, H,
                                             float(eps), _dt(x), _stream(x))
            _hip._check(rc, "smt_rmsnorm_fwd")
        ctx.save_for_backward(h, w, rstd)
        ctx.shape = x.shape
        return h.view(x.shape), _tag(y.view(x.shape), _hip.RECOMPUTE_RMSNORM, h, None, w, rstd)

    @staticmethod
    def backward(ctx, dh, dy):
        h, w, rstd = ctx.saved_tensors
        rows, H = h.shape
        lib = _hip.load()
        dw = None
        if dy is None:
            dx = dh
        elif ctx.needs_input_grad[2] or dh is None or not _reg_hidden(H):
            # weight grad (full fine-tuning warm-up; the residual gradient added in the same pass),
            # no residual gradient, or a hidden size the one-pass kernel does not take: the plain
            # norm backward
            dx, dw = _rmsnorm_bwd(h, w, rstd, dy, ctx.needs_input_grad[2], dh)
            dx = dx.view(ctx.shape)
        elif getattr(ctx, "quant_grad", False):
            from .fp8 import rmsnorm_bwd_add_quant
            dx, q, sq = rmsnorm_bwd_add_quant(_rows2d(dy), h, w, rstd, _rows2d(dh))
            dx = dx.view(ctx.shape)
            dx._smt_q8 = (dx._version, q, sq)
        else:
            dy2, dh2 = _rows2d(dy), _rows2d(dh)
            dx = torch.empty_like(h)
            rc = lib.smt_rmsnorm_bwd_add(dy2.data_ptr(), dy2.stride(0), h.data_ptr(), H, w.data_ptr(), rstd.data_ptr(),
                                         dh2.data_ptr(), dh2.stride(0), dx.data_ptr(), H, rows, H, _dt(h), _stream(h))
            _hip._check(rc, "smt_rmsnorm_bwd_add")
            dx = dx.view(ctx.shape)
        return dx, dx, dw, None, None, None


_RESIDUAL_NORM = os.environ.get("SMT_FUSED_RESIDUAL_NORM", "1") != "0"
# SMT_FUSED_LAYER_TAIL=0: the MLP residual add stays a separate add before the next layer's input norm
_LAYER_TAIL = os.environ.get("SMT_FUSED_LAYER_TAIL", "1") != "0"


def _recomputed(layer) -> bool:
    """transformers' per-layer gradient checkpointing is active for ``layer`` (its forward runs again
    in the backward; the fused tail below must then not span it)."""
    return bool(getattr(layer, "gradient_checkpointing", False) and layer.training)


def _attn_quant(attn, H):
    """(quant, need_y) of a norm feeding this attention's q/k/v (fp8 consumers), as below."""
    if H in (1024, 2048, 4096, 8192) and all(hasattr(attn, n) for n in ("q_proj", "k_proj", "v_proj")):
        from .fp8 import norm_consumers
        return norm_consumers(attn.q_proj, attn.k_proj, attn.v_proj)
    return (False, True)


def fused_decoder_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                                use_cache=False, position_embeddings=None, **kwargs):
    """Drop-in for ``LlamaDecoderLayer.forward`` with the attention residual add fused into the
    post-attention RMSNorm (:class:`FusedAddRMSNormFn`) and the input norm's two gradients summed in
    its backward (:class:`FusedRMSNormResFn`); the same ops in the same order otherwise."""
    norm1 = self.input_layernorm
    attn, mlp = self.self_attn, self.mlp
    H = hidden_states.shape[-1]
    q1 = q2 = (False, True)
    if H in (1024, 2048, 4096, 8192) and all(hasattr(attn, n) for n in ("q_proj", "k_proj", "v_proj")):
        from .fp8 import norm_consumers
        q1 = norm_consumers(attn.q_proj, attn.k_proj, attn.v_proj)
        if hasattr(mlp, "gate_proj") and hasattr(mlp, "up_proj"):
            q2 = norm_consumers(mlp.gate_proj, mlp.up_proj)
    # the previous layer may have normalised this input already (its fused tail, below): same values
    # as the input norm computes here, and its backward sums the residual gradient the same way
    st = hidden_states.__dict__.pop("_smt_normed", None)
    if (st is not None and st[0] is norm1.weight and st[1] == q1 and st[3] == hidden_states._version
            and not _recomputed(self)):
        residual, hidden_states = hidden_states, st[2]
    elif _RESIDUAL_NORM:
        hidden_states, residual = FusedRMSNormResFn.apply(hidden_states, norm1.weight, norm1.variance_epsilon, *q1)
    else:
        residual = hidden_states
        hidden_states = norm1(hidden_states)
    hidden_states, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask,
                                      position_ids=position_ids, past_key_values=past_key_values, use_cache=use_cache,
                                      position_embeddings=position_embeddings, **kwargs)
    norm = self.post_attention_layernorm
    residual, hidden_states = FusedAddRMSNormFn.apply(hidden_states, residual, norm.weight, norm.variance_epsilon, *q2)
    hidden_states = self.mlp(hidden_states)
    ref = self.__dict__.get("_smt_next_layer")
    nxt = ref() if ref is not None else None
    if _LAYER_TAIL and _RESIDUAL_NORM and nxt is not None and not _recomputed(self) and not _recomputed(nxt):
        # the MLP residual add fused with the NEXT layer's input RMSNorm (one add+norm pass instead of
        # an add and a norm): the layer still returns h = residual + mlp_out, with the normalised h
        # attached for the next layer, which uses it only if it receives this very tensor unchanged
        # (fp8 attention: the norm also emits the next q/k/v's e4m3 rows, and its backward the
        # down_proj data gradient's, as the next layer's own input norm would)
        qn = _attn_quant(nxt.self_attn, H)
        n1 = nxt.input_layernorm
        h, y = FusedAddRMSNormFn.apply(hidden_states, residual, n1.weight, n1.variance_epsilon, *qn)
        h.__dict__["_smt_normed"] = (n1.weight, qn, y, h._version)
        return h
    return residual + hidden_states


# ------------------------------------------------------------------------------------------------
# RoPE
# ------------------------------------------------------------------------------------------------
def _rope_desc(inp: torch.Tensor, out: torch.Tensor) -> _hip.RopeTensor:
    sb, sh, ss, sd = inp.stride()
    ob, oh, os_, od = out.stride()
    if sd != 1 or od != 1:
        raise RuntimeError("fused rope: head_dim must be the innermost dimension")
    return _hip.RopeTensor(inp.data_ptr(), out.data_ptr(), sb, sh, ss, ob, oh, os_, inp.shape[1], 0)


def _rope_launch(fn_name, q, k, cos, sin, q_layout=None, k_layout=None, in_place=False):
    """Launch the fused rope kernel on q and k; outputs take ``*_layout`` = (shape, stride) (default:
    the input's own layout: [B, S, H, D] storage under the [B, H, S, D] view for HF q/k), or
    overwrite q and k (``in_place``: every thread reads its element pairs before writing them)."""
    B, _Hq, S, D = q.shape
    if cos.dim() != 3 or cos.stride(-1) != 1 or cos.shape != sin.shape or cos.stride() != sin.stride():
        cos, sin = cos.contiguous(), sin.contiguous()
    if cos.shape[0] != B:
        # HF's position embeddings are [1, S, D] for a batch: a zero batch stride instead of B copies
        cos, sin = cos.expand(B, -1, -1), sin.expand(B, -1, -1)
    q = _rope_ready(q)
    k = _rope_ready(k)
    qs, qst = q_layout or (q.shape, q.stride())
    ks, kst = k_layout or (k.shape, k.stride())
    if in_place:
        qo, ko = q, k
    else:
        qo = torch.empty_strided(qs, qst, dtype=q.dtype, device=q.device)
        ko = torch.empty_strided(ks, kst, dtype=k.dtype, device=k.device)
    dq, dk = _rope_desc(q, qo), _rope_desc(k, ko)
    lib = _hip.load()
    rc = getattr(lib, fn_name)(ctypes.byref(dq), ctypes.byref(dk), cos.data_ptr(), sin.data_ptr(), cos.stride(0),
                               cos.stride(1), B, S, D, _dt(q), _stream(q))
    _hip._check(rc, fn_name)
    return qo, ko


def _rope_ready(t: torch.Tensor) -> torch.Tensor:
    """16-byte aligned rows and 8-element strides with head_dim innermost, else a contiguous copy."""
    if t.stride(-1) == 1 and not any(s % 8 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


class FusedRoPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        for t, n in ((q, "q"), (k, "k"), (cos, "cos"), (sin, "sin")):
            _need(t, "rope " + n, like=q)
        qo, ko = _rope_launch("smt_rope_fwd", q, k, cos, sin)
        ctx.save_for_backward(cos, sin)
        # grads go back in q/k's own layout, so the transpose/view backward of q_proj's output is free
        ctx.layouts = ((q.shape, q.stride()), (k.shape, k.stride()))
        return qo, ko

    @staticmethod
    def backward(ctx, dqo, dko):
        cos, sin = ctx.saved_tensors
        ql, kl = ctx.layouts
        if dqo is None:
            dqo = torch.zeros(ql[0], dtype=cos.dtype, device=cos.device)
        if dko is None:
            dko = torch.zeros(kl[0], dtype=cos.dtype, device=cos.device)
        # the flash attention's joint [dq | dk | dv] gradient (FlashAttnFn joint): rotate the q / k
        # slices in place, so q_proj and k_proj receive slices of the one buffer (dgrad's joint GEMM)
        joint = (getattr(dqo, "_smt_joint", False) and getattr(dko, "_smt_joint", False)
                 and _rope_ready(dqo) is dqo and _rope_ready(dko) is dko)
        dq, dk = _rope_launch("smt_rope_bwd", dqo, dko, cos, sin, ql, kl, in_place=joint)
        return dq, dk, None, None


def fused_apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1):
    """Drop-in for ``transformers.models.llama.modeling_llama.apply_rotary_pos_emb`` (q/k in
    ``[B, heads, S, head_dim]``, cos/sin ``[B, S, head_dim]``)."""
    if unsqueeze_dim != 1:
        raise NotImplementedError("fused rope: unsqueeze_dim=1 layout only")
    return FusedRoPEFn.apply(q, k, cos, sin)


# ------------------------------------------------------------------------------------------------
# SwiGLU
# ------------------------------------------------------------------------------------------------
class FusedSwiGLUFn(torch.autograd.Function):
    """When gate and up are the two members of one fp8 group (``fp8_linears``), the backward also
    emits their joint e4m3 gradient rows (``fp8.swiglu_bwd_quant``) for the group's single data-
    gradient GEMM, and the bf16 gradients only for a member that needs them (an SMT module's tile
    weight gradient); the others get a zero-stride placeholder that nothing reads."""

    @staticmethod
    def forward(ctx, gate, up, quant_out=False, need_bf16_out=True):
        _need(gate, "swiglu")
        _need(up, "swiglu", like=gate)
        from .fp8 import swiglu_group
        ctx.fp8 = swiglu_group(gate, up)
        g = gate.contiguous()
        u = up.contiguous()
        ctx.save_for_backward(g, u)
        if quant_out:
            # fp8 down_proj: emit its per-row e4m3 input directly (cached on the output, where
            # fp8.quant_rows_cached finds it); the bf16 output only if the consumer reads it
            from .fp8 import swiglu_fwd_quant
            q, sq, h = swiglu_fwd_quant(g, u, need_bf16_out)
            if h is None:
                h = g.new_zeros(()).expand(g.shape)
            h._smt_q8 = (h._version, q, sq)
            return h
        h = torch.empty_like(g)
        rc = _hip.load().smt_swiglu_fwd(g.data_ptr(), u.data_ptr(), h.data_ptr(), g.numel(), _dt(g), _stream(g))
        _hip._check(rc, "smt_swiglu_fwd")
        return _tag(h, _hip.RECOMPUTE_SWIGLU, _rows2d(g), _rows2d(u))

    @staticmethod
    def backward(ctx, dh):
        g, u = ctx.saved_tensors
        dh = dh.contiguous()
        if ctx.fp8 is not None and not ctx.fp8[0].parts and ctx.fp8[0].prequant is None:
            from .fp8 import swiglu_bwd_quant
            acc, need_dg, need_du = ctx.fp8
            q, sq, dg, du = swiglu_bwd_quant(g, u, dh, need_dg, need_du)
            out_g, out_u = _grad_or_placeholder(g, dg, need_dg), _grad_or_placeholder(u, du, need_du)
            # the e4m3 rows stand for exactly these two tensors: the group checks that they reach
            # gate and up unchanged (not summed with another consumer's gradient)
            acc.prequant = (q, sq, (out_g, out_u))
            return out_g, out_u, None, None
        dg = torch.empty_like(g)
        du = torch.empty_like(u)
        rc = _hip.load().smt_swiglu_bwd(g.data_ptr(), u.data_ptr(), dh.data_ptr(), dg.data_ptr(), du.data_ptr(),
                                        g.numel(), _dt(g), _stream(g))
        _hip._check(rc, "smt_swiglu_bwd")
        return dg, du, None, None


def _grad_or_placeholder(like: torch.Tensor, grad, need) -> torch.Tensor:
    """The SwiGLU backward's gradient of gate (up) for autograd: the bf16 gradient itself, or a
    zero-stride placeholder of its shape that nothing reads -- carrying, when the producer wrote only the
    SMT module's row blocks (``need == ("mx_rows", tiles)``), that packed gradient as ``_smt_gpack``
    for linearZ.backward."""
    if grad is not None and need is True:
        return grad
    ph = like.new_zeros(()).expand_as(like)
    if grad is not None:
        ph._smt_gpack = grad
        from .fp8 import MxRowsNeed
        if isinstance(need, MxRowsNeed):
            need.delivered = True
    return ph


# ------------------------------------------------------------------------------------------------
# decode linears (opt-in: patch_llama(decode_linears=True))
# ------------------------------------------------------------------------------------------------
class DecodeLinearStats:
    """Routed launches of the decode-linear kernel by kind (``single``, ``group``: q/k/v in one launch,
    ``swiglu``: gate, up and SwiGLU in one launch). ``bias`` counts, among the ``single`` and ``group`` launches,
    those that added at least one bias (smt_linear_skinny_bias), once per launch; it is an attribute beside
    :meth:`as_dict`, whose keys stay the three kinds. A graph replay runs no Python and counts nothing."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.single = 0
        self.group = 0
        self.swiglu = 0
        self.bias = 0

    def as_dict(self) -> dict:
        return {"single": self.single, "group": self.group, "swiglu": self.swiglu}


decode_linear_stats = DecodeLinearStats()
# the two fused launches of the routing, read at call time (scripts/generate_cache_bench.py times the token with
# each off): q/k/v as one grouped launch, and gate/up/SwiGLU as one launch
DECODE_LINEAR_GROUP = True
DECODE_LINEAR_SWIGLU = True
# biased projections (Qwen2's q, k and v) go to the kernel's bias epilogue; off: they run what they ran before
DECODE_LINEAR_BIAS = True
# The routing's size rule: a launch goes to the kernel only if K <= 4096 and its weights hold at most 2^25
# elements (sum of N times K; 64 MiB of 16-bit weights). Every measured launch inside the rule, (N, K) =
# (4096, 4096), (1024, 4096) and the grouped (6144, 4096), is 1.3-3.0x faster than hipBLASLt, which sits on a
# floor of about 15 us per launch there; every measured launch outside it (K = 5120 and up, or N = 13824 and
# up) is slower or inside the baseline's own spread, 0.47-1.01x: hipBLASLt streams those at 0.40-0.74 of 8 TB/s
# (profiles/r20_decode_linear_bench.jsonl).
DECODE_LINEAR_MAX_K = 4096
DECODE_LINEAR_MAX_WEIGHT_ELEMS = 1 << 25
# Biased launches (against F.linear(x, W, b) per projection, profiles/r22_decode_linear_bench.jsonl): the grouped
# q/k/v launches, 2048 x 1536 and 4608 x 3584, are 2.0-6.9x faster at M = 1, 4, 16 and every single launch at
# K = 1536 is 1.19-2.2x faster, so those stay inside the rule above. A single biased weight at K = 3584 is faster
# at M <= 4 (1.08-2.0x) but at M = 16 3584 x 3584 gains only 1.03x and 512 x 3584 loses (0.91-0.93x): a single
# biased launch with K above DECODE_LINEAR_BIAS_SINGLE_MAX_K is routed at up to DECODE_LINEAR_BIAS_FEW_ROWS rows
# only (rows 5-15 were not timed and count as 16).
DECODE_LINEAR_BIAS_SINGLE_MAX_K = 2048
DECODE_LINEAR_BIAS_FEW_ROWS = 4


def _decode_routes(x, weights, biases=(), need_cuda: bool = True, allow_bias: bool = False) -> bool:
    """The routing's decision for one launch: :func:`decode_linear_reason` admits it and the size rule holds,
    for a single biased weight also the ``DECODE_LINEAR_BIAS_*`` constants. ``allow_bias``: only the PLAIN call
    sites of :func:`decode_routed_linear_forward` pass it; the gate/up/SwiGLU launch has no biased form, so a
    biased MLP pair is refused here and runs the unfused path."""
    if decode_linear_reason(x, weights, biases, need_cuda, allow_bias=allow_bias) is not None:
        return False
    K = x.shape[-1]
    if (len(weights) == 1 and any(b is not None for b in biases) and K > DECODE_LINEAR_BIAS_SINGLE_MAX_K
            and x.numel() // K > DECODE_LINEAR_BIAS_FEW_ROWS):
        return False
    return K <= DECODE_LINEAR_MAX_K and sum(w.shape[0] for w in weights) * K <= DECODE_LINEAR_MAX_WEIGHT_ELEMS


def _aligned16(t: torch.Tensor) -> bool:
    return (t.storage_offset() * t.element_size()) % 16 == 0 and (t.device.type == "meta" or t.data_ptr() % 16 == 0)


def decode_linear_reason(x: torch.Tensor, weights, biases=(), need_cuda: bool = True, allow_bias: bool = False):
    """Why ``x @ W^T`` for these weights cannot go to the decode-linear kernel (smt_linear_skinny), or
    None if it can. The one predicate of the routing; every condition of include/smt_linear.h:
    gradients off; ROCm bf16 / fp16 tensors of one dtype; 1..16 rows after flattening the leading
    dimensions; no bias and no fp8 copy on a weight; K % 32 == 0, N % 16 == 0; unit inner strides, row
    strides multiples of 8 and 16-byte aligned storage. ``need_cuda=False`` lifts the device condition
    (the host tests run the rest on CPU and meta tensors). ``allow_bias=True`` (the routing's form) admits
    biases that the bias epilogue takes (smt_linear_skinny_bias): one entry per weight, each None or 1-D ``[N]``
    of x's dtype on x's device, unit stride, 16-byte aligned, no gradient needed."""
    if torch.is_grad_enabled():
        if allow_bias and any(b is not None and b.requires_grad for b in biases):
            return "bias needs a gradient (gradients are enabled)"
        return "gradients are enabled"
    if not allow_bias and any(b is not None for b in biases):
        return "bias"
    if x.dtype not in (torch.bfloat16, torch.float16):
        return f"dtype {x.dtype}"
    if need_cuda and x.device.type != "cuda":
        return f"device {x.device}"
    if x.dim() < 1 or x.shape[-1] == 0:
        return "x has no feature dimension"
    K = x.shape[-1]
    rows = x.numel() // K
    if not 1 <= rows <= _hip.SKINNY_MAX_M:
        return f"{rows} rows"
    if K % 32:
        return f"K {K} is not a multiple of 32"
    if x.stride(-1) != 1 or not _aligned16(x):
        return "x inner stride or alignment"
    if not (x.is_contiguous() or (x.dim() == 2 and x.stride(0) % 8 == 0 and x.stride(0) >= K)):
        return "x rows do not flatten to one aligned stride"
    if not 1 <= len(weights) <= _hip.SKINNY_MAX_OUT:
        return f"{len(weights)} weights"
    for w in weights:
        if w.dim() != 2 or w.shape[1] != K:
            return f"weight shape {tuple(w.shape)} for K {K}"
        if w.dtype != x.dtype or w.device != x.device:
            return f"weight {w.dtype} on {w.device} beside x {x.dtype} on {x.device}"
        if getattr(w, "_smt_fp8", None) is not None:
            return "fp8 weight"
        if w.shape[0] == 0 or w.shape[0] % 16:
            return f"N {w.shape[0]} is not a multiple of 16"
        if w.stride(1) != 1 or w.stride(0) % 8 or w.stride(0) < K or not _aligned16(w):
            return "weight stride or alignment"
    if any(b is not None for b in biases):
        if len(biases) != len(weights):
            return f"{len(biases)} biases for {len(weights)} weights"
        for b, w in zip(biases, weights):
            if b is None:
                continue
            if b.dim() != 1 or b.shape[0] != w.shape[0]:
                return f"bias shape {tuple(b.shape)} for N {w.shape[0]}"
            if b.dtype != x.dtype or b.device != x.device:
                return f"bias {b.dtype} on {b.device} beside x {x.dtype} on {x.device}"
            if b.stride(0) != 1 or not _aligned16(b):
                return "bias stride or alignment"
    return None


def _decode_call(x, weights, epilogue, what, biases=None):
    biased = biases is not None and any(b is not None for b in biases)
    why = decode_linear_reason(x, weights, tuple(biases) if biased else (), allow_bias=True)
    if why is not None:                 # no quiet fall-back: the routing asks the predicate first
        raise RuntimeError(f"{what}: the call does not qualify for the decode-linear kernel ({why})")
    if epilogue == _hip.SKINNY_SWIGLU and weights[0].shape[0] != weights[1].shape[0]:
        raise RuntimeError(f"{what}: gate and up of unequal width")
    K = x.shape[-1]
    ys = _hip.linear_skinny(x.reshape(-1, K), list(weights), epilogue, biases=list(biases) if biased else None)
    if biased:
        decode_linear_stats.bias += 1
    return [y.view(*x.shape[:-1], y.shape[-1]) for y in ys]


def decode_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    """``x @ weight^T (+ bias)`` for at most 16 rows of ``x``: the weight-streaming kernel on a ROCm device (an
    error if the call does not qualify, :func:`decode_linear_reason`), ``F.linear`` on the CPU. The bias is
    added in fp32 before the one rounding (smt_linear_skinny_bias)."""
    if x.device.type != "cuda":
        return torch.matmul(x, weight.t()) if bias is None else torch.nn.functional.linear(x, weight, bias)
    y = _decode_call(x, (weight,), _hip.SKINNY_PLAIN, "decode_linear", None if bias is None else (bias,))[0]
    decode_linear_stats.single += 1
    return y


def decode_linear_group(x: torch.Tensor, weights, biases=None) -> list:
    """``[x @ W^T for W in weights]`` (1..3 weights) as one launch that reads ``x`` once; bit for bit
    the single calls. ``biases``: one entry per weight, None or that output's bias."""
    if x.device.type != "cuda":
        if biases is None:
            return [torch.matmul(x, w.t()) for w in weights]
        return [torch.matmul(x, w.t()) if b is None else torch.nn.functional.linear(x, w, b) for w, b in zip(weights, biases)]
    ys = _decode_call(x, tuple(weights), _hip.SKINNY_PLAIN, "decode_linear_group", biases)
    decode_linear_stats.group += 1
    return ys


def decode_swiglu(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor) -> torch.Tensor:
    """``silu(x @ w_gate^T) * (x @ w_up^T)`` as one launch; bit for bit two :func:`decode_linear` calls
    and the fused SwiGLU forward. On the CPU, torch's chain."""
    if x.device.type != "cuda":
        return torch.nn.functional.silu(torch.matmul(x, w_gate.t())) * torch.matmul(x, w_up.t())
    y = _decode_call(x, (w_gate, w_up), _hip.SKINNY_SWIGLU, "decode_swiglu")[0]
    decode_linear_stats.swiglu += 1
    return y


# ------------------------------------------------------------------------------------------------
# decode linears on e4m3 operands (opt-in: patch_llama(decode_linears=True, decode_fp8=True))
# ------------------------------------------------------------------------------------------------
class DecodeFp8Stats:
    """Launches of the e4m3 decode-linear kernel by kind, and ``quant``: the activation quantisations
    (smt_quant_rows_e4m3) those calls had to launch themselves because no producer had left the copy on the
    tensor (o_proj's and down_proj's input). A graph replay runs no Python and counts nothing."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.single = 0
        self.group = 0
        self.swiglu = 0
        self.quant = 0

    def as_dict(self) -> dict:
        return {"single": self.single, "group": self.group, "swiglu": self.swiglu, "quant": self.quant}


decode_fp8_stats = DecodeFp8Stats()
# The fp8 routing's size rule (read at call time; DECODE_FP8_RULE = False sends every qualifying launch to the
# kernel, which scripts/generate_cache_bench.py uses to time the token without the rule). A launch goes to the
# kernel only if K <= 4096 and its e4m3 weights (sum of N times K bytes) hold at most 2^25 bytes at any number of
# rows, or at most 2^27 bytes at up to 4 rows. Measured against today's route (fp8.quant_rows where the copy is
# not there, torch._scaled_mm per weight) at M = 1, 4, 16 (profiles/r21_decode_linear_fp8_bench.jsonl):
# inside the rule, (N, K) = (4096, 4096), (1024, 4096), the grouped (6144, 4096) and o_proj with its quantisation
# launch are 1.32-3.48x faster at every M, (14336, 4096) and the SwiGLU pair 1.37-1.83x at M = 1 and 4, each in
# every round with a margin far above the baseline's spread; outside it, (14336, 4096) at M = 16 (0.74x), the pair
# at M = 16 (1.05x in the recorded run, 0.98x in the run before it: a margin that changes sign between two runs),
# K = 14336 (0.87-1.03x, inside the spread where above 1) and the 13B shapes (0.42-0.75x; 13b.gate at M <= 4 was
# 1.05-1.11x, which the K limit gives up) keep today's route.
DECODE_FP8_RULE = True
DECODE_FP8_MAX_K = 4096
DECODE_FP8_MAX_WEIGHT_BYTES = 1 << 25
DECODE_FP8_FEW_ROWS = 4
DECODE_FP8_MAX_WEIGHT_BYTES_FEW_ROWS = 1 << 27


def _fp8_copy(w):
    """The Fp8Weight of ``w``: ``w`` itself, or the copy a weight tensor carries as ``_smt_fp8``; None if neither."""
    fw = getattr(w, "_smt_fp8", w)
    return fw if hasattr(fw, "w8") and hasattr(fw, "sw") else None


def decode_linear_fp8_reason(x: torch.Tensor, fws, biases=(), need_cuda: bool = True):
    """Why ``x @ W^T`` on the e4m3 copies ``fws`` (``Fp8Weight``s, or weights that carry one as ``_smt_fp8``)
    cannot go to smt_linear_skinny_fp8, or None if it can: gradients off; a ROCm bf16 activation of 1..16
    rows (bf16 only: the row quantiser smt_quant_rows_e4m3 reads nothing else, although the kernel itself also
    writes fp16); every weight with its e4m3 copy; no bias; K % 64 == 0, N % 16 == 0; w8 with unit inner
    stride, a row stride that is a multiple of 16 and 16-byte aligned storage, contiguous fp32 scales. The
    strides of ``x`` do not matter: the kernel reads its e4m3 copy (``fp8.quant_rows_cached``), which is
    contiguous. ``need_cuda=False`` lifts the device condition."""
    if torch.is_grad_enabled():
        return "gradients are enabled"
    if any(b is not None for b in biases):
        return "bias"
    if x.dtype != torch.bfloat16:
        return f"dtype {x.dtype} (the e4m3 row quantiser reads bf16)"
    if need_cuda and x.device.type != "cuda":
        return f"device {x.device}"
    if x.dim() < 1 or x.shape[-1] == 0:
        return "x has no feature dimension"
    K = x.shape[-1]
    rows = x.numel() // K
    if not 1 <= rows <= _hip.SKINNY_MAX_M:
        return f"{rows} rows"
    if K % 64:
        return f"K {K} is not a multiple of 64"
    if not 1 <= len(fws) <= _hip.SKINNY_MAX_OUT:
        return f"{len(fws)} weights"
    for w in fws:
        fw = _fp8_copy(w)
        if fw is None:
            return "weight without an fp8 copy"
        w8, sw = fw.w8, fw.sw
        if w8.dim() != 2 or w8.shape[1] != K or w8.element_size() != 1:
            return f"w8 shape {tuple(w8.shape)} {w8.dtype} for K {K}"
        if w8.device != x.device or sw.device != x.device:
            return f"fp8 weight on {w8.device} beside x on {x.device}"
        if w8.shape[0] == 0 or w8.shape[0] % 16:
            return f"N {w8.shape[0]} is not a multiple of 16"
        if w8.stride(1) != 1 or w8.stride(0) % 16 or w8.stride(0) < K or not _aligned16(w8):
            return "w8 stride or alignment"
        if sw.dtype != torch.float32 or sw.numel() != w8.shape[0] or not sw.is_contiguous() or not _aligned16(sw):
            return "sw is not a contiguous, 16-byte aligned fp32 vector of N scales"
    return None


def _decode_fp8_routes(x, weights, biases=(), need_cuda: bool = True) -> bool:
    """The fp8 routing's decision for one launch: :func:`decode_linear_fp8_reason` admits it and, unless
    ``DECODE_FP8_RULE`` is off, the size rule holds."""
    if decode_linear_fp8_reason(x, weights, biases, need_cuda) is not None:
        return False
    if not DECODE_FP8_RULE:
        return True
    K = x.shape[-1]
    limit = DECODE_FP8_MAX_WEIGHT_BYTES_FEW_ROWS if x.numel() // K <= DECODE_FP8_FEW_ROWS else DECODE_FP8_MAX_WEIGHT_BYTES
    return K <= DECODE_FP8_MAX_K and sum(_fp8_copy(w).w8.shape[0] for w in weights) * K <= limit


def _decode_fp8_call(x, fws, epilogue, what):
    why = decode_linear_fp8_reason(x, fws)
    if why is not None:                 # no quiet fall-back: the routing asks the predicate first
        raise RuntimeError(f"{what}: the call does not qualify for the e4m3 decode-linear kernel ({why})")
    fws = [_fp8_copy(w) for w in fws]
    if epilogue == _hip.SKINNY_SWIGLU and fws[0].w8.shape[0] != fws[1].w8.shape[0]:
        raise RuntimeError(f"{what}: gate and up of unequal width")
    from .fp8 import quant_rows_cached
    c = x.__dict__.get("_smt_q8")
    if c is None or c[0] != x._version:
        decode_fp8_stats.quant += 1
    x8, sx = quant_rows_cached(x)
    ys = _hip.linear_skinny_fp8(x8, sx, [(fw.w8, fw.sw) for fw in fws], x.dtype, epilogue)
    return [y.view(*x.shape[:-1], y.shape[-1]) for y in ys]


def decode_linear_fp8(x: torch.Tensor, fw) -> torch.Tensor:
    """``x @ W^T`` for at most 16 rows of a bf16 ``x`` on the e4m3 copy ``fw`` (an ``Fp8Weight``) of ``W``: one
    launch of the weight-streaming kernel (smt_linear_skinny_fp8) on ``fw.w8`` / ``fw.sw`` as they are at the
    call, and on the e4m3 copy of ``x`` that ``fp8.quant_rows_cached`` returns (the one the fused RMSNorm left
    on ``x``, else one smt_quant_rows_e4m3 launch). An error if the call does not qualify
    (:func:`decode_linear_fp8_reason`). No CPU path: the fp8 path has none."""
    y = _decode_fp8_call(x, (fw,), _hip.SKINNY_PLAIN, "decode_linear_fp8")[0]
    decode_fp8_stats.single += 1
    return y


def decode_linear_group_fp8(x: torch.Tensor, fws) -> list:
    """``[x @ W^T for W in ...]`` on 1..3 e4m3 copies as one launch that reads the e4m3 ``x`` once; bit for bit
    the single calls."""
    ys = _decode_fp8_call(x, tuple(fws), _hip.SKINNY_PLAIN, "decode_linear_group_fp8")
    decode_fp8_stats.group += 1
    return ys


def decode_swiglu_fp8(x: torch.Tensor, fw_gate, fw_up) -> torch.Tensor:
    """``silu(x @ W_gate^T) * (x @ W_up^T)`` on the e4m3 copies as one launch; bit for bit two
    :func:`decode_linear_fp8` calls and the fused SwiGLU forward."""
    y = _decode_fp8_call(x, (fw_gate, fw_up), _hip.SKINNY_SWIGLU, "decode_swiglu_fp8")[0]
    decode_fp8_stats.swiglu += 1
    return y


def _sync_for_decode(*mods) -> None:
    """The SMT modules' write-back of their tiles into W, as their own forward does first. ``sync_weight``
    also re-quantises the rows and columns of the e4m3 copies that the tiles touch (``Fp8Weight.refresh``), as
    the module's own forward does at that point, so the fp8 route needs nothing more: after it ``w8`` holds
    the rows the module's forward would use."""
    for m in mods:
        if getattr(m, "writeback_on_forward", False) and hasattr(m, "sync_weight"):
            m.sync_weight()


def _decode_prev_forward(self, x):
    prev = self.__dict__.get("_smt_decode_prev_forward")
    return prev(x) if prev is not None else type(self).forward(self, x)


def decode_routed_linear_forward(self, x):
    """Instance forward of a routed projection: a qualifying call (a decode step) goes to the kernel,
    anything else to the forward the module had. A q_proj with ``_smt_decode_group`` computes k_proj's and
    v_proj's outputs in the same launch and attaches them to ``x``; k_proj and v_proj take them only from
    that very tensor at the same version and for their own weight."""
    st = x.__dict__.get("_smt_decode_kv") if isinstance(x, torch.Tensor) else None
    if st is not None:
        if st[0] == x._version and not torch.is_grad_enabled():
            for i in (1, 3):
                if st[i] is self.weight and st[i + 1] is not None:
                    y = st[i + 1]
                    st[i + 1] = None
                    if st[2] is None and st[4] is None:
                        del x.__dict__["_smt_decode_kv"]
                    return y
        else:
            del x.__dict__["_smt_decode_kv"]
    bias = getattr(self, "bias", None)
    # the bias epilogue: on for what patch_model / route_decode_linears(bias=True) routed, while the switch is on
    with_bias = bool(DECODE_LINEAR_BIAS and self.__dict__.get("_smt_decode_bias"))
    fp8 = self.__dict__.get("_smt_decode_fp8", False)
    group = self.__dict__.get("_smt_decode_group")
    if group is not None and DECODE_LINEAR_GROUP:
        kv = [r() for r in group]
        if all(m is not None for m in kv):
            ws = (self.weight, kv[0].weight, kv[1].weight)
            if fp8 and _decode_fp8_routes(x, ws, (bias, kv[0].bias, kv[1].bias)):
                _sync_for_decode(self, *kv)
                q, k, v = decode_linear_group_fp8(x, ws)
                x.__dict__["_smt_decode_kv"] = [x._version, ws[1], k, ws[2], v]
                return q
            bs = (bias, kv[0].bias, kv[1].bias)
            if _decode_routes(x, ws, bs, allow_bias=with_bias):
                _sync_for_decode(self, *kv)
                q, k, v = decode_linear_group(x, ws, bs)
                x.__dict__["_smt_decode_kv"] = [x._version, ws[1], k, ws[2], v]
                return q
    if fp8 and _decode_fp8_routes(x, (self.weight,), (bias,)):
        _sync_for_decode(self)
        return decode_linear_fp8(x, self.weight)
    if _decode_routes(x, (self.weight,), (bias,), allow_bias=with_bias):
        _sync_for_decode(self)
        return decode_linear(x, self.weight, bias)
    return _decode_prev_forward(self, x)


def _decode_routable(m) -> bool:
    from .smt.smt import LinearLayer_MatrixSparsity
    return (type(m) is nn.Linear or isinstance(m, LinearLayer_MatrixSparsity)) and "_smt_decode_routed" not in m.__dict__


def _route_decode_linear(m) -> None:
    if "forward" in m.__dict__:
        m.__dict__["_smt_decode_prev_forward"] = m.__dict__["forward"]
    m.forward = decode_routed_linear_forward.__get__(m, type(m))
    m.__dict__["_smt_decode_routed"] = True


def _unroute_decode_linear(m) -> None:
    if m.__dict__.pop("_smt_decode_routed", None):
        m.__dict__.pop("forward", None)
        prev = m.__dict__.pop("_smt_decode_prev_forward", None)
        if prev is not None:
            m.__dict__["forward"] = prev
    m.__dict__.pop("_smt_decode_group", None)
    m.__dict__.pop("_smt_decode_fp8", None)
    m.__dict__.pop("_smt_decode_bias", None)


def route_decode_linears(model: nn.Module, fp8: bool = False, family: "ModelFamily" = None, bias: bool = True) -> int:
    """What ``patch_llama(decode_linears=True)`` adds, by itself: the routed forwards of the projections
    and of a bias-free ``lm_head``, the q/k/v group and the MLPs' fused launch. ``fp8``
    (``patch_llama(decode_fp8=True)``): the routed forwards and the MLPs first try the e4m3 kernel on weights
    that carry an fp8 copy. ``family``: whose classes to match. The default is now the model's own
    (:func:`model_family`), else LLaMA's: a direct call on a Qwen2 model, which used to match no class and route
    nothing, routes its projections. ``bias`` (default on): the routed projections that carry a bias go to the
    kernel's bias epilogue; off, they run what they ran before, as every biased projection did until now.
    :func:`patch_llama` passes the LLaMA family and ``bias=False`` and so routes exactly what it always routed;
    :func:`patch_model` passes the model's family and ``bias=True``. Returns the number of linears
    routed by this call. :func:`unroute_decode_linears` (and :func:`unpatch_llama`) removes all of it."""
    fam = family or model_family(model) or FAMILIES["llama"]
    routed = 0
    for m in model.modules():
        if isinstance(m, fam.attention):
            names = ("q_proj", "k_proj", "v_proj", "o_proj")
        elif isinstance(m, fam.mlp):
            names = ("gate_proj", "up_proj", "down_proj")
            m.__dict__["_smt_decode_linears"] = True
            if fp8:
                m.__dict__["_smt_decode_fp8"] = True
        elif isinstance(m, fam.causal_lm):
            names = ("lm_head",) if getattr(getattr(m, "lm_head", None), "bias", None) is None else ()
        else:
            continue
        for n in names:
            lin = getattr(m, n, None)
            if lin is not None and _decode_routable(lin):
                _route_decode_linear(lin)
                routed += 1
            if fp8 and lin is not None and lin.__dict__.get("_smt_decode_routed"):
                lin.__dict__["_smt_decode_fp8"] = True
            if bias and lin is not None and lin.__dict__.get("_smt_decode_routed"):
                lin.__dict__["_smt_decode_bias"] = True
        if isinstance(m, fam.attention) and all(
                getattr(m, n, None) is not None and getattr(m, n).__dict__.get("_smt_decode_routed") for n in names[:3]):
            m.q_proj.__dict__["_smt_decode_group"] = (weakref.ref(m.k_proj), weakref.ref(m.v_proj))
    return routed


def unroute_decode_linears(model: nn.Module) -> None:
    for m in model.modules():
        m.__dict__.pop("_smt_decode_linears", None)
        m.__dict__.pop("_smt_decode_fp8", None)
        _unroute_decode_linear(m)


def fused_mlp_forward(self, x):
    """Drop-in for ``LlamaMLP.forward`` (SiLU activation). With an fp8 down_proj the SwiGLU also emits
    down_proj's quantised input; a frozen plain down_proj then never reads the bf16 activation."""
    if self.__dict__.get("_smt_decode_linears") and DECODE_LINEAR_SWIGLU:
        # patch_llama(decode_linears=True): gate, up and the SwiGLU of a decode step as one launch
        g, u = self.gate_proj, self.up_proj
        if (g.__dict__.get("_smt_decode_routed") and u.__dict__.get("_smt_decode_routed")
                and g.weight.shape[0] == u.weight.shape[0]):
            if self.__dict__.get("_smt_decode_fp8") and _decode_fp8_routes(x, (g.weight, u.weight), (g.bias, u.bias)):
                _sync_for_decode(g, u)
                return self.down_proj(decode_swiglu_fp8(x, g.weight, u.weight))
            if _decode_routes(x, (g.weight, u.weight), (g.bias, u.bias)):
                _sync_for_decode(g, u)
                return self.down_proj(decode_swiglu(x, g.weight, u.weight))
    from .fp8 import sole_swiglu_consumer
    with sole_swiglu_consumer():             # gate / up feed only the SwiGLU below
        gate, up = self.gate_proj(x), self.up_proj(x)
    d = self.down_proj
    if getattr(d.weight, "_smt_fp8", None) is not None and gate.shape[-1] <= 16384:
        from . import fp8
        if fp8.FUSED_SWIGLU_QUANT and fp8.FUSED_SWIGLU_FWD_QUANT:
            frozen_plain = type(d) is torch.nn.Linear and not d.weight.requires_grad
            return d(FusedSwiGLUFn.apply(gate, up, True, not frozen_plain))
    return d(FusedSwiGLUFn.apply(gate, up))


# ------------------------------------------------------------------------------------------------
# causal-LM cross entropy
# ------------------------------------------------------------------------------------------------
class FusedCrossEntropyFn(torch.autograd.Function):
    """``F.cross_entropy(logits.float(), labels, ignore_index, reduction=sum) / denom`` over 16-bit
    (bf16 / fp16) logits ``[N, V]`` without the fp32 copy: one pass for the row log-sum-exp, one for the
    gradient in the logits' dtype. ``denom``: fp32 device scalar (valid-label count for the mean, or num_items_in_batch)."""

    @staticmethod
    def forward(ctx, logits2d, labels, ignore_index, denom):
        _need(logits2d, "cross entropy logits")
        if logits2d.stride(1) != 1 or logits2d.stride(0) % 8 or logits2d.data_ptr() % 16:
            logits2d = logits2d.contiguous()
        N, V = logits2d.shape
        labels = labels.to(device=logits2d.device, dtype=torch.int64).contiguous()
        if labels.numel() != N:
            raise ValueError(f"cross entropy: {labels.numel()} labels for {N} logit rows")
        lse = torch.empty(N, dtype=torch.float32, device=logits2d.device)
        rows = torch.empty(N, dtype=torch.float32, device=logits2d.device)
        rc = _hip.load().smt_ce_fwd(logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), N, V,
                                    int(ignore_index), lse.data_ptr(), rows.data_ptr(), _dt(logits2d), _stream(logits2d))
        _hip._check(rc, "smt_ce_fwd")
        ctx.save_for_backward(logits2d, labels, lse, denom)
        ctx.ignore_index = int(ignore_index)
        return rows.sum() / denom

    @staticmethod
    def backward(ctx, dloss):
        logits2d, labels, lse, denom = ctx.saved_tensors
        N, V = logits2d.shape
        scale = (dloss.float() / denom).reshape(1).contiguous()
        dlogits = torch.empty_like(logits2d)
        rc = _hip.load().smt_ce_bwd(logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), lse.data_ptr(),
                                    scale.data_ptr(), N, V, ctx.ignore_index, dlogits.data_ptr(), dlogits.stride(0),
                                    _dt(logits2d), _stream(logits2d))
        _hip._check(rc, "smt_ce_bwd")
        return dlogits, None, None, None


def fused_causal_lm_loss(logits, labels, vocab_size, num_items_in_batch=None, ignore_index=-100,
                         shift_labels=None, **kwargs):
    """Drop-in for ``transformers.loss.loss_utils.ForCausalLMLoss`` (the loss of
    ``LlamaForCausalLM.forward``): labels shifted left by one with ``ignore_index`` padding, mean over
    non-ignored tokens, or sum / ``num_items_in_batch``."""
    logits2d = logits.reshape(-1, vocab_size)
    shift = _shifted_labels(labels, ignore_index, shift_labels).to(logits2d.device)
    if num_items_in_batch is None:
        denom = (shift != ignore_index).sum().to(torch.float32)
    else:
        denom = torch.as_tensor(num_items_in_batch, device=logits2d.device).to(torch.float32)
    return FusedCrossEntropyFn.apply(logits2d, shift, ignore_index, denom)


def _shifted_labels(labels, ignore_index, shift_labels):
    """ForCausalLMLoss's label shift: position s is scored against token s + 1, the last position
    against ``ignore_index``."""
    if shift_labels is None:
        labels = nn.functional.pad(labels, (0, 1), value=ignore_index)
        shift_labels = labels[..., 1:]
    return shift_labels.reshape(-1)


# ------------------------------------------------------------------------------------------------
# LM head + causal-LM cross entropy, row chunk by row chunk
# ------------------------------------------------------------------------------------------------
LM_HEAD_CHUNK_ROWS = int(os.environ.get("SMT_LM_HEAD_CHUNK_ROWS", "4096"))
# a trainable head (the warm-up) adds each chunk's dlogits^T @ hidden into an fp32 [V, H] accumulator:
# longer chunks mean fewer, longer-K GEMMs (4096-row chunks: 8 x 4.37 ms at the 8B head,
# profiles/r05_k_kernel_stats.csv). The chunk buffer is transient in the forward, below the warm-up's
# peak (the backward's bf16 gradients of every parameter).
LM_HEAD_DW_CHUNK_ROWS = int(os.environ.get("SMT_LM_HEAD_DW_CHUNK_ROWS", "16384"))
# fp16 only: the forward's dlogits carry 2^(ceil(log2(denom)) + this) / denom, i.e. lie in [-32, 32]
# (FusedLMHeadLossFn). dh = dlogits @ W is a p-weighted average of W's rows times that factor: below
# 64 max|W|, three decades under fp16's 65504 for any head whose weights are below 1.
LM_HEAD_FP16_HEADROOM_BITS = 4


class FusedLMHeadLossFn(torch.autograd.Function):
    """``lm_head`` (no bias) followed by :class:`FusedCrossEntropyFn`, without the full ``[T, V]``
    logits. At B 16 x S 2048 x V 128256 the unfused pair keeps the bf16 logits (8.4 GB) for the loss
    backward and allocates the same again for ``dlogits`` at the start of the backward, when every
    activation of the step is still alive: that 16.8 GB is the SMT step's peak HBM (and the
    full fine-tuning warm-up's).

    Here each chunk of ``LM_HEAD_CHUNK_ROWS`` rows runs, inside the forward: the logits GEMM
    (``hidden @ W^T``), the row log-sum-exp (``smt_ce_fwd``), and (when ``hidden`` or ``W`` needs a
    gradient) ``dlogits`` for a unit upstream gradient written over the chunk's logits
    (``smt_ce_bwd`` in place; each element is read and written by one thread), the data gradient
    ``dlogits @ W`` (TN on the engine's transposed copy when there is one, as
    :class:`..engine.FrozenLinearFn` runs it) and, for a trainable head (the warm-up), the chunk's
    ``dlogits^T @ hidden`` added into an fp32 ``[V, H]`` accumulator (hipBLASLt bf16 x bf16 -> fp32,
    beta 1), rounded to bf16 once after the last chunk. Only ``dh [T, H]`` (268 MB) and ``dW``
    are kept; the backward scales them by the upstream gradient.

    Per row this is the unfused arithmetic: the same GEMM products, the same kernels and, for the
    upstream gradient 1 that ``loss.backward()`` gives (``engine.backward`` with one accumulation
    step), the same ``dlogits`` scale ``1 / denom``. Any other upstream gradient is applied to the
    16-bit ``dh`` / ``dW`` (one more rounding than folding it into ``dlogits`` first, exact for powers
    of two while the result stays in the format's normal range).

    bf16 has fp32's exponent range, so ``dlogits / denom`` survives its rounding whatever the upstream
    gradient will be. fp16 does not: at N rows a non-label entry is about ``p / N``, below fp16's
    smallest subnormal (6e-8) from N x V of a few million on, and the loss scale that exists to lift
    it arrives only in the backward, after the rounding. (Applied to the fp16 ``dh`` by ``torch.mul``
    it was also cast to fp16 first: 2^16, the engine's initial scale, became inf.) For fp16 the
    forward therefore computes ``dlogits`` with the scale ``k / denom``, ``k = 2^(ceil(log2(denom))
    + 4)`` taken from ``denom``'s exponent on the device (no host synchronisation): ``k / denom`` lies
    in [16, 32), ``dlogits`` in [-32, 32] (eager's own values at loss scale 2^16 and N = 4096, 8 x
    eager's at N = 32768). ``dh`` is an average of ``W``'s rows times that factor and cannot overflow;
    ``dW`` is a sum over all rows, so its fp32 accumulator is rounded to fp16 under one shared
    power-of-two exponent taken from its largest entry. The backward multiplies by ``dloss / k`` (and
    that exponent) in fp32 and rounds once: an exact rescale for the power-of-two ``dloss`` a loss
    scaler gives, so the one rounding that can lose range is the last one, at the magnitude eager
    rounds at. Same kernels, same GEMMs, the chunked memory profile; the bf16 path is the ``k = 1``
    case and is not touched (tests/test_gpu_fp16_loss_scale.py).

    Whether hipBLASLt picks the same kernel for a chunk's GEMM shape as for the whole batch's
    decides bit-identity of the logits and ``dh``; ``dW`` sums the same fp32 products in chunk order
    before its one rounding. tests/test_gpu_cross_entropy.py checks both."""

    @staticmethod
    def forward(ctx, hidden, weight, weight_t, labels, ignore_index, denom, chunk_rows, grad_enabled=True):
        _need(hidden, "lm head loss")
        _need(weight, "lm head loss", like=hidden)
        h2 = _rows2d(hidden)
        N, H = h2.shape
        V = weight.shape[0]
        if weight.shape[1] != H:
            raise ValueError(f"lm head loss: weight {tuple(weight.shape)} for hidden size {H}")
        if V % 8:
            raise ValueError(f"lm head loss: vocabulary {V} is not a multiple of 8")
        labels = labels.to(device=hidden.device, dtype=torch.int64).contiguous()
        if labels.numel() != N:
            raise ValueError(f"lm head loss: {labels.numel()} labels for {N} rows")
        # needs_input_grad reflects requires_grad even under torch.no_grad() (an evaluation forward with
        # labels): the caller passes the grad mode it ran under (inside forward it is always off)
        need_dh = bool(ctx.needs_input_grad[0]) and grad_enabled
        need_dw = bool(ctx.needs_input_grad[1]) and grad_enabled
        lib = _hip.load()
        stream = _stream(hidden)
        dt = _dt(hidden)
        lse = torch.empty(N, dtype=torch.float32, device=hidden.device)
        rows = torch.empty(N, dtype=torch.float32, device=hidden.device)
        dh = torch.empty((N, H), dtype=hidden.dtype, device=hidden.device) if need_dh else None
        denom32 = denom.to(torch.float32)
        prescale = None
        if hidden.dtype == torch.float16:
            # k = 2^(ceil(log2(denom)) + LM_HEAD_FP16_HEADROOM_BITS) from denom's exponent field, on the
            # device: k / denom lies in [16, 32)
            mant, expo = torch.frexp(denom32)
            expo = expo - (mant == 0.5).to(expo.dtype) + LM_HEAD_FP16_HEADROOM_BITS
            prescale = _pow2(expo)
            scale = (prescale / denom32).reshape(1).contiguous()
        else:
            scale = (1.0 / denom32).reshape(1).contiguous()
        C = max(1, min(max(int(chunk_rows), LM_HEAD_DW_CHUNK_ROWS if need_dw else 0), N))
        buf = torch.empty((C, V), dtype=hidden.dtype, device=hidden.device)
        w_dgrad = weight_t.t() if weight_t is not None else weight
        acc = torch.empty((V, H), dtype=torch.float32, device=hidden.device) if need_dw else None
        for r0 in range(0, N, C):
            c = min(C, N - r0)
            lg = buf[:c]
            hc = h2[r0:r0 + c]
            torch.mm(hc, weight.t(), out=lg)
            rc = lib.smt_ce_fwd(lg.data_ptr(), lg.stride(0), labels[r0:].data_ptr(), c, V, int(ignore_index),
                                lse[r0:].data_ptr(), rows[r0:].data_ptr(), dt, stream)
            _hip._check(rc, "smt_ce_fwd")
            if need_dh or need_dw:
                rc = lib.smt_ce_bwd(lg.data_ptr(), lg.stride(0), labels[r0:].data_ptr(), lse[r0:].data_ptr(),
                                    scale.data_ptr(), c, V, int(ignore_index), lg.data_ptr(), lg.stride(0), dt, stream)
                _hip._check(rc, "smt_ce_bwd")
            if need_dh:
                torch.mm(lg, w_dgrad, out=dh[r0:r0 + c])
            if need_dw:
                if r0 == 0:
                    torch.mm(lg.t(), hc, out_dtype=torch.float32, out=acc)
                else:
                    torch.addmm(acc, lg.t(), hc, out_dtype=torch.float32, out=acc)
        del buf
        dw = dw_prescale = None
        if need_dw and prescale is not None:
            # fp16: dW sums N rows of dlogits x hidden (not an average like dh), so its magnitude is
            # not known before the sum is. It is kept as fp16 under one shared power-of-two exponent
            # taken from the accumulator's largest entry (that entry lands in [2^14, 2^15))
            lo, hi = torch.aminmax(acc)
            _m, e = torch.frexp(torch.maximum(hi, -lo))
            shift = _pow2(torch.clamp(15 - e, min=-112, max=60))
            dw = acc.mul_(shift).to(weight.dtype)
            dw_prescale = prescale * shift
            del acc
        elif need_dw:
            dw = acc.to(weight.dtype)
            del acc
        ctx.save_for_backward(dh, dw, prescale, dw_prescale)
        ctx.shape = hidden.shape
        return rows.sum() / denom

    @staticmethod
    def backward(ctx, dloss):
        dh, dw, prescale, dw_prescale = ctx.saved_tensors
        scale = dloss.float()
        if prescale is not None:
            gh = _mul_fp32_scalar(dh, scale / prescale).view(ctx.shape) if dh is not None else None
            gw = _mul_fp32_scalar(dw, scale / dw_prescale) if dw is not None else None
            return gh, gw, None, None, None, None, None, None
        gh = torch.mul(dh, scale).view(ctx.shape) if dh is not None else None
        gw = torch.mul(dw, scale) if dw is not None else None
        return gh, gw, None, None, None, None, None, None


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for an integer tensor e in [-126, 127], built in the exponent field: exact, where
    ``torch.ldexp`` on the device goes through ``pow`` (measured: ldexp(1, 16) = 65535.996)."""
    return torch.bitwise_left_shift(e.to(torch.int32) + 127, 23).view(torch.float32)


def _mul_fp32_scalar(t: torch.Tensor, s: torch.Tensor, chunk: int = 1 << 24) -> torch.Tensor:
    """``t * s`` for a contiguous fp16 ``t`` and an fp32 device scalar ``s``, the fp32 product rounded
    once. ``torch.mul(t, s)`` casts ``s`` to fp16 first: 2^16 becomes inf (and 0 x inf a nan), 1/3 loses
    13 bits. The fp32 product goes through ``chunk``-element pieces (64 MB), not a copy of ``t``."""
    out = torch.empty_like(t)
    src, dst = t.view(-1), out.view(-1)
    for i in range(0, src.numel(), chunk):
        dst[i:i + chunk].copy_(src[i:i + chunk].float().mul_(s))
    return out


def fused_lm_head_loss(hidden, lm_head: nn.Linear, labels, num_items_in_batch=None, ignore_index=-100,
                       shift_labels=None, chunk_rows=None):
    """``ForCausalLMLoss(lm_head(hidden), labels)`` through :class:`FusedLMHeadLossFn`."""
    shift = _shifted_labels(labels, ignore_index, shift_labels).to(hidden.device)
    if num_items_in_batch is None:
        denom = (shift != ignore_index).sum().to(torch.float32)
    else:
        denom = torch.as_tensor(num_items_in_batch, device=hidden.device).to(torch.float32)
    wt = getattr(lm_head.weight, "_smt_weight_t", None)
    return FusedLMHeadLossFn.apply(hidden, lm_head.weight, wt, shift, ignore_index, denom,
                                   LM_HEAD_CHUNK_ROWS if chunk_rows is None else chunk_rows, torch.is_grad_enabled())


def _fusable_lm_head(head) -> bool:
    w = getattr(head, "weight", None)
    return (type(head) is nn.Linear and head.bias is None and isinstance(w, torch.Tensor)
            and w.device.type == "cuda" and w.dtype in (torch.bfloat16, torch.float16)
            and getattr(w, "_smt_fp8", None) is None)


def fused_causal_lm_forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                            inputs_embeds=None, labels=None, use_cache=None, logits_to_keep=0, **kwargs):
    """Drop-in for ``LlamaForCausalLM.forward``. With labels, a bias-free bf16 ``lm_head`` (frozen in the
    SMT phase, trainable in the warm-up) and the fused loss patched in, the loss comes from
    :func:`fused_lm_head_loss` and the output carries
    ``logits=None`` (``fine_tune.py:710-711`` reads only ``outputs.loss``); anything else runs
    transformers' own forward."""
    if (labels is None or not _fusable_lm_head(self.lm_head) or not isinstance(logits_to_keep, int)
            or logits_to_keep != 0 or kwargs.get("return_dict") is False
            or getattr(self, "loss_function", None) is not fused_causal_lm_loss):
        return type(self).forward(self, input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                                  past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels,
                                  use_cache=use_cache, logits_to_keep=logits_to_keep, **kwargs)
    kwargs.pop("return_dict", None)
    from transformers.modeling_outputs import CausalLMOutputWithPast
    outputs = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                         past_key_values=past_key_values, inputs_embeds=inputs_embeds, use_cache=use_cache, **kwargs)
    loss = fused_lm_head_loss(outputs.last_hidden_state, self.lm_head, labels,
                              num_items_in_batch=kwargs.get("num_items_in_batch"),
                              shift_labels=kwargs.get("shift_labels"))
    return CausalLMOutputWithPast(loss=loss, logits=None, past_key_values=outputs.past_key_values,
                                  hidden_states=outputs.hidden_states, attentions=outputs.attentions)


# ------------------------------------------------------------------------------------------------
# causal flash attention
# ------------------------------------------------------------------------------------------------
def _attn_tensor(t: torch.Tensor) -> _hip.AttnTensor:
    sb, sh, ss, sd = t.stride()
    if sd != 1:
        raise RuntimeError("flash attention: head_dim must be the innermost dimension")
    return _hip.AttnTensor(t.data_ptr(), sb, sh, ss)


def _attn_ref(t: torch.Tensor):
    """The tensor's descriptor as the C entry points take it (``const smt_attn_tensor*``)."""
    return ctypes.byref(_attn_tensor(t))


def _attn_ready(t: torch.Tensor) -> torch.Tensor:
    if t.stride(-1) == 1 and not any(s % 8 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


class KeyMask:
    """The key mask of a padded batch as the smt_flash kernels take it (include/smt_attention.h,
    ``smt_attn_*_kmask``): ``bits`` int64 [B, ceil(S/64)] on the device, bit j%64 of word j/64 set =
    key j takes part. Built by :func:`smt_flash_mask` from transformers' 2-D ``attention_mask``
    (the reference's collator passes ``input_ids != pad_token_id``, helper.py:194-204)."""

    __slots__ = ("bits", "S")

    def __init__(self, bits: torch.Tensor, S: int):
        self.bits, self.S = bits, int(S)

    @classmethod
    def from_padding_mask(cls, mask2d: torch.Tensor) -> "KeyMask":
        B, S = mask2d.shape
        W = -(-S // 64)
        m = torch.zeros(B, W * 64, dtype=torch.int64, device=mask2d.device)
        m[:, :S] = mask2d.to(torch.bool).to(torch.int64)
        shifts = torch.arange(64, dtype=torch.int64, device=mask2d.device)
        # distinct powers of two: the int64 sum is the bitwise OR (bit 63 wraps to the sign bit)
        bits = (m.view(B, W, 64) << shifts).sum(-1)
        return cls(bits.contiguous(), S)


class DocMask:
    """The document mask of packed rows as the smt_flash kernels take it (include/smt_attention.h,
    ``smt_attn_*_docs``): several samples concatenated into one row, block-diagonal causal attention.
    ``start`` / ``end``: int32 [B, S]; ``start[b, i]`` is the index of the first token of token i's
    document, ``end[b, i]`` one past its last token; query q sees key j iff ``start[q] <= j <= q``.
    The constructors use tensor ops only (no host synchronisation) and work on any device. Padding in
    a packed row is a trailing document of its own, with labels of -100."""

    __slots__ = ("start", "end", "S")

    def __init__(self, start: torch.Tensor, end: torch.Tensor, S: int):
        self.start, self.end, self.S = start, end, int(S)

    @classmethod
    def _from_first(cls, first: torch.Tensor) -> "DocMask":
        """``first`` bool [B, S]: token i opens a document (column 0 always does)."""
        B, S = first.shape
        first = first.clone()
        first[:, 0] = True
        idx = torch.arange(S, dtype=torch.int32, device=first.device).expand(B, S)
        start = torch.where(first, idx, torch.zeros_like(idx)).cummax(-1).values
        last = torch.cat([first[:, 1:], first.new_ones(B, 1)], dim=1)            # token i closes a document
        end = torch.where(last, idx + 1, torch.full_like(idx, S)).flip(-1).cummin(-1).values.flip(-1)
        return cls(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous(), S)

    @classmethod
    def from_position_ids(cls, position_ids: torch.Tensor) -> "DocMask":
        """A new document starts wherever the position does not follow the previous one by 1
        (transformers' ``find_packed_sequence_indices``). ``position_ids``: [B, S]."""
        pos = position_ids
        if pos.dim() != 2:
            raise ValueError(f"DocMask.from_position_ids: [B, S] position ids expected, got {tuple(pos.shape)}")
        first = torch.cat([pos.new_ones(pos.shape[0], 1, dtype=torch.bool), pos[:, 1:] - pos[:, :-1] != 1], dim=1)
        return cls._from_first(first)

    @classmethod
    def from_sequence_ids(cls, ids: torch.Tensor) -> "DocMask":
        """A new document starts wherever the id differs from the previous token's. ``ids``: [B, S]."""
        if ids.dim() != 2:
            raise ValueError(f"DocMask.from_sequence_ids: [B, S] ids expected, got {tuple(ids.shape)}")
        first = torch.cat([ids.new_ones(ids.shape[0], 1, dtype=torch.bool), ids[:, 1:] != ids[:, :-1]], dim=1)
        return cls._from_first(first)

    @classmethod
    def from_cu_seqlens(cls, cu_seqlens, B: int, S: int, device=None) -> "DocMask":
        """Cumulative document lengths ``[0, l0, l0 + l1, ..., S]`` (the flash-attention varlen
        convention): one 1-D tensor or list for ``B == 1``, or a list of B of them. Tokens past the
        last entry belong to the last document."""
        rows = cu_seqlens
        if isinstance(rows, torch.Tensor):
            rows = [rows] if rows.dim() == 1 else list(rows)
        elif len(rows) == 0 or not isinstance(rows[0], (list, tuple, torch.Tensor)):
            rows = [rows]
        if len(rows) != B:
            raise ValueError(f"DocMask.from_cu_seqlens: {len(rows)} rows of cu_seqlens for a batch of {B}")
        if device is None:
            device = next((r.device for r in rows if isinstance(r, torch.Tensor)), torch.device("cpu"))
        first = torch.zeros(B, S + 1, dtype=torch.bool, device=device)             # column S takes the closing S
        for b, r in enumerate(rows):
            r = torch.as_tensor(r, dtype=torch.int64, device=device).clamp(0, S)
            first[b].index_fill_(0, r, True)
        return cls._from_first(first[:, :S])


_DOC_AND_KEY_MASK = ("flash attention: a document mask and a key mask together are not supported; padding in a "
                     "packed row is expressed as a trailing document of its own, whose labels are -100")


def dropout_threshold(p: float) -> int:
    """The 8-bit threshold ``t`` of the attention-dropout keep function (include/smt_attention.h):
    ``clamp(floor(p * 256 + 0.5), 0, 255)``; ``p`` outside [0, 1) raises."""
    t = _hip.load().smt_attn_dropout_threshold(float(p))
    if t < 0:
        raise ValueError(f"flash attention: dropout p = {p} is outside [0, 1)")
    return t


def dropout_effective_p(p: float) -> float:
    """The drop rate the kernels apply for ``dropout_p=p``: ``t / 256``. Kept probabilities are scaled
    by ``1 / (1 - dropout_effective_p(p))``."""
    return dropout_threshold(p) / 256.0


def _seed_tensor(seed, device) -> torch.Tensor:
    """The 64-bit dropout seed as a 1-element int64 device tensor (an int is taken modulo 2^64)."""
    if seed is None:
        raise ValueError("flash attention: a dropout seed is needed (an int or a 1-element int64 device tensor)")
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != device:
            raise ValueError("flash attention: seed must be an int or a 1-element int64 tensor on q's device")
        return seed.reshape(1)
    s = int(seed) & (2 ** 64 - 1)
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s], dtype=torch.int64, device=device)


def flash_dropout_mask(B: int, Hq: int, S: int, p: float, seed, device) -> torch.Tensor:
    """The keep mask the smt_flash kernels apply for (``p``, ``seed``): bool ``[B, Hq, S, S]``, element
    (b, h, q, key) True = that probability is kept. Written by ``smt_attn_dropout_mask`` from the
    kernels' own keep function (a test oracle's input and a debugging aid)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("flash_dropout_mask: a ROCm device is needed (the mask is written by a HIP kernel)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = dropout_threshold(p)
    seed_t = _seed_tensor(seed, device) if t else None
    keep = torch.empty(B, Hq, S, S, dtype=torch.uint8, device=device)
    shape = _hip.AttnShape(B, Hq, Hq, S, 1.0, _hip.DTYPE_BF16)
    with torch.cuda.device(device):
        rc = _hip.load().smt_attn_dropout_mask(keep.data_ptr(), float(p), _hip._ptr(seed_t),
                                               ctypes.byref(shape), _stream(keep))
    _hip._check(rc, "smt_attn_dropout_mask")
    return keep.bool()


def _key_mask_args(key_mask, B: int, S: int, device, prefix: str, noun: str):
    """(pointer, row stride) of an optional :class:`KeyMask` over the S keys of B rows, as the C entry
    points take them; ``prefix`` and ``noun`` word the caller's message."""
    if key_mask is None:
        return None, 0
    if key_mask.S != S or key_mask.bits.shape[0] != B or key_mask.bits.device != device:
        raise ValueError(f"{prefix}: key mask for [{key_mask.bits.shape[0]}, {key_mask.S}] keys, "
                         f"{noun} has [{B}, {S}]")
    return key_mask.bits.data_ptr(), key_mask.bits.shape[1]


class FlashAttnFn(torch.autograd.Function):
    """Causal GQA attention: q [B, Hq, S, 128], k / v [B, Hkv, S, 128] (any strides with head_dim
    innermost) -> o [B, S, Hq, 128] (the layout transformers' attention functions return).
    ``key_mask``: optional :class:`KeyMask` (padded batches); ``doc_mask``: optional :class:`DocMask`
    (packed rows; not together with a key mask). ``dropout_p``: attention dropout inside
    the kernels (the keep function of include/smt_attention.h; effective rate
    :func:`dropout_effective_p`); ``seed``: an int or a 1-element int64 device tensor, drawn from the
    device generator when None (no host sync; ``torch.utils.checkpoint`` replays it). ``any_length``:
    take any S >= 1 (default: S % 4 == 0 only, as before the ``smt_attn_*_ld`` entry points). Either
    way lse and delta are ``[B, Hq, lse_ld]`` with ``lse_ld = (S + 3) & ~3``, the 16-byte rows the
    dK / dV kernel fetches; q, k, v, o and do are never padded or copied for the length."""

    @staticmethod
    def forward(ctx, q, k, v, scale, key_mask=None, joint=False, dropout_p=0.0, seed=None, doc_mask=None,
                any_length=False):
        if doc_mask is not None and key_mask is not None:
            raise NotImplementedError(_DOC_AND_KEY_MASK)
        for t, n in ((q, "q"), (k, "k"), (v, "v")):
            _need(t, "flash attention " + n, like=q)
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        if D != 128 or k.shape != (B, Hkv, S, D) or v.shape != k.shape or Hq % Hkv or S < 1 or (S % 4 and not any_length):
            raise NotImplementedError(f"flash attention: head_dim 128, Hq % Hkv == 0, S % 4 == 0 "
                                      f"(any S >= 1 with any_length=True) (q {tuple(q.shape)}, k {tuple(k.shape)})")
        q, k, v = _attn_ready(q), _attn_ready(k), _attn_ready(v)
        for t in (q, k, v):
            if S * t.stride(2) * 2 >= 2 ** 31:
                raise NotImplementedError("flash attention: per-head extent must stay below 2 GiB")
        o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(B, Hq, (S + 3) & ~3, dtype=torch.float32, device=q.device)
        shape = _hip.AttnShape(B, Hq, Hkv, S, float(scale), _dt(q))
        km, km_ld = _key_mask_args(key_mask, B, S, q.device, "flash attention", "batch")
        ds = de = None
        if doc_mask is not None:
            ds, de = doc_mask.start, doc_mask.end
            for t in (ds, de):
                if t.shape != (B, S) or t.dtype != torch.int32 or t.device != q.device or not t.is_contiguous():
                    raise ValueError(f"flash attention: document mask arrays must be contiguous int32 [{B}, {S}] on "
                                     f"q's device (got {t.dtype} {tuple(t.shape)} on {t.device})")
        dropout_p = float(dropout_p)
        seed_t = None
        if dropout_p != 0.0 and dropout_threshold(dropout_p):
            seed_t = (torch.empty(1, dtype=torch.int64, device=q.device).random_() if seed is None
                      else _seed_tensor(seed, q.device))
        T, P = _attn_ref, _hip._ptr
        rc = _hip.load().smt_attn_fwd_ld(T(q), T(k), T(v), T(o.transpose(1, 2)), lse.data_ptr(), lse.shape[2], km, km_ld,
                                         P(ds), P(de), dropout_p if seed_t is not None else 0.0, P(seed_t),
                                         ctypes.byref(shape), _stream(q))
        _hip._check(rc, "smt_attn_fwd_ld")
        ctx.save_for_backward(q, k, v, o, lse, key_mask.bits if key_mask is not None else None, seed_t, ds, de)
        ctx.dropout_p = dropout_p
        ctx.scale = float(scale)
        ctx.joint = bool(joint)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, km, seed_t, ds, de = ctx.saved_tensors
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        do = _attn_ready(do)
        if ctx.joint:
            # one [B, S, (Hq + 2 Hkv) D] buffer holding [dq | dk | dv] row by row: q/k/v_proj's data
            # gradients then run as one GEMM (dgrad.py, the engine's joint transposed copy)
            J = torch.empty(B, S, (Hq + 2 * Hkv) * D, dtype=q.dtype, device=q.device)
            dq = J[:, :, :Hq * D].view(B, S, Hq, D).transpose(1, 2)
            dk = J[:, :, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D).transpose(1, 2)
            dv = J[:, :, (Hq + Hkv) * D:].view(B, S, Hkv, D).transpose(1, 2)
            dq._smt_joint = dk._smt_joint = True
        else:
            dq = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device)
            dk = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype, device=k.device)
            dv = torch.empty_strided(v.shape, v.stride(), dtype=v.dtype, device=v.device)
        delta = torch.empty_like(lse)
        if do.dtype != q.dtype:
            do = do.to(q.dtype)
        shape = _hip.AttnShape(B, Hq, Hkv, S, ctx.scale, _dt(q))
        T, P = _attn_ref, _hip._ptr
        rc = _hip.load().smt_attn_bwd_ld(T(q), T(k), T(v), T(o.transpose(1, 2)), T(do.transpose(1, 2)), lse.data_ptr(),
                                         delta.data_ptr(), lse.shape[2], T(dq), T(dk), T(dv), P(km),
                                         km.shape[1] if km is not None else 0, P(ds), P(de),
                                         ctx.dropout_p if seed_t is not None else 0.0, P(seed_t),
                                         ctypes.byref(shape), _stream(q))
        _hip._check(rc, "smt_attn_bwd_ld")
        return dq, dk, dv, None, None, None, None, None, None, None


def flash_attention(q, k, v, scale=None, key_mask: "KeyMask" = None, joint: bool = False, dropout_p: float = 0.0,
                    seed=None, doc_mask: "DocMask" = None, any_length: bool = False):
    """Causal attention ``[B, Hq, S, 128]`` x ``[B, Hkv, S, 128]`` -> ``[B, S, Hq, 128]``; with
    ``key_mask`` the keys it clears take no part (padded batches). ``joint``: the gradients of q, k
    and v go out as slices of one ``[B, S, (Hq + 2 Hkv) * 128]`` buffer (same values). ``dropout_p``:
    attention dropout applied inside the kernels, forward and backward (effective rate
    :func:`dropout_effective_p`, mask :func:`flash_dropout_mask`); ``seed``: an int or a 1-element
    int64 device tensor, drawn from the device generator when None. ``doc_mask``: a :class:`DocMask`
    for packed rows (block-diagonal causal attention; the kernels skip the K/V tiles no row of a
    workgroup sees); not together with ``key_mask``. ``any_length``: take any ``S >= 1``, forward and
    backward, natively (no padded copies); the default refuses ``S % 4 != 0`` as it always did. At
    ``S % 4 == 0`` both give the same bits."""
    if doc_mask is not None and key_mask is not None:
        raise NotImplementedError(_DOC_AND_KEY_MASK)
    return FlashAttnFn.apply(q, k, v, scale if scale is not None else q.shape[-1] ** -0.5, key_mask, joint,
                             dropout_p, seed, doc_mask, any_length)


class CacheMask:
    """What :func:`smt_flash_mask` returns for a call against a KV cache: ``key_mask`` (a
    :class:`KeyMask` over the ``kv_length`` cached keys, or None), the absolute position ``q_offset``
    of the call's first query and ``kv_length``. ``q_offset`` is an int, or, for a decode step on a
    static cache, an integer tensor that stays on its device (``flash_attention_cached`` hands it to
    the kernel). ``prefill``: None, or, for the first forward on a static cache (offset 0, fewer
    queries than key slots), the mask of the same-length call over the first ``q_length`` keys as a
    one-element tuple (a :class:`KeyMask` or None), which the training forward kernel then runs."""

    __slots__ = ("key_mask", "q_offset", "kv_length", "prefill")

    def __init__(self, key_mask, q_offset, kv_length: int, prefill=None):
        self.key_mask, self.kv_length, self.prefill = key_mask, int(kv_length), prefill
        self.q_offset = q_offset if isinstance(q_offset, torch.Tensor) else int(q_offset)


def _device_positions(t: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """A tensor-valued ``q_offset`` as the kernel reads it: int64, one element or one per batch row,
    on q's device. int64 is used in place; int32 (or a strided ``[B]``) costs one device op. Nothing
    here reads a value."""
    if t.device != q.device:
        raise ValueError(f"cached flash attention: q_offset tensor on {t.device}, q on {q.device}")
    if t.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"cached flash attention: q_offset tensor of dtype {t.dtype} (int64 or int32)")
    if t.dim() > 1 or t.numel() not in (1, q.shape[0]):
        raise ValueError(f"cached flash attention: q_offset tensor of shape {tuple(t.shape)} (0-d, [1] or "
                         f"[{q.shape[0]}])")
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t if t.numel() == 1 or t.stride(0) == 1 else t.contiguous()


def flash_attention_cached(q, k, v, scale=None, key_mask: "KeyMask" = None, q_offset=None,
                           num_splits: int = None, return_lse: bool = False):
    """Attention of ``Sq`` new positions against a KV cache, forward only (``smt_attn_fwd_cached``, the
    split-KV decode kernel): q ``[B, Hq, Sq, 128]``, k / v ``[B, Hkv, Skv, 128]`` (any strides with
    head_dim innermost: a slice of a pre-allocated buffer, a ``[B, S, H, D]``-ordered cache) ->
    ``[B, Sq, Hq, 128]``. Query i sits at position ``q_offset + i`` (default ``Skv - Sq``: the queries
    are the last positions) and sees key j iff ``j <= q_offset + i`` and ``key_mask`` (over the Skv
    keys) keeps j; K / V rows at ``q_offset + Sq`` and later are never read. Any ``Skv``.
    ``q_offset`` may be an integer tensor on q's device, 0-d, ``[1]`` or ``[B]`` (one position per
    batch row): the kernel reads it (``smt_attn_fwd_cached_pos``), the host never does, so the call
    can be captured in a graph and replayed while the tensor changes; ``Skv`` is then the capacity of
    the buffers, the split count and the workspace follow the capacity, and a value outside
    ``[0, Skv - Sq]`` is saturated into it by the kernel. For a given ``num_splits`` the result equals
    the integer call's bit for bit.
    ``num_splits``: how many workgroups share one (batch, kv head)'s key range (None: the library's
    default for the shape); the result is bit-reproducible for a given value. ``return_lse``: also
    return the fp32 ``[B, Hq, Sq]`` log-sum-exp (log2 units, include/smt_attention.h). The workspace
    comes from torch's allocator; nothing synchronises with the host. There is no backward: an input
    that requires grad while gradients are enabled raises."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise NotImplementedError("flash_attention_cached: cached attention has no backward (inference only); run "
                                  "under torch.no_grad() or detach the inputs")
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(t, "cached flash attention " + n, like=q)
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape:
        raise NotImplementedError(f"cached flash attention: 4-D q, k, v (q {tuple(q.shape)}, k {tuple(k.shape)}, "
                                  f"v {tuple(v.shape)})")
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    if D != 128 or k.shape != (B, Hkv, Skv, D) or Hq % Hkv or Sq < 1:
        raise NotImplementedError(f"cached flash attention: head_dim 128, Hq % Hkv == 0, Sq >= 1 "
                                  f"(q {tuple(q.shape)}, k {tuple(k.shape)})")
    pos = None
    if isinstance(q_offset, torch.Tensor):
        pos, q_offset = _device_positions(q_offset, q), None
        if Sq > Skv:
            raise ValueError(f"cached flash attention: {Sq} query positions against {Skv} key slots")
    else:
        q_offset = Skv - Sq if q_offset is None else int(q_offset)
        if q_offset < 0 or q_offset + Sq > Skv:
            raise ValueError(f"cached flash attention: queries at positions [{q_offset}, {q_offset + Sq}) of {Skv} key slots")
    num_splits = 0 if num_splits is None else int(num_splits)
    if num_splits < 0:
        raise ValueError(f"cached flash attention: num_splits = {num_splits}")
    q, k, v = _attn_ready(q), _attn_ready(k), _attn_ready(v)
    for t in (k, v):
        if Skv * t.stride(2) * 2 >= 2 ** 31:
            raise NotImplementedError("cached flash attention: per-head extent must stay below 2 GiB")
    km, km_ld = _key_mask_args(key_mask, B, Skv, q.device, "cached flash attention", "cache")
    o = torch.empty(B, Sq, Hq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, Hq, Sq, dtype=torch.float32, device=q.device) if return_lse else None
    shape = _hip.AttnShape(B, Hq, Hkv, Skv, float(scale if scale is not None else D ** -0.5), _dt(q))
    lib = _hip.load()
    if num_splits == 0:
        num_splits = lib.smt_attn_cached_splits(ctypes.byref(shape), Sq)
        _hip._check(min(num_splits, 0), "smt_attn_cached_splits")
    ws_bytes = lib.smt_attn_cached_workspace(ctypes.byref(shape), Sq, num_splits)
    _hip._check(min(ws_bytes, 0), "smt_attn_cached_workspace")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes else None
    tensors = (_attn_ref(q), _attn_ref(k), _attn_ref(v), _attn_ref(o.transpose(1, 2)), _hip._ptr(lse), km, km_ld)
    tail = (num_splits, _hip._ptr(ws), ctypes.byref(shape), _stream(q))
    with torch.cuda.device(q.device):
        if pos is not None:
            rc = lib.smt_attn_fwd_cached_pos(*tensors, Sq, pos.data_ptr(), 0 if pos.numel() == 1 else 1, *tail)
        else:
            rc = lib.smt_attn_fwd_cached(*tensors, Sq, q_offset, *tail)
    _hip._check(rc, "smt_attn_fwd_cached_pos" if pos is not None else "smt_attn_fwd_cached")
    return (o, lse) if return_lse else o


def flash_attention_beams(q, k_prompt, v_prompt, k_gen, v_gen, ancestors, num_beams, prompt_len, gen_len,
                          prompt_key_mask: "KeyMask" = None, scale=None, num_splits: int = None,
                          return_lse: bool = False):
    """One decode position of beam search against a beam-shared cache, forward only
    (``smt_attn_fwd_beams``, include/smt_attention.h): N samples x ``num_beams`` beams, row
    ``r = n * num_beams + beam``. q ``[N * nb, Hq, 1, 128]``; k_prompt / v_prompt ``[N, Hkv, P_cap, 128]``
    (the prompt once per sample, ``prompt_len <= P_cap`` keys valid); k_gen / v_gen
    ``[N * nb, Hkv, T_cap, 128]`` (row = physical slot, position = generation step, ``gen_len <= T_cap``
    steps valid, the current token's included); ``ancestors`` uint8 ``[N * nb, >= gen_len]``:
    ``ancestors[r, j]`` is the slot (0..nb-1) of r's sample that holds the step-j key of row r's
    hypothesis -> ``[N * nb, 1, Hq, 128]``. Row r sees prompt key j iff ``prompt_key_mask`` (a
    :class:`KeyMask` whose ``bits`` are ``[N, >= ceil(prompt_len / 64)]``, rows of any stride; None:
    every key) keeps it, and generated entry (slot s, step j) iff ``ancestors[r, j] == s``; generated
    entries have no mask of their own. Any strides with head_dim innermost. K / V rows past
    ``prompt_len`` / ``gen_len`` are never read, and no address depends on a value in ``ancestors`` (a
    value >= nb matches nothing; a row that sees no key at all gets zeros and lse = +inf).
    ``num_splits``, ``return_lse`` (fp32 ``[N * nb, Hq]``, log2 units): as in
    :func:`flash_attention_cached`. ``prompt_len`` is a host integer; nothing synchronises with the
    host. ``gen_len`` is a host integer, or a one-element int32 tensor on q's device: the kernel reads
    it (``smt_attn_fwd_beams_pos``), the host never does, so the call can be captured in a graph and
    replayed while the counter, the buffers and ``ancestors`` change in place. The kernel saturates
    the counter into ``[1, T_cap]``; ``ancestors`` is then ``[N * nb, >= T_cap]``, and the split count
    and the workspace follow the capacity. For a given ``num_splits`` the result equals the integer
    call's with ``gen_len = clamp(counter, 1, T_cap)`` bit for bit. There is no backward: an input that
    requires grad while gradients are enabled raises."""
    tensors = (q, k_prompt, v_prompt, k_gen, v_gen)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("flash_attention_beams: beam-shared attention has no backward (inference only); run "
                                  "under torch.no_grad() or detach the inputs")
    for t, n in zip(tensors, ("q", "k_prompt", "v_prompt", "k_gen", "v_gen")):
        _need(t, "beam-shared flash attention " + n, like=q)
    steps = None
    if isinstance(gen_len, torch.Tensor):
        steps = gen_len
        if steps.device != q.device or steps.dtype != torch.int32 or steps.numel() != 1:
            raise ValueError(f"beam-shared flash attention: a tensor gen_len is one int32 element on {q.device} (got "
                             f"{steps.dtype} {tuple(steps.shape)} on {steps.device})")
        gen_len = k_gen.shape[2] if k_gen.dim() == 4 else 0     # the host's arithmetic runs on the capacity
    nb, P, T = int(num_beams), int(prompt_len), int(gen_len)
    if any(t.dim() != 4 for t in tensors) or v_prompt.shape != k_prompt.shape or v_gen.shape != k_gen.shape:
        raise NotImplementedError("beam-shared flash attention: 4-D q, k_prompt / v_prompt and k_gen / v_gen of equal "
                                  f"shapes (q {tuple(q.shape)}, k_prompt {tuple(k_prompt.shape)}, v_prompt "
                                  f"{tuple(v_prompt.shape)}, k_gen {tuple(k_gen.shape)}, v_gen {tuple(v_gen.shape)})")
    R, Hq, Sq, D = q.shape
    Hkv, T_cap = k_gen.shape[1], k_gen.shape[2]
    if nb < 1 or R % nb:
        raise ValueError(f"beam-shared flash attention: {R} rows are no multiple of num_beams = {nb}")
    N, P_cap = R // nb, k_prompt.shape[2]
    if D != 128 or Sq != 1 or Hq % Hkv or k_gen.shape != (R, Hkv, T_cap, D) or k_prompt.shape != (N, Hkv, P_cap, D):
        raise NotImplementedError(f"beam-shared flash attention: head_dim 128, one query position, Hq % Hkv == 0, "
                                  f"k_prompt [N, Hkv, P_cap, 128], k_gen [N * nb, Hkv, T_cap, 128] (q {tuple(q.shape)}, "
                                  f"k_prompt {tuple(k_prompt.shape)}, k_gen {tuple(k_gen.shape)}, nb {nb})")
    if not 0 <= P <= P_cap or not 1 <= T <= T_cap:
        raise ValueError(f"beam-shared flash attention: prompt_len {P} of {P_cap}, gen_len {T} of {T_cap} "
                         "(gen_len counts the current token's key, so it is at least 1)")
    anc = ancestors
    if (not isinstance(anc, torch.Tensor) or anc.dtype != torch.uint8 or anc.device != q.device or anc.dim() != 2
            or anc.shape[0] != R or anc.shape[1] < T):
        raise ValueError(f"beam-shared flash attention: ancestors must be uint8 [{R}, >= {T}] on {q.device}")
    if anc.stride(1) != 1:
        anc = anc.contiguous()
    num_splits = 0 if num_splits is None else int(num_splits)
    if num_splits < 0:
        raise ValueError(f"beam-shared flash attention: num_splits = {num_splits}")
    q, k_gen, v_gen = _attn_ready(q), _attn_ready(k_gen), _attn_ready(v_gen)
    if P:
        k_prompt, v_prompt = _attn_ready(k_prompt), _attn_ready(v_prompt)
    pm, pm_ld = None, 0
    if prompt_key_mask is not None and P:
        bits = prompt_key_mask.bits
        if (bits.dim() != 2 or bits.dtype != torch.int64 or bits.device != q.device or bits.shape[0] != N
                or bits.shape[1] < -(-P // 64) or prompt_key_mask.S < P):
            raise ValueError(f"beam-shared flash attention: prompt key mask for [{bits.shape[0]}, {prompt_key_mask.S}] "
                             f"keys, the prompt segment has [{N}, {P}]")
        if bits.stride(1) != 1:
            bits = bits.contiguous()
        pm, pm_ld = bits.data_ptr(), bits.stride(0) if N > 1 else bits.shape[1]
    o = torch.empty(R, 1, Hq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(R, Hq, dtype=torch.float32, device=q.device) if return_lse else None
    shape = _hip.AttnShape(N, Hq, Hkv, P + T, float(scale if scale is not None else D ** -0.5), _dt(q))
    lib = _hip.load()
    if num_splits == 0:
        num_splits = lib.smt_attn_beams_splits(ctypes.byref(shape), nb, P, T)
        _hip._check(min(num_splits, 0), "smt_attn_beams_splits")
    ws_bytes = lib.smt_attn_beams_workspace(ctypes.byref(shape), nb, P, T, num_splits)
    _hip._check(min(ws_bytes, 0), "smt_attn_beams_workspace")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes else None
    fn = "smt_attn_fwd_beams" if steps is None else "smt_attn_fwd_beams_pos"
    with torch.cuda.device(q.device):
        rc = getattr(lib, fn)(_attn_ref(q), _attn_ref(k_prompt), _attn_ref(v_prompt), _attn_ref(k_gen),
                              _attn_ref(v_gen), _attn_ref(o.transpose(1, 2)), _hip._ptr(lse), pm, pm_ld,
                              anc.data_ptr(), anc.stride(0) if R > 1 else anc.shape[1], nb, P, P_cap,
                              T if steps is None else steps.data_ptr(), T_cap,
                              num_splits, _hip._ptr(ws), ctypes.byref(shape), _stream(q))
    _hip._check(rc, fn)
    return (o, lse) if return_lse else o


def kv_append(k_new, v_new, k_gen, v_gen, steps) -> None:
    """One decode step's K / V into the generated buffers of a beam-shared cache
    (``smt_attn_kv_append_pos``): k_new / v_new ``[R, Hkv, 1, 128]`` (any strides with head_dim
    innermost: the model hands over a transposed view) go into row ``clamp(steps, 1, T_cap) - 1`` of
    k_gen / v_gen ``[R, Hkv, T_cap, 128]``, in one launch. ``steps``: the one-element int32 counter on
    the buffers' device that :func:`flash_attention_beams` takes as ``gen_len``; the kernel reads it,
    the host never does, and no value of it can send the write outside the buffers."""
    for t, n in ((k_new, "k_new"), (v_new, "v_new"), (k_gen, "k_gen"), (v_gen, "v_gen")):
        _need(t, "kv_append " + n, like=k_gen)
    if k_gen.dim() != 4 or v_gen.shape != k_gen.shape or k_gen.shape[3] != 128:
        raise NotImplementedError(f"kv_append: k_gen / v_gen [R, Hkv, T_cap, 128] (got {tuple(k_gen.shape)}, "
                                  f"{tuple(v_gen.shape)})")
    R, Hkv, T_cap, D = k_gen.shape
    if k_new.shape != (R, Hkv, 1, D) or v_new.shape != (R, Hkv, 1, D):
        raise ValueError(f"kv_append: k_new / v_new must be [{R}, {Hkv}, 1, {D}] (got {tuple(k_new.shape)}, "
                         f"{tuple(v_new.shape)})")
    if (not isinstance(steps, torch.Tensor) or steps.device != k_gen.device or steps.dtype != torch.int32
            or steps.numel() != 1):
        raise ValueError(f"kv_append: steps is one int32 element on {k_gen.device}")
    if not (k_gen.stride(3) == 1 and v_gen.stride(3) == 1 and _attn_ready(k_gen) is k_gen and _attn_ready(v_gen) is v_gen):
        raise ValueError("kv_append: k_gen / v_gen need head_dim innermost and 16-byte aligned rows (they are written in place)")
    new = []
    for t in (k_new, v_new):
        # the stride of a one-element dimension carries no meaning: drop it before the alignment test
        t = t.as_strided(t.shape, (t.stride(0), t.stride(1), 0, t.stride(3)))
        new.append(_attn_ready(t))
    with torch.cuda.device(k_gen.device):
        rc = _hip.load().smt_attn_kv_append_pos(_attn_ref(new[0]), _attn_ref(new[1]), _attn_ref(k_gen), _attn_ref(v_gen),
                                                steps.data_ptr(), R, Hkv, T_cap, _dt(k_gen), _stream(k_gen))
    _hip._check(rc, "smt_attn_kv_append_pos")


def _beam_decode(layer, query, attention_mask, scaling):
    """A decode step on a :class:`~sparse_matrix_tuning_amd.beam_cache.BeamSharedCache`: ``layer`` is the
    cache layer that tagged the K / V its ``update`` returned. The prompt's key mask is the
    :class:`CacheMask`'s, rows ``[::nb]`` and the words of the first ``prompt_len`` keys (a view: the
    beams of a sample share their padding); the columns of generated positions are not consulted.
    A ``device_steps`` cache builds those words once, at its first decode step, and keeps them in its
    state (a copy: the mask ``generate()`` grows is then no input of a later step), and hands the
    kernel its device counter in place of ``layer.steps`` (``smt_attn_fwd_beams_pos``)."""
    if attention_mask is not None and not isinstance(attention_mask, CacheMask):
        raise NotImplementedError("smt_flash attention: a decode step on a BeamSharedCache takes the CacheMask "
                                  f"smt_flash_mask builds (got {type(attention_mask).__name__})")
    st = layer.state
    nb, P = st.num_beams, layer.prompt_len
    if st.device_steps:
        if st.prompt_mask is None:
            km = attention_mask.key_mask if attention_mask is not None else None
            st.prompt_mask = (KeyMask(km.bits[::nb, :-(-P // 64)].clone(), P) if km is not None and P else None,)
        return flash_attention_beams(query, layer.k_prompt, layer.v_prompt, layer.k_gen, layer.v_gen, st.anc, nb, P,
                                     st.counter, prompt_key_mask=st.prompt_mask[0], scale=scaling)
    km = attention_mask.key_mask if attention_mask is not None else None
    pm = KeyMask(km.bits[::nb, :-(-P // 64)], P) if km is not None else None
    return flash_attention_beams(query, layer.k_prompt, layer.v_prompt, layer.k_gen, layer.v_gen, layer.state.anc, nb, P,
                                 layer.steps, prompt_key_mask=pm, scale=scaling)


def smt_flash_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None,
                                is_causal=None, **kwargs):
    """transformers attention-function signature (``AttentionInterface``). Causal self-attention,
    unpadded (``attention_mask`` None), padded (a :class:`KeyMask` from :func:`smt_flash_mask`) or
    packed (a :class:`DocMask` from :func:`smt_flash_mask` or built by the caller);
    ``dropout`` (transformers passes the config's ``attention_dropout`` in training mode, 0.0 in eval)
    runs inside the kernels; anything else raises rather than silently changing semantics.

    A call against a KV cache (a :class:`CacheMask` from :func:`smt_flash_mask`, or fewer queries than
    keys) runs :func:`flash_attention_cached`, forward only: dropout or a :class:`DocMask` with a
    cache raises. A tensor ``q_offset`` in the :class:`CacheMask` (a decode step on a static cache) is
    passed through to the kernel; the first forward on a static cache (``CacheMask.prefill``) runs the
    training forward kernel on the first ``Sq`` rows of the buffer. A decode step on a
    :class:`~sparse_matrix_tuning_amd.beam_cache.BeamSharedCache` (its ``update`` tags the K / V it returns
    with the cache layer) runs :func:`flash_attention_beams` on that layer's buffers; without that cache
    nothing changes.
    Every same-length call goes to :func:`flash_attention` with ``any_length=True``: the
    reference's collator pads a batch to its longest sample (helper.py:191-205), so S is any integer in
    training, in the evaluation loss and in the prefill of ``generate()``. A gradient-free call takes
    that route too: at B 16, Hq 32, Hkv 8 the training forward measured 3.3-3.7x (S 2047) and 2.1x
    (S 301) faster than the cached kernel, which re-reads K / V once per 32 / G query positions
    ("Any sequence length"; profiles/r10_anylen_forward_routes.jsonl)."""
    if attention_mask is not None and not isinstance(attention_mask, (KeyMask, DocMask, CacheMask)):
        raise NotImplementedError("smt_flash attention: only key-padding and document masks built by smt_flash_mask "
                                  f"are supported (got {type(attention_mask).__name__})")
    if is_causal is False or not getattr(module, "is_causal", True):
        raise NotImplementedError("smt_flash attention: causal attention only")
    Sq, Skv = query.shape[2], key.shape[2]
    cached = isinstance(attention_mask, CacheMask) or Sq != Skv
    dropout = float(dropout or 0.0)
    beam_layer = getattr(key, "_smt_beam", None)
    if beam_layer is not None:                     # a decode step on a BeamSharedCache (its update tags K / V)
        if dropout != 0.0:
            raise NotImplementedError("smt_flash attention: dropout with a KV cache (the beam kernel is inference only)")
        return _beam_decode(beam_layer, query, attention_mask, scaling), None
    if cached:
        if dropout != 0.0:
            raise NotImplementedError("smt_flash attention: dropout with a KV cache (the cached kernel is inference only)")
        if isinstance(attention_mask, DocMask):
            raise NotImplementedError("smt_flash attention: packed rows (a document mask) with a KV cache")
        km, q_offset = attention_mask, None
        if isinstance(attention_mask, CacheMask):
            if attention_mask.kv_length != Skv:
                raise ValueError(f"smt_flash attention: mask built for {attention_mask.kv_length} cached keys, the "
                                 f"cache holds {Skv}")
            km, q_offset = attention_mask.key_mask, attention_mask.q_offset
            if attention_mask.prefill is not None and Sq < Skv:
                # the prefill on a static cache: the first Sq slots hold this call's keys, the rest
                # are behind the causal edge; the training forward as for the DynamicCache prefill
                return flash_attention(query, key[:, :, :Sq], value[:, :, :Sq], scaling, attention_mask.prefill[0],
                                       any_length=True), None
        return flash_attention_cached(query, key, value, scaling, km, q_offset), None
    # the engine marks attention modules whose q/k/v_proj share a joint transposed copy
    docs = attention_mask if isinstance(attention_mask, DocMask) else None
    return flash_attention(query, key, value, scaling, None if docs is not None else attention_mask,
                           joint=getattr(module, "_smt_joint_qkv_grad", False), dropout_p=dropout,
                           doc_mask=docs, any_length=True), None


def _closure_vars(fn) -> dict:
    cells = getattr(fn, "__closure__", None) or ()
    names = getattr(getattr(fn, "__code__", None), "co_freevars", ())
    return dict(zip(names, (c.cell_contents for c in cells)))


def _packed_sequence_ids(mask_function):
    """The [B, S] id tensor when ``mask_function`` is exactly what transformers' ``create_causal_mask``
    builds for a packed batch, ``and_masks(causal_mask_function, packed_sequence_mask_function(ids))``,
    else None. Recognised by structure (the closures), never by calling it: a sliding-window function
    answers "token q sees q-1" as well, and a call could not tell a user's extra mask apart."""
    from transformers import masking_utils as mu
    if getattr(mask_function, "__code__", None) is not _inner_code(mu.and_masks, "and_mask"):
        return None
    parts = _closure_vars(mask_function).get("mask_functions")
    if not isinstance(parts, tuple) or len(parts) != 2 or parts[0] is not mu.causal_mask_function:
        return None
    if getattr(parts[1], "__code__", None) is not _inner_code(mu.packed_sequence_mask_function, "inner_mask"):
        return None
    ids = _closure_vars(parts[1]).get("packed_sequence_mask")
    return ids if isinstance(ids, torch.Tensor) and ids.dim() == 2 else None


def _inner_code(factory, name: str):
    """The code object of the function ``name`` that ``factory`` defines and returns."""
    return next((c for c in factory.__code__.co_consts if getattr(c, "co_name", None) == name), None)


def smt_flash_mask(batch_size, q_length, kv_length, q_offset=0, kv_offset=0, mask_function=None,
                   attention_mask=None, **kwargs):
    """transformers mask-interface builder for ``smt_flash`` (what ``create_causal_mask`` calls):
    ``None`` for a plain causal batch (no mask, or every key valid), a :class:`KeyMask` for a padded
    one: the causal mask AND the 2-D padding mask, exactly the mask ``sdpa_mask`` would materialise
    as [B, 1, S, S]; a :class:`DocMask` for a packed batch (restarting ``position_ids`` and no
    ``attention_mask``: transformers hands over causal AND ``packed_sequence_mask_function(ids)``).
    A call against a KV cache (``q_length != kv_length`` or ``q_offset != 0``: the decode steps of
    ``generate()`` with the default ``DynamicCache``) gets a :class:`CacheMask`: the offset, the cache
    length and the 2-D ``attention_mask`` (of a left-padded batch) as a :class:`KeyMask` over the
    ``kv_length`` keys, built without a host synchronisation (nothing asks whether every key is valid:
    this runs once per generated token).
    A static cache (``cache_implementation="static"``) hands over its fill level as a device tensor
    and a mask over the keys written so far, shorter than the buffer. At ``q_length == 1`` the
    :class:`CacheMask` carries a copy of that tensor and nothing reads it on the host; at
    ``q_length > 1`` (the prefill, once per ``generate()``) it is read once. The short mask is
    extended to the buffer with tensor ops; the slots beyond it are behind the causal edge.
    Anything the kernels do not implement (``kv_offset != 0`` or tensor-valued, sliding windows,
    custom mask functions, packed rows together with a cache) raises."""
    from transformers.masking_utils import causal_mask_function
    packed_ids = None
    if mask_function is not None and mask_function is not causal_mask_function:
        packed_ids = _packed_sequence_ids(mask_function)
        if packed_ids is None:
            raise NotImplementedError("smt_flash attention: custom mask functions are not supported (causal, or "
                                      "causal AND transformers' packed-sequence mask)")
    if isinstance(kv_offset, torch.Tensor):
        raise NotImplementedError("smt_flash attention: a tensor-valued kv_offset (a sliding or offset cache) is not "
                                  "supported")
    if kv_offset:
        raise NotImplementedError("smt_flash attention: kv_offset != 0 (a sliding or offset cache) is not supported")
    static = isinstance(q_offset, torch.Tensor)           # a static cache's fill level, on its device
    if static:
        if q_offset.numel() != 1 or q_offset.dtype not in (torch.int64, torch.int32):
            raise NotImplementedError(f"smt_flash attention: a tensor q_offset is one int64 / int32 element, got "
                                      f"{q_offset.dtype} {tuple(q_offset.shape)}")
        if q_length == 1:
            # A decode step: the kernel reads the position. A copy, because the cache advances its
            # counter in place before the attention of this forward runs.
            q_offset = q_offset.clone()
        else:
            q_offset = int(q_offset)                      # the prefill: one host read per forward
    if static or q_offset or q_length != kv_length:
        if packed_ids is not None:
            raise NotImplementedError("smt_flash attention: packed rows together with a KV cache are not supported")
        if not isinstance(q_offset, torch.Tensor) and (q_offset < 0 or q_offset + q_length > kv_length):
            raise NotImplementedError(f"smt_flash attention: queries [{q_offset}, {q_offset + q_length}) do not fit "
                                      f"{kv_length} cached keys")
        km, short = None, False
        if attention_mask is not None:
            am = attention_mask
            if am.dim() != 2 or am.shape[0] != batch_size:
                raise NotImplementedError(f"smt_flash attention: 2-D [B, S] padding mask expected, got {tuple(am.shape)}")
            short = am.shape[1] < kv_length
            if short:
                # A static cache: the mask covers the q_offset + q_length keys written so far, the
                # buffer more. The slots beyond it are behind the causal edge whatever their bits say.
                if isinstance(q_offset, int) and am.shape[1] < q_offset + q_length:
                    raise NotImplementedError(f"smt_flash attention: padding mask over {am.shape[1]} keys, queries up "
                                              f"to position {q_offset + q_length}")
                am = torch.nn.functional.pad(am, (0, kv_length - am.shape[1]))
            km = KeyMask.from_padding_mask(am[:, :kv_length])
        prefill = None
        if 1 < q_length < kv_length and (static or short) and q_offset == 0:
            # the first forward on a static cache: a same-length call on the first q_length slots
            pm = None
            if attention_mask is not None:
                pm = attention_mask[:, :q_length].to(torch.bool)
                pm = None if bool(pm.all()) else KeyMask.from_padding_mask(pm)
            prefill = (pm,)
        return CacheMask(km, q_offset, kv_length, prefill)
    if packed_ids is not None:
        if attention_mask is not None:
            raise NotImplementedError(_DOC_AND_KEY_MASK)
        if packed_ids.shape != (batch_size, kv_length):
            raise NotImplementedError(f"smt_flash attention: packed-sequence ids of shape {tuple(packed_ids.shape)} for "
                                      f"a [{batch_size}, {kv_length}] batch")
        return DocMask.from_sequence_ids(packed_ids)
    if attention_mask is None:
        return None
    am = attention_mask
    if am.dim() != 2 or am.shape[0] != batch_size or am.shape[1] < kv_length:
        raise NotImplementedError(f"smt_flash attention: 2-D [B, S] padding mask expected, got {tuple(am.shape)}")
    am = am[:, :kv_length].to(torch.bool)
    if bool(am.all()):
        return None
    return KeyMask.from_padding_mask(am)


ATTN_NAME = "smt_flash"


def register_attention() -> str:
    """Register ``smt_flash`` with transformers (attention function + its mask builder)."""
    from transformers import AttentionInterface
    from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS
    AttentionInterface.register(ATTN_NAME, smt_flash_attention_forward)
    ALL_MASK_ATTENTION_FUNCTIONS.register(ATTN_NAME, smt_flash_mask)
    return ATTN_NAME


# ------------------------------------------------------------------------------------------------
_EAGER = {}


class ModelFamily:
    """One architecture the fused path serves: its transformers modelling module (imported on first use), whose
    module-level ``apply_rotary_pos_emb`` the attention looks up at call time, and the classes the patch
    matches. ``rope_key``: where ``_EAGER`` keeps transformers' own function while the module global is patched."""

    def __init__(self, name, module, rmsnorm, mlp, decoder, attention, causal_lm, rope_key):
        self.name, self.module_name, self.rope_key = name, module, rope_key
        self._names = dict(rmsnorm=rmsnorm, mlp=mlp, decoder=decoder, attention=attention, causal_lm=causal_lm)

    @property
    def module(self):
        import importlib
        ml = importlib.import_module(self.module_name)
        if self.rope_key not in _EAGER:
            _EAGER[self.rope_key] = ml.apply_rotary_pos_emb
        return ml

    def __getattr__(self, kind):
        names = self.__dict__.get("_names", {})
        if kind not in names:
            raise AttributeError(kind)
        return getattr(self.module, names[kind])


FAMILIES = {
    "llama": ModelFamily("llama", "transformers.models.llama.modeling_llama", "LlamaRMSNorm", "LlamaMLP",
                         "LlamaDecoderLayer", "LlamaAttention", "LlamaForCausalLM", "rope"),
    "qwen2": ModelFamily("qwen2", "transformers.models.qwen2.modeling_qwen2", "Qwen2RMSNorm", "Qwen2MLP",
                         "Qwen2DecoderLayer", "Qwen2Attention", "Qwen2ForCausalLM", "rope_qwen2"),
}
_KINDS = ("rmsnorm", "mlp", "decoder", "attention", "causal_lm")


def model_family(model: nn.Module):
    """The :data:`FAMILIES` entry whose classes ``model`` is built from, or None. A family whose modelling module
    was never imported cannot have built the model and is not imported for the question."""
    for fam in FAMILIES.values():
        if _has_classes_of(model, fam):
            return fam
    return None


def _has_classes_of(model: nn.Module, fam) -> bool:
    import sys
    if fam.module_name not in sys.modules:
        return False
    classes = tuple(getattr(fam, k) for k in _KINDS)
    return any(isinstance(m, classes) for m in model.modules())


def _ml():
    return FAMILIES["llama"].module


def eager_apply_rotary_pos_emb(*a, **k):
    """transformers' own apply_rotary_pos_emb (for comparisons while the module global is patched)."""
    return _ml() and _EAGER["rope"](*a, **k)


class DecodeGraph:
    """The decode runner of one ``BeamSharedCache(graph=True)``, hence of one ``generate()`` call: the
    first decode step runs eagerly (the warm-up: allocator, code objects, the GEMM library's choices,
    and the cache's prompt mask words), the second is captured with ``torch.cuda.graph`` (one stream, a
    private pool; the forward is a linear chain), the later ones replay it. What changes from step to
    step reaches the graph through fixed buffers (``input_ids``, ``position_ids``, ``cache_position``
    where the caller passes one) and through device memory the kernels read themselves: the cache's
    counter, its buffers and its ancestry table. The growing 2-D ``attention_mask`` is no input. A
    capture that raises, raises: nothing falls back."""

    _DYNAMIC_ROPE = ("dynamic", "longrope")              # their tables follow the running length (a host read per step)

    def __init__(self, cache):
        # the cache owns its runner; a weak reference back, so that the pair is no reference cycle and a
        # dropped cache frees its graph and its private pool at once, not at some later collection
        self._cache = weakref.ref(cache)
        self.decodes = 0
        self.graph = self.static = self.logits = self.keys = None

    @property
    def cache(self):
        return self._cache()

    @staticmethod
    def _rope_types(model):
        found = []
        rot = getattr(getattr(model, "model", None), "rotary_emb", None)
        found.append(getattr(rot, "rope_type", None))
        for name in ("rope_parameters", "rope_scaling"):
            par = getattr(model.config, name, None)
            if isinstance(par, dict):
                found += [par.get("rope_type"), par.get("type")]
        return [t for t in found if isinstance(t, str)]

    def warm_up(self, model) -> None:
        """Before the first decode step, which the caller runs eagerly."""
        bad = [t for t in self._rope_types(model) if t in self._DYNAMIC_ROPE]
        if bad:
            raise NotImplementedError(f"BeamSharedCache(graph=True): rope_type {bad[0]!r} recomputes its tables from "
                                      "the running length at every step; a captured decode step cannot follow it "
                                      "(use graph=False)")
        self.decodes = 1

    def step(self, forward, input_ids, position_ids, tensors: dict, passthrough: dict):
        """A decode step after the warm-up. ``forward(**kw)``: the model's eager forward; ``tensors``:
        further per-step tensor inputs (``cache_position``) by name; ``passthrough``: what is the same
        at every step."""
        cache = self.cache
        self.decodes += 1
        if cache.layers[0].steps >= cache.state.capacity:
            raise RuntimeError(f"BeamSharedCache: max_new_tokens = {cache.state.capacity} generated positions are full")
        host_pos = position_ids is None                  # the model's own: arange(1) + the cache's length
        if host_pos:
            position_ids = torch.full((1, 1), cache.get_seq_length(), dtype=torch.int64, device=input_ids.device)
        inputs = dict(tensors, input_ids=input_ids, position_ids=position_ids)
        # what the captured step was called with, the tensors' values apart
        keys = (host_pos, tuple(sorted((k, v.shape, v.dtype) for k, v in inputs.items())),
                tuple(sorted((k, repr(v)) for k, v in passthrough.items())))
        if self.graph is None:
            self.static, self.keys = {k: v.clone() for k, v in inputs.items()}, keys
            steps = [ly.steps for ly in cache.layers]
            torch.cuda.synchronize(input_ids.device)
            graph = torch.cuda.CUDAGraph()
            # No garbage collection inside the capture: torch.cuda.graph no longer collects before it
            # begins, and a dead cycle that holds device memory or another graph (an earlier call's
            # objects) would be freed in the middle of the captured forward, which aborts the process.
            # Collect now, then keep the collector off until the capture has ended.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph):
                    out = forward(**self.static, attention_mask=None, past_key_values=cache, **passthrough)
            except BaseException:
                for ly, n in zip(cache.layers, steps):   # the capture launched nothing: the host count goes back
                    ly.steps = n
                raise
            finally:
                if gc_was_on:
                    gc.enable()
            self.graph, self.logits = graph, out.logits
            cache.graph_captures += 1
            graph.replay()                               # capturing ran nothing: this is the step itself
        else:
            if keys != self.keys:
                raise RuntimeError("BeamSharedCache(graph=True): this decode step's arguments differ from the captured "
                                   f"step's ({keys} vs {self.keys}); one cache serves one generate() call")
            for k, v in inputs.items():
                self.static[k].copy_(v)
            self.graph.replay()
            for ly in cache.layers:                      # what update() counts on the host
                ly.steps += 1
            cache.graph_replays += 1
        from transformers.modeling_outputs import CausalLMOutputWithPast
        return CausalLMOutputWithPast(loss=None, logits=self.logits.clone(), past_key_values=cache)


def smt_causal_lm_forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                          inputs_embeds=None, labels=None, use_cache=None, logits_to_keep=0, **kwargs):
    """The model-level forward ``patch_llama(attention=True)`` installs. A graphed decode step (gradients
    off, ``past_key_values`` a ``BeamSharedCache(graph=True)`` past its prefill, ``input_ids`` ``[R, 1]``,
    no labels, ``inputs_embeds``, hidden-state / attention outputs or ``return_dict=False``) goes to the
    cache's :class:`DecodeGraph`; every other call passes through unchanged to what ran before:
    :func:`fused_causal_lm_forward` where the fused LM-head loss is on, else transformers' forward."""
    from .beam_cache import BeamSharedCache
    prev = fused_causal_lm_forward if self.__dict__.get("_smt_lm_head_forward") else type(self).forward
    eager = lambda **kw: prev(self, **kw)
    cache = past_key_values
    if (isinstance(cache, BeamSharedCache) and cache.graph and not torch.is_grad_enabled()
            and cache.layers[0].is_initialized and isinstance(input_ids, torch.Tensor) and input_ids.dim() == 2
            and input_ids.shape[1] == 1 and input_ids.is_cuda and labels is None and inputs_embeds is None
            and kwargs.get("return_dict") is not False and not kwargs.get("output_hidden_states")
            and not kwargs.get("output_attentions")
            and not any(isinstance(v, torch.Tensor) for k, v in kwargs.items() if k != "cache_position")):
        if cache.decode_runner is None:
            cache.decode_runner = DecodeGraph(cache)
        runner = cache.decode_runner
        tensors = {k: kwargs.pop(k) for k in ("cache_position",) if isinstance(kwargs.get(k), torch.Tensor)}
        passthrough = dict(kwargs, use_cache=use_cache, logits_to_keep=logits_to_keep)
        if runner.decodes == 0:                          # the warm-up step: eager, with the mask as it came
            runner.warm_up(self)
            return eager(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                         past_key_values=cache, use_cache=use_cache, logits_to_keep=logits_to_keep, **tensors, **kwargs)
        return runner.step(eager, input_ids, position_ids, tensors, passthrough)
    return eager(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                 past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels, use_cache=use_cache,
                 logits_to_keep=logits_to_keep, **kwargs)


def _keep_2d_mask(config=None, inputs_embeds=None, attention_mask=None, **kwargs):
    """``create_masks_for_generate`` of a patched model: the 2-D padding mask as it came."""
    return attention_mask


def _patch(model, fam, what, attention, loss, lm_head_loss, decode_linears, decode_fp8) -> dict:
    """The body of :func:`patch_llama` and :func:`patch_model` over the classes of ``fam``."""
    if decode_fp8 and not decode_linears:
        raise ValueError(f"{what}(decode_fp8=True) needs decode_linears=True: the fp8 route is part of that routing")
    ml = fam.module
    counts = {"rmsnorm": 0, "mlp": 0, "rope": 1, "attention": 0, "loss": 0, "decoder": 0, "lm_head_loss": 0}
    if lm_head_loss is None:
        lm_head_loss = os.environ.get("SMT_LM_HEAD_LOSS", "1") != "0"
    if loss and hasattr(type(model), "loss_function"):
        model.loss_function = fused_causal_lm_loss
        counts["loss"] = 1
        if lm_head_loss and isinstance(model, fam.causal_lm):
            model.forward = fused_causal_lm_forward.__get__(model, type(model))
            counts["lm_head_loss"] = 1
    if attention:
        cfg = getattr(model, "config", None)
        if cfg is None:
            raise RuntimeError(f"{what}(attention=True) needs a transformers model with a config")
        if "smt_prev_attn" not in _EAGER:
            _EAGER["smt_prev_attn"] = cfg._attn_implementation
        cfg._attn_implementation = register_attention()
        counts["attention"] = sum(1 for m in model.modules() if isinstance(m, fam.attention))
        # generate() sends a static cache on a GPU through torch.compile unless told otherwise, and
        # torch.compile cannot trace the ctypes launches
        gen = getattr(model, "generation_config", None)
        if gen is not None and "_smt_prev_disable_compile" not in model.__dict__:
            model.__dict__["_smt_prev_disable_compile"] = getattr(gen, "disable_compile", False)
            gen.disable_compile = True
        if isinstance(model, fam.causal_lm):
            # the model-level forward that hands the decode steps of a BeamSharedCache(graph=True) to the
            # cache's DecodeGraph; every other call passes through to what ran before
            model.__dict__["_smt_lm_head_forward"] = bool(counts["lm_head_loss"])
            model.forward = smt_causal_lm_forward.__get__(model, type(model))
        if gen is not None:
            # ... and, for a compilable cache, builds the mask before the forward and passes the
            # result in place of the 2-D mask; only a 4-D tensor survives that. Keep the 2-D mask:
            # the forward builds the CacheMask itself, as with a DynamicCache.
            model.__dict__["create_masks_for_generate"] = _keep_2d_mask
    for m in model.modules():
        if isinstance(m, fam.rmsnorm):
            m.forward = fused_rmsnorm_forward.__get__(m, type(m))
            counts["rmsnorm"] += 1
        elif isinstance(m, fam.decoder):
            m.forward = fused_decoder_layer_forward.__get__(m, type(m))
            counts["decoder"] += 1
        elif isinstance(m, fam.mlp):
            act = getattr(m, "act_fn", None)
            if act is None or "silu" not in type(act).__name__.lower():
                raise NotImplementedError(f"fused MLP: SiLU activation only (got {type(act).__name__})")
            m.forward = fused_mlp_forward.__get__(m, type(m))
            counts["mlp"] += 1
        elif isinstance(m, nn.ModuleList) and len(m) > 1 and all(isinstance(x, fam.decoder) for x in m):
            # each decoder layer's fused tail normalises for the layer after it (a weak reference:
            # not a submodule)
            for i in range(len(m) - 1):
                m[i].__dict__["_smt_next_layer"] = weakref.ref(m[i + 1])
    ml.apply_rotary_pos_emb = fused_apply_rotary_pos_emb
    if decode_linears:
        counts["decode_linears"] = route_decode_linears(model, fp8=decode_fp8, family=fam, bias=what == "patch_model")
    return counts


def patch_llama(model: nn.Module, attention: bool = True, loss: bool = True, lm_head_loss: bool = None,
                decode_linears: bool = False, decode_fp8: bool = False) -> dict:
    """Route a transformers LLaMA model's RMSNorm / RoPE / SwiGLU / attention-residual add (and, with ``attention``, its
    attention; with ``loss``, its causal-LM loss) through the fused kernels. RoPE is patched at
    module level (``modeling_llama.apply_rotary_pos_emb``, looked up by ``LlamaAttention.forward`` at
    call time); attention by switching ``config._attn_implementation`` to the registered
    ``smt_flash``; the loss through the model's ``loss_function`` attribute. ``lm_head_loss``
    (default: ``SMT_LM_HEAD_LOSS``, on): with ``loss``, the model's forward runs the LM head and the
    loss together, chunk by chunk, without the full logits (:func:`fused_causal_lm_forward`).
    With ``attention``, a ``LlamaForCausalLM`` also gets :func:`smt_causal_lm_forward`, which replays the
    decode steps of a ``BeamSharedCache(graph=True)`` from a captured graph and passes every other call
    through unchanged (to :func:`fused_causal_lm_forward` where that is on, else to transformers').
    With ``attention``, ``generation_config.disable_compile`` is set and the model keeps the 2-D mask
    in ``generate()`` (``create_masks_for_generate``), so that ``cache_implementation="static"`` runs
    the kernels eagerly; :func:`unpatch_llama` restores both.
    ``decode_linears`` (off by default; nothing below exists on a model patched without it): the q/k/v/o and
    gate/up/down projections that are ``nn.Linear`` or ``LinearLayer_MatrixSparsity``, and a bias-free
    ``lm_head``, get :func:`decode_routed_linear_forward`: calls that :func:`decode_linear_reason` admits (no
    gradients, at most 16 rows: the decode steps) run the weight-streaming kernel of ``include/smt_linear.h``,
    q/k/v as one launch and gate/up/SwiGLU as one launch, where K is within
    ``DECODE_LINEAR_MAX_K`` and the launch's weights within ``DECODE_LINEAR_MAX_WEIGHT_ELEMS`` (the shapes at
    which the kernel measured faster than hipBLASLt); every
    other call runs what it ran before.
    ``decode_fp8`` (off by default, needs ``decode_linears``; without it no code path changes): on weights that
    carry an e4m3 copy (``engine.attach_fp8_weights``) the routed forwards first try the e4m3 weight-streaming
    kernel (smt_linear_skinny_fp8) where :func:`decode_linear_fp8_reason` admits the call and the
    ``DECODE_FP8_*`` size rule holds, and then fall through to what they do without it.
    Returns counts of patched modules (with ``decode_linears``, also the routed linears). Idempotent."""
    return _patch(model, FAMILIES["llama"], "patch_llama", attention, loss, lm_head_loss, decode_linears, decode_fp8)


def unpatch_llama(model: nn.Module = None) -> None:
    """Undo :func:`patch_llama` (module-level RoPE; per-instance forwards of ``model`` if given)."""
    _unpatch(model, FAMILIES["llama"])


def _unpatch(model, fam) -> None:
    ml = fam.module
    ml.apply_rotary_pos_emb = _EAGER[fam.rope_key]
    if model is not None and "smt_prev_attn" in _EAGER and getattr(model, "config", None) is not None:
        model.config._attn_implementation = _EAGER.pop("smt_prev_attn")
    if model is not None:
        if "_smt_prev_disable_compile" in model.__dict__:
            prev = model.__dict__.pop("_smt_prev_disable_compile")
            if getattr(model, "generation_config", None) is not None:
                model.generation_config.disable_compile = prev
        if model.__dict__.get("create_masks_for_generate") is _keep_2d_mask:
            del model.__dict__["create_masks_for_generate"]
        if "_loss_function" in model.__dict__:
            del model.__dict__["_loss_function"]
        if "forward" in model.__dict__:
            del model.__dict__["forward"]
        model.__dict__.pop("_smt_lm_head_forward", None)
        for m in model.modules():
            if isinstance(m, (fam.rmsnorm, fam.mlp, fam.decoder)) and "forward" in m.__dict__:
                del m.__dict__["forward"]
            m.__dict__.pop("_smt_next_layer", None)
        unroute_decode_linears(model)


def _refusal(model: nn.Module, fam) -> str:
    """Why :func:`patch_model` cannot serve ``model``, or None. Asked before anything is changed."""
    if fam is None:
        return (f"{type(model).__name__} is of no family the fused path knows "
                f"({', '.join(sorted(FAMILIES))}: their transformers classes)")
    others = [f for f in FAMILIES.values() if f is not fam and _has_classes_of(model, f)]
    if others:
        return f"the model mixes the classes of {fam.name} and {others[0].name}"
    cfg = getattr(model, "config", None)
    if cfg is None:
        return "the model has no transformers config"
    layer_types = getattr(cfg, "layer_types", None) or ()
    if "sliding_attention" in layer_types:
        return ("layer_types holds 'sliding_attention': the smt_flash kernels have no sliding window "
                f"({sum(1 for t in layer_types if t == 'sliding_attention')} of {len(layer_types)} layers)")
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    if head_dim != 128:
        return f"head_dim {head_dim}: the attention kernels are built for 128"
    for m in model.modules():
        if isinstance(m, fam.mlp):
            act = getattr(m, "act_fn", None)
            if act is None or "silu" not in type(act).__name__.lower():
                return f"fused MLP: SiLU activation only (got {type(act).__name__})"
    return None


def patch_model(model: nn.Module, attention: bool = True, loss: bool = True, lm_head_loss: bool = None,
                decode_linears: bool = False, decode_fp8: bool = False) -> dict:
    """:func:`patch_llama` for any family of :data:`FAMILIES` (LLaMA, Qwen2): the family is read from the
    model's classes and the same body runs over that family's RMSNorm, MLP, decoder-layer, attention and
    causal-LM classes and its modelling module's ``apply_rotary_pos_emb``; the keywords and the returned counts
    are :func:`patch_llama`'s. One thing differs from :func:`patch_llama` on a LLaMA model as well: with
    ``decode_linears`` the routed projections that carry a bias (Qwen2's q, k and v; a LLaMA model's with
    ``attention_bias=True``) go through the decode-linear kernel's bias epilogue, where :func:`patch_llama` leaves
    them on ``F.linear`` as before. The fused gate/up/SwiGLU launch takes no bias under either.
    Refused with ``NotImplementedError`` before anything is changed: a model of no known family or of two, a
    config whose ``layer_types`` holds ``"sliding_attention"``, a ``head_dim`` other than 128, an MLP whose
    activation is not SiLU. The RoPE patch is process-global per family, as :func:`patch_llama`'s is."""
    fam = model_family(model)
    why = _refusal(model, fam)
    if why is not None:
        raise NotImplementedError(f"patch_model: {why}")
    return _patch(model, fam, "patch_model", attention, loss, lm_head_loss, decode_linears, decode_fp8)


def unpatch_model(model: nn.Module) -> None:
    """Undo :func:`patch_model`: the per-instance forwards of ``model`` and the module-level RoPE of the
    model's family; the other family's modelling module is left as it is."""
    fam = model_family(model)
    if fam is None:
        raise NotImplementedError(f"unpatch_model: {type(model).__name__} is of no family the fused path knows")
    _unpatch(model, fam)
