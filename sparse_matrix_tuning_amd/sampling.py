"""Token selection for ``num_beams == 1`` on the device and the decoding loop that uses it.

:func:`sample_token` is what transformers' ``GenerationMixin._sample`` does between the model's logits and
the next token: ``logits.float()`` -> ``RepetitionPenaltyLogitsProcessor`` -> ``MinLength`` /
``MinNewTokensLength`` suppression -> temperature -> top-k -> top-p -> min-p -> ``softmax`` ->
``torch.multinomial`` (or ``argmax``). On a ROCm device it is one call of ``smt_sample_token``
(csrc/sample_kernels.hip, C ABI include/smt_sample.h, which states the contract): two launches, no
whole-vocabulary sort, a draw that is a pure function of ``(seed, step, row, token)``. ``impl="torch"`` and
CPU tensors run a torch restatement of the same contract -- the same hash, value thresholds that keep or
drop a group of equal values as a whole, the Gumbel argmax -- not transformers' chain: the draw is not
torch's Philox stream, so a sampled run equals ``torch.multinomial``'s in distribution only.

:func:`smt_sample` is transformers 5.15's ``_sample`` with the float copy, the processors and the token
selection replaced by one :func:`sample_token` call; pass it as
``model.generate(..., custom_generate=smt_sample)``. Whatever it does not cover is handed to
``type(model)._sample`` unchanged and counted in ``stats.delegated``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from . import _hip

SAMPLE_CHUNK = 2048          # SMT_SAMPLE_CHUNK of include/smt_sample.h
MAX_SUPPRESSED = 8           # SMT_SAMPLE_MAX_SUPPRESSED
_MASK = 0xFFFFFFFF


class LoopStats:
    """Counters of :func:`smt_sample`: ``calls``, of which ``delegated`` went to transformers' ``_sample``
    (``reasons`` says why); ``seed`` is the 64-bit seed of the last call that did not delegate."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.calls = 0
        self.delegated = 0
        self.reasons = []
        self.seed = None


stats = LoopStats()


def _mix(x: torch.Tensor) -> torch.Tensor:
    """``mix`` of include/smt_attention.h on int64 tensors that hold uint32 values."""
    x = x ^ (x >> 16)
    x = (x * 0x21F0AAAD) & _MASK
    x = x ^ (x >> 15)
    x = (x * 0x735A2D97) & _MASK
    return x ^ (x >> 15)


def gumbel(seed: int, step: int, rows: torch.Tensor, vocab: int) -> torch.Tensor:
    """fp32 ``[len(rows), vocab]``: ``g_v`` of include/smt_sample.h for the absolute row numbers ``rows``
    (int64), in torch's fp32 ``log`` (the kernel's ``logf`` may differ from it in the last place)."""
    seed_lo, seed_hi = seed & _MASK, (seed >> 32) & _MASK
    head = _mix((seed_lo + (rows & _MASK) * 0x9E3779B9) & _MASK) ^ seed_hi
    row_key = _mix((head + (step & _MASK) * 0x85EBCA6B) & _MASK)
    v = torch.arange(vocab, dtype=torch.int64, device=rows.device)
    word = _mix(row_key[:, None] ^ ((v * 0x9E3779B1) & _MASK)[None, :])
    u = ((word >> 8).float() + 0.5) * 2.0 ** -24
    u = u.clamp(max=1.0 - 2.0 ** -24)
    return -torch.log(-torch.log(u))


def scaled_logits(logits, sequences, cur_len, penalty, suppressed, temperature) -> torch.Tensor:
    """``z`` of include/smt_sample.h, fp32 ``[R, V]``: every step one correctly rounded fp32 operation."""
    x = logits.to(copy=True, dtype=torch.float32)
    rows, vocab = x.shape
    if penalty != 1.0 and cur_len:
        ids = sequences[:, :cur_len]
        inside = (ids >= 0) & (ids < vocab)                                  # ids outside [0, V) match nothing
        seen = torch.zeros(rows, vocab + 1, dtype=torch.bool, device=x.device)
        seen.scatter_(1, torch.where(inside, ids, vocab), True)
        pen = torch.tensor(penalty, dtype=torch.float32, device=x.device)
        x = torch.where(seen[:, :vocab], torch.where(x < 0, x * pen, x / pen), x)
    for s in suppressed:
        if 0 <= s < vocab:
            x[:, s] = -math.inf
    z = x / torch.tensor(temperature, dtype=torch.float32, device=x.device)
    return z + 0.0                                                           # -0 -> +0


def _lowest_argmax(score: torch.Tensor) -> torch.Tensor:
    best = score.max(dim=1, keepdim=True).values
    ids = torch.arange(score.shape[1], device=score.device).expand_as(score)
    return torch.where(score == best, ids, score.shape[1] - 1).min(dim=1).values


def _torch_sample(logits, sequences, cur_len, penalty, suppressed, temperature, top_k, top_p, min_p, do_sample, seed, step,
                  row0):
    """The contract of include/smt_sample.h in torch ops: masses and their sums in fp64."""
    z = scaled_logits(logits, sequences, cur_len, penalty, suppressed, temperature)
    rows, vocab = z.shape
    srt = torch.sort(z, dim=1, descending=True).values
    top = srt[:, :1]
    keep = torch.ones_like(srt, dtype=torch.bool)                            # in sorted order: always a prefix
    if 0 < top_k < vocab:
        keep &= srt >= srt[:, top_k - 1:top_k]
    if top_p < 1.0:
        thr = float(torch.tensor(1.0 - float(torch.tensor(top_p, dtype=torch.float32).double()), dtype=torch.float32))
        w = torch.where(keep, torch.exp(srt.double() - top.double()), 0.0)
        total = w.sum(dim=1, keepdim=True)
        cum = torch.cumsum(w, dim=1)
        first = torch.searchsorted(-srt, -srt, right=False)                  # where a value's group of equals starts
        above = torch.where(first > 0, torch.gather(cum, 1, (first - 1).clamp(min=0)), 0.0)
        keep &= (above < (1.0 - thr) * total) | (srt == top)
    if min_p > 0.0:
        log_min_p = torch.tensor(math.log(float(torch.tensor(min_p, dtype=torch.float32))), dtype=torch.float32)
        keep &= ~((srt - top) < log_min_p.to(z.device))
    kept = keep.sum(dim=1)
    threshold = torch.gather(srt, 1, (kept - 1).clamp(min=0)[:, None])
    score = z
    if do_sample:
        score = z + gumbel(seed, step, torch.arange(row0, row0 + rows, dtype=torch.int64, device=z.device), vocab)
    token = _lowest_argmax(torch.where(z >= threshold, score, -math.inf))
    return token, threshold[:, 0], kept.int()


def sample_token(logits: torch.Tensor, sequences: torch.Tensor, cur_len: int, *, repetition_penalty: float = 1.0,
                 suppressed: Sequence[int] = (), temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 min_p: float = 0.0, do_sample: bool = True, seed: int = 0, step: int = 0, row0: int = 0,
                 impl: Optional[str] = None):
    """The next token of every row: ``(token int64 [R], threshold fp32 [R], kept int32 [R])``. The kept set
    of row r is ``{v : z_v >= threshold[r]}``, ``kept[r]`` its size (include/smt_sample.h has the contract).

    ``logits``: ``[R, V]`` bf16 / fp16 / fp32; ``sequences``: int64 ``[R, >= cur_len]``, the rows' token
    history in ``[:, :cur_len]``; ``suppressed``: token ids scored ``-inf`` (more than 8 take the torch
    restatement); ``top_k <= 0``, ``top_p >= 1`` and ``min_p <= 0`` switch a filter off; ``do_sample=False``
    is the argmax. ``seed`` (64 bits), ``step`` and the absolute row number ``row0 + r`` key the draw.
    ``impl``: ``None`` (the kernel for device tensors, the restatement otherwise), ``"torch"`` (always the
    restatement) or ``"hip"`` (the kernel, or an error where it cannot run)."""
    if impl not in (None, "torch", "hip"):
        raise ValueError(f"sample_token: impl {impl!r} is not None, 'torch' or 'hip'")
    if logits.dim() != 2:
        raise ValueError(f"sample_token: logits must be [rows, vocab], got {tuple(logits.shape)}")
    rows, vocab = logits.shape
    if rows < 1 or vocab < 1:
        raise ValueError(f"sample_token: empty logits {tuple(logits.shape)}")
    sequences = sequences.reshape(rows, -1) if sequences.dim() != 2 else sequences
    if sequences.dtype != torch.int64 or sequences.shape[0] != rows or sequences.shape[1] < cur_len or cur_len < 0:
        raise ValueError(f"sample_token: sequences must be int64 [{rows}, >= {cur_len}], got {sequences.dtype} "
                         f"{tuple(sequences.shape)}")
    if not (repetition_penalty > 0):
        raise ValueError(f"sample_token: repetition_penalty must be > 0, got {repetition_penalty}")
    if not (0 < temperature < math.inf):
        raise ValueError(f"sample_token: temperature must be > 0 and finite, got {temperature}")
    if not (top_p > 0):
        raise ValueError(f"sample_token: top_p must be > 0, got {top_p}")
    if not (min_p <= 1):
        raise ValueError(f"sample_token: min_p must be <= 1, got {min_p}")
    if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 32 and 0 <= row0 and row0 + rows <= 2 ** 32):
        raise ValueError(f"sample_token: seed {seed}, step {step} or row0 {row0} out of range")
    suppressed = tuple(int(s) for s in suppressed)
    top_k = int(top_k) if 0 < top_k < vocab else 0
    on_device = logits.device.type == "cuda"
    if impl == "hip" and not (on_device and len(suppressed) <= MAX_SUPPRESSED):
        raise RuntimeError("sample_token: impl='hip' needs device tensors and at most 8 suppressed ids")
    if impl == "torch" or not on_device or len(suppressed) > MAX_SUPPRESSED:
        return _torch_sample(logits, sequences, cur_len, float(repetition_penalty), suppressed, float(temperature), top_k,
                             float(top_p), float(min_p), bool(do_sample), seed, step, row0)

    lib = _hip.load()
    dev = _hip._require_device(logits, sequences)
    if logits.dtype not in _hip._DT:
        raise RuntimeError(f"sample_token: bf16, fp16 or fp32 logits only (got {logits.dtype})")
    if logits.stride(1) != 1 or (logits.stride(0) * logits.element_size()) % 16 or logits.data_ptr() % 16 \
            or logits.stride(0) < vocab:
        logits = logits.contiguous()
        if (vocab * logits.element_size()) % 16 or logits.data_ptr() % 16:      # rows the kernel cannot take
            pad = torch.empty(rows, (vocab + 7) // 8 * 8, dtype=logits.dtype, device=dev)
            pad[:, :vocab] = logits
            logits = pad[:, :vocab]
    if cur_len and sequences.stride(1) != 1:
        sequences = sequences.contiguous()
    need = lib.smt_sample_workspace(rows, vocab)
    if need < 0:
        _hip._check(-1, "smt_sample_workspace")
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    token = torch.empty(rows, dtype=torch.int32, device=dev)
    threshold = torch.empty(rows, dtype=torch.float32, device=dev)
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    ids = (ctypes.c_int64 * max(1, len(suppressed)))(*suppressed)
    _hip._check(lib.smt_sample_token(logits.data_ptr(), logits.stride(0), _hip._DT[logits.dtype], rows, vocab,
                                     sequences.data_ptr() if cur_len else None, sequences.stride(0), cur_len,
                                     float(repetition_penalty), ids, len(suppressed), float(temperature), top_k, float(top_p),
                                     float(min_p), 1 if do_sample else 0, seed, step, row0, token.data_ptr(),
                                     threshold.data_ptr(), kept.data_ptr(), workspace.data_ptr(), _hip._stream(dev)),
                "smt_sample_token")
    return token.long(), threshold, kept


class _Plan:
    """What the logits processors of a supported call amount to."""

    def __init__(self):
        self.penalty = 1.0
        self.prompt_ignore_length = 0
        self.min_rules = []             # (threshold, offset, ids): ids are -inf while cur_len - offset < threshold
        self.temperature = 1.0
        self.top_k = 0
        self.top_p = 1.0
        self.min_p = 0.0

    def suppressed(self, cur_len: int):
        ids = []
        for threshold, offset, eos in self.min_rules:
            if cur_len - offset < threshold:
                ids += [i for i in eos if i not in ids]
        return ids


def _plan(model, logits_processor, generation_config, synced_gpus):
    """A :class:`_Plan`, or the reason (a string) why transformers' loop has to run instead."""
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                        MinPLogitsWarper, RepetitionPenaltyLogitsProcessor,
                                                        TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    g = generation_config
    if synced_gpus:
        return "synced_gpus"
    if g.return_dict_in_generate and (g.output_scores or g.output_logits or g.output_attentions or g.output_hidden_states):
        return "per-step outputs"
    if model.config.is_encoder_decoder:
        return "encoder-decoder model"
    if g.renormalize_logits:
        return "renormalize_logits"
    plan = _Plan()
    # transformers' order: the penalty and the length rules (a -inf stays -inf under the penalty, so these
    # commute: a penalty passed as `logits_processor=` comes after the length rules), then temperature,
    # top-k, top-p, min-p
    order = {RepetitionPenaltyLogitsProcessor: 0, MinLengthLogitsProcessor: 1, MinNewTokensLengthLogitsProcessor: 1,
             TemperatureLogitsWarper: 2, TopKLogitsWarper: 3, TopPLogitsWarper: 4, MinPLogitsWarper: 5}
    last, seen_penalty = -1, False
    for p in logits_processor or ():
        stage = order.get(type(p))
        if stage is None:
            return f"logits processor {type(p).__name__}"
        if stage == 0 and seen_penalty:
            return "more than one repetition penalty"
        seen_penalty |= stage == 0
        if max(stage, 1) < last or (stage == last and stage >= 2):
            return f"logits processors in another order ({type(p).__name__})"
        last = max(stage, 1)
        if stage >= 3 and (p.min_tokens_to_keep != 1 or p.filter_value != -math.inf):
            return f"min_tokens_to_keep or filter_value of {type(p).__name__}"
        if stage == 0:
            if p.logits_indices is not None or p.cu_seq_lens_q is not None:
                return "repetition penalty over packed logits"
            plan.penalty = float(p.penalty)
            plan.prompt_ignore_length = int(p.prompt_ignore_length or 0)
        elif type(p) is MinLengthLogitsProcessor:
            plan.min_rules.append((p.min_length, 0, [int(i) for i in p.eos_token_id.reshape(-1).tolist()]))
        elif type(p) is MinNewTokensLengthLogitsProcessor:
            plan.min_rules.append((p.min_new_tokens, p.prompt_length_to_skip,
                                   [int(i) for i in p.eos_token_id.reshape(-1).tolist()]))
        elif stage == 2:
            plan.temperature = float(p.temperature)
        elif stage == 3:
            plan.top_k = int(p.top_k)
        elif stage == 4:
            plan.top_p = float(p.top_p)
        else:
            plan.min_p = float(p.min_p)
    return plan


def smt_sample(model, input_ids, logits_processor, stopping_criteria, generation_config, synced_gpus=False, streamer=None,
               sample_seed=None, sample_impl=None, **model_kwargs):
    """transformers' ``GenerationMixin._sample`` with the float copy, the logits processors and the token
    selection as one :func:`sample_token` call on ``outputs.logits[:, -1]``;
    ``model.generate(..., custom_generate=smt_sample)``.

    Covered: ``num_beams == 1`` with ``do_sample`` true or false; at most one
    ``RepetitionPenaltyLogitsProcessor`` (with its ``prompt_ignore_length``), ``MinLength`` /
    ``MinNewTokensLength``, then the temperature, top-k, top-p and min-p warpers in transformers' order with
    ``min_tokens_to_keep == 1`` and ``filter_value == -inf``; any stopping criteria, eos list, streamer and
    cache (``BeamSharedCache(config, 1, max_new_tokens, graph=True)`` included: the selection runs outside
    the captured graph); a plain tensor, or ``return_dict_in_generate`` without per-step outputs. Anything
    else runs ``type(model)._sample`` with the same arguments and bumps ``stats.delegated``.

    The draw of row r at a step is keyed by ``(seed, cur_len, r)``, ``cur_len`` the absolute position of the
    token. transformers 5.15's ``generate`` hands a callable ``custom_generate`` only the callable's own keywords,
    so a streamer is bound with ``functools.partial(smt_sample, streamer=...)``. ``sample_seed=None`` draws one 64-bit seed per call from torch's default CPU generator, so
    ``torch.manual_seed`` governs it; an int pins it. ``sample_impl`` is :func:`sample_token`'s ``impl``."""
    from transformers.generation.utils import ALL_CACHE_NAMES, GenerateDecoderOnlyOutput
    if generation_config.num_beams is not None and generation_config.num_beams > 1:
        raise ValueError("smt_sample: num_beams > 1 is smt_beam_search's")
    stats.calls += 1
    plan = _plan(model, logits_processor, generation_config, synced_gpus)
    if isinstance(plan, str):
        stats.delegated += 1
        stats.reasons.append(plan)
        return type(model)._sample(model, input_ids, logits_processor=logits_processor,
                                   stopping_criteria=stopping_criteria, generation_config=generation_config,
                                   synced_gpus=synced_gpus, streamer=streamer, **model_kwargs)
    if sample_seed is None:
        lo, hi = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()
        sample_seed = (hi << 32) | lo
    seed = int(sample_seed) & (2 ** 64 - 1)
    stats.seed = seed

    # init values
    pad_token_id = generation_config._pad_token_tensor
    return_dict_in_generate = generation_config.return_dict_in_generate
    has_eos_stopping_criteria = any(hasattr(criteria, "eos_token_id") for criteria in stopping_criteria)
    do_sample = bool(generation_config.do_sample)

    # keep track of which sequences are already finished
    batch_size, cur_len = input_ids.shape[:2]
    this_peer_finished = False
    unfinished_sequences = torch.ones(batch_size, dtype=torch.long, device=input_ids.device)
    if pad_token_id is not None:
        pad_token_id = pad_token_id.to(input_ids.device)

    model_forward = (model.get_compiled_call(generation_config.compile_config)
                     if model._valid_auto_compile_criteria(model_kwargs, generation_config) else model.__call__)

    prefill_consumed = False
    outputs = model._prefill(input_ids, generation_config, model_kwargs,
                             is_first_iteration=not generation_config.is_assistant)

    with model._optimize_model_for_decode():
        while model._has_unfinished_sequences(this_peer_finished, synced_gpus, device=input_ids.device):
            if prefill_consumed:
                next_sequence_length = 1 if model_kwargs["use_cache"] else None
                model_inputs = model.prepare_inputs_for_generation(
                    input_ids, next_sequence_length=next_sequence_length, **model_kwargs)
                outputs = model_forward(**model_inputs, return_dict=True)
            prefill_consumed = True
            model_kwargs = model._update_model_kwargs_for_generation(
                outputs, model_kwargs, is_encoder_decoder=model.config.is_encoder_decoder)

            # float copy, processors and token selection: one call that reads the logits in their own format
            logits = outputs.logits[:, -1]
            if logits.device != input_ids.device:
                logits = logits.to(input_ids.device)
            skip = min(plan.prompt_ignore_length, cur_len)
            next_tokens, _, _ = sample_token(
                logits, input_ids[:, skip:], cur_len - skip, repetition_penalty=plan.penalty,
                suppressed=plan.suppressed(cur_len), temperature=plan.temperature, top_k=plan.top_k, top_p=plan.top_p,
                min_p=plan.min_p, do_sample=do_sample, seed=seed, step=cur_len, row0=0, impl=sample_impl)
            del logits

            # finished sentences should have their next token be a padding token
            if has_eos_stopping_criteria:
                next_tokens = next_tokens * unfinished_sequences + pad_token_id * (1 - unfinished_sequences)

            # update generated ids, model inputs, and length for next step
            input_ids = torch.cat([input_ids, next_tokens[:, None]], dim=-1)
            cur_len += 1
            if streamer is not None:
                streamer.put(next_tokens.cpu())

            unfinished_sequences = unfinished_sequences & ~stopping_criteria(input_ids, None)
            this_peer_finished = unfinished_sequences.max() == 0
            del outputs

    if streamer is not None:
        streamer.end()

    if return_dict_in_generate:
        cache = None
        if any(cache_key in model_kwargs for cache_key in ALL_CACHE_NAMES):
            cache_key = next(cache_key for cache_key in ALL_CACHE_NAMES if cache_key in model_kwargs)
            cache = model_kwargs[cache_key]
        return GenerateDecoderOnlyOutput(sequences=input_ids, scores=None, logits=None, attentions=None, hidden_states=None,
                                         past_key_values=cache)
    return input_ids
