"""Beam-search scoring on the device and the decoding loop that uses it.

:func:`beam_topk` is steps b and c of transformers' ``GenerationMixin._beam_search`` for one token:
``logits.float()`` -> ``log_softmax`` -> ``RepetitionPenaltyLogitsProcessor`` -> ``MinLength`` /
``MinNewTokensLength`` suppression -> the add of the running beam scores -> the reshape to
``[N, num_beams * V]`` -> ``torch.topk``. On a ROCm device it is one call of ``smt_beam_topk``
(csrc/beam_kernels.hip, C ABI include/smt_beam.h): three launches that read the logits in their own
format, no ``[R, V]`` fp32 tensor. ``impl="torch"``, CPU tensors and ``k > 32`` run transformers' own
chain of ops, the twin the tests compare the kernel against.

:func:`smt_beam_search` is transformers 5.15's ``_beam_search`` with those two steps replaced by one
:func:`beam_topk` call; pass it as ``model.generate(..., custom_generate=smt_beam_search)``. Whatever it
does not cover is handed to ``type(model)._beam_search`` unchanged and counted in ``stats.delegated``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from . import _hip

BEAM_CHUNK = 2048            # SMT_BEAM_CHUNK of include/smt_beam.h: elements of a row one workgroup reduces
MAX_K = 32                   # SMT_BEAM_MAX_K
MAX_SUPPRESSED = 8           # SMT_BEAM_MAX_SUPPRESSED


class LoopStats:
    """Counters of :func:`smt_beam_search`: ``calls``, of which ``delegated`` went to transformers'
    ``_beam_search``; ``sequences_scores`` are the returned hypotheses' final scores of the last call
    that did not delegate (transformers returns them only together with the per-step scores)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.calls = 0
        self.delegated = 0
        self.reasons = []
        self.sequences_scores = None


stats = LoopStats()


def _torch_chain(logits, beam_scores, sequences, cur_len, num_beams, k, penalty, suppressed):
    """transformers' own ops, in its order (generation/utils.py ``_beam_search`` steps b and c)."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    rows, vocab = logits.shape
    batch = rows // num_beams
    x = logits.to(copy=True, dtype=torch.float32)
    log_probs = torch.nn.functional.log_softmax(x, dim=-1)
    if penalty != 1.0:
        log_probs = RepetitionPenaltyLogitsProcessor(penalty=float(penalty))(sequences[:, :cur_len], log_probs)
    if len(suppressed):
        ids = torch.tensor(list(suppressed), device=logits.device)
        mask = torch.isin(torch.arange(vocab, device=logits.device), ids)
        log_probs = torch.where(mask, -math.inf, log_probs)
    log_probs = log_probs.view(batch, num_beams, vocab) + beam_scores.reshape(batch, num_beams)[:, :, None]
    log_probs = torch.reshape(log_probs, (batch, num_beams * vocab))
    return torch.topk(log_probs, k=k)


def beam_topk(logits: torch.Tensor, beam_scores: torch.Tensor, sequences: torch.Tensor, cur_len: int, num_beams: int,
              k: int, repetition_penalty: float = 1.0, suppressed: Sequence[int] = (), impl: Optional[str] = None):
    """The ``k`` best continuations of every sample: ``(top_scores [N, k] fp32, top_index [N, k] int64)``,
    descending, ``top_index = beam * V + token``.

    ``logits``: ``[N * num_beams, V]`` bf16 / fp16 / fp32, row ``n * num_beams + beam``; ``beam_scores``:
    fp32, ``N * num_beams`` values; ``sequences``: int64 ``[N * num_beams, >= cur_len]``, the rows' token
    history in ``[:, :cur_len]`` (prompt and padding included, as transformers passes it to its
    processors); ``suppressed``: at most 8 token ids scored ``-inf`` (more take the torch chain).
    ``impl``: ``None`` (the kernel for device tensors, the chain otherwise), ``"torch"`` (always the chain) or
    ``"hip"`` (the kernel, or an error where it cannot run)."""
    if impl not in (None, "torch", "hip"):
        raise ValueError(f"beam_topk: impl {impl!r} is not None, 'torch' or 'hip'")
    if logits.dim() != 2:
        raise ValueError(f"beam_topk: logits must be [rows, vocab], got {tuple(logits.shape)}")
    rows, vocab = logits.shape
    if num_beams < 1 or rows % num_beams:
        raise ValueError(f"beam_topk: {rows} rows are not a multiple of num_beams {num_beams}")
    sequences = sequences.reshape(rows, -1) if sequences.dim() != 2 else sequences
    if sequences.dtype != torch.int64 or sequences.shape[0] != rows or sequences.shape[1] < cur_len or cur_len < 0:
        raise ValueError(f"beam_topk: sequences must be int64 [{rows}, >= {cur_len}], got {sequences.dtype} "
                         f"{tuple(sequences.shape)}")
    if beam_scores.dtype != torch.float32 or beam_scores.numel() != rows:
        raise ValueError(f"beam_topk: beam_scores must hold {rows} fp32 values")
    if not (repetition_penalty > 0):
        raise ValueError(f"beam_topk: repetition_penalty must be > 0, got {repetition_penalty}")
    if not 1 <= k <= num_beams * vocab:
        raise ValueError(f"beam_topk: k {k} outside [1, {num_beams * vocab}]")
    suppressed = tuple(int(s) for s in suppressed)
    on_device = logits.device.type == "cuda"
    if impl == "hip" and not (on_device and k <= MAX_K and len(suppressed) <= MAX_SUPPRESSED):
        raise RuntimeError("beam_topk: impl='hip' needs device tensors, k <= 32 and at most 8 suppressed ids")
    if impl == "torch" or not on_device or k > MAX_K or len(suppressed) > MAX_SUPPRESSED:
        return _torch_chain(logits, beam_scores, sequences, cur_len, num_beams, k, repetition_penalty, suppressed)

    lib = _hip.load()
    dev = _hip._require_device(logits, beam_scores, sequences)
    if logits.dtype not in _hip._DT:
        raise RuntimeError(f"beam_topk: bf16, fp16 or fp32 logits only (got {logits.dtype})")
    if logits.stride(1) != 1 or (logits.stride(0) * logits.element_size()) % 16 or logits.data_ptr() % 16 \
            or logits.stride(0) < vocab:
        logits = logits.contiguous()
        if (vocab * logits.element_size()) % 16 or logits.data_ptr() % 16:      # rows the kernel cannot take
            pad = torch.empty(rows, (vocab + 7) // 8 * 8, dtype=logits.dtype, device=dev)
            pad[:, :vocab] = logits
            logits = pad[:, :vocab]
    if cur_len and sequences.stride(1) != 1:
        sequences = sequences.contiguous()
    beam_scores = beam_scores.reshape(rows).contiguous()
    batch = rows // num_beams
    need = lib.smt_beam_topk_workspace(batch, num_beams, vocab, k)
    if need < 0:
        _hip._check(-1, "smt_beam_topk_workspace")
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    top_scores = torch.empty(batch, k, dtype=torch.float32, device=dev)
    top_index = torch.empty(batch, k, dtype=torch.int32, device=dev)
    ids = (ctypes.c_int64 * max(1, len(suppressed)))(*suppressed)
    _hip._check(lib.smt_beam_topk(logits.data_ptr(), logits.stride(0), _hip._DT[logits.dtype], batch, num_beams, vocab,
                                  beam_scores.data_ptr(), sequences.data_ptr() if cur_len else None,
                                  sequences.stride(0), cur_len, float(repetition_penalty), ids, len(suppressed), k,
                                  top_scores.data_ptr(), top_index.data_ptr(), workspace.data_ptr(), _hip._stream(dev)),
                "smt_beam_topk")
    return top_scores, top_index.long()


class _Plan:
    """What the logits processors of a supported call amount to."""

    def __init__(self):
        self.penalty = 1.0
        self.prompt_ignore_length = 0
        self.min_rules = []             # (threshold, offset, ids): ids are -inf while cur_len - offset < threshold

    def suppressed(self, cur_len: int):
        ids = []
        for threshold, offset, eos in self.min_rules:
            if cur_len - offset < threshold:
                ids += [i for i in eos if i not in ids]
        return ids


def _plan(model, logits_processor, generation_config, synced_gpus):
    """A :class:`_Plan`, or the reason (a string) why transformers' loop has to run instead."""
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    g = generation_config
    if synced_gpus:
        return "synced_gpus"
    if g.do_sample:
        return "do_sample"
    if g.num_beams < 2:
        return "num_beams < 2"
    if g.return_dict_in_generate and (g.output_scores or g.output_logits or g.output_attentions or g.output_hidden_states):
        return "per-step outputs"
    if g.low_memory:
        return "low_memory"
    if model.config.is_encoder_decoder:
        return "encoder-decoder model"
    if type(model).__name__ in ("MoshiDepthDecoder", "ImageGPTForCausalImageModeling", "BarkSemanticModel"):
        return "vocabulary size of its own"
    plan = _Plan()
    seen_penalty = False
    for p in logits_processor or ():
        if type(p) is RepetitionPenaltyLogitsProcessor:
            if seen_penalty or p.logits_indices is not None or p.cu_seq_lens_q is not None:
                return "more than one repetition penalty"
            seen_penalty = True
            plan.penalty = float(p.penalty)
            plan.prompt_ignore_length = int(p.prompt_ignore_length or 0)
        elif type(p) is MinLengthLogitsProcessor:
            plan.min_rules.append((p.min_length, 0, [int(i) for i in p.eos_token_id.reshape(-1).tolist()]))
        elif type(p) is MinNewTokensLengthLogitsProcessor:
            plan.min_rules.append((p.min_new_tokens, p.prompt_length_to_skip,
                                   [int(i) for i in p.eos_token_id.reshape(-1).tolist()]))
        else:
            return f"logits processor {type(p).__name__}"
    return plan


def smt_beam_search(model, input_ids, logits_processor, stopping_criteria, generation_config, synced_gpus=False,
                    beam_topk_impl=None, **model_kwargs):
    """transformers' ``GenerationMixin._beam_search`` with steps b and c as one :func:`beam_topk` call on
    ``model_outputs.logits[:, -1]``; ``model.generate(..., custom_generate=smt_beam_search)``.

    Covered: ``do_sample=False``, ``num_beams >= 2``; no logits processor, one
    ``RepetitionPenaltyLogitsProcessor`` (with its ``prompt_ignore_length``), ``MinLength`` /
    ``MinNewTokensLength``; any ``length_penalty``, ``early_stopping``, ``eos_token_id`` list and cache
    (``BeamSharedCache(graph=True)`` included); a plain tensor, or ``return_dict_in_generate`` without
    per-step scores, logits, attentions or hidden states. Anything else runs ``type(model)._beam_search``
    with the same arguments and bumps ``stats.delegated``. ``beam_topk_impl`` is :func:`beam_topk`'s
    ``impl`` (``generate(..., beam_topk_impl="torch")`` runs the same loop on transformers' op chain)."""
    from transformers.generation.utils import ALL_CACHE_NAMES, GenerateBeamDecoderOnlyOutput
    stats.calls += 1
    plan = _plan(model, logits_processor, generation_config, synced_gpus)
    if isinstance(plan, str):
        stats.delegated += 1
        stats.reasons.append(plan)
        return type(model)._beam_search(model, input_ids, logits_processor=logits_processor,
                                        stopping_criteria=stopping_criteria, generation_config=generation_config,
                                        synced_gpus=synced_gpus, **model_kwargs)

    # 1. init beam_search values
    pad_token_id = generation_config._pad_token_tensor
    eos_token_id = generation_config._eos_token_tensor
    return_dict_in_generate = generation_config.return_dict_in_generate
    early_stopping = generation_config.early_stopping
    length_penalty = generation_config.length_penalty
    max_length = generation_config.max_length
    num_beams = generation_config.num_beams
    num_return_sequences = generation_config.num_return_sequences

    batch_size_unflattened, cur_len = input_ids.shape[:2]
    batch_size = batch_size_unflattened // num_beams
    vocab_size = model.config.get_text_config().vocab_size
    decoder_prompt_len = cur_len
    this_peer_finished = False
    device = input_ids.device

    n_eos_tokens = eos_token_id.shape[0] if eos_token_id is not None else 0
    beams_to_keep = max(2, 1 + n_eos_tokens) * num_beams
    top_num_beam_mask = torch.cat(
        (torch.ones((num_beams), dtype=torch.bool), torch.zeros((beams_to_keep - num_beams), dtype=torch.bool)),
        dim=0).to(device)

    # 3. init running tensors and static-shaped placeholders
    output_fill_value = pad_token_id or eos_token_id[0] if eos_token_id is not None else -1
    running_sequences = torch.full((batch_size, num_beams, max_length), fill_value=output_fill_value,
                                   dtype=torch.int64, device=device)
    running_sequences[:, :, :cur_len] = model._unflatten_beam_dim(input_ids, batch_size, num_beams)
    sequences = running_sequences.detach().clone()
    running_beam_scores = torch.zeros((batch_size, num_beams), dtype=torch.float, device=device)
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((batch_size, num_beams), fill_value=-1e9, dtype=torch.float, device=device)
    is_sent_finished = torch.zeros((batch_size, num_beams), dtype=torch.bool, device=device)
    is_early_stop_heuristic_unsatisfied = torch.ones((batch_size, 1), dtype=torch.bool, device=device)
    next_token_hits_stopping_criteria = torch.zeros((batch_size, num_beams), dtype=torch.bool, device=device)
    running_beam_indices = torch.full((batch_size, num_beams, max_length - cur_len), fill_value=-1, dtype=torch.int32,
                                      device=device)
    beam_indices = running_beam_indices.detach().clone()
    batch_offset = torch.arange(batch_size, device=device).view(-1, 1) * num_beams

    flat_running_sequences = input_ids
    prefill_consumed = False
    model_outputs = model._prefill(input_ids, generation_config, model_kwargs,
                                   is_first_iteration=not generation_config.is_assistant)

    # 4. run the generation loop
    while model._has_unfinished_sequences(this_peer_finished, synced_gpus, device=device):
        if prefill_consumed:
            # a. Forward current tokens, obtain the logits
            flat_running_sequences = model._flatten_beam_dim(running_sequences[:, :, :cur_len])
            next_sequence_length = 1 if model_kwargs["use_cache"] else None
            model_inputs = model.prepare_inputs_for_generation(
                flat_running_sequences, next_sequence_length=next_sequence_length, **model_kwargs)
            model_outputs = model(**model_inputs, return_dict=True)
        prefill_consumed = True
        model_kwargs = model._update_model_kwargs_for_generation(
            model_outputs, model_kwargs, is_encoder_decoder=model.config.is_encoder_decoder)

        # b + c. log-probabilities, processors, the running scores and the top K of every sample: one call
        logits = model_outputs.logits[:, -1, :]
        if logits.shape[-1] != vocab_size:
            raise ValueError(f"smt_beam_search: logits of width {logits.shape[-1]}, vocabulary {vocab_size}")
        if logits.device != device:
            logits = logits.to(device)
        skip = min(plan.prompt_ignore_length, cur_len)
        topk_log_probs, topk_indices = beam_topk(
            logits, running_beam_scores, flat_running_sequences[:, skip:], cur_len - skip, num_beams, beams_to_keep,
            repetition_penalty=plan.penalty, suppressed=plan.suppressed(cur_len), impl=beam_topk_impl)
        del model_outputs, logits

        # the rest of _get_top_k_continuations
        topk_current_beam_indices = topk_indices // vocab_size
        topk_running_beam_indices = model._gather_beams(running_beam_indices, topk_current_beam_indices)
        topk_running_sequences = model._gather_beams(running_sequences, topk_current_beam_indices)
        topk_ids = topk_indices % vocab_size
        topk_running_sequences[:, :, cur_len] = topk_ids
        topk_running_beam_indices[:, :, cur_len - decoder_prompt_len] = topk_current_beam_indices + batch_offset

        # d. Check which running sequences have finished
        next_token_hits_stopping_criteria = stopping_criteria(
            model._flatten_beam_dim(topk_running_sequences[:, :, : cur_len + 1]), None)
        next_token_hits_stopping_criteria = model._unflatten_beam_dim(
            next_token_hits_stopping_criteria, batch_size, beams_to_keep)

        # e. Get the non-finished running `num_beams` sequences for the next generation step
        running_sequences, running_beam_scores, running_beam_indices = model._get_running_beams_for_next_iteration(
            topk_log_probs=topk_log_probs, topk_running_sequences=topk_running_sequences,
            topk_running_beam_indices=topk_running_beam_indices,
            next_token_hits_stopping_criteria=next_token_hits_stopping_criteria, num_beams=num_beams)

        # f. Update the completed beams if a new high score in a finished sequence is found
        sequences, beam_scores, beam_indices, is_sent_finished = model._update_finished_beams(
            sequences=sequences, topk_running_sequences=topk_running_sequences, beam_scores=beam_scores,
            topk_log_probs=topk_log_probs, beam_indices=beam_indices,
            topk_running_beam_indices=topk_running_beam_indices,
            is_early_stop_heuristic_unsatisfied=is_early_stop_heuristic_unsatisfied, is_sent_finished=is_sent_finished,
            next_token_hits_stopping_criteria=next_token_hits_stopping_criteria, top_num_beam_mask=top_num_beam_mask,
            num_beams=num_beams, cur_len=cur_len, decoder_prompt_len=decoder_prompt_len, length_penalty=length_penalty,
            early_stopping=early_stopping)

        # g. Prepare remaining data for the next iteration: the cache follows the beams
        if any(cache_key in model_kwargs for cache_key in ALL_CACHE_NAMES):
            cache_key = next(cache_key for cache_key in ALL_CACHE_NAMES if cache_key in model_kwargs)
            beam_idx = model._flatten_beam_dim(running_beam_indices[..., cur_len - decoder_prompt_len])
            if hasattr(model, "_reorder_cache"):
                model_kwargs[cache_key] = model._reorder_cache(model_kwargs[cache_key], beam_idx)
            elif hasattr(model_kwargs[cache_key], "reorder_cache"):
                model_kwargs[cache_key].reorder_cache(beam_idx)
            else:
                raise ValueError(f"{type(model).__name__} cannot use beam search with a cache currently, as the cache "
                                 "cannot be reordered")

        cur_len = cur_len + 1
        is_early_stop_heuristic_unsatisfied = model._check_early_stop_heuristic(
            is_early_stop_heuristic_unsatisfied=is_early_stop_heuristic_unsatisfied,
            running_beam_scores=running_beam_scores, beam_scores=beam_scores, is_sent_finished=is_sent_finished,
            cur_len=cur_len, max_length=max_length, decoder_prompt_len=decoder_prompt_len,
            early_stopping=early_stopping, length_penalty=length_penalty)
        this_peer_finished = not model._beam_search_has_unfinished_sequences(
            is_early_stop_heuristic_unsatisfied, is_sent_finished, next_token_hits_stopping_criteria, early_stopping)

    # 5. prepare outputs
    sequences = model._flatten_beam_dim(sequences[:, :num_return_sequences, :])
    beam_scores = model._flatten_beam_dim(beam_scores[:, :num_return_sequences])
    beam_indices = model._flatten_beam_dim(beam_indices[:, :num_return_sequences, :])
    max_generated_length = ((beam_indices + 1).bool()).sum(dim=1).max()
    output_length = decoder_prompt_len + max_generated_length
    sequences = sequences[:, :output_length]
    beam_indices = beam_indices[:, :max_generated_length]
    stats.sequences_scores = beam_scores

    if return_dict_in_generate:
        cache = None
        if any(cache_key in model_kwargs for cache_key in ALL_CACHE_NAMES):
            cache_key = next(cache_key for cache_key in ALL_CACHE_NAMES if cache_key in model_kwargs)
            cache = model_kwargs[cache_key]
        # transformers returns sequences_scores only with output_scores, which this loop hands over to it
        return GenerateBeamDecoderOnlyOutput(sequences=sequences, sequences_scores=None, scores=None, logits=None,
                                             beam_indices=beam_indices, attentions=None, hidden_states=None,
                                             past_key_values=cache)
    return sequences
