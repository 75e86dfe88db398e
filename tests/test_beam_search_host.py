"""beam_search without a GPU: the torch path of beam_topk against the chain of ops written out by hand as
transformers' _beam_search runs it, smt_beam_search against plain generate() on a CPU fp32 tiny LLaMA (the
config of tests/test_gpu_generate_graph.py), the delegation of what the loop does not cover, and every
refusal of the C ABI (they return before any HIP call)."""
import ctypes
import math
import os
import re

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import beam_search as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, NEW = 4, 12


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "smt_beam.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("SMT_BEAM_CHUNK") == bs.BEAM_CHUNK
    assert define("SMT_BEAM_MAX_K") == bs.MAX_K and define("SMT_BEAM_MAX_SUPPRESSED") == bs.MAX_SUPPRESSED


def _chain(logits, beam_scores, sequences, cur_len, nb, k, penalty, suppressed):
    """generation/utils.py _beam_search steps b and c with generation/logits_process.py's processors."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    R, V = logits.shape
    x = logits.to(copy=True, dtype=torch.float32)
    log_probs = torch.nn.functional.log_softmax(x, dim=-1)
    procs = LogitsProcessorList()
    if penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=penalty))
    if suppressed:
        procs.append(MinLengthLogitsProcessor(cur_len + 1, list(suppressed)))
    log_probs = procs(sequences[:, :cur_len], log_probs)
    log_probs = log_probs.view(R // nb, nb, V) + beam_scores.view(R // nb, nb)[:, :, None]
    return torch.topk(torch.reshape(log_probs, (R // nb, nb * V)), k=k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("penalty, suppressed", [(1.0, ()), (1.1, ()), (1.3, (5, 77)), (0.8, (0,))])
def test_torch_path_is_the_transformers_chain(dtype, penalty, suppressed):
    g = torch.Generator().manual_seed(0)
    N, V, cur_len, k = 3, 301, 9, 8
    logits = (torch.randn(N * NB, V, generator=g) * 3).to(dtype)
    beam_scores = -torch.rand(N, NB, generator=g) * 5
    sequences = torch.randint(0, V, (N * NB, cur_len + 4), generator=g)
    sequences[:, 3] = sequences[:, 2]                                    # a duplicate
    want = _chain(logits, beam_scores, sequences, cur_len, NB, k, penalty, suppressed)
    for impl in ("torch", None):                                          # CPU tensors take the chain either way
        got = bs.beam_topk(logits, beam_scores, sequences, cur_len, NB, k, repetition_penalty=penalty,
                           suppressed=suppressed, impl=impl)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
    big = bs.beam_topk(logits, beam_scores, sequences, cur_len, NB, 40, repetition_penalty=penalty, suppressed=suppressed)
    assert big[0].shape == (N, 40)                                        # k > 32: the chain
    with pytest.raises(RuntimeError, match="impl='hip'"):
        bs.beam_topk(logits, beam_scores, sequences, cur_len, NB, k, impl="hip")


def test_wrapper_refuses_bad_arguments():
    x, s, q = torch.zeros(8, 16), torch.zeros(8), torch.zeros(8, 4, dtype=torch.int64)
    for bad in (lambda: bs.beam_topk(x, s, q, 4, 3, 2), lambda: bs.beam_topk(x, s, q, 5, 4, 2),
                lambda: bs.beam_topk(x, s, q.int(), 4, 4, 2), lambda: bs.beam_topk(x, s.double(), q, 4, 4, 2),
                lambda: bs.beam_topk(x, s, q, 4, 4, 0), lambda: bs.beam_topk(x, s, q, 4, 4, 65),
                lambda: bs.beam_topk(x, s, q, 4, 4, 2, repetition_penalty=0.0),
                lambda: bs.beam_topk(x, s, q, 4, 4, 2, repetition_penalty=float("nan")),
                lambda: bs.beam_topk(x, s, q, 4, 4, 2, impl="triton")):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64,
                      pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    torch.manual_seed(3)
    model = LlamaForCausalLM(cfg).float().eval()
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 512, (2, 13), generator=g)
    mask = torch.ones_like(ids)
    ids[1, :6], mask[1, :6] = 0, 0                                       # left padding
    return model, ids, mask


def _pair(tiny, seed=None, **kw):
    """(transformers' result with output_scores, so that it returns sequences_scores; smt_beam_search's
    sequences; its final scores; whether it delegated)."""
    model, ids, mask = tiny
    args = dict(input_ids=ids, attention_mask=mask, num_beams=NB, do_sample=False, max_new_tokens=NEW, **kw)
    if seed is not None:
        torch.manual_seed(seed)
    want = model.generate(return_dict_in_generate=True, output_scores=True, **args)
    bs.stats.reset()
    if seed is not None:
        torch.manual_seed(seed)
    got = model.generate(custom_generate=bs.smt_beam_search, **args)
    assert bs.stats.calls == 1
    return want, got, bs.stats.sequences_scores, bs.stats.delegated


@pytest.mark.parametrize("kw", [{}, {"repetition_penalty": 1.1}, {"repetition_penalty": 1.1, "min_new_tokens": 6},
                                {"min_length": 20}, {"num_return_sequences": 3, "repetition_penalty": 1.3},
                                {"early_stopping": True, "length_penalty": 2.0}], ids=str)
def test_loop_equals_generate(tiny, kw):
    want, got, scores, delegated = _pair(tiny, **kw)
    assert delegated == 0
    assert torch.equal(got, want.sequences) and torch.equal(scores, want.sequences_scores)


def test_prompt_ignore_length_is_an_offset(tiny):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    mk = lambda: [RepetitionPenaltyLogitsProcessor(penalty=1.5, prompt_ignore_length=9)]
    model, ids, mask = tiny
    args = dict(input_ids=ids, attention_mask=mask, num_beams=NB, do_sample=False, max_new_tokens=NEW)
    want = model.generate(logits_processor=mk(), return_dict_in_generate=True, output_scores=True, **args)
    bs.stats.reset()
    real, seen = bs.beam_topk, []
    bs.beam_topk = lambda logits, scores, seq, cur_len, *a, **k: (seen.append((seq.shape[1], cur_len)),
                                                                  real(logits, scores, seq, cur_len, *a, **k))[1]
    try:
        got = model.generate(logits_processor=mk(), custom_generate=bs.smt_beam_search, **args)
    finally:
        bs.beam_topk = real
    assert seen == [(4 + t, 4 + t) for t in range(NEW)]                   # 13 prompt tokens, 9 of them ignored
    assert bs.stats.delegated == 0 and torch.equal(got, want.sequences)
    assert torch.equal(bs.stats.sequences_scores, want.sequences_scores)


@pytest.mark.parametrize("length_penalty", [1.0, 0.5])
def test_hypotheses_finish_on_an_eos_list(tiny, length_penalty):
    """The eos ids are tokens a first run produced, so hypotheses do finish (and K grows to 3 * num_beams)."""
    model, ids, mask = tiny
    first = model.generate(input_ids=ids, attention_mask=mask, num_beams=NB, do_sample=False, max_new_tokens=NEW,
                           repetition_penalty=1.1)
    eos = sorted({int(first[0, 13 + 3]), int(first[1, 13 + 5])})
    kw = dict(eos_token_id=eos, repetition_penalty=1.1, length_penalty=length_penalty)
    want, got, scores, delegated = _pair(tiny, **kw)
    assert delegated == 0
    assert torch.equal(got, want.sequences) and torch.equal(scores, want.sequences_scores)
    generated = want.sequences[:, 13:]
    assert torch.isin(generated, torch.tensor(eos)).any(dim=1).all()       # every returned hypothesis finished
    as_dict = model.generate(input_ids=ids, attention_mask=mask, num_beams=NB, do_sample=False, max_new_tokens=NEW,
                             custom_generate=bs.smt_beam_search, return_dict_in_generate=True, **kw)
    assert torch.equal(as_dict.sequences, want.sequences) and as_dict.sequences_scores is None
    assert torch.equal(as_dict.beam_indices, want.beam_indices)


@pytest.mark.parametrize("kw, reason", [
    ({"no_repeat_ngram_size": 2}, "NoRepeatNGram"), ({"do_sample": True, "top_k": 20}, "do_sample"),
    ({"return_dict_in_generate": True, "output_scores": True}, "per-step"),
    ({"return_dict_in_generate": True, "output_logits": True}, "per-step"),
    ({"repetition_penalty": 1.1, "renormalize_logits": True}, "LogitNormalization")], ids=str)
def test_unsupported_cases_delegate(tiny, kw, reason):
    model, ids, mask = tiny
    args = dict(input_ids=ids, attention_mask=mask, num_beams=NB, max_new_tokens=NEW, **{"do_sample": False, **kw})
    torch.manual_seed(5)
    want = model.generate(**args)
    bs.stats.reset()
    torch.manual_seed(5)
    got = model.generate(custom_generate=bs.smt_beam_search, **args)
    assert bs.stats.delegated == 1 and reason in bs.stats.reasons[0]
    if isinstance(want, torch.Tensor):
        assert torch.equal(got, want)
    else:
        assert torch.equal(got.sequences, want.sequences)
        for name in ("scores", "logits"):
            a, b = getattr(want, name), getattr(got, name)
            assert (a is None) == (b is None) and (a is None or all(torch.equal(x, y) for x, y in zip(a, b)))


def test_synced_gpus_and_greedy_delegate(tiny):
    model = tiny[0]
    cfg = model.generation_config
    assert bs._plan(model, [], cfg, True) == "synced_gpus"
    from copy import deepcopy
    one = deepcopy(cfg)
    one.num_beams = 1
    assert bs._plan(model, [], one, False) == "num_beams < 2"


def test_c_abi_refusals():
    """Every -1 / -2 of smt_beam_topk comes back without a device: the pointers are never dereferenced."""
    lib = _hip.load(build_if_missing=True)
    p, stream = ctypes.c_void_p(4096), None
    sup = (ctypes.c_int64 * 2)(1, 2)
    good = dict(logits=p, ld=512, dtype=_hip.DTYPE_BF16, N=2, nb=4, V=512, beam_scores=p, sequences=p, seq_ld=16,
                cur_len=16, penalty=1.1, suppressed=sup, n_suppressed=2, K=8, top_scores=p, top_index=p, workspace=p)

    def call(**kw):
        a = {**good, **kw}
        return lib.smt_beam_topk(a["logits"], a["ld"], a["dtype"], a["N"], a["nb"], a["V"], a["beam_scores"],
                                 a["sequences"], a["seq_ld"], a["cur_len"], a["penalty"], a["suppressed"],
                                 a["n_suppressed"], a["K"], a["top_scores"], a["top_index"], a["workspace"], stream)

    invalid = [dict(logits=None), dict(beam_scores=None), dict(sequences=None), dict(top_scores=None),
               dict(top_index=None), dict(workspace=None), dict(N=0), dict(nb=0), dict(V=0), dict(ld=511),
               dict(seq_ld=15), dict(cur_len=-1), dict(K=0), dict(K=33), dict(V=1, ld=8, nb=4, K=5), dict(dtype=7),
               dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=math.nan), dict(n_suppressed=-1),
               dict(n_suppressed=9), dict(suppressed=None), dict(nb=5, V=2 ** 30, ld=2 ** 30)]
    for kw in invalid:
        assert call(**kw) == -1, kw
        assert lib.smt_beam_last_error().startswith(b"smt_beam_topk: "), kw
    misaligned = [dict(logits=ctypes.c_void_p(4098)), dict(ld=516), dict(dtype=_hip.DTYPE_FP32, ld=514),
                  dict(workspace=ctypes.c_void_p(4104)), dict(sequences=ctypes.c_void_p(4100))]
    for kw in misaligned:
        assert call(**kw) == -2, kw
    assert b"aligned" in lib.smt_beam_last_error()
    assert lib.smt_beam_topk_workspace(0, 4, 512, 8) == -1 and lib.smt_beam_topk_workspace(2, 4, 512, 33) == -1
    # per (row, chunk): a float2 partial and K 8-byte candidates; the partials rounded up to 16 bytes
    assert lib.smt_beam_topk_workspace(4, 4, 128256, 8) == 16 * 63 * 8 + 16 * 63 * 8 * 8
    assert lib.smt_beam_topk_workspace(1, 1, 1, 1) == 16 + 8
