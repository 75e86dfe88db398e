"""sampling.smt_sample without a GPU, through the torch restatement of the contract, on a CPU fp32 tiny LLaMA
(the config of tests/test_beam_search_host.py): greedy against plain generate(), the seeding of a sampled run,
every delegation, return_dict_in_generate, the wrapper's and the C ABI's refusals."""
import ctypes
import math
import os
import re

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import beam_search as bs
from sparse_matrix_tuning_amd import sampling as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = 12
SAMPLED = dict(do_sample=True, temperature=0.6, top_p=0.95, top_k=50, repetition_penalty=1.1)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "smt_sample.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("SMT_SAMPLE_CHUNK") == sp.SAMPLE_CHUNK and define("SMT_SAMPLE_MAX_SUPPRESSED") == sp.MAX_SUPPRESSED


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


def _run(tiny, **kw):
    model, ids, mask = tiny
    sp.stats.reset()
    out = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, custom_generate=sp.smt_sample, **kw)
    assert sp.stats.calls == 1
    return out


@pytest.mark.parametrize("kw", [{}, {"repetition_penalty": 1.1}, {"repetition_penalty": 1.3, "min_new_tokens": 6},
                                {"min_length": 20}], ids=str)
def test_greedy_equals_generate(tiny, kw):
    model, ids, mask = tiny
    want = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False, **kw)
    got = _run(tiny, do_sample=False, **kw)
    assert sp.stats.delegated == 0 and torch.equal(got, want)


def test_greedy_stops_on_an_eos_list_and_pads(tiny):
    model, ids, mask = tiny
    first = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False)
    eos = [int(first[0, 13 + 3])]                                        # row 0 finishes early and is padded
    want = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False, eos_token_id=eos)
    got = _run(tiny, do_sample=False, eos_token_id=eos)
    assert sp.stats.delegated == 0 and torch.equal(got, want) and (got[0, 13 + 4:] == 0).all()


def test_a_sampled_run_follows_its_seed(tiny):
    a = _run(tiny, sample_seed=11, **SAMPLED)
    assert sp.stats.delegated == 0 and sp.stats.seed == 11
    b = _run(tiny, sample_seed=11, **SAMPLED)
    c = _run(tiny, sample_seed=12, **SAMPLED)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.shape == (2, 13 + NEW) and ((a >= 0) & (a < 512)).all()


def test_manual_seed_governs_the_default_seed(tiny):
    torch.manual_seed(21)
    a = _run(tiny, **SAMPLED)
    seed_a = sp.stats.seed
    b = _run(tiny, **SAMPLED)                                            # the generator has moved on
    seed_b = sp.stats.seed
    torch.manual_seed(21)
    c = _run(tiny, **SAMPLED)
    assert seed_a == sp.stats.seed != seed_b and 0 <= seed_a < 2 ** 64
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_every_step_is_one_call_with_the_plan(tiny):
    """What the loop hands to sample_token: the warpers' values, the absolute position as the step, the
    history less prompt_ignore_length, eos suppressed while min_new_tokens holds."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    real, seen = sp.sample_token, []
    sp.sample_token = lambda logits, seq, cur_len, **k: (seen.append((seq.shape[1], cur_len, k)), real(logits, seq, cur_len, **k))[1]
    try:
        _run(tiny, sample_seed=5, do_sample=True, temperature=0.6, top_k=20, top_p=0.9, min_p=0.02, min_new_tokens=3,
             logits_processor=[RepetitionPenaltyLogitsProcessor(penalty=1.5, prompt_ignore_length=9)])
    finally:
        sp.sample_token = real
    assert sp.stats.delegated == 0
    assert [(a, b) for a, b, _ in seen] == [(4 + t, 4 + t) for t in range(NEW)]
    for t, (_, _, k) in enumerate(seen):
        assert k["step"] == 13 + t and k["seed"] == 5 and k["row0"] == 0 and k["do_sample"] is True
        assert (k["repetition_penalty"], k["temperature"], k["top_k"], k["top_p"], k["min_p"]) == (1.5, 0.6, 20, 0.9, 0.02)
        assert list(k["suppressed"]) == ([2] if t < 3 else [])


def test_return_dict_in_generate(tiny):
    plain = _run(tiny, sample_seed=3, **SAMPLED)
    out = _run(tiny, sample_seed=3, return_dict_in_generate=True, **SAMPLED)
    assert sp.stats.delegated == 0 and torch.equal(out.sequences, plain)
    assert out.scores is None and out.logits is None and out.past_key_values is not None


class _Streamer:
    def __init__(self):
        self.got, self.ended = [], False

    def put(self, value):
        self.got.append(value)

    def end(self):
        self.ended = True


def test_a_streamer_gets_every_token(tiny):
    """generate() of transformers 5.15 does not pass `streamer=` on to a callable custom_generate (it hands
    over only the callable's own keywords), so the streamer is bound to the loop."""
    import functools
    model, ids, mask = tiny
    s = _Streamer()
    sp.stats.reset()
    out = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, sample_seed=3,
                         custom_generate=functools.partial(sp.smt_sample, streamer=s), **SAMPLED)
    assert sp.stats.delegated == 0 and s.ended and len(s.got) == NEW
    assert torch.equal(torch.stack(s.got, dim=1), out[:, 13:]) and torch.equal(out, _run(tiny, sample_seed=3, **SAMPLED))


@pytest.mark.parametrize("kw, reason", [
    ({"no_repeat_ngram_size": 2}, "NoRepeatNGram"), ({"typical_p": 0.5}, "TypicalLogitsWarper"),
    ({"renormalize_logits": True}, "renormalize_logits"),
    ({"return_dict_in_generate": True, "output_scores": True}, "per-step"),
    ({"return_dict_in_generate": True, "output_logits": True}, "per-step"),
    ({"return_dict_in_generate": True, "output_hidden_states": True}, "per-step"),
    ({"return_dict_in_generate": True, "output_attentions": True}, "per-step")], ids=str)
def test_unsupported_cases_delegate(tiny, kw, reason):
    model, ids, mask = tiny
    args = dict(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, **{**SAMPLED, **kw})
    torch.manual_seed(5)
    want = model.generate(**args)
    sp.stats.reset()
    torch.manual_seed(5)
    got = model.generate(custom_generate=sp.smt_sample, **args)
    assert sp.stats.calls == 1 and sp.stats.delegated == 1 and reason in sp.stats.reasons[0]
    if isinstance(want, torch.Tensor):
        assert torch.equal(got, want)
    else:
        assert torch.equal(got.sequences, want.sequences)
        for name in ("scores", "logits"):
            a, b = getattr(want, name), getattr(got, name)
            assert (a is None) == (b is None) and (a is None or all(torch.equal(x, y) for x, y in zip(a, b)))


def test_the_other_reasons(tiny):
    from copy import deepcopy
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    model = tiny[0]
    cfg = model.generation_config
    assert sp._plan(model, [], cfg, True) == "synced_gpus"
    assert "another order" in sp._plan(model, [TopKLogitsWarper(5), TemperatureLogitsWarper(0.5)], cfg, False)
    assert "another order" in sp._plan(model, [TemperatureLogitsWarper(0.5), RepetitionPenaltyLogitsProcessor(1.1)], cfg, False)
    assert "more than one" in sp._plan(model, [RepetitionPenaltyLogitsProcessor(1.1)] * 2, cfg, False)
    assert "min_tokens_to_keep" in sp._plan(model, [TopPLogitsWarper(0.9, min_tokens_to_keep=2)], cfg, False)
    assert "filter_value" in sp._plan(model, [TopKLogitsWarper(5, filter_value=-1e4)], cfg, False)
    enc = deepcopy(model.config)
    enc.is_encoder_decoder = True
    fake = type("M", (), {"config": enc})()
    assert sp._plan(fake, [], cfg, False) == "encoder-decoder model"
    beams = deepcopy(cfg)
    beams.num_beams = 2
    with pytest.raises(ValueError, match="num_beams"):
        sp.smt_sample(model, tiny[1], [], [], beams)


def test_beam_search_still_hands_do_sample_over(tiny):
    model, ids, mask = tiny
    args = dict(input_ids=ids, attention_mask=mask, num_beams=4, max_new_tokens=NEW, do_sample=True, top_k=20)
    torch.manual_seed(5)
    want = model.generate(**args)
    bs.stats.reset()
    sp.stats.reset()
    torch.manual_seed(5)
    got = model.generate(custom_generate=bs.smt_beam_search, **args)
    assert bs.stats.delegated == 1 and bs.stats.reasons == ["do_sample"] and sp.stats.calls == 0
    assert torch.equal(got, want)


def test_wrapper_refuses_bad_arguments():
    x, q = torch.zeros(8, 16), torch.zeros(8, 4, dtype=torch.int64)
    for bad in (lambda: sp.sample_token(x[0], q, 4), lambda: sp.sample_token(x, q, 5), lambda: sp.sample_token(x, q.int(), 4),
                lambda: sp.sample_token(x, q[:7], 4), lambda: sp.sample_token(x, q, -1),
                lambda: sp.sample_token(x, q, 4, repetition_penalty=0.0),
                lambda: sp.sample_token(x, q, 4, repetition_penalty=float("nan")),
                lambda: sp.sample_token(x, q, 4, temperature=0.0), lambda: sp.sample_token(x, q, 4, temperature=math.inf),
                lambda: sp.sample_token(x, q, 4, top_p=0.0), lambda: sp.sample_token(x, q, 4, min_p=1.5),
                lambda: sp.sample_token(x, q, 4, seed=2 ** 64), lambda: sp.sample_token(x, q, 4, seed=-1),
                lambda: sp.sample_token(x, q, 4, step=2 ** 32), lambda: sp.sample_token(x, q, 4, row0=-1),
                lambda: sp.sample_token(x, q, 4, impl="triton")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="impl='hip'"):
        sp.sample_token(x, q, 4, impl="hip")
    many = sp.sample_token(x, q, 4, suppressed=range(9), do_sample=False)          # more than 8 ids: the restatement
    assert many[0].tolist() == [9] * 8 and many[2].tolist() == [16] * 8


def test_c_abi_refusals():
    """Every -1 / -2 of smt_sample_token comes back without a device: the pointers are never dereferenced."""
    lib = _hip.load(build_if_missing=True)
    p, stream = ctypes.c_void_p(4096), None
    sup = (ctypes.c_int64 * 2)(1, 2)
    good = dict(logits=p, ld=512, dtype=_hip.DTYPE_BF16, R=8, V=512, sequences=p, seq_ld=16, cur_len=16, penalty=1.1,
                suppressed=sup, n_suppressed=2, temperature=0.6, top_k=50, top_p=0.95, min_p=0.05, mode=1, seed=7, step=3,
                row0=0, token=p, threshold=p, kept=p, workspace=p)

    def call(**kw):
        a = {**good, **kw}
        return lib.smt_sample_token(a["logits"], a["ld"], a["dtype"], a["R"], a["V"], a["sequences"], a["seq_ld"],
                                    a["cur_len"], a["penalty"], a["suppressed"], a["n_suppressed"], a["temperature"],
                                    a["top_k"], a["top_p"], a["min_p"], a["mode"], a["seed"], a["step"], a["row0"],
                                    a["token"], a["threshold"], a["kept"], a["workspace"], stream)

    invalid = [dict(logits=None), dict(sequences=None), dict(token=None), dict(threshold=None), dict(kept=None),
               dict(workspace=None), dict(R=0), dict(V=0), dict(V=2 ** 31, ld=2 ** 31), dict(ld=511), dict(seq_ld=15),
               dict(cur_len=-1), dict(dtype=7), dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=math.nan),
               dict(n_suppressed=-1), dict(n_suppressed=9), dict(suppressed=None), dict(temperature=0.0),
               dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf), dict(top_p=0.0),
               dict(top_p=math.nan), dict(min_p=1.5), dict(min_p=math.nan), dict(mode=2), dict(mode=-1)]
    for kw in invalid:
        assert call(**kw) == -1, kw
        assert lib.smt_sample_last_error().startswith(b"smt_sample_token: "), kw
    misaligned = [dict(logits=ctypes.c_void_p(4098)), dict(ld=516), dict(dtype=_hip.DTYPE_FP32, ld=514),
                  dict(workspace=ctypes.c_void_p(4104)), dict(sequences=ctypes.c_void_p(4100)),
                  dict(token=ctypes.c_void_p(4098))]
    for kw in misaligned:
        assert call(**kw) == -2, kw
    assert b"aligned" in lib.smt_sample_last_error()
    assert lib.smt_sample_workspace(0, 512) == -1 and lib.smt_sample_workspace(2, 2 ** 31) == -1
    # per row: z and the candidate list, each padded to whole chunks of fp32 / uint32, and a maximum per chunk
    assert lib.smt_sample_workspace(16, 152064) == 16 * 75 * 2048 * 8 + 16 * 75 * 4
    assert lib.smt_sample_workspace(1, 1) == 2048 * 8 + 16
