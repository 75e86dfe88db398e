"""smt_beam_search on the device: the bf16 tiny LLaMA of tests/test_gpu_generate_graph.py (hidden 512, 2
layers, Hq 4, Hkv 2, head_dim 128, vocabulary 512; 2 left-padded prompts x 4 beams), patch_llama-ed, with
BeamSharedCache(graph=True), repetition_penalty 1.1 and min_new_tokens (so the eos id is suppressed).

Teacher-forced: one generate() runs the loop on transformers' chain of ops (impl="torch") while every
beam_topk call also runs the kernel on the same logits, scores and history. At every step the fp64
reference's top K + 1 are asserted to be 64 bounds apart (tests/beam_ref.py; SEED is one where they are),
the kernel's indices have to be the reference's and its scores within the bound, and where the reference
has no exact tie the torch chain has to pick the same indices in the same order.

Then generate(custom_generate=smt_beam_search) on the kernel returns the sequences of the same loop with
impl="torch", with replayed decode graphs and nothing delegated.

The three calls capture three graphs in one process, each while the earlier caches are still alive or just
dropped: the collector has to be off inside every capture (fused_llama.DecodeGraph.step)."""
import gc

import pytest
import torch

from tests.beam_ref import check, ref64, ref_topk
from tests.test_gpu_generate_beams import NB, PROMPT, _inputs
from tests.test_gpu_generate_graph import _config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, NEW, PENALTY = 6, 10, 1.1


def generate_both(seed):
    """dict(steps: per beam_topk call the CPU copies of its inputs and of both results, forced / hip / torch:
    generate()'s sequences, *_cache: the caches, stats: (calls, delegated))."""
    from transformers import LlamaForCausalLM
    from sparse_matrix_tuning_amd import beam_search as bs
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import patch_llama, unpatch_llama
    torch.manual_seed(seed)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    ids, mask, _ = _inputs(DEV)
    r, steps, real = {}, [], bs.beam_topk
    captured = []                                       # gc.isenabled() at every layer-0 call inside a capture
    hook = model.model.layers[0].register_forward_pre_hook(
        lambda m, a: captured.append(gc.isenabled()) if torch.cuda.is_current_stream_capturing() else None)

    def both(logits, beam_scores, sequences, cur_len, num_beams, k, repetition_penalty=1.0, suppressed=(), impl=None):
        twin = real(logits, beam_scores, sequences, cur_len, num_beams, k, repetition_penalty, suppressed, impl="torch")
        hip = real(logits, beam_scores, sequences, cur_len, num_beams, k, repetition_penalty, suppressed, impl="hip")
        steps.append(dict(logits=logits.cpu(), beam_scores=beam_scores.reshape(-1).cpu(), sequences=sequences.cpu(),
                          cur_len=cur_len, nb=num_beams, K=k, penalty=repetition_penalty, suppressed=tuple(suppressed),
                          torch=tuple(t.cpu() for t in twin), hip=tuple(t.cpu() for t in hip)))
        return twin

    def generate(name, impl):
        cache = BeamSharedCache(model.config, NB, NEW, graph=True)
        r[name + "_cache"] = cache
        with torch.no_grad():
            r[name] = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, min_new_tokens=NEW,
                                     do_sample=False, num_beams=NB, repetition_penalty=PENALTY, past_key_values=cache,
                                     custom_generate=bs.smt_beam_search, beam_topk_impl=impl)

    patch_llama(model)
    bs.stats.reset()
    try:
        bs.beam_topk = both
        try:
            generate("forced", "torch")
        finally:
            bs.beam_topk = real
        generate("hip", None)
        generate("torch", "torch")
    finally:
        hook.remove()
        unpatch_llama(model)
    r["steps"], r["stats"], r["gc_in_capture"] = steps, (bs.stats.calls, bs.stats.delegated), captured
    return r


@pytest.fixture(scope="module")
def run():
    return generate_both(SEED)


def test_teacher_forced_steps(run):
    steps = run["steps"]
    assert len(steps) == NEW
    for t, s in enumerate(steps):
        assert s["penalty"] == PENALTY and s["suppressed"] == (2,) and s["K"] == 2 * NB and s["cur_len"] == PROMPT + t
        score, bound = ref64(s["logits"], s["beam_scores"], s["sequences"], s["cur_len"], NB, PENALTY, s["suppressed"])
        check(f"step {t}", *s["hip"], score, bound, s["K"])
        top, _, _ = ref_topk(score, bound, s["K"])
        if not (top[:, :-1] == top[:, 1:]).any():
            assert torch.equal(s["torch"][1], s["hip"][1]), t


def test_generate_returns_the_torch_loops_sequences(run):
    assert run["hip"].shape == (2, PROMPT + NEW)
    assert torch.equal(run["hip"], run["torch"]) and torch.equal(run["hip"], run["forced"])
    ids, _, _ = _inputs(DEV)
    assert torch.equal(run["hip"][:, :PROMPT], ids)
    assert run["stats"] == (3, 0)                       # three calls, none delegated
    for name in ("hip", "torch", "forced"):
        cache = run[name + "_cache"]
        assert cache.graph_captures == 1 and cache.graph_replays > 0
    assert run["gc_in_capture"] == [False] * 3 and gc.isenabled()       # off inside each capture, back on after
