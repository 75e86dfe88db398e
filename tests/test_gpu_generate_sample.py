"""smt_sample on the device: bf16 tiny LLaMA (tests/test_gpu_generate_graph.py's config) and Qwen2
(tests/test_gpu_qwen2.py's model "a") models under patch_model, 2 left-padded prompts, with a DynamicCache and
with BeamSharedCache(config, 1, NEW, graph=True).

Sampled (temperature 0.6, top-k 8, top-p 0.9, repetition penalty 1.1, min_new_tokens 3): the loop on the
kernel returns the tokens of the same loop on the torch restatement of the contract. Every sample_token call
of the restatement's run is recorded, and the reference of tests/sample_ref.py has to be at least 64 bounds
separated on each of them (the seeds are ones where it is): there the contract leaves one answer. Greedy:
the loop on the kernel returns transformers' own greedy generate(). Nothing is delegated."""
import pytest
import torch

from tests import sample_ref as ref
from tests.test_gpu_generate_beams import PROMPT, _inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEW, SEED = 10, 2024
SAMPLED = dict(do_sample=True, temperature=0.6, top_k=8, top_p=0.9, repetition_penalty=1.1, min_new_tokens=3)


def _model(family):
    torch.manual_seed(4)
    if family == "llama":
        from transformers import LlamaForCausalLM
        from tests.test_gpu_generate_graph import _config
        return LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    from transformers import Qwen2ForCausalLM
    from tests.test_gpu_qwen2 import _config
    return Qwen2ForCausalLM(_config("a", "sdpa")).to(DEV).bfloat16().eval()


@pytest.fixture(scope="module", params=["llama", "qwen2"])
def run(request):
    """Per cache kind: the sampled sequences on the kernel and on the restatement, the restatement's recorded
    calls, the greedy sequences of the loop and of transformers, and the loop's counters."""
    from transformers import DynamicCache
    from sparse_matrix_tuning_amd import sampling as sp
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import patch_model, unpatch_model
    model = _model(request.param)
    ids, mask, _ = _inputs(DEV)
    caches = {"dynamic": lambda: DynamicCache(config=model.config),
              "graph": lambda: BeamSharedCache(model.config, 1, NEW, graph=True)}
    r, real = {}, sp.sample_token

    def generate(cache, **kw):
        with torch.no_grad():
            return model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, past_key_values=cache, **kw)

    patch_model(model)
    sp.stats.reset()
    try:
        for kind, mk in caches.items():
            calls = []

            def recording(logits, sequences, cur_len, **kw):
                calls.append(dict(logits=logits.cpu(), sequences=sequences.cpu(), cur_len=cur_len, kw=dict(kw)))
                return real(logits, sequences, cur_len, **kw)

            sp.sample_token = recording
            try:
                twin = generate(mk(), custom_generate=sp.smt_sample, sample_seed=SEED, sample_impl="torch", **SAMPLED)
            finally:
                sp.sample_token = real
            cache = mk()
            hip = generate(cache, custom_generate=sp.smt_sample, sample_seed=SEED, sample_impl="hip", **SAMPLED)
            greedy = generate(mk(), custom_generate=sp.smt_sample, sample_impl="hip", do_sample=False, repetition_penalty=1.1)
            theirs = generate(mk(), do_sample=False, repetition_penalty=1.1)
            r[kind] = dict(twin=twin.cpu(), hip=hip.cpu(), calls=calls, greedy=greedy.cpu(), theirs=theirs.cpu(), cache=cache)
    finally:
        unpatch_model(model)
    r["stats"] = (sp.stats.calls, sp.stats.delegated)
    return r


@pytest.mark.parametrize("kind", ["dynamic", "graph"])
def test_every_step_of_the_restatements_run_is_separated(run, kind):
    calls = run[kind]["calls"]
    assert len(calls) == NEW
    for t, c in enumerate(calls):
        kw = c["kw"]
        assert kw["step"] == PROMPT + t == c["cur_len"] and kw["seed"] == SEED and kw["impl"] == "torch"
        assert list(kw["suppressed"]) == ([2] if t < 3 else [])
        case = dict(logits=c["logits"], sequences=c["sequences"], cur_len=c["cur_len"], penalty=kw["repetition_penalty"],
                    suppressed=kw["suppressed"], temperature=kw["temperature"], top_k=kw["top_k"], top_p=kw["top_p"],
                    min_p=kw["min_p"])
        want = ref.reference(case, seed=SEED, step=kw["step"], row0=0)
        print(f"{kind} step {t}: separation {want['separation']:.0f} bounds, kept {want['kept'].tolist()}")
        assert want["separation"] >= 64, (kind, t, want["separation"])
        assert torch.equal(run[kind]["twin"][:, PROMPT + t], want["drawn"]), (kind, t)


@pytest.mark.parametrize("kind", ["dynamic", "graph"])
def test_the_kernels_tokens_are_the_restatements(run, kind):
    r = run[kind]
    assert r["hip"].shape == (2, PROMPT + NEW) and torch.equal(r["hip"], r["twin"])
    assert not torch.equal(r["hip"], r["greedy"])                       # it did sample


@pytest.mark.parametrize("kind", ["dynamic", "graph"])
def test_greedy_is_transformers_greedy(run, kind):
    assert torch.equal(run[kind]["greedy"], run[kind]["theirs"])


def test_nothing_is_delegated_and_the_graph_replays(run):
    assert run["stats"] == (6, 0)                                       # three loop calls per cache kind
    cache = run["graph"]["cache"]
    assert cache.graph_captures == 1 and cache.graph_replays > 0
