"""Graph-replayed decode steps: a patch_llama-ed model with BeamSharedCache(graph=True) captures the
decode forward once per generate() call (the second decode step; the first runs eagerly as the
warm-up) and replays it for the remaining tokens.

Model, inputs and script are those of tests/test_gpu_generate_beams.py (its config repeated here:
hidden 512, 2 layers, Hq 4, Hkv 2, head_dim 128, vocabulary 512; 2 left-padded prompts x 4 beams, six
teacher-forced steps with a scripted beam_idx after every forward), with the fp32 eager twin and the
bf16 sdpa model run before patching.

The graphed run is compared with the eager run on the same device-steps path
(device_steps=True, graph=False): the same kernels with the same launch parameters, so the logits are
required to be torch.equal at the prefill and at every step, and generate() to return the same
sequences. Both runs also meet the bar of tests/test_gpu_generate.py against the twin: relative norm
error <= max(8e-3, 1.5 x the sdpa model's error)."""
import pytest
import torch

from tests.test_gpu_generate_beams import (NB, NEW, PROMPT, ROWS, STEPS, _inputs, _prefill_and_decode, _rel)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _config(attn, **kw):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                       num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64,
                       pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation=attn, **kw)


def _generate(model, cache, ids, mask, num_beams):
    """generate() with ``cache``: (the sequences, per forward the generated buffers' addresses or None)."""
    seen = []
    hook = model.register_forward_pre_hook(lambda m, a: seen.append(
        tuple((ly.k_gen.data_ptr(), ly.v_gen.data_ptr()) for ly in cache.layers)
        if cache.layers[0].is_initialized else None))
    try:
        with torch.no_grad():
            out = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, min_new_tokens=NEW,
                                 do_sample=False, num_beams=num_beams, past_key_values=cache)
    finally:
        hook.remove()
    return out, seen


@pytest.fixture(scope="module")
def run():
    """Everything once: the twin's and the sdpa model's teacher-forced runs, then on the patched model the
    teacher-forced runs and generate() calls with the eager device-steps cache and with the graphed one.
    A failure of a later part is kept for the test that needs it."""
    from transformers import DynamicCache, LlamaForCausalLM
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import patch_llama, unpatch_llama
    torch.manual_seed(3)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    twin = LlamaForCausalLM(_config("eager"))
    twin.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    twin = twin.to(DEV).float().eval()
    ids, mask, tokens = _inputs(DEV)
    r = {"ref": _prefill_and_decode(twin, DynamicCache(config=twin.config), ids, mask, tokens),
         "sdpa": _prefill_and_decode(model, DynamicCache(config=model.config), ids, mask, tokens)}
    del twin
    patch_llama(model)
    mk = lambda nb, cap, graph: BeamSharedCache(model.config, nb, cap, device_steps=True, graph=graph)

    def attempt(key, fn):
        try:
            r[key] = fn()
        except Exception as e:                           # reported by the test that needs it
            r[key] = e

    try:
        for name, graph in (("eager", False), ("graph", True)):
            cache = mk(NB, STEPS, graph)
            r[name + "_cache"] = cache
            attempt(name, lambda: _prefill_and_decode(model, cache, ids, mask, tokens))
        for name, graph in (("eager", False), ("graph", True)):
            for nb in (NB, 1):
                cache = mk(nb, NEW, graph)
                r[f"{name}_gen{nb}_cache"] = cache
                attempt(f"{name}_gen{nb}", lambda: _generate(model, cache, ids, mask, nb))
        again = mk(NB, NEW, True)                        # the same model, a fresh cache: a capture of its own
        r["again_cache"] = again
        attempt("again", lambda: _generate(model, again, ids, mask, NB))

        def with_labels():
            with torch.no_grad():
                return model(input_ids=ids, attention_mask=mask, labels=ids.masked_fill(mask == 0, -100))
        attempt("labels", with_labels)
    finally:
        unpatch_llama(model)
    return r


def _get(run, key):
    if isinstance(run[key], Exception):
        raise run[key]
    return run[key]


def test_teacher_forced_logits_equal_the_eager_device_steps_run(run):
    ref, sdpa, eager, graph = run["ref"], run["sdpa"], _get(run, "eager"), _get(run, "graph")
    assert graph.shape == eager.shape == ref.shape == (1 + STEPS, ROWS, 512) and torch.isfinite(graph).all()
    for t in range(1 + STEPS):
        eg, ee, es = _rel(graph[t], ref[t]), _rel(eager[t], ref[t]), _rel(sdpa[t], ref[t])
        print(f"step {t}: graph rel err {eg:.3e}, eager device-steps {ee:.3e}, sdpa {es:.3e}, "
              f"graph == eager: {torch.equal(graph[t], eager[t])}")
    for t in range(1 + STEPS):
        assert torch.equal(graph[t], eager[t]), t
        es = _rel(sdpa[t], ref[t])
        assert _rel(graph[t], ref[t]) <= max(8e-3, 1.5 * es), t
        assert _rel(eager[t], ref[t]) <= max(8e-3, 1.5 * es), t
    # six decode steps: one eager, one captured, four replayed
    gc, ec = run["graph_cache"], run["eager_cache"]
    assert gc.graph_captures == 1 and gc.graph_replays == 4
    assert ec.graph_captures == 0 and ec.graph_replays == 0 and ec.decode_runner is None
    for c in (gc, ec):
        assert c.ancestry_updates == 1 + STEPS and all(ly.steps == STEPS for ly in c.layers)
        assert int(c.steps_tensor) == STEPS
    assert torch.equal(gc.ancestors, ec.ancestors)
    for a, b in zip(gc.layers, ec.layers):
        assert torch.equal(a.k_gen, b.k_gen) and torch.equal(a.v_gen, b.v_gen)


def test_generate_returns_the_eager_sequences(run):
    (out, seen), (ref, _) = _get(run, f"graph_gen{NB}"), _get(run, f"eager_gen{NB}")
    assert out.shape == (2, PROMPT + NEW) and torch.equal(out, ref)
    ids, _, _ = _inputs(DEV)
    assert torch.equal(out[:, :PROMPT], ids)
    cache = run[f"graph_gen{NB}_cache"]
    # one prefill, then NEW - 1 decode forwards on buffers that never move: one eager, one captured, the rest replayed
    assert len(seen) == NEW and seen[0] is None and len(set(seen[1:])) == 1
    assert seen[1] == tuple((ly.k_gen.data_ptr(), ly.v_gen.data_ptr()) for ly in cache.layers)
    assert cache.graph_captures == 1 and cache.graph_replays == NEW - 3
    assert all(ly.steps == NEW - 1 for ly in cache.layers) and int(cache.steps_tensor) == NEW - 1
    assert cache.ancestry_updates == len(seen)
    assert int(cache.ancestors.max()) < NB


def test_the_same_model_afterwards(run):
    """Greedy decoding is num_beams = 1 with the same cache; a second generate() with a fresh cache
    captures once more and returns the same sequences; a forward with labels still returns the fused loss."""
    (out, _), (ref, _) = _get(run, "graph_gen1"), _get(run, "eager_gen1")
    assert out.shape == (2, PROMPT + NEW) and torch.equal(out, ref)
    c1 = run["graph_gen1_cache"]
    assert c1.graph_captures == 1 and c1.graph_replays == NEW - 3
    out2, seen2 = _get(run, "again")
    assert torch.equal(out2, _get(run, f"graph_gen{NB}")[0])
    again = run["again_cache"]
    assert again.graph_captures == 1 and again.graph_replays == NEW - 3 and len(seen2) == NEW
    assert again.decode_runner is not run[f"graph_gen{NB}_cache"].decode_runner
    labelled = _get(run, "labels")
    assert labelled.logits is None and torch.isfinite(labelled.loss) and 0 < labelled.loss.item() < 20


def test_dynamic_rope_is_refused():
    from transformers import LlamaForCausalLM
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import patch_llama, unpatch_llama
    torch.manual_seed(4)
    cfg = _config("sdpa", rope_parameters={"rope_type": "dynamic", "factor": 2.0, "rope_theta": 10000.0})
    model = LlamaForCausalLM(cfg).to(DEV).bfloat16().eval()
    ids, mask, tokens = _inputs(DEV)
    ids, mask = ids.repeat_interleave(NB, 0), mask.repeat_interleave(NB, 0)
    patch_llama(model)
    try:
        cache = BeamSharedCache(model.config, NB, 4, graph=True)
        with torch.no_grad():
            model(input_ids=ids, attention_mask=mask, position_ids=(mask.cumsum(-1) - 1).clamp(min=0),
                  past_key_values=cache, use_cache=True)
            mask = torch.cat([mask, mask.new_ones(ROWS, 1)], dim=1)
            with pytest.raises(NotImplementedError, match="dynamic"):
                model(input_ids=tokens[0][:, None], attention_mask=mask, position_ids=mask.sum(-1, keepdim=True) - 1,
                      past_key_values=cache, use_cache=True)
        assert cache.graph_captures == 0 and all(ly.steps == 0 for ly in cache.layers)
    finally:
        unpatch_llama(model)
