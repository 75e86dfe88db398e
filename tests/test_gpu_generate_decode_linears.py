"""generate() on a model patched with patch_llama(decode_linears=True): the dense linears of every decode
step run the weight-streaming kernel (include/smt_linear.h), q/k/v as one launch and gate/up/SwiGLU as one.

Model, inputs and script are those of tests/test_gpu_generate_beams.py and tests/test_gpu_generate_graph.py
(hidden 512, intermediate 1024, 2 layers, Hq 4, Hkv 2, vocabulary 512; 2 left-padded prompts x 4 beams, six
teacher-forced steps), imported from those files. The graphed cache is compared with the eager device-steps
cache on the same routed model: the same kernels with the same launch parameters, so the logits must be
torch.equal at every step and generate() must return the same sequences; both meet the existing bar
against the fp32 twin, relative norm error <= max(8e-3, 1.5 x the sdpa model's)."""
import pytest
import torch

from tests import linear_ref as lr
from tests.attn_ref import assert_within_bounds
from tests.test_gpu_generate_beams import (NB, NEW, PROMPT, ROWS, STEPS, _inputs, _prefill_and_decode, _rel)
from tests.test_gpu_generate_graph import _config, _generate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAYERS = 2
# one decode step: per layer the q/k/v group, o_proj, the gate/up/SwiGLU launch and down_proj; then the head
PER_STEP = {"single": 2 * LAYERS + 1, "group": LAYERS, "swiglu": LAYERS}


def _times(n):
    return {k: n * v for k, v in PER_STEP.items()}


@pytest.fixture(scope="module")
def run():
    """Everything once, as in tests/test_gpu_generate_graph.py, on a model patched with the routing; the
    launch counters are read after each part."""
    from transformers import DynamicCache, LlamaForCausalLM
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd import fused_llama as fl
    torch.manual_seed(3)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    twin = LlamaForCausalLM(_config("eager"))
    twin.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    twin = twin.to(DEV).float().eval()
    ids, mask, tokens = _inputs(DEV)
    r = {"ref": _prefill_and_decode(twin, DynamicCache(config=twin.config), ids, mask, tokens),
         "sdpa": _prefill_and_decode(model, DynamicCache(config=model.config), ids, mask, tokens)}
    del twin
    r["counts"] = fl.patch_llama(model, decode_linears=True)
    mk = lambda nb, cap, graph: BeamSharedCache(model.config, nb, cap, device_steps=True, graph=graph)

    def attempt(key, fn):
        fl.decode_linear_stats.reset()
        try:
            r[key] = fn()
        except Exception as e:                           # reported by the test that needs it
            r[key] = e
        r[key + "_stats"] = fl.decode_linear_stats.as_dict()

    try:
        def prefill_only():
            with torch.no_grad():
                rows, m = ids.repeat_interleave(NB, 0), mask.repeat_interleave(NB, 0)
                return model(input_ids=rows, attention_mask=m, position_ids=(m.cumsum(-1) - 1).clamp(min=0),
                             past_key_values=mk(NB, STEPS, False), use_cache=True).logits[:, -1].float()
        attempt("prefill", prefill_only)
        for name, graph in (("eager", False), ("graph", True)):
            cache = mk(NB, STEPS, graph)
            r[name + "_cache"] = cache
            attempt(name, lambda: _prefill_and_decode(model, cache, ids, mask, tokens))
        for name, graph in (("eager", False), ("graph", True)):
            for nb in (NB, 1):
                cache = mk(nb, NEW, graph)
                r[f"{name}_gen{nb}_cache"] = cache
                attempt(f"{name}_gen{nb}", lambda: _generate(model, cache, ids, mask, nb))
    finally:
        fl.unpatch_llama(model)
    r["left"] = [n for n, m in model.named_modules() if any(k.startswith("_smt_decode") for k in m.__dict__)]
    return r


def _get(run, key):
    if isinstance(run[key], Exception):
        raise run[key]
    return run[key]


def test_teacher_forced_logits(run):
    ref, sdpa, eager, graph = run["ref"], run["sdpa"], _get(run, "eager"), _get(run, "graph")
    assert graph.shape == eager.shape == ref.shape == (1 + STEPS, ROWS, 512) and torch.isfinite(graph).all()
    for t in range(1 + STEPS):
        print(f"step {t}: graph rel err {_rel(graph[t], ref[t]):.3e}, eager device-steps {_rel(eager[t], ref[t]):.3e}, "
              f"sdpa {_rel(sdpa[t], ref[t]):.3e}, graph == eager: {torch.equal(graph[t], eager[t])}")
    for t in range(1 + STEPS):
        assert torch.equal(graph[t], eager[t]), t
        es = _rel(sdpa[t], ref[t])
        assert _rel(graph[t], ref[t]) <= max(8e-3, 1.5 * es), t
        assert _rel(eager[t], ref[t]) <= max(8e-3, 1.5 * es), t
    assert torch.equal(_get(run, "prefill"), eager[0])
    gc = run["graph_cache"]
    assert gc.graph_captures == 1 and gc.graph_replays == STEPS - 2


def test_the_kernel_ran_in_the_decode_steps_only(run):
    assert run["counts"]["decode_linears"] == 7 * LAYERS + 1
    _get(run, "prefill"), _get(run, "eager"), _get(run, "graph")
    assert run["prefill_stats"] == _times(0)                  # 8 x 13 rows: nothing qualifies
    assert run["eager_stats"] == _times(STEPS)
    assert run["graph_stats"] == _times(2)                    # the warm-up step and the captured one run Python
    assert run["left"] == []


def test_generate_returns_the_eager_sequences(run):
    for nb in (NB, 1):                                        # num_beams = 1: two rows, M = 2
        (out, seen), (ref, _) = _get(run, f"graph_gen{nb}"), _get(run, f"eager_gen{nb}")
        assert out.shape == (2, PROMPT + NEW) and torch.equal(out, ref)
        cache = run[f"graph_gen{nb}_cache"]
        assert len(seen) == NEW and cache.graph_captures == 1 and cache.graph_replays == NEW - 3
        assert run[f"eager_gen{nb}_stats"] == _times(NEW - 1)
        assert run[f"graph_gen{nb}_stats"] == _times(2)


@pytest.fixture(scope="module")
def layer_model():
    """A second model of the same config whose first layer's q_proj and down_proj are SMT modules with two
    tiles each, patched with the routing."""
    from transformers import LlamaForCausalLM
    from sparse_matrix_tuning_amd import fused_llama as fl
    from sparse_matrix_tuning_amd.smt.smt import LinearLayer_MatrixSparsity
    torch.manual_seed(5)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    layer = model.model.layers[0]
    layer.self_attn.q_proj = LinearLayer_MatrixSparsity(layer.self_attn.q_proj.weight, index_list=[(0, 1), (1, 0)])
    layer.mlp.down_proj = LinearLayer_MatrixSparsity(layer.mlp.down_proj.weight, index_list=[(1, 3), (0, 0)])
    fl.patch_llama(model, decode_linears=True)
    yield model
    fl.unpatch_llama(model)


@pytest.mark.parametrize("name", ["q_proj", "down_proj"])
def test_smt_modules_still_sync_their_tiles(layer_model, name):
    from sparse_matrix_tuning_amd import fused_llama as fl
    layer = layer_model.model.layers[0]
    mod = layer.self_attn.q_proj if name == "q_proj" else layer.mlp.down_proj
    assert mod.__dict__["forward"].__func__ is fl.decode_routed_linear_forward and mod.writeback_on_forward
    g = torch.Generator().manual_seed(2)
    x = torch.randn(ROWS, 1, mod.weight.shape[1], generator=g).bfloat16().to(DEV)
    fl.decode_linear_stats.reset()
    with torch.no_grad():
        before = mod(x)
        mod.selected_weight.data.copy_(torch.randn(mod.selected_weight.shape, generator=g).bfloat16())
        after = mod(x)
    stats = fl.decode_linear_stats.as_dict()
    assert stats == ({"single": 0, "group": 2, "swiglu": 0} if name == "q_proj" else {"single": 2, "group": 0, "swiglu": 0})
    assert not torch.equal(before, after)
    r, c = mod.index_list[0]
    assert torch.equal(mod.weight[r * 256:(r + 1) * 256, c * 256:(c + 1) * 256], mod.selected_weight[:256])   # synced
    ref, bound = lr.ref64_bound(x.view(ROWS, -1).cpu(), mod.weight.detach().cpu())
    assert_within_bounds(name, after.view(ROWS, -1).cpu(), ref, bound, dims="sd")


def test_calls_that_do_not_qualify_take_the_unrouted_path(layer_model):
    from sparse_matrix_tuning_amd import fused_llama as fl
    attn = layer_model.model.layers[1].self_attn
    g = torch.Generator().manual_seed(9)
    x17 = torch.randn(17, 1, 512, generator=g).bfloat16().to(DEV)
    x16 = torch.randn(16, 1, 512, generator=g).bfloat16().to(DEV)
    fl.decode_linear_stats.reset()
    for mod in (attn.q_proj, attn.o_proj):
        with torch.no_grad():
            many = mod(x17)
        with torch.enable_grad():
            graded = mod(x16)
        assert fl.decode_linear_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0}
        assert "_smt_decode_kv" not in x17.__dict__ and "_smt_decode_kv" not in x16.__dict__
        unrouted = torch.nn.Linear.forward
        with torch.no_grad():
            assert torch.equal(many, unrouted(mod, x17))
        assert torch.equal(graded, unrouted(mod, x16))
