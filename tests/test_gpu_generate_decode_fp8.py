"""generate() on an fp8 model patched with patch_llama(decode_linears=True, decode_fp8=True): the frozen decoder
linears of every decode step run the e4m3 weight-streaming kernel (smt_linear_skinny_fp8, include/smt_linear.h)
on the model's own w8 / sw, q/k/v as one launch and gate/up/SwiGLU as one; the bf16 LM head keeps the bf16 kernel.

The layout of tests/test_gpu_generate_decode_linears.py (2 left-padded prompts x 4 beams, six teacher-forced
steps, helpers imported from the same files) on a 2-layer LLaMA of hidden 1024, intermediate 2048, Hq 8, Hkv 2,
head_dim 128, vocabulary 512, frozen, with engine.attach_fp8_weights. The yardstick is the same model's bf16
logits before the fp8 copies are attached: the routed logits' relative distance to it may exceed the unrouted
fp8 model's own distance by at most a factor 1.5 (both are fp8 quantisations of the same operands and differ
only in summation order, as the existing test's 1.5 * es)."""
import pytest
import torch

from tests import linear_fp8_ref as fr
from tests.attn_ref import assert_within_bounds
from tests.test_gpu_generate_beams import (NB, NEW, PROMPT, ROWS, STEPS, _inputs, _prefill_and_decode, _rel)
from tests.test_gpu_generate_graph import _generate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAYERS = 2
HIDDEN, INTER = 1024, 2048
# one decode step, per layer: the q/k/v group and the gate/up/SwiGLU launch read the e4m3 copy the fused RMSNorm
# left on their input; o_proj and down_proj quantise theirs (one smt_quant_rows_e4m3 launch each)
PER_STEP = {"single": 2 * LAYERS, "group": LAYERS, "swiglu": LAYERS, "quant": 2 * LAYERS}
HEAD_PER_STEP = {"single": 1, "group": 0, "swiglu": 0}           # the bf16 kernel: the LM head has no fp8 copy


def _times(n, per=PER_STEP):
    return {k: n * v for k, v in per.items()}


def _config():
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS, num_attention_heads=8,
                       num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64,
                       pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="sdpa")


def _frozen_model(seed):
    from transformers import LlamaForCausalLM
    torch.manual_seed(seed)
    model = LlamaForCausalLM(_config()).to(DEV).bfloat16().eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


@pytest.fixture(scope="module")
def run():
    """Everything once: the bf16 logits, then with the fp8 copies attached the unrouted logits, then the routed
    model's teacher-forced runs and generate() calls on the eager device-steps cache and on the graphed one."""
    from sparse_matrix_tuning_amd import engine
    from sparse_matrix_tuning_amd import fused_llama as fl
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    model = _frozen_model(3)
    ids, mask, tokens = _inputs(DEV)
    mk = lambda nb, cap, graph: BeamSharedCache(model.config, nb, cap, device_steps=True, graph=graph)
    r = {}
    with torch.no_grad():
        fl.patch_llama(model)
        try:
            r["bf16"] = _prefill_and_decode(model, mk(NB, STEPS, False), ids, mask, tokens)
        finally:
            fl.unpatch_llama(model)
        assert engine.attach_fp8_weights(model) > 0
        fl.patch_llama(model)
        try:
            r["fp8"] = _prefill_and_decode(model, mk(NB, STEPS, False), ids, mask, tokens)
        finally:
            fl.unpatch_llama(model)
    r["counts"] = fl.patch_llama(model, decode_linears=True, decode_fp8=True)

    def attempt(key, fn):
        fl.decode_fp8_stats.reset()
        fl.decode_linear_stats.reset()
        try:
            with torch.no_grad():
                r[key] = fn()
        except Exception as e:                           # reported by the test that needs it
            r[key] = e
        r[key + "_stats"] = fl.decode_fp8_stats.as_dict()
        r[key + "_bf16_stats"] = fl.decode_linear_stats.as_dict()

    try:
        def prefill_only():
            rows, m = ids.repeat_interleave(NB, 0), mask.repeat_interleave(NB, 0)
            return model(input_ids=rows, attention_mask=m, position_ids=(m.cumsum(-1) - 1).clamp(min=0),
                         past_key_values=mk(NB, STEPS, False), use_cache=True).logits[:, -1].float()
        attempt("prefill", prefill_only)
        for name, graph in (("eager", False), ("graph", True)):
            cache = mk(NB, STEPS, graph)
            r[name + "_cache"] = cache
            attempt(name, lambda: _prefill_and_decode(model, cache, ids, mask, tokens))
        for name, graph in (("eager", False), ("graph", True)):
            cache = mk(NB, NEW, graph)
            r[name + "_gen_cache"] = cache
            attempt(name + "_gen", lambda: _generate(model, cache, ids, mask, NB))
    finally:
        fl.unpatch_llama(model)
    r["left"] = [n for n, m in model.named_modules() if any(k.startswith("_smt_decode") for k in m.__dict__)]
    r["forwards"] = [n for n, m in model.named_modules()
                     if "forward" in m.__dict__ and getattr(m.__dict__["forward"], "__func__", None)
                     is not engine._frozen_linear_forward]
    return r


def _get(run, key):
    if isinstance(run[key], Exception):
        raise run[key]
    return run[key]


def test_teacher_forced_logits(run):
    bf16, fp8, eager, graph = run["bf16"], run["fp8"], _get(run, "eager"), _get(run, "graph")
    assert graph.shape == eager.shape == bf16.shape == (1 + STEPS, ROWS, 512) and torch.isfinite(graph).all()
    for t in range(1 + STEPS):
        print(f"step {t}: routed fp8 rel distance to bf16 {_rel(graph[t], bf16[t]):.3e}, unrouted fp8 {_rel(fp8[t], bf16[t]):.3e}, "
              f"graph == eager: {torch.equal(graph[t], eager[t])}")
    for t in range(1 + STEPS):
        assert torch.equal(graph[t], eager[t]), t
        assert _rel(eager[t], bf16[t]) <= 1.5 * _rel(fp8[t], bf16[t]), t
    assert torch.equal(_get(run, "prefill"), eager[0])
    gc = run["graph_cache"]
    assert gc.graph_captures == 1 and gc.graph_replays == STEPS - 2


def test_the_kernel_ran_in_the_decode_steps_only(run):
    assert run["counts"]["decode_linears"] == 7 * LAYERS + 1
    _get(run, "prefill"), _get(run, "eager"), _get(run, "graph")
    assert run["prefill_stats"] == _times(0) and run["prefill_bf16_stats"] == _times(0, HEAD_PER_STEP)
    assert run["eager_stats"] == _times(STEPS)
    assert run["graph_stats"] == _times(2)                    # the warm-up step and the captured one run Python
    # the bf16 kernel ran for the LM head alone: nothing of it for a weight with an fp8 copy
    assert run["eager_bf16_stats"] == _times(STEPS, HEAD_PER_STEP) and run["graph_bf16_stats"] == _times(2, HEAD_PER_STEP)


def test_generate_returns_the_eager_sequences(run):
    (out, seen), (ref, _) = _get(run, "graph_gen"), _get(run, "eager_gen")
    assert out.shape == (2, PROMPT + NEW) and torch.equal(out, ref)
    cache = run["graph_gen_cache"]
    assert len(seen) == NEW and cache.graph_captures == 1 and cache.graph_replays == NEW - 3
    assert run["eager_gen_stats"] == _times(NEW - 1) and run["graph_gen_stats"] == _times(2)


def test_unpatch_restores_every_forward(run):
    assert run["left"] == []
    assert run["forwards"] == []          # only attach_fp8_weights' own instance forwards remain, as before the patch


@pytest.fixture(scope="module")
def layer_model():
    """A second model whose first layer's q_proj and down_proj are SMT modules with two tiles each (and
    writeback_on_forward, as outside the engine), with fp8 copies, patched with the fp8 routing."""
    from sparse_matrix_tuning_amd import engine
    from sparse_matrix_tuning_amd import fused_llama as fl
    from sparse_matrix_tuning_amd.smt.smt import LinearLayer_MatrixSparsity
    model = _frozen_model(5)
    layer = model.model.layers[0]
    layer.self_attn.q_proj = LinearLayer_MatrixSparsity(layer.self_attn.q_proj.weight, index_list=[(0, 1), (1, 0)])
    layer.mlp.down_proj = LinearLayer_MatrixSparsity(layer.mlp.down_proj.weight, index_list=[(1, 3), (0, 0)])
    engine.attach_fp8_weights(model)
    fl.patch_llama(model, decode_linears=True, decode_fp8=True)
    yield model
    fl.unpatch_llama(model)


@pytest.mark.parametrize("name", ["q_proj", "down_proj"])
def test_smt_modules_still_sync_their_tiles_and_the_kernel_sees_the_current_w8(layer_model, name):
    from sparse_matrix_tuning_amd import fp8 as f8
    from sparse_matrix_tuning_amd import fused_llama as fl
    layer = layer_model.model.layers[0]
    mod = layer.self_attn.q_proj if name == "q_proj" else layer.mlp.down_proj
    fw = mod.weight._smt_fp8
    assert mod.__dict__["forward"].__func__ is fl.decode_routed_linear_forward and mod.writeback_on_forward
    g = torch.Generator().manual_seed(2)
    x = torch.randn(ROWS, 1, mod.weight.shape[1], generator=g).bfloat16().to(DEV)
    fl.decode_fp8_stats.reset()
    fl.decode_linear_stats.reset()
    with torch.no_grad():
        before = mod(x)
        w8_before = fw.w8.clone()
        mod.selected_weight.data.copy_((torch.randn(mod.selected_weight.shape, generator=g) * 0.05).bfloat16())
        after = mod(x)
    # x is quantised once: the second call finds the copy on the tensor
    want = {"single": 0, "group": 2, "swiglu": 0, "quant": 1} if name == "q_proj" else {"single": 2, "group": 0, "swiglu": 0, "quant": 1}
    assert fl.decode_fp8_stats.as_dict() == want and fl.decode_linear_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0}
    assert not torch.equal(before, after)
    r, c = mod.index_list[0]
    assert torch.equal(mod.weight[r * 256:(r + 1) * 256, c * 256:(c + 1) * 256], mod.selected_weight[:256])   # synced
    # ... and re-quantised: w8 / sw are those of the current W, and the result is the product of exactly them
    q_now, s_now = f8.quant_rows(mod.weight.detach())
    assert torch.equal(fw.w8.view(torch.uint8), q_now.view(torch.uint8)) and torch.equal(fw.sw, s_now)
    assert not torch.equal(fw.w8.view(torch.uint8), w8_before.view(torch.uint8))
    x8, sx = f8.quant_rows_cached(x)
    ref, bound = fr.ref64_bound(x8.view(torch.uint8).cpu().numpy(), sx.cpu().numpy(), fw.w8.view(torch.uint8).cpu().numpy(),
                                fw.sw.cpu().numpy(), torch.bfloat16)
    assert_within_bounds(name, after.view(ROWS, -1).cpu(), ref, bound, dims="sd")


def test_calls_that_do_not_qualify_take_the_path_they_took_before(layer_model):
    from sparse_matrix_tuning_amd import engine
    from sparse_matrix_tuning_amd import fused_llama as fl
    attn = layer_model.model.layers[1].self_attn
    g = torch.Generator().manual_seed(9)
    x17 = torch.randn(17, 1, HIDDEN, generator=g).bfloat16().to(DEV)
    x16 = torch.randn(16, 1, HIDDEN, generator=g).bfloat16().to(DEV)
    fl.decode_fp8_stats.reset()
    fl.decode_linear_stats.reset()
    for mod in (attn.q_proj, attn.o_proj):
        with torch.no_grad():
            many = mod(x17)
        with torch.enable_grad():
            graded = mod(x16)
        assert fl.decode_fp8_stats.as_dict() == _times(0) and fl.decode_linear_stats.as_dict() == _times(0, HEAD_PER_STEP)
        assert "_smt_decode_kv" not in x17.__dict__ and "_smt_decode_kv" not in x16.__dict__
        before = engine._frozen_linear_forward               # what attach_fp8_weights gave the module
        with torch.no_grad():
            assert torch.equal(many, before(mod, x17))
        assert torch.equal(graded, before(mod, x16))
    # a weight without an fp8 copy: the LM head goes to the bf16 kernel, as without decode_fp8
    head = layer_model.lm_head
    with torch.no_grad():
        y = head(x16)
        assert fl.decode_fp8_stats.as_dict() == _times(0) and fl.decode_linear_stats.as_dict() == HEAD_PER_STEP
        assert torch.equal(y, fl.decode_linear(x16, head.weight))
