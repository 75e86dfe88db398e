"""Qwen2 models on the fused path (patch_model): training parity, decode parity with the routed decode linears and
their bias epilogue, and the attention kernels at the Qwen2 head groups G = 6 and G = 7.

Models: tiny Qwen2ForCausalLM, 2 layers, intermediate 1024, vocabulary 512, head_dim 128:
  (a) hidden 1536, Hq 12, Hkv 2: the 1.5B distill's attention geometry, G = 6, the register path of the fused norm
      (1536 % 512 == 0), with tie_word_embeddings off and on;
  (b) hidden 1792, Hq 14, Hkv 2: G = 7 as in the 7B, the general norm path.

The bar is the project's existing relation: the patched model's error against an fp32 eager twin with the same
weights is at most max(8e-3, 1.5 x the unpatched bf16 sdpa model's error against that twin).

The decode part is the script of tests/test_gpu_generate_decode_linears.py (2 left-padded prompts x 4 beams, six
teacher-forced steps, then generate()), whose helpers are imported; only the model construction is new.

At kernel level, what no existing test covers: tests/test_gpu_attention_bounds.py runs the training kernels at
G in {1, 2, 8}, the cached kernel at G in {1, 4, 8} and the beam kernel at G = 4, nb = 3 (12 columns); no group
that is not a power of two. Here: forward + backward at
S = 130, flash_attention_cached at Sq 1 and 3 against 70 keys, and flash_attention_beams at nb = 4 (24 and 28
of the 32 columns of a block), each at G = 6 and 7 against the per-element bounds of tests/attn_ref.py."""
import pytest
import torch

from tests.attn_ref import D, allowed_cached, allowed_causal, check_outputs, inputs, ref64_bounds
from tests.test_gpu_generate_beams import NB, NEW, PROMPT, ROWS, STEPS, _inputs, _prefill_and_decode, _rel
from tests.test_gpu_generate_graph import _generate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAYERS = 2
MODELS = {"a": dict(hidden_size=1536, num_attention_heads=12), "a_tied": dict(hidden_size=1536, num_attention_heads=12,
                                                                              tie_word_embeddings=True),
          "b": dict(hidden_size=1792, num_attention_heads=14)}
# one decode step: per layer the q/k/v group (with its three biases: one biased launch), o_proj, the
# gate/up/SwiGLU launch and down_proj; then the head
PER_STEP = {"single": 2 * LAYERS + 1, "group": LAYERS, "swiglu": LAYERS, "bias": LAYERS}


def _times(n):
    return {k: n * v for k, v in PER_STEP.items()}


def _stats(fl):
    return dict(fl.decode_linear_stats.as_dict(), bias=fl.decode_linear_stats.bias)


def _config(name, attn):
    from transformers import Qwen2Config
    kw = dict(tie_word_embeddings=False)
    kw.update(MODELS[name])
    return Qwen2Config(intermediate_size=1024, num_hidden_layers=LAYERS, num_key_value_heads=2, vocab_size=512,
                       max_position_embeddings=128, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                       attn_implementation=attn, **kw)


def _models(name, seed):
    """(the bf16 sdpa model, its fp32 eager twin) with the same weights and biases that are not zero."""
    from transformers import Qwen2ForCausalLM
    torch.manual_seed(seed)
    model = Qwen2ForCausalLM(_config(name, "sdpa"))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("_proj.bias"):                      # transformers initialises them to zero
                p.normal_(0.0, 0.5)
    model = model.to(DEV).bfloat16()
    twin = Qwen2ForCausalLM(_config(name, "eager"))
    twin.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    return model, twin.to(DEV).float()


# ---- training parity ---------------------------------------------------------------------------------------------
WATCHED = ("model.embed_tokens.weight", "model.layers.0.self_attn.q_proj.weight", "model.layers.0.self_attn.q_proj.bias",
           "model.layers.1.mlp.down_proj.weight")


def _train_step(model, ids, mask, labels):
    model.zero_grad(set_to_none=True)
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    out.loss.backward()
    params = dict(model.named_parameters())
    return out.loss.detach().double().item(), {n: params[n].grad.detach().float().clone() for n in WATCHED}


@pytest.fixture(scope="module", params=list(MODELS))
def trained(request):
    from sparse_matrix_tuning_amd import fused_llama as fl
    name = request.param
    model, twin = _models(name, seed=11)
    model.train()
    twin.train()
    g = torch.Generator().manual_seed(4)
    B, S = 2, 96
    ids = torch.randint(3, 512, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[1, 71:] = 0                                           # a padded batch
    ids[1, 71:] = 0
    labels = torch.where(mask.bool(), ids, torch.full_like(ids, -100))
    ids, mask, labels = ids.to(DEV), mask.to(DEV), labels.to(DEV)
    r = {"name": name, "ref": _train_step(twin, ids, mask, labels), "sdpa": _train_step(model, ids, mask, labels)}
    del twin
    with torch.no_grad():
        r["logits_before"] = model(input_ids=ids, attention_mask=mask).logits.clone()
    r["counts"] = fl.patch_model(model)
    try:
        r["smt"] = _train_step(model, ids, mask, labels)
    finally:
        fl.unpatch_model(model)
    with torch.no_grad():
        r["logits_after"] = model(input_ids=ids, attention_mask=mask).logits
    r["left"] = [n for n, m in model.named_modules() if "forward" in m.__dict__ or any(k.startswith("_smt_") for k in m.__dict__)]
    return r


def test_training_step_matches_the_fp32_twin(trained):
    (loss_ref, g_ref), (loss_sdpa, g_sdpa), (loss_smt, g_smt) = trained["ref"], trained["sdpa"], trained["smt"]
    e, es = abs(loss_smt - loss_ref) / abs(loss_ref), abs(loss_sdpa - loss_ref) / abs(loss_ref)
    print(f"{trained['name']} loss: ref {loss_ref:.6f}, patched rel err {e:.3e}, sdpa {es:.3e}")
    rows = [("loss", e, es)]
    for n in WATCHED:
        rows.append((n, _rel(g_smt[n], g_ref[n]), _rel(g_sdpa[n], g_ref[n])))
        print(f"{trained['name']} grad {n}: patched rel err {rows[-1][1]:.3e}, sdpa {rows[-1][2]:.3e}")
        assert g_ref[n].abs().max() > 0
    for what, e, es in rows:
        assert e <= max(8e-3, 1.5 * es), (what, e, es)


def test_every_kind_was_patched_and_unpatch_restores_the_model(trained):
    counts = trained["counts"]
    assert counts == {"rmsnorm": 2 * LAYERS + 1, "mlp": LAYERS, "rope": 1, "attention": LAYERS, "loss": 1,
                      "decoder": LAYERS, "lm_head_loss": 1}
    assert trained["left"] == []
    assert torch.equal(trained["logits_before"], trained["logits_after"])


# ---- decode parity -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(MODELS))
def run(request):
    """Everything once, as in tests/test_gpu_generate_decode_linears.py, on a Qwen2 model under
    patch_model(decode_linears=True); the launch counters are read after each part."""
    from transformers import DynamicCache
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd import fused_llama as fl
    model, twin = _models(request.param, seed=3)
    model.eval()
    twin.eval()
    ids, mask, tokens = _inputs(DEV)
    r = {"ref": _prefill_and_decode(twin, DynamicCache(config=twin.config), ids, mask, tokens),
         "sdpa": _prefill_and_decode(model, DynamicCache(config=model.config), ids, mask, tokens)}
    del twin
    r["counts"] = fl.patch_model(model, decode_linears=True)
    mk = lambda nb, cap, graph: BeamSharedCache(model.config, nb, cap, device_steps=True, graph=graph)

    def attempt(key, fn):
        fl.decode_linear_stats.reset()
        try:
            r[key] = fn()
        except Exception as e:                           # reported by the test that needs it
            r[key] = e
        r[key + "_stats"] = _stats(fl)

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
        try:                                             # the same steps with the bias routing off
            fl.DECODE_LINEAR_BIAS = False
            attempt("nobias", lambda: _prefill_and_decode(model, mk(NB, STEPS, False), ids, mask, tokens))
        finally:
            fl.DECODE_LINEAR_BIAS = True
    finally:
        fl.unpatch_model(model)
    r["left"] = [n for n, m in model.named_modules() if any(k.startswith("_smt_") for k in m.__dict__)]
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
    gc = run["graph_cache"]
    assert gc.graph_captures == 1 and gc.graph_replays == STEPS - 2


def test_the_kernel_ran_in_the_decode_steps_with_one_biased_launch_per_group(run):
    assert run["counts"]["decode_linears"] == 7 * LAYERS + 1
    assert all(v > 0 for v in run["counts"].values()), run["counts"]
    _get(run, "eager"), _get(run, "graph"), _get(run, "nobias")
    assert run["eager_stats"] == _times(STEPS)
    assert run["graph_stats"] == _times(2)                    # the warm-up step and the captured one run Python
    # bias routing off: q, k and v run what they ran before, everything else is routed as it was
    assert run["nobias_stats"] == {"single": STEPS * (2 * LAYERS + 1), "group": 0, "swiglu": STEPS * LAYERS, "bias": 0}
    ref, sdpa, nobias = run["ref"], run["sdpa"], run["nobias"]
    for t in range(1 + STEPS):
        assert _rel(nobias[t], ref[t]) <= max(8e-3, 1.5 * _rel(sdpa[t], ref[t])), t
    assert run["left"] == []


def test_generate_returns_the_eager_sequences(run):
    for nb in (NB, 1):                                        # num_beams = 1: two rows, M = 2
        (out, seen), (ref, _) = _get(run, f"graph_gen{nb}"), _get(run, f"eager_gen{nb}")
        assert out.shape == (2, PROMPT + NEW) and torch.equal(out, ref)
        cache = run[f"graph_gen{nb}_cache"]
        assert len(seen) == NEW and cache.graph_captures == 1 and cache.graph_replays == NEW - 3
        assert run[f"eager_gen{nb}_stats"] == _times(NEW - 1)
        assert run[f"graph_gen{nb}_stats"] == _times(2)


def test_a_biased_mlp_keeps_its_biases_and_patch_llama_keeps_f_linear():
    """LlamaConfig(attention_bias=True, mlp_bias=True): the gate/up/SwiGLU launch has no biased form, so a decode
    step's MLP must run the unfused path with its biases under either patch; q_proj's bias goes through the
    epilogue under patch_model and through F.linear, as before, under patch_llama."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from sparse_matrix_tuning_amd import fused_llama as fl
    torch.manual_seed(21)
    cfg = LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, vocab_size=512, attention_bias=True, mlp_bias=True,
                      attn_implementation="sdpa")
    model = LlamaForCausalLM(cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("_proj.bias"):
                p.normal_(0.0, 1.0)
    model = model.to(DEV).bfloat16().eval()
    layer = model.model.layers[0]
    x = torch.randn(4, 1, 512, device=DEV).bfloat16()
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
    with torch.no_grad():
        mlp_want, q_want = layer.mlp(x), layer.self_attn.q_proj(x)
        g, u, d = layer.mlp.gate_proj, layer.mlp.up_proj, layer.mlp.down_proj
        dropped = d(torch.nn.functional.silu(torch.nn.functional.linear(x, g.weight)) * torch.nn.functional.linear(x, u.weight))
        assert rel(dropped, mlp_want) > 0.3                                            # the biases matter here
        for patch, unpatch, biased in ((fl.patch_llama, fl.unpatch_llama, 0), (fl.patch_model, fl.unpatch_model, 1)):
            patch(model, decode_linears=True)
            try:
                fl.decode_linear_stats.reset()
                mlp_got = layer.mlp(x)
                assert fl.decode_linear_stats.swiglu == 0 and fl.decode_linear_stats.group == 0
                assert rel(mlp_got, mlp_want) < 2e-2, (patch.__name__, rel(mlp_got, mlp_want))
                fl.decode_linear_stats.reset()
                q_got = layer.self_attn.q_proj(x)
                assert (fl.decode_linear_stats.group, fl.decode_linear_stats.bias) == (biased, biased)
                assert rel(q_got, q_want) < 1e-2
                if not biased:
                    assert torch.equal(q_got, q_want)
            finally:
                unpatch(model)


# ---- the attention kernels at G = 6 and G = 7 --------------------------------------------------------------------
SCALE = D ** -0.5
HKV = 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("G", [6, 7])
def test_training_kernels_at_the_qwen2_groups(G, dtype):
    from sparse_matrix_tuning_amd.fused_llama import flash_attention
    B, S = 2, 130
    q, k, v, g = inputs(B, HKV * G, HKV, S, "hf", dtype, 7 * S + G)
    o = flash_attention(q, k, v, any_length=True)
    lse = o.grad_fn.saved_tensors[4][:, :, :S].clone()
    o.backward(g)
    R = ref64_bounds(q, k, v, g, SCALE, allowed_causal(S))
    check_outputs(f"train G{G} S{S} {str(dtype)[6:]}", {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "lse2": lse}, R)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("G", [6, 7])
@pytest.mark.parametrize("Sq", [1, 3])
def test_cached_kernel_at_the_qwen2_groups(Sq, G, dtype):
    from sparse_matrix_tuning_amd.fused_llama import KeyMask, flash_attention_cached
    B, Skv = 2, 70
    torch.manual_seed(1000 * Skv + 10 * Sq + G)
    mk = lambda H, S: torch.randn(B, S, H, D, device=DEV).to(dtype).transpose(1, 2)
    q, k, v = mk(HKV * G, Sq), mk(HKV, Skv), mk(HKV, Skv)
    keep = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
    keep[0, :9] = False                                       # a left-padded row, and a hole
    keep[1, 40] = False
    for masked in (False, True):
        R = ref64_bounds(q, k, v, None, SCALE, allowed_cached(B, Sq, Skv, Skv - Sq, keep if masked else None))
        km = KeyMask.from_padding_mask(keep) if masked else None
        for ns in (1, 2):
            o, lse = flash_attention_cached(q, k, v, key_mask=km, num_splits=ns, return_lse=True)
            check_outputs(f"cached Sq{Sq} G{G} {str(dtype)[6:]} mask {masked} splits {ns}", {"o": o, "lse2": lse}, R)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("G", [6, 7])
def test_beam_kernel_at_the_qwen2_groups(G, dtype):
    """nb = 4: 4 G = 24 and 28 columns of the 32-column block."""
    from sparse_matrix_tuning_amd.fused_llama import KeyMask, flash_attention_beams
    from tests.test_gpu_attention_beams import N, _case as beam_case, _gather, _keep as beam_keep
    nb, P, T = 4, 70, 5
    q, kp, vp, kg, vg, anc = beam_case(HKV * G, HKV, nb, P, T, dtype=dtype)
    k, v = _gather(kp, vp, kg, vg, anc, nb, P, T)
    pk = torch.ones(N, P, dtype=torch.bool, device=DEV)
    pk[1, :9] = False
    pk[0, 40] = False
    tiles = -(-P // 64) + nb * -(-T // 64)
    for prompt_keep in (None, pk):
        keep = beam_keep(anc, nb, P, T, prompt_keep)
        R = ref64_bounds(q, k, v, None, SCALE, keep[:, None, None, :], tiles=tiles)
        km = KeyMask.from_padding_mask(prompt_keep) if prompt_keep is not None else None
        for ns in (None, 1, 3):
            o, lse = flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T, prompt_key_mask=km, num_splits=ns,
                                           return_lse=True)
            check_outputs(f"beams G{G} {str(dtype)[6:]} mask {prompt_keep is not None} splits {ns}",
                          {"o": o, "lse2": lse[..., None]}, R)
