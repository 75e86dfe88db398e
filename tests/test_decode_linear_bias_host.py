"""The bias epilogue of the decode linears and the model-family table, without a GPU: the references of
tests/linear_bias_ref.py checked against the fp32 emulation (and shown to reject each wrong kernel), the C ABI's
refusals (smt_linear_skinny_bias returns before any HIP call), the routing predicate's biased form, the CPU path
of the wrappers, and what patch_model / unpatch_model put into and take out of tiny Qwen2 and LLaMA models."""
import ctypes
import os

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_bias_ref as br
from tests.attn_ref import assert_within_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANTS = ["dropped", "other", "by_row", "after_rounding", "truncate"]


def test_the_entry_is_declared_and_exported():
    lib = _hip.load(build_if_missing=True)
    assert "smt_linear_skinny_bias" in _hip.ABI_FUNCTIONS and hasattr(lib, "smt_linear_skinny_bias")
    text = open(os.path.join(ROOT, "include", "smt_linear.h")).read()
    assert "int smt_linear_skinny_bias(" in text and "RN_out( acc[m][n] + (float)b[n] )" in text
    assert lib.smt_abi_version() == 13 and ctypes.sizeof(_hip.SkinnyOut) == 40            # additive: no bump


# ---- the references themselves ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("K", [32, 544])
def test_emulation_meets_the_integer_reference_and_every_mutant_fails_it(M, K):
    dt = torch.bfloat16
    x, (wq, wk), (bq, bk) = br.int_inputs(M, (48, 16), K, dt, seed=M + K)
    want = br.exact(x, wk, bk)
    assert torch.equal(br.emulate(x, wk, bk), want)
    assert want[M - 1, 15].item() == 258.0 and want[M - 1, 0].item() == 264.0            # the planted elements
    for mutant in MUTANTS:
        got = br.emulate(x, wk, bk, mutant=mutant, other=bq)
        assert not torch.equal(got, want), mutant
    # the planted case for double rounding: 257 -> 256, 256 + 1 = 257 -> 256
    assert br.emulate(x, wk, bk, mutant="after_rounding")[M - 1, 15].item() == 256.0
    assert br.emulate(x, wk, bk, mutant="truncate")[M - 1, 0].item() == 262.0
    # an output without a bias is linear_ref's
    assert torch.equal(br.emulate(x, wk, None), br.exact(x, wk, None))
    assert br.exact(x, wk, None)[M - 1, 15].item() == 256.0 and br.exact(x, wk, None)[M - 1, 0].item() == 260.0


def test_exact_reference_in_fp16():
    x, (w,), (b,) = br.int_inputs(5, (48,), 544, torch.float16, seed=1)
    want = br.exact(x, w, b)
    assert torch.equal(br.emulate(x, w, b), want) and want[4, 47].item() == 258.0 and want[4, 0].item() == 263.0
    for mutant in ("dropped", "by_row"):
        assert not torch.equal(br.emulate(x, w, b, mutant=mutant), want), mutant


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M, N, K", [(1, 16, 32), (5, 48, 544), (16, 256, 544)])
def test_emulation_lies_inside_the_bound_and_a_dropped_bias_does_not(M, N, K, dtype):
    x, (w,), (b,) = br.normal_inputs(M, (N,), K, dtype, seed=N + K)
    ref, bound = br.ref64_bound(x, w, b)
    worst = assert_within_bounds("emulation", br.emulate(x, w, b), ref, bound, dims="sd")
    print(f"{dtype} {M}x{N}x{K}: worst err / bound {worst:.3f}")
    with pytest.raises(AssertionError, match="outside"):
        assert_within_bounds("bias dropped", br.emulate(x, w, b, mutant="dropped"), ref, bound, dims="sd")
    ref0, bound0 = br.ref64_bound(x, w, None)
    assert_within_bounds("no bias", br.emulate(x, w, None), ref0, bound0, dims="sd")


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------
def _call(lib, biases=(0, 0, 0), null_array=False, **kw):
    a = dict(x=4096, ldx=64, M=4, K=64, dtype=_hip.DTYPE_BF16, n_out=3, epilogue=_hip.SKINNY_PLAIN)
    a.update(kw)
    outs = (_hip.SkinnyOut * 3)()
    for i in range(3):
        outs[i].w, outs[i].ldw, outs[i].y, outs[i].ldy, outs[i].N = 8192 + 4096 * i, 64, 65536 + 4096 * i, 32, 32
    ptrs = (ctypes.c_void_p * 3)(*[b or None for b in biases])
    return lib.smt_linear_skinny_bias(a["x"], a["ldx"], a["M"], a["K"], a["dtype"], outs, None if null_array else ptrs,
                                      a["n_out"], a["epilogue"], None, None)


def test_abi_refuses_invalid_arguments_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    err = lambda: lib.smt_linear_last_error().decode()
    assert _call(lib, null_array=True) == -1 and "null biases" in err()
    assert _call(lib, biases=(0, 1 << 20, 0), epilogue=_hip.SKINNY_SWIGLU, n_out=2) == -1 and "PLAIN" in err()
    assert _call(lib, biases=(1 << 20, 0, (1 << 20) + 8)) == -2 and "align" in err() and "output 2" in err()
    assert _call(lib, biases=((1 << 20) + 2, 0, 0)) == -2 and "output 0" in err()
    # what smt_linear_skinny refuses, this entry refuses with the same codes
    for kw, rc in ((dict(M=17), -1), (dict(K=48), -1), (dict(dtype=_hip.DTYPE_FP32), -1), (dict(x=None), -1),
                   (dict(ldx=32), -1), (dict(x=4104), -2), (dict(ldx=68), -2), (dict(n_out=4), -1)):
        assert _call(lib, biases=(1 << 20, 0, 0), **kw) == rc, kw
        assert "smt_linear_skinny_bias" in err()


def test_wrapper_checks_its_biases():
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        _hip.linear_skinny(x, [w], biases=[torch.zeros(32, dtype=torch.bfloat16)])


# ---- the routing predicate ---------------------------------------------------------------------------------------
def test_predicate_admits_aligned_biases_and_names_each_violation():
    for dev in ("cpu", "meta"):
        mk = lambda *shape, dtype=torch.bfloat16: torch.empty(*shape, dtype=dtype, device=dev)
        x, w, w2 = mk(4, 4, 64), mk(32, 64), mk(16, 64)
        ok = lambda *a, **k: fl.decode_linear_reason(*a, need_cuda=False, **k)
        with torch.no_grad():
            assert ok(x, (w,), (mk(32),)) == "bias"                                        # the defaults stay
            assert ok(x, (w, w2, w2), (mk(32), None, None)) == "bias"
            assert ok(x, (w,), (mk(32),), allow_bias=True) is None
            assert ok(x, (w, w2, w2), (mk(32), mk(16), mk(16)), allow_bias=True) is None
            assert ok(x, (w, w2, w2), (None, mk(16), None), allow_bias=True) is None
            assert ok(x, (w, w2), (None, None), allow_bias=True) is None and ok(x, (w,), (), allow_bias=True) is None
            assert "bias shape" in ok(x, (w,), (mk(1, 32),), allow_bias=True)              # 2-D
            assert "bias shape" in ok(x, (w,), (mk(16),), allow_bias=True)
            assert "bias torch.float32" in ok(x, (w,), (mk(32, dtype=torch.float32),), allow_bias=True)
            assert "bias stride or alignment" == ok(x, (w,), (mk(40)[1:33],), allow_bias=True)   # offset by one element
            assert "bias stride or alignment" == ok(x, (w,), (mk(64)[::2],), allow_bias=True)
            assert "biases for" in ok(x, (w, w2), (mk(32),), allow_bias=True)
            assert "rows" in ok(mk(17, 64), (w,), (mk(32),), allow_bias=True)              # the rest still holds
            b = mk(32).requires_grad_()
            assert ok(x, (w,), (b,), allow_bias=True) is None                              # gradients are off
        with torch.enable_grad():
            assert "bias needs a gradient" in ok(x, (w,), (b,), allow_bias=True)
            assert "gradients" in ok(x, (w,), (mk(32),), allow_bias=True) and "gradients" in ok(x, (w,), (b,))
    with torch.no_grad():
        other = torch.empty(32, dtype=torch.bfloat16, device="meta")
        assert "beside" in fl.decode_linear_reason(torch.empty(4, 64, dtype=torch.bfloat16), (torch.empty(32, 64, dtype=torch.bfloat16),),
                                                   (other,), need_cuda=False, allow_bias=True)


def test_size_rule_of_the_biased_route_and_where_a_bias_is_admitted():
    mk = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device="meta")
    routes = lambda *a: fl._decode_routes(*a, need_cuda=False, allow_bias=True)          # the PLAIN call sites' form
    with torch.no_grad():
        for H, Nq, Nkv in ((1536, 1536, 256), (3584, 3584, 512)):                          # the Qwen2 distills
            x, ws, bs = mk(16, 1, H), (mk(Nq, H), mk(Nkv, H), mk(Nkv, H)), (mk(Nq), mk(Nkv), mk(Nkv))
            assert routes(x, ws, bs)
            # a single biased weight: at every row count up to K = 2048, at up to 4 rows above it
            for i in (0, 1):
                assert routes(x, ws[i:i + 1], bs[i:i + 1]) == (H <= 2048)
                assert routes(mk(4, 1, H), ws[i:i + 1], bs[i:i + 1])
                assert routes(mk(5, 1, H), ws[i:i + 1], bs[i:i + 1]) == (H <= 2048)
                assert routes(x, ws[i:i + 1], (None,))                                     # the unbiased rule is as it was
            # without the keyword, which is how every other call site asks, a bias is refused as before
            assert not fl._decode_routes(x, ws, bs, need_cuda=False)
            assert fl._decode_routes(x, ws, (None, None, None), need_cuda=False)
        assert not routes(mk(16, 1, 4096), (mk(8208, 4096),), (mk(8208),))                 # the 2^25 limit
        # the gate/up/SwiGLU launch has no biased form: fused_mlp_forward asks without the keyword, and a biased
        # pair (LlamaConfig(mlp_bias=True)) must not route, whatever DECODE_LINEAR_BIAS says
        x, g, u, b = mk(4, 1, 2048), mk(1024, 2048), mk(1024, 2048), mk(1024)
        assert fl.DECODE_LINEAR_BIAS and fl._decode_routes(x, (g, u), (None, None), need_cuda=False)
        for pair in ((b, b), (b, None), (None, b)):
            assert not fl._decode_routes(x, (g, u), pair, need_cuda=False)


def test_only_patch_model_turns_the_bias_epilogue_on():
    """patch_llama routes what it always routed: on a LLaMA model with biased projections they keep running
    F.linear. patch_model marks the routed linears for the bias epilogue; unpatching removes the mark."""
    marked = lambda m: sorted(n for n, x in m.named_modules() if x.__dict__.get("_smt_decode_bias"))
    model = _tiny("llama", attention_bias=True, mlp_bias=True)
    try:
        assert fl.patch_llama(model, attention=False, loss=False, decode_linears=True)["decode_linears"] == 15
        assert marked(model) == []
    finally:
        fl.unpatch_llama(model)
    for family in ("llama", "qwen2"):
        model = _tiny(family, **(dict(attention_bias=True, mlp_bias=True) if family == "llama" else {}))
        try:
            assert fl.patch_model(model, decode_linears=True)["decode_linears"] == 15
            assert len(marked(model)) == 15
        finally:
            fl.unpatch_model(model)
        assert marked(model) == []
        try:
            assert fl.route_decode_linears(model, bias=False) == 15 and marked(model) == []
        finally:
            fl.unroute_decode_linears(model)


def test_cpu_wrappers_are_f_linear_and_count_nothing():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, generator=g).bfloat16()
    ws = [torch.randn(n, 64, generator=g).bfloat16() for n in (32, 16, 48)]
    bs = [torch.randn(32, generator=g).bfloat16(), None, torch.randn(48, generator=g).bfloat16()]
    fl.decode_linear_stats.reset()
    assert fl.decode_linear_stats.bias == 0
    assert torch.equal(fl.decode_linear(x, ws[0], bs[0]), torch.nn.functional.linear(x, ws[0], bs[0]))
    for got, w, b in zip(fl.decode_linear_group(x, ws, bs), ws, bs):
        assert torch.equal(got, torch.nn.functional.linear(x, w, b))
    assert fl.decode_linear_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0} and fl.decode_linear_stats.bias == 0


# ---- the family table ------------------------------------------------------------------------------------------
def _tiny(family, **kw):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen2Config, Qwen2ForCausalLM
    Config, Model = (Qwen2Config, Qwen2ForCausalLM) if family == "qwen2" else (LlamaConfig, LlamaForCausalLM)
    args = dict(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, vocab_size=96, max_position_embeddings=32, attn_implementation="eager")
    args.update(kw)
    with torch.device("meta"):
        return Model(Config(**args))


def _rope(family):
    import importlib
    return importlib.import_module(fl.FAMILIES[family].module_name)


@pytest.mark.parametrize("family", ["qwen2", "llama"])
def test_patch_model_patches_every_kind_and_unpatch_model_removes_all_of_it(family):
    model = _tiny(family)
    other = "llama" if family == "qwen2" else "qwen2"
    eager = {f: _rope(f).apply_rotary_pos_emb for f in ("llama", "qwen2")}
    assert eager[family] is not fl.fused_apply_rotary_pos_emb and eager[other] is not fl.fused_apply_rotary_pos_emb
    assert fl.model_family(model) is fl.FAMILIES[family]
    try:
        counts = fl.patch_model(model, decode_linears=True)
        assert set(counts) == {"rmsnorm", "mlp", "rope", "attention", "loss", "decoder", "lm_head_loss", "decode_linears"}
        assert all(v > 0 for v in counts.values()), counts
        assert counts["rmsnorm"] == 5 and counts["mlp"] == counts["decoder"] == counts["attention"] == 2
        assert counts["decode_linears"] == 2 * 7 + 1
        assert _rope(family).apply_rotary_pos_emb is fl.fused_apply_rotary_pos_emb
        assert _rope(other).apply_rotary_pos_emb is eager[other]                           # the other family's: untouched
        assert model.__dict__["forward"].__func__ is fl.smt_causal_lm_forward and model.__dict__["_smt_lm_head_forward"]
        layers = model.model.layers
        assert layers[0].__dict__["_smt_next_layer"]() is layers[1] and "_smt_next_layer" not in layers[1].__dict__
        q = layers[0].self_attn.q_proj
        assert "_smt_decode_group" in q.__dict__ and (q.bias is not None) == (family == "qwen2")
        assert model.config._attn_implementation == fl.ATTN_NAME
    finally:
        fl.unpatch_model(model)
    assert _rope(family).apply_rotary_pos_emb is eager[family] and _rope(other).apply_rotary_pos_emb is eager[other]
    assert model.config._attn_implementation == "eager"
    for n, m in model.named_modules():
        assert "forward" not in m.__dict__ and not any(k.startswith("_smt_") for k in m.__dict__), n


def test_patch_llama_on_a_qwen2_model_still_matches_nothing():
    model = _tiny("qwen2")
    try:
        counts = fl.patch_llama(model, attention=False, loss=False, decode_linears=True)
        assert counts["rmsnorm"] == counts["mlp"] == counts["decoder"] == counts["decode_linears"] == 0
    finally:
        fl.unpatch_llama(model)


def test_patch_model_refuses_before_it_changes_anything():
    sliding = _tiny("qwen2", use_sliding_window=True, sliding_window=16, max_window_layers=1)
    assert "sliding_attention" in sliding.config.layer_types
    cases = [(sliding, "sliding_attention"), (_tiny("qwen2", hidden_size=128), "head_dim 64"),
             (_tiny("llama", hidden_size=128), "head_dim 64"), (_tiny("llama", hidden_act="gelu"), "SiLU"),
             (torch.nn.Linear(4, 4), "no family")]
    eager = {f: _rope(f).apply_rotary_pos_emb for f in ("llama", "qwen2")}
    for model, why in cases:
        with pytest.raises(NotImplementedError, match=why):
            fl.patch_model(model, decode_linears=True)
        for n, m in model.named_modules():
            assert "forward" not in m.__dict__ and not any(k.startswith("_smt_") for k in m.__dict__), (why, n)
        if getattr(model, "config", None) is not None:
            assert model.config._attn_implementation == "eager"
        assert all(_rope(f).apply_rotary_pos_emb is eager[f] for f in eager)
    with pytest.raises(NotImplementedError, match="no family"):
        fl.unpatch_model(torch.nn.Linear(4, 4))
