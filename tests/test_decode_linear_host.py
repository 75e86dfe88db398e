"""The decode linears without a GPU: every refusal of the C ABI (include/smt_linear.h; they return before any
HIP call), the two references of tests/linear_ref.py checked against an fp32 emulation of the kernel's
reduction (and shown to fail when they should), the routing predicate on CPU and meta tensors, what
patch_llama(decode_linears=...) puts into the modules and takes out again, and the CPU path of the wrappers."""
import ctypes
import os
import re

import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_ref as lr
from tests.attn_ref import assert_within_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16, 32), (3, 48, 96), (16, 32, 14336)]


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "smt_linear.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("SMT_LINEAR_KSPLIT") == _hip.SKINNY_KSPLIT == lr.KSPLIT
    assert define("SMT_LINEAR_MAX_M") == _hip.SKINNY_MAX_M and define("SMT_LINEAR_MAX_OUT") == _hip.SKINNY_MAX_OUT
    assert define("SMT_SKINNY_PLAIN") == _hip.SKINNY_PLAIN and define("SMT_SKINNY_SWIGLU") == _hip.SKINNY_SWIGLU
    assert ctypes.sizeof(_hip.SkinnyOut) == 40 and _hip.ABI_VERSION == 13


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(x=4096, ldx=64, M=4, K=64, dtype=_hip.DTYPE_BF16, n_out=2, epilogue=_hip.SKINNY_PLAIN,
             w=[8192, 8192 + 4096, 8192 + 8192], ldw=[64, 64, 64], y=[65536, 65536 + 4096, 65536 + 8192], ldy=[32, 32, 32],
             N=[32, 32, 32], outs=True)
    a.update(kw)
    outs = (_hip.SkinnyOut * 4)()
    for i in range(3):
        outs[i].w, outs[i].ldw, outs[i].y, outs[i].ldy, outs[i].N = a["w"][i], a["ldw"][i], a["y"][i], a["ldy"][i], a["N"][i]
    po = outs if a["outs"] else None
    ws = lib.smt_linear_skinny_workspace(a["M"], a["K"], po, a["n_out"], a["epilogue"])
    rc = lib.smt_linear_skinny(a["x"], a["ldx"], a["M"], a["K"], a["dtype"], po, a["n_out"], a["epilogue"], None, None)
    return rc, ws


def test_abi_refuses_invalid_arguments_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    three = lambda v, i, new: [new if j == i else v for j in range(3)]
    invalid_sizes = [dict(M=0), dict(M=17), dict(K=0), dict(K=48), dict(K=-32), dict(N=[24, 32, 32]), dict(N=[32, 0, 32]),
                     dict(n_out=0), dict(n_out=4), dict(epilogue=2), dict(epilogue=-1), dict(outs=False),
                     dict(epilogue=_hip.SKINNY_SWIGLU, n_out=1), dict(epilogue=_hip.SKINNY_SWIGLU, n_out=3),
                     dict(epilogue=_hip.SKINNY_SWIGLU, n_out=2, N=[32, 48, 32])]
    for kw in invalid_sizes:                                 # the workspace query refuses these too
        rc, ws = _call(lib, **kw)
        assert rc == -1 and ws == -1, kw
        assert lib.smt_linear_last_error().decode()
    invalid = [dict(dtype=_hip.DTYPE_FP32), dict(dtype=7), dict(x=None), dict(w=three(8192, 1, None)),
               dict(y=three(65536, 0, None)), dict(ldx=32), dict(ldw=three(64, 0, 56)), dict(ldy=three(32, 1, 24)),
               dict(epilogue=_hip.SKINNY_SWIGLU, y=three(65536, 0, None))]
    for kw in invalid:
        rc, ws = _call(lib, **kw)
        assert rc == -1 and ws == 0, kw
    misaligned = [dict(x=4104), dict(ldx=68), dict(w=three(8192, 1, 8200)), dict(ldw=three(64, 0, 68)),
                  dict(y=three(65536, 1, 65538)), dict(ldy=three(32, 0, 36))]
    for kw in misaligned:
        rc, ws = _call(lib, **kw)
        assert rc == -2 and ws == 0, kw
        assert "align" in lib.smt_linear_last_error().decode()
    # outputs past n_out are not looked at, nor is the second y of a SWIGLU call: these pass every check
    # and fail only at the launch on a machine without a GPU, or not at all (nothing is checked here but
    # that they are not refused as invalid)
    assert lib.smt_linear_skinny_workspace(16, 14336, (_hip.SkinnyOut * 1)(_hip.SkinnyOut(N=128256)), 1, 0) == 0


def test_wrapper_needs_device_tensors():
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        _hip.linear_skinny(x, [w])


# ---- the references themselves ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_emulation_meets_the_integer_reference_and_the_bar_can_fail(M, N, K):
    dt = torch.bfloat16
    for scale in (False, True):
        x, w = lr.int_inputs(M, N, K, dt, seed=K + M, row_scale=scale)
        want = lr.exact(x, w)
        assert torch.equal(lr.emulate(x, w), want)
        assert torch.equal(lr.emulate(x, w, ksplit=1), want)                 # any order: the sums are exact
    x, w = lr.int_inputs(M, N, K, dt, seed=K + M)
    want = lr.exact(x, w)
    assert want[M - 1, N - 1].item() == 260.0                              # the planted tie, rounded to even
    assert not torch.equal(lr.emulate(x, w, trunc=True), want)
    k = int((x[0] * w[0]).abs().argmax())
    if K == 32:
        assert not torch.equal(lr.emulate(x, w, drop=(0, 0, k)), want)
    if M > 1:
        swapped = x.clone()
        swapped[[0, 1]] = x[[1, 0]]
        assert not torch.equal(lr.emulate(swapped, w), want)


def test_exact_reference_in_fp16():
    x, w = lr.int_inputs(5, 32, 544, torch.float16, seed=1, row_scale=True)
    assert torch.equal(lr.emulate(x, w), lr.exact(x, w))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_emulation_lies_inside_the_bound(M, N, K, dtype):
    x, w = lr.normal_inputs(M, N, K, dtype, seed=N + K)
    ref, bound = lr.ref64_bound(x, w)
    worst = assert_within_bounds("emulation", lr.emulate(x, w), ref, bound, dims="sd")
    print(f"{dtype} {M}x{N}x{K}: worst err / bound {worst:.3f}")
    if K == 32:
        p = (x[0].double() * w[0].double()).abs()
        with pytest.raises(AssertionError, match="outside"):
            assert_within_bounds("one product dropped", lr.emulate(x, w, drop=(0, 0, int(p.argmax()))), ref, bound, dims="sd")


# ---- the routing predicate ---------------------------------------------------------------------------------------
def test_predicate_names_each_disqualifier():
    for dev in ("cpu", "meta"):
        mk = lambda *shape, dtype=torch.bfloat16: torch.empty(*shape, dtype=dtype, device=dev)
        x, w = mk(4, 4, 64), mk(32, 64)
        ok = lambda *a, **k: fl.decode_linear_reason(*a, need_cuda=False, **k)
        with torch.no_grad():
            assert ok(x, (w,)) is None and ok(x, (w, w, mk(16, 64)), (None, None, None)) is None
            assert ok(mk(16, 64), (w,)) is None and ok(mk(64), (w,)) is None
            assert ok(mk(16, 128)[:, :64], (w,)) is None and ok(x, (mk(32, 128)[:, :64],)) is None
            assert "device" in fl.decode_linear_reason(x, (w,))
            assert ok(x, (w,), (mk(32),)) == "bias"
            assert "dtype" in ok(mk(4, 64, dtype=torch.float32), (mk(32, 64, dtype=torch.float32),))
            assert "beside" in ok(x, (mk(32, 64, dtype=torch.float16),))
            assert "rows" in ok(mk(17, 64), (w,)) and "rows" in ok(mk(2, 9, 64), (w,)) and "rows" in ok(mk(0, 64), (w,))
            assert "K 48" in ok(mk(4, 48), (mk(32, 48),))
            assert "N 24" in ok(x, (mk(24, 64),))
            assert "weight shape" in ok(x, (mk(32, 96),))
            assert "stride" in ok(mk(4, 128)[:, ::2], (w,)) and "alignment" in ok(mk(4, 72)[:, 4:68], (w,))
            assert "flatten" in ok(mk(4, 68)[:, :64], (w,)) and "flatten" in ok(mk(2, 4, 128)[:, :, :64], (w,))
            assert "weight stride" in ok(x, (mk(32, 68)[:, :64],)) and "weight stride" in ok(x, (mk(64, 32).t(),))
            assert "weights" in ok(x, (w, w, w, w)) and "weights" in ok(x, ())
            tagged = mk(32, 64)
            tagged._smt_fp8 = object()
            assert ok(x, (tagged,)) == "fp8 weight"
        with torch.enable_grad():
            assert "gradients" in ok(x, (w,))


def test_size_rule_of_the_routing():
    """The routing sends a launch to the kernel only at the sizes where it measured faster than hipBLASLt."""
    mk = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device="meta")
    routes = lambda x, ws: fl._decode_routes(x, ws, need_cuda=False)
    with torch.no_grad():
        x = mk(16, 1, 4096)
        assert routes(x, (mk(4096, 4096),)) and routes(x, (mk(1024, 4096),))
        assert routes(x, (mk(4096, 4096), mk(1024, 4096), mk(1024, 4096)))          # 6144 x 4096: 2^24 * 1.5
        assert routes(x, (mk(8192, 4096),)) and not routes(x, (mk(8208, 4096),))     # the 2^25 limit
        assert not routes(x, (mk(14336, 4096), mk(14336, 4096))) and not routes(x, (mk(128256, 4096),))
        assert not routes(mk(16, 1, 14336), (mk(4096, 14336),)) and not routes(mk(16, 1, 5120), (mk(5120, 5120),))
        assert routes(mk(8, 1, 512), (mk(1024, 512), mk(1024, 512)))
        assert not routes(mk(17, 1, 4096), (mk(4096, 4096),))                        # the predicate comes first


# ---- what patch_llama puts into the modules --------------------------------------------------------------------
def _tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=32, vocab_size=96, max_position_embeddings=32,
                      attn_implementation="eager")
    with torch.device("meta"):
        return LlamaForCausalLM(cfg)


def _linears(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.Linear)}


def test_routing_is_opt_in_and_unpatch_removes_it():
    model = _tiny()
    lin = _linears(model)
    assert len(lin) == 2 * 7 + 1
    try:
        counts = fl.patch_llama(model, attention=False, loss=False)
        assert "decode_linears" not in counts
        for n, m in lin.items():
            assert "forward" not in m.__dict__ and not any(k.startswith("_smt_decode") for k in m.__dict__), n
        assert not any("_smt_decode_linears" in m.__dict__ for m in model.modules())
        counts = fl.patch_llama(model, attention=False, loss=False, decode_linears=True)
        assert counts["decode_linears"] == len(lin)
        for n, m in lin.items():
            assert m.__dict__["forward"].__func__ is fl.decode_routed_linear_forward, n
            assert ("_smt_decode_group" in m.__dict__) == n.endswith("q_proj"), n
        assert fl.patch_llama(model, attention=False, loss=False, decode_linears=True)["decode_linears"] == 0   # idempotent
    finally:
        fl.unpatch_llama(model)
    for n, m in lin.items():
        assert "forward" not in m.__dict__ and not any(k.startswith("_smt_decode") for k in m.__dict__), n
    assert not any("_smt_decode_linears" in m.__dict__ for m in model.modules())


def test_a_biased_head_and_an_earlier_instance_forward_are_respected():
    model = _tiny()
    model.lm_head.bias = torch.nn.Parameter(torch.zeros(96, device="meta"))
    down = model.model.layers[0].mlp.down_proj
    marker = lambda x: "earlier"
    down.forward = marker
    try:
        counts = fl.patch_llama(model, attention=False, loss=False, decode_linears=True)
        assert counts["decode_linears"] == 14 and "forward" not in model.lm_head.__dict__
        assert down.__dict__["_smt_decode_prev_forward"] is marker
        with torch.no_grad():
            assert down(torch.zeros(17, 128)) == "earlier"              # a CPU fp32 call does not qualify
    finally:
        fl.unpatch_llama(model)
    assert down.__dict__["forward"] is marker


# ---- the wrappers on the CPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_cpu_wrappers_are_the_torch_chain(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, generator=g).to(dtype)
    ws = [torch.randn(n, 64, generator=g).to(dtype) for n in (32, 16, 48)]
    fl.decode_linear_stats.reset()
    assert torch.equal(fl.decode_linear(x, ws[0]), torch.nn.functional.linear(x, ws[0]))
    for got, w in zip(fl.decode_linear_group(x, ws), ws):
        assert torch.equal(got, torch.nn.functional.linear(x, w))
    up = torch.randn(32, 64, generator=g).to(dtype)
    want = torch.nn.functional.silu(torch.nn.functional.linear(x, ws[0])) * torch.nn.functional.linear(x, up)
    assert torch.equal(fl.decode_swiglu(x, ws[0], up), want)
    assert fl.decode_linear_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0}       # no kernel ran
