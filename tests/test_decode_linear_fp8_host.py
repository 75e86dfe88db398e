"""The e4m3 decode linears without a GPU: the two references of tests/linear_fp8_ref.py checked against an fp32
emulation of the kernel (and shown to fail for every mutant, on the inputs tests/test_gpu_decode_linear_fp8.py
uses), the C ABI's refusals (they return before any HIP call), the fp8 routing predicate on CPU tensors, and
patch_llama's decode_fp8 keyword."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sparse_matrix_tuning_amd import _hip
from sparse_matrix_tuning_amd import fused_llama as fl
from tests import linear_fp8_ref as fr
from tests import linear_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
# the GPU test's cases on which the mutants are run: every path of the K split, M = 1 and M > 1
MUTANT_CASES = [c for c in fr.CASES if c[:3] in ((5, 48, 576), (16, 16, 4160), (1, 16, 64), (16, 16, 14336))]


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "smt_linear.h")).read()
    assert int(re.search(r"#define SMT_LINEAR_KSPLIT (\d+)", text).group(1)) == fr.KSPLIT == lr.KSPLIT == _hip.SKINNY_KSPLIT
    assert "K % 64 == 0" in text and fr.KSTEP == 64
    assert ctypes.sizeof(_hip.SkinnyFp8Out) == 48 and _hip.ABI_VERSION == 13
    assert {"smt_linear_skinny_fp8", "smt_linear_skinny_fp8_workspace"} <= set(_hip.ABI_FUNCTIONS)


def test_cases_cover_what_the_issue_names():
    shapes = {c[:3] for c in fr.CASES}
    for K in (64, 512, 576, 4160):
        for N in (16, 48):
            for M in (1, 5, 16):
                assert (M, N, K) in shapes
    assert {(M, 16, 14336) for M in (1, 5, 16)} <= shapes and not any(c[2] == 14336 and c[1] != 16 for c in fr.CASES)
    assert any(c[3] for c in fr.CASES)


# ---- the references themselves ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M, N, K, pad", fr.CASES)
def test_emulation_meets_both_references(M, N, K, pad):
    ld = K + pad if pad else None
    x8, sx, w8, sw = fr.int_inputs(M, N, K, seed=M + N + K, ldx=ld, ldw=ld)
    assert not any(float(np.log2(s)).is_integer() for s in (*sx[:-1], *sw[:-1])) and sx[-1] == 1 and sw[-1] == 1
    for dtype in DTYPES:
        want = fr.exact(x8, sx, w8, sw, dtype)
        assert torch.equal(fr.emulate(x8, sx, w8, sw, dtype), want)
        assert torch.equal(fr.emulate(x8, sx, w8, sw, dtype, ksplit=1), want)        # any order: acc is exact
    assert fr.exact(x8, sx, w8, sw, torch.bfloat16)[M - 1, N - 1].item() == 260.0    # the planted tie, to even
    x, w = fr.normal_bf16(M, N, K, seed=N + K)
    (x8, sx), (w8, sw) = fr.quant_host(x, ld), fr.quant_host(w, ld)
    for dtype in DTYPES:
        ref, bound = fr.ref64_bound(x8, sx, w8, sw, dtype)
        assert fr.within(fr.emulate(x8, sx, w8, sw, dtype), ref, bound)


@pytest.mark.parametrize("mut", fr.MUTANTS, ids=lambda m: next(iter(m)))
def test_each_mutant_fails_a_reference_on_the_gpu_tests_inputs(mut):
    caught_exact = caught_bound = 0
    for M, N, K, pad in MUTANT_CASES:
        if M == 1 and ("wrong_sx" in mut or "swap_rows" in mut):
            continue                                                                 # one row: nothing to mix up
        kw = fr.mutant_kwargs(mut, M, N)
        x8, sx, w8, sw = fr.int_inputs(M, N, K, seed=M + N + K)
        caught_exact += not torch.equal(fr.emulate(x8, sx, w8, sw, torch.bfloat16, **kw),
                                        fr.exact(x8, sx, w8, sw, torch.bfloat16))
        x, w = fr.normal_bf16(M, N, K, seed=N + K)
        (x8, sx), (w8, sw) = fr.quant_host(x), fr.quant_host(w)
        if "drop" in kw:                                     # the largest product of the element, not the planted one
            p = np.abs(fr.R.e4m3_decode(x8[0]) * fr.R.e4m3_decode(w8[0]))
            kw = {"drop": (0, 0, int(p.argmax()))}
        ref, bound = fr.ref64_bound(x8, sx, w8, sw, torch.bfloat16)
        caught_bound += not fr.within(fr.emulate(x8, sx, w8, sw, torch.bfloat16, **kw), ref, bound)
    applicable = sum(1 for c in MUTANT_CASES if not (c[0] == 1 and ("wrong_sx" in mut or "swap_rows" in mut)))
    print(f"{mut}: the integer bar caught it in {caught_exact}, the bound in {caught_bound} of {applicable} cases")
    # the integer bar sees every mutant wherever it can differ: rounding before the scales changes nothing while
    # |acc| <= 256 (M = 1, K = 64), which bf16 holds exactly
    assert caught_exact >= applicable - ("scale_after_round" in mut) and caught_exact >= 1


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(x=4096, ldx=64, sx=1024, M=4, K=64, dtype=_hip.DTYPE_BF16, n_out=2, epilogue=_hip.SKINNY_PLAIN,
             w=[8192, 8192 + 4096, 8192 + 8192], sw=[2048, 2048 + 256, 2048 + 512], ldw=[64, 64, 64],
             y=[65536, 65536 + 4096, 65536 + 8192], ldy=[32, 32, 32], N=[32, 32, 32], outs=True)
    a.update(kw)
    outs = (_hip.SkinnyFp8Out * 4)()
    for i in range(3):
        o = outs[i]
        o.w8, o.sw, o.ldw, o.y, o.ldy, o.N = a["w"][i], a["sw"][i], a["ldw"][i], a["y"][i], a["ldy"][i], a["N"][i]
    po = outs if a["outs"] else None
    ws = lib.smt_linear_skinny_fp8_workspace(a["M"], a["K"], po, a["n_out"], a["epilogue"])
    rc = lib.smt_linear_skinny_fp8(a["x"], a["ldx"], a["sx"], a["M"], a["K"], a["dtype"], po, a["n_out"], a["epilogue"],
                                   None, None)
    return rc, ws


def test_abi_refuses_invalid_arguments_before_any_hip_call():
    lib = _hip.load(build_if_missing=True)
    three = lambda v, i, new: [new if j == i else v for j in range(3)]
    for kw in [dict(M=0), dict(M=17), dict(K=0), dict(K=32), dict(K=96), dict(K=-64), dict(N=[24, 32, 32]),
               dict(N=[32, 0, 32]), dict(n_out=0), dict(n_out=4), dict(epilogue=2), dict(outs=False),
               dict(epilogue=_hip.SKINNY_SWIGLU, n_out=1), dict(epilogue=_hip.SKINNY_SWIGLU, n_out=3),
               dict(epilogue=_hip.SKINNY_SWIGLU, n_out=2, N=[32, 48, 32])]:
        rc, ws = _call(lib, **kw)
        assert rc == -1 and ws == -1, kw
        assert lib.smt_linear_last_error().decode()
    for kw in [dict(dtype=_hip.DTYPE_FP32), dict(dtype=7), dict(x=None), dict(sx=None), dict(w=three(8192, 1, None)),
               dict(sw=three(2048, 0, None)), dict(y=three(65536, 0, None)), dict(ldx=48), dict(ldw=three(64, 0, 48)),
               dict(ldy=three(32, 1, 24))]:
        rc, ws = _call(lib, **kw)
        assert rc == -1 and ws == 0, kw
    for kw in [dict(x=4104), dict(ldx=72), dict(sx=1026), dict(w=three(8192, 1, 8200)), dict(sw=three(2048, 1, 2052)),
               dict(ldw=three(64, 0, 72)), dict(y=three(65536, 1, 65544)), dict(ldy=three(32, 0, 36))]:
        rc, ws = _call(lib, **kw)
        assert rc == -2 and ws == 0, kw
        assert "align" in lib.smt_linear_last_error().decode()
    assert lib.smt_linear_skinny_fp8_workspace(16, 14336, (_hip.SkinnyFp8Out * 1)(_hip.SkinnyFp8Out(N=4096)), 1, 0) == 0


def test_wrapper_needs_device_tensors():
    x8, w8 = torch.zeros(4, 64, dtype=torch.uint8), torch.zeros(32, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        _hip.linear_skinny_fp8(x8, torch.ones(4), [(w8, torch.ones(32))], torch.bfloat16)


# ---- the routing predicate ---------------------------------------------------------------------------------------
def _fw(n, k, ld=None, dtype=torch.uint8):
    w8 = torch.zeros(n, ld or k, dtype=dtype)[:, :k]
    return SimpleNamespace(w8=w8, sw=torch.ones(n))


def test_predicate_admits_and_names_each_disqualifier():
    mk = lambda *shape, dtype=torch.bfloat16: torch.empty(*shape, dtype=dtype)
    ok = lambda *a, **k: fl.decode_linear_fp8_reason(*a, need_cuda=False, **k)
    x, fw = mk(4, 4, 64), _fw(32, 64)
    tagged = mk(32, 64)
    tagged._smt_fp8 = fw
    with torch.no_grad():
        assert ok(x, (fw,)) is None and ok(x, (tagged,)) is None and ok(x, (fw, tagged, _fw(16, 64)), (None,) * 3) is None
        assert ok(mk(16, 64), (fw,)) is None and ok(mk(64), (fw,)) is None and ok(x, (_fw(32, 64, ld=80),)) is None
        assert ok(x, (_fw(32, 64, dtype=torch.float8_e4m3fn),)) is None
        # the kernel reads the e4m3 copy of x, so x's own strides do not matter (the fused RMSNorm hands over a
        # zero-stride placeholder that carries only the copy)
        assert ok(mk(()).expand(2, 8, 64), (fw,)) is None and ok(mk(4, 128)[:, ::2], (fw,)) is None
        assert "device" in fl.decode_linear_fp8_reason(x, (fw,))
        assert ok(x, (fw,), (mk(32),)) == "bias"
        assert "dtype" in ok(mk(4, 64, dtype=torch.float32), (fw,)) and "dtype" in ok(mk(4, 64, dtype=torch.float16), (fw,))
        assert "rows" in ok(mk(17, 64), (fw,)) and "rows" in ok(mk(2, 9, 64), (fw,)) and "rows" in ok(mk(0, 64), (fw,))
        assert "K 96" in ok(mk(4, 96), (_fw(32, 96),)) and "K 32" in ok(mk(4, 32), (_fw(32, 32),))
        assert "N 24" in ok(x, (_fw(24, 64),))
        assert "w8 shape" in ok(x, (_fw(32, 128),)) and "w8 shape" in ok(x, (_fw(32, 64, dtype=torch.bfloat16),))
        assert "w8 stride" in ok(x, (_fw(32, 64, ld=72),))
        assert "w8 stride" in ok(x, (SimpleNamespace(w8=torch.zeros(32, 80, dtype=torch.uint8)[:, 8:72], sw=torch.ones(32)),))
        assert "sw" in ok(x, (SimpleNamespace(w8=fw.w8, sw=torch.ones(64)[::2]),))
        assert "sw" in ok(x, (SimpleNamespace(w8=fw.w8, sw=torch.ones(32, dtype=torch.float64)),))
        assert "without an fp8 copy" in ok(x, (mk(32, 64),)) and "without an fp8 copy" in ok(x, (fw, mk(32, 64)))
        assert "weights" in ok(x, (fw,) * 4) and "weights" in ok(x, ())
        # the bf16 predicate still refuses such a weight, in the words the existing tests compare
        assert fl.decode_linear_reason(x, (tagged,), need_cuda=False) == "fp8 weight"
    with torch.enable_grad():
        assert "gradients" in ok(x, (fw,))


def test_calls_refuse_what_does_not_qualify_and_count_nothing():
    fl.decode_fp8_stats.reset()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="does not qualify.*device"):
            fl.decode_linear_fp8(torch.zeros(4, 64, dtype=torch.bfloat16), _fw(32, 64))
        with pytest.raises(RuntimeError, match="does not qualify.*device"):                # no CPU path
            fl.decode_swiglu_fp8(torch.zeros(4, 64, dtype=torch.bfloat16), _fw(32, 64), _fw(32, 64))
    assert fl.decode_fp8_stats.as_dict() == {"single": 0, "group": 0, "swiglu": 0, "quant": 0}
    assert fl.decode_linear_stats.as_dict().keys() == {"single", "group", "swiglu"}       # the bf16 route's stay as they are


def test_size_rule_of_the_fp8_routing(monkeypatch):
    """The rule's constants are the measured ones (profiles/r21_decode_linear_fp8_bench.jsonl); with
    DECODE_FP8_RULE off every qualifying launch routes."""
    routes = lambda x, ws: fl._decode_fp8_routes(x, ws, need_cuda=False)
    x = torch.empty(16, 1, 4096, dtype=torch.bfloat16, device="meta")
    mk = lambda n, k: SimpleNamespace(w8=torch.empty(n, k, dtype=torch.uint8, device="meta"),
                                      sw=torch.empty(n, dtype=torch.float32, device="meta"))
    xm = lambda m, k=4096: torch.empty(m, 1, k, dtype=torch.bfloat16, device="meta")
    with torch.no_grad():
        assert not routes(torch.empty(17, 4096, dtype=torch.bfloat16, device="meta"), (mk(4096, 4096),))
        for m in (1, 4, 16):                                                  # the attention projections: any M
            assert routes(xm(m), (mk(4096, 4096),)) and routes(xm(m), (mk(1024, 4096),))
            assert routes(xm(m), (mk(4096, 4096), mk(1024, 4096), mk(1024, 4096)))
            assert routes(xm(m), (mk(8192, 4096),)) and not routes(xm(m, 14336), (mk(4096, 14336),))
            assert not routes(xm(m, 5120), (mk(5120, 5120),)) and not routes(xm(m, 5120), (mk(13824, 5120),))
        for m in (1, 4):                                                      # the MLP's gate and pair: up to 4 rows
            assert routes(xm(m), (mk(14336, 4096),)) and routes(xm(m), (mk(14336, 4096), mk(14336, 4096)))
            assert not routes(xm(m), (mk(32784, 4096),))                      # the 2^27 limit
        for m in (5, 16):
            assert not routes(xm(m), (mk(14336, 4096),)) and not routes(xm(m), (mk(14336, 4096), mk(14336, 4096)))
            assert not routes(xm(m), (mk(8208, 4096),))                       # the 2^25 limit
        assert routes(xm(8, 1024), (mk(2048, 1024), mk(2048, 1024)))
        monkeypatch.setattr(fl, "DECODE_FP8_RULE", False)
        assert routes(x, (mk(14336, 4096), mk(14336, 4096)))
        assert routes(torch.empty(16, 14336, dtype=torch.bfloat16, device="meta"), (mk(4096, 14336),))
        assert not routes(torch.empty(17, 4096, dtype=torch.bfloat16, device="meta"), (mk(4096, 4096),))


# ---- patch_llama's keyword ---------------------------------------------------------------------------------------
def _tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=32, vocab_size=96, max_position_embeddings=32,
                      attn_implementation="eager")
    with torch.device("meta"):
        return LlamaForCausalLM(cfg)


def test_decode_fp8_needs_decode_linears_and_unpatch_removes_it():
    model = _tiny()
    marks = lambda: [k for m in model.modules() for k in m.__dict__ if k.startswith("_smt_decode")]
    with pytest.raises(ValueError, match="decode_linears"):
        fl.patch_llama(model, attention=False, loss=False, decode_fp8=True)
    assert not marks() and not any("forward" in m.__dict__ for m in model.modules())      # nothing was patched
    try:
        fl.patch_llama(model, attention=False, loss=False, decode_linears=True)
        assert "_smt_decode_fp8" not in marks()                                           # opt-in: off by default
        fl.patch_llama(model, attention=False, loss=False, decode_linears=True, decode_fp8=True)
        lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
        assert all(m.__dict__.get("_smt_decode_fp8") for m in lin)
        assert all(m.__dict__.get("_smt_decode_fp8") for m in model.modules() if type(m).__name__ == "LlamaMLP")
    finally:
        fl.unpatch_llama(model)
    assert not marks() and not any("forward" in m.__dict__ for m in model.modules())
