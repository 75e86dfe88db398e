"""Time the e4m3 decode-linear kernel (smt_linear_skinny_fp8, include/smt_linear.h) against the route an fp8
model's decode step takes today (fp8.quant_rows where the e4m3 copy of the activation is not already there,
then torch._scaled_mm with rowwise scales, one per weight) on the same tensors, M = 1, 4 and 16 rows, at the
decoder shapes of scripts/decode_linear_bench.py (the head stays bf16 in the fp8 path and is not here):

  LLaMA-3-8B   q 4096x4096 and k/v 1024x4096 alone and as the grouped launch (6144x4096), o 4096x4096, gate
               14336x4096 alone and gate + up as the SwiGLU pair, down 4096x14336
  LLaMA-2-13B  q 5120x5120, gate 13824x5120, down 5120x13824

What each row pays for the activation's e4m3 copy is what the model pays there. q, k/v, the group, gate and the
pair read the copy the fused RMSNorm left (neither route launches a quantisation). o_proj's input comes from the
attention: both routes launch smt_quant_rows_e4m3. down_proj's input: today's route gets it from the SwiGLU
kernel that also quantises (smt_swiglu_fwd_quant_e4m3, counted in the pair's row), the kernel's route gets bf16
from its SwiGLU epilogue and launches the quantisation, so the down row charges it to the kernel alone.

``--impl scaled_mm`` times today's route alone; ``--impl both`` alternates the two for ``--rounds`` rounds in
one process. Method as scripts/decode_linear_bench.py: every call takes the next of a ring of weight copies
larger than the 256 MiB Infinity Cache; ``kernel_us`` is the summed device time of the kernels one call launches
(torch.profiler); ``frac_8TBps`` the e4m3 weight bytes over it as a fraction of 8 TB/s. One JSON line per (shape,
M, impl, round) (``kind: sample``) and per (shape, M) (``kind: row``): medians, the per-round ratio scaled_mm / smt,
the baseline's own spread (max - min of its rounds over its median), and ``admit``: the kernel was faster in every
round and its smallest margin was larger than that spread."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd import _hip  # noqa: E402
from sparse_matrix_tuning_amd import fp8 as f8  # noqa: E402
from sparse_matrix_tuning_amd import fused_llama as fl  # noqa: E402
from scripts.decode_linear_bench import kernel_us  # noqa: E402

# (name, kind, Ns, K, today's route quantises x, the kernel's route quantises x)
SHAPES = [
    ("8b.q", "single", [4096], 4096, False, False), ("8b.kv", "single", [1024], 4096, False, False),
    ("8b.qkv", "group", [4096, 1024, 1024], 4096, False, False), ("8b.o", "single", [4096], 4096, True, True),
    ("8b.gate", "single", [14336], 4096, False, False), ("8b.gate_up", "swiglu", [14336, 14336], 4096, False, False),
    ("8b.down", "single", [4096], 14336, False, True),
    ("13b.q", "single", [5120], 5120, False, False), ("13b.gate", "single", [13824], 5120, False, False),
    ("13b.down", "single", [5120], 13824, False, True),
]


def fp8_weight(N, K):
    w8, sw = f8.quant_rows(torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02)
    return SimpleNamespace(w8=w8, sw=sw, sw_row=sw.view(1, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", default="both", choices=["both", "scaled_mm", "smt"])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--shapes", nargs="*", default=None, help="names out of: " + " ".join(s[0] for s in SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--ring-bytes", type=float, default=320e6, help="least total bytes of the weight copies a run cycles through")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_linear_fp8_bench: needs the GPU (a timing from anywhere else says nothing)")
    _hip.load()
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    torch.manual_seed(0)
    impls = ["scaled_mm", "smt"] if a.impl == "both" else [a.impl]
    for name, kind, Ns, K, base_quant, smt_quant in SHAPES:
        if a.shapes and name not in a.shapes:
            continue
        wbytes = sum(Ns) * K
        n = max(2, int(a.ring_bytes // wbytes) + 1)
        ring = [[fp8_weight(N, K) for N in Ns] for _ in range(n)]
        state = {"i": 0}

        def weights():
            state["i"] = (state["i"] + 1) % n
            return ring[state["i"]]

        for M in a.M:
            x = torch.randn(M, 1, K, device="cuda", dtype=torch.bfloat16)
            x2 = x.view(M, K)
            cached = f8.quant_rows(x2)

            def scaled_mm():
                a_q = f8.quant_rows(x2) if base_quant else cached
                ys = [f8.fp8_matmul(None, fw.w8, fw.sw_row, a_q=a_q) for fw in weights()]
                return f8.swiglu_fwd_quant(ys[0], ys[1], False) if kind == "swiglu" else ys

            def smt():
                ws = weights()
                if smt_quant:
                    x.__dict__.pop("_smt_q8", None)
                else:
                    x._smt_q8 = (x._version, *cached)
                if kind == "swiglu":
                    return fl.decode_swiglu_fp8(x, *ws)
                return fl.decode_linear_group_fp8(x, ws) if kind == "group" else [fl.decode_linear_fp8(x, ws[0])]

            fns = {"scaled_mm": scaled_mm, "smt": smt}
            samples = {i: [] for i in impls}
            errors = {}
            with torch.no_grad():
                for rnd in range(a.rounds):
                    for impl in impls:
                        if impl in errors:
                            continue
                        try:
                            us, kernels = kernel_us(fns[impl], a.iters)
                        except RuntimeError as e:            # a shape the library refuses is a result, not a crash
                            errors[impl] = str(e).splitlines()[0][:200]
                            continue
                        samples[impl].append(us)
                        emit({"kind": "sample", "shape": name, "op": kind, "N": Ns, "K": K, "M": M, "impl": impl, "round": rnd,
                              "kernel_us": round(us, 2), "frac_8TBps": round(wbytes / (us * 1e-6) / 8e12, 3),
                              "weight_bytes": wbytes, "copies": n, "quant_launch": base_quant if impl == "scaled_mm" else smt_quant,
                              "kernels": kernels})
            row = {"kind": "row", "shape": name, "op": kind, "N": Ns, "K": K, "M": M, "weight_bytes": wbytes,
                   "quant_launch": {"scaled_mm": base_quant, "smt": smt_quant}}
            if errors:
                row["errors"] = errors
            for impl in impls:
                if samples[impl]:
                    med = statistics.median(samples[impl])
                    row[impl + "_us"] = [round(v, 2) for v in samples[impl]]
                    row[impl + "_median_us"] = round(med, 2)
                    row[impl + "_frac_8TBps"] = round(wbytes / (med * 1e-6) / 8e12, 3)
            b, s = samples.get("scaled_mm", []), samples.get("smt", [])
            if b:
                row["scaled_mm_spread"] = round((max(b) - min(b)) / statistics.median(b), 3)
            if b and s and len(b) == len(s):
                row["scaled_mm_over_smt"] = [round(x_ / y_, 3) for x_, y_ in zip(b, s)]
                row["smt_faster_every_round"] = all(y_ < x_ for x_, y_ in zip(b, s))
                margin = min((x_ - y_) / statistics.median(b) for x_, y_ in zip(b, s))
                row["smallest_margin"] = round(margin, 3)
                row["admit"] = bool(row["smt_faster_every_round"] and margin > row["scaled_mm_spread"])
            emit(row)
        del ring
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
