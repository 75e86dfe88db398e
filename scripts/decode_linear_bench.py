"""Time the decode-linear kernel (smt_linear_skinny, include/smt_linear.h) against torch.matmul (hipBLASLt)
on the same tensors at the dense-linear shapes of a decode step, M = 1, 4 and 16 rows, bf16:

  LLaMA-3-8B   q/o 4096x4096, k/v 1024x4096, q+k+v as one grouped launch (6144x4096), gate or up 14336x4096
               alone and as the SwiGLU pair, down 4096x14336, the head 128256x4096
  LLaMA-2-13B  5120x5120, 13824x5120, 5120x13824
  Qwen2 1.5B   q/o 1536x1536, k/v 256x1536, q+k+v grouped (2048x1536)      (the DeepSeek-R1 distills' shapes)
  Qwen2 7B     q/o 3584x3584, k/v 512x3584, q+k+v grouped (4608x3584)

``--bias`` gives every weight of a ``single`` or ``group`` row a bias, as Qwen2's q, k and v have one: the kernel's
bias epilogue (smt_linear_skinny_bias) against ``F.linear(x, W, b)`` per projection, which is what the unrouted
model runs. The lines carry ``bias: true``; SwiGLU rows have no biased form and are skipped.

``--impl matmul`` times the baseline alone: how far hipBLASLt is from a plain weight stream at these shapes.
``--impl both`` alternates the two for ``--rounds`` rounds in one process. For a grouped or SwiGLU row the
baseline is what the model runs today: one torch.matmul per weight, and for SwiGLU the fused SwiGLU forward
after them.

Every call takes the next of a ring of weight copies larger than the 256 MiB Infinity Cache, as the layers
of a model do, so the bytes come from HBM. ``kernel_us`` is the summed device time of the kernels one call
launches (torch.profiler); ``frac_8TBps`` the weight bytes over it as a fraction of 8 TB/s. One JSON line per
(shape, M, impl, round) (``kind: sample``) and per (shape, M) (``kind: row``): both medians, the per-round
ratio matmul / smt, and the baseline's own spread (max - min of its rounds, over its median)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd import _hip  # noqa: E402
from sparse_matrix_tuning_amd import fused_llama as fl  # noqa: E402

SHAPES = [
    ("8b.qo", "single", [4096], 4096), ("8b.kv", "single", [1024], 4096), ("8b.qkv", "group", [4096, 1024, 1024], 4096),
    ("8b.gate", "single", [14336], 4096), ("8b.gate_up", "swiglu", [14336, 14336], 4096),
    ("8b.down", "single", [4096], 14336), ("8b.head", "single", [128256], 4096),
    ("13b.qo", "single", [5120], 5120), ("13b.gate", "single", [13824], 5120), ("13b.down", "single", [5120], 13824),
    ("qwen1.5b.qo", "single", [1536], 1536), ("qwen1.5b.kv", "single", [256], 1536),
    ("qwen1.5b.qkv", "group", [1536, 256, 256], 1536),
    ("qwen7b.qo", "single", [3584], 3584), ("qwen7b.kv", "single", [512], 3584), ("qwen7b.qkv", "group", [3584, 512, 512], 3584),
]


def kernel_us(fn, iters):
    """(summed device us per call, {kernel name: us per call}) of the kernels fn launches."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t > 0:
            out[ev.key[:48]] = round(t / iters, 2)
    return sum(out.values()), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", default="both", choices=["both", "matmul", "smt"])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--shapes", nargs="*", default=None, help="names out of: " + " ".join(s[0] for s in SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--ring-bytes", type=float, default=320e6, help="least total bytes of the weight copies a run cycles through")
    ap.add_argument("--bias", action="store_true", help="every weight with a bias: the bias epilogue against F.linear")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_linear_bench: needs the GPU (a timing from anywhere else says nothing)")
    _hip.load()
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    torch.manual_seed(0)
    impls = ["matmul", "smt"] if a.impl == "both" else [a.impl]
    for name, kind, Ns, K in SHAPES:
        if (a.shapes and name not in a.shapes) or (a.bias and kind == "swiglu"):
            continue
        wbytes = sum(Ns) * K * 2
        n = max(2, int(a.ring_bytes // wbytes) + 1)
        ring = [[torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for N in Ns] for _ in range(n)]
        bias_ring = [[torch.randn(N, device="cuda", dtype=torch.bfloat16) if a.bias else None for N in Ns] for _ in range(n)]
        state = {"i": 0}

        def weights():
            state["i"] = (state["i"] + 1) % n
            return ring[state["i"]]

        def biases():                                        # of the weights the last weights() returned
            return bias_ring[state["i"]]

        for M in a.M:
            x = torch.randn(M, 1, K, device="cuda", dtype=torch.bfloat16)

            def matmul():
                ws = weights()
                if a.bias:
                    return [torch.nn.functional.linear(x, w, b) for w, b in zip(ws, biases())]
                ys = [torch.matmul(x, w.t()) for w in ws]
                return fl.FusedSwiGLUFn.apply(*ys) if kind == "swiglu" else ys

            def smt():
                ws = weights()
                if kind == "swiglu":
                    return fl.decode_swiglu(x, *ws)
                bs = biases()
                return fl.decode_linear_group(x, ws, bs) if kind == "group" else [fl.decode_linear(x, ws[0], bs[0])]

            fns = {"matmul": matmul, "smt": smt}
            samples = {i: [] for i in impls}
            with torch.no_grad():
                for rnd in range(a.rounds):
                    for impl in impls:
                        us, kernels = kernel_us(fns[impl], a.iters)
                        samples[impl].append(us)
                        emit({"kind": "sample", "shape": name, "op": kind, "bias": a.bias, "N": Ns, "K": K, "M": M, "impl": impl, "round": rnd,
                              "kernel_us": round(us, 2), "frac_8TBps": round(wbytes / (us * 1e-6) / 8e12, 3),
                              "weight_bytes": wbytes, "copies": n, "kernels": kernels})
            row = {"kind": "row", "shape": name, "op": kind, "bias": a.bias, "N": Ns, "K": K, "M": M, "weight_bytes": wbytes}
            for impl in impls:
                med = statistics.median(samples[impl])
                row[impl + "_us"] = [round(v, 2) for v in samples[impl]]
                row[impl + "_median_us"] = round(med, 2)
                row[impl + "_frac_8TBps"] = round(wbytes / (med * 1e-6) / 8e12, 3)
            if "matmul" in samples:
                b = samples["matmul"]
                row["matmul_spread"] = round((max(b) - min(b)) / statistics.median(b), 3)
            if len(impls) == 2:
                row["matmul_over_smt"] = [round(b / s, 3) for b, s in zip(samples["matmul"], samples["smt"])]
                row["smt_faster_every_round"] = all(s < b for b, s in zip(samples["matmul"], samples["smt"]))
            emit(row)
        del ring, bias_ring
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
