"""Time one beam-search scoring step: ``beam_topk`` on the kernel (smt_beam_topk, three launches) against
``impl="torch"``, transformers' chain of ops (float copy, log_softmax, the repetition penalty's gather /
where / scatter, the add, topk), at the evaluation shape: R 16 = 4 prompts x 4 beams, V 128256, bf16,
repetition penalty 1.1, K 8 and 16, history 256 and 512 tokens.

One JSON line per (impl, K, cur_len, round); the two alternate within a round, for ``--rounds`` rounds,
after one warm-up of each. Per call:
  ``device_us``   sum of the kernels' durations from torch's profiler (its own run of ``--profiled`` calls)
  ``launches``    device kernels per call in that run
  ``host_us``     host clock around ``--calls`` back-to-back calls without a synchronise: the enqueue cost
  ``wall_us``     host clock around the same calls up to the synchronise that ends them
One ``"impl": "ratio"`` line per (K, cur_len, round) divides torch by kernel. Both pick the same indices
(``same_index``) on the seeded input, or the line says so."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd.beam_search import beam_topk  # noqa: E402


def device_time(fn, calls):
    """(sum of device kernel time per call in us, kernels per call) from torch's profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    total = sum(e.device_time_total for e in kernels)
    return total / calls, len(kernels) / calls


def host_time(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e6 * (t1 - t0) / calls, 1e6 * (t2 - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--cur-len", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--penalty", type=float, default=1.1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--profiled", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_topk_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rows = a.prompts * a.beams
    logits = (torch.randn(rows, a.vocab, generator=g) * 2).bfloat16().to(dev)
    scores = (-torch.rand(rows, generator=g) * 4).to(dev)
    history = torch.randint(0, a.vocab, (rows, max(a.cur_len)), generator=g).to(dev)
    for k in a.k:
        for cur_len in a.cur_len:
            fns = {impl: (lambda impl=impl: beam_topk(logits, scores, history, cur_len, a.beams, k,
                                                       repetition_penalty=a.penalty, impl=impl))
                   for impl in ("hip", "torch")}
            outs = {impl: fn() for impl, fn in fns.items()}                  # warm-up
            same = bool(torch.equal(outs["hip"][1], outs["torch"][1]))
            err = float((outs["hip"][0] - outs["torch"][0]).abs().max())
            for rnd in range(a.rounds):
                res = {}
                for impl, fn in fns.items():
                    dev_us, launches = device_time(fn, a.profiled)
                    host_us, wall_us = host_time(fn, a.calls)
                    res[impl] = (dev_us, host_us, wall_us)
                    print(json.dumps({"impl": impl, "round": rnd, "rows": rows, "vocab": a.vocab, "k": k,
                                      "cur_len": cur_len, "penalty": a.penalty, "dtype": "bf16",
                                      "device_us": round(dev_us, 2), "launches": round(launches, 2),
                                      "host_us": round(host_us, 2), "wall_us": round(wall_us, 2), "calls": a.calls,
                                      "same_index": same, "max_score_diff": err}), flush=True)
                print(json.dumps({"impl": "ratio", "round": rnd, "k": k, "cur_len": cur_len,
                                  "device_torch_over_hip": round(res["torch"][0] / res["hip"][0], 2),
                                  "host_torch_over_hip": round(res["torch"][1] / res["hip"][1], 2),
                                  "wall_torch_over_hip": round(res["torch"][2] / res["hip"][2], 2)}), flush=True)


if __name__ == "__main__":
    main()
