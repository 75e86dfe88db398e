"""Time one token selection for ``num_beams == 1``: ``sample_token`` on the kernel (smt_sample_token, two
launches) against what transformers' ``_sample`` runs between the logits and the token -- the float copy,
its processor list (repetition penalty, temperature, top-k, top-p, min-p), ``softmax`` and
``torch.multinomial`` (or ``argmax``) -- at the decoding shape: R 16, V 128256 and 152064, bf16, repetition
penalty 1.1 with a 512-token history. Settings: (T 0.6, k 50, p 0.95), (k 0, p 0.95), (k 0, p 1, min-p 0.05), greedy.

One JSON line per (impl, vocab, setting, round); the two alternate within a round, for ``--rounds`` rounds,
after one warm-up of each. Per call:
  ``device_us``   sum of the kernels' durations from torch's profiler (its own run of ``--profiled`` calls)
  ``launches``    device kernels per call in that run
  ``host_us``     host clock around ``--calls`` back-to-back calls without a synchronise: the enqueue cost
  ``wall_us``     host clock around the same calls up to the synchronise that ends them
One ``"impl": "ratio"`` line per (vocab, setting, round) divides the chain by the kernel. ``kept_mean`` is the
kernel's mean kept-set size; ``same_kept`` says whether the chain keeps as many tokens in every row (on bf16
logits the contract may keep more: a whole group of equal values at the top-p threshold)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd.sampling import sample_token  # noqa: E402

SETTINGS = {
    "T0.6_k50_p0.95": dict(do_sample=True, temperature=0.6, top_k=50, top_p=0.95, min_p=0.0),
    "k0_p0.95": dict(do_sample=True, temperature=1.0, top_k=0, top_p=0.95, min_p=0.0),
    "k0_p1_minp0.05": dict(do_sample=True, temperature=1.0, top_k=0, top_p=1.0, min_p=0.05),
    "greedy": dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0),
}


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


def chain(logits, history, penalty, s):
    """transformers' ``_sample`` between ``outputs.logits[:, -1]`` and ``next_tokens``; returns the tokens
    and the processed scores."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinPLogitsWarper,
                                                        RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    procs = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=penalty)])
    if s["do_sample"]:
        if s["temperature"] != 1.0:
            procs.append(TemperatureLogitsWarper(s["temperature"]))
        if s["top_k"]:
            procs.append(TopKLogitsWarper(top_k=s["top_k"]))
        if s["top_p"] < 1.0:
            procs.append(TopPLogitsWarper(top_p=s["top_p"]))
        if s["min_p"] > 0.0:
            procs.append(MinPLogitsWarper(min_p=s["min_p"]))

    def fn():
        scores = procs(history, logits.to(copy=True, dtype=torch.float32))
        if s["do_sample"]:
            return torch.multinomial(torch.nn.functional.softmax(scores, dim=-1), num_samples=1).squeeze(1), scores
        return torch.argmax(scores, dim=-1), scores
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, nargs="+", default=[128256, 152064])
    ap.add_argument("--cur-len", type=int, default=512)
    ap.add_argument("--penalty", type=float, default=1.1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--profiled", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    for vocab in a.vocab:
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(a.rows, vocab, generator=g) * 2).bfloat16().to(dev)
        history = torch.randint(0, vocab, (a.rows, a.cur_len), generator=g).to(dev)
        for name, s in SETTINGS.items():
            fns = {"hip": lambda s=s: sample_token(logits, history, a.cur_len, repetition_penalty=a.penalty, seed=1, step=a.cur_len,
                                                   impl="hip", **s),
                   "torch": chain(logits, history, a.penalty, s)}
            outs = {impl: fn() for impl, fn in fns.items()}                  # warm-up
            kept = outs["hip"][2].float()
            same = bool(torch.equal((outs["torch"][1] > -float("inf")).sum(dim=1).int(), outs["hip"][2]))
            for rnd in range(a.rounds):
                res = {}
                for impl, fn in fns.items():
                    dev_us, launches = device_time(fn, a.profiled)
                    host_us, wall_us = host_time(fn, a.calls)
                    res[impl] = (dev_us, host_us, wall_us)
                    print(json.dumps({"impl": impl, "round": rnd, "rows": a.rows, "vocab": vocab, "setting": name,
                                      "cur_len": a.cur_len, "penalty": a.penalty, "dtype": "bf16",
                                      "device_us": round(dev_us, 2), "launches": round(launches, 2),
                                      "host_us": round(host_us, 2), "wall_us": round(wall_us, 2), "calls": a.calls,
                                      "kept_mean": round(float(kept.mean()), 1), "same_kept": same}), flush=True)
                print(json.dumps({"impl": "ratio", "round": rnd, "vocab": vocab, "setting": name,
                                  "device_torch_over_hip": round(res["torch"][0] / res["hip"][0], 2),
                                  "host_torch_over_hip": round(res["torch"][1] / res["hip"][1], 2),
                                  "wall_torch_over_hip": round(res["torch"][2] / res["hip"][2], 2)}), flush=True)


if __name__ == "__main__":
    main()
