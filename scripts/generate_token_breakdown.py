"""Where a generated token's time goes in beam search on ``BeamSharedCache(graph=True)``: one profiled
``generate()`` per leg at the evaluation shape of scripts/generate_cache_bench.py (4 left-padded prompts x
4 beams, random-init weights of the bench.py model), split with torch's profiler into
  ``forward``   the model call (prefill once, then the eager, the captured and the replayed decode steps)
  ``scoring``   steps b and c of ``_beam_search``: the ``beam_topk`` call of ``smt_beam_search``
  ``rest``      everything else in the loop: gathers of the running beams, stopping criteria, finished-beam
                bookkeeping, ``reorder_cache``, ``prepare_inputs_for_generation``
Legs: ``torch`` is ``smt_beam_search`` with ``beam_topk_impl="torch"``, transformers' own chain of ops in
transformers' own order (tests/test_beam_search_host.py holds it ``torch.equal`` to ``_beam_search``), and
``hip`` the same loop on the kernel. One JSON line per leg: ``wall_ms_per_token`` of an unprofiled call, then
from the profiled call the host time inside each range (``*_host_ms``; the profiler slows the host, so they
are shares, not end-to-end figures), the device time of all kernels (``device_ms``) and the kernels per
token. Host ranges include waiting for the device where the loop synchronises."""
import argparse
import json
import os
import sys
import time

import torch
from torch.profiler import ProfilerActivity, profile, record_function

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MODELS, build_model  # noqa: E402
from sparse_matrix_tuning_amd import beam_search  # noqa: E402
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import patch_llama  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(MODELS))
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--repetition-penalty", type=float, default=1.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_token_breakdown: needs the GPU")
    dev = torch.device("cuda", 0)
    model = build_model(a.model, dev).eval()
    model.generation_config.pad_token_id = 0
    patch_llama(model)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, MODELS[a.model]["vocab_size"], (a.prompts, a.prompt_len), generator=g)
    mask = torch.ones_like(ids)
    for b in range(a.prompts):
        pad = (b * a.prompt_len) // 8
        ids[b, :pad], mask[b, :pad] = 0, 0
    ids, mask = ids.to(dev), mask.to(dev)

    ranges = []
    model.register_forward_pre_hook(lambda m, args: ranges.append(record_function("smt_forward").__enter__()))
    model.register_forward_hook(lambda m, args, out: ranges.pop().__exit__(None, None, None))
    real = beam_search.beam_topk

    def scoring(*args, **kw):
        with record_function("smt_scoring"):
            return real(*args, **kw)
    beam_search.beam_topk = scoring

    def run(impl):
        cache = BeamSharedCache(model.config, a.beams, a.new, graph=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        with torch.no_grad():
            out = model.generate(input_ids=ids, attention_mask=mask, num_beams=a.beams, do_sample=False,
                                 max_new_tokens=a.new, min_new_tokens=a.new, repetition_penalty=a.repetition_penalty,
                                 past_key_values=cache, custom_generate=beam_search.smt_beam_search, beam_topk_impl=impl)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    outs = {}
    for leg, impl in (("torch", "torch"), ("hip", None)):
        run(impl)                                              # untimed
        wall, outs[leg] = run(impl)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            total, _ = run(impl)
        events = prof.events()
        host = {name: sum(e.cpu_time_total for e in events if e.name == name) / 1e3
                for name in ("smt_forward", "smt_scoring")}
        kernels = [e for e in events if e.device_type == torch.autograd.DeviceType.CUDA]
        line = {"leg": leg, "model": a.model, "prompts": a.prompts, "beams": a.beams, "prompt_len": a.prompt_len,
                "new_tokens": a.new, "repetition_penalty": a.repetition_penalty,
                "wall_ms_per_token": round(1e3 * wall / a.new, 3),
                "profiled_ms_per_token": round(1e3 * total / a.new, 3),
                "forward_host_ms": round(host["smt_forward"] / a.new, 3),
                "scoring_host_ms": round(host["smt_scoring"] / a.new, 3),
                "rest_host_ms": round((1e3 * total - host["smt_forward"] - host["smt_scoring"]) / a.new, 3),
                "device_ms": round(sum(e.device_time_total for e in kernels) / 1e3 / a.new, 3),
                "kernels_per_token": round(len(kernels) / a.new, 1),
                "delegated": beam_search.stats.delegated}
        print(json.dumps(line), flush=True)
    print(json.dumps({"leg": "same_tokens", "hip_equals_torch": bool(torch.equal(outs["hip"], outs["torch"]))}), flush=True)


if __name__ == "__main__":
    main()
