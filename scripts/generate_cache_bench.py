"""Time a whole ``generate()`` of a patch_llama-ed model with transformers' default DynamicCache against
``cache_implementation="static"`` (the device-position decode kernel, smt_attn_fwd_cached_pos) and
against ``past_key_values=BeamSharedCache(...)`` (the beam kernel, smt_attn_fwd_beams; K / V are never
reordered or concatenated) and against ``BeamSharedCache(..., graph=True)`` (the same kernels with
the step count on the device, the decode forward captured once and replayed: ``beam_shared_graph``): the
evaluation setting of the reference's run_commonsense_parallel.py in small, 4 left-padded prompts x 4
beams, random-init weights of the bench.py model, ``--new`` tokens (one or more sizes; the reference
generates 256) forced with ``min_new_tokens``.

One JSON line per (cache, size, round): wall seconds of the call between device synchronisations, and ms
per generated token. The four alternate for ``--rounds`` rounds after one untimed call each. The graph
leg's lines also carry ``capture_ms``, the wall time of the capture (torch.cuda.graph around the second
decode forward, the step's own first replay included) measured around it between synchronisations, and
the cache's ``graph_captures`` / ``graph_replays``; its ``seconds`` include the capture. One
``"cache": "ratio"`` line per (size, round) divides the ``beam_shared`` leg by the graph leg. The first
three legs are bound by the host (a decode step is about 500 launches at 32 layers)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MODELS, build_model  # noqa: E402
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import DecodeGraph, patch_llama  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(MODELS))
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, nargs="+", default=[64])
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_cache_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    model = build_model(a.model, dev).eval()
    model.generation_config.pad_token_id = 0
    patch_llama(model)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, MODELS[a.model]["vocab_size"], (a.prompts, a.prompt_len), generator=g)
    mask = torch.ones_like(ids)
    for b in range(a.prompts):                             # left padding: 0, 1/8, 2/8, ... of the prompt
        pad = (b * a.prompt_len) // 8
        ids[b, :pad], mask[b, :pad] = 0, 0
    ids, mask = ids.to(dev), mask.to(dev)
    # the capture's own cost: DecodeGraph.step captures at the cache's second decode step; time that call
    capture = {}
    step = DecodeGraph.step

    def timed_step(self, *args, **kw):
        if self.graph is not None:
            return step(self, *args, **kw)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = step(self, *args, **kw)
        torch.cuda.synchronize()
        capture["ms"] = 1e3 * (time.perf_counter() - t)
        return out
    DecodeGraph.step = timed_step

    for new in a.new:
        kinds = (("dynamic", lambda: {}), ("static", lambda: {"cache_implementation": "static"}),
                 ("beam_shared", lambda: {"past_key_values": BeamSharedCache(model.config, a.beams, new)}),
                 ("beam_shared_graph", lambda: {"past_key_values": BeamSharedCache(model.config, a.beams, new, graph=True)}))

        def run(kw):
            kw = kw()
            torch.cuda.synchronize()
            t = time.perf_counter()
            with torch.no_grad():
                out = model.generate(input_ids=ids, attention_mask=mask, num_beams=a.beams, do_sample=False,
                                     max_new_tokens=new, min_new_tokens=new, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t, out, kw.get("past_key_values")

        outs = {name: run(kw)[1] for name, kw in kinds}    # untimed
        same = {name: bool(torch.equal(outs["dynamic"], o)) for name, o in outs.items()}
        same_graph = bool(torch.equal(outs["beam_shared"], outs["beam_shared_graph"]))
        for rnd in range(a.rounds):
            secs = {}
            for name, kw in kinds:
                s, out, cache = run(kw)
                secs[name] = s
                line = {"cache": name, "round": rnd, "model": a.model, "prompts": a.prompts, "beams": a.beams,
                        "prompt_len": a.prompt_len, "new_tokens": new, "seconds": round(s, 4),
                        "ms_per_token": round(1e3 * s / new, 3), "shape": list(out.shape),
                        "same_tokens_as_dynamic": same[name]}
                if name == "beam_shared_graph":
                    line.update(capture_ms=round(capture["ms"], 2), graph_captures=cache.graph_captures,
                                graph_replays=cache.graph_replays, same_tokens_as_beam_shared=same_graph,
                                ms_per_token_without_capture=round((1e3 * s - capture["ms"]) / new, 3))
                print(json.dumps(line), flush=True)
            print(json.dumps({"cache": "ratio", "round": rnd, "new_tokens": new,
                              "seconds_beam_shared_over_graph": round(secs["beam_shared"] / secs["beam_shared_graph"], 3),
                              "seconds_dynamic_over_graph": round(secs["dynamic"] / secs["beam_shared_graph"], 3)}),
                  flush=True)


if __name__ == "__main__":
    main()
