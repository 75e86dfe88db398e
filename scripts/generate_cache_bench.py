"""Time a whole ``generate()`` of a patch_llama-ed model with transformers' default DynamicCache against
``cache_implementation="static"`` (the device-position decode kernel, smt_attn_fwd_cached_pos) and
against ``past_key_values=BeamSharedCache(...)`` (the beam kernel, smt_attn_fwd_beams; K / V are never
reordered or concatenated): the
evaluation setting of the reference's run_commonsense_parallel.py in small, 4 left-padded prompts x 4
beams, random-init weights of the bench.py model, ``--new`` tokens forced with ``min_new_tokens``.

One JSON line per (cache, round): wall seconds of the call between device synchronisations, and ms per
generated token. The three alternate for ``--rounds`` rounds after one untimed call each. All are bound
by the host (a decode step is about 500 launches at 32 layers); nothing here is captured in a graph."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MODELS, build_model  # noqa: E402
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import patch_llama  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(MODELS))
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, default=64)
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
    kinds = (("dynamic", lambda: {}), ("static", lambda: {"cache_implementation": "static"}),
             ("beam_shared", lambda: {"past_key_values": BeamSharedCache(model.config, a.beams, a.new)}))

    def run(kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with torch.no_grad():
            out = model.generate(input_ids=ids, attention_mask=mask, num_beams=a.beams, do_sample=False,
                                 max_new_tokens=a.new, min_new_tokens=a.new, **kw())
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    outs = {name: run(kw)[1] for name, kw in kinds}        # untimed
    same = {name: bool(torch.equal(outs["dynamic"], o)) for name, o in outs.items()}
    for rnd in range(a.rounds):
        for name, kw in kinds:
            s, out = run(kw)
            print(json.dumps({"cache": name, "round": rnd, "model": a.model, "prompts": a.prompts, "beams": a.beams,
                              "prompt_len": a.prompt_len, "new_tokens": a.new, "seconds": round(s, 4),
                              "ms_per_token": round(1e3 * s / a.new, 3), "shape": list(out.shape),
                              "same_tokens_as_dynamic": same[name]}), flush=True)


if __name__ == "__main__":
    main()
