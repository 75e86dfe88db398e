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
three legs are bound by the host (a decode step is about 500 launches at 32 layers).

``--loop transformers smt`` adds the decoding loop as an axis: transformers' ``_beam_search`` and
``custom_generate=smt_beam_search`` (sparse_matrix_tuning_amd/beam_search.py: the scoring of a token as one
smt_beam_topk call). The (cache, loop) legs alternate within a round; every line carries ``loop``, and the
smt legs ``same_tokens_as_transformers_loop`` (the same cache under transformers' loop) and the loop's
``delegated`` count. ``--repetition-penalty 1.1`` is the reference's setting; ``--caches`` picks the legs.

``--decode-linears [all single nogroup noswiglu ...]`` (default ``all`` when given bare) adds, for every
``beam_shared_graph`` leg, the same leg on the model patched with ``patch_llama(decode_linears=True)``: the
decode steps' dense linears on the weight-streaming kernel (``cache`` stays ``beam_shared_graph``, the line's
``decode_linears`` names the variant: ``all`` = q/k/v as one launch and gate/up/SwiGLU as one, ``single`` =
neither, ``nogroup`` / ``noswiglu`` = without the one, ``unbounded*`` = the same without the routing's size
rule, every qualifying launch on the kernel). The routing is put on and taken off between legs
(``route_decode_linears`` / ``unroute_decode_linears``), outside the timing; the leg without the flag runs
the modules as ``patch_llama(model)`` leaves them. The ratio line carries
``seconds_graph_over_<variant>`` per loop.

``--model qwen2-7b`` builds a random-weight Qwen2ForCausalLM of the 7B DeepSeek-R1 distill's shape (28 layers, hidden
3584, Hq 28, Hkv 4, intermediate 18944, vocabulary 152064; q, k and v with a bias) in place of the bench.py model;
every model is patched with ``patch_model``. The ``nobias`` variant of ``--decode-linears`` is ``all`` with the bias
routing off (``DECODE_LINEAR_BIAS``): biased projections then run what they run without the flag.

``--fp8`` adds, for every ``beam_shared_graph`` leg, three legs on a second model of the same weights, frozen,
with ``engine.attach_fp8_weights`` (config 5): ``fp8_base`` = that model as ``patch_llama(model)`` leaves it
(``fp8.quant_rows`` + ``torch._scaled_mm`` per projection: the baseline of the other two), ``fp8`` = with
``patch_llama(decode_linears=True, decode_fp8=True)``'s routing and its ``DECODE_FP8_*`` size rule, and
``fp8_unbounded`` = the same with the rule removed (every qualifying launch on the e4m3 kernel). Their lines carry
``fp8_launches`` (``decode_fp8_stats``) and the ratio line ``seconds_fp8_base_over_<variant>`` per loop.

``--sample`` decodes with ``do_sample=True, temperature=0.6, top_k=50, top_p=0.95`` (run it with ``--beams 1`` and the
rows as ``--prompts``), and ``--loop transformers smt_sample`` puts ``custom_generate=smt_sample``
(sparse_matrix_tuning_amd/sampling.py: the selection of a token as one smt_sample_token call) beside transformers'
``_sample``. The two draw from different streams, so their tokens differ; the ratio line carries
``seconds_<leg>_transformers_over_smt_sample`` for every leg that ran under both."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MODELS, build_model  # noqa: E402
from sparse_matrix_tuning_amd import beam_search, sampling  # noqa: E402
from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache  # noqa: E402
from sparse_matrix_tuning_amd import fused_llama  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import DecodeGraph, patch_model  # noqa: E402

QWEN2 = {"qwen2-7b": dict(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28,
                          num_attention_heads=28, num_key_value_heads=4, rope_theta=10000.0, rms_norm_eps=1e-6,
                          max_position_embeddings=8192, tie_word_embeddings=False, initializer_range=0.02)}

DL_RULE, DL_MAX_K = fused_llama.DECODE_LINEAR_MAX_WEIGHT_ELEMS, fused_llama.DECODE_LINEAR_MAX_K
# variant: (q/k/v as one launch, gate/up/SwiGLU as one launch, the size rule's limit)
DL_VARIANTS = {"all": (True, True, DL_RULE), "single": (False, False, DL_RULE), "nogroup": (False, True, DL_RULE),
               "noswiglu": (True, False, DL_RULE), "unbounded": (True, True, 1 << 62),
               "unbounded_single": (False, False, 1 << 62), "unbounded_nogroup": (False, True, 1 << 62),
               "unbounded_noswiglu": (True, False, 1 << 62), "nobias": (True, True, DL_RULE)}
FP8_VARIANTS = {"fp8_base": None, "fp8": True, "fp8_unbounded": False}      # variant: DECODE_FP8_RULE (None: unrouted)


def build_qwen2(name, device):
    """bench.build_model's recipe for a Qwen2 shape; the q/k/v biases, which transformers zeroes, are drawn too."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(**QWEN2[name])
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(1234)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(device):
            model = Qwen2ForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("_proj.bias"):
                p.normal_(0.0, 0.02)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(MODELS) + sorted(QWEN2))
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, nargs="+", default=[64])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--loop", nargs="+", default=["transformers"], choices=["transformers", "smt", "smt_sample"])
    ap.add_argument("--sample", action="store_true", help="do_sample=True, temperature 0.6, top_k 50, top_p 0.95")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--caches", nargs="+", default=["dynamic", "static", "beam_shared", "beam_shared_graph"],
                    choices=["dynamic", "static", "beam_shared", "beam_shared_graph"])
    ap.add_argument("--decode-linears", nargs="*", default=None, choices=sorted(DL_VARIANTS),
                    help="add beam_shared_graph legs on a model patched with decode_linears=True")
    ap.add_argument("--fp8", action="store_true",
                    help="add beam_shared_graph legs on a frozen model with attach_fp8_weights: " + " ".join(FP8_VARIANTS))
    a = ap.parse_args()
    if a.decode_linears is not None and not a.decode_linears:
        a.decode_linears = ["all"]
    if not torch.cuda.is_available():
        raise SystemExit("generate_cache_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    if a.fp8 and a.model in QWEN2:
        raise SystemExit("generate_cache_bench: --fp8 runs on the bench.py models")
    model = (build_qwen2 if a.model in QWEN2 else build_model)(a.model, dev).eval()
    model.generation_config.pad_token_id = 0
    patch_model(model)
    fp8_model = None
    if a.fp8:
        from sparse_matrix_tuning_amd import engine
        fp8_model = build_model(a.model, dev).eval()          # the same seed: the same weights
        fp8_model.generation_config.pad_token_id = 0
        for p in fp8_model.parameters():
            p.requires_grad_(False)
        engine.attach_fp8_weights(fp8_model)
        patch_model(fp8_model)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, model.config.vocab_size, (a.prompts, a.prompt_len), generator=g)
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
        caches = {"dynamic": lambda: {}, "static": lambda: {"cache_implementation": "static"},
                  "beam_shared": lambda: {"past_key_values": BeamSharedCache(model.config, a.beams, new)},
                  "beam_shared_graph": lambda: {"past_key_values": BeamSharedCache(model.config, a.beams, new, graph=True)}}
        extra = {} if a.repetition_penalty == 1.0 else {"repetition_penalty": a.repetition_penalty}
        loops = {"transformers": {}, "smt": {"custom_generate": beam_search.smt_beam_search},
                 "smt_sample": {"custom_generate": sampling.smt_sample, "sample_seed": 1}}
        mode = dict(do_sample=True, temperature=0.6, top_k=50, top_p=0.95) if a.sample else dict(do_sample=False)
        leg = lambda cache, loop: cache if loop == "transformers" else f"{cache}+{loop}"
        variants = lambda c: [None] + ((list(a.decode_linears or ()) + (list(FP8_VARIANTS) if a.fp8 else []))
                                       if c == "beam_shared_graph" else [])
        kinds = tuple((leg(c if v is None else f"{c}@{v}", lp), (lambda c=c, lp=lp: {**caches[c](), **loops[lp], **extra}))
                      for c in a.caches for v in variants(c) for lp in a.loop)
        first = kinds[0][0]
        variant_of = lambda name: name.split("+")[0].partition("@")[2] or None
        routed = {"now": None}

        def route(v):
            """The model patched for variant ``v`` (None: without the decode linears)."""
            if v != routed["now"]:
                fused_llama.unroute_decode_linears(model)
                if fp8_model is not None:
                    fused_llama.unroute_decode_linears(fp8_model)
                if v in FP8_VARIANTS:
                    if FP8_VARIANTS[v] is not None:
                        fused_llama.route_decode_linears(fp8_model, fp8=True)
                        fused_llama.DECODE_FP8_RULE = FP8_VARIANTS[v]
                        (fused_llama.DECODE_LINEAR_GROUP, fused_llama.DECODE_LINEAR_SWIGLU,
                         fused_llama.DECODE_LINEAR_MAX_WEIGHT_ELEMS) = DL_VARIANTS["all"]
                        fused_llama.DECODE_LINEAR_MAX_K = DL_MAX_K
                elif v is not None:
                    fused_llama.route_decode_linears(model)
                    (fused_llama.DECODE_LINEAR_GROUP, fused_llama.DECODE_LINEAR_SWIGLU,
                     fused_llama.DECODE_LINEAR_MAX_WEIGHT_ELEMS) = DL_VARIANTS[v]
                    fused_llama.DECODE_LINEAR_MAX_K = DL_MAX_K if DL_VARIANTS[v][2] == DL_RULE else 1 << 30
                    fused_llama.DECODE_LINEAR_BIAS = v != "nobias"
                routed["now"] = v

        def run(kw, v=None):
            route(v)
            kw = kw()
            fused_llama.decode_linear_stats.reset()
            fused_llama.decode_fp8_stats.reset()
            beam_search.stats.reset()
            sampling.stats.reset()
            m = fp8_model if v in FP8_VARIANTS else model
            torch.cuda.synchronize()
            t = time.perf_counter()
            with torch.no_grad():
                out = m.generate(input_ids=ids, attention_mask=mask, num_beams=a.beams, max_new_tokens=new,
                                 min_new_tokens=new, **mode, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t, out, kw.get("past_key_values")

        outs = {name: run(kw, variant_of(name))[1] for name, kw in kinds}    # untimed
        same = {name: bool(torch.equal(outs[first], o)) for name, o in outs.items()}
        same_graph = ("beam_shared" in outs and "beam_shared_graph" in outs
                      and bool(torch.equal(outs["beam_shared"], outs["beam_shared_graph"])))
        for rnd in range(a.rounds):
            secs = {}
            for name, kw in kinds:
                s, out, cache = run(kw, variant_of(name))
                secs[name] = s
                line = {"cache": name.split("+")[0].split("@")[0], "loop": name.partition("+")[2] or "transformers",
                        "repetition_penalty": a.repetition_penalty,
                        "round": rnd, "model": a.model, "prompts": a.prompts, "beams": a.beams,
                        "prompt_len": a.prompt_len, "new_tokens": new, "seconds": round(s, 4),
                        "ms_per_token": round(1e3 * s / new, 3), "shape": list(out.shape),
                        f"same_tokens_as_{first}": same[name]}
                if a.decode_linears is not None or a.fp8:
                    line.update(decode_linears=variant_of(name), routed_launches=fused_llama.decode_linear_stats.as_dict(),
                                biased_launches=fused_llama.decode_linear_stats.bias)
                    if variant_of(name) in FP8_VARIANTS:
                        line.update(fp8_launches=fused_llama.decode_fp8_stats.as_dict())
                    base = name.replace("@" + str(variant_of(name)), "@fp8_base" if variant_of(name) in FP8_VARIANTS else "")
                    if variant_of(name) is not None and base in outs:
                        line.update(same_tokens_as_unrouted=bool(torch.equal(outs[base], outs[name])))
                if "+" in name:
                    line.update(delegated=(sampling if name.endswith("+smt_sample") else beam_search).stats.delegated)
                    if name.split("+")[0] in outs:
                        line.update(same_tokens_as_transformers_loop=bool(torch.equal(outs[name.split("+")[0]], outs[name])))
                if name.startswith("beam_shared_graph"):
                    line.update(capture_ms=round(capture["ms"], 2), graph_captures=cache.graph_captures,
                                graph_replays=cache.graph_replays, same_tokens_as_beam_shared=same_graph,
                                ms_per_token_without_capture=round((1e3 * s - capture["ms"]) / new, 3))
                print(json.dumps(line), flush=True)
            ratio = {"cache": "ratio", "round": rnd, "new_tokens": new}
            if "beam_shared_graph" in secs:
                for other in ("beam_shared", "dynamic"):
                    if other in secs:
                        ratio[f"seconds_{other}_over_graph"] = round(secs[other] / secs["beam_shared_graph"], 3)
            for v in a.decode_linears or ():
                for lp in a.loop:
                    base, dl = leg("beam_shared_graph", lp), leg(f"beam_shared_graph@{v}", lp)
                    if base in secs and dl in secs:
                        ratio[f"seconds_graph_over_{v}" + ("" if lp == "transformers" else "_" + lp)] = round(secs[base] / secs[dl], 3)
            for v in (v for v in FP8_VARIANTS if a.fp8 and v != "fp8_base"):
                for lp in a.loop:
                    base, dl = leg("beam_shared_graph@fp8_base", lp), leg(f"beam_shared_graph@{v}", lp)
                    if base in secs and dl in secs:
                        ratio[f"seconds_fp8_base_over_{v}" + ("" if lp == "transformers" else "_" + lp)] = round(secs[base] / secs[dl], 3)
            for c in a.caches:
                if c in secs and c + "+smt" in secs:
                    ratio[f"seconds_{c}_transformers_over_smt"] = round(secs[c] / secs[c + "+smt"], 3)
            for name in secs:
                if name + "+smt_sample" in secs:
                    ratio[f"seconds_{name}_transformers_over_smt_sample"] = round(secs[name] / secs[name + "+smt_sample"], 3)
            print(json.dumps(ratio), flush=True)


if __name__ == "__main__":
    main()
