"""Time one decode step of beam search, cache work plus attention, for one layer: today's route
(transformers' DynamicCache: ``index_select`` of K and V by beam_idx, ``torch.cat`` of the step's K / V,
then smt_attn_fwd_cached through fused_llama.flash_attention_cached) against the beam-shared cache
(the ancestry-table update, the in-place write of the step's K / V, then smt_attn_fwd_beams through
fused_llama.flash_attention_beams), at the evaluation shape of the reference's
run_commonsense_parallel.py: N = 4 prompts x nb = 4 beams = 16 rows, Hq 32, Hkv 8, bf16, prompt
lengths P in {256, 1024} and T in {1, 128, 256} generated positions (the current token's included).

One JSON line per (P, T, impl, round); the two routes and the two bare kernels alternate ``--rounds``
times (default 2), and one ``"impl": "ratio"`` line per (P, T, round) divides them:
  ``dyn_step``      index_select + cat + flash_attention_cached on [16, Hkv, P + T, 128]
  ``beam_step``     ancestry update + K / V write + flash_attention_beams (the ancestry update runs once
                    per token for all layers in BeamSharedCache; here every call pays it)
  ``cached_kernel`` flash_attention_cached alone on the gathered [16, Hkv, P + T, 128] cache
  ``beam_kernel``   flash_attention_beams alone on the beam-shared buffers (the same keys), at the default
                    split count; ``beam_kernel@N`` (``--splits``): at N splits
``us`` = device-event time per call over back-to-back calls (includes whatever the host cannot enqueue
fast enough), ``kernel_us`` = the summed device time of the kernels one call launches (torch.profiler),
``kernels`` = that sum by kernel. ``rel_diff`` (kernel lines): the two kernels' results against each
other. Every call takes the next of a ring of K / V copies larger than the 256 MB Infinity Cache, as
the layers of a model do, so the bytes come from HBM (``kv_copies``).

``--pos`` times the device-counter form in place of the DynamicCache comparison (T is then a fill level
of the ``--T-cap`` buffers; profiles/r15_beam_decode_step_pos.jsonl):
  ``beam_kernel``        as above: host T, the default split count of (P, T)
  ``beam_kernel@cap``    host T at the split count the capacity gives (``splits``), which is what the
                         device-counter call runs with: the cost of the capacity-sized split count alone
  ``beam_kernel_pos``    flash_attention_beams with gen_len a device tensor (smt_attn_fwd_beams_pos)
  ``beam_step``          ancestry update + two slice copies + the host-T kernel
  ``beam_step_pos``      ancestry update + kv_append (smt_attn_kv_append_pos) + the device-counter kernel
and one ``"impl": "pos_ratio"`` line per (P, T, round). ``bit_identical``: beam_kernel_pos against
beam_kernel@cap on the same buffers."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd import _hip  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import flash_attention_beams, flash_attention_cached, kv_append  # noqa: E402
from attn_decode_bench import kernel_us, timed  # noqa: E402


def genealogy(N, nb, T, T_cap, seed):
    """uint8 [N * nb, T_cap] after T steps of a simulated beam search (random within-sample beam_idx)."""
    g = torch.Generator().manual_seed(seed)
    R = N * nb
    anc = (torch.arange(R) % nb).to(torch.uint8)[:, None].repeat(1, T_cap)
    base = torch.arange(R) // nb * nb
    for t in range(1, T):
        anc[:, :t] = anc[base + torch.randint(0, nb, (R,), generator=g)][:, :t]
    return anc.cuda()


def pos_legs(a, N, nb, Hq, Hkv, P, T, T_cap, anc, beam_idx, mk):
    """The --pos legs of one (P, T): host T against the device counter, kernel alone and whole step."""
    R, D = N * nb, 128
    n = max(2, int(a.ring_bytes // (2 * (N * P + R * T_cap) * Hkv * D * 2)))
    ring = [(mk(N, Hkv, P, D), mk(N, Hkv, P, D), mk(R, Hkv, T_cap, D), mk(R, Hkv, T_cap, D)) for _ in range(n)]
    q = mk(R, 1, Hq, D).transpose(1, 2)
    k_new, v_new = mk(R, 1, Hkv, D).transpose(1, 2), mk(R, 1, Hkv, D).transpose(1, 2)
    cnt = torch.tensor([T], dtype=torch.int32, device="cuda")
    shape = _hip.AttnShape(N, Hq, Hkv, P + T_cap, D ** -0.5, _hip.DTYPE_BF16)
    lib = _hip.load()
    ns_cap = lib.smt_attn_beams_splits(ctypes.byref(shape), nb, P, T_cap)
    ns_own = lib.smt_attn_beams_splits(ctypes.byref(shape), nb, P, T)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % n
        return state["i"]

    def reorder():
        if T > 1:
            anc[:, :T - 1] = anc.index_select(0, beam_idx)[:, :T - 1]

    def beam_step():
        kp, vp, kg, vg = ring[nxt()]
        reorder()
        kg[:, :, T - 1:T].copy_(k_new)
        vg[:, :, T - 1:T].copy_(v_new)
        return flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T)

    def beam_step_pos():
        kp, vp, kg, vg = ring[nxt()]
        reorder()
        kv_append(k_new, v_new, kg, vg, cnt)
        return flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, cnt)

    impls = [("beam_kernel", lambda: flash_attention_beams(q, *ring[nxt()], anc, nb, P, T)),
             ("beam_kernel@cap", lambda: flash_attention_beams(q, *ring[nxt()], anc, nb, P, T, num_splits=ns_cap)),
             ("beam_kernel_pos", lambda: flash_attention_beams(q, *ring[nxt()], anc, nb, P, cnt)),
             ("beam_step", beam_step), ("beam_step_pos", beam_step_pos)]
    same = bool(torch.equal(flash_attention_beams(q, *ring[0], anc, nb, P, cnt),
                            flash_attention_beams(q, *ring[0], anc, nb, P, T, num_splits=ns_cap)))
    anc0 = anc.clone()
    for rnd in range(a.rounds):
        res = {}
        for name, f in impls:
            us = timed(f, a.iters)
            k_us, kernels = kernel_us(f, min(a.iters, 50))
            anc.copy_(anc0)
            res[name] = (us, k_us)
            print(json.dumps({"impl": name, "round": rnd, "N": N, "nb": nb, "Hq": Hq, "Hkv": Hkv, "P": P, "T": T,
                              "T_cap": T_cap, "splits": ns_own if name in ("beam_kernel", "beam_step") else ns_cap,
                              "us": round(us, 2), "kernel_us": round(k_us, 2), "kv_copies": n, "kernels": kernels,
                              "bit_identical": same}), flush=True)
        k = lambda name: res[name][1]
        print(json.dumps({"impl": "pos_ratio", "round": rnd, "P": P, "T": T, "T_cap": T_cap,
                          "splits_own": ns_own, "splits_cap": ns_cap,
                          "kernel_us_pos_minus_host": round(k("beam_kernel_pos") - k("beam_kernel"), 2),
                          "kernel_us_cap_splits_minus_own": round(k("beam_kernel@cap") - k("beam_kernel"), 2),
                          "kernel_us_pos_minus_cap_splits": round(k("beam_kernel_pos") - k("beam_kernel@cap"), 2),
                          "kernel_us_pos_over_host": round(k("beam_kernel_pos") / k("beam_kernel"), 3),
                          "step_kernel_us_pos_over_host": round(k("beam_step_pos") / k("beam_step"), 3),
                          "step_us_pos_over_host": round(res["beam_step_pos"][0] / res["beam_step"][0], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--nb", type=int, default=4)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--P", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--T", type=int, nargs="*", default=[1, 128, 256])
    ap.add_argument("--T-cap", type=int, default=256, help="capacity of the generated buffers (max_new_tokens)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="forced split counts of the beam kernel to time "
                    "beside the default (impl beam_kernel@N)")
    ap.add_argument("--pos", action="store_true", help="the device-counter legs (smt_attn_fwd_beams_pos, "
                    "smt_attn_kv_append_pos) against host T, in place of the DynamicCache comparison")
    ap.add_argument("--ring-bytes", type=float, default=1.5e9, help="total bytes of the K/V copies a run cycles through")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_beam_bench: needs the GPU (a timing from anywhere else says nothing)")
    N, nb, Hq, Hkv, D = a.N, a.nb, a.Hq, a.Hkv, 128
    R, dt = N * nb, torch.bfloat16
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=dt)
    torch.manual_seed(0)
    for P in a.P:
        for T in a.T:
            T_cap = max(a.T_cap, T)
            anc = genealogy(N, nb, T, T_cap, 1000 * P + T)
            base = torch.arange(R, device="cuda") // nb * nb
            beam_idx = base + torch.randint(0, nb, (R,), device="cuda")
            dyn_bytes = 2 * R * Hkv * (P + T) * D * 2
            n = max(2, int(a.ring_bytes // dyn_bytes))
            # the beam-shared buffers, and the per-row cache a DynamicCache holds for the same hypotheses
            if a.pos:
                pos_legs(a, N, nb, Hq, Hkv, P, T, T_cap, anc, beam_idx, mk)
                continue
            beam_ring = [(mk(N, Hkv, P, D), mk(N, Hkv, P, D), mk(R, Hkv, T_cap, D), mk(R, Hkv, T_cap, D)) for _ in range(n)]
            src = base[:, None] + anc[:, :T].long()
            step = torch.arange(T, device="cuda")[None, :]
            dyn_ring = []
            for kp, vp, kg, vg in beam_ring:
                dyn_ring.append(tuple(torch.cat([p.repeat_interleave(nb, 0), g[src, :, step].permute(0, 2, 1, 3)], 2).contiguous()
                                      for p, g in ((kp, kg), (vp, vg))))
            q = mk(R, 1, Hq, D).transpose(1, 2)
            k_new, v_new = mk(R, Hkv, 1, D), mk(R, Hkv, 1, D)
            state = {"i": 0}

            def nxt():
                state["i"] = (state["i"] + 1) % n
                return state["i"]

            def dyn_step():
                k, v = dyn_ring[nxt()]
                k, v = k[:, :, :P + T - 1], v[:, :, :P + T - 1]            # the cache before this step
                if P + T - 1 > 0:
                    k, v = k.index_select(0, beam_idx), v.index_select(0, beam_idx)      # reorder_cache
                k, v = torch.cat([k, k_new], dim=-2), torch.cat([v, v_new], dim=-2)      # DynamicLayer.update
                return flash_attention_cached(q, k, v)

            def beam_step():
                kp, vp, kg, vg = beam_ring[nxt()]
                if T > 1:
                    anc[:, :T - 1] = anc.index_select(0, beam_idx)[:, :T - 1]            # reorder_cache
                kg[:, :, T - 1:T].copy_(k_new)                                           # BeamSharedLayer.update
                vg[:, :, T - 1:T].copy_(v_new)
                return flash_attention_beams(q, kp, vp, kg, vg, anc, nb, P, T)

            def cached_kernel():
                return flash_attention_cached(q, *dyn_ring[nxt()])

            def beam_kernel():
                return flash_attention_beams(q, *beam_ring[nxt()], anc, nb, P, T)

            state["i"] = 0
            o_c = cached_kernel().float()
            state["i"] = 0
            o_b = beam_kernel().float()
            rel_diff = ((o_b - o_c).norm() / o_c.norm()).item()
            impls = [("dyn_step", dyn_step), ("beam_step", beam_step), ("cached_kernel", cached_kernel),
                     ("beam_kernel", beam_kernel)]
            for ns in a.splits:
                impls.append((f"beam_kernel@{ns}",
                              lambda ns=ns: flash_attention_beams(q, *beam_ring[nxt()], anc, nb, P, T, num_splits=ns)))
            anc0 = anc.clone()
            for rnd in range(a.rounds):
                res = {}
                for name, f in impls:
                    us = timed(f, a.iters)
                    k_us, kernels = kernel_us(f, min(a.iters, 50))
                    anc.copy_(anc0)                        # beam_step permutes the table: the same genealogy for every run
                    res[name] = (us, k_us)
                    line = {"impl": name, "round": rnd, "N": N, "nb": nb, "Hq": Hq, "Hkv": Hkv, "P": P, "T": T,
                            "T_cap": T_cap, "us": round(us, 2), "kernel_us": round(k_us, 2), "kv_copies": n,
                            "kernels": kernels}
                    if name in ("cached_kernel", "beam_kernel"):
                        line["rel_diff"] = round(rel_diff, 5)
                    print(json.dumps(line), flush=True)
                print(json.dumps({"impl": "ratio", "round": rnd, "P": P, "T": T,
                                  "step_us_dyn_over_beam": round(res["dyn_step"][0] / res["beam_step"][0], 3),
                                  "step_kernel_us_dyn_over_beam": round(res["dyn_step"][1] / res["beam_step"][1], 3),
                                  "kernel_us_cached_over_beam": round(res["cached_kernel"][1] / res["beam_kernel"][1], 3)}),
                      flush=True)
            del beam_ring, dyn_ring


if __name__ == "__main__":
    main()
