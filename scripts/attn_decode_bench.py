"""Time the gfx950 cached (split-KV decode) attention, smt_attn_fwd_cached through
fused_llama.flash_attention_cached, against torch sdpa on the same tensors at the evaluation shape of
the reference's run_commonsense_parallel.py: B = 16 (4 prompts x 4 beams), Hq 32, Hkv 8, Sq 1,
Skv in {512, 2048, 8192}, bf16, contiguous [B, Hkv, Skv, 128] caches (what DynamicCache holds).

One JSON line per (Skv, impl): ``us`` = device-event time per call over back-to-back calls (includes
whatever the host cannot enqueue fast enough), ``kernel_us`` = the summed device time of the kernels
one call launches (torch.profiler; two kernels for a split smt call), and ``frac_8TBps`` = the
distinct K/V bytes (2 * B * Hkv * Skv * 128 * 2) over kernel_us, as a fraction of 8 TB/s. Every call
takes the next of a ring of K/V copies larger than the 256 MB Infinity Cache, as the layers of a model
do, so the bytes come from HBM.

impl: ``smt`` (default split count), ``smt@N`` (N splits; ``--splits`` adds more), ``sdpa`` (enable_gqa,
what transformers' sdpa path calls without a mask) and ``sdpa_repeat`` (K/V repeated to Hq heads first,
what it does with a padding mask).

``--static``: the device-position call (``q_offset`` a device tensor, smt_attn_fwd_cached_pos; what a
static cache's decode step runs) against the host-offset call of the same library on the same
tensors, at true lengths ``--Skv`` in buffers of capacity = the length and of capacity
``--capacity`` (default 8192) for all of them. Both take the default split count of the capacity
(``--splits`` adds forced counts), so a pair differs only in where the position comes from; the pair
alternates ``--rounds`` times (default 2 here). One JSON line per (length, capacity, splits, impl,
round): ``impl`` ``host`` / ``pos``, ``kernel_us`` and ``us`` as above, ``frac_8TBps`` over the K/V bytes
of the true length, ``equal``: the two results are bit-identical. The ring holds enough copies that
the rows a run touches exceed the Infinity Cache (``kv_copies``), within ``--ring-cap-bytes``."""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd import _hip  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import flash_attention_cached  # noqa: E402


def timed(fn, iters):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e[0].record()
    for _ in range(iters):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / iters * 1e3


def kernel_us(fn, iters):
    """(summed device us per call, {kernel name: us per call}) of the kernels fn launches."""
    from torch.profiler import ProfilerActivity, profile
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
            out[ev.key[:64]] = round(t / iters, 2)
    return sum(out.values()), out


def static_mode(a):
    B, Hq, Hkv, Sq, D = a.B, a.Hq, a.Hkv, a.Sq, 128
    lib = _hip.load()
    torch.manual_seed(0)
    q = torch.randn(B, Sq, Hq, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
    for cap_mode in ("length", "fixed"):
        for L in a.Skv:
            C = L if cap_mode == "length" else a.capacity
            if C < L or (cap_mode == "fixed" and C == L):
                continue                                   # capacity == length is the first pass
            touched = 2 * B * Hkv * L * D * 2
            per_copy = 2 * B * Hkv * C * D * 2
            n = max(2, min(int(a.ring_bytes // touched), int(a.ring_cap_bytes // per_copy)))
            ring = [(torch.randn(B, Hkv, C, D, device="cuda", dtype=torch.bfloat16),
                     torch.randn(B, Hkv, C, D, device="cuda", dtype=torch.bfloat16)) for _ in range(n)]
            shape = _hip.AttnShape(B, Hq, Hkv, C, D ** -0.5, _hip.DTYPE_BF16)
            default = lib.smt_attn_cached_splits(ctypes.byref(shape), Sq)
            pos = torch.full((), L - Sq, dtype=torch.int64, device="cuda")
            state = {"i": 0}

            def kv():
                state["i"] = (state["i"] + 1) % n
                return ring[state["i"]]

            for ns in [default] + [x for x in a.splits if x != default and 1 < x <= -(-C // 64)]:
                impls = [("host", lambda ns=ns: flash_attention_cached(q, *kv(), q_offset=L - Sq, num_splits=ns)),
                         ("pos", lambda ns=ns: flash_attention_cached(q, *kv(), q_offset=pos, num_splits=ns))]
                outs = []
                for _, f in impls:
                    state["i"] = 0
                    outs.append(f())
                equal = bool(torch.equal(outs[0], outs[1]))
                for rnd in range(a.rounds):
                    for name, f in impls:
                        us = timed(f, a.iters)
                        k_us, kernels = kernel_us(f, min(a.iters, 50))
                        print(json.dumps({"mode": "static", "impl": name, "round": rnd, "B": B, "Hq": Hq, "Hkv": Hkv,
                                          "Sq": Sq, "length": L, "capacity": C, "splits": ns,
                                          "default_splits": ns == default, "us": round(us, 2),
                                          "kernel_us": round(k_us, 2),
                                          "frac_8TBps": round(touched / (k_us * 1e-6) / 8e12, 3), "kv_copies": n,
                                          "equal": equal, "kernels": kernels}), flush=True)
            del ring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--Sq", type=int, default=1)
    ap.add_argument("--Skv", type=int, nargs="*", default=[512, 2048, 8192])
    ap.add_argument("--splits", type=int, nargs="*", default=[1], help="split counts to time beside the default")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=None, help="default 1, 2 with --static")
    ap.add_argument("--static", action="store_true", help="device-position call against the host-offset call")
    ap.add_argument("--capacity", type=int, default=8192, help="--static: the fixed buffer capacity of the second pass")
    ap.add_argument("--ring-cap-bytes", type=float, default=32e9, help="--static: upper bound of the ring's size")
    ap.add_argument("--ring-bytes", type=float, default=1.5e9, help="total bytes of the K/V copies a run cycles through")
    ap.add_argument("--no-sdpa", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_bench: needs the GPU (a timing from anywhere else says nothing)")
    if a.rounds is None:
        a.rounds = 2 if a.static else 1
    if a.static:
        return static_mode(a)
    B, Hq, Hkv, Sq, D = a.B, a.Hq, a.Hkv, a.Sq, 128
    lib = _hip.load()
    torch.manual_seed(0)
    for Skv in a.Skv:
        kv_bytes = 2 * B * Hkv * Skv * D * 2
        n = max(2, int(a.ring_bytes // kv_bytes))
        ring = [(torch.randn(B, Hkv, Skv, D, device="cuda", dtype=torch.bfloat16),
                 torch.randn(B, Hkv, Skv, D, device="cuda", dtype=torch.bfloat16)) for _ in range(n)]
        q = torch.randn(B, Sq, Hq, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
        shape = _hip.AttnShape(B, Hq, Hkv, Skv, D ** -0.5, _hip.DTYPE_BF16)
        default = lib.smt_attn_cached_splits(ctypes.byref(shape), Sq)
        state = {"i": 0}

        def kv():
            state["i"] = (state["i"] + 1) % n
            return ring[state["i"]]

        impls = [("smt", lambda: flash_attention_cached(q, *kv(), q_offset=Skv - Sq))]
        for ns in a.splits:
            if ns != default and ns <= -(-Skv // 64):
                impls.append((f"smt@{ns}", lambda ns=ns: flash_attention_cached(q, *kv(), q_offset=Skv - Sq, num_splits=ns)))
        if not a.no_sdpa and Sq == 1:                      # Sq == 1 sees every key: no mask to build
            impls.append(("sdpa", lambda: F.scaled_dot_product_attention(q, *kv(), enable_gqa=True)))

            def rep():
                k, v = kv()
                return F.scaled_dot_product_attention(q, k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1))
            impls.append(("sdpa_repeat", rep))
        ref = None
        for rnd in range(a.rounds):
            for name, f in impls:
                if rnd == 0:                               # the same result before the same timing
                    state["i"] = 0
                    o = f()
                    o = (o if name.startswith("smt") else o.transpose(1, 2)).float()
                    ref = o if ref is None else ref
                    err = ((o - ref).norm() / ref.norm()).item()
                us = timed(f, a.iters)
                k_us, kernels = kernel_us(f, min(a.iters, 50))
                print(json.dumps({"impl": name, "round": rnd, "B": B, "Hq": Hq, "Hkv": Hkv, "Sq": Sq, "Skv": Skv,
                                  "splits": default if name == "smt" else (int(name[4:]) if "@" in name else None),
                                  "us": round(us, 2), "kernel_us": round(k_us, 2),
                                  "frac_8TBps": round(kv_bytes / (k_us * 1e-6) / 8e12, 3), "kv_copies": n,
                                  "rel_diff_vs_smt": round(err, 5), "kernels": kernels}), flush=True)
        del ring


if __name__ == "__main__":
    main()
