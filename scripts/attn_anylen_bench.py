"""The gfx950 flash attention at sequence lengths that are not a multiple of 4
(fused_llama.flash_attention(any_length=True)), at the shape of scripts/attn_bench.py: B=16, Hq=32, Hkv=8,
D=128, bf16, causal, q/k/v in the HF layout. One JSON line per measurement.

Default: for every length of ``--S`` the mean device time of the forward, dQ and dK/dV kernels of a
forward + backward (torch.profiler), ``--rounds`` times over the whole list in turn, so that the
run-to-run spread shows beside a difference between lengths.

``--forward-only``: a gradient-free same-length call (an eval-loss batch, the prefill of generate())
through its two possible routes, the training forward kernel and the split-KV cached kernel
(flash_attention_cached with q_offset 0), by device events."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.attn_bench import kernel_times, timed  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import flash_attention, flash_attention_cached  # noqa: E402

KERNELS = (("fwd_ms", "attn_fwd"), ("dq_ms", "attn_dq"), ("dkdv_ms", "attn_dkdv"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--S", type=int, nargs="+", default=[2048, 2047, 2046, 2045])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--forward-only", action="store_true")
    a = ap.parse_args()
    B, Hq, Hkv, D = a.B, a.Hq, a.Hkv, 128
    torch.manual_seed(0)
    data = {}
    for S in a.S:
        mk = lambda H: torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2).requires_grad_(True)
        data[S] = (mk(Hq), mk(Hkv), mk(Hkv), torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16))
    for rnd in range(a.rounds):
        for S in a.S:
            q, k, v, g = data[S]
            rec = {"B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "round": rnd}
            if a.forward_only:
                with torch.no_grad():
                    rec["training_fwd_ms"] = round(timed(lambda: flash_attention(q, k, v, any_length=True), a.iters), 4)
                    rec["cached_fwd_ms"] = round(timed(lambda: flash_attention_cached(q, k, v, q_offset=0), a.iters), 4)
            else:
                def fb():
                    q.grad = k.grad = v.grad = None          # no gradient-accumulation adds in the timing
                    flash_attention(q, k, v, any_length=True).backward(g)
                times = kernel_times(fb, a.iters)
                for key, name in KERNELS:
                    rec[key] = round(sum(t for n, t in times.items() if name in n), 4)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
