"""The e4m3 quantisers at the bench's shapes (T = 32768 token rows; 4096 and 14336 columns), event
timed, interleaved rounds in one process. Prints one JSON line: median / min / max ms per call over
the rounds. Run it twice per library (SMT_HIP_LIB picks one) to get the run-to-run spread."""
import json
import os
import statistics

import torch

from sparse_matrix_tuning_amd import fp8 as f8

T, H, N = 32768, 4096, 14336


def timed(fn, iters=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    torch.manual_seed(0)
    dev = "cuda"
    xh = torch.randn(T, H, device=dev).bfloat16()
    rh = torch.randn(T, H, device=dev).bfloat16()
    wh = (1 + 0.1 * torch.randn(H, device=dev)).bfloat16()
    rstd = torch.rand(T, device=dev) + 0.5
    g = (torch.randn(T, N, device=dev) * 3).bfloat16()
    u = torch.randn(T, N, device=dev).bfloat16()
    dh = (torch.randn(T, N, device=dev) * 1e-3).bfloat16()
    qkv = [torch.randn(T, c, device=dev).bfloat16() for c in (4096, 1024, 1024)]
    W = (torch.randn(N, H, device=dev) * 0.02).bfloat16()
    fns = {"quant_rows_4096": lambda: f8.quant_rows(xh),
           "quant_rows_14336": lambda: f8.quant_rows(g),
           "quant_rows_cat_qkv": lambda: f8.quant_rows_cat(qkv),
           "quant_rows_cat_gate_up": lambda: f8.quant_rows_cat([g, u]),
           "quant_cols_t_14336x4096": lambda: f8.quant_cols_t(W),
           "rmsnorm_quant_4096": lambda: f8.rmsnorm_quant(xh, rh, wh, 1e-5, False),
           "rmsnorm_bwd_add_quant_4096": lambda: f8.rmsnorm_bwd_add_quant(xh, rh, wh, rstd, xh),
           "swiglu_fwd_quant_14336": lambda: f8.swiglu_fwd_quant(g, u, False),
           "swiglu_bwd_quant_14336": lambda: f8.swiglu_bwd_quant(g, u, dh, False, False)}
    for f in fns.values():
        f()
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(7):
        for k, f in fns.items():
            res[k].append(timed(f))
    out = {"lib": os.environ.get("SMT_HIP_LIB", "in-tree"), "rows": T, "unit": "ms per call"}
    for k, v in res.items():
        out[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
