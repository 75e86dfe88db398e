"""Time the gfx950 flash attention on packed rows (document mask, ``smt_attn_*_docs``) against the plain
causal kernels at the LLaMA-3-8B step shape: B=16, Hq=32, Hkv=8, S=2048, D=128, bf16, q/k/v in the HF
layout (transposed views of [B, S, H, D]).

Mixes (``--mix``):
  plain    the plain causal kernels of this tree (smt_attn_fwd / smt_attn_bwd)
  parent   the same entry points of another build of the library (``--parent-lib PATH``, e.g. the
           parent commit's), loaded beside this tree's in the same process
  one      one document per row through the document-mask kernels (their overhead)
  eight    eight documents of S/8 tokens per row
  skewed   a fixed-seed mix of many short and a few long documents whose boundaries do not align to 64

Forward and backward (dQ + dK/dV) are timed separately with device events around ``--iters`` calls of
the C entry points on preallocated buffers, after a warm-up of every variant; the whole list is
measured ``--rounds`` times in turn so that the run-to-run spread shows beside the differences. One
JSON line per (round, mix), with the ratio of visible work to the plain causal row: by (q, key)
elements and by 64 x 64 score tiles."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_matrix_tuning_amd import _hip  # noqa: E402
from sparse_matrix_tuning_amd.fused_llama import DocMask  # noqa: E402

D = 128


def documents(mix, B, S):
    """Document lengths per row."""
    if mix == "one":
        return [[S] for _ in range(B)]
    if mix == "eight":
        return [[S // 8] * 8 for _ in range(B)]
    gen = torch.Generator().manual_seed(2048)
    rows = []
    for _ in range(B):
        lens, left = [], S
        while left:
            long = torch.rand((), generator=gen).item() < 0.12
            n = int(torch.randint(300, 900, (), generator=gen)) if long else int(torch.randint(5, 150, (), generator=gen))
            n = min(n | 1, left)                          # odd lengths: boundaries off every tile edge
            lens.append(n)
            left -= n
        rows.append(lens)
    return rows


def visible(rows, S):
    """(elements, 64 x 64 tiles) a row mix makes visible, summed over rows."""
    el = tiles = 0
    for lens in rows:
        at = 0
        start = []
        for n in lens:
            el += n * (n + 1) // 2
            start += [at] * n
            at += n
        for i in range(0, S, 64):
            tiles += i // 64 - min(start[i:i + 64]) // 64 + 1
    return el, tiles


def timed(fn, iters):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(iters):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mix", nargs="*", default=["plain", "one", "eight", "skewed"])
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    B, Hq, Hkv, S = a.B, a.Hq, a.Hkv, a.S
    if not torch.cuda.is_available():
        raise SystemExit("attn_packed_bench: a ROCm device is needed")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mk = lambda H: torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    q, k, v, g = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    o, dq, dk, dv = (torch.empty_like(t) for t in (q, q, k, v))
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    T = lambda t: ctypes.byref(_hip.AttnTensor(t.data_ptr(), *t.stride()[:3]))
    shape = ctypes.byref(_hip.AttnShape(B, Hq, Hkv, S, D ** -0.5, _hip.DTYPE_BF16))
    stream = torch.cuda.current_stream().cuda_stream
    lib = _hip.load()
    libs = {"plain": lib}
    if "parent" in a.mix:
        if not a.parent_lib:
            raise SystemExit("attn_packed_bench: --mix parent needs --parent-lib")
        par = ctypes.CDLL(a.parent_lib)
        for name in ("smt_attn_fwd", "smt_attn_bwd"):
            getattr(par, name).restype, getattr(par, name).argtypes = _hip._SIGS[name]
        libs["parent"] = par

    def check(rc):
        if rc:
            raise RuntimeError(f"attention call failed (status {rc}): {lib.smt_attn_last_error().decode()}")

    causal = (S * (S + 1) // 2 * B, sum(i // 64 + 1 for i in range(0, S, 64)) * B)
    variants = {}
    for mix in a.mix:
        if mix in libs:
            L = libs[mix]
            fwd = lambda L=L: check(L.smt_attn_fwd(T(q), T(k), T(v), T(o), lse.data_ptr(), shape, stream))
            bwd = lambda L=L: check(L.smt_attn_bwd(T(q), T(k), T(v), T(o), T(g), lse.data_ptr(), delta.data_ptr(), T(dq),
                                                   T(dk), T(dv), shape, stream))
            vis = causal
        else:
            rows = documents(mix, B, S)
            dm = DocMask.from_cu_seqlens([torch.tensor([0] + lens).cumsum(0) for lens in rows], B, S, device=dev)
            ds, de = dm.start, dm.end
            fwd = lambda ds=ds, de=de: check(lib.smt_attn_fwd_docs(T(q), T(k), T(v), T(o), lse.data_ptr(), ds.data_ptr(),
                                                                   de.data_ptr(), 0.0, None, shape, stream))
            bwd = lambda ds=ds, de=de: check(lib.smt_attn_bwd_docs(T(q), T(k), T(v), T(o), T(g), lse.data_ptr(),
                                                                   delta.data_ptr(), T(dq), T(dk), T(dv), ds.data_ptr(),
                                                                   de.data_ptr(), 0.0, None, shape, stream))
            vis = visible(rows, S)
        variants[mix] = (fwd, bwd, vis)
    for fwd, bwd, _ in variants.values():                 # warm up every variant (code objects)
        for _ in range(3):
            fwd()
            bwd()
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for mix, (fwd, bwd, vis) in variants.items():
            fwd()                                         # the backward below reads this mix's o and lse
            f_ms = timed(fwd, a.iters)
            b_ms = timed(bwd, a.iters)
            print(json.dumps({"mix": mix, "round": rnd, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "iters": a.iters,
                              "fwd_ms": round(f_ms, 4), "bwd_ms": round(b_ms, 4),
                              "causal_over_visible_elements": round(causal[0] / vis[0], 2),
                              "causal_over_visible_tiles64": round(causal[1] / vis[1], 2)}), flush=True)


if __name__ == "__main__":
    main()
