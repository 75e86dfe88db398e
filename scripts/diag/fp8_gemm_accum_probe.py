"""How exactly does the rowwise-scaled e4m3 GEMM (torch._scaled_mm, hipBLASLt) add its products?

At the shapes of the GEMM-seam tests (M 96, N 256, K 512, bf16 out, all scales 1) one dot product
is built from three e4m3 products: +448 * 448 = 200704, a small power of two 2^s, and -200704. Its
exact value is 2^s, a bf16 number. An fp32 chain that meets the two large terms before the small
one returns 2^s for every s; one that adds the small term to 200704 first loses it below
ulp(200704) / 2 = 2^-7. A dot-product unit that aligns the products of one instruction to the
largest exponent and keeps t bits below it loses the small term below 2^(17 - t).

Three placements of (big, small, -big) along K: all within the first 16 products; small far from a
cancelling pair; and the pair split with the small term between them. Prints one JSON line per
placement with the smallest s that survives, and one line with the error of random operands
relative to sum |a b| with and without a 2^10 outlier row / column."""
import json

import numpy as np
import torch

M, N, K = 96, 256, 512
F8 = torch.float8_e4m3fn


def mm(a, b):
    one_m = torch.ones(a.shape[0], 1, device="cuda")
    one_n = torch.ones(1, b.shape[0], device="cuda")
    return torch._scaled_mm(a.to(F8), b.to(F8).t(), scale_a=one_m, scale_b=one_n, out_dtype=torch.bfloat16)


def small_pairs():
    """(s, u, v) with u * v = 2^s, u and v e4m3 powers of two, s from -18 to 16."""
    out = []
    for s in range(-18, 17):
        eu = max(-9, min(8, s // 2))
        ev = s - eu
        if -9 <= ev <= 8:
            out.append((s, 2.0 ** eu, 2.0 ** ev))
    return out


def placement(name, k_big, k_small, k_neg, big=448.0):
    pairs = small_pairs()
    a = torch.zeros(M, K, device="cuda")
    b = torch.zeros(N, K, device="cuda")
    b[:, k_big], b[:, k_neg] = big, big
    a[:, k_big], a[:, k_neg] = big, -big
    for i, (_s, u, v) in enumerate(pairs):
        a[i, k_small] = u
        b[i, k_small] = v
    y = mm(a, b).float().cpu().numpy()
    kept = [s for i, (s, _u, _v) in enumerate(pairs) if y[i, i] == 2.0 ** s]
    wrong = [(s, float(y[i, i])) for i, (s, _u, _v) in enumerate(pairs) if y[i, i] not in (0.0, 2.0 ** s)]
    print(json.dumps({"placement": name, "big_product_log2": float(np.log2(big * big)), "k": [k_big, k_small, k_neg],
                      "smallest_surviving_log2": min(kept) if kept else None,
                      "lost_log2": [s for s, _, _ in pairs if s not in kept], "neither_0_nor_exact": wrong}),
          flush=True)


def random_error(outlier):
    g = torch.Generator().manual_seed(1)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(N, K, generator=g)
    if outlier:
        a[:, 13] *= 1024
        b[:, 13] *= 1024
    a8 = (a * (448 / a.abs().amax(dim=1, keepdim=True))).cuda().to(F8)
    b8 = (b * (448 / b.abs().amax(dim=1, keepdim=True))).cuda().to(F8)
    y = mm(a8, b8).double().cpu().numpy()
    A, B = a8.double().cpu().numpy(), b8.double().cpu().numpy()
    v, s = A @ B.T, np.abs(A) @ np.abs(B).T
    exp = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    past_bf16 = np.maximum(np.abs(y - v) - 2.0 ** (exp - 8), 0)             # beyond half a bf16 step of v
    print(json.dumps({"random_operands": "outlier column" if outlier else "plain",
                      "max_err_past_half_bf16_step_over_sum_abs_in_2^-24": float((past_bf16 / s).max() * 2.0 ** 24),
                      "max_err_over_sum_abs_in_2^-24": float((np.abs(y - v) / s).max() * 2.0 ** 24)}), flush=True)


if __name__ == "__main__":
    placement("one instruction: big, small, -big adjacent", 0, 1, 2)
    placement("one instruction, big = 16 * 16", 0, 1, 2, big=16.0)
    placement("one instruction, big = 0.5 * 0.5", 0, 1, 2, big=0.5)
    placement("small far after the cancelling pair", 0, 300, 1)
    placement("small between the pair, far from both", 0, 200, 400)
    placement("small far before the pair", 300, 5, 301)
    random_error(False)
    random_error(True)
