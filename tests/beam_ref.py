"""fp64 reference of the beam-search scoring step (sparse_matrix_tuning_amd.beam_search.beam_topk) with a
per-element bound derived from the kernel's own roundings, and the planted inputs the GPU tests share
(tests/test_gpu_beam_topk.py, tests/test_gpu_generate_beam_loop.py). Everything here runs on the CPU.

The bound, with eps = 2^-24 the unit roundoff of fp32 and x the logits, exact in fp32:
  * S = sum_v exp(x_v - M) as the kernel forms it. Term v goes through fl(x_v - M_c) (relative error
    eps, |x_v - M_c| eps in the exponent), expf (budget 2 ulp = 4 eps), the chunk's sum (7 serial adds per
    thread, 6 butterfly levels, 3 adds over the 4 waves: 16 eps), the factor expf(fl(M_c - M)) (|M_c - M| eps
    + 4 eps), the product (eps) and the sum over chunks (ceil(chunks / 256) - 1 serial adds, 6 levels, 3
    adds). |x_v - M_c| + |M_c - M| = M - x_v, so
        dS / S <= eps * (sum_v p_v (M - x_v) + 9 + 16 + combine_adds),   p = softmax(x),
    plus V * 2^-126 for terms in the subnormal range (S >= 1: the row's maximum contributes exp(0)).
  * lse = fl(M + logf(S)):  d_lse <= dS / S + 4 eps |log S| + eps |lse|       (logf budget 2 ulp)
  * lp = fl(x_v - lse):     d_lp <= d_lse + eps |lp|
  * q = lp * penalty or lp / penalty (correctly rounded; a sign decided differently within d_lp of zero
    is covered by the factor):   d_q <= d_lp * max(penalty, 1 / penalty) + eps |q|
  * score = fl(q + beam_score):  d <= d_q + eps |score|        (64 at the first step's -1e9)
all times 1.001 for the second-order terms. A suppressed token is exactly -inf.
"""
import math

import torch

from sparse_matrix_tuning_amd.beam_search import BEAM_CHUNK

EPS = 2.0 ** -24
C = BEAM_CHUNK


def ref64(logits, beam_scores, sequences, cur_len, nb, penalty=1.0, suppressed=()):
    """(scores, bound): fp64 [N, nb * V] each, of CPU inputs; the penalty is the fp32 value the kernel gets."""
    x = logits.double()
    R, V = x.shape
    pf = float(torch.tensor(penalty, dtype=torch.float32))
    M = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - M)
    S = e.sum(dim=1, keepdim=True)
    lse = M + torch.log(S)
    nchunks = (V + C - 1) // C
    combine_adds = (nchunks + 255) // 256 - 1 + 6 + 3
    dS = EPS * (((e / S) * (M - x)).sum(dim=1, keepdim=True) + 9 + 16 + combine_adds) + V * 2.0 ** -126
    d_lse = dS + 4 * EPS * torch.log(S).abs() + EPS * lse.abs()
    lp = x - lse
    d = d_lse + EPS * lp.abs()
    seen = torch.zeros(R, V, dtype=torch.bool)
    for r in range(R):
        ids = sequences[r, :cur_len]
        ids = ids[(ids >= 0) & (ids < V)]
        seen[r, ids] = True
    q = torch.where(seen, torch.where(lp < 0, lp * pf, lp / pf), lp)
    d = torch.where(seen, d * max(pf, 1 / pf) + EPS * q.abs(), d)
    score = q + beam_scores.double().reshape(R, 1)
    d = (d + EPS * score.abs()) * 1.001
    for s in suppressed:
        if 0 <= s < V:
            score[:, s] = -math.inf
            d[:, s] = 0.0
    return score.reshape(R // nb, nb * V), d.reshape(R // nb, nb * V)


def ref_topk(score, bound, K):
    """The reference's K + 1 best (K if there are no more): (scores, indices, bounds), descending, equal scores by
    lower flat index (a stable sort)."""
    k1 = min(K + 1, score.shape[1])
    s, i = torch.sort(score, dim=1, descending=True, stable=True)
    return s[:, :k1], i[:, :k1], torch.gather(bound, 1, i[:, :k1])


def separation(s, b):
    """min over neighbours of the sorted reference scores of gap / max(bound), exact ties left out."""
    gap = s[:, :-1] - s[:, 1:]
    width = torch.maximum(b[:, :-1], b[:, 1:])
    ratio = torch.where(gap == 0, torch.full_like(gap, math.inf), gap / width)
    return float(ratio.min()) if ratio.numel() else math.inf


def assert_separated(s, b, what):
    """The reference's top K + 1 are pairwise at least 64 bounds apart, planted (exact) ties excepted."""
    assert torch.isfinite(s).all(), what
    sep = separation(s, b)
    assert sep >= 64, f"{what}: reference scores only {sep:.1f} bounds apart"


def check(what, got_scores, got_index, score, bound, K):
    """Indices: the reference's set and order. Scores: within the bound; bit-equal where the reference ties."""
    s, i, b = ref_topk(score, bound, K)
    assert_separated(s, b, what)
    got_scores, got_index = got_scores.cpu(), got_index.cpu().long()
    assert got_scores.shape == got_index.shape == (score.shape[0], K), what
    assert got_scores.dtype == torch.float32
    assert ((got_index >= 0) & (got_index < score.shape[1])).all(), what
    err = (got_scores.double() - s[:, :K]).abs()
    print(f"{what}: max err / bound {float((err / b[:, :K]).max()):.3f}, separation {separation(s, b):.0f} bounds, "
          f"indices equal: {torch.equal(got_index, i[:, :K])}")
    assert torch.equal(got_index, i[:, :K]), what
    assert (err <= b[:, :K]).all(), what
    tie = s[:, :K - 1] == s[:, 1:K]
    assert torch.equal(got_scores[:, :-1][tie], got_scores[:, 1:][tie]), what


def build_case(seed, N, nb, V, K, dtype, cur_len=24, first_step=False, plants=(), extra_cols=3):
    """CPU inputs of one case: dict(logits [R, V] dtype, beam_scores [R] fp32, sequences [R, cur_len + extra]
    int64, cur_len, nb, K, suppressed). History on both sides of every chunk edge, a duplicated id and the
    ids -1 and V (ignored) are always there; ``plants`` adds, by name:
      one_chunk  all K winners of sample 0 in one chunk of its last beam
      last       a winner of sample 1 % N in the last element of the last chunk
      ties_row   an exact tie inside a row of sample 2 % N
      twin_rows  beams 0 and 1 of sample 2 % N identical, with equal beam scores
      suppressed a suppressed id that would otherwise win in every sample
    """
    g = torch.Generator().manual_seed(seed)
    R = N * nb
    x = (torch.randn(R, V, generator=g) * 2).to(dtype)
    if first_step:
        bs = torch.full((N, nb), -1e9)
        bs[:, 0] = 0.0
        bs = bs.reshape(R)
    else:
        bs = -(torch.rand(R, generator=g) * 4)
    seq = torch.randint(0, V, (R, cur_len + extra_cols), generator=g)
    nchunks = (V + C - 1) // C
    edges = [0, V - 1]
    for c in range(1, nchunks):
        edges += [c * C - 1, c * C]
    assert len(edges) + 4 <= cur_len
    seq[:, :len(edges)] = torch.tensor(edges)
    seq[:, cur_len - 1] = -1
    seq[:, cur_len - 2] = V
    seq[:, cur_len - 3] = seq[:, cur_len - 4]
    suppressed = []
    if "one_chunk" in plants:
        r, lo = nb - 1, (1 if nchunks > 1 else 0) * C
        for j in range(K):
            x[r, lo + 3 + 5 * j] = 20 + 0.25 * j
    if "last" in plants:
        x[(1 % N) * nb, V - 1] = 30.0
    if "ties_row" in plants:
        r, a, b = (2 % N) * nb + nb - 1, 5, V - 3
        x[r, a] = x[r, b] = 25.0
        seq[r][(seq[r] == a) | (seq[r] == b)] = 1
    if "twin_rows" in plants and nb >= 2:
        r0 = (2 % N) * nb
        bs[r0] = 0.5                                         # above every other beam: the twins' candidates win
        x[r0 + 1], seq[r0 + 1], bs[r0 + 1] = x[r0], seq[r0], bs[r0]
    if "suppressed" in plants:
        s = V // 2
        x[:, s] = 40.0
        suppressed = [s, V + 5, -7]                         # two ids outside [0, V): they match nothing
    return dict(logits=x, beam_scores=bs.float(), sequences=seq, cur_len=cur_len, nb=nb, K=K, suppressed=suppressed)


# (name, build_case arguments): every V of {1, 7, C-1, C, C+1, 2C+3, 128256}, N of {1, 3}, nb of {1, 4, 5},
# K of {1, 2, 8, 16, 32} and the three dtypes; the seeds are ones at which the reference is separated
CASES = [
    ("V1", dict(seed=0, N=3, nb=4, V=1, K=2, dtype=torch.float32, cur_len=8)),
    ("V7", dict(seed=1, N=1, nb=5, V=7, K=8, dtype=torch.bfloat16, cur_len=8)),
    ("C-1", dict(seed=2, N=3, nb=4, V=C - 1, K=16, dtype=torch.float16, plants=("one_chunk", "last", "ties_row"))),
    ("C", dict(seed=3, N=1, nb=1, V=C, K=32, dtype=torch.bfloat16, plants=("last",))),
    ("C+1", dict(seed=4, N=3, nb=5, V=C + 1, K=8, dtype=torch.float32, plants=("last", "suppressed", "twin_rows"))),
    ("2C+3 planted", dict(seed=5, N=3, nb=4, V=2 * C + 3, K=16, dtype=torch.bfloat16,
                          plants=("one_chunk", "last", "ties_row", "twin_rows", "suppressed"))),
    ("2C+3 first step", dict(seed=6, N=3, nb=4, V=2 * C + 3, K=8, dtype=torch.float16, first_step=True,
                             plants=("last",))),
    ("2C+3 K1", dict(seed=7, N=1, nb=5, V=2 * C + 3, K=1, dtype=torch.float32, plants=("last",))),
    ("2C+3 K32", dict(seed=8, N=3, nb=1, V=2 * C + 3, K=32, dtype=torch.bfloat16, plants=("one_chunk", "ties_row"))),
    ("2C+3 K2 fp16", dict(seed=9, N=1, nb=4, V=2 * C + 3, K=2, dtype=torch.float16, plants=("twin_rows",))),
    ("128256", dict(seed=10, N=4, nb=4, V=128256, K=8, dtype=torch.bfloat16, cur_len=300, plants=("last", "suppressed"))),
]
