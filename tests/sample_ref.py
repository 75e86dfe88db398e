"""Reference of the token selection (sparse_matrix_tuning_amd.sampling.sample_token, contract in
include/smt_sample.h) with bounds derived from the kernel's own roundings, and the planted inputs the
tests share (tests/test_sample_ref_host.py, tests/test_gpu_sample.py, tests/test_gpu_generate_sample.py). Everything here runs on the CPU.

z is computed in torch fp32 with the contract's operations, one correctly rounded operation each, so it is
the kernel's z bit for bit. The kept set, its threshold and the Gumbel scores are computed in fp64. A
decision of the kernel can differ from the reference's only where a deciding quantity lies within its
bound of its threshold; with eps = 2^-24 the unit roundoff of fp32:
  * top-k is exact (an order statistic of z).
  * top-p. The kernel keeps v iff A(v) < P with A(v) the sum over {j : z_j > z_v} of the integers
    q_j = round(expf(fl(z_j - M)) * 2^40) and P = ceil((double)W_q * (1 - thr)), W_q the sum of q over the
    top-k survivors. In units of 2^-40: fl(z_j - M) has relative error eps, that is |z_j - M| eps in the
    exponent; expf has a budget of 2 ulp = 4 eps; together w_j eps (|z_j - M| + 5) with second-order terms,
    plus 2^-41 for the rounding to an integer (which also covers terms that round to 0):
        e_j = 1.001 w_j eps (|z_j - M| + 5) + 2^-41
        |A(v) - P| is decided alike if it exceeds  sum_{z_j > z_v} e_j + (1 - thr) sum_j e_j + W 2^-50 + 2^-40
    (the last two: the conversion of W_q to double and the product, and the ceil). The integer sums are exact.
  * min-p. fl(z_v - M) against (float)log((double)min_p): |z_v - M - log(min_p)| is decided alike if it
    exceeds 1.001 eps (|z_v - M| + |log(min_p)|). z_v = M gives exactly 0 on both sides: kept.
  * the draw. s_v = fl(z_v + g_v), g_v = -logf(-logf(u_v)) with u_v exact: the inner logf has 4 eps relative
    error, which is 4 eps absolute after the outer logarithm; the outer logf 4 eps |g_v|; the sum eps |s_v|:
        d_v = 1.001 eps (4 + 4 |g_v| + |s_v|)
    and the best kept score wins alike if it leads the second best by more than the sum of their bounds.
`separation` is the smallest of these distances in units of its bound; the cases are chosen so that it is
at least 64 (planted exact ties decide alike by construction and are left out).
"""
import math

import torch

from sparse_matrix_tuning_amd.sampling import SAMPLE_CHUNK

EPS = 2.0 ** -24
C = SAMPLE_CHUNK
MASK = 0xFFFFFFFF
SEED, STEP, ROW0 = 0x9A3C5E7F12B4D608, 37, 5          # of the draw in every case


def mix(x):
    """include/smt_attention.h's mix on int64 tensors (or ints) holding uint32 values."""
    x = x ^ (x >> 16)
    x = (x * 0x21F0AAAD) & MASK
    x = x ^ (x >> 15)
    x = (x * 0x735A2D97) & MASK
    return x ^ (x >> 15)


def uniforms(seed, step, rows, V):
    """u_v of the header as fp32 [len(rows), V]; rows are absolute row numbers (row0 + r)."""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    head = mix((seed & MASK) + rows * 0x9E3779B9 & MASK) ^ (seed >> 32)
    row_key = mix((head + step * 0x85EBCA6B) & MASK)
    word = mix(row_key[:, None] ^ ((torch.arange(V, dtype=torch.int64) * 0x9E3779B1) & MASK)[None, :])
    u = ((word >> 8).to(torch.float32) + torch.tensor(0.5)) * torch.tensor(2.0 ** -24)
    return torch.minimum(u, torch.tensor(1.0 - 2.0 ** -24))


def gumbel64(seed, step, rows, V):
    return -torch.log(-torch.log(uniforms(seed, step, rows, V).double()))


def z_ref(logits, sequences, cur_len, penalty, suppressed, temperature):
    """z of the header in fp32, row by row."""
    x = logits.float().clone()
    R, V = x.shape
    pen, temp = torch.tensor(penalty, dtype=torch.float32), torch.tensor(temperature, dtype=torch.float32)
    for r in range(R):
        ids = sequences[r, :cur_len]
        ids = torch.unique(ids[(ids >= 0) & (ids < V)])
        if penalty != 1.0 and len(ids):
            v = x[r, ids]
            x[r, ids] = torch.where(v < 0, v * pen, v / pen)
    for s in suppressed:
        if 0 <= s < V:
            x[:, s] = -math.inf
    z = x / temp
    return torch.where(z == 0, torch.zeros_like(z), z)


def select_row(z, top_k, top_p, min_p):
    """(keep mask, separation) of one row of z (fp32 [V])."""
    V = z.numel()
    zd = z.double()
    M = zd.max()
    surv = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        surv = z >= torch.topk(z, top_k).values[-1]
    keep, sep = surv.clone(), math.inf
    top = zd == M
    if top_p < 1.0:
        thr = float(torch.tensor(1.0 - float(torch.tensor(top_p, dtype=torch.float32)), dtype=torch.float32))
        dist = torch.where(surv & (zd > -math.inf), (zd - M).abs(), torch.zeros_like(zd))
        w = torch.where(surv, torch.exp(zd - M), torch.zeros_like(zd))
        e = 1.001 * w * EPS * (dist + 5) + surv * 2.0 ** -41
        order = torch.sort(zd, descending=True, stable=True).indices
        zs, cw, ce = zd[order], torch.cumsum(w[order], 0), torch.cumsum(e[order], 0)
        first = torch.searchsorted(-zs, -zs, right=False)                # start of each group of equal values
        prev = (first - 1).clamp(min=0)
        A = torch.where(first > 0, cw[prev], torch.zeros_like(cw))
        dA = torch.where(first > 0, ce[prev], torch.zeros_like(ce))
        W, dW = cw[-1], ce[-1]
        P = (1.0 - thr) * W
        bound = dA + (1.0 - thr) * dW + W * 2.0 ** -50 + 2.0 ** -40
        s = surv[order]
        sep = min(sep, float(((A - P).abs() / bound)[s].min()))
        keep_s = (A < P) | (zs == M)
        keep[order] &= keep_s
    if min_p > 0.0:
        lmp = math.log(float(torch.tensor(min_p, dtype=torch.float32)))
        d = zd - M - lmp
        keep &= ~(d < 0) | top
        judged = ~top & (zd > -math.inf)
        if judged.any():
            bound = 1.001 * EPS * ((zd - M).abs() + abs(lmp))
            sep = min(sep, float((d.abs() / bound)[judged].min()))
    return keep, sep


def reference(case, seed=SEED, step=STEP, row0=ROW0):
    """dict(z, keep [R, V] bool, threshold fp32 [R], kept int32 [R], greedy int64 [R], drawn int64 [R],
    separation) of a case of `build_case`, the draw keyed by (seed, step, row0 + r)."""
    z = z_ref(case["logits"], case["sequences"], case["cur_len"], case["penalty"], case["suppressed"], case["temperature"])
    R, V = z.shape
    g = gumbel64(seed, step, [row0 + r for r in range(R)], V)
    keep = torch.zeros(R, V, dtype=torch.bool)
    threshold, kept = torch.zeros(R), torch.zeros(R, dtype=torch.int32)
    greedy, drawn = torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.int64)
    sep = math.inf
    for r in range(R):
        keep[r], s = select_row(z[r], case["top_k"], case["top_p"], case["min_p"])
        sep = min(sep, s)
        threshold[r], kept[r] = z[r][keep[r]].min(), keep[r].sum()
        assert torch.equal(keep[r], z[r] >= threshold[r])                # a value threshold
        greedy[r] = int(torch.nonzero(z[r] == z[r].max())[0])
        score = torch.where(keep[r], z[r].double() + g[r], torch.full((V,), -math.inf, dtype=torch.float64))
        bound = 1.001 * EPS * (4 + 4 * g[r].abs() + score.abs())
        best = torch.topk(score, min(2, V))
        drawn[r] = int(best.indices[0])
        if V > 1 and best.values[1] > -math.inf:
            sep = min(sep, float((best.values[0] - best.values[1]) / (bound[best.indices[0]] + bound[best.indices[1]])))
    return dict(z=z, keep=keep, threshold=threshold, kept=kept, greedy=greedy, drawn=drawn, separation=sep)


def build_case(seed, R, V, dtype, top_k=0, top_p=1.0, min_p=0.0, temperature=1.0, penalty=1.1, cur_len=64, plants=(),
               ktie=None, ptie=None):
    """CPU inputs of one case. A row is a tail of randn * 1.5 and a head of min(24, V) tokens from 20 down
    in steps of 0.37 (plus a jitter) at random places: the filters then cut inside the head, where
    neighbouring values differ by whole percents of the mass. History on both sides of every chunk edge, a
    duplicated id and the ids -1 and V (ignored) are always there; every head token of an even row and
    every other one of an odd row is in the history too. By name:
      last        the maximum of row 0 in the last element of the last chunk
      suppressed  a suppressed id that would otherwise win in every row
      one_finite  the last row holds one finite value
      ktie=k      row 0: the k-th largest value a second time, at C - 1 and C (across a chunk edge)
      ptie=j      row 0: head value j a second time, at 2C - 1 and 2C; the cases choose j so that it is the
                  top-p threshold
    """
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 1.5
    seq = torch.randint(0, V, (R, cur_len + 3), generator=g)
    nchunks = (V + C - 1) // C
    edges = [0, V - 1]
    for c in range(1, nchunks):
        edges += [c * C - 1, c * C]
    H = min(24, V)
    assert len(edges) + H + 4 <= cur_len
    seq[:, :len(edges)] = torch.tensor(edges)
    reserved = {C - 1, C, 2 * C - 1, 2 * C, V - 1, V // 2, V // 3}
    free = torch.tensor([v for v in range(V) if v not in reserved] or list(range(V)))
    for r in range(R):
        pos = free[torch.randperm(len(free), generator=g)[:H]]
        val = 20.0 - 0.37 * torch.arange(len(pos)) + torch.rand(len(pos), generator=g) * 0.1
        if r == 0 and ktie is not None:
            pos[ktie - 1] = C - 1
            x[r, C] = val[ktie - 1]
        if r == 0 and ptie is not None:
            pos[ptie] = 2 * C - 1
            x[r, 2 * C] = val[ptie]
        x[r, pos] = val
        told = pos if r % 2 == 0 else pos[::2]
        seq[r, len(edges):len(edges) + len(told)] = told
    seq[:, cur_len - 1] = -1
    seq[:, cur_len - 2] = V
    seq[:, cur_len - 3] = seq[:, cur_len - 4]
    suppressed = []
    if "last" in plants:
        x[0, V - 1] = 23.0
    if "one_finite" in plants:
        x[R - 1] = -math.inf
        x[R - 1, V // 3] = 1.5
    if "suppressed" in plants:
        x[:, V // 2] = 40.0
        suppressed = [V // 2, V + 5, -7]                     # two ids outside [0, V): they match nothing
    return dict(logits=x.to(dtype), sequences=seq, cur_len=cur_len, penalty=penalty, suppressed=suppressed,
                temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)


F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# (name, build_case arguments): every V of {1, 7, C-1, C, C+1, 2C+3, 152064}, R of {1, 3, 16}, the three dtypes,
# top_k of {0, 1, 2, 50, V, V+5}, top_p of {1, 0.95, 0.5, 1e-6}, min_p of {0, 0.05, 1}, temperature of {1, 0.6, 1.3},
# penalty of {1, 1.1}; the seeds are ones at which the reference is separated
CASES = [
    ("V1", dict(seed=0, R=3, V=1, dtype=F32, top_k=1, top_p=0.95)),
    ("V7", dict(seed=1, R=1, V=7, dtype=BF16, top_k=12, top_p=0.5, min_p=0.05, temperature=0.6)),
    ("C-1", dict(seed=2, R=16, V=C - 1, dtype=F16, top_k=50, top_p=0.95, temperature=0.6,
                 plants=("last", "suppressed", "one_finite"))),
    ("C", dict(seed=3, R=3, V=C, dtype=BF16, top_k=C, min_p=0.05, temperature=1.3, penalty=1.0)),
    ("C+1 ktie", dict(seed=4, R=3, V=C + 1, dtype=F32, top_k=2, ktie=2)),
    ("2C+3 ties", dict(seed=5, R=3, V=2 * C + 3, dtype=BF16, top_k=8, top_p=0.95, temperature=0.6, ktie=7, ptie=5,
                       plants=("suppressed",))),
    ("2C+3 top-p", dict(seed=6, R=16, V=2 * C + 3, dtype=F32, top_p=0.5, temperature=1.3, plants=("last",))),
    ("2C+3 tiny p", dict(seed=7, R=1, V=2 * C + 3, dtype=F16, top_p=1e-6, penalty=1.0)),
    ("2C+3 min-p 1", dict(seed=8, R=3, V=2 * C + 3, dtype=BF16, top_k=50, top_p=0.95, min_p=1.0, temperature=0.6)),
    ("2C+3 k1", dict(seed=9, R=3, V=2 * C + 3, dtype=F32, top_k=1, top_p=0.95, min_p=0.05)),
    ("2C+3 off", dict(seed=10, R=3, V=2 * C + 3, dtype=F16, plants=("one_finite", "last"))),
    ("2C+3 min-p", dict(seed=11, R=3, V=2 * C + 3, dtype=F32, min_p=0.05, temperature=0.6, plants=("suppressed",))),
    ("152064", dict(seed=12, R=3, V=152064, dtype=BF16, top_k=50, top_p=0.95, min_p=0.05, temperature=0.6, cur_len=300,
                    plants=("last", "suppressed"))),
    ("152064 top-p", dict(seed=13, R=1, V=152064, dtype=F32, top_p=0.95, temperature=0.6, cur_len=300)),
]


def frequency_case():
    """One row of 64 logits, 9 of them kept by top-k, drawn 4096 rows x 16 steps: (logits [4096, 64],
    sequences, probabilities [64] of the kept distribution)."""
    g = torch.Generator().manual_seed(99)
    x = torch.randn(64, generator=g) * 1.5
    keep = x >= torch.topk(x, 9).values[-1]
    p = torch.where(keep, torch.exp(x.double() - x.double().max()), torch.zeros(64, dtype=torch.float64))
    return x.repeat(4096, 1), torch.zeros(4096, 1, dtype=torch.int64), p / p.sum()


def assert_frequencies(tokens, p, what):
    """65536 draws: every token within 5 sigma of its probability, none outside the kept set."""
    n = tokens.numel()
    counts = torch.bincount(tokens.reshape(-1).cpu(), minlength=64).double()
    assert counts[p == 0].sum() == 0, f"{what}: draws outside the kept set"
    sigma = torch.sqrt(n * p * (1 - p))
    dev = ((counts - n * p).abs() / sigma)[p > 0]
    print(f"{what}: largest deviation {float(dev.max()):.2f} sigma over {int((p > 0).sum())} kept tokens")
    assert dev.max() <= 5, f"{what}: {float(dev.max()):.2f} sigma"
