"""The reference of tests/sample_ref.py on its own, without a GPU: every shared case is separated, the
planted inputs are what they claim to be, the kept set agrees with transformers' own warper objects, and
the contract's hash and Gumbel draw reproduce the kept distribution."""
import math

import pytest
import torch

from tests import sample_ref as ref
from tests.sample_ref import C, CASES, build_case

KW = dict(CASES)


@pytest.fixture(scope="module")
def refs():
    """Inputs and reference of every case, computed once and left unchanged."""
    out = {}
    for name, kw in CASES:
        case = build_case(**kw)
        out[name] = (case, ref.reference(case))
    return out


@pytest.mark.parametrize("name", [name for name, _ in CASES])
def test_every_case_is_separated(name, refs):
    case, r = refs[name]
    print(f"{name}: separation {r['separation']:.0f} bounds, kept {r['kept'].tolist()}")
    assert r["separation"] >= 64, f"{name}: only {r['separation']:.1f} bounds"


def test_the_plants_are_what_they_claim(refs):
    case, r = refs["C+1 ktie"]                                   # the k-th value tied across a chunk edge: both survive
    assert r["z"][0, C - 1] == r["z"][0, C] == r["threshold"][0] and r["kept"][0] == KW["C+1 ktie"]["top_k"] + 1
    case, r = refs["2C+3 ties"]
    z, k = r["z"][0], KW["2C+3 ties"]["top_k"]
    assert z[C - 1] == z[C] == torch.topk(z, k).values[-1] == torch.topk(z, k + 1).values[-1]
    assert z[2 * C - 1] == z[2 * C] == r["threshold"][0]         # the top-p threshold's group spans two chunks
    for name in ("C-1", "2C+3 top-p", "152064"):                 # the winner in the last element of the last chunk
        assert refs[name][1]["greedy"][0] == KW[name]["V"] - 1
    for name in ("C-1", "2C+3 ties", "152064"):                  # a suppressed id that would win
        case, r = refs[name]
        s = case["suppressed"][0]
        assert (case["logits"][:, s].float() == 40).all() and (r["z"][:, s] == -math.inf).all() and not r["keep"][:, s].any()
    for name in ("C-1", "2C+3 off"):                             # a row with one finite value
        assert torch.isfinite(refs[name][1]["z"][-1]).sum() == 1
    assert refs["2C+3 off"][1]["kept"].tolist() == [2 * C + 3] * 3
    assert refs["2C+3 tiny p"][1]["kept"].tolist() == [1]        # top_p 1e-6 keeps only the maximum
    assert refs["2C+3 min-p 1"][1]["kept"].tolist() == [1, 1, 1]


def _transformers_keep(case):
    """The kept set of transformers' processor objects on the CPU. Their gather / scatter take no id outside
    [0, V) (the contract ignores those), so the planted -1 and V become 0, a token the history holds anyway."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor, MinPLogitsWarper,
                                                        RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    x = case["logits"].float()
    V, cur_len = x.shape[1], case["cur_len"]
    seq = case["sequences"][:, :cur_len].clone()
    assert (seq == 0).any(dim=1).all()
    seq[(seq < 0) | (seq >= V)] = 0
    procs = LogitsProcessorList()
    if case["penalty"] != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=case["penalty"]))
    inside = [s for s in case["suppressed"] if 0 <= s < V]
    if inside:
        procs.append(MinLengthLogitsProcessor(cur_len + 1, inside))
    if case["temperature"] != 1.0:
        procs.append(TemperatureLogitsWarper(case["temperature"]))
    if case["top_k"]:
        procs.append(TopKLogitsWarper(top_k=case["top_k"]))
    if case["top_p"] < 1.0:
        procs.append(TopPLogitsWarper(top_p=case["top_p"]))
    if case["min_p"] > 0.0:
        procs.append(MinPLogitsWarper(min_p=case["min_p"]))
    return procs(seq, x) > -math.inf


@pytest.mark.parametrize("name", [name for name, _ in CASES])
def test_kept_set_against_transformers(name, refs):
    """fp32 logits: transformers' set exactly. bf16 / fp16 logits: a superset whose extra members share one
    value (transformers cuts inside the group of equal values at the top-p threshold)."""
    case, r = refs[name]
    theirs = _transformers_keep(case)
    ours = r["keep"] & (r["z"] > -math.inf)
    assert not (theirs & ~ours).any()
    extra = ours & ~theirs
    if case["logits"].dtype == torch.float32:
        assert not extra.any()
    for row in range(extra.shape[0]):
        assert torch.unique(r["z"][row][extra[row]]).numel() <= 1


def test_the_draw_reproduces_the_kept_distribution():
    x, _, p = ref.frequency_case()
    keep = p > 0
    tokens = []
    for step in range(16):
        g = ref.gumbel64(ref.SEED, step, list(range(4096)), 64)
        score = torch.where(keep, x.double() + g, torch.full_like(g, -math.inf))
        tokens.append(score.argmax(dim=1))
    ref.assert_frequencies(torch.stack(tokens), p, "reference")


def test_the_twin_is_the_same_contract(refs):
    """sampling.sample_token on CPU tensors (the torch restatement the loop tests run on) against the
    reference: threshold, count and both tokens."""
    from sparse_matrix_tuning_amd.sampling import sample_token
    for name, (case, r) in refs.items():
        for do_sample, want in ((False, r["greedy"]), (True, r["drawn"])):
            token, threshold, kept = sample_token(
                case["logits"], case["sequences"], case["cur_len"], repetition_penalty=case["penalty"],
                suppressed=case["suppressed"], temperature=case["temperature"], top_k=case["top_k"], top_p=case["top_p"],
                min_p=case["min_p"], do_sample=do_sample, seed=ref.SEED, step=ref.STEP, row0=ref.ROW0)
            assert torch.equal(threshold, r["threshold"]) and torch.equal(kept, r["kept"]), name
            assert torch.equal(token, want), (name, do_sample)
