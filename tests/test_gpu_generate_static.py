"""generate() on a patch_llama-ed model through transformers' static cache
(``cache_implementation="static"``): a pre-allocated K / V buffer per layer whose fill level is a device
tensor. The prefill of the left-padded 13-token batch runs the training forward kernel on the first 13
slots; every decode step runs the device-position decode kernel (smt_attn_fwd_cached_pos) against the
whole buffer, the position read by the kernel.

Model, twin and inputs are those of tests/test_gpu_generate.py, recreated here: a randomly initialised
LLaMA (hidden 512, 2 layers, Hq 4, Hkv 2, head_dim 128, vocabulary 512) in bf16 and its unpatched fp32
``attn_implementation="eager"`` twin with the same bf16-rounded weights; prompts of 13 and 7 tokens
(left-padded to 13), then 6 fixed tokens one at a time.

Teacher-forced check, through ``StaticCache(max_cache_len=19)``: the last-position logits of the prefill
and of each decode step against the twin's full-sequence logits. Bar per step, as in that file:
relative norm error <= max(8e-3, 1.5 x the error of the same bf16 model with
``attn_implementation="sdpa"`` through the same static-cache sequence).

generate check: greedy and num_beams=4 with ``cache_implementation="static"`` and no other flag return
[2, 21]; every greedily generated token's logit in the twin's teacher-forced pass lies within delta of
that position's maximum, delta = the largest absolute logit error of the teacher-forced check.
patch_llama sets ``generation_config.disable_compile`` (generate() would otherwise send a static cache
through torch.compile) and unpatch_llama puts back what was there."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PROMPT, LENS, STEPS, NEW = 13, (13, 7), 6, 8


def _config(attn):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                       num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64,
                       pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation=attn)


def _inputs(device):
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 512, (2, PROMPT + STEPS), generator=g)
    mask = torch.ones(2, PROMPT + STEPS, dtype=torch.int64)
    for b, n in enumerate(LENS):
        ids[b, :PROMPT - n] = 0
        mask[b, :PROMPT - n] = 0
    return ids.to(device), mask.to(device)


def _positions(mask):
    return (mask.cumsum(-1) - 1).clamp(min=0)


@torch.no_grad()
def _full_logits(twin, ids, mask):
    return twin(input_ids=ids, attention_mask=mask, position_ids=_positions(mask), use_cache=False).logits.float()


@torch.no_grad()
def _prefill_and_decode(model, ids, mask):
    """Last-position logits of the prefill and of each teacher-forced decode step through a static cache
    of exactly PROMPT + STEPS slots: [1 + STEPS, B, V]. The mask of each call covers the keys written so
    far, as generate() passes it."""
    from transformers import StaticCache
    pos = _positions(mask)
    cache = StaticCache(config=model.config, max_cache_len=PROMPT + STEPS)
    out = model(input_ids=ids[:, :PROMPT], attention_mask=mask[:, :PROMPT], position_ids=pos[:, :PROMPT],
                past_key_values=cache, use_cache=True)
    steps = [out.logits[:, -1].float()]
    for t in range(PROMPT, PROMPT + STEPS):
        out = model(input_ids=ids[:, t:t + 1], attention_mask=mask[:, :t + 1], position_ids=pos[:, t:t + 1],
                    past_key_values=cache, use_cache=True)
        assert out.logits.shape[1] == 1
        steps.append(out.logits[:, -1].float())
    assert int(cache.get_seq_length()) == PROMPT + STEPS
    return torch.stack(steps)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def run():
    """Everything once: the twin's logits, the sdpa run, then the patched model's teacher-forced run and
    its two generate() calls; unpatched again before the twin scores the generated sequence."""
    from transformers import LlamaForCausalLM
    from sparse_matrix_tuning_amd.fused_llama import patch_llama, unpatch_llama
    torch.manual_seed(3)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    twin = LlamaForCausalLM(_config("eager"))
    twin.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    twin = twin.to(DEV).float().eval()
    ids, mask = _inputs(DEV)
    ref = _full_logits(twin, ids, mask)[:, PROMPT - 1:PROMPT + STEPS].transpose(0, 1)      # [1 + STEPS, B, V]
    sdpa = _prefill_and_decode(model, ids, mask)
    r = {"ref": ref, "sdpa": sdpa, "compile_before": model.generation_config.disable_compile}
    counts = patch_llama(model)
    try:
        assert counts["attention"] == 2 and model.config._attn_implementation == "smt_flash"
        r["compile_patched"] = model.generation_config.disable_compile
        try:
            r["smt"] = _prefill_and_decode(model, ids, mask)
        except Exception as e:                           # reported by the tests that need it
            r["smt"] = e
        for name, kw in (("greedy", {}), ("beams", {"num_beams": 4})):
            try:
                with torch.no_grad():
                    r[name] = model.generate(input_ids=ids[:, :PROMPT], attention_mask=mask[:, :PROMPT],
                                             max_new_tokens=NEW, min_new_tokens=NEW, do_sample=False,
                                             cache_implementation="static", **kw)
            except Exception as e:
                r[name] = e
    finally:
        unpatch_llama(model)
    r["compile_after"] = model.generation_config.disable_compile
    if isinstance(r["greedy"], torch.Tensor):
        gmask = torch.cat([mask[:, :PROMPT], torch.ones(2, NEW, dtype=mask.dtype, device=DEV)], dim=1)
        r["greedy_twin"] = _full_logits(twin, r["greedy"], gmask)
    return r


def _get(run, name):
    if isinstance(run[name], Exception):
        raise run[name]
    return run[name]


def test_teacher_forced_prefill_and_decode(run):
    ref, sdpa, smt = run["ref"], run["sdpa"], _get(run, "smt")
    assert smt.shape == ref.shape == (1 + STEPS, 2, 512) and torch.isfinite(smt).all()
    errs = []
    for t in range(1 + STEPS):
        e, es = _rel(smt[t], ref[t]), _rel(sdpa[t], ref[t])
        print(f"step {t}: smt_flash rel err {e:.3e}, sdpa {es:.3e}, max abs err {(smt[t] - ref[t]).abs().max().item():.3e}")
        errs.append((t, e, es))
    for t, e, es in errs:
        assert e <= max(8e-3, 1.5 * es), (t, e, es)


@pytest.mark.parametrize("name", ["greedy", "beams"])
def test_generate_runs(run, name):
    out = _get(run, name)
    assert out.shape == (2, PROMPT + NEW)
    ids, _ = _inputs(DEV)
    assert torch.equal(out[:, :PROMPT], ids[:, :PROMPT])


def test_greedy_tokens_are_the_twins_argmax_up_to_rounding(run):
    out = _get(run, "greedy")
    delta = (_get(run, "smt") - run["ref"]).abs().max().item()
    logits = run["greedy_twin"]                                        # [B, PROMPT + NEW, V]
    for p in range(PROMPT, PROMPT + NEW):
        row = logits[:, p - 1]
        chosen = row.gather(1, out[:, p:p + 1]).squeeze(1)
        gap = (row.max(-1).values - chosen)
        print(f"position {p}: gap to the twin's maximum {gap.tolist()}, delta {delta:.3e}")
        assert (gap <= delta).all(), (p, gap.tolist(), delta)


def test_disable_compile_is_set_and_restored(run):
    assert run["compile_patched"] is True
    assert run["compile_after"] == run["compile_before"]
