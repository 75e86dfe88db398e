"""Beam search on a patch_llama-ed model through BeamSharedCache: the prefill of a left-padded batch,
then decoding with the beam kernel (smt_attn_fwd_beams) against a cache that is never reordered.

Model: the tiny LLaMA of tests/test_gpu_generate.py (its config repeated here: hidden 512, 2 layers,
Hq 4, Hkv 2, head_dim 128, vocabulary 512), bf16, and its fp32 ``attn_implementation="eager"`` twin
with the same (bf16-rounded) weights. patch_llama swaps RoPE at module level, so the twin and the sdpa
model run before patching.

Teacher-forced check: prompts of 13 and 7 tokens (left-padded to 13), expanded to 4 beams as
generate() expands them; six decode steps with fixed tokens (different per beam) and a scripted
within-sample beam_idx after the prefill and after every step, one of which lets a single hypothesis
take over all beams of its sample. The same script runs through the patched model with
BeamSharedCache, the bf16 sdpa model with DynamicCache and the fp32 eager twin with DynamicCache; the
last-position logits of the prefill and of every step meet the bar of tests/test_gpu_generate.py:
relative norm error <= max(8e-3, 1.5 x the sdpa model's error) against the twin.

generate check: num_beams=4, max_new_tokens=8 returns [2, 21] with the prompt intact, the generated
buffers keep their addresses over all decode forwards, and the ancestry table is updated once per
generated token, not once per layer. No token equality with a DynamicCache run is asserted: two
attention kernels round differently and a randomly initialised model has near-ties."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PROMPT, LENS, STEPS, NEW, NB = 13, (13, 7), 6, 8, 4
ROWS = 2 * NB

# beam_idx offsets within the sample, after the prefill and after each of the six steps
SCRIPT = [
    [0, 1, 2, 3],
    [1, 0, 0, 3],
    [2, 2, 1, 0],
    [3, 3, 3, 3],           # one hypothesis takes over: the other slots' entries are dead from here on
    [0, 1, 1, 2],
    [2, 0, 3, 1],
    [1, 1, 0, 2],
]


def _config(attn):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                       num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64,
                       pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation=attn)


def _inputs(device):
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, 512, (2, PROMPT), generator=g)
    mask = torch.ones(2, PROMPT, dtype=torch.int64)
    for b, n in enumerate(LENS):
        ids[b, :PROMPT - n] = 0
        mask[b, :PROMPT - n] = 0
    tokens = torch.randint(3, 512, (STEPS, ROWS), generator=g)           # a different stream per beam
    return ids.to(device), mask.to(device), tokens.to(device)


def _beam_idx(step, device):
    """The flat beam_idx of SCRIPT[step]; sample 1 uses the list reversed."""
    off = torch.tensor([SCRIPT[step], SCRIPT[step][::-1]], device=device)
    return (torch.arange(2, device=device)[:, None] * NB + off).reshape(-1)


@torch.no_grad()
def _prefill_and_decode(model, cache, ids, mask, tokens):
    """Last-position logits of the prefill and of each teacher-forced decode step: [1 + STEPS, ROWS, V]."""
    ids, mask = ids.repeat_interleave(NB, 0), mask.repeat_interleave(NB, 0)
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    out = model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True)
    steps = [out.logits[:, -1].float()]
    cache.reorder_cache(_beam_idx(0, ids.device))
    for t in range(STEPS):
        mask = torch.cat([mask, mask.new_ones(ROWS, 1)], dim=1)
        out = model(input_ids=tokens[t][:, None], attention_mask=mask, position_ids=mask.sum(-1, keepdim=True) - 1,
                    past_key_values=cache, use_cache=True)
        assert out.logits.shape[1] == 1
        steps.append(out.logits[:, -1].float())
        cache.reorder_cache(_beam_idx(t + 1, ids.device))
    return torch.stack(steps)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def run():
    """Everything once: the twin's and the sdpa model's runs on a DynamicCache, then the patched model's
    teacher-forced run and its generate() call on a BeamSharedCache."""
    from transformers import DynamicCache, LlamaForCausalLM
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import patch_llama, unpatch_llama
    torch.manual_seed(3)
    model = LlamaForCausalLM(_config("sdpa")).to(DEV).bfloat16().eval()
    twin = LlamaForCausalLM(_config("eager"))
    twin.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    twin = twin.to(DEV).float().eval()
    ids, mask, tokens = _inputs(DEV)
    r = {"ref": _prefill_and_decode(twin, DynamicCache(config=twin.config), ids, mask, tokens),
         "sdpa": _prefill_and_decode(model, DynamicCache(config=model.config), ids, mask, tokens)}
    patch_llama(model)
    try:
        cache = BeamSharedCache(model.config, NB, STEPS)
        r["smt"] = _prefill_and_decode(model, cache, ids, mask, tokens)
        r["smt_cache"] = cache
        gen_cache = BeamSharedCache(model.config, NB, NEW)
        seen = []                                        # per forward: the generated buffers' addresses, or None
        hook = model.register_forward_pre_hook(lambda m, a: seen.append(
            tuple((ly.k_gen.data_ptr(), ly.v_gen.data_ptr()) for ly in gen_cache.layers)
            if gen_cache.layers[0].is_initialized else None))
        try:
            with torch.no_grad():
                r["beams"] = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, min_new_tokens=NEW,
                                            do_sample=False, num_beams=NB, past_key_values=gen_cache)
        except Exception as e:                           # reported by the test that needs it
            r["beams"] = e
        finally:
            hook.remove()
        r["gen_cache"], r["seen"] = gen_cache, seen
    finally:
        unpatch_llama(model)
    return r


def test_teacher_forced_beam_decode(run):
    ref, sdpa, smt = run["ref"], run["sdpa"], run["smt"]
    assert smt.shape == ref.shape == (1 + STEPS, ROWS, 512) and torch.isfinite(smt).all()
    cache = run["smt_cache"]
    assert cache.ancestry_updates == 1 + STEPS and all(ly.steps == STEPS for ly in cache.layers)
    # the take-over left dead slots: every row of sample 0 reads step 0 from one slot
    assert len(set(cache.ancestors[:NB, 0].tolist())) == 1
    errs = []
    for t in range(1 + STEPS):
        e, es = _rel(smt[t], ref[t]), _rel(sdpa[t], ref[t])
        print(f"step {t}: smt_flash rel err {e:.3e}, sdpa {es:.3e}, max abs err {(smt[t] - ref[t]).abs().max().item():.3e}")
        errs.append((t, e, es))
    for t, e, es in errs:
        assert e <= max(8e-3, 1.5 * es), (t, e, es)


def test_generate_with_the_beam_shared_cache(run):
    out = run["beams"]
    if isinstance(out, Exception):
        raise out
    assert out.shape == (2, PROMPT + NEW)
    ids, _, _ = _inputs(DEV)
    assert torch.equal(out[:, :PROMPT], ids)
    cache, seen = run["gen_cache"], run["seen"]
    # one prefill, then NEW - 1 decode forwards on buffers that never move
    assert len(seen) == NEW and seen[0] is None
    assert len(set(seen[1:])) == 1
    assert seen[1] == tuple((ly.k_gen.data_ptr(), ly.v_gen.data_ptr()) for ly in cache.layers)
    assert all(ly.steps == NEW - 1 and ly.k_prompt.shape[0] == 2 and ly.k_gen.shape[:3] == (ROWS, 2, NEW)
               for ly in cache.layers)
    # once per generated token for both layers together
    assert cache.ancestry_updates == len(seen)
    assert int(cache.ancestors.max()) < NB
