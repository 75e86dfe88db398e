"""A KV cache for beam search that never moves K / V (:class:`BeamSharedCache`).

transformers' ``DynamicCache`` under ``generate(num_beams=nb)`` copies the whole cache twice per
generated token and layer (``reorder_cache``: ``index_select``; ``update``: ``torch.cat``) and holds the
prompt's K / V once per beam although the beams of a sample share it. This cache stores the prompt once
per sample, writes each step's K / V into pre-allocated buffers at the row ("physical slot") that
produced it, and keeps ONE small ancestry table for all layers: ``anc[r, j]`` is the slot of row r's
sample that holds the step-j key of the hypothesis row r carries now. ``reorder_cache`` permutes that
table and nothing else; the decode attention (``smt_attn_fwd_beams``, include/smt_attention.h; reached
through ``smt_flash`` on a :func:`~sparse_matrix_tuning_amd.fused_llama.patch_llama`-ed model) reads
every physical row once per sample and decides by comparison which beam sees it.

With ``device_steps=True`` the number of generated positions also lives in ONE int32 counter on the
device, shared by all layers: ``update`` appends through ``smt_attn_kv_append_pos`` at the row the
counter names and returns the whole buffers, and the attention (``smt_attn_fwd_beams_pos``) reads the
counter itself, so no launch parameter of a decode step depends on the step and the step can be
captured in a graph and replayed (``graph=True``: the decode runner of
:mod:`~sparse_matrix_tuning_amd.fused_llama` does that on a ``patch_llama``-ed model).

The bookkeeping here is plain torch and runs on CPU tensors as well (tests/test_attention_beams_host.py,
tests/test_attention_beams_pos_host.py).
"""
from __future__ import annotations

import torch
from transformers.cache_utils import Cache, CacheLayerMixin


class _BeamState:
    """What the layers of one :class:`BeamSharedCache` share: the beam count, the capacity and the
    ancestry table (allocated by the first prefill ``update``). With ``device_steps``: also the int32
    counter of generated positions (the current token's included; allocated with the table, advanced
    once per forward) and the prompt's key-mask words (built at the first decode step)."""

    def __init__(self, num_beams: int, max_new_tokens: int, device_steps: bool = False):
        self.num_beams, self.capacity = int(num_beams), int(max_new_tokens)
        self.anc = None                    # uint8 [N * nb, capacity]
        self.reorders = 0                  # ancestry updates so far (one per generated token)
        self.device_steps = bool(device_steps)
        self.counter = None                # int32 [1] (device_steps)
        self.prompt_mask = None            # (KeyMask or None,) once the first decode step has built it

    def ensure(self, rows: int, device) -> None:
        if self.anc is None:
            # every column starts as "my own slot": the entry a row writes at step j is its own until a
            # reorder hands the row another hypothesis, and reorders only touch the steps written so far
            own = (torch.arange(rows, device=device) % self.num_beams).to(torch.uint8)
            self.anc = own[:, None].repeat(1, self.capacity).contiguous()
            if self.device_steps:
                self.counter = torch.zeros(1, dtype=torch.int32, device=device)
        elif self.anc.shape[0] != rows or self.anc.device != device:
            raise ValueError(f"BeamSharedCache: {rows} rows on {device}, the ancestry table has "
                             f"{self.anc.shape[0]} on {self.anc.device}")


class BeamSharedLayer(CacheLayerMixin):
    """One layer of a :class:`BeamSharedCache`: ``k_prompt`` / ``v_prompt`` ``[N, Hkv, P, D]`` (one copy
    per sample), ``k_gen`` / ``v_gen`` ``[N * nb, Hkv, capacity, D]`` (row = physical slot, position =
    generation step) and ``steps``, the number of generated positions written."""

    is_compileable = False
    is_sliding = False

    def __init__(self, state: _BeamState, index: int = 0):
        super().__init__()
        self.state = state
        self.index = index                 # layer 0 advances the shared device counter
        self.k_prompt = self.v_prompt = self.k_gen = self.v_gen = None
        self.prompt_len = 0
        self.steps = 0

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        nb, cap = self.state.num_beams, self.state.capacity
        rows, hkv, plen, dim = key_states.shape
        if rows % nb:
            raise ValueError(f"BeamSharedCache: {rows} rows are no multiple of num_beams = {nb} (generate() expands "
                             "the batch to batch * num_beams rows before the prefill)")
        self.dtype, self.device = key_states.dtype, key_states.device
        self.state.ensure(rows, key_states.device)
        # the beams of a sample hold identical prompt rows: keep the first of each group
        self.k_prompt = key_states[::nb].contiguous()
        self.v_prompt = value_states[::nb].contiguous()
        self.prompt_len = plen
        self.k_gen = torch.empty(rows, hkv, cap, dim, dtype=key_states.dtype, device=key_states.device)
        self.v_gen = torch.empty_like(self.k_gen)
        self.keys, self.values = self.k_gen, self.v_gen
        self.is_initialized = True

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        """The prefill (the first call) stores rows ``[::nb]`` as the prompt segment and returns its
        inputs: the prefill attention is the same-length call it always was. A decode call writes the
        step's K / V into the generated buffers in place (no ``cat``) and returns views of them that
        carry this layer as ``_smt_beam``, which is what ``smt_flash`` routes on. With ``device_steps``
        the decode call goes through :meth:`_update_device_steps` and returns the whole buffers."""
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
            return key_states, value_states
        if key_states.shape[2] != 1:
            raise NotImplementedError(f"BeamSharedCache: {key_states.shape[2]} new positions after the prefill "
                                      "(one decode position per call)")
        if key_states.shape[0] != self.k_gen.shape[0]:
            raise ValueError(f"BeamSharedCache: {key_states.shape[0]} rows, the cache holds {self.k_gen.shape[0]}")
        t = self.steps
        if t >= self.state.capacity:
            raise RuntimeError(f"BeamSharedCache: max_new_tokens = {self.state.capacity} generated positions are full")
        if self.state.device_steps:
            return self._update_device_steps(key_states, value_states)
        self.k_gen[:, :, t:t + 1].copy_(key_states)
        self.v_gen[:, :, t:t + 1].copy_(value_states)
        self.steps = t + 1
        k, v = self.k_gen[:, :, :t + 1], self.v_gen[:, :, :t + 1]
        k._smt_beam = v._smt_beam = self
        return k, v

    def _update_device_steps(self, key_states, value_states):
        """The decode ``update`` with the counter on the device: layer 0 advances it (once per forward),
        every layer appends at row ``clamp(counter, 1, capacity) - 1`` and returns the WHOLE buffers,
        tagged; the attention reads the counter. The host's ``steps`` follows for ``get_seq_length``,
        the capacity check above and ``reorder_cache``. Nothing here depends on the step but that
        count, so the launches of one step are those of every step."""
        st = self.state
        if self.index == 0:
            st.counter.add_(1)
        if self.k_gen.device.type == "cuda":
            from .fused_llama import kv_append
            kv_append(key_states, value_states, self.k_gen, self.v_gen, st.counter)
        else:
            row = st.counter.clamp(1, st.capacity).long() - 1
            self.k_gen.index_copy_(2, row, key_states)
            self.v_gen.index_copy_(2, row, value_states)
        self.steps += 1
        k, v = self.k_gen[:], self.v_gen[:]
        k._smt_beam = v._smt_beam = self
        return k, v

    def get_seq_length(self) -> int:
        return self.prompt_len + self.steps if self.is_initialized else 0

    def get_mask_sizes(self, query_length: int) -> tuple[int, int]:
        return self.get_seq_length() + query_length, 0

    def get_max_length(self) -> int:
        return self.prompt_len + self.state.capacity if self.is_initialized else -1

    def reset(self) -> None:
        self.k_prompt = self.v_prompt = self.k_gen = self.v_gen = self.keys = self.values = None
        self.prompt_len = self.steps = 0
        self.is_initialized = False

    def gather(self):
        """The per-row ``[N * nb, Hkv, P + steps, D]`` K / V a ``DynamicCache`` would hold (copies)."""
        nb, t = self.state.num_beams, self.steps
        rows = self.k_gen.shape[0]
        first = torch.arange(rows, device=self.k_gen.device) // nb * nb
        src = first[:, None] + self.state.anc[:, :t].long()            # [rows, t]: the row that holds step j
        step = torch.arange(t, device=self.k_gen.device)[None, :]
        out = []
        for prompt, gen in ((self.k_prompt, self.k_gen), (self.v_prompt, self.v_gen)):
            g = gen[src, :, step].permute(0, 2, 1, 3)                  # [rows, Hkv, t, D]
            out.append(torch.cat([prompt.repeat_interleave(nb, dim=0), g], dim=2))
        return out[0], out[1]

    def reorder_cache(self, beam_idx: torch.LongTensor) -> None:
        raise NotImplementedError("BeamSharedCache: the ancestry table is shared; call the cache's reorder_cache")

    def offload(self):
        raise NotImplementedError("BeamSharedCache: offloading is not supported")

    def crop(self, tokens_to_remove: int) -> None:
        raise NotImplementedError("BeamSharedCache: crop is not supported")

    def batch_repeat_interleave(self, repeats: int) -> None:
        raise NotImplementedError("BeamSharedCache: batch_repeat_interleave is not supported (pass the cache to "
                                  "generate(num_beams=...), which expands the batch before the prefill)")

    def batch_select_indices(self, indices: torch.Tensor) -> None:
        raise NotImplementedError("BeamSharedCache: batch_select_indices is not supported")


class BeamSharedCache(Cache):
    """``generate(..., num_beams=nb, past_key_values=BeamSharedCache(model.config, nb, max_new_tokens))`` on a
    ``patch_llama``-ed model. ``max_new_tokens`` is the capacity of the generated buffers (a decode step
    beyond it raises). One cache serves one ``generate()`` call.

    Keys of generated positions are always valid: the prompt's padding comes from the 2-D
    ``attention_mask`` (rows ``[::nb]``, the first ``prompt_len`` columns), the columns ``generate()``
    appends for generated tokens are not consulted.

    ``ancestors``: uint8 ``[N * nb, max_new_tokens]``; ``ancestors[r, j]`` for ``j <`` the steps written
    is the slot (0..nb-1, row ``r // nb * nb + slot`` of the generated buffers) whose position j holds
    the step-j key of row r's hypothesis. ``reorder_cache(beam_idx)`` is
    ``ancestors[r, :t] = ancestors[beam_idx[r], :t]``: once per generated token for all layers, a few
    hundred bytes; K / V never move. ``beam_idx`` must stay within each sample's rows, as beam search's does.
    """

    def __init__(self, config, num_beams: int, max_new_tokens: int, device_steps: bool = False, graph: bool = False):
        if int(num_beams) < 1 or int(num_beams) > 255:
            raise ValueError(f"BeamSharedCache: num_beams = {num_beams} (1..255: slots are stored as uint8)")
        if int(max_new_tokens) < 1:
            raise ValueError(f"BeamSharedCache: max_new_tokens = {max_new_tokens}")
        self.graph = bool(graph)
        self.state = _BeamState(num_beams, max_new_tokens, device_steps=bool(device_steps) or self.graph)
        self.graph_captures = self.graph_replays = 0       # the decode runner's (fused_llama.py)
        self.decode_runner = None
        cfg = config.get_text_config(decoder=True) if hasattr(config, "get_text_config") else config
        super().__init__(layers=[BeamSharedLayer(self.state, i) for i in range(cfg.num_hidden_layers)])

    @property
    def num_beams(self) -> int:
        return self.state.num_beams

    @property
    def device_steps(self) -> bool:
        return self.state.device_steps

    @property
    def steps_tensor(self):
        """The int32 ``[1]`` counter of generated positions on the cache's device (``device_steps``), or None."""
        return self.state.counter

    @property
    def ancestors(self):
        return self.state.anc

    @property
    def ancestry_updates(self) -> int:
        """How many times ``reorder_cache`` has run (once per generated token, not once per layer)."""
        return self.state.reorders

    def reorder_cache(self, beam_idx: torch.LongTensor) -> None:
        st = self.state
        st.reorders += 1
        t = self.layers[0].steps
        if st.anc is None or t == 0:
            return                          # only the prompt so far, and the beams of a sample share it
        if any(layer.steps != t for layer in self.layers):
            raise RuntimeError("BeamSharedCache: reorder_cache between the layers of one forward")
        st.anc[:, :t] = st.anc.index_select(0, beam_idx.to(st.anc.device))[:, :t]

    def gather(self, layer_idx: int):
        return self.layers[layer_idx].gather()

    def reset(self):
        for layer in self.layers:
            layer.reset()
        if self.state.counter is not None:
            self.state.counter.zero_()                  # for whoever still holds it; a new one comes with the table
        self.state.anc = self.state.counter = self.state.prompt_mask = None
        self.state.reorders = 0
        self.decode_runner = None

    def crop(self, tokens_to_remove: int) -> None:
        raise NotImplementedError("BeamSharedCache: crop is not supported")

    def batch_repeat_interleave(self, repeats: int):
        raise NotImplementedError("BeamSharedCache: batch_repeat_interleave is not supported (pass the cache to "
                                  "generate(num_beams=...), which expands the batch before the prefill)")

    def batch_select_indices(self, indices: torch.Tensor):
        raise NotImplementedError("BeamSharedCache: batch_select_indices is not supported")
