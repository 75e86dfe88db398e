"""A BeamSharedCache(graph=True) and its DecodeGraph are no reference cycle: dropping the cache frees both at
once (and with them the captured graph and its private pool), not at a later garbage collection, which may
come inside another cache's capture. No GPU: nothing here touches a device."""
import gc
import weakref


def _config():
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                       num_key_value_heads=2, head_dim=128, vocab_size=512, max_position_embeddings=64)


def test_a_dropped_cache_frees_its_runner_without_the_collector():
    from sparse_matrix_tuning_amd.beam_cache import BeamSharedCache
    from sparse_matrix_tuning_amd.fused_llama import DecodeGraph
    was_on = gc.isenabled()
    gc.disable()
    try:
        cache = BeamSharedCache(_config(), 4, 8, graph=True)
        cache.decode_runner = DecodeGraph(cache)
        assert cache.decode_runner.cache is cache
        dead = [weakref.ref(cache), weakref.ref(cache.decode_runner)]
        del cache
        assert all(r() is None for r in dead)
    finally:
        if was_on:
            gc.enable()
