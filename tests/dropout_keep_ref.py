"""numpy restatement of the attention-dropout keep function (include/smt_attention.h), written from
the header's definition and shared by tests/test_attention_dropout_host.py (statistics) and
tests/test_gpu_attention_dropout.py (bit-for-bit against the kernels' exported mask)."""
import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def mix(x):
    """uint32 arithmetic with wrap-around, carried in uint64 arrays (products masked to 32 bits)."""
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x21F0AAAD)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x735A2D97)) & _M32
    x = x ^ (x >> np.uint64(15))
    return x


def threshold(p: float) -> int:
    """t = clamp(floor(p * 256 + 0.5), 0, 255) in fp32, as the library computes it."""
    t = math.floor(float(np.float32(p) * np.float32(256.0) + np.float32(0.5)))
    return min(max(t, 0), 255)


def keep_mask(B: int, Hq: int, S: int, p: float, seed: int) -> np.ndarray:
    """bool [B, Hq, S, S]: element (b, h, q, key) is kept."""
    seed = int(seed) & (2 ** 64 - 1)
    seed_lo, seed_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    t = threshold(p)
    bh = np.arange(B * Hq, dtype=np.uint64)
    head_key = mix((seed_lo + bh * np.uint64(0x9E3779B9)) & _M32) ^ seed_hi                        # [BH]
    q = np.arange(S, dtype=np.uint64)
    row_key = mix((head_key[:, None] + ((q * np.uint64(0x85EBCA6B)) & _M32)[None, :]) & _M32)     # [BH, S]
    key = np.arange(S, dtype=np.uint64)
    key_term = ((key >> np.uint64(2)) * np.uint64(0x9E3779B1)) & _M32
    word = mix(row_key[:, :, None] ^ key_term[None, None, :])                                     # [BH, S, S]
    byte = (word >> (np.uint64(8) * (key & np.uint64(3)))[None, None, :]) & np.uint64(0xFF)
    return (byte >= np.uint64(t)).reshape(B, Hq, S, S)
