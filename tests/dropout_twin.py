"""Host replica of the dropout masks the HIP kernels draw (a test helper, like helpers.py), bit for bit.

Restates, in numpy uint32 arithmetic with wrap-around:
  * `medp_mix_epoch`  (multimodal_edema_prediction_amd/csrc/common.h:89): seed + epoch * 0x9E3779B9, or the seed itself when no epoch
    counter is registered (medp_rng_set_epoch_ptr(NULL));
  * `medp_hash`       (common.h:203-208): one 32-bit hash per (seed, stream id, element index);
  * `dropout_scale`   (common.h:210-213): keep iff (h >> 8) * 2^-24 >= p in fp32, kept elements scaled by 1 / (1 - p);
  * the fp32 scale every launcher passes, `1.f / (1.f - p)` (fusion_ops.hip, attention_small.hip, attention_fq_split.hip,
    attention_dh16.hip);
  * the element index of each layout: the flat index of a contiguous tensor (fusion_ops.hip: gelu_dropout_*, dropout_add) and
    ((b * H + h) * Lq + q) * Lk + j for attention probabilities (attention_small.hip, attention_fq_split.hip; attention_dh16.hip
    with Lq = Lk = N), in uint32.
"""
from __future__ import annotations

import contextlib

import numpy as np

U32 = np.uint32


def _u32(x) -> np.ndarray:
    """uint32 view of an int or an integer array, wrapped modulo 2^32."""
    if isinstance(x, np.ndarray):
        return x.astype(U32)
    return np.asarray(int(x) & 0xFFFFFFFF, dtype=U32)


def mix_epoch(seed: int, epoch) -> np.ndarray:
    """The per-launch seed after the RNG epoch is mixed in; `epoch` None = no counter registered."""
    s = _u32(seed)
    if epoch is None:
        return s
    with np.errstate(over="ignore"):
        return (s + _u32(epoch) * U32(0x9E3779B9)).astype(U32)


def medp_hash(seed, sid, idx) -> np.ndarray:
    seed = _u32(seed)
    sid = _u32(sid)
    x = _u32(idx)
    with np.errstate(over="ignore"):
        x = (x * U32(0x9E3779B1)) ^ (seed + U32(0x7F4A7C15) * (sid + U32(1)))
        x ^= x >> U32(16)
        x *= U32(0x85EBCA6B)
        x ^= x >> U32(13)
        x *= U32(0xC2B2AE35)
        x ^= x >> U32(16)
        x += seed * U32(0x27D4EB2F)
        x ^= x >> U32(15)
        x *= U32(0x2C1B3C6D)
        x ^= x >> U32(12)
    return x.astype(U32)


def uniform(seed: int, sid: int, idx, epoch=None) -> np.ndarray:
    """fp32 u = (h >> 8) * 2^-24 in [0, 1), the number `dropout_scale` compares with p (seed: the per-call seed)."""
    h = medp_hash(mix_epoch(seed, epoch), sid, idx)
    return (h >> U32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(seed: int, sid: int, idx, p: float, epoch=None) -> np.ndarray:
    """bool mask: True where the kernels keep the element."""
    return uniform(seed, sid, idx, epoch) >= np.float32(p)


def scale(p: float) -> np.float32:
    """The fp32 factor kept elements are multiplied by."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def mask_scale(seed: int, sid: int, idx, p: float, epoch=None) -> np.ndarray:
    """fp32 keep_mask * scale(p): exactly the factor `dropout_scale` returns per element."""
    return np.where(keep_mask(seed, sid, idx, p, epoch), scale(p), np.float32(0)).astype(np.float32)


def flat_index(shape) -> np.ndarray:
    """Element-wise kernels: the flat index of the contiguous tensor (truncated to uint32 as the kernels do)."""
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(U32).reshape(shape)


def attn_index(B: int, H: int, Lq: int, Lk: int) -> np.ndarray:
    """Attention probabilities [B, H, Lq, Lk]: ((b * H + h) * Lq + q) * Lk + j in uint32."""
    b = np.arange(B, dtype=U32).reshape(B, 1, 1, 1)
    h = np.arange(H, dtype=U32).reshape(1, H, 1, 1)
    q = np.arange(Lq, dtype=U32).reshape(1, 1, Lq, 1)
    j = np.arange(Lk, dtype=U32).reshape(1, 1, 1, Lk)
    with np.errstate(over="ignore"):
        return (((b * U32(H) + h) * U32(Lq) + q) * U32(Lk) + j).astype(U32)


@contextlib.contextmanager
def pinned_epoch(value, device="cuda"):
    """Pin the library's RNG epoch for a GPU test: register an int32 counter holding `value` (None: no counter), and hand the
    registration back to its previous owner (graph_step._EPOCH_OWNER) on exit, so tests may run in any order.  Yields the counter."""
    import torch
    from multimodal_edema_prediction_amd import graph_step
    from multimodal_edema_prediction_amd.abi import check, lib

    def register(t):
        if t is None:
            check(lib().medp_rng_set_epoch_ptr(None), "rng_set_epoch_ptr")
            graph_step._EPOCH_OWNER[0] = None
        else:
            graph_step._register_epoch(t)

    prev = graph_step._EPOCH_OWNER[0]
    ep = None if value is None else torch.full((1,), int(value), dtype=torch.int32, device=device)
    try:
        register(ep)
        yield ep
    finally:
        torch.cuda.synchronize()
        register(prev)
