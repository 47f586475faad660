"""FLIP patch dropout: which patch tokens a training forward of the vision tower keeps.

Reference: ``PatchDropout`` (src/open_clip/transformer.py:48-89), applied in ``VisionTransformer._embeds`` (:794) after the
positional embedding and before ``ln_pre``: per image a uniformly random ``K = max(1, int(n * (1 - p)))`` of the ``n`` patch
tokens survive, the class token always does.  The reference keeps them in ``topk`` (random) order; this build keeps them in
ascending patch order -- the class-token feature and every gradient are invariant to the token order, because the positions
are added before the drop.

The subset is a pure function of four integers -- (seed, draw, sample, patch) -> 32-bit key through murmur3's finaliser, the
``K`` smallest ``(key, patch)`` are kept -- so the device kernel (``sc_patch_keep``) needs no generator state, ranks draw
differently (``sample0 = rank * B``) and a resumed run continues the sequence from the ``draw`` counter alone.  This module
is the host restatement of that kernel, bit for bit, in numpy: tests, oracles and tools use it to know what the device drew."""
from __future__ import annotations

import numpy as np

GOLDEN = 0x9E3779B9
_M32 = 0xFFFFFFFF


def num_keep(n: int, p: float) -> int:
    """Patch tokens kept out of ``n`` at dropout fraction ``p`` (transformer.py:73: ``max(1, int(num_tokens * keep_prob))``)."""
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"patch dropout {p!r}: must be in [0, 1)")
    return max(1, int(int(n) * (1.0 - float(p))))


def check_fraction(p) -> float:
    """``p`` as a float in [0, 1), else ValueError (the reference asserts ``0 <= prob < 1.``, transformer.py:56)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"patch dropout {p!r}: must be in [0, 1)")
    return p


def mix32(h: np.ndarray) -> np.ndarray:
    """murmur3's 32-bit finaliser on uint32 arrays (wrapping arithmetic)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def patch_keys(seed: int, draw: int, sample0: int, B: int, n: int) -> np.ndarray:
    """uint32 [B, n]: the sort keys of sample ``sample0 + b``'s patches at draw ``draw``."""
    with np.errstate(over="ignore"):
        h = mix32(np.array([(int(seed) + GOLDEN) & _M32], dtype=np.uint32))
        h = mix32(h ^ np.uint32(int(draw) & _M32))
        sample = ((int(sample0) + np.arange(B, dtype=np.int64)) & _M32).astype(np.uint32)
        h = mix32(h ^ sample)                                                    # [B]
        j = ((np.arange(n, dtype=np.int64) * GOLDEN) & _M32).astype(np.uint32)   # [n]
        return mix32(h[:, None] ^ j[None, :])


def keep_indices_host(seed: int, draw: int, sample0: int, B: int, n: int, K: int) -> np.ndarray:
    """int32 [B, K], ascending per row: the patches ``sc_patch_keep`` keeps for the same arguments."""
    if not (B > 0 and 0 < K <= n):
        raise ValueError(f"keep_indices_host: bad shape B={B} n={n} K={K}")
    keys = patch_keys(seed, draw, sample0, B, n)
    order = np.argsort(keys, axis=1, kind="stable")          # by (key, patch): a stable sort breaks ties by index
    return np.sort(order[:, :K], axis=1).astype(np.int32)


def slots_from_keep(keep: np.ndarray, n: int) -> np.ndarray:
    """int32 [B, n]: the kept position of patch j in sample b, or -1 (the inverse map the embedding backward walks)."""
    keep = np.asarray(keep)
    B, K = keep.shape
    slot = np.full((B, n), -1, dtype=np.int32)
    slot[np.arange(B)[:, None], keep] = np.arange(K, dtype=np.int32)[None, :]
    return slot


def validate_keep(idx, B: int, n: int, K: int) -> np.ndarray:
    """An explicit index set (SpatialClipNet.set_patch_keep) as int32 [B, K]: integer, in range, strictly ascending per row."""
    a = np.asarray(idx.detach().cpu().numpy() if hasattr(idx, "detach") else idx)
    if a.dtype.kind not in "iu":
        raise TypeError(f"patch keep indices must be integers, got {a.dtype}")
    if a.shape != (B, K):
        raise ValueError(f"patch keep indices must be [{B}, {K}] (batch, kept patches), got {tuple(a.shape)}")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"patch keep indices must lie in [0, {n})")
    if K > 1 and not (np.diff(a, axis=1) > 0).all():
        raise ValueError("patch keep indices must be strictly ascending per row")
    return a.astype(np.int32)
