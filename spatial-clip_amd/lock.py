"""Locked towers (LiT, https://arxiv.org/abs/2111.07991): which parameters ``CLIP.lock_image_tower(unlocked_groups)`` /
``CLIP.lock_text_tower(unlocked_layers)`` of the reference freeze (src/open_clip/model.py:304-310, transformer.py:710-741 and
:1360-1455), and what that means for the flat buffers.  Pure host code: importing it needs no device.

A locked parameter has ``requires_grad=False`` in the reference, so AdamW never sees it: no update, no decoupled weight decay, no
moments; the clip norm and the gradient exchange cover the trainable gradients only.  Here that becomes a shorter schedule of the
same launches: the backward stops at the first trainable block (the tower's *floor*), and the optimiser, the norm, the
accumulator and the reducer run over ``trainable_ranges`` of the flat buffers instead of the whole of them."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

_BLOCK_LEAVES = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                 "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                 "mlp.c_proj.bias")


def _block(prefix: str, i: int) -> List[str]:
    return [f"{prefix}{i}.{leaf}" for leaf in _BLOCK_LEAVES]


def vision_groups(layers: int, no_ln_pre: bool = False) -> List[List[str]]:
    """VisionTransformer.lock's groups, in its order: stem, each of resblocks[:-1], [resblocks[-1], ln_post], proj."""
    stem = ["visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding"]
    if not no_ln_pre:
        stem += ["visual.ln_pre.weight", "visual.ln_pre.bias"]
    pre = "visual.transformer.resblocks."
    groups = [stem] + [_block(pre, i) for i in range(layers - 1)]
    groups.append(_block(pre, layers - 1) + ["visual.ln_post.weight", "visual.ln_post.bias"])
    groups.append(["visual.proj"])
    return groups


def text_groups(layers: int) -> List[List[str]]:
    """lock_text_tower's groups: embeddings, each of resblocks[:-1], [resblocks[-1], ln_final], text_projection."""
    pre = "transformer.resblocks."
    groups = [["token_embedding.weight", "positional_embedding"]] + [_block(pre, i) for i in range(layers - 1)]
    groups.append(_block(pre, layers - 1) + ["ln_final.weight", "ln_final.bias"])
    groups.append(["text_projection"])
    return groups


def check_count(value, what: str) -> int:
    ok = isinstance(value, int) and not isinstance(value, bool) and value >= 0
    if not ok:
        raise ValueError(f"{what}={value!r}: an integer >= 0 (the number of parameter groups, counted from the output end, "
                         "that stay trainable)")
    return int(value)


def split_groups(groups: Sequence[Sequence[str]], unlocked: int) -> Tuple[List[str], List[str]]:
    """(locked names, trainable names) of a tower whose last ``unlocked`` groups stay trainable (a count past the number of
    groups unlocks everything, as ``groups[-n:]`` does in the reference)."""
    n = min(int(unlocked), len(groups))
    cut = len(groups) - n
    locked = [name for g in groups[:cut] for name in g]
    free = [name for g in groups[cut:] for name in g]
    return locked, free


class TowerLock:
    """What a tower's forward / backward need to know of its lock: ``floor`` = index of the first trainable block (``layers``:
    no block is trainable), whether the stem and the output projection are trainable.  ``None`` counts mean "not locked"."""

    def __init__(self, layers: int, unlocked: Optional[int] = None):
        self.layers = int(layers)
        n_groups = self.layers + 2
        g = n_groups if unlocked is None else min(int(unlocked), n_groups)
        self.unlocked = g
        self.proj = g >= 1
        self.stem = g >= n_groups
        self.floor = max(0, self.layers + 1 - g) if g >= 2 else self.layers

    @property
    def any_trainable(self) -> bool:
        return self.proj

    @property
    def head_only(self) -> bool:
        """Only the output projection is trainable: the tower's backward is that one weight gradient."""
        return self.proj and self.floor >= self.layers


def check_lock_request(precision: str, exchange_mode: str) -> None:
    """The two refusals of a lock, before anything is built.  ValueError."""
    if str(precision).startswith("fp8"):
        raise ValueError("a locked tower with precision='fp8' is not supported: the delayed e4m3 scales of blocks whose "
                         "backward never runs would never be updated; use precision='bf16' with a lock")
    if exchange_mode == "sharded":
        raise ValueError("a locked tower with SC_GRAD_EXCHANGE=sharded is not supported: the sharded exchange splits every "
                         "bucket of the whole flat buffer over the ranks; use SC_GRAD_EXCHANGE=allreduce (the default)")


def merge_ranges(specs, locked, total: int, align: int) -> List[Tuple[int, int]]:
    """Merged, sorted (lo, hi) ranges of a flat buffer laid out by ``specs`` (``.name``, ``.offset``, ``.numel``; each spec
    takes its size rounded up to ``align`` floats) that hold parameters outside ``locked``.  The last spec's range runs to
    ``total``: it takes the zero padding behind it."""
    out: List[Tuple[int, int]] = []
    for k, s in enumerate(specs):
        if s.name in locked:
            continue
        lo = s.offset
        hi = total if k == len(specs) - 1 else s.offset + (max(s.numel, 1) + align - 1) // align * align
        if out and out[-1][1] == lo:
            out[-1] = (out[-1][0], hi)
        else:
            out.append((lo, hi))
    return out


def intersect(ranges: Sequence[Tuple[int, int]], lo: int, hi: int) -> List[Tuple[int, int]]:
    """The parts of [lo, hi) inside the sorted, disjoint ``ranges``."""
    return [(max(a, lo), min(b, hi)) for a, b in ranges if a < hi and lo < b]
