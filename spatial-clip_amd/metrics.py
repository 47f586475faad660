"""In-batch retrieval metrics with the reference's names: ``ContrastiveMetrics(prefix)`` -> R@1 / R@5 / R@10
(``src/models/components/metrics.py:8-52``).  Hit counting runs on the device (rank of the diagonal among the row)
and is accumulated in int32 counters; ``compute()`` is the only host synchronisation."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import comm, ops      # ops binds the kernel library on first call, not on import: retrieval_summary needs no device


class ContrastiveMetrics:
    KS = (1, 5, 10)

    def __init__(self, prefix: str):
        self.prefix = prefix
        self.hits = None
        self.total = 0

    def _ensure(self, device) -> None:
        if self.hits is None:
            self.hits = torch.zeros(3, dtype=torch.int32, device=device)

    def update(self, logits: torch.Tensor, target: torch.Tensor = None) -> None:
        """logits [B, B'] with the positive of row i at column i (the module always passes target = arange)."""
        B, G = logits.shape
        self._ensure(logits.device)
        ops.recall_hits(logits.contiguous().float(), G, B, 0, self.hits)
        self.total += B

    def add_hits(self, n: int) -> None:
        """Hits were accumulated into ``self.hits`` by the fused loss; only count the rows."""
        self.total += n

    __call__ = update

    def compute(self) -> Dict[str, float]:
        if self.hits is None or self.total == 0:
            return {f"{self.prefix}R@{k}": float("nan") for k in self.KS}
        hits = self.hits.to(torch.float64)
        total = torch.tensor(float(self.total), dtype=torch.float64, device=hits.device)
        if comm.is_dist():            # dist_reduce_fx="sum" of the reference metric states
            both = torch.cat([hits, total.view(1)])
            torch.distributed.all_reduce(both)
            hits, total = both[:3], both[3]
        vals = (hits / total).tolist()
        return {f"{self.prefix}R@{k}": v for k, v in zip(self.KS, vals)}

    def reset(self) -> None:
        if self.hits is not None:
            self.hits.zero_()
        self.total = 0


def check_retrieval_ks(ks) -> tuple:
    ks = tuple(ks)
    if not ks or any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in ks):
        raise ValueError(f"full_retrieval: ks must be a non-empty sequence of positive ints, got {ks!r}")
    return ks


def retrieval_summary(rank_i2t, rank_t2i, ks=(1, 5, 10), prefix: str = "") -> Dict[str, float]:
    """Host half of :class:`RetrievalMetrics`, pure numpy: the quantities of the reference's ``get_clip_metrics``
    (src/open_clip_train/train.py:391-398) under its names, from the 0-based ranks of the ground truth in each direction:
    ``{dir}_mean_rank`` = mean + 1, ``{dir}_median_rank`` = floor(median) + 1, ``{dir}_R@k`` = mean(rank < k) for
    dir in image_to_text, text_to_image, plus ``retrieval_num_samples``."""
    ks = check_retrieval_ks(ks)
    r_i = np.asarray(rank_i2t).astype(np.int64).reshape(-1)
    r_t = np.asarray(rank_t2i).astype(np.int64).reshape(-1)
    if r_i.shape != r_t.shape:
        raise ValueError(f"retrieval_summary: {r_i.shape[0]} image->text ranks vs {r_t.shape[0]} text->image ranks")
    out: Dict[str, float] = {}
    for name, r in (("image_to_text", r_i), ("text_to_image", r_t)):
        if r.size == 0:
            vals = [float("nan")] * (2 + len(ks))
        else:
            vals = [float(r.mean() + 1), float(np.floor(np.median(r)) + 1)] + [float(np.mean(r < k)) for k in ks]
        out[f"{prefix}{name}_mean_rank"], out[f"{prefix}{name}_median_rank"] = vals[0], vals[1]
        for k, v in zip(ks, vals[2:]):
            out[f"{prefix}{name}_R@{k}"] = v
    out[f"{prefix}retrieval_num_samples"] = float(r_i.size)
    return out


class RetrievalMetrics:
    """Full-set retrieval metrics: image->text and text->image mean rank, median rank and R@k over ALL pairs fed since the
    last ``reset()`` -- open_clip's ``get_clip_metrics`` (src/open_clip_train/train.py:383-400), independent of the batch
    size, where :class:`ContrastiveMetrics` ranks a positive among the columns of its own batch only.

    ``update`` appends the fp32 feature rows to two device buffers that grow geometrically (no host sync); ``compute``
    launches ``ops.retrieval_ranks`` once over everything (the N x N similarities are never stored: 2 N D floats of
    features + 2 N ints) and copies the two int32 rank vectors to the host, the only synchronisation.  Memory: a buffer
    doubles when full, so up to twice the stored rows stay allocated per side, and while one side grows its old and its new
    buffer are both alive (three times the stored rows of that side, for the length of one copy).  ``reset()`` keeps the
    buffers: only the first pass over a split grows them.

    Deviations from the reference: ranks are taken on the raw cosines, not on ``logit_scale * cosine`` -- a positive scale
    preserves the order except where its rounding makes or breaks a tie; and ties have a defined order (the stable
    descending sort: equal scores rank by index) where the reference's ``argsort`` leaves it open.  A pair whose own
    similarity is not finite is ranked last."""

    def __init__(self, prefix: str, ks=(1, 5, 10)):
        self.prefix = prefix
        self.ks = check_retrieval_ks(ks)
        self.image = None          # [capacity, D] fp32 each
        self.text = None
        self.n = 0

    def _grow(self, need: int, D: int, device) -> None:
        cap = 0 if self.image is None else self.image.shape[0]
        if self.image is not None and self.image.shape[1] != D:
            raise ValueError(f"RetrievalMetrics: feature width changed from {self.image.shape[1]} to {D}")
        if need <= cap:
            return
        new_cap = max(need, 2 * cap, 1024)
        for name in ("image", "text"):
            buf = torch.empty((new_cap, D), dtype=torch.float32, device=device)
            if self.n:
                buf[:self.n].copy_(getattr(self, name)[:self.n])
            setattr(self, name, buf)

    def update(self, image_features: torch.Tensor, text_features: torch.Tensor) -> None:
        if comm.is_dist():
            raise ValueError("full_retrieval (RetrievalMetrics) is single-process for now: under a process group the "
                             "validation features would have to be gathered and the text->image counts all-reduced")
        if image_features.dim() != 2 or image_features.shape != text_features.shape:
            raise ValueError(f"RetrievalMetrics: expected two [B, D] feature matrices, got {tuple(image_features.shape)} "
                             f"and {tuple(text_features.shape)}")
        B, D = image_features.shape
        if B == 0:
            return
        self._grow(self.n + B, D, image_features.device)
        self.image[self.n:self.n + B].copy_(image_features.detach())
        self.text[self.n:self.n + B].copy_(text_features.detach())
        self.n += B

    __call__ = update

    def ranks(self):
        """(rank_i2t, rank_t2i): device int32 [n] each, one kernel launch, no host sync."""
        return ops.retrieval_ranks(self.image[:self.n], self.text[:self.n])

    def compute(self) -> Dict[str, float]:
        if self.n == 0:
            return retrieval_summary([], [], self.ks, self.prefix)
        r_i, r_t = self.ranks()
        both = torch.stack([r_i, r_t]).cpu().numpy()
        return retrieval_summary(both[0], both[1], self.ks, self.prefix)

    def reset(self) -> None:
        self.n = 0


class ZeroShotGeneExpressionMetric:
    """``src/metrics/zero_shot.py`` with the same constructor, ``update(preds_logits, captions)`` and ``compute()``.

    The caption -> rank-weighted target vector step is string work and stays on the host (one [B, n_genes] float
    matrix per batch, copied once); the sample-wise Pearson correlation and the two metric states (sum of PCC, count)
    live on the device (``sc_pcc_rows``), ``compute()`` is the only host synchronisation and sums the states over
    ranks like the reference's ``dist_reduce_fx="sum"``."""

    def __init__(self, global_hvg_path: Optional[str] = None, dist_sync_on_step: bool = False):
        self.gene_to_idx: Dict[str, int] = {}
        self.num_global_genes = 0
        if global_hvg_path and os.path.exists(global_hvg_path):
            with open(global_hvg_path, "r") as f:
                genes = [line.strip() for line in f if line.strip()]
            self.gene_to_idx = {gene: i for i, gene in enumerate(genes)}
            self.num_global_genes = len(genes)
        self.state = None                      # device float32 [2]: sum_pcc, total_count

    def _compute_rank_weighted_vector(self, caption_list: List[str], device) -> torch.Tensor:
        t = np.zeros((len(caption_list), self.num_global_genes), dtype=np.float32)
        for i, caption in enumerate(caption_list):
            names = caption.split()
            n = len(names)
            for rank, gene in enumerate(names):
                j = self.gene_to_idx.get(gene)
                if j is not None:
                    t[i, j] = 1.0 - (0.8 * rank / max(n, 1))
        return torch.from_numpy(t).to(device, non_blocking=True)

    def update(self, preds_logits: torch.Tensor, captions: List[str]) -> None:
        if self.num_global_genes == 0:
            return
        if preds_logits.shape != (len(captions), self.num_global_genes):
            raise ValueError(f"preds_logits {tuple(preds_logits.shape)} vs {len(captions)} captions x "
                             f"{self.num_global_genes} genes")
        if self.state is None:
            self.state = torch.zeros(2, dtype=torch.float32, device=preds_logits.device)
        targets = self._compute_rank_weighted_vector(captions, preds_logits.device)
        ops.pcc_rows(preds_logits.float().contiguous(), targets, None, self.state)

    __call__ = update

    def compute(self) -> float:
        if self.state is None:
            return 0.0
        st = self.state.to(torch.float64)
        if comm.is_dist():
            torch.distributed.all_reduce(st)
        s, n = st.tolist()
        return s / n if n > 0 else 0.0

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()
