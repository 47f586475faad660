"""ClipLoss / SpatialLoss / SigLipLoss / DistillClipLoss with the reference's constructor kwargs, forward kwargs and return contract
(``{"contrastive_loss": 0-d tensor}``), computed by the fused device-side contrastive head.

Mirrors ``src/models/components/losses.py:11-141`` (SpatialLoss; ClipLoss wrapper over open_clip's ClipLoss,
``src/open_clip/loss.py:68-155``).  Distributed behaviour is the INTENDED one: rank / world size
are read from the live process group at call time, the global batch is formed with one packed all-gather and the
gradient of the gather (``gather_with_grad=True``) is one reduce-scatter."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import comm, ops
from .contrastive import contrastive_forward_backward, distill_forward_backward, siglip_forward_backward


class _ContrastiveFn(torch.autograd.Function):
    """Forward computes the loss AND its feature / scale / bias gradients (for an upstream gradient of 1); backward
    scales them by the actual upstream gradient.  ``logit_bias`` (may be None) is an autograd input: its gradient is
    the d_bias the loss kernels form anyway."""

    @staticmethod
    def forward(ctx, image_features, text_features, logit_scale, logit_bias, owner, kw):
        rank, W = comm.world()
        dist_on = comm.is_dist()
        ids_i, ids_t = kw.get("image_tile_ids"), kw.get("text_tile_ids")
        img = image_features.detach().contiguous().float()
        txt = text_features.detach().contiguous().float()
        B, D = img.shape
        all_i = all_t = all_ids_i = all_ids_t = late = None
        fg = owner.prefetched
        need_ids = owner.mode == "spatial"
        if dist_on and fg is not None and fg.has("text", txt) and fg.has("image", img) \
                and (not need_ids or fg.with_ids("text")):
            # the gathers were launched from inside the net's forward on the communication stream; the image
            # features are only waited for after the first similarity GEMM has been enqueued
            all_t, all_ids_i, all_ids_t = fg.take("text")
            late = lambda: fg.take("image")[0]
        elif dist_on:
            all_i, all_t, all_ids_i, all_ids_t = comm.gather_packed(img, txt, ids_i if need_ids else None,
                                                                     ids_t if need_ids else None)
        common = dict(mode=owner.mode, image_tile_ids=ids_i, text_tile_ids=ids_t, all_image_tile_ids=all_ids_i,
                      all_text_tile_ids=all_ids_t, neighbor_tile_ids=kw.get("neighbor_tile_ids"),
                      neighbor_alphas=kw.get("neighbor_alphas"), cap_logit_scale=owner.cap_logit_scale,
                      temp_reg_weight=owner.temp_reg_weight, neighbor_alpha_scale=owner.neighbor_alpha_scale,
                      logit_bias=logit_bias, recall_hits=owner.recall_hits, want_recall=False)
        if dist_on and owner.mode == "clip" and not owner.local_loss:
            # loss.py:119-121: every rank forms the full [G,G] logits of the global batch (labels arange(G))
            if late is not None:
                all_i = late()
            res = contrastive_forward_backward(all_i, all_t, logit_scale.detach(), rank=0,
                                               recall_rows=(rank * B, B), **common)
            tot = torch.cat([res["d_image"] + res["d_all_image"], res["d_text"] + res["d_all_text"]], dim=1)
            if owner.gather_with_grad:
                both = comm.reduce_scatter_sum(tot)                 # every rank contributes its (identical) full-loss term
            else:
                both = tot[rank * B:(rank + 1) * B]                  # loss.py:58-61: only the spliced local shard has grad
            d_img, d_txt = both[:, :D].contiguous(), both[:, D:].contiguous()
        else:
            res = contrastive_forward_backward(img, txt, logit_scale.detach(), all_image=all_i, all_text=all_t,
                                               rank=rank if dist_on else 0, late_all_image=late, join_local=not dist_on,
                                               **common)
            if dist_on and owner.gather_with_grad:
                # autograd of torch.distributed.nn.all_gather (loss.py:50-52): SUM over ranks, keep own rows
                both = comm.reduce_scatter_sum(res["d_all"])
                d_img = res["d_image"] + both[:, :D]
                d_txt = res["d_text"] + both[:, D:]
            elif dist_on:
                d_img, d_txt = res["d_image"], res["d_text"]     # loss.py:54-63 with local_loss: remote shards detached
            else:           # single process: the head's GEMMs accumulated the gathered-feature terms onto the direct ones
                d_img, d_txt = res["d_image"], res["d_text"]
        ctx.flat = res["grads"] if d_img is res["d_image"] and d_txt is res["d_text"] else None
        ctx.save_for_backward(d_img, d_txt, res["d_scale"], res["d_bias"])
        owner.last = res
        return res["loss"]

    @staticmethod
    def backward(ctx, g):
        d_img, d_txt, d_s, d_b = ctx.saved_tensors
        g = g.detach().reshape(1).float()
        want_b = ctx.needs_input_grad[3]
        if ctx.flat is not None and g.is_cuda:     # d_image | d_text | d_scale | d_bias are one buffer: one launch applies the upstream gradient
            out = ops.scale_by_scalar(ctx.flat, g, torch.empty_like(ctx.flat))
            n = d_img.numel()
            return out[:n].view_as(d_img), out[n:2 * n].view_as(d_txt), out[2 * n], \
                (out[2 * n + 1] if want_b else None), None, None
        return d_img * g, d_txt * g, d_s * g, (d_b * g if want_b else None), None, None


class _LossBase(torch.nn.Module):
    mode = "clip"
    cap_logit_scale: Optional[float] = None
    temp_reg_weight: float = 0.0
    neighbor_alpha_scale: float = 1.0

    def _init_common(self, local_loss, gather_with_grad, rank, world_size, use_horovod):
        if use_horovod:
            raise NotImplementedError("Horovod is out of scope (SURVEY.md 2.1); use torch.distributed / RCCL")
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.use_horovod = use_horovod
        # rank / world_size ctor kwargs are accepted for signature parity (loss.py:71-78) but the LIVE process group
        # decides at call time: under Lightning the reference constructs its losses before the group exists and
        # therefore never gathers ("distributed quirk"); the intended behaviour is built here
        self.recall_hits: Optional[torch.Tensor] = None
        self.prefetched: Optional[comm.FeatureGather] = None      # set by the module: gathers launched inside the net
        self.last: Dict[str, torch.Tensor] = {}

    @property
    def rank(self) -> int:
        return comm.world()[0]

    @property
    def world_size(self) -> int:
        return comm.world()[1]


class ClipLoss(_LossBase):
    """``ClipLoss(local_loss, gather_with_grad, cache_labels, rank, world_size, use_horovod)``.
    ``local_loss=True``: each rank scores its B rows against the global batch ([B,G], loss.py:116-118);
    ``local_loss=False``: each rank forms the full [G,G] logits (loss.py:119-121) -- W times the work for the same
    optimisation objective, kept for parity with the constructor default.  ``gather_with_grad=False`` detaches the
    remote shards (loss.py:54-63)."""
    mode = "clip"

    def __init__(self, local_loss: bool = False, gather_with_grad: bool = False, cache_labels: bool = False,
                 rank: int = 0, world_size: int = 1, use_horovod: bool = False):
        super().__init__()
        self._init_common(local_loss, gather_with_grad, rank, world_size, use_horovod)
        self.cache_labels = cache_labels

    def forward(self, image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                logit_bias: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        loss = _ContrastiveFn.apply(image_features, text_features, logit_scale, logit_bias, self, {})
        return {"contrastive_loss": loss}


class SpatialLoss(_LossBase):
    """Multi-positive spatial-neighbour loss: soft labels from the tile-id join, STE-capped temperature,
    temperature regulariser (losses.py:16-42 ctor, :44-124 forward)."""
    mode = "spatial"

    def __init__(self, local_loss: bool = False, gather_with_grad: bool = False, rank: int = 0, world_size: int = 1,
                 use_horovod: bool = False, cap_logit_scale: Optional[float] = None, temp_reg_weight: float = 0.0,
                 float32_logits: bool = False, neighbor_alpha_scale: float = 1.0):
        super().__init__()
        self._init_common(local_loss, gather_with_grad, rank, world_size, use_horovod)
        self.cap_logit_scale = cap_logit_scale
        self.temp_reg_weight = temp_reg_weight
        self.float32_logits = float32_logits        # logits are always fp32 on this path
        self.neighbor_alpha_scale = neighbor_alpha_scale

    def forward(self, image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                image_tile_ids: torch.Tensor, text_tile_ids: torch.Tensor, neighbor_tile_ids: torch.Tensor,
                neighbor_alphas: torch.Tensor, logit_bias: Optional[torch.Tensor] = None,
                output_dict: bool = True) -> Dict[str, torch.Tensor]:
        kw = {"image_tile_ids": image_tile_ids, "text_tile_ids": text_tile_ids,
              "neighbor_tile_ids": neighbor_tile_ids, "neighbor_alphas": neighbor_alphas}
        loss = _ContrastiveFn.apply(image_features, text_features, logit_scale, logit_bias, self, kw)
        return {"contrastive_loss": loss}


class _SigLipFn(torch.autograd.Function):
    """Sigmoid loss forward AND its feature / scale / bias gradients (upstream gradient 1); backward scales them."""

    @staticmethod
    def forward(ctx, image_features, text_features, logit_scale, logit_bias, owner):
        rank, W = comm.world()
        dist_on = comm.is_dist()
        img = image_features.detach().contiguous().float()
        txt = text_features.detach().contiguous().float()
        B, D = img.shape
        all_t = None
        if dist_on:
            fg = owner.prefetched
            if fg is not None and fg.has("text", txt):
                all_t = fg.take("text")[0]       # launched from inside the net's forward, under the vision tower
            else:
                all_t = comm.gather_rows(txt)
        res = siglip_forward_backward(img, txt, logit_scale.detach(), logit_bias, all_text=all_t,
                                      rank=rank if dist_on else 0, recall_hits=owner.recall_hits,
                                      join_local=not dist_on)
        if dist_on:
            # autograd of the text exchange (neighbour_exchange_*_with_grad / all_gather): every rank's d all_text summed
            # onto the owner's rows -- the image features are never gathered, so they have only the direct term
            res["d_text"].copy_(comm.reduce_scatter_sum(res["d_all_text"]))
        ctx.flat = res["grads"]
        ctx.B, ctx.D = B, D
        owner.last = res
        return res["loss"]

    @staticmethod
    def backward(ctx, g):
        g = g.detach().reshape(1).float()
        flat = ctx.flat
        out = ops.scale_by_scalar(flat, g, torch.empty_like(flat)) if g.is_cuda else flat * g
        n = ctx.B * ctx.D
        d_b = out[2 * n + 1] if ctx.needs_input_grad[3] else None
        return out[:n].view(ctx.B, ctx.D), out[n:2 * n].view(ctx.B, ctx.D), out[2 * n], d_b, None


class SigLipLoss(_LossBase):
    """``SigLipLoss(cache_labels, rank, world_size, dist_impl)`` (open_clip, src/open_clip/loss.py:330-460): sigmoid
    loss of the local images against the global batch of texts, positives on the rank's own diagonal block.
    ``forward(image_features, text_features, logit_scale, logit_bias, output_dict=False)`` returns the 0-d loss, or
    ``{"contrastive_loss": loss}`` with ``output_dict=True``.

    Distributed: every ``dist_impl`` of the reference (bidir / shift neighbour exchange, reduce, gather) computes the
    same objective -- rank r scores its B images against all G texts, with gradients flowing back to the remote text
    features.  Here it is formed once for all four: one all-gather of the text features (launched under the vision
    tower; the image features are not gathered) and one [G, D] reduce-scatter of the remote text gradients.
    ``dist_impl`` therefore changes only the summation order relative to the reference.  Rank / world size are read
    from the live process group at call time, like the other losses here."""
    skip_gather = ("image",)

    def __init__(self, cache_labels: bool = False, rank: int = 0, world_size: int = 1,
                 dist_impl: Optional[str] = None):
        super().__init__()
        self._init_common(False, True, rank, world_size, False)
        self.cache_labels = cache_labels
        self.dist_impl = dist_impl or "bidir"
        assert self.dist_impl in ("bidir", "shift", "reduce", "gather")

    def forward(self, image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                logit_bias: Optional[torch.Tensor] = None, output_dict: bool = False):
        loss = _SigLipFn.apply(image_features, text_features, logit_scale, logit_bias, self)
        return {"contrastive_loss": loss} if output_dict else loss


class _DistillFn(torch.autograd.Function):
    """One node, two outputs (contrastive_loss, distill_loss).  Forward forms both losses and, per term, the feature / scale
    gradients for an upstream gradient of 1; backward is g_c * grads_c + g_d * grads_d -- exact for any pair of upstream
    gradients, which one pre-summed gradient buffer would not be.  The teacher's features and scale get no gradient."""

    @staticmethod
    def forward(ctx, image_features, text_features, logit_scale, dist_image_features, dist_text_features, dist_logit_scale,
                owner):
        rank, W = comm.world()
        dist_on = comm.is_dist()
        img = image_features.detach().contiguous().float()
        txt = text_features.detach().contiguous().float()
        t_img = dist_image_features.detach().contiguous().float()
        t_txt = dist_text_features.detach().contiguous().float()
        B, D = img.shape
        all_i = all_t = t_all_i = t_all_t = late = None
        fg = owner.prefetched
        if dist_on and fg is not None and fg.has("text", txt) and fg.has("image", img):
            all_t = fg.take("text")[0]
            late = lambda: fg.take("image")[0]
        elif dist_on:
            all_i, all_t = comm.gather_packed(img, txt, None, None)[:2]
        if dist_on:             # the teacher's features travel like the student's (no prefetch: its forward is already over)
            t_all_i, t_all_t = comm.gather_packed(t_img, t_txt, None, None)[:2]
        s, s_t = logit_scale.detach(), dist_logit_scale.detach()
        if dist_on and not owner.local_loss:
            # loss.py:119-121: every rank forms the full [G,G] logits of the global batch (labels arange(G))
            if late is not None:
                all_i = late()
            res = distill_forward_backward(all_i, all_t, s, t_all_i, t_all_t, s_t, rank=0, recall_hits=owner.recall_hits,
                                           recall_rows=(rank * B, B))
            terms = []
            for tag in ("c", "d"):      # the reduce-scatter operand does not depend on the upstream gradients per term only
                d_all = res["d_all_" + tag]
                tot = torch.cat([res["d_image_" + tag] + d_all[:, :D], res["d_text_" + tag] + d_all[:, D:]], dim=1)
                both = comm.reduce_scatter_sum(tot) if owner.gather_with_grad else tot[rank * B:(rank + 1) * B]
                terms.append((both[:, :D].contiguous(), both[:, D:].contiguous(), res["d_scale_" + tag]))
            ctx.flat = None
        else:
            res = distill_forward_backward(img, txt, s, t_img, t_txt, s_t, all_image=all_i, all_text=all_t,
                                           dist_all_image=t_all_i, dist_all_text=t_all_t, rank=rank if dist_on else 0,
                                           recall_hits=owner.recall_hits, late_all_image=late, join_local=not dist_on)
            terms = []
            for tag in ("c", "d"):
                d_i, d_t = res["d_image_" + tag], res["d_text_" + tag]
                if dist_on and owner.gather_with_grad:
                    # autograd of torch.distributed.nn.all_gather (loss.py:50-52), one reduce-scatter per term
                    both = comm.reduce_scatter_sum(res["d_all_" + tag])
                    d_i, d_t = d_i + both[:, :D], d_t + both[:, D:]
                terms.append((d_i, d_t, res["d_scale_" + tag]))
            flat = not (dist_on and owner.gather_with_grad)
            ctx.flat = (res["grads_c"], res["grads_d"]) if flat else None
        ctx.B, ctx.D = B, D
        ctx.save_for_backward(*terms[0], *terms[1])
        owner.last = res
        return res["contrastive_loss"], res["distill_loss"]

    @staticmethod
    def backward(ctx, g_c, g_d):
        g_c = g_c.detach().reshape(1).float()
        g_d = g_d.detach().reshape(1).float()
        if ctx.flat is not None and g_c.is_cuda:     # both terms are flat buffers: one launch forms g_c * grads_c + g_d * grads_d
            a, b = ctx.flat
            out = ops.axpby_scalars(a, g_c, b, g_d, torch.empty_like(a))
            n = ctx.B * ctx.D
            return out[:n].view(ctx.B, ctx.D), out[n:2 * n].view(ctx.B, ctx.D), out[2 * n], None, None, None, None
        i_c, t_c, s_c, i_d, t_d, s_d = ctx.saved_tensors
        return i_c * g_c + i_d * g_d, t_c * g_c + t_d * g_d, (s_c * g_c + s_d * g_d).reshape(()), None, None, None, None


class DistillClipLoss(ClipLoss):
    """``DistillClipLoss(local_loss, gather_with_grad, cache_labels, rank, world_size, use_horovod)`` (open_clip,
    src/open_clip/loss.py:203-239): ClipLoss on the student plus the cross-entropy of the student's softmax rows against a
    frozen teacher's, per direction.  ``forward(image_features, text_features, logit_scale, dist_image_features,
    dist_text_features, dist_logit_scale, output_dict=False)`` returns ``(contrastive_loss, distill_loss)`` or the dict of
    the two; the training loss is their sum.  The teacher's tensors are detached.  Layouts and gathers as in ClipLoss; the
    teacher's features are gathered with a second packed all-gather, and with ``gather_with_grad`` each term has its own
    reduce-scatter in forward (the operand is independent of the upstream gradient only per term)."""

    def forward(self, image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                dist_image_features: torch.Tensor, dist_text_features: torch.Tensor, dist_logit_scale: torch.Tensor,
                output_dict: bool = False):
        c, d = _DistillFn.apply(image_features, text_features, logit_scale, dist_image_features, dist_text_features,
                                dist_logit_scale, self)
        return {"contrastive_loss": c, "distill_loss": d} if output_dict else (c, d)
