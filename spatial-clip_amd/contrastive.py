"""Device-side contrastive head: similarity GEMMs -> sparse soft labels -> fused CE (+ temperature regulariser)
forward AND backward in one pass (the loss is always differentiated during training, so the gradients w.r.t. the
features are produced while the similarity matrix is still hot).

Reference semantics: open_clip ClipLoss (src/open_clip/loss.py:91-155, local_loss layout) and SpatialLoss
(src/models/components/losses.py:44-124).  Nothing here synchronises with the host.

The six matrix products (two similarity matrices, four gradient products) are exact-fp32 MFMA GEMMs
(``sc_sgemm_f32_grouped``): one launch for the forward pair, one for the backward four.

``siglip_forward_backward``: the sigmoid loss (open_clip SigLipLoss, src/open_clip/loss.py:330-460) on the same GEMMs --
one similarity matrix (image . all_text^T), one elementwise loss pass, two gradient products, only the text features
gathered.

``distill_forward_backward``: ClipLoss plus the distillation term against a frozen teacher (open_clip DistillClipLoss,
src/open_clip/loss.py:203-239) -- the student's and the teacher's similarity matrices in one grouped launch, one rows pass
(``sc_distill_loss``) that leaves the two gradient fields in their place, the gradient products once per field."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from . import ops


def _rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, D] with unit inner stride (the row stride may exceed D: gathered features sit in the packed
    receive buffer of the all-gather and are read in place)."""
    t = t.float()
    return t if t.stride(1) == 1 else t.contiguous()


def _sim_problems(f_i, f_t, a_t, a_i, z):
    """The two similarity products of one net: z[0] = image . all_text^T (needs only ``a_t``), z[1] = text . all_image^T."""
    B, D = f_i.shape
    G = a_t.shape[0]
    p_it = (f_i, f_i.stride(0), 1, a_t, a_t.stride(0), 1, z[0], G, B, G, D)
    if a_i is None:
        return [p_it]
    return [p_it, (f_t, f_t.stride(0), 1, a_i, a_i.stride(0), 1, z[1], G, B, G, D)]


def _grad_problems(dz, f_i, f_t, a_t, a_i, d_image, d_text, d_all=None):
    """Feature-gradient products of one dz[2][B][G]: the two direct terms (dz . gathered features -> d_image / d_text), then
    the two gathered-feature terms (dz^T . local features) -- written to ``d_all`` [G, 2D] = d_all_image | d_all_text, or,
    without it (single process, G == B), accumulated onto d_text / d_image (run those after the direct pair)."""
    B, D = f_i.shape
    G = a_t.shape[0]
    direct = [(dz[0], G, 1, a_t, 1, a_t.stride(0), d_image, D, B, D, G),     # dz_it . all_text        (K = G: first)
              (dz[1], G, 1, a_i, 1, a_i.stride(0), d_text, D, B, D, G)]      # dz_ti . all_image
    if d_all is None:
        return direct, [(dz[0], 1, G, f_i, 1, f_i.stride(0), d_text, D, G, D, B, 1),     # += dz_it^T . image = d all_text
                        (dz[1], 1, G, f_t, 1, f_t.stride(0), d_image, D, G, D, B, 1)]    # += dz_ti^T . text  = d all_image
    return direct, [(dz[0], 1, G, f_i, 1, f_i.stride(0), d_all[:, D:], 2 * D, G, D, B),   # dz_it^T . image  -> d all_text
                    (dz[1], 1, G, f_t, 1, f_t.stride(0), d_all[:, :D], 2 * D, G, D, B)]   # dz_ti^T . text   -> d all_image


def contrastive_forward_backward(
        image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor, *, mode: str = "clip",
        all_image: Optional[torch.Tensor] = None, all_text: Optional[torch.Tensor] = None, rank: int = 0,
        image_tile_ids: Optional[torch.Tensor] = None, text_tile_ids: Optional[torch.Tensor] = None,
        all_image_tile_ids: Optional[torch.Tensor] = None, all_text_tile_ids: Optional[torch.Tensor] = None,
        neighbor_tile_ids: Optional[torch.Tensor] = None, neighbor_alphas: Optional[torch.Tensor] = None,
        cap_logit_scale: Optional[float] = None, temp_reg_weight: float = 0.0, neighbor_alpha_scale: float = 1.0,
        logit_bias: Optional[torch.Tensor] = None, recall_hits: Optional[torch.Tensor] = None,
        recall_rows: Optional[tuple] = None,
        late_all_image: Optional[Callable[[], torch.Tensor]] = None, join_local: bool = False,
        want_recall: bool = True) -> Dict[str, torch.Tensor]:
    """Returns loss (0-d), d_image/d_text [B,D] (direct terms), d_all [G,2D] = d_all_image | d_all_text (this rank's
    contribution to EVERY rank's features = the operand of the reduce-scatter that is the autograd of
    torch.distributed.nn.all_gather, loss.py:50-52), d_scale, d_bias, recall_hits (R@1/5/10 hit counters).

    ``late_all_image``: callable returning ``all_image`` -- invoked only after the first similarity GEMM
    (image . all_text^T, which does not need it) has been enqueued, so a still-running all-gather of the image
    features overlaps with that GEMM.  ``recall_rows = (row0, n)``: the rows of z[0] whose diagonal block feeds R@k
    (default: all B rows, diagonal at column rank*B).  ``join_local`` (single process, G == B): the gathered-feature
    terms are accumulated straight onto the direct terms by the GEMMs (``d_image`` / ``d_text`` then hold the complete
    feature gradients and no ``d_all`` is formed).  ``want_recall=False`` skips the R@k counters.
    ``grads``: one flat fp32 buffer [2 B D + 2] = d_image | d_text | d_scale | d_bias (one launch scales all four in
    backward)."""
    f_i = _rows(image_features)
    f_t = _rows(text_features)
    a_t = f_t if all_text is None else _rows(all_text)
    dev = f_i.device
    B, D = f_i.shape
    G = a_t.shape[0]
    if f_t.shape != f_i.shape:
        raise ValueError("feature shapes disagree")
    if (rank + 1) * B > G:
        raise ValueError(f"rank {rank} with local batch {B} does not fit global batch {G}")
    scale = logit_scale.detach().reshape(1).float()
    z = torch.empty((2, B, G), dtype=torch.float32, device=dev)
    if late_all_image is not None:
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, None, z))
        a_i = _rows(late_all_image())
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, a_i, z)[1:])
    else:
        a_i = f_i if all_image is None else _rows(all_image)
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, a_i, z))
    if a_i.shape[0] != G:
        raise ValueError("gathered image / text batches disagree")

    if mode == "clip":
        nlab = 1
        lab_col = torch.empty((2, B, 1), dtype=torch.int32, device=dev)
        lab_w = torch.empty((2, B, 1), dtype=torch.float32, device=dev)
        ops.onehot_labels(B, rank, lab_col, lab_w)
        cap, w = 0.0, 0.0
    elif mode == "spatial":
        if neighbor_tile_ids is None or neighbor_alphas is None or image_tile_ids is None or text_tile_ids is None:
            raise ValueError("spatial mode needs tile ids, neighbor_tile_ids and neighbor_alphas")
        K = neighbor_tile_ids.shape[1]
        nlab = K + 1
        ids_i = image_tile_ids if all_image_tile_ids is None else all_image_tile_ids
        ids_t = text_tile_ids if all_text_tile_ids is None else all_text_tile_ids
        lab_col = torch.empty((2, B, nlab), dtype=torch.int32, device=dev)
        lab_w = torch.empty((2, B, nlab), dtype=torch.float32, device=dev)
        ops.neighbor_join(ids_i.contiguous(), ids_t.contiguous(), neighbor_tile_ids.contiguous(),
                          neighbor_alphas.contiguous().float(), B, G, K, rank, neighbor_alpha_scale, lab_col, lab_w)
        cap = float(cap_logit_scale) if cap_logit_scale is not None else 0.0
        w = float(temp_reg_weight)
    else:
        raise ValueError(f"unknown contrastive mode {mode!r}")

    bias = None if logit_bias is None else logit_bias.detach().reshape(1).float()
    rowstats = torch.empty((2 * B, 4), dtype=torch.float32, device=dev)
    loss_out = torch.empty(4, dtype=torch.float32, device=dev)
    ops.contrastive_loss_fwd(z, B, G, scale, cap, bias, lab_col, lab_w, nlab, w, rowstats, loss_out)
    if want_recall or recall_hits is not None:
        if recall_hits is None:
            recall_hits = torch.zeros(3, dtype=torch.int32, device=dev)
        if recall_rows is None:
            ops.recall_hits(z[0], G, B, rank * B, recall_hits)
        else:           # a window of a [G,G] matrix: rows row0.. whose diagonal sits at the same column offset
            row0, nrow = recall_rows
            ops.recall_hits(z[0][row0:], G, nrow, row0, recall_hits)
    rowgrad = torch.empty((2 * B, 2), dtype=torch.float32, device=dev)
    grads = torch.empty(2 * B * D + 2, dtype=torch.float32, device=dev)     # d_image | d_text | d_scale | d_bias
    d_image, d_text = grads[:B * D].view(B, D), grads[B * D:2 * B * D].view(B, D)
    d_scale = grads[2 * B * D:2 * B * D + 1]
    d_bias = grads[2 * B * D + 1:]
    ops.contrastive_loss_bwd(z, B, G, scale, cap, bias, lab_col, lab_w, nlab, w, rowstats, loss_out, None, rowgrad,
                             d_scale, d_bias)
    out = {"loss": loss_out[0], "gap": loss_out[1], "d_image": d_image, "d_text": d_text, "d_scale": d_scale[0],
           "d_bias": d_bias[0], "recall_hits": recall_hits, "grads": grads}
    if join_local:
        if G != B or rank != 0:
            raise ValueError("join_local: only for the single-process head (G == B)")
        direct, joined = _grad_problems(z, f_i, f_t, a_t, a_i, d_image, d_text)
        ops.sgemm_grouped(direct)
        ops.sgemm_grouped(joined)
        return out
    d_all = torch.empty((G, 2 * D), dtype=torch.float32, device=dev)       # d_all_image | d_all_text
    direct, gathered = _grad_problems(z, f_i, f_t, a_t, a_i, d_image, d_text, d_all)
    ops.sgemm_grouped(direct + gathered)
    out.update(d_all=d_all, d_all_image=d_all[:, :D], d_all_text=d_all[:, D:])
    return out


def siglip_forward_backward(
        image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
        logit_bias: Optional[torch.Tensor] = None, *, all_text: Optional[torch.Tensor] = None, rank: int = 0,
        recall_hits: Optional[torch.Tensor] = None, join_local: bool = False) -> Dict[str, torch.Tensor]:
    """Sigmoid loss of the local images against the (gathered) texts, forward AND backward for an upstream gradient of 1.

    Rank r scores its B images against all G texts; the positives are the diagonal of its own block (columns r*B..),
    every other pair is a negative -- the objective of every ``dist_impl`` of the reference.  ``logit_scale`` is the
    exponentiated scale; ``logit_bias`` may be None.  Returns loss (0-d), d_image [B,D] (complete), d_scale, d_bias (of
    the exponentiated scale / the bias), ``grads`` = one flat buffer [2 B D + 2] = d_image | d_text | d_scale | d_bias,
    and either (``join_local``, single process, G == B) d_text = dz^T . image written into ``grads``, or
    d_all_text [G,D] = this rank's contribution to every rank's text features (the reduce-scatter operand); d_text
    is then left for the caller to fill."""
    f_i = _rows(image_features)
    f_t = _rows(text_features)
    a_t = f_t if all_text is None else _rows(all_text)
    dev = f_i.device
    B, D = f_i.shape
    G = a_t.shape[0]
    if f_t.shape != f_i.shape or a_t.shape[1] != D:
        raise ValueError("feature shapes disagree")
    if (rank + 1) * B > G:
        raise ValueError(f"rank {rank} with local batch {B} does not fit global batch {G}")
    scale = logit_scale.detach().reshape(1).float()
    bias = None if logit_bias is None else logit_bias.detach().reshape(1).float()
    z = torch.empty((B, G), dtype=torch.float32, device=dev)
    ops.sgemm_grouped([(f_i, f_i.stride(0), 1, a_t, a_t.stride(0), 1, z, G, B, G, D)])     # z = image . all_text^T
    grads = torch.empty(2 * B * D + 2, dtype=torch.float32, device=dev)     # d_image | d_text | d_scale | d_bias
    d_image, d_text = grads[:B * D].view(B, D), grads[B * D:2 * B * D].view(B, D)
    d_scale, d_bias = grads[2 * B * D:2 * B * D + 1], grads[2 * B * D + 1:]
    rowpart = torch.empty((B, 3), dtype=torch.float32, device=dev)
    loss_out = torch.empty(1, dtype=torch.float32, device=dev)
    ops.siglip_loss(z, B, G, rank * B, scale, bias, rowpart, loss_out, d_scale, d_bias, recall_hits)   # z <- dz
    out = {"loss": loss_out[0], "d_image": d_image, "d_text": d_text, "d_scale": d_scale[0], "d_bias": d_bias[0],
           "recall_hits": recall_hits, "grads": grads}
    direct = (z, G, 1, a_t, 1, a_t.stride(0), d_image, D, B, D, G)              # dz . all_text   -> d image
    if join_local:
        if G != B or rank != 0:
            raise ValueError("join_local: only for the single-process head (G == B)")
        ops.sgemm_grouped([direct, (z, 1, G, f_i, 1, f_i.stride(0), d_text, D, G, D, B)])   # dz^T . image -> d text
        return out
    d_all_text = torch.empty((G, D), dtype=torch.float32, device=dev)
    ops.sgemm_grouped([direct, (z, 1, G, f_i, 1, f_i.stride(0), d_all_text, D, G, D, B)])  # dz^T . image -> d all_text
    out.update(d_all_text=d_all_text)
    return out


def distill_forward_backward(
        image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
        dist_image_features: torch.Tensor, dist_text_features: torch.Tensor, dist_logit_scale: torch.Tensor, *,
        all_image: Optional[torch.Tensor] = None, all_text: Optional[torch.Tensor] = None,
        dist_all_image: Optional[torch.Tensor] = None, dist_all_text: Optional[torch.Tensor] = None, rank: int = 0,
        recall_hits: Optional[torch.Tensor] = None, recall_rows: Optional[tuple] = None,
        late_all_image: Optional[Callable[[], torch.Tensor]] = None, join_local: bool = False) -> Dict[str, torch.Tensor]:
    """ClipLoss plus the distillation term against a frozen teacher (open_clip DistillClipLoss, src/open_clip/loss.py:203-239),
    forward AND backward of both terms for upstream gradients of 1.

    The student's [B, D] features and the teacher's [B, D_t] features (D_t may differ: only the teacher's similarity matrices
    are formed from them) give z_s, z_t [2, B, G]; one ``sc_distill_loss`` pass turns z_s into the CE gradient field and z_t
    into the distillation gradient field, and the gradient GEMMs of ``contrastive_forward_backward`` run once per field.
    Returns ``contrastive_loss`` / ``distill_loss`` (0-d), ``grads_c`` / ``grads_d``: flat fp32 [2 B D + 2] = d_image | d_text |
    d_scale | d_bias (bias slot zero; the scale is the exponentiated student scale; the teacher gets no gradient), their views
    ``d_image_c`` ... ``d_scale_d``, ``recall_hits``, and -- unless ``join_local`` (single process, G == B: the gathered-feature
    terms are accumulated onto the direct ones) -- ``d_all_c`` / ``d_all_d`` [G, 2D] = d_all_image | d_all_text, the reduce-scatter
    operands.  ``late_all_image`` / ``recall_rows``: as in ``contrastive_forward_backward``.  Nothing synchronises with the host."""
    f_i, f_t = _rows(image_features), _rows(text_features)
    t_i, t_t = _rows(dist_image_features.detach()), _rows(dist_text_features.detach())
    a_t = f_t if all_text is None else _rows(all_text)
    ta_t = t_t if dist_all_text is None else _rows(dist_all_text)
    ta_i = t_i if dist_all_image is None else _rows(dist_all_image)
    dev = f_i.device
    B, D = f_i.shape
    G = a_t.shape[0]
    if f_t.shape != f_i.shape or a_t.shape[1] != D:
        raise ValueError("feature shapes disagree")
    if t_i.shape != t_t.shape or t_i.shape[0] != B or ta_t.shape[1] != t_i.shape[1] or ta_i.shape[1] != t_i.shape[1]:
        raise ValueError("teacher feature shapes disagree")
    if ta_t.shape[0] != G or ta_i.shape[0] != G:
        raise ValueError("the teacher's gathered batch differs from the student's")
    if (rank + 1) * B > G:
        raise ValueError(f"rank {rank} with local batch {B} does not fit global batch {G}")
    scale = logit_scale.detach().reshape(1).float()
    tscale = dist_logit_scale.detach().reshape(1).float()
    z_s = torch.empty((2, B, G), dtype=torch.float32, device=dev)
    z_t = torch.empty((2, B, G), dtype=torch.float32, device=dev)
    teacher = _sim_problems(t_i, t_t, ta_t, ta_i, z_t)
    if late_all_image is not None:
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, None, z_s) + teacher)
        a_i = _rows(late_all_image())
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, a_i, z_s)[1:])
    else:
        a_i = f_i if all_image is None else _rows(all_image)
        ops.sgemm_grouped(_sim_problems(f_i, f_t, a_t, a_i, z_s) + teacher)
    if a_i.shape[0] != G or a_i.shape[1] != D:
        raise ValueError("gathered image / text batches disagree")

    rowpart = torch.empty((2 * B, 4), dtype=torch.float32, device=dev)
    loss_out = torch.empty(4, dtype=torch.float32, device=dev)
    n = B * D
    grads = torch.empty((2, 2 * n + 2), dtype=torch.float32, device=dev)   # per term: d_image | d_text | d_scale | d_bias
    grads_c, grads_d = grads[0], grads[1]
    hits_in_kernel = recall_hits is not None and recall_rows is None
    if recall_hits is not None and recall_rows is not None:   # a window of a [G,G] matrix (see contrastive_forward_backward)
        row0, nrow = recall_rows
        ops.recall_hits(z_s[0][row0:], G, nrow, row0, recall_hits)
    ops.distill_loss(z_s, z_t, B, G, rank * B, scale, tscale, rowpart, loss_out, grads_c[2 * n:2 * n + 1],
                     grads_d[2 * n:2 * n + 1], recall_hits if hits_in_kernel else None)        # z_s <- dz_c, z_t <- dz_d
    grads[:, 2 * n + 1].zero_()                                             # the bias slots (DistillClipLoss has no bias)
    out = {"contrastive_loss": loss_out[0], "distill_loss": loss_out[1], "ce_image": loss_out[2], "ce_text": loss_out[3],
           "grads_c": grads_c, "grads_d": grads_d, "recall_hits": recall_hits}
    views = {}
    for tag, g in (("c", grads_c), ("d", grads_d)):
        views[tag] = (g[:n].view(B, D), g[n:2 * n].view(B, D))
        out.update({f"d_image_{tag}": views[tag][0], f"d_text_{tag}": views[tag][1], f"d_scale_{tag}": g[2 * n]})
    if join_local:
        if G != B or rank != 0:
            raise ValueError("join_local: only for the single-process head (G == B)")
        dc, jc = _grad_problems(z_s, f_i, f_t, a_t, a_i, *views["c"])
        dd, jd = _grad_problems(z_t, f_i, f_t, a_t, a_i, *views["d"])
        ops.sgemm_grouped(dc + dd)
        ops.sgemm_grouped(jc + jd)
        return out
    d_all = torch.empty((2, G, 2 * D), dtype=torch.float32, device=dev)     # per term: d_all_image | d_all_text
    for k, (tag, dz) in enumerate((("c", z_s), ("d", z_t))):
        direct, gathered = _grad_problems(dz, f_i, f_t, a_t, a_i, *views[tag], d_all[k])
        ops.sgemm_grouped(direct + gathered)
    out.update(d_all_c=d_all[0], d_all_d=d_all[1])
    return out
