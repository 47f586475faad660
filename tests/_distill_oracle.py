"""Float64 restatement of the distillation loss (open_clip DistillClipLoss) with CLOSED-FORM gradients -- no autograd, so that
the formulae the kernel implements are pinned on their own (tests/test_cpu_distill.py holds them to the reference's goldens):

  x_s = s z_s, x_t = s_t z_t per direction (image->text: z = image . all_text^T; text->image: z = text . all_image^T)
  CE_i = lse(x_s,i) - x_s,i[diag]                      d CE_i / d x_s,ij = p_s,ij - onehot_ij        diag = col0 + i
  D_i  = lse(x_s,i) - sum_j p_t,ij x_s,ij              d D_i  / d x_s,ij = p_s,ij - p_t,ij           (teacher detached)
  contrastive = (mean_i CE^it + mean_i CE^ti) / 2,  distill = (mean_i D^it + mean_i D^ti) / 2.

``distill_terms`` works on B local rows against G gathered columns (G == B, rank 0 for one process) and returns, per term
("c" contrastive, "d" distill): the loss, the direct feature gradients d_image / d_text [B, D], this rank's contribution to
the gathered features d_all_image / d_all_text [G, D], and d_scale (of the exponentiated student scale)."""
import torch


def _f64(x):
    return torch.as_tensor(x).detach().to("cpu", torch.float64)


def distill_terms(image, text, scale, dist_image, dist_text, dist_scale, all_image=None, all_text=None,
                  dist_all_image=None, dist_all_text=None, rank=0):
    f_i, f_t, t_i, t_t = _f64(image), _f64(text), _f64(dist_image), _f64(dist_text)
    a_i = f_i if all_image is None else _f64(all_image)
    a_t = f_t if all_text is None else _f64(all_text)
    ta_i = t_i if dist_all_image is None else _f64(dist_all_image)
    ta_t = t_t if dist_all_text is None else _f64(dist_all_text)
    s, st = float(scale), float(dist_scale)
    B, G = f_i.shape[0], a_t.shape[0]
    onehot = torch.zeros(B, G, dtype=torch.float64)
    onehot[torch.arange(B), rank * B + torch.arange(B)] = 1.0
    out = {k: {"loss": 0.0, "d_scale": 0.0} for k in ("c", "d")}
    # (local rows, gathered columns, teacher rows, teacher columns, name of the local gradient, name of the gathered gradient)
    for rows, cols, trows, tcols, g_local, g_all in ((f_i, a_t, t_i, ta_t, "d_image", "d_all_text"),
                                                     (f_t, a_i, t_t, ta_i, "d_text", "d_all_image")):
        z = rows @ cols.T
        x = s * z
        lse = torch.logsumexp(x, dim=1, keepdim=True)
        p_s = torch.exp(x - lse)
        p_t = torch.softmax(st * (trows @ tcols.T), dim=1)
        per_row = {"c": (lse - x)[onehot.bool()], "d": (p_t * (lse - x)).sum(dim=1)}
        target = {"c": onehot, "d": p_t}
        for k in ("c", "d"):
            dx = (p_s - target[k]) * (0.5 / B)
            out[k]["loss"] = out[k]["loss"] + 0.5 * per_row[k].mean()
            out[k]["d_scale"] = out[k]["d_scale"] + (dx * z).sum()
            out[k][g_local] = s * dx @ cols
            out[k][g_all] = s * dx.T @ rows
    return out


def distill_single(image, text, scale, dist_image, dist_text, dist_scale):
    """One process (G == B): the complete feature gradients = direct + gathered terms.  Returns the golden files' keys."""
    o = distill_terms(image, text, scale, dist_image, dist_text, dist_scale)
    res = {"closs": o["c"]["loss"], "dloss": o["d"]["loss"]}
    for k in ("c", "d"):
        res["gimg_" + k] = o[k]["d_image"] + o[k]["d_all_image"]
        res["gtxt_" + k] = o[k]["d_text"] + o[k]["d_all_text"]
        res["gscale_" + k] = o[k]["d_scale"]
    return res


def distill_ranks(image, text, scale, dist_image, dist_text, dist_scale, world, local_loss):
    """``world`` ranks of B = G / world rows each with gather_with_grad=True: per rank the golden files' keys.  local_loss:
    rank r scores its rows against the global batch and receives every rank's gathered-feature terms for its rows; otherwise
    every rank forms the same [G, G] loss and the summed gradient of its rows is ``world`` times the single-process one."""
    G = image.shape[0]
    B = G // world
    res = []
    if not local_loss:
        full = distill_single(image, text, scale, dist_image, dist_text, dist_scale)
        for r in range(world):
            sl = slice(r * B, (r + 1) * B)
            one = {"closs": full["closs"], "dloss": full["dloss"]}
            for k in ("c", "d"):
                one["gimg_" + k] = world * full["gimg_" + k][sl]
                one["gtxt_" + k] = world * full["gtxt_" + k][sl]
                one["gscale_" + k] = full["gscale_" + k]
            res.append(one)
        return res
    per = [distill_terms(image[r * B:(r + 1) * B], text[r * B:(r + 1) * B], scale, dist_image[r * B:(r + 1) * B],
                         dist_text[r * B:(r + 1) * B], dist_scale, image, text, dist_image, dist_text, rank=r)
           for r in range(world)]
    for r in range(world):
        sl = slice(r * B, (r + 1) * B)
        one = {"closs": per[r]["c"]["loss"], "dloss": per[r]["d"]["loss"]}
        for k in ("c", "d"):
            one["gimg_" + k] = per[r][k]["d_image"] + sum(p[k]["d_all_image"][sl] for p in per)
            one["gtxt_" + k] = per[r][k]["d_text"] + sum(p[k]["d_all_text"][sl] for p in per)
            one["gscale_" + k] = per[r][k]["d_scale"]
        res.append(one)
    return res
