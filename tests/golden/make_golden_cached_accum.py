#!/usr/bin/env python3
"""Golden vectors for cached-feature gradient accumulation (Trainer accum_freq = 2; open_clip's ``--accum-freq``): the
REFERENCE's tiny CLIP with text tower trained on the first four micro-batches of 6 of make_golden_accum.py as two batches of
G = 12, two optimiser steps.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cached_accum.py

Model and losses are the reference's own classes (``make_golden.import_reference``); AdamW, the warm-up 2 of 10 cosine
schedule and clip 1.0 are make_golden_accum.py's.  Writes ``cached_accum_tiny_text.npz`` (data only; the starting weights are
the ``p0.*`` of ``train3_tiny_text.npz``, referred to by SHA-256 as make_golden_accum.py does):

(a) the G-batch run with open_clip's ClipLoss in fp32: per step the loss, the pre-clip gradient norm and the post-step values
    of the four tensors test_gpu_grad_accum.py bounds, the step-0 gradients of those tensors and of ``logit_scale``; and the
    same run under ``torch.autocast("cpu", dtype=torch.bfloat16)``, the yardstick of the bounds.
(b) open_clip's accumulation loop (open_clip_train/train.py:151-192: cache the features without grad, then per micro-batch a
    forward with grad, the loss of the whole batch with that micro-batch's features spliced in, backward) written out in plain
    PyTorch on group 0.  ASSERTED here: every gradient but ``logit_scale``'s equals (a)'s to fp32 rounding, and
    ``logit_scale``'s is N times (a)'s -- the loop backpropagates the full-batch loss N times, and the scale takes part in
    every one of them.  Both scalars are stored (``g0.logit_scale``, ``g0_loop.logit_scale``).
(c) the distance between (a) and Lightning's ``accumulate_grad_batches=2`` (make_golden_accum.py's loop: ``(loss / N)
    .backward()`` per micro-batch of 6) with the same ClipLoss on the same four micro-batches, per checked quantity, against
    twice the bound the GPU test grants that quantity (``max(constant, 1.5 x autocast distance)``).  ASSERTED for the two
    losses and the two gradient norms.  For the four post-step parameter tensors the figures are printed and stored
    (``sep.*`` = distance, bound) but cannot be asserted: the schedule these runs share gives step 0 a learning rate of 0
    and step 1 one of 5e-4, and AdamW moves no element by more than its learning rate per step, so after two steps two runs
    from the same weights are at most ~1e-3 apart, below twice the 3e-3 floor of the bound, whatever the data.  The losses
    and gradient norms are what tell the G-pair objective from two 6-pair ones.
(d) a SpatialLoss variant on group 0 (reference SpatialLoss, cap_logit_scale 40, temp_reg_weight 0.05, neighbor_alpha_scale
    0.5): tile ids unique over the 12 rows, K = 3; every row names one neighbour that sits in the OTHER micro-batch, one in
    its own and one in neither; one alpha <= 0.  Stores the G-batch loss, the step-0 gradients of ``visual.proj``,
    ``text_projection`` and ``logit_scale``, the autocast run of the same, and the two per-micro-batch losses.  ASSERTED: the
    group loss differs from the mean of the two micro-batch losses by more than twice the loss bound."""
import sys

sys.dont_write_bytecode = True
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_accum as MA  # noqa: E402

N, MICRO, B = 2, 4, 6
G = N * B
STEPS = MICRO // N
BOUNDED = MA.BOUNDED
SPATIAL_GRADS = ("visual.proj", "text_projection", "logit_scale")
K = 3


def group_batch(batches, s):
    """Group s: its N micro-batches as one batch of G."""
    mem = batches[s * N:(s + 1) * N]
    return torch.cat([b["images"] for b in mem]), torch.cat([b["texts"] for b in mem])


def features(clip, images, texts):
    return clip.encode_image(images, normalize=True), clip.encode_text(texts, normalize=True)


def new_run(model, tiny, p0):
    clip = model.CLIP(**tiny)
    clip.load_state_dict(p0)
    opt = torch.optim.AdamW(clip.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, MA.lam)
    return clip, opt, sched


def grads_of(clip):
    return {k: p.grad.detach().clone() for k, p in clip.named_parameters()}


def train_groups(model, crit, tiny, p0, batches, autocast):
    """(a): one loss over G = N * B pairs per optimiser step."""
    clip, opt, sched = new_run(model, tiny, p0)
    losses, norms, post, g0 = [], [], [], None
    for s in range(STEPS):
        images, texts = group_batch(batches, s)
        opt.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f_i, f_t = features(clip, images, texts)
            l = crit(f_i, f_t, clip.logit_scale.exp(), output_dict=True)["contrastive_loss"]
        l.backward()
        if s == 0:
            g0 = grads_of(clip)
        losses.append(float(l.detach()))
        norms.append(float(torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)))
        opt.step()
        sched.step()
        post.append({k: clip.state_dict()[k].detach().clone() for k in BOUNDED})
    return losses, norms, post, g0


def open_clip_loop_grads(model, crit, tiny, p0, batches):
    """(b): the gradient open_clip's --accum-freq loop leaves in front of the optimiser for group 0."""
    clip, opt, _ = new_run(model, tiny, p0)
    mem = batches[:N]
    acc_i, acc_t = [], []
    with torch.no_grad():
        for b in mem:
            f_i, f_t = features(clip, b["images"], b["texts"])
            acc_i.append(f_i)
            acc_t.append(f_t)
    opt.zero_grad()
    for j, b in enumerate(mem):
        f_i, f_t = features(clip, b["images"], b["texts"])
        in_i = torch.cat(acc_i[:j] + [f_i] + acc_i[j + 1:])
        in_t = torch.cat(acc_t[:j] + [f_t] + acc_t[j + 1:])
        crit(in_i, in_t, clip.logit_scale.exp(), output_dict=True)["contrastive_loss"].backward()
    return grads_of(clip)


def train_lightning(model, crit, tiny, p0, batches):
    """(c): make_golden_accum.train's loop (Lightning's accumulate_grad_batches = N) with the ClipLoss of (a)."""
    clip, opt, sched = new_run(model, tiny, p0)
    losses, norms, post = [], [], []
    opt.zero_grad()
    for i, b in enumerate(batches):
        f_i, f_t = features(clip, b["images"], b["texts"])
        l = crit(f_i, f_t, clip.logit_scale.exp(), output_dict=True)["contrastive_loss"]
        (l / N).backward()
        losses.append(float(l.detach()))
        if (i + 1) % N == 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)))
            opt.step()
            sched.step()
            opt.zero_grad()
            post.append({k: clip.state_dict()[k].detach().clone() for k in BOUNDED})
    return losses, norms, post


def spatial_inputs(gen):
    ids = 10_000 + torch.arange(G)
    nb = torch.empty((G, K), dtype=torch.long)
    for r in range(G):
        m, q = divmod(r, B)
        nb[r, 0] = ids[(r + B) % G]                 # in the other micro-batch
        nb[r, 1] = ids[m * B + (q + 1) % B]         # in its own
        nb[r, 2] = 99_000_000 + r                   # in neither
    al = torch.rand((G, K), generator=gen) + 0.1
    al = al / al.sum(dim=1, keepdim=True)
    al[4, 1] = -0.3                                 # alpha <= 0 is skipped
    return ids, nb, al


def spatial_run(model, ref_losses, tiny, p0, images, texts, ids, nb, al, autocast):
    clip, opt, _ = new_run(model, tiny, p0)
    crit = ref_losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                  neighbor_alpha_scale=0.5, float32_logits=True)
    opt.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        f_i, f_t = features(clip, images, texts)
        l = crit(f_i, f_t, clip.logit_scale.exp(), ids, ids.clone(), nb, al)["contrastive_loss"]
    l.backward()
    g = grads_of(clip)
    return float(l.detach()), {k: g[k] for k in SPATIAL_GRADS}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, oc_loss, ref_losses = MG.import_reference()
    z = np.load(os.path.join(HERE, "train3_tiny_text.npz"), allow_pickle=False)
    tiny = json.loads(str(z["cfg"]))
    p0 = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0.")}
    batches = MA.make_batches()[:MICRO]
    crit = oc_loss.ClipLoss()

    # ---- (a)
    losses, norms, post, g0 = train_groups(model, crit, tiny, p0, batches, autocast=False)
    ac_losses, ac_norms, ac_post, ac_g0 = train_groups(model, crit, tiny, p0, batches, autocast=True)

    # ---- (b)
    loop = open_clip_loop_grads(model, crit, tiny, p0, batches)
    worst = 0.0
    for k, g in g0.items():
        if k == "logit_scale":
            continue
        rel = float((loop[k] - g).abs().max()) / max(float(g.abs().max()), 1e-12)
        worst = max(worst, rel)
        assert rel <= 2e-5, (k, rel)
    s_a, s_loop = float(g0["logit_scale"]), float(loop["logit_scale"])
    assert abs(s_loop - N * s_a) <= 2e-5 * abs(N * s_a), (s_a, s_loop)
    print(f"(b) open_clip loop: worst relative gradient difference {worst:.3g}; logit_scale gradient {s_loop:.8g} = "
          f"{s_loop / s_a:.6f} x {s_a:.8g}")

    # ---- (c)
    l_losses, l_norms, l_post = train_lightning(model, crit, tiny, p0, batches)
    sep = {}
    for s in range(STEPS):
        mean_micro = sum(l_losses[s * N:(s + 1) * N]) / N       # what Lightning's run logs for the group, averaged
        bound = max(4e-3 if s == 0 else 2e-2, 1.5 * abs(ac_losses[s] - losses[s]))
        sep[f"loss{s}"] = (abs(mean_micro - losses[s]), bound)
        bound = max(0.05, 1.5 * abs(ac_norms[s] - norms[s]) / norms[s])
        sep[f"grad_norm{s}"] = (abs(l_norms[s] - norms[s]) / norms[s], bound)
    for k in BOUNDED:
        bound = max(3e-3, 1.5 * float((ac_post[-1][k] - post[-1][k]).abs().max()))
        sep["p." + k] = (float((l_post[-1][k] - post[-1][k]).abs().max()), bound)
    print("(c) distance to accumulate_grad_batches=2 vs bound:", {k: (f"{d:.3g}", f"{b:.3g}") for k, (d, b) in sep.items()})
    for k, (d, b) in sep.items():
        if not k.startswith("p."):
            assert d >= 2.0 * b, f"{k}: the Lightning form is only {d:.3g} away, the bound is {b:.3g}: choose other data"

    # ---- (d)
    gen = torch.Generator().manual_seed(MA.SEED + 1000)
    ids, nb, al = spatial_inputs(gen)
    images, texts = group_batch(batches, 0)
    sp_loss, sp_g = spatial_run(model, ref_losses, tiny, p0, images, texts, ids, nb, al, autocast=False)
    sp_ac_loss, sp_ac_g = spatial_run(model, ref_losses, tiny, p0, images, texts, ids, nb, al, autocast=True)
    micro = []
    for m in range(N):
        r = slice(m * B, (m + 1) * B)
        micro.append(spatial_run(model, ref_losses, tiny, p0, images[r], texts[r], ids[r], nb[r], al[r], autocast=False)[0])
    sp_bound = max(4e-3, 1.5 * abs(sp_ac_loss - sp_loss))
    print(f"(d) spatial group loss {sp_loss:.6f} (autocast {sp_ac_loss:.6f}), micro-batch losses {micro}, bound {sp_bound:.3g}")
    assert abs(sp_loss - sum(micro) / N) >= 2.0 * sp_bound, "the spatial group loss is too close to the micro-batch mean"

    arrs = {"cfg": json.dumps(tiny), "warmup": MA.WARM, "total": MA.TOTAL, "accum_freq": N, "micro_batch": B,
            "batches_from": "train_accum2_tiny_text.npz", "p0_from": "train3_tiny_text.npz", "p0_sha256": MA.p0_digest(z),
            "losses": np.array(losses), "grad_norms": np.array(norms), "autocast_losses": np.array(ac_losses),
            "autocast_grad_norms": np.array(ac_norms), "g0_loop.logit_scale": np.array(s_loop),
            "lightning_losses": np.array(l_losses), "lightning_grad_norms": np.array(l_norms),
            "sp.ids": ids, "sp.nb": nb, "sp.alpha": al, "sp.loss": np.array(sp_loss), "sp.autocast_loss": np.array(sp_ac_loss),
            "sp.micro_losses": np.array(micro)}
    for k, (d, b) in sep.items():
        arrs["sep." + k] = np.array([d, b])
    for k in BOUNDED + ("logit_scale",):
        arrs["g0." + k] = g0[k]
        arrs["autocast_g0." + k] = ac_g0[k]
    for s in range(STEPS):
        for k in BOUNDED:
            arrs[f"p{s}." + k] = post[s][k]
            arrs[f"autocast_p{s}." + k] = ac_post[s][k]
    for k in SPATIAL_GRADS:
        arrs["sp.g0." + k] = sp_g[k]
        arrs["sp.autocast_g0." + k] = sp_ac_g[k]
    # the four micro-batches are those of train_accum2_tiny_text.npz (b0 .. b3): not stored again, checked by value here
    acc = np.load(os.path.join(HERE, "train_accum2_tiny_text.npz"), allow_pickle=False)
    for i, b in enumerate(batches):
        assert np.array_equal(acc[f"b{i}.images"], b["images"].numpy()) and np.array_equal(acc[f"b{i}.texts"], b["texts"].numpy())
    MG.npz("cached_accum_tiny_text.npz", **arrs)
    print("losses", losses, "\nautocast", ac_losses, "\nnorms", norms, "\nautocast", ac_norms)
    print("bytes", os.path.getsize(os.path.join(HERE, "cached_accum_tiny_text.npz")))


if __name__ == "__main__":
    main()
