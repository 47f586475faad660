#!/usr/bin/env python3
"""Golden vectors for gradient accumulation (Trainer accumulate_grad_batches = 2): the REFERENCE's tiny CLIP trained over
five distinct micro-batches, three optimiser steps, the third from a group of one whose loss is still divided by 2.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_accum.py

``lightning`` is not installed where this runs, so the loop below is the plain PyTorch loop that Lightning's automatic
optimisation performs with ``accumulate_grad_batches=N``: ``(loss / N).backward()`` for every batch; after batch i with
``(i + 1) % N == 0``, and after the epoch's last batch, ``clip_grad_norm_`` -> ``optimizer.step()`` -> ``scheduler.step()``
-> ``zero_grad()``.  Model, loss and optimiser are the reference's own classes (``make_golden.import_reference``) with the
SpatialLoss / AdamW settings, warm-up 2 of 10 steps and clip 1.0 of the train3 section of make_golden.py.

Writes ``train_accum2_tiny_text.npz``: the five batches, the five micro-batch losses, the three pre-clip gradient norms and
the final values of the four parameters the test bounds -- once in fp32 (the expected values) and once under
``torch.autocast("cpu", dtype=torch.bfloat16)``, the reference's own bf16-mixed policy (the yardstick for the bounds).  The
starting weights are the ``p0.*`` of ``train3_tiny_text.npz`` and are NOT stored again: a copy of them beside the five batches
would take this file past 1 MiB.  Their SHA-256 (``p0_digest``: names and bytes in name order) is stored as ``p0_sha256`` and
the test asserts it, so regenerating train3_tiny_text.npz with other weights fails loudly instead of shifting the expected
values.  Only .npz data is written; no reference source is copied."""
import sys

sys.dont_write_bytecode = True
import hashlib
import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N, MICRO, B = 2, 5, 6
WARM, TOTAL = 2, 10
BOUNDED = ("visual.proj", "text_projection", "token_embedding.weight", "visual.conv1.weight")
SEED = 90      # of the seeds tried (40 .. 110 by tens) the one whose N = 1 run lands furthest outside the bounds


def p0_digest(z):
    """SHA-256 over the ``p0.*`` entries of an opened train3_tiny_text.npz: each name, then its array's bytes, in name order."""
    h = hashlib.sha256()
    for k in sorted(k for k in z.files if k.startswith("p0.")):
        h.update(k.encode())
        h.update(np.ascontiguousarray(z[k]).tobytes())
    return h.hexdigest()


def make_batches():
    out = []
    for i in range(MICRO):
        g = torch.Generator().manual_seed(SEED + i)
        images = torch.randn(B, 3, 32, 32, generator=g)
        texts = torch.zeros(B, 16, dtype=torch.long)
        for b in range(B):
            n = int(torch.randint(3, 14, (1,), generator=g))
            texts[b, 0] = 95
            texts[b, 1:1 + n] = torch.randint(1, 95, (n,), generator=g)
            texts[b, 1 + n] = 96      # EOT = max id
        ids, nb, al = MG.make_batch_ids(B, 4, g)
        out.append({"images": images, "texts": texts, "ids": ids, "nb": nb, "alpha": al})
    return out


def lam(step):
    if step < WARM:
        return step / max(1, WARM)
    pr = (step - WARM) / max(1, TOTAL - WARM)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * pr)))


def train(model, ref_losses, tiny, p0, batches, every, autocast):
    clip = model.CLIP(**tiny)
    clip.load_state_dict(p0)
    opt = torch.optim.AdamW(clip.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    crit = ref_losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                  neighbor_alpha_scale=0.5, float32_logits=True)
    losses, norms = [], []
    opt.zero_grad()
    for i, b in enumerate(batches):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f_i = clip.encode_image(b["images"], normalize=True)
            f_t = clip.encode_text(b["texts"], normalize=True)
            l = crit(f_i, f_t, clip.logit_scale.exp(), b["ids"], b["ids"].clone(), b["nb"], b["alpha"])["contrastive_loss"]
        (l / every).backward()
        losses.append(float(l.detach()))
        if (i + 1) % every == 0 or i == len(batches) - 1:
            norms.append(float(torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)))
            opt.step()
            sched.step()
            opt.zero_grad()
    return losses, norms, {k: v.detach().clone() for k, v in clip.state_dict().items()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, _, ref_losses = MG.import_reference()
    z = np.load(os.path.join(HERE, "train3_tiny_text.npz"), allow_pickle=False)
    tiny = json.loads(str(z["cfg"]))
    p0 = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0.")}
    batches = make_batches()
    losses, norms, pN = train(model, ref_losses, tiny, p0, batches, N, autocast=False)
    ac_losses, ac_norms, ac_pN = train(model, ref_losses, tiny, p0, batches, N, autocast=True)
    assert len(losses) == MICRO and len(norms) == 3
    # the fixture must tell the feature from its absence: five plain steps (N = 1) leave at least one bounded tensor outside
    # the bound the test grants the accumulated run
    _, _, p1 = train(model, ref_losses, tiny, p0, batches, 1, autocast=False)
    miss = {}
    for k in BOUNDED:
        bound = max(3e-3, 1.5 * float((ac_pN[k] - pN[k]).abs().max()))
        miss[k] = (float((p1[k] - pN[k]).abs().max()), bound)
    print("N = 1 deviation vs bound:", miss)
    # (by a fifth at least: the HIP run this is asserted on carries bf16 noise)
    assert any(d > 1.2 * b for d, b in miss.values()), "choose other seeds: N = 1 stays too close to the parameter bounds"
    arrs = {"cfg": json.dumps(tiny), "warmup": WARM, "total": TOTAL, "every": N, "p0_from": "train3_tiny_text.npz",
            "p0_sha256": p0_digest(z),
            "losses": np.array(losses), "grad_norms": np.array(norms),
            "autocast_losses": np.array(ac_losses), "autocast_grad_norms": np.array(ac_norms)}
    for i, b in enumerate(batches):
        for k, v in b.items():
            arrs[f"b{i}.{k}"] = v
    for k in BOUNDED:
        arrs["pN." + k] = pN[k]
        arrs["autocast_pN." + k] = ac_pN[k]
    MG.npz("train_accum2_tiny_text.npz", **arrs)
    print("losses", losses, "\nautocast", ac_losses, "\nnorms", norms, "\nautocast", ac_norms)
    print("bytes", os.path.getsize(os.path.join(HERE, "train_accum2_tiny_text.npz")))


if __name__ == "__main__":
    main()
