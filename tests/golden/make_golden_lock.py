#!/usr/bin/env python3
"""Golden vectors for locked towers (LiT): the REFERENCE's tiny CLIP with ``lock_image_tower`` / ``lock_text_tower`` applied,
trained for three steps by the train3 recipe of make_golden.py (same batch, SpatialLoss arguments, AdamW lr 1e-3, betas
(0.9, 0.98), eps 1e-6, weight_decay 0.1, clip 1.0, warm-up 2 of 10 steps).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lock.py

Three variants, one ``train3_tiny_text_lock_<variant>.npz`` each:

    img0        lock_image_tower(0)
    img2        lock_image_tower(2)
    img0_txt1   lock_image_tower(0) + lock_text_tower(1)

Each holds the three losses, the three pre-clip gradient norms, ``trainable`` (JSON list of the names with requires_grad),
``p3.<name>`` for the TRAINABLE tensors -- the script asserts that every locked tensor of the reference is bit-identical to its
``p0`` after the three steps, so the test checks those against ``p0`` and no copy is stored -- and the step-0 gradients of the
trainable tensors before clipping.  To stay under the 1 MiB limit for a committed file the gradients are stored as
``g0.<name>`` = float16 of ``g / g0s.<name>`` with ``g0s.<name>`` = max|g| (fp32 scalar): the rounding is at most 2^-11 of the
tensor's max-abs, which the test takes OFF its 4 % bound.  ``ac_rel`` (JSON) is the yardstick of that bound: per trainable
tensor, max|g_autocast - g_fp32| / max|g_fp32| of the same step under ``torch.autocast("cpu", dtype=torch.bfloat16)``.

The starting weights are the ``p0.*`` of ``train3_tiny_text.npz`` and are not stored again; ``p0_sha256``
(make_golden_accum.p0_digest) pins them.

``lock_groups_manifest.json``: for the same tiny CLIP, the reference's list of ``requires_grad`` names after
``lock_image_tower(g)`` for g = 0 .. layers + 3 (key ``image``) and after ``lock_text_tower(k)`` for k = 0 .. layers + 3 (key
``text``), each applied alone to a fresh model.  Only data is written; no reference source is copied."""
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

VARIANTS = {"img0": ((0,), None), "img2": ((2,), None), "img0_txt1": ((0,), (1,))}


def apply_lock(clip, image, text):
    if image is not None:
        clip.lock_image_tower(*image)
    if text is not None:
        clip.lock_text_tower(*text)


def train(model, ref_losses, tiny, p0, z, image, text, autocast):
    clip = model.CLIP(**tiny)
    clip.load_state_dict(p0)
    apply_lock(clip, image, text)
    trainable = [n for n, p in clip.named_parameters() if p.requires_grad]
    opt = torch.optim.AdamW(clip.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, MA.lam)
    crit = ref_losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                  neighbor_alpha_scale=0.5, float32_logits=True)
    images, texts = torch.from_numpy(z["images"]), torch.from_numpy(z["texts"])
    ids, nb, al = torch.from_numpy(z["ids"]), torch.from_numpy(z["nb"]), torch.from_numpy(z["alpha"])
    losses, norms, g0 = [], [], {}
    for step in range(3):
        opt.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f_i = clip.encode_image(images, normalize=True)
            f_t = clip.encode_text(texts, normalize=True)
            l = crit(f_i, f_t, clip.logit_scale.exp(), ids, ids.clone(), nb, al)["contrastive_loss"]
        l.backward()
        if step == 0:
            named = dict(clip.named_parameters())
            assert all(named[n].grad is None for n in named if n not in trainable)
            g0 = {n: named[n].grad.detach().clone().float() for n in trainable}
        norms.append(float(torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)))
        opt.step()
        sched.step()
        losses.append(float(l.detach()))
    return losses, norms, g0, trainable, {k: v.detach().clone() for k, v in clip.state_dict().items()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, _, ref_losses = MG.import_reference()
    z = np.load(os.path.join(HERE, "train3_tiny_text.npz"), allow_pickle=False)
    tiny = json.loads(str(z["cfg"]))
    assert int(z["warmup"]) == MA.WARM and int(z["total"]) == MA.TOTAL
    p0 = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0.")}
    for tag, (image, text) in VARIANTS.items():
        losses, norms, g0, trainable, p3 = train(model, ref_losses, tiny, p0, z, image, text, autocast=False)
        _, _, ac_g0, _, _ = train(model, ref_losses, tiny, p0, z, image, text, autocast=True)
        for k, v in p3.items():
            if k not in trainable:
                assert torch.equal(v, p0[k]), f"{tag}: locked tensor {k} moved in the reference"
            else:
                assert not torch.equal(v, p0[k]) or v.numel() == 0, f"{tag}: trainable tensor {k} did not move"
        arrs = {"cfg": json.dumps(tiny), "warmup": MA.WARM, "total": MA.TOTAL, "p0_from": "train3_tiny_text.npz",
                "p0_sha256": MA.p0_digest(z), "trainable": json.dumps(trainable),
                "losses": np.array(losses), "grad_norms": np.array(norms),
                "ac_rel": json.dumps({k: float((ac_g0[k] - g0[k]).abs().max() / g0[k].abs().max().clamp_min(1e-30))
                                      for k in trainable})}
        for k in trainable:
            arrs["p3." + k] = p3[k]
            scale = float(g0[k].abs().max())
            arrs["g0s." + k] = np.float32(scale)
            arrs["g0." + k] = (g0[k] / max(scale, 1e-30)).numpy().astype(np.float16)
        name = f"train3_tiny_text_lock_{tag}.npz"
        MG.npz(name, **arrs)
        size = os.path.getsize(os.path.join(HERE, name))
        print(tag, "losses", losses, "norms", norms, "trainable", len(trainable), "bytes", size)
        assert size < 1024 * 1024, f"{name}: {size} bytes is past the limit for a committed file"
    layers_v, layers_t = tiny["vision_cfg"]["layers"], tiny["text_cfg"]["layers"]
    manifest = {"cfg": tiny, "image": {}, "text": {}}
    for g in range(layers_v + 4):
        clip = model.CLIP(**tiny)
        clip.lock_image_tower(g)
        manifest["image"][str(g)] = [n for n, p in clip.named_parameters() if p.requires_grad]
    for k in range(layers_t + 4):
        clip = model.CLIP(**tiny)
        clip.lock_text_tower(k)
        manifest["text"][str(k)] = [n for n, p in clip.named_parameters() if p.requires_grad]
    with open(os.path.join(HERE, "lock_groups_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("manifest", {t: {k: len(v) for k, v in manifest[t].items()} for t in ("image", "text")})


if __name__ == "__main__":
    main()
