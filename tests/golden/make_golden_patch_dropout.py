#!/usr/bin/env python3
"""Golden vectors of FLIP patch dropout from the REFERENCE's own vision tower (imported, never copied; recipe and caveats:
make_golden.py).  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_patch_dropout.py

The reference's tiny CLIP with ``vision_cfg.patch_dropout = 0.5`` runs ``encode_image`` in train mode on the CPU in fp32.  The
indices its PatchDropout draws (``torch.randn(B, n).topk(K)`` under a fixed seed) are recomputed beside it and verified
against what the module actually let through.  Recorded: images, the vision weights, the drawn indices (topk order), the
normalised features, the target of the fixed scalar loss ``sum(normalize(features) * target)`` and the gradient of every vision
parameter -> tests/golden/patch_dropout_tiny.npz."""
import sys

sys.dont_write_bytecode = True
import os

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, npz  # noqa: E402

CFG = {"embed_dim": 32,
       "vision_cfg": {"image_size": 32, "layers": 2, "width": 64, "patch_size": 8, "head_width": 32, "mlp_ratio": 2.0,
                      "patch_dropout": 0.5},
       "text_cfg": {"context_length": 16, "vocab_size": 97, "width": 64, "heads": 2, "layers": 1}}
B, DRAW_SEED = 6, 1234


def main():
    torch.set_num_threads(8)
    model, _, _ = import_reference()
    torch.manual_seed(21)
    clip = model.CLIP(**CFG)
    for n, p_ in clip.named_parameters():
        if p_.ndim == 1 and "logit" not in n:
            p_.data.add_(0.05 * torch.randn_like(p_))
    clip.train()
    g = torch.Generator().manual_seed(22)
    images = torch.randn(B, 3, 32, 32, generator=g)
    target = torch.randn(B, CFG["embed_dim"], generator=g)
    n_patch = (32 // 8) ** 2
    K = max(1, int(n_patch * 0.5))
    torch.manual_seed(DRAW_SEED)
    drawn = torch.randn(B, n_patch).topk(K, dim=-1).indices          # what PatchDropout.forward will draw next
    seen = {}
    hook = clip.visual.patch_dropout.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach(), y=o.detach()))
    torch.manual_seed(DRAW_SEED)
    feats = F.normalize(clip.encode_image(images), dim=-1)
    hook.remove()
    want = seen["x"][:, 1:][torch.arange(B)[:, None], drawn]
    assert seen["y"].shape[1] == K + 1 and torch.equal(seen["y"][:, 1:], want), "the recomputed indices are not the module's"
    loss = (feats * target).sum()
    loss.backward()
    arrs = {"images": images, "target": target, "keep_topk_order": drawn.to(torch.int32), "features": feats, "loss": loss}
    for k, v in clip.visual.state_dict().items():
        arrs["w.visual." + k] = v
    for k, p_ in clip.visual.named_parameters():
        arrs["g.visual." + k] = p_.grad if p_.grad is not None else torch.zeros_like(p_)
    npz("patch_dropout_tiny.npz", **arrs)


if __name__ == "__main__":
    main()
