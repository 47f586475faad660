#!/usr/bin/env python3
"""The default vision tower's bits on a fixed seed and batch -> tests/golden/pool_default_path_bits.npz.

Run on an MI355X from a checkout of the commit IN FRONT OF the pool_type / no_ln_pre / final_ln_after_pool fields (built with
its own kernels); the file in the tree was recorded that way.  It uses nothing those fields add, so a later checkout must
reproduce the same bits -- which is what tests/test_gpu_pool_towers.py::test_default_config_takes_the_old_path_and_gives_its_bits
holds: tiny tower (32 px, patch 8, width 64, 2 layers, head 32, embed 32) + gene-MLP(100 -> 64), seed 3, perturbed 1-D
parameters, synthetic batch 12, both residual streams; normalised image features and four gradients of
sum(image_features * target).

    python tests/golden/make_golden_pool_default.py [ROOT_OF_THE_CHECKOUT_TO_RECORD]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import spatial_clip_amd  # noqa: E402,F401
from spatial_clip_amd import data, model_configs as mc, net  # noqa: E402

GRADS = ("visual.conv1.weight", "visual.ln_pre.weight", "visual.positional_embedding", "visual.ln_post.bias")


def perturb(netobj, seed=11):
    g = torch.Generator().manual_seed(seed)
    sd = netobj.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    netobj.load_state_dict(sd)


def main():
    target = torch.randn(12, 32, generator=torch.Generator().manual_seed(5))
    out = {"target": target.numpy()}
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(100, 64))
    for stream in ("bf16", "fp32"):
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3, residual_stream=stream)
        perturb(n)
        batch = data.synthetic_batch(12, 32, 100, K=4, step=0)
        o = n(batch["images"].cuda(), batch["texts"].cuda())
        out[f"image_features.{stream}"] = o["image_features"].detach().cpu().numpy()
        (o["image_features"] * target.cuda()).sum().backward()
        torch.cuda.synchronize()
        for k in GRADS:
            out[f"g.{stream}.{k}"] = n.store.g(k).cpu().numpy().copy()
    np.savez_compressed(os.path.join(HERE, "pool_default_path_bits.npz"), **out)
    print("wrote pool_default_path_bits.npz from", os.path.dirname(spatial_clip_amd.__file__))


if __name__ == "__main__":
    main()
