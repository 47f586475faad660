#!/usr/bin/env python3
"""Parity yardstick of the dropping training step (tests/test_gpu_patch_dropout.py::test_dropping_step_vs_oracle): for every
case of that test, the distance of the HIP step from the fp32 oracle beside the distance of the SAME oracle composition run
under ``torch.autocast(bfloat16)`` -- the reference's own precision policy, as tools/autocast_noise.py uses it -- from the
fp32 oracle.  Metric of the test: features max|d|, loss |d|, per parameter tensor max|g - g_fp32| / max|g_fp32|.  Lists every
tensor whose HIP distance exceeds 4 %, and the worst tensor of each side.  Run on the GPU box:

    python tools/patch_dropout_parity.py > profiles/patch_dropout_parity.txt"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import spatial_clip_amd  # noqa: F401
from oracle import spatial_clip_oracle as O
from spatial_clip_amd import data, losses, model_configs as mc, module, net, patch_dropout as pd
from tests import _patchdrop_oracle as PO
from tests.test_gpu_patch_dropout import perturb, tiny_cfgs


def oracle(batch, params, ocfg, keep, loss_kind, autocast):
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    aten = O.USE_ATEN_KERNELS
    O.USE_ATEN_KERNELS = bool(autocast) or aten
    try:
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bool(autocast)):
            f = PO.net_forward_keep(batch["images"], batch["texts"], p, ocfg, keep)
            fi, ft, sc = f["image_features"].float(), f["text_features"].float(), f["logit_scale"].float()
            if loss_kind == "clip":
                lo = O.clip_loss(fi, ft, sc)
            else:
                lo = O.spatial_loss(fi, ft, sc, batch["image_tile_ids"], batch["text_tile_ids"], batch["neighbor_tile_ids"],
                                    batch["neighbor_alphas"])
        lo.backward()
    finally:
        O.USE_ATEN_KERNELS = aten
    return fi.detach(), float(lo.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


def rel(g, ref):
    return float((g - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def main():
    geoms = [(64, 32, 32, 8), (128, 64, 48, 16)]
    print("# tools/patch_dropout_parity.py: distance from the fp32 oracle -- HIP step | the oracle under torch.autocast(bfloat16)")
    for (w, hw, im, pa), loss_kind, stream, drop in itertools.product(geoms, ("clip", "spatial"), ("bf16", "fp32"), (0.5, 0.75)):
        cfg, ocfg = tiny_cfgs(w, hw, 2, im, pa)
        B, seed = 12, 3
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, residual_stream=stream, force_patch_dropout=drop)
        perturb(n)
        params = {k: v.cpu() for k, v in n.state_dict().items()}
        batch = data.synthetic_batch(B, im, cfg.gene.n_genes, K=4, step=0)
        n_patch = cfg.vision.tokens - 1
        keep = pd.keep_indices_host(seed, 0, 0, B, n_patch, pd.num_keep(n_patch, drop))
        f32, l32, g32 = oracle(batch, params, ocfg, keep, loss_kind, False)
        f16, l16, g16 = oracle(batch, params, ocfg, keep, loss_kind, True)
        if loss_kind == "clip":
            loss_fn = losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
        else:
            loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                         neighbor_alpha_scale=0.5, float32_logits=True)
        m = module.SpatialClipLitModule(n, loss_fn, None, None)
        out = m.model_step({k: v.cuda() for k, v in batch.items()})
        out["loss"].backward()
        torch.cuda.synchronize()
        gh = {k: n.store.g(k).cpu() for k in params}
        hip = {k: rel(gh[k], g32[k]) for k in params}
        ac = {k: rel(g16[k], g32[k]) for k in params}
        kh, ka = max(hip, key=hip.get), max(ac, key=ac.get)
        print(f"width {w} patch {pa} loss {loss_kind} stream {stream} p {drop}: "
              f"features {float((out['image_features'].detach().cpu() - f32).abs().max()):.2e} | {float((f16 - f32).abs().max()):.2e}; "
              f"loss {abs(float(out['loss'].detach()) - l32):.2e} | {abs(l16 - l32):.2e}; "
              f"worst gradient {hip[kh]:.4f} ({kh}) | {ac[ka]:.4f} ({ka})")
        for k in params:
            if hip[k] > 0.04:
                print(f"    over 4 %: {k}: HIP {hip[k]:.4f} | autocast {ac[k]:.4f} (max|g_fp32| {float(g32[k].abs().max()):.3e})")


if __name__ == "__main__":
    main()
