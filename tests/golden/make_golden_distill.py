#!/usr/bin/env python3
"""Golden vectors for the distillation loss, from the REFERENCE's own open_clip.loss.DistillClipLoss.

Run in the build container only (imports the reference, never copies it; the outputs are inputs + expected outputs):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distill.py

Outputs (float64 throughout, so that tests/_distill_oracle.py can be held to 1e-12; features, never logits)
  distill_w1_B{7,12,64}.npz            one process, B as named, (D, D_t) in {(16, 16), (64, 48)}, (s, s_t) in
  distill_w1_B300_D{16,64}_{tag}.npz   {(14.3, 14.3), (100, 100), (10, 100), (100, 1)}: both losses and the gradients of EACH
                                       loss separately w.r.t. the image features, the text features and the student scale.
                                       B = 300 is split per (D, tag): every file stays under the size limit for a fixture.
                                       Each file lists its cases under "cases" = [[B, D, D_t, tag], ...].
  distill_w2.npz                       a 2-rank gloo spawn (B = 8 per rank, D = 32, D_t = 24, gather_with_grad=True) for
                                       local_loss True and False; per rank the same quantities after every rank's backward."""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, npz, unit  # noqa: E402

W1_B = (7, 12, 64, 300)
W1_D = ((16, 16), (64, 48))
W1_S = {"s14_t14": (14.3, 14.3), "s100_t100": (100.0, 100.0), "s10_t100": (10.0, 100.0), "s100_t1": (100.0, 1.0)}
SPLIT_B = 300           # from this batch size on: one file per (D, tag)
MW_B, MW_D, MW_DT, MW_S, MW_ST = 8, 32, 24, 14.3, 25.0
KEYS = ("closs", "dloss", "gimg_c", "gtxt_c", "gscale_c", "gimg_d", "gtxt_d", "gscale_d")


def features(B, D, Dt, seed):
    """Student pairs (text = noisy image) and an unrelated, better aligned teacher of another width."""
    g = torch.Generator().manual_seed(seed)
    img = unit(torch.randn(B, D, generator=g, dtype=torch.float64)).float()
    txt = unit(img.double() + 0.8 * torch.randn(B, D, generator=g, dtype=torch.float64)).float()
    timg = unit(torch.randn(B, Dt, generator=g, dtype=torch.float64)).float()
    ttxt = unit(timg.double() + 0.4 * torch.randn(B, Dt, generator=g, dtype=torch.float64)).float()
    return img, txt, timg, ttxt


def distill_case(crit, img, txt, timg, ttxt, s, st):
    """Both losses and the gradients of each on its own (two backward passes through one graph)."""
    i = img.double().clone().requires_grad_(True)
    t = txt.double().clone().requires_grad_(True)
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    ti = timg.double().clone().requires_grad_(True)
    tt = ttxt.double().clone().requires_grad_(True)
    c, d = crit(i, t, sc, ti.detach(), tt.detach(), torch.tensor(st, dtype=torch.float64))
    gc = torch.autograd.grad(c, [i, t, sc], retain_graph=True)
    gd = torch.autograd.grad(d, [i, t, sc])
    vals = (c.detach(), d.detach(), gc[0], gc[1], gc[2], gd[0], gd[1], gd[2])
    return {k: np.asarray(v.numpy(), dtype=np.float64) for k, v in zip(KEYS, vals)}


def _worker(rank, world, feats, ret):
    sys.dont_write_bytecode = True
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29581 + world)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, loss_mod, _ = import_reference()
    B = feats[0].shape[0] // world
    sl = slice(rank * B, (rank + 1) * B)
    out = {}
    for local in (True, False):
        crit = loss_mod.DistillClipLoss(local_loss=local, gather_with_grad=True, rank=rank, world_size=world)
        out["local" if local else "global"] = distill_case(crit, *(f[sl] for f in feats), MW_S, MW_ST)
        dist.barrier()
    ret[rank] = out
    dist.destroy_process_group()


def multi_rank(world):
    import torch.multiprocessing as mp
    feats = features(world * MW_B, MW_D, MW_DT, 200 + world)
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, feats, ret), nprocs=world, join=True)
        res = dict(ret)
    arrs = dict(zip(("img", "txt", "timg", "ttxt"), feats), scale=MW_S, dist_scale=MW_ST, world=world)
    for r in range(world):
        for layout, vals in res[r].items():
            for k, v in vals.items():
                arrs[f"r{r}_{layout}_{k}"] = v
    npz(f"distill_w{world}.npz", **arrs)


def main():
    torch.set_num_threads(8)
    _, loss_mod, _ = import_reference()
    crit = loss_mod.DistillClipLoss()
    for B in W1_B:
        files = {}
        for D, Dt in W1_D:
            feats = features(B, D, Dt, 10 * B + D)
            for tag, (s, st) in W1_S.items():
                name = f"distill_w1_B{B}.npz" if B < SPLIT_B else f"distill_w1_B{B}_D{D}_{tag}.npz"
                arrs = files.setdefault(name, {"cases": [], "scales": json.dumps(W1_S)})
                arrs["cases"].append([B, D, Dt, tag])
                for k, f in zip(("img", "txt", "timg", "ttxt"), feats):
                    arrs[f"B{B}_D{D}_{k}"] = f
                for k, v in distill_case(crit, *feats, s, st).items():
                    arrs[f"B{B}_D{D}_{tag}_{k}"] = v
        for name, arrs in files.items():
            arrs["cases"] = json.dumps(arrs["cases"])
            npz(name, **arrs)
    multi_rank(2)


if __name__ == "__main__":
    main()
