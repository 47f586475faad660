#!/usr/bin/env python3
"""Golden vectors for the sigmoid (SigLIP) loss and the learnable logit bias, from the REFERENCE's own modules.

Run in the build container only (imports the reference, never copies it; the outputs are inputs + expected outputs):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_siglip.py

Outputs
  siglip_w1.npz           open_clip.loss.SigLipLoss in float64, one process: B in {7, 12, 64}, D in {16, 64},
                          (s, b) in {(10, -10), (14.3, 0), (100, -10), (10, None)}; loss and the gradients w.r.t. the
                          features, the exponentiated scale and the bias.
  siglip_w2.npz / _w4.npz 2- and 4-rank gloo spawns of the same loss for every dist_impl (bidir, shift, reduce,
                          gather -- all four run on gloo); per rank: loss and the local gradients after every rank's
                          backward.  The four agree with each other to fp64 rounding (asserted here).
  loss_bias_grad.npz      ClipLoss and SpatialLoss (W = 1) with a bias that requires grad: loss and d_bias.
  train3_siglip_tiny.npz  the train3_tiny_text recipe (make_golden.py) on CLIP(**tiny, init_logit_scale=log(10),
                          init_logit_bias=-10) with SigLipLoss: losses, grad norms, p3 weights (batch and p0 weights
                          are train3_tiny_text.npz's, p0 logit_scale / logit_bias are stored here)."""
import math
import os
import sys

sys.dont_write_bytecode = True
import json

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, make_batch_ids, npz, sd_np, unit  # noqa: E402

W1_B = (7, 12, 64)
W1_D = (16, 64)
W1_SB = {"s10_bm10": (10.0, -10.0), "s14_b0": (14.3, 0.0), "s100_bm10": (100.0, -10.0), "s10_nob": (10.0, None)}
DIST_IMPLS = ("bidir", "shift", "reduce", "gather")
MW_B, MW_D, MW_S, MW_BIAS = 8, 32, 10.0, -10.0


def features(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    img = unit(torch.randn(B, D, generator=g, dtype=torch.float64)).float()
    txt = unit(img.double() + 0.8 * torch.randn(B, D, generator=g, dtype=torch.float64)).float()
    return img, txt


def siglip_case(loss_mod, img, txt, s, b):
    i = img.double().requires_grad_(True)
    t = txt.double().requires_grad_(True)
    st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    bt = None if b is None else torch.tensor(b, dtype=torch.float64, requires_grad=True)
    l = loss_mod.SigLipLoss()(i, t, st, bt)
    l.backward()
    return {"loss": l.detach().numpy(), "gimg": i.grad.float().numpy(), "gtxt": t.grad.float().numpy(),
            "gscale": st.grad.numpy(), "gbias": np.float64(0.0) if bt is None else bt.grad.numpy()}


def _worker(rank, world, img, txt, ret):
    sys.dont_write_bytecode = True
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29561 + world)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, loss_mod, _ = import_reference()
    B = img.shape[0] // world
    sl = slice(rank * B, (rank + 1) * B)
    out = {}
    for impl in DIST_IMPLS:
        i = img[sl].double().clone().requires_grad_(True)
        t = txt[sl].double().clone().requires_grad_(True)
        s = torch.tensor(MW_S, dtype=torch.float64, requires_grad=True)
        b = torch.tensor(MW_BIAS, dtype=torch.float64, requires_grad=True)
        l = loss_mod.SigLipLoss(rank=rank, world_size=world, dist_impl=impl)(i, t, s, b)
        l.backward()
        out[impl] = {"loss": l.detach().numpy(), "gimg": i.grad.numpy(), "gtxt": t.grad.numpy(),
                     "gscale": s.grad.numpy(), "gbias": b.grad.numpy()}
        dist.barrier()
    ret[rank] = out
    dist.destroy_process_group()


def multi_rank(world):
    import torch.multiprocessing as mp
    img, txt = features(world * MW_B, MW_D, 100 + world)
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, img, txt, ret), nprocs=world, join=True)
        res = dict(ret)
    arrs = {"img": img, "txt": txt, "scale": MW_S, "bias": MW_BIAS, "world": world}
    for r in range(world):
        first = res[r][DIST_IMPLS[0]]
        for impl in DIST_IMPLS:
            for k, v in res[r][impl].items():
                assert np.allclose(v, first[k], rtol=1e-12, atol=1e-14), (world, r, impl, k)
                arrs[f"r{r}_{impl}_{k}"] = np.asarray(v, dtype=np.float64 if np.ndim(v) == 0 else np.float32)
    npz(f"siglip_w{world}.npz", **arrs)


def main():
    torch.set_num_threads(8)
    model, loss_mod, ref_losses = import_reference()

    # ---------------- single rank ------------------------------------------------------------
    arrs = {"cases": json.dumps([[B, D, tag] for B in W1_B for D in W1_D for tag in W1_SB]),
            "sb": json.dumps(W1_SB)}
    for B in W1_B:
        for D in W1_D:
            img, txt = features(B, D, 10 * B + D)
            arrs[f"B{B}_D{D}_img"], arrs[f"B{B}_D{D}_txt"] = img, txt
            for tag, (s, b) in W1_SB.items():
                for k, v in siglip_case(loss_mod, img, txt, s, b).items():
                    arrs[f"B{B}_D{D}_{tag}_{k}"] = v
    npz("siglip_w1.npz", **arrs)

    # ---------------- multi rank (gloo) --------------------------------------------------------
    multi_rank(2)
    multi_rank(4)

    # ---------------- bias gradient of ClipLoss / SpatialLoss -----------------------------------
    B, D, s, b = 12, 32, 14.2857, -3.0
    img, txt = features(B, D, 7)
    ids, nb, al = make_batch_ids(B, 4, torch.Generator().manual_seed(8))
    arrs = {"img": img, "txt": txt, "ids": ids, "nb": nb, "alpha": al, "scale": s, "bias": b}
    for name in ("clip", "spatial"):
        i = img.double().requires_grad_(True)
        t = txt.double().requires_grad_(True)
        st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
        bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
        if name == "clip":
            l = ref_losses.ClipLoss(local_loss=True, gather_with_grad=True)(i, t, st, bt)["contrastive_loss"]
        else:
            crit = ref_losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0,
                                          temp_reg_weight=0.05, neighbor_alpha_scale=0.5, float32_logits=False)
            l = crit(i, t, st, ids, ids.clone(), nb, al, logit_bias=bt)["contrastive_loss"]
        l.backward()
        arrs[f"{name}_loss"], arrs[f"{name}_gbias"] = l.detach().numpy(), bt.grad.numpy()
        arrs[f"{name}_gimg"], arrs[f"{name}_gtxt"] = i.grad.float().numpy(), t.grad.float().numpy()
        arrs[f"{name}_gscale"] = st.grad.numpy()
    npz("loss_bias_grad.npz", **arrs)

    # ---------------- tiny training_step x3 with the sigmoid loss -------------------------------
    t3 = np.load(os.path.join(HERE, "train3_tiny_text.npz"))
    tiny = json.loads(str(t3["cfg"]))
    images, texts = torch.from_numpy(t3["images"]), torch.from_numpy(t3["texts"])
    torch.manual_seed(6)
    clip = model.CLIP(**tiny, init_logit_scale=math.log(10), init_logit_bias=-10)
    p0 = sd_np(clip)
    opt = torch.optim.AdamW(clip.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    warm, total = 2, 10

    def lam(step):
        if step < warm:
            return step / max(1, warm)
        pr = (step - warm) / max(1, total - warm)
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * pr)))

    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    crit = loss_mod.SigLipLoss()
    losses, norms = [], []
    for step in range(3):
        opt.zero_grad()
        f_i = clip.encode_image(images, normalize=True)
        f_t = clip.encode_text(texts, normalize=True)
        l = crit(f_i, f_t, clip.logit_scale.exp(), clip.logit_bias)
        l.backward()
        l = l.detach()
        n = torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)
        opt.step()
        sched.step()
        losses.append(float(l))
        norms.append(float(n))
    # the initial weights are train3_tiny_text.npz's p0 (same seed, same init order) but for logit_scale / logit_bias:
    # only those two are stored, which keeps the file under the size limit for a committed fixture
    for k, v in p0.items():
        if "logit" not in k:
            assert np.array_equal(v.numpy(), t3["p0." + k]), k
    arrs = {"losses": np.array(losses), "grad_norms": np.array(norms), "cfg": json.dumps(tiny), "warmup": warm,
            "total": total, "init_logit_scale": math.log(10), "init_logit_bias": -10.0,
            "p0.logit_scale": p0["logit_scale"], "p0.logit_bias": p0["logit_bias"]}
    for k, v in sd_np(clip).items():
        arrs["p3." + k] = v
    npz("train3_siglip_tiny.npz", **arrs)


if __name__ == "__main__":
    main()
