"""Sigmoid (SigLIP) loss and the learnable logit bias on the device, against the REFERENCE's own numbers
(tests/golden/make_golden_siglip.py): the head and SigLipLoss at one rank, 2 and 4 gloo ranks for every dist_impl, the
bias gradient of ClipLoss / SpatialLoss, three training steps, checkpoints, graph replay and the training entry point."""
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, contrastive, data, graph, losses, model_configs as mc, module, net, optim
    return comm, contrastive, data, graph, losses, mc, module, net, optim


def _npz(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _close_scalar(got, want, rel):
    return abs(float(got) - float(want)) <= 5e-6 + rel * abs(float(want))


def _check(got, want, tag):
    """got / want: dicts of loss, gimg, gtxt, gscale, gbias (want: the reference's, for the same upstream gradient)."""
    assert _close_scalar(got["loss"], want["loss"], 2e-6), (tag, "loss", float(got["loss"]), float(want["loss"]))
    for k in ("gimg", "gtxt"):
        np.testing.assert_allclose(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64),
                                   atol=2e-6, rtol=1e-4, err_msg=f"{tag} {k}")
    for k in ("gscale", "gbias"):
        assert _close_scalar(got[k], want[k], 1e-5), (tag, k, float(got[k]), float(want[k]))


# ---------------------------------------------------------------------------------------------------------- one rank
def _w1_cases(golden_dir):
    z = _npz(golden_dir, "siglip_w1.npz")
    sb = json.loads(str(z["sb"]))
    return z, sb, json.loads(str(z["cases"]))


@pytest.mark.parametrize("upstream", [1.0, -2.5])
def test_siglip_single_rank_matches_reference(golden_dir, upstream):
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    z, sb, cases = _w1_cases(golden_dir)
    assert len(cases) == 24
    for B, D, tag in cases:
        s, b = sb[tag]
        p = f"B{B}_D{D}_{tag}_"
        img = torch.from_numpy(z[f"B{B}_D{D}_img"]).cuda()
        txt = torch.from_numpy(z[f"B{B}_D{D}_txt"]).cuda()
        want = {k: z[p + k] * (upstream if k != "loss" else 1.0) for k in ("loss", "gimg", "gtxt", "gscale", "gbias")}
        # the head function: gradients for an upstream gradient of 1
        st = torch.tensor(s, device="cuda")
        bt = None if b is None else torch.tensor(b, device="cuda")
        res = C.siglip_forward_backward(img, txt, st, bt, join_local=True)
        if upstream == 1.0:
            _check({"loss": res["loss"], "gimg": res["d_image"].cpu(), "gtxt": res["d_text"].cpu(),
                    "gscale": res["d_scale"], "gbias": want["gbias"] if b is None else res["d_bias"]}, want, f"head {p}")
            res2 = C.siglip_forward_backward(img, txt, st, bt, join_local=True)
            assert torch.equal(res["grads"], res2["grads"]) and torch.equal(res["loss"], res2["loss"]), p   # bitwise
        # the loss class under autograd
        i = img.clone().requires_grad_(True)
        t = txt.clone().requires_grad_(True)
        sg = torch.tensor(s, device="cuda", requires_grad=True)
        bg = None if b is None else torch.tensor(b, device="cuda", requires_grad=True)
        loss = losses.SigLipLoss()(i, t, sg, bg)
        assert loss.dim() == 0
        loss.backward(torch.tensor(upstream, device="cuda"))
        got = {"loss": loss.detach(), "gimg": i.grad.cpu(), "gtxt": t.grad.cpu(), "gscale": sg.grad,
               "gbias": want["gbias"] if bg is None else bg.grad}
        _check(got, want, f"loss {p} g={upstream}")


def test_siglip_output_dict_and_dist_impl():
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    with pytest.raises(AssertionError):
        losses.SigLipLoss(dist_impl="ring")
    f = torch.nn.functional.normalize(torch.randn(8, 16, device="cuda"), dim=-1)
    out = losses.SigLipLoss(dist_impl="gather")(f, f, torch.tensor(10.0, device="cuda"), None, output_dict=True)
    assert set(out) == {"contrastive_loss"} and out["contrastive_loss"].dim() == 0


# ------------------------------------------------------------------------------------------------------- multi rank
def _siglip_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, losses, model_configs as mc, module, net
    z = np.load(os.path.join(ROOT, "tests", "golden", f"siglip_w{world}.npz"))
    img, txt = torch.from_numpy(z["img"]), torch.from_numpy(z["txt"])
    B = img.shape[0] // world
    sl = slice(rank * B, (rank + 1) * B)
    out = {}
    for impl in ("bidir", "shift", "reduce", "gather"):
        i = img[sl].cuda().requires_grad_(True)
        t = txt[sl].cuda().requires_grad_(True)
        s = torch.tensor(float(z["scale"]), device="cuda", requires_grad=True)
        b = torch.tensor(float(z["bias"]), device="cuda", requires_grad=True)
        l = losses.SigLipLoss(rank=rank, world_size=world, dist_impl=impl)(i, t, s, b)
        l.backward()
        out[impl] = {"loss": float(l), "gimg": i.grad.cpu().numpy(), "gtxt": t.grad.cpu().numpy(),
                     "gscale": float(s.grad), "gbias": float(b.grad)}
    # one module step: the text features travel in ONE all-gather launched from the net, the image side is not gathered,
    # and the remote text gradients come back in ONE [G, D] reduce-scatter
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 1, 32), text=None, gene=mc.GeneCfg(100, 64),
                      init_logit_bias=-10.0)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=1)
    m = module.SpatialClipLitModule(n, losses.SigLipLoss(dist_impl="bidir"), None, None)
    from spatial_clip_amd import data
    batch = {k: v.cuda() for k, v in data.synthetic_batch(4, 32, 100, K=4, step=rank).items()}
    before = {k: list(v) for k, v in comm.STATS.items()}
    res = m.model_step(batch)
    res["loss"].backward()
    torch.cuda.synchronize()
    after = {k: list(v) for k, v in comm.STATS.items()}
    delta = {k: [after[k][0] - before.get(k, [0, 0])[0], after[k][1] - before.get(k, [0, 0])[1]] for k in after}
    out["step"] = {"launched": m._feature_gather.launched, "delta": delta,
                   "bias_grad_finite": bool(torch.isfinite(n.store.g("logit_bias")).all())}
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_siglip_multi_rank_matches_reference(world):
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_siglip_worker, args=(world, 29731 + world, ret), nprocs=world, join=True)
        res = dict(ret)
    z = np.load(os.path.join(ROOT, "tests", "golden", f"siglip_w{world}.npz"))
    G, D = z["img"].shape
    for r in range(world):
        for impl in ("bidir", "shift", "reduce", "gather"):
            want = {k: z[f"r{r}_{impl}_{k}"] for k in ("loss", "gimg", "gtxt", "gscale", "gbias")}
            _check(res[r][impl], want, f"W={world} rank {r} {impl}")
        st = res[r]["step"]
        assert st["launched"] == 1, st                                   # text side only
        assert st["delta"]["all_gather(features|ids)"][0] == 1, st["delta"]
        rs = st["delta"]["reduce_scatter(d features)"]
        assert rs[0] == 1 and rs[1] == world * 4 * 32 * 4, rs           # [G, D] fp32 (G = W * 4, D = 32)
        assert st["bias_grad_finite"]


# ---------------------------------------------------------------------------------- bias gradient of ClipLoss / Spatial
def test_clip_and_spatial_loss_bias_gradient(golden_dir):
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    z = _npz(golden_dir, "loss_bias_grad.npz")
    img, txt = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["txt"]).cuda()
    ids, nb, al = (torch.from_numpy(z[k]).cuda() for k in ("ids", "nb", "alpha"))
    for name in ("clip", "spatial"):
        if name == "clip":
            crit = losses.ClipLoss(local_loss=True, gather_with_grad=True)
        else:
            crit = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                      neighbor_alpha_scale=0.5, float32_logits=True)
        i, t = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        s = torch.tensor(float(z["scale"]), device="cuda", requires_grad=True)
        b = torch.tensor(float(z["bias"]), device="cuda", requires_grad=True)
        extra = () if name == "clip" else (ids, ids.clone(), nb, al)
        l = crit(i, t, s, *extra, logit_bias=b)["contrastive_loss"]
        l.backward()
        assert b.grad is not None
        _check({"loss": l.detach(), "gimg": i.grad.cpu(), "gtxt": t.grad.cpu(), "gscale": s.grad, "gbias": b.grad},
               {k: z[f"{name}_{k}"] for k in ("loss", "gimg", "gtxt", "gscale", "gbias")}, name)


@pytest.mark.parametrize("kind", ["clip", "spatial"])
def test_clip_and_spatial_without_bias_grad_are_unchanged(golden_dir, kind):
    """No bias, or a bias that does not require grad: the loss node returns the head's own gradients, scaled by the
    upstream gradient in one launch -- the bits of the path before the bias became an autograd input."""
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    z = _npz(golden_dir, "loss_bias_grad.npz")
    img, txt = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["txt"]).cuda()
    ids, nb, al = (torch.from_numpy(z[k]).cuda() for k in ("ids", "nb", "alpha"))
    s0 = torch.tensor(float(z["scale"]), device="cuda")
    kw = {} if kind == "clip" else dict(image_tile_ids=ids, text_tile_ids=ids, neighbor_tile_ids=nb, neighbor_alphas=al,
                                        cap_logit_scale=40.0, temp_reg_weight=0.05, neighbor_alpha_scale=0.5)
    for bias in (None, torch.tensor(float(z["bias"]), device="cuda")):
        ref = C.contrastive_forward_backward(img, txt, s0, mode=kind, logit_bias=bias, join_local=True, want_recall=False,
                                             **kw)
        g = torch.tensor(-2.5, device="cuda")
        want = ref["grads"][:-1] * g            # d_image | d_text | d_scale
        if kind == "clip":
            crit = losses.ClipLoss(local_loss=True, gather_with_grad=True)
        else:
            crit = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                      neighbor_alpha_scale=0.5, float32_logits=True)
        i, t = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        s = s0.clone().requires_grad_(True)
        extra = () if kind == "clip" else (ids, ids, nb, al)
        l = crit(i, t, s, *extra, logit_bias=bias)["contrastive_loss"]
        assert torch.equal(l.detach(), ref["loss"])
        l.backward(g)
        got = torch.cat([i.grad.reshape(-1), t.grad.reshape(-1), s.grad.reshape(1)])
        assert torch.equal(got, want), kind


# ------------------------------------------------------------------------------------------------- three training steps
def test_reference_three_training_steps_siglip(golden_dir):
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    z = _npz(golden_dir, "train3_siglip_tiny.npz")
    t3 = _npz(golden_dir, "train3_tiny_text.npz")
    c = json.loads(str(z["cfg"]))
    v, t = c["vision_cfg"], c["text_cfg"]
    cfg = mc.ModelCfg(embed_dim=c["embed_dim"],
                      vision=mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64)),
                      text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, init_logit_scale=float(z["init_logit_scale"]),
                           init_logit_bias=float(z["init_logit_bias"]))
    p0 = {k[3:]: torch.from_numpy(t3[k]) for k in t3.files if k.startswith("p0.")}
    p0["logit_scale"] = torch.from_numpy(z["p0.logit_scale"])
    p0["logit_bias"] = torch.from_numpy(z["p0.logit_bias"])
    n.load_state_dict(p0)
    m = module.SpatialClipLitModule(
        n, losses.SigLipLoss(), functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=int(z["warmup"])))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = int(z["total"]), None, int(z["total"])
    m.trainer = T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    batch = {"images": torch.from_numpy(t3["images"]).cuda(), "texts": torch.from_numpy(t3["texts"]).cuda()}
    for step in range(3):
        loss = m.training_step(batch, step)
        loss.backward()
        nc = opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()
        assert abs(float(loss.detach()) - float(z["losses"][step])) < (4e-3 if step < 2 else 2e-2), \
            (step, float(loss.detach()), float(z["losses"][step]))
        assert abs(float(nc[0]) - float(z["grad_norms"][step])) < 0.05 * float(z["grad_norms"][step])
    for k in ("visual.proj", "text_projection", "token_embedding.weight", "visual.conv1.weight", "logit_bias",
              "logit_scale"):
        assert float((n.store.p(k).cpu() - torch.from_numpy(z["p3." + k])).abs().max()) < 3e-3, k
    assert float(n.store.p("logit_bias")) != -10.0


# ---------------------------------------------------------------------------------------------------------- checkpoints
def _tiny_cfg(mc, bias):
    return mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 1, 32), text=None, gene=mc.GeneCfg(100, 64),
                       init_logit_bias=bias)


def test_checkpoints_with_and_without_bias(golden_dir, tmp_path):
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    plain = net.SpatialClipNet("custom", None, model_cfg=_tiny_cfg(mc, None), seed=2)
    biased = net.SpatialClipNet("custom", None, model_cfg=_tiny_cfg(mc, -10.0), seed=2)
    assert plain.model.logit_bias is None and "logit_bias" not in plain.state_dict()
    assert float(biased.model.logit_bias) == -10.0
    # a CLIP checkpoint (no bias) into a bias net: bias 0, no missing-key error (factory.py:211-213)
    sd = plain.state_dict()
    biased.load_checkpoint_state_dict(dict(sd))
    assert float(biased.store.p("logit_bias")) == 0.0
    biased.load_state_dict(dict(sd))
    assert float(biased.store.p("logit_bias")) == 0.0
    # a [1]-shaped bias is reshaped
    sd1 = dict(sd, logit_bias=torch.tensor([-7.5]), logit_scale=sd["logit_scale"].reshape(1))
    biased.load_checkpoint_state_dict(sd1)
    assert float(biased.store.p("logit_bias")) == -7.5
    # .safetensors and TorchScript files carry the key
    from safetensors.torch import save_file
    src = biased.state_dict()
    src["logit_bias"] = torch.tensor(-4.25)
    f1 = str(tmp_path / "w.safetensors")
    save_file({k: v.cpu().contiguous() for k, v in src.items()}, f1)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for k, v in src.items():
                self.register_buffer(k.replace(".", "__"), v.cpu())
    f2 = str(tmp_path / "w.pt")
    torch.jit.script(M()).save(f2)
    for f, want in ((f1, -4.25),):
        got = net.read_checkpoint_file(f)
        assert float(got["logit_bias"]) == want
        n2 = net.SpatialClipNet("custom", f, model_cfg=_tiny_cfg(mc, -10.0), seed=3)
        assert float(n2.store.p("logit_bias")) == want
        assert torch.equal(n2.store.p("visual.proj").cpu(), src["visual.proj"].cpu())
    ts = net.read_checkpoint_file(f2)
    assert float(ts["logit_bias"]) == -4.25


# ---------------------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_of_a_siglip_step_is_bit_identical(monkeypatch):
    comm, C, data, graph, losses, mc, module, net, optim = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "0")
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64),
                      init_logit_scale=2.302585092994046, init_logit_bias=-10.0)
    B, steps = 24, 6
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=s).items()} for s in range(steps)]
    res = {}
    for mode in ("eager", "graph"):
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
        m = module.SpatialClipLitModule(
            n, losses.SigLipLoss(), functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6,
                                                      weight_decay=0.1),
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=3))

        class T:
            max_steps, max_epochs, estimated_stepping_batches = 40, None, 40
        m.trainer = T()
        oc = m.configure_optimizers()
        opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        ls = []
        for i in range(steps):
            loss = step.eager(batches[i]) if mode == "eager" else step(batches[i])
            sched.step()
            ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        res[mode] = dict(loss=ls, w=n.store.master.detach().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                         bias=float(n.store.p("logit_bias")), replays=step.replays, failed=step.failed)
    assert res["graph"]["failed"] is None, res["graph"]["failed"]
    assert res["graph"]["replays"] == steps - 1
    assert res["eager"]["loss"] == res["graph"]["loss"], (res["eager"]["loss"], res["graph"]["loss"])
    for k in ("w", "m", "v"):
        assert torch.equal(res["eager"][k], res["graph"][k]), k
    assert res["eager"]["bias"] == res["graph"]["bias"] != -10.0
    assert all(np.isfinite(res["eager"]["loss"]))


# ------------------------------------------------------------------------------------------------------ training entry
def test_train_entry_point_with_the_sigmoid_loss(tmp_path):
    env = dict(os.environ, PROJECT_ROOT=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "spatial_clip_amd.train", "experiment=smoke_shards", "loss=siglip",
           "model.net.init_logit_bias=-10", "model.net.init_logit_scale=2.302585", "trainer.max_steps=4",
           "trainer.fast_dev_run=False", "trainer.max_epochs=1", "data.steps_per_epoch=4", "data.val_steps=1",
           "save_ckpt=True", "callbacks=default", "test=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert last, r.stdout[-2000:]
    metrics = eval(last[-1], {"nan": float("nan"), "inf": float("inf")})      # the dict train.main prints
    assert all(np.isfinite(float(v)) for k, v in metrics.items() if "loss" in k and isinstance(v, (int, float))), metrics
    ckpts = glob.glob(os.path.join(str(tmp_path), "**", "last.ckpt"), recursive=True)
    assert ckpts, r.stdout[-2000:]
    sd = torch.load(ckpts[0], map_location="cpu", weights_only=False)["state_dict"]
    assert "logit_bias" in sd and float(sd["logit_bias"]) != -10.0, float(sd.get("logit_bias", float("nan")))
    # a non-finite loss on any step would have left non-finite gradients and weights behind
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
