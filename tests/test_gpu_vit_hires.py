"""Vision towers above 320 tokens end to end: ViT-L/14 at 336 px (577 tokens: attention on sc_attention_stream.hip) against
the fp32 oracle at reduced and full depth, training steps, graph replay, checkpoint resize, force_image_size and the
training entry point with experiment=vitl14_336_gene_b64."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O

pytestmark = pytest.mark.gpu

N_GENES = 512
# gradients: judged as tests/test_gpu_parity_depth.py judges them, against the reference policy's own autocast (fp32
# stream) on the same weights and batch
GRAD_MEDIAN_OVER_YARDSTICK = 1.35
GRAD_REL_L2_WORST = 0.05


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs, module, net, optim, parity
    return data, graph, losses, model_configs, module, net, optim, parity


def _cfgs(layers=2, name="ViT-L-14-336-gene", n_genes=N_GENES, image_size=None):
    mc = _pkg()[3]
    cfg = mc.get_model_config(name, n_genes=n_genes, image_size=image_size)
    if layers is not None:
        cfg.vision.layers = layers
    v = cfg.vision
    ocfg = O.ModelCfg(cfg.embed_dim, O.VisionCfg(v.image_size, v.patch_size, v.width, v.layers, v.head_width), None,
                      O.GeneCfg(cfg.gene.n_genes, cfg.gene.hidden))
    return cfg, ocfg


def _perturb(n, seed=11, scale=0.02):
    g = torch.Generator().manual_seed(seed)
    sd = n.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + scale * torch.randn(v.shape, generator=g)
    n.load_state_dict(sd)


def _spatial_loss(losses):
    return losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                              neighbor_alpha_scale=0.5, float32_logits=True)


def _oracle(batch, p0, ocfg, autocast=False, grads=True):
    p = {k: t.clone().requires_grad_(grads) for k, t in p0.items()}
    O.USE_ATEN_KERNELS = True
    try:
        with torch.set_grad_enabled(grads), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f = O.net_forward(batch["images"], batch["texts"], p, ocfg)
            f = {k: (t.float() if isinstance(t, torch.Tensor) else t) for k, t in f.items()}
            loss = O.spatial_loss(f["image_features"], f["text_features"], f["logit_scale"], batch["image_tile_ids"],
                                  batch["text_tile_ids"], batch["neighbor_tile_ids"], batch["neighbor_alphas"])
        if grads:
            loss.backward()
    finally:
        O.USE_ATEN_KERNELS = False
    g = {k: t.grad.double() for k, t in p.items() if t.grad is not None} if grads else None
    return f, float(loss.detach()), g


def test_vitl14_336_reduced_depth_vs_fp32_oracle():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=2)
    assert cfg.vision.tokens == 577 and cfg.vision.heads == 16 and cfg.vision.width == 1024
    B = 8
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=4, residual_stream="fp32")
    _perturb(n)
    p0 = {k: t.cpu().clone() for k, t in n.state_dict().items()}
    batch = data.synthetic_batch(B, 336, N_GENES, K=4)
    f32, loss32, g32 = _oracle(batch, p0, ocfg)
    _, _, gpol = _oracle(batch, p0, ocfg, autocast=True)
    m = module.SpatialClipLitModule(n, _spatial_loss(losses), None, None)
    out = m.model_step({k: t.cuda() for k, t in batch.items()})
    out["loss"].backward()
    torch.cuda.synchronize()
    df = float((out["image_features"].detach().float().cpu() - f32["image_features"].detach()).abs().max())
    dl = abs(float(out["loss"].detach()) - loss32)
    assert df <= parity.FEATURE_TOLERANCE["bf16"], df
    assert dl <= parity.LOSS_TOLERANCE["bf16"], dl
    keys = [k for k in g32 if float(g32[k].norm()) > 1e-9]
    assert len(keys) >= 25, len(keys)

    def rel(grads):
        return {k: float((grads[k] - g32[k]).norm() / g32[k].norm()) for k in keys}

    ours = rel({k: n.store.g(k).detach().cpu().double() for k in keys})
    yard = rel(gpol)
    med, ymed = float(np.median(list(ours.values()))), float(np.median(list(yard.values())))
    worst = max(ours, key=ours.get)
    print(f"[ViT-L-14-336 x 2 layers, B={B}] |d feature| {df:.2e}, |d loss| {dl:.2e}; gradient relative L2 median {med:.4f} "
          f"(reference policy {ymed:.4f}), worst {ours[worst]:.4f} ({worst}; policy worst {max(yard.values()):.4f})")
    assert med <= GRAD_MEDIAN_OVER_YARDSTICK * ymed, (med, ymed)
    assert ours[worst] <= max(GRAD_REL_L2_WORST, GRAD_MEDIAN_OVER_YARDSTICK * max(yard.values())), (worst, ours[worst])


def test_vitl14_336_full_depth_forward_vs_fp32_oracle():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=None)
    assert cfg.vision.layers == 24 and cfg.vision.tokens == 577
    B = 16
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=6, residual_stream="fp32")
    p0 = {k: t.cpu() for k, t in n.state_dict().items()}
    batch = data.synthetic_batch(B, 336, N_GENES, K=4)
    f32, loss32, _ = _oracle(batch, p0, ocfg, grads=False)
    m = module.SpatialClipLitModule(n, _spatial_loss(losses), None, None)
    with torch.no_grad():
        out = m.model_step({k: t.cuda() for k, t in batch.items()})
    torch.cuda.synchronize()
    df = float((out["image_features"].float().cpu() - f32["image_features"]).abs().max())
    dl = abs(float(out["loss"]) - loss32)
    print(f"[ViT-L-14-336-gene full depth, B={B}] |d feature| {df:.2e}, |d loss| {dl:.2e}")
    assert df <= parity.FEATURE_TOLERANCE["bf16"], df
    assert dl <= parity.LOSS_TOLERANCE["bf16"], dl


def _module(n, losses, module, optim, warmup=2, total=10):
    m = module.SpatialClipLitModule(
        n, _spatial_loss(losses), functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def test_vitl14_336_three_training_steps_vs_oracle():
    """The bounds of tests/test_gpu_model.py's three-step test (fp32 residual stream)."""
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=2)
    B = 8
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=5, residual_stream="fp32")
    _perturb(n, scale=0.05)
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    m, opt, sched = _module(n, losses, module, optim)
    O.USE_ATEN_KERNELS = True
    try:
        tr = O.OracleTrainer(ocfg, params, loss="spatial", lr=1e-3, warmup=2, total_steps=10)
        for step in range(3):
            batch = data.synthetic_batch(B, 336, N_GENES, K=4, step=step)
            ref = tr.training_step(batch)
            loss = m.training_step({k: v.cuda() for k, v in batch.items()}, step)
            loss.backward()
            nc = opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
            assert abs(float(loss.detach()) - float(ref["loss"])) < 4e-3, (step, float(loss.detach()), float(ref["loss"]))
            assert abs(float(nc[0]) - float(ref["grad_norm"])) < 0.03 * float(ref["grad_norm"]) + 1e-4
    finally:
        O.USE_ATEN_KERNELS = False
    for k in ("visual.proj", "gene.fc2.weight", "visual.transformer.resblocks.1.attn.in_proj_weight",
              "visual.transformer.resblocks.1.mlp.c_fc.weight"):
        a, b = n.store.p(k).cpu(), tr.p[k].detach()
        assert float((a - b).abs().max()) < 2.5e-3, k


def test_vitl14_336_graph_replay_is_bit_identical(monkeypatch):
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    monkeypatch.setenv("SC_GRAPH", "1")
    monkeypatch.setenv("SC_OVERLAP", "0")
    cfg, _ = _cfgs(layers=2)
    B, steps = 8, 3
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(B, 336, N_GENES, K=4, step=s).items()} for s in range(steps)]
    res = {}
    for mode in ("eager", "graph"):
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
        m, opt, sched = _module(n, losses, module, optim, warmup=3, total=40)
        step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        ls = []
        for i in range(steps):
            loss = step.eager(batches[i]) if mode == "eager" else step(batches[i])
            sched.step()
            ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        res[mode] = dict(loss=ls, w=n.store.master.detach().clone(), replays=step.replays, failed=step.failed)
        del n, m, opt, step
    assert res["graph"]["failed"] is None, res["graph"]["failed"]
    assert res["graph"]["replays"] == steps - 1
    assert res["eager"]["loss"] == res["graph"]["loss"], (res["eager"]["loss"], res["graph"]["loss"])
    assert torch.equal(res["eager"]["w"], res["graph"]["w"])
    assert all(np.isfinite(res["eager"]["loss"]))


def test_vitl14_224_checkpoint_loads_into_336(tmp_path):
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    cfg224, _ = _cfgs(layers=2, name="ViT-L-14-gene")
    cfg336, _ = _cfgs(layers=2)
    a = net.SpatialClipNet("custom", None, model_cfg=cfg224, seed=1)
    sa = {k: v.cpu() for k, v in a.state_dict().items()}
    assert sa["visual.positional_embedding"].shape == (257, 1024)
    path = tmp_path / "vitl14_224.pt"
    torch.save({"state_dict": sa}, path)
    b = net.SpatialClipNet("custom", str(path), model_cfg=cfg336, seed=2)
    sb = b.state_dict()
    assert sb["visual.positional_embedding"].shape == (577, 1024)
    want = {"visual.positional_embedding": sa["visual.positional_embedding"].clone()}
    net.resize_pos_embed(want, (24, 24))
    torch.testing.assert_close(sb["visual.positional_embedding"].cpu(), want["visual.positional_embedding"])
    for k in sa:
        if k != "visual.positional_embedding":
            assert torch.equal(sa[k], sb[k].cpu()), k
    batch = data.synthetic_batch(4, 336, N_GENES, K=4)
    with torch.no_grad():
        out = b(batch["images"].cuda(), batch["texts"].cuda())
    assert out["image_features"].shape == (4, cfg336.embed_dim) and torch.isfinite(out["image_features"]).all()


def test_force_image_size_vitb16_trains_one_step():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=N_GENES, seed=7, force_image_size=384)
    assert n.cfg.vision.image_size == 384 and n.cfg.vision.tokens == 577
    assert tuple(n.state_dict()["visual.positional_embedding"].shape) == (577, 768)
    m, opt, sched = _module(n, losses, module, optim, warmup=0)          # no warm-up: the first step moves the weights
    w0 = n.store.master.detach().clone()
    batch = {k: v.cuda() for k, v in data.synthetic_batch(8, 384, N_GENES, K=4).items()}
    loss = m.training_step(batch, 0)
    loss.backward()
    opt.step(grad_scale=1.0, max_norm=1.0)
    sched.step()
    n.store.wait_all()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    assert torch.isfinite(n.store.master).all() and not torch.equal(w0, n.store.master)
    with pytest.raises(ValueError, match="patch size"):
        net.SpatialClipNet("ViT-B-16-gene", None, n_genes=N_GENES, force_image_size=385)


def test_train_entry_vitl14_336_experiment(monkeypatch, tmp_path):
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    from spatial_clip_amd import train
    metrics = train.main(["experiment=vitl14_336_gene_b64", "data.batch_size=8", "data.n_genes=2000",
                          "data.steps_per_epoch=2", "data.val_steps=1", "trainer.max_steps=2",
                          "trainer.log_every_n_steps=1", "test=False"])
    assert "train/loss" in metrics and np.isfinite(float(metrics["train/loss"])), metrics
    assert "val/loss" in metrics and np.isfinite(float(metrics["val/loss"])), metrics
