"""ViT-H towers (width 1280 = 16 heads of 80: attention on sc_attention_stream.hip) end to end: the reference's own
ResidualAttentionBlock at head dim 80 through one HIP block, ViT-H-14-gene against the fp32 oracle at reduced and full
depth, ViT-H-16 with the reference text tower (causal head dim 64 beside head dim 80), training steps, graph replay,
state_dict round trips, the construction-time refusal of 378 px and the training entry point with
experiment=vith14_gene_b128.  Helpers and constants are those of tests/test_gpu_vit_hires.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_GENES = 512
# gradients: judged as tests/test_gpu_parity_depth.py judges them, against the reference policy's own autocast (fp32
# stream) on the same weights and batch
GRAD_MEDIAN_OVER_YARDSTICK = 1.35
GRAD_REL_L2_WORST = 0.05


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs, module, net, optim, parity
    return data, graph, losses, model_configs, module, net, optim, parity


def _cfgs(layers=2, name="ViT-H-14-gene", n_genes=N_GENES, text_layers=None):
    mc = _pkg()[3]
    cfg = mc.get_model_config(name, n_genes=n_genes)
    if layers is not None:
        cfg.vision.layers = layers
    v = cfg.vision
    ov = O.VisionCfg(v.image_size, v.patch_size, v.width, v.layers, v.head_width)
    if cfg.text is not None:
        if text_layers is not None:
            cfg.text.layers = text_layers
        t = cfg.text
        ocfg = O.ModelCfg(cfg.embed_dim, ov, O.TextCfg(t.context_length, t.vocab_size, t.width, t.heads, t.layers, t.mlp_ratio),
                          None, quick_gelu=bool(cfg.quick_gelu))
    else:
        ocfg = O.ModelCfg(cfg.embed_dim, ov, None, O.GeneCfg(cfg.gene.n_genes, cfg.gene.hidden))
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


# ------------------------------------------------------------------------------------------ the reference's block at dh = 80
def _one_block_stack(d, heads, causal, res16, mlp):
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import model_configs as mc, net, towers
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, d, 1, d // heads, mlp / d), text=None, gene=mc.GeneCfg(64, 32))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=0)
    stack = towers.TransformerStack(n.store, "visual.transformer.resblocks.", d, heads, 1, mlp, causal=causal,
                                    cls_only_last=False, res16_ok=res16)
    stack.res_stream = "bf16" if res16 else "fp32"
    return n, stack


@pytest.mark.parametrize("name", ["blk_dh80", "blk_dh80_causal"])
@pytest.mark.parametrize("res16", [False, True])
def test_reference_block_fixture_dh80_through_one_hip_block(name, res16):
    """tests/test_gpu_parity_depth.py::test_reference_block_fixture_through_one_hip_block on the head-dim-80 fixtures: its
    procedure and its bounds (y, gx relative L2 <= 0.006; every parameter gradient relative L2 <= 0.015 and max-abs <= 0.02 of
    the largest entry), copied: they come from bf16 operand rounding with fp32 accumulation, not from the head dim.  The
    fixtures keep their weight matrices and those matrices' gradients in files of their own (tests/golden/
    make_golden_vith.py) and use MLP width 160."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    z.update(np.load(os.path.join(GOLDEN, "blk_dh80_weights.npz")))
    z.update(np.load(os.path.join(GOLDEN, name + "_wgrads.npz")))
    heads, causal = int(z["heads"]), bool(int(z["causal"]))
    x = torch.from_numpy(z["x"]).float()
    Bn, L, d = x.shape
    assert d // heads == 80 and sum(k.startswith("p.") for k in z) == sum(k.startswith("g.") for k in z) == 12
    n, stack = _one_block_stack(d, heads, causal, res16, mlp=z["p.mlp.c_fc.weight"].shape[0])
    sd = n.state_dict()
    for k in z:
        if k.startswith("p."):
            assert tuple(sd["visual.transformer.resblocks.0." + k[2:]].shape) == z[k].shape, k
            sd["visual.transformer.resblocks.0." + k[2:]] = torch.from_numpy(z[k]).float()
    n.load_state_dict(sd)
    M = Bn * L
    y = stack.forward(x.reshape(M, d).cuda().contiguous(), Bn, L)
    torch.cuda.synchronize()
    yh = y.float().cpu().reshape(Bn, L, d)
    yr = torch.from_numpy(z["y"]).float()

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def mx(a, b):
        return float((a - b).abs().max() / b.abs().max())
    e_y = rel(yh, yr)
    gy = torch.from_numpy(z["gy"]).float().reshape(M, d).cuda().contiguous()
    dres = gy.clone()
    dres_bf = gy.to(torch.bfloat16)
    n.store.grad.zero_()
    out = stack.backward(dres, dres_bf, last_bias_colsum_done=False)
    torch.cuda.synchronize()
    gx = out.float().cpu().reshape(Bn, L, d)
    e_gx = rel(gx, torch.from_numpy(z["gx"]).float())
    errs = {}
    for k in z:
        if k.startswith("g."):
            gh = n.store.g("visual.transformer.resblocks.0." + k[2:]).cpu()
            gr = torch.from_numpy(z[k]).float()
            errs[k[2:]] = (rel(gh, gr), mx(gh, gr))
    worst = max(errs, key=lambda k: errs[k][0])
    print(f"[{name}, residual stream {'bf16' if res16 else 'fp32'}] relative L2: y {e_y:.4f}, gx {e_gx:.4f}, worst parameter "
          f"gradient {worst} {errs[worst][0]:.4f} (max-abs {errs[worst][1]:.4f})")
    assert e_y <= 0.006, e_y
    assert e_gx <= 0.006, e_gx
    for k, (r, a) in errs.items():
        assert r <= 0.015 and a <= 0.02, (k, r, a)


# ------------------------------------------------------------------------------------------ ViT-H-14-gene against the oracle
def test_vith14_reduced_depth_vs_fp32_oracle():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=2)
    assert cfg.vision.tokens == 257 and cfg.vision.heads == 16 and cfg.vision.width == 1280 and cfg.vision.head_width == 80
    B = 8
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=4, residual_stream="fp32")
    _perturb(n)
    p0 = {k: t.cpu().clone() for k, t in n.state_dict().items()}
    batch = data.synthetic_batch(B, 224, N_GENES, K=4)
    f32, loss32, g32 = _oracle(batch, p0, ocfg)
    _, _, gpol = _oracle(batch, p0, ocfg, autocast=True)
    m = module.SpatialClipLitModule(n, _spatial_loss(losses), None, None)
    out = m.model_step({k: t.cuda() for k, t in batch.items()})
    out["loss"].backward()
    torch.cuda.synchronize()
    df = float((out["image_features"].detach().float().cpu() - f32["image_features"].detach()).abs().max())
    dl = abs(float(out["loss"].detach()) - loss32)
    keys = [k for k in g32 if float(g32[k].norm()) > 1e-9]

    def rel(grads):
        return {k: float((grads[k] - g32[k]).norm() / g32[k].norm()) for k in keys}

    ours = rel({k: n.store.g(k).detach().cpu().double() for k in keys})
    yard = rel(gpol)
    med, ymed = float(np.median(list(ours.values()))), float(np.median(list(yard.values())))
    worst = max(ours, key=ours.get)
    print(f"[ViT-H-14 x 2 layers, B={B}] |d feature| {df:.2e}, |d loss| {dl:.2e}; gradient relative L2 median {med:.4f} "
          f"(reference policy {ymed:.4f}), worst {ours[worst]:.4f} ({worst}; policy worst {max(yard.values()):.4f})")
    assert df <= parity.FEATURE_TOLERANCE["bf16"], df
    assert dl <= parity.LOSS_TOLERANCE["bf16"], dl
    assert len(keys) >= 25, len(keys)
    assert med <= GRAD_MEDIAN_OVER_YARDSTICK * ymed, (med, ymed)
    assert ours[worst] <= max(GRAD_REL_L2_WORST, GRAD_MEDIAN_OVER_YARDSTICK * max(yard.values())), (worst, ours[worst])


def test_vith14_full_depth_forward_vs_fp32_oracle():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=None)
    assert cfg.vision.layers == 32 and cfg.vision.tokens == 257
    B = 8
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=6, residual_stream="fp32")
    p0 = {k: t.cpu() for k, t in n.state_dict().items()}
    batch = data.synthetic_batch(B, 224, N_GENES, K=4)
    f32, loss32, _ = _oracle(batch, p0, ocfg, grads=False)
    m = module.SpatialClipLitModule(n, _spatial_loss(losses), None, None)
    with torch.no_grad():
        out = m.model_step({k: t.cuda() for k, t in batch.items()})
    torch.cuda.synchronize()
    df = float((out["image_features"].float().cpu() - f32["image_features"]).abs().max())
    dl = abs(float(out["loss"]) - loss32)
    print(f"[ViT-H-14-gene full depth, B={B}] |d feature| {df:.2e}, |d loss| {dl:.2e}")
    assert df <= parity.FEATURE_TOLERANCE["bf16"], df
    assert dl <= parity.LOSS_TOLERANCE["bf16"], dl


def test_vith16_with_reference_text_tower_vs_fp32_oracle():
    """ViT-H-16 (197 tokens, head dim 80) with the reference's text tower (77 tokens causal, 16 heads of 64) at 2 + 2 layers:
    both attention families in one step."""
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=2, name="ViT-H-16", text_layers=2)
    assert cfg.vision.tokens == 197 and cfg.vision.head_width == 80 and cfg.text.width // cfg.text.heads == 64
    B = 8
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=8, residual_stream="fp32")
    _perturb(n)
    p0 = {k: t.cpu().clone() for k, t in n.state_dict().items()}
    base = data.synthetic_batch(B, 224, 64, K=4)
    batch = dict(base, texts=data.synthetic_captions(B, 77, 49408, seed=5))
    f32, loss32, g32 = _oracle(batch, p0, ocfg)
    m = module.SpatialClipLitModule(n, _spatial_loss(losses), None, None)
    out = m.model_step({k: t.cuda() for k, t in batch.items()})
    out["loss"].backward()
    torch.cuda.synchronize()
    dfi = float((out["image_features"].detach().float().cpu() - f32["image_features"].detach()).abs().max())
    dft = float((out["text_features"].detach().float().cpu() - f32["text_features"].detach()).abs().max())
    dl = abs(float(out["loss"].detach()) - loss32)
    print(f"[ViT-H-16 + text tower, 2 + 2 layers, B={B}] |d image feature| {dfi:.2e}, |d text feature| {dft:.2e}, "
          f"|d loss| {dl:.2e}")
    assert max(dfi, dft) <= parity.FEATURE_TOLERANCE["bf16"], (dfi, dft)
    assert dl <= parity.LOSS_TOLERANCE["bf16"], dl
    for k in ("visual.transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.0.attn.in_proj_weight"):
        r = float((n.store.g(k).detach().cpu().double() - g32[k]).norm() / g32[k].norm())
        assert r <= GRAD_REL_L2_WORST, (k, r)


# ------------------------------------------------------------------------------------------ training
def _module(n, losses, module, optim, warmup=2, total=10, lr=1e-3):
    m = module.SpatialClipLitModule(
        n, _spatial_loss(losses), functools.partial(optim.FusedAdamW, lr=lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def test_vith14_three_steps_on_a_fixed_batch_loss_falls():
    """Three AdamW updates on one batch, each step beside the fp32 oracle trainer (bounds of the three-step tests of
    tests/test_gpu_vit_hires.py / test_gpu_model.py: loss 4e-3, gradient norm 3 %), then a fourth evaluation: the loss is
    finite and falls from step to step.  lr 3e-5 without warm-up: the first Adam update moves every weight by lr whatever
    its gradient, and on a freshly initialised 1280-wide net the fp32 oracle itself goes UP on it at 1e-3 and at 1e-4
    (2.09 -> 2.20) and falls by 0.016 or more per step at 3e-5 (2.089, 2.040, 2.024, 2.002), four times the loss bound."""
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    cfg, ocfg = _cfgs(layers=2)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=5, residual_stream="fp32")
    _perturb(n, scale=0.05)
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    m, opt, sched = _module(n, losses, module, optim, warmup=0, lr=3e-5)
    batch = data.synthetic_batch(8, 224, N_GENES, K=4)
    dbatch = {k: v.cuda() for k, v in batch.items()}
    ls, ref_ls = [], []
    O.USE_ATEN_KERNELS = True
    try:
        tr = O.OracleTrainer(ocfg, params, loss="spatial", lr=3e-5, warmup=0, total_steps=10)
        for step in range(3):
            ref = tr.training_step(batch)
            loss = m.training_step(dbatch, step)
            loss.backward()
            nc = opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
            ls.append(float(loss.detach()))
            ref_ls.append(float(ref["loss"]))
            assert abs(ls[-1] - ref_ls[-1]) < 4e-3, (step, ls, ref_ls)
            assert abs(float(nc[0]) - float(ref["grad_norm"])) < 0.03 * float(ref["grad_norm"]) + 1e-4
    finally:
        O.USE_ATEN_KERNELS = False
    with torch.no_grad():
        ls.append(float(m.model_step(dbatch)["loss"]))
    n.store.wait_all()
    torch.cuda.synchronize()
    print(f"[ViT-H-14 x 2 layers, fixed batch] loss {ls} (oracle {ref_ls})")
    assert all(np.isfinite(ls)) and torch.isfinite(n.store.master).all()
    assert ls[0] > ls[1] > ls[2] > ls[3], ls


def test_vith14_graph_replay_is_bit_identical(monkeypatch):
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    monkeypatch.setenv("SC_GRAPH", "1")
    monkeypatch.setenv("SC_OVERLAP", "0")
    cfg, _ = _cfgs(layers=2)
    B, steps = 8, 3
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(B, 224, N_GENES, K=4, step=s).items()} for s in range(steps)]
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


# ------------------------------------------------------------------------------------------ state dicts, construction
def test_vith14_state_dict_round_trip():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    cfg, _ = _cfgs(layers=2)
    a = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=1)
    _perturb(a)
    sa = {k: v.cpu().clone() for k, v in a.state_dict().items()}
    assert tuple(sa["visual.transformer.resblocks.1.attn.in_proj_weight"].shape) == (3840, 1280)
    b = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=2)
    assert not torch.equal(b.state_dict()["visual.proj"].cpu(), sa["visual.proj"])
    b.load_state_dict(sa)
    sb = b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k].cpu()), k
    batch = data.synthetic_batch(4, 224, N_GENES, K=4)
    with torch.no_grad():
        fa = a(batch["images"].cuda(), batch["texts"].cuda())["image_features"]
        fb = b(batch["images"].cuda(), batch["texts"].cuda())["image_features"]
    assert torch.equal(fa, fb) and torch.isfinite(fa).all()


def test_vith16_loads_a_state_dict_with_the_reference_keys():
    """A state_dict with exactly the keys and shapes of open_clip's ViT-H-16 (tests/golden/state_dict_manifest_vith.json)
    loads into the full-size net and comes back unchanged."""
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    ref = json.load(open(os.path.join(GOLDEN, "state_dict_manifest_vith.json")))["ViT-H-16"]
    n = net.SpatialClipNet("ViT-H-16", None, seed=1)
    assert {k: list(v.shape) for k, v in n.state_dict().items()} == ref
    g = torch.Generator().manual_seed(2)
    sd = {k: (torch.full(shp, 0.01 * (i % 7 + 1)) if len(shp) != 1 else torch.randn(shp, generator=g))
          for i, (k, shp) in enumerate(ref.items())}
    n.load_state_dict(sd)
    back = n.state_dict()
    for k in ("visual.transformer.resblocks.31.attn.in_proj_weight", "visual.transformer.resblocks.0.ln_1.weight",
              "visual.positional_embedding", "visual.proj", "transformer.resblocks.23.mlp.c_proj.weight", "text_projection",
              "token_embedding.weight", "logit_scale"):
        assert torch.equal(back[k].cpu(), sd[k]), k


def test_vith14_at_378_px_is_refused_at_construction():
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    with pytest.raises(ValueError, match=r"head dim 80 at 730 tokens.*up to 320 tokens"):
        net.SpatialClipNet("ViT-H-14-gene", None, n_genes=N_GENES, force_image_size=378)
    bad = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(224, 16, 176, 2, 88), text=None, gene=mc.GeneCfg(64, 32))
    with pytest.raises(ValueError, match=r"head dim 88.*32 / 64 / 80"):
        net.SpatialClipNet("custom", None, model_cfg=bad)


def test_train_entry_vith14_experiment(monkeypatch, tmp_path):
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    data, graph, losses, mc, module, net, optim, parity = _pkg()
    from spatial_clip_amd import train
    metrics = train.main(["experiment=vith14_gene_b128", "data.batch_size=8", "data.n_genes=2000",
                          "data.steps_per_epoch=2", "data.val_steps=1", "trainer.max_steps=2",
                          "trainer.log_every_n_steps=1", "test=False"])
    assert "train/loss" in metrics and np.isfinite(float(metrics["train/loss"])), metrics
    assert "val/loss" in metrics and np.isfinite(float(metrics["val/loss"])), metrics
