"""Average-pooled / no-ln_pre vision towers and the text tower's pooling options through the HIP towers, end to end.

Geometries, batch, losses and bounds of tests/test_gpu_model.py::test_forward_backward_vs_oracle: features 5e-3, loss 6e-3
(bf16 stream) / 4e-3 (fp32), every gradient within 4 % of its tensor's max-abs, against the fp32 oracle composition of
tests/_pool_oracle.py (held against the reference's own fixtures by tests/test_cpu_pool_config.py); then the reference's
fixtures themselves, the evaluation forwards, recomputation, checkpoints, the e4m3 path and the graphed step."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O
from tests import _pool_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLIPA = dict(pool_type="avg", no_ln_pre=True, final_ln_after_pool=True)
VARIANTS = {"clipa": CLIPA, "avg": dict(pool_type="avg"), "no_ln_pre": dict(no_ln_pre=True)}


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, ops, optim, patch_dropout as pd
    return data, graph, losses, mc, module, net, ops, optim, pd


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).cuda()


def tiny_cfgs(width, head_width, image, patch, flags, layers=2, embed=32, n_genes=100, hidden=64, mlp_ratio=4.0):
    *_, mc, _, _, _, _, _ = _pkg()
    cfg = mc.ModelCfg(embed_dim=embed, vision=mc.VisionCfg(image, patch, width, layers, head_width, mlp_ratio, **flags),
                      text=None, gene=mc.GeneCfg(n_genes, hidden))
    ocfg = O.ModelCfg(embed_dim=embed, vision=O.VisionCfg(image, patch, width, layers, head_width, mlp_ratio), text=None,
                      gene=O.GeneCfg(n_genes, hidden))
    return cfg, ocfg


def perturb(netobj, seed=11):
    """Make biases / LN affine non-trivial so that their gradients are exercised."""
    g = torch.Generator().manual_seed(seed)
    sd = netobj.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    netobj.load_state_dict(sd)


def _clip_loss(losses):
    return losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)


# Cases that miss the 4 % gradient bound, with the yardstick that replaces it there (as tests/test_gpu_patch_dropout.py does): the
# distance of the SAME oracle composition under torch.autocast(bfloat16) from the fp32 oracle; the bound becomes 1.5 x that
# distance (profiles/pool_towers_parity.txt).  Key: (variant, width, loss, stream, drop).
AUTOCAST_YARDSTICK = {}


def _bad_gradients(n, p, yardstick=None):
    bad = []
    for k in p:
        g_ref = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
        g = n.store.g(k).cpu()
        tol = max(0.04, 1.5 * (yardstick or {}).get(k, 0.0)) * float(g_ref.abs().max()) + 1e-6
        err = float((g - g_ref).abs().max())
        print(f"grad {k}: max|d| {err:.3e} of max|ref| {float(g_ref.abs().max()):.3e}")
        if err > tol:
            bad.append((k, err, float(g_ref.abs().max())))
    return bad


CASES = [(v, w, hw, im, pa, "clip", st, tol, None)
         for v in VARIANTS for (w, hw, im, pa) in ((64, 32, 32, 8), (128, 64, 48, 16)) for st, tol in (("bf16", 6e-3), ("fp32", 4e-3))]
CASES += [("clipa", 64, 32, 32, 8, "spatial", "bf16", 6e-3, None), ("clipa", 128, 64, 48, 16, "clip", "bf16", 6e-3, 0.5)]


@pytest.mark.parametrize("variant,width,head_width,image,patch,loss_kind,stream,loss_tol,drop", CASES)
def test_step_vs_oracle(variant, width, head_width, image, patch, loss_kind, stream, loss_tol, drop):
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    flags = VARIANTS[variant]
    cfg, ocfg = tiny_cfgs(width, head_width, image, patch, flags)
    B, seed = 12, 3
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, residual_stream=stream, force_patch_dropout=drop)
    assert n.vision.stack.cls_only_last is (flags.get("pool_type", "tok") == "tok")
    assert ("visual.ln_pre.weight" in n.state_dict()) is (not flags.get("no_ln_pre", False))
    perturb(n)
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    batch = data.synthetic_batch(B, image, cfg.gene.n_genes, K=4, step=0)
    keep, n_patch = None, cfg.vision.tokens - 1
    if drop:
        keep = pd.keep_indices_host(seed, 0, 0, B, n_patch, pd.num_keep(n_patch, drop))
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    f = PO.net_forward(batch["images"], batch["texts"], p, ocfg, keep=keep, **flags)
    if loss_kind == "clip":
        lo = O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"])
        loss_fn = _clip_loss(losses)
    else:
        lo = O.spatial_loss(f["image_features"], f["text_features"], f["logit_scale"], batch["image_tile_ids"],
                            batch["text_tile_ids"], batch["neighbor_tile_ids"], batch["neighbor_alphas"])
        loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0,
                                     temp_reg_weight=0.05, neighbor_alpha_scale=0.5, float32_logits=True)
    lo.backward()
    m = module.SpatialClipLitModule(n, loss_fn, None, None)
    out = m.model_step({k: v.cuda() for k, v in batch.items()})
    if drop:
        assert np.array_equal(n.vision.keep_idx.cpu().numpy(), keep) and n.vision.L_run == keep.shape[1] + 1
    df = float((out["image_features"].cpu() - f["image_features"].detach()).abs().max())
    dl = abs(float(out["loss"].detach()) - float(lo.detach()))
    print(f"features max|d| {df:.3e}; loss |d| {dl:.3e}")
    assert df < 5e-3
    assert (out["text_features"].cpu() - f["text_features"].detach()).abs().max() < 5e-3
    assert dl < loss_tol
    out["loss"].backward()
    torch.cuda.synchronize()
    bad = _bad_gradients(n, p, AUTOCAST_YARDSTICK.get((variant, width, loss_kind, stream, drop)))
    assert not bad, bad
    if drop:        # the positional rows of patches no sample kept: exact zeros
        for j in sorted(set(range(n_patch)) - set(keep.reshape(-1).tolist())):
            assert float(n.store.g("visual.positional_embedding")[1 + j].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the reference's fixtures
def _z(name):
    return np.load(os.path.join(GOLDEN, name))


def _load_weights(n, z):
    sd = {k: v.cpu() for k, v in n.state_dict().items()}
    names = [k[2:] for k in z.files if k.startswith("w.")]
    assert set(names) <= set(sd), set(names) - set(sd)
    assert {k for k in sd if not k.startswith("gene.") and k != "logit_scale"} <= set(names)
    for k in names:
        assert tuple(sd[k].shape) == z["w." + k].shape, k
        sd[k] = torch.from_numpy(z["w." + k])
    n.load_state_dict(sd)


def _fixture_gradients(n, zg):
    bad = []
    for k in zg.files:
        if not k.startswith("g."):
            continue
        g_ref, g = torch.from_numpy(zg[k]), n.store.g(k[2:]).cpu().reshape(zg[k].shape)
        err, top = float((g - g_ref).abs().max()), float(g_ref.abs().max())
        print(f"grad {k[2:]}: max|d| {err:.3e} of max|ref| {top:.3e}")
        if err > 0.04 * top + 1e-6:
            bad.append((k, err, top))
    return bad


@pytest.mark.parametrize("stream", ["bf16", "fp32"])
def test_reference_clipa_fixture_both_towers(stream):
    """The reference's tiny CLIP with the CLIPA vision AND text settings (text: pool 'last', no causal mask): features of both
    towers within 5e-3, every gradient of sum(f_img * t_img) + sum(f_txt * t_txt) within 4 % of its tensor's max-abs."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    z, zg = _z("clipa_tiny.npz"), _z("clipa_tiny_grads.npz")
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32, 2.0, **CLIPA),
                      text=mc.TextCfg(16, 97, 64, 2, 1, 4.0, "last", True), gene=None)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=0, residual_stream=stream)
    assert n.second.stack.causal is False and n.second.pool_type == "last"
    _load_weights(n, z)
    out = n(_dev(z["images"]), _dev(z["tokens"]))
    assert bool((n.second.bufs.get("eot", (6,), torch.int32) == 15).all())
    di = float((out["image_features"].cpu() - torch.from_numpy(z["image_features"])).abs().max())
    dt = float((out["text_features"].cpu() - torch.from_numpy(z["text_features"])).abs().max())
    print(f"features max|d|: image {di:.3e}, text {dt:.3e}")
    assert di < 5e-3 and dt < 5e-3
    ((out["image_features"] * _dev(z["target_image"])).sum() + (out["text_features"] * _dev(z["target_text"])).sum()).backward()
    torch.cuda.synchronize()
    bad = _fixture_gradients(n, zg)
    assert not bad, bad


@pytest.mark.parametrize("stream", ["bf16", "fp32"])
def test_reference_avg_only_fixture(stream):
    """The second reference tower: pool 'avg' alone (ln_pre kept, ln_post on every token before the pool)."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    z, za = _z("clipa_tiny.npz"), _z("clipa_tiny_avg.npz")
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32, 2.0, pool_type="avg"), text=None,
                      gene=mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=0, residual_stream=stream)
    _load_weights(n, za)
    texts = torch.randn(6, 200, generator=torch.Generator().manual_seed(1)).cuda()
    out = n(_dev(z["images"]), texts)
    df = float((out["image_features"].cpu() - torch.from_numpy(za["features"])).abs().max())
    print(f"features max|d| {df:.3e}")
    assert df < 5e-3
    (out["image_features"] * _dev(z["target_image"])).sum().backward()
    torch.cuda.synchronize()
    bad = _fixture_gradients(n, za)
    assert not bad, bad


@pytest.mark.parametrize("pool,causal", [("first", True), ("first", False), ("argmax", False)])
def test_text_pooling_options_vs_oracle(pool, causal):
    """The text pool types the fixture does not hold, against the oracle composition; 'first' under the causal mask sees only
    token 0, and a non-causal tower sends gradient to the positions behind the pooled one (the embedding backward must not
    skip them)."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=mc.TextCfg(16, 97, 64, 2, 2, 4.0, pool, not causal),
                      gene=None)
    ocfg = O.ModelCfg(embed_dim=32, vision=O.VisionCfg(32, 8, 64, 2, 32), text=O.TextCfg(16, 97, 64, 2, 2, 4.0), gene=None)
    B = 12
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=4)
    perturb(n)
    tokens = data.synthetic_captions(B, 16, 97, seed=0)
    images = data.synthetic_batch(B, 32, 100, K=4, step=0)["images"]
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in n.state_dict().items()}
    ft = PO.encode_text(tokens, p, ocfg, pool_type=pool, no_causal_mask=not causal)
    target = torch.randn(B, 32, generator=torch.Generator().manual_seed(2))
    (ft * target).sum().backward()
    out = n(images.cuda(), tokens.cuda())
    assert float((out["text_features"].cpu() - ft.detach()).abs().max()) < 5e-3
    (out["text_features"] * target.cuda()).sum().backward()
    torch.cuda.synchronize()
    text_keys = [k for k in p if not k.startswith("visual.") and k != "logit_scale"]
    bad = _bad_gradients(n, {k: p[k] for k in text_keys})
    assert not bad, bad
    g_pos = n.store.g("positional_embedding")
    if causal and pool == "first":
        assert float(g_pos[1:].abs().max()) == 0.0
    else:
        assert float(g_pos[1:].abs().max()) > 0.0 and float(g_pos[-1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ modes
def _cfg(flags=CLIPA, **kw):
    *_, mc, _, _, _, _, _ = _pkg()
    return mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32, **flags), text=None, gene=mc.GeneCfg(200, 64), **kw)


def _batch(B=12, step=0):
    data, *_ = _pkg()
    return {k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=step).items()}


def test_evaluation_forwards_agree_with_the_training_forward():
    *_, net, _, _, _ = _pkg()
    b = _batch()
    n = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3)
    perturb(n)
    want = n(b["images"], b["texts"])["image_features"].detach().clone()
    raw = n.vision.raw_features().clone()
    with torch.no_grad():
        assert torch.equal(n(b["images"], b["texts"])["image_features"], want)
    assert torch.equal(n.model.encode_image(b["images"], normalize=True), want)
    assert torch.equal(n.model.encode_image(b["images"]), raw)
    n.eval()
    assert torch.equal(n(b["images"], b["texts"])["image_features"], want)
    # with patch dropout the evaluation forwards run all tokens: the bits of the net without it
    n5 = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3, force_patch_dropout=0.5)
    perturb(n5)
    dropped = n5(b["images"], b["texts"])["image_features"]
    assert n5.vision.L_run == 9 and not torch.equal(dropped, want)
    assert torch.equal(n5.model.encode_image(b["images"], normalize=True), want)
    with torch.no_grad():
        assert torch.equal(n5(b["images"], b["texts"])["image_features"], want)


@pytest.mark.parametrize("variant", ["clipa", "avg"])
def test_grad_checkpointing_is_bit_identical(variant):
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    b = _batch()
    got = []
    for rc in (False, True):
        n = net.SpatialClipNet("custom", None, model_cfg=_cfg(VARIANTS[variant]), seed=3, grad_checkpointing=rc)
        perturb(n)
        m = module.SpatialClipLitModule(n, _clip_loss(losses), None, None)
        out = m.model_step(b)
        out["loss"].backward()
        torch.cuda.synchronize()
        got.append((out["image_features"].detach().clone(), {k: n.store.g(k).clone() for k in n.state_dict()}))
    assert torch.equal(got[0][0], got[1][0])
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k


def test_checkpoint_round_trip_keeps_the_reference_layout():
    *_, net, _, _, _ = _pkg()
    b = _batch()
    n = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3)
    perturb(n)
    sd = n.state_dict()
    assert not any("ln_pre" in k for k in sd) and "visual.ln_post.weight" in sd
    assert sorted(n.vision.param_names_stem()) == ["visual.class_embedding", "visual.conv1.weight", "visual.positional_embedding"]
    with torch.no_grad():
        want = n(b["images"], b["texts"])["image_features"].clone()
    n2 = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=99)
    n2.load_state_dict({k: v.cpu() for k, v in sd.items()})
    n3 = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=98)
    n3.load_checkpoint_state_dict({"state_dict": {"net.model." + k: v.cpu() for k, v in sd.items()}})
    with torch.no_grad():
        assert torch.equal(n2(b["images"], b["texts"])["image_features"], want)
        assert torch.equal(n3(b["images"], b["texts"])["image_features"], want)
    assert list(n2.state_dict()) == list(sd)
    # a state_dict WITH ln_pre (a 'tok' / ln_pre checkpoint) does not load into the no_ln_pre net under strict=True, nor the reverse
    with_ln = net.SpatialClipNet("custom", None, model_cfg=_cfg({}), seed=3).state_dict()
    assert "visual.ln_pre.weight" in with_ln
    with pytest.raises(KeyError, match="ln_pre"):
        n2.load_state_dict({k: v.cpu() for k, v in with_ln.items()}, strict=True)
    with pytest.raises(KeyError, match="ln_pre"):
        net.SpatialClipNet("custom", None, model_cfg=_cfg({}), seed=3).load_state_dict({k: v.cpu() for k, v in sd.items()})


def test_e4m3_path_within_its_stated_bounds():
    """precision="fp8" with the CLIPA tower: geometry and bounds of tests/test_gpu_patch_dropout.py::
    test_e4m3_path_drops_patches_within_its_stated_bounds without dropout (width 256, B = 128, 17 tokens = 17 K tiles of 128, so
    the e4m3 MLP weight gradients run in every block, the full-width last one included): second step at lr = 0 against the fp32
    oracle, loss 1e-2, features 4e-2, gradients 35 % of max-abs."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 256, 3, 64, **CLIPA), text=None, gene=mc.GeneCfg(200, 64))
    ocfg = O.ModelCfg(embed_dim=64, vision=O.VisionCfg(32, 8, 256, 3, 64), text=None, gene=O.GeneCfg(200, 64))
    B = 128
    batch = data.synthetic_batch(B, 32, 200, K=4, step=0)
    db = {k: v.cuda() for k, v in batch.items()}
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=9, precision="fp8")
    m = module.SpatialClipLitModule(n, _clip_loss(losses), None, None)
    for _ in range(2):
        out = m.model_step(db)
        out["loss"].backward()
    torch.cuda.synchronize()
    assert n.vision.L_run == 17 and n.vision.stack.fwd.w8 and not n.vision.stack.cls_only_last
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in n.state_dict().items()}
    f = PO.net_forward(batch["images"], batch["texts"], p, ocfg, **CLIPA)
    lo = O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"])
    lo.backward()
    dl = abs(float(out["loss"].detach()) - float(lo.detach()))
    df = float((out["image_features"].detach().cpu() - f["image_features"].detach()).abs().max())
    worst = max((float((n.store.g(k).cpu() - p[k].grad).abs().max() / p[k].grad.abs().max()), k)
                for k in p if p[k].grad is not None and float(p[k].grad.abs().max()) > 0)
    print(f"[fp8 + CLIPA tower] |d loss| {dl:.2e}, max|d feature| {df:.2e}, worst gradient {worst[0]:.3f} ({worst[1]})")
    assert dl < 1e-2 and df < 4e-2 and worst[0] < 0.35


def _trainable(cfg, seed=3):
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    m = module.SpatialClipLitModule(
        n, _clip_loss(losses), functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=3))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = 40, None, 40
    m.trainer = T()
    oc = m.configure_optimizers()
    return n, m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def test_graphed_step_replays_the_eager_bits(monkeypatch):
    """A CLIPA gene net is capturable (no host synchronisation, no per-step host argument in the new head), and three replayed
    steps are bit-identical to three eager ones (tests/test_gpu_graph.py::test_graph_replay_is_bit_identical_to_the_eager_step)."""
    data, graph, *_ = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    steps = 4
    batches = [_batch(24, s) for s in range(steps)]
    res = {}
    for mode in ("eager", "graph"):
        n, m, opt, sched = _trainable(_cfg())
        step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        assert step.capturable() is None
        ls = []
        for b in batches:
            loss = step.eager(b) if mode == "eager" else step(b)
            sched.step()
            ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        res[mode] = dict(loss=ls, w=n.store.master.detach().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                         replays=step.replays, failed=step.failed)
    assert res["graph"]["failed"] is None, res["graph"]["failed"]
    assert res["graph"]["replays"] == steps - 1 and res["eager"]["replays"] == 0
    assert res["eager"]["loss"] == res["graph"]["loss"], (res["eager"]["loss"], res["graph"]["loss"])
    for k in ("w", "m", "v"):
        assert torch.equal(res["eager"][k], res["graph"][k]), f"{k}: graph replay differs from the eager step"


# ------------------------------------------------------------------------------------------------ the public surface
def test_overrides_reach_the_towers_and_refused_keys_raise():
    *_, mc, _, net, _, _, _ = _pkg()
    kw = dict(n_genes=200, gene_hidden=64)
    base = dict(image_size=32, patch_size=8, width=64, layers=2, head_width=32)
    n = net.SpatialClipNet("ViT-B-16-gene", None, vision_cfg=dict(base, **CLIPA), **kw)
    v = n.vision
    assert (v.pool_type, v.no_ln_pre, v.final_ln_after_pool, v.stack.cls_only_last, v.L) == ("avg", True, True, False, 17)
    # force_image_size / force_patch_dropout keep the last word
    n = net.SpatialClipNet("ViT-B-16-gene", None, vision_cfg=dict(base, patch_dropout=0.25), force_image_size=48,
                           force_patch_dropout=0.5, **kw)
    assert n.cfg.vision.image_size == 48 and n.cfg.vision.patch_dropout == 0.5 and n.vision.stack.cls_only_last is True
    for key, value in (("ls_init_value", 1e-5), ("attentional_pool", True), ("pool_type", "none"), ("timm_model_name", "x"),
                       ("pos_embed_type", "rope"), ("output_tokens", True), ("bogus", 1)):
        with pytest.raises(ValueError, match=key):
            net.SpatialClipNet("ViT-B-16-gene", None, vision_cfg=dict(base, **{key: value}), **kw)
    with pytest.raises(ValueError, match="text_cfg"):
        net.SpatialClipNet("ViT-B-16-gene", None, vision_cfg=base, text_cfg={"pool_type": "last"}, **kw)
    text = dict(context_length=16, vocab_size=97, width=64, heads=2, layers=1, pool_type="last", no_causal_mask=True)
    for key, value in (("hf_model_name", "roberta-base"), ("embed_cls", True), ("ls_init_value", 0.1), ("bogus", 1)):
        with pytest.raises(ValueError, match=key):
            net.SpatialClipNet("ViT-B-16", None, vision_cfg=base, text_cfg=dict(text, **{key: value}))
    # a tower configured for another tokenizer passes token ids through and refuses strings, naming the tokenizer
    n = net.SpatialClipNet("ViT-B-16", None, vision_cfg=base,
                           text_cfg=dict(text, hf_tokenizer_name="bert-base-uncased", tokenizer_kwargs={"strip_sep_token": True}))
    assert n.second.stack.causal is False and n.second.pool_type == "last" and n.second.L == 16
    ids = torch.arange(32).view(2, 16) % 97
    assert torch.equal(n.tokenizer(ids), ids) and n.tokenizer(ids.tolist()).dtype == torch.int64
    for s in ("a tile of tissue", ["one", "two"]):
        with pytest.raises(ValueError, match="bert-base-uncased"):
            n.tokenizer(s)


def test_default_config_takes_the_old_path_and_gives_its_bits():
    """No new field set: the class-token-only last block, ln_pre in the layout, and -- on a fixed seed and batch -- the bits
    the tower gave before these fields existed (tests/golden/pool_default_path_bits.npz, recorded on an MI355X from the
    commit in front of this feature)."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    z = _z("pool_default_path_bits.npz")
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(100, 64))
    for stream in ("bf16", "fp32"):
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3, residual_stream=stream)
        assert n.vision.stack.cls_only_last is True and n.vision.pool_type == "tok" and not n.vision.no_ln_pre
        assert "visual.ln_pre.weight" in n.state_dict()
        perturb(n)
        batch = data.synthetic_batch(12, 32, 100, K=4, step=0)
        out = n(batch["images"].cuda(), batch["texts"].cuda())
        assert np.array_equal(out["image_features"].detach().cpu().numpy(), z[f"image_features.{stream}"])
        (out["image_features"] * _dev(z["target"])).sum().backward()
        torch.cuda.synchronize()
        for k in ("visual.conv1.weight", "visual.ln_pre.weight", "visual.positional_embedding", "visual.ln_post.bias"):
            assert np.array_equal(n.store.g(k).cpu().numpy(), z[f"g.{stream}.{k}"]), k
