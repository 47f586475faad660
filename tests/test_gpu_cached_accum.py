"""Cached-feature gradient accumulation on the device (Trainer accum_freq; open_clip's --accum-freq):
the group step against the reference's own run at batch N * B (tests/golden/make_golden_cached_accum.py), the logit_scale
gradient counted once, SpatialLoss neighbours across micro-batches, exact replay of the patch-dropout draws, the cached and
the plain route of this build side by side against the fp32 oracle, activation memory, and the Trainer's loop.

Bounds.  Losses, gradient norms and post-step parameters: the rule and constants of test_gpu_grad_accum.py for this model and
these batches, ``max(constant, 1.5 x what the reference's own bf16 autocast run deviates by)`` with 4e-3 / 2e-2 (loss before /
after the first optimiser step), 0.05 (relative gradient norm), 3e-3 (parameter, max-abs).  Gradient tensors, which that file
does not bound: the same rule with test_gpu_model.py's gradient constant, 4 % of the reference tensor's max-abs."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O

pytestmark = pytest.mark.gpu

BOUNDED = ("visual.proj", "text_projection", "token_embedding.weight", "visual.conv1.weight")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, model_configs as mc, module, net, ops, optim, streams
    return data, losses, mc, module, net, ops, optim, streams


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}


def _p0_digest(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    h = hashlib.sha256()
    for k in sorted(k for k in z.files if k.startswith("p0.")):
        h.update(k.encode())
        h.update(np.ascontiguousarray(z[k]).tobytes())
    return h.hexdigest()


def _tiny_text_net(golden_dir):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    z = _load(golden_dir, "train3_tiny_text.npz")
    c = json.loads(str(z["cfg"]))
    v, t = c["vision_cfg"], c["text_cfg"]
    cfg = mc.ModelCfg(embed_dim=c["embed_dim"],
                      vision=mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64)),
                      text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg)
    n.load_state_dict({k[3:]: val for k, val in z.items() if k.startswith("p0.")})
    return n, cfg


def _module(n, loss_fn, warmup=2, total=10):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _grad_bound(ref, ac):
    """Gradient tensors (module docstring): max(4 % of the reference tensor's max-abs, 1.5 x the autocast run's distance)."""
    return max(0.04 * float(ref.abs().max()) + 1e-6, 1.5 * float((ac - ref).abs().max()))


def _golden(golden_dir):
    z = _load(golden_dir, "cached_accum_tiny_text.npz")
    assert int(z["accum_freq"]) == 2 and int(z["micro_batch"]) == 6 and str(z["p0_from"]) == "train3_tiny_text.npz"
    assert _p0_digest(golden_dir, "train3_tiny_text.npz") == str(z["p0_sha256"]), \
        "train3_tiny_text.npz no longer holds the starting weights this fixture was generated from: regenerate it too"
    batches = _load(golden_dir, str(z["batches_from"]))
    micro = [{"images": batches[f"b{i}.images"].cuda(), "texts": batches[f"b{i}.texts"].cuda()} for i in range(4)]
    return z, micro


# ---------------------------------------------------------------------------------------------- the reference's G-batch run
@pytest.fixture(scope="module")
def clip_run(golden_dir):
    """cached_group_step + FusedAdamW + scheduler over the fixture's two groups of 2 x 6, shared (and left unchanged)."""
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    z, micro = _golden(golden_dir)
    n, _ = _tiny_text_net(golden_dir)
    m, opt, sched = _module(n, losses.ClipLoss(), warmup=int(z["warmup"]), total=int(z["total"]))
    assert hasattr(m, "cached_group_step"), "this build has no cached-feature group step"
    acc = m.group_accumulator(2)
    out = {"losses": [], "norms": [], "post": [], "z": z}
    for s in range(2):
        partial = acc.sumsq_partial()
        loss = m.cached_group_step(micro[2 * s:2 * s + 2], partial=partial)
        if s == 0:
            torch.cuda.synchronize()
            out["g0"] = {k: n.store.g(k).detach().cpu().clone() for k in BOUNDED + ("logit_scale",)}
        with streams.chain_stream():
            nc = opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
        sched.step()
        n.store.wait_all()
        torch.cuda.synchronize()
        out["losses"].append(float(loss.detach()))
        out["norms"].append(float(nc[0]))
        out["post"].append({k: n.store.p(k).detach().cpu().clone() for k in BOUNDED})
    out["opt"], out["sched"] = opt, sched
    return out


def test_parity_with_the_reference_at_batch_12(clip_run):
    """Two optimiser steps at G = 12 from four micro-batches of 6 against the reference's own classes in fp32 at batch 12.
    Fails on a build without the feature (and, by the fixture's record (c), on one that sums two 6-pair losses instead).

    Measured on an MI355X, this build / the autocast yardstick: see DESIGN.md section 4o."""
    z = clip_run["z"]
    assert clip_run["opt"].step_count == 2 and clip_run["sched"].last_epoch == 2
    fails = []
    for s in range(2):
        ref, ac = float(z["losses"][s]), float(z["autocast_losses"][s])
        bound = max(4e-3 if s == 0 else 2e-2, 1.5 * abs(ac - ref))
        d = abs(clip_run["losses"][s] - ref)
        print(f"  loss[{s}] {clip_run['losses'][s]:.6f} ref {ref:.6f} |d| {d:.3g} autocast |d| {abs(ac - ref):.3g} bound {bound:.3g}")
        if d > bound:
            fails.append(("loss", s, d, bound))
        ref, ac = float(z["grad_norms"][s]), float(z["autocast_grad_norms"][s])
        bound = max(0.05, 1.5 * abs(ac - ref) / ref)
        d = abs(clip_run["norms"][s] - ref) / ref
        print(f"  grad_norm[{s}] {clip_run['norms'][s]:.5f} ref {ref:.5f} rel {d:.3g} autocast rel {abs(ac - ref) / ref:.3g} "
              f"bound {bound:.3g}")
        if d > bound:
            fails.append(("grad_norm", s, d, bound))
        for k in BOUNDED:
            ac_dev = float((z[f"autocast_p{s}." + k] - z[f"p{s}." + k]).abs().max())
            bound = max(3e-3, 1.5 * ac_dev)
            d = float((clip_run["post"][s][k] - z[f"p{s}." + k]).abs().max())
            print(f"  step {s} {k}: max|d| {d:.3g} autocast max|d| {ac_dev:.3g} bound {bound:.3g}")
            if d > bound:
                fails.append((k, s, d, bound))
    for k in BOUNDED:       # the step-0 gradients, before the clip
        bound = _grad_bound(z["g0." + k], z["autocast_g0." + k])
        d = float((clip_run["g0"][k] - z["g0." + k]).abs().max())
        print(f"  step-0 gradient {k}: max|d| {d:.3g} of max|g| {float(z['g0.' + k].abs().max()):.3g} bound {bound:.3g}")
        if d > bound:
            fails.append(("g0." + k, d, bound))
    assert not fails, fails
    # the fixture's record (c): Lightning's accumulate_grad_batches=2 on the same micro-batches misses these bounds twice over
    for s in range(2):
        for q in (f"loss{s}", f"grad_norm{s}"):
            d, b = (float(x) for x in z["sep." + q])
            assert d >= 2.0 * b


def test_logit_scale_gradient_is_counted_once(clip_run):
    """open_clip's loop backpropagates the full-batch loss N times, so ``logit_scale`` gets N times its gradient (the fixture's
    record (b): asserted there with the reference's own code); this build applies the gradient of the G-pair loss."""
    z = clip_run["z"]
    ref, ac, loop = float(z["g0.logit_scale"]), float(z["autocast_g0.logit_scale"]), float(z["g0_loop.logit_scale"])
    assert abs(loop - 2.0 * ref) <= 2e-5 * abs(loop)
    got = float(clip_run["g0"]["logit_scale"])
    bound = _grad_bound(z["g0.logit_scale"], z["autocast_g0.logit_scale"])
    print(f"  d logit_scale {got:.6f}: reference at batch 12 {ref:.6f} (autocast {ac:.6f}), open_clip's loop {loop:.6f}; bound {bound:.3g}")
    assert abs(got - ref) <= bound
    assert abs(got - ref) < abs(got - loop)


# ---------------------------------------------------------------------------------------------- SpatialLoss across micro-batches
def test_spatial_neighbours_in_the_other_micro_batch_get_their_weight(golden_dir):
    """Record (d): 12 unique tile ids; every row names a neighbour in the OTHER micro-batch, one in its own, one in neither;
    one alpha <= 0.  The reference's SpatialLoss at batch 12 is the expected value."""
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    z, micro = _golden(golden_dir)
    n, _ = _tiny_text_net(golden_dir)
    loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                 neighbor_alpha_scale=0.5, float32_logits=True)
    m, _, _ = _module(n, loss_fn)
    group = []
    for j in range(2):
        r = slice(6 * j, 6 * j + 6)
        group.append({**micro[j], "image_tile_ids": z["sp.ids"][r].cuda(), "text_tile_ids": z["sp.ids"][r].clone().cuda(),
                      "neighbor_tile_ids": z["sp.nb"][r].cuda(), "neighbor_alphas": z["sp.alpha"][r].cuda()})
    loss = float(m.cached_group_step(group).detach())
    torch.cuda.synchronize()
    ref, ac = float(z["sp.loss"]), float(z["sp.autocast_loss"])
    bound = max(4e-3, 1.5 * abs(ac - ref))
    print(f"  spatial group loss {loss:.6f} ref {ref:.6f} |d| {abs(loss - ref):.3g} autocast |d| {abs(ac - ref):.3g} bound {bound:.3g}")
    fails = [] if abs(loss - ref) <= bound else [("loss", abs(loss - ref), bound)]
    for k in ("visual.proj", "text_projection", "logit_scale"):
        b = _grad_bound(z["sp.g0." + k], z["sp.autocast_g0." + k])
        d = float((n.store.g(k).detach().cpu() - z["sp.g0." + k]).abs().max())
        print(f"  step-0 gradient {k}: max|d| {d:.3g} of max|g| {float(z['sp.g0.' + k].abs().max()):.3g} bound {b:.3g}")
        if d > b:
            fails.append((k, d, b))
    assert not fails, fails
    # the same build on each micro-batch alone: neighbours in the other micro-batch are lost, 5 negatives instead of 11
    alone = []
    with torch.no_grad():
        for b in group:
            alone.append(float(m.model_step(b)["loss"].detach()))
    mean = sum(alone) / 2
    print(f"  per-micro-batch losses {alone} (reference {[float(x) for x in z['sp.micro_losses']]}): mean {mean:.6f}")
    assert abs(loss - mean) > bound and abs(float(z["sp.micro_losses"].mean()) - ref) >= 2.0 * bound


# ---------------------------------------------------------------------------------------------- replay
def _gene_cfg(mc, image=32, layers=2, bias=None, scale=None):
    kw = {} if bias is None else {"init_logit_bias": bias, "init_logit_scale": scale}
    return mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(image, 8, 64, layers, 32), text=None, gene=mc.GeneCfg(100, 64), **kw)


def _micro_batches(data, N, B, image=32, step=0):
    full = data.synthetic_batch(N * B, image, 100, K=4, step=step)
    return full, [{k: v[j * B:(j + 1) * B].cuda() for k, v in full.items()} for j in range(N)]


def test_phase_two_replays_the_cached_forward_exactly(monkeypatch):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    from spatial_clip_amd.patch_dropout import num_keep
    N, B = 3, 4
    n = net.SpatialClipNet("custom", None, model_cfg=_gene_cfg(mc), seed=3, force_patch_dropout=0.5)
    m = module.SpatialClipLitModule(n, losses.ClipLoss(), None, None)
    m.train()
    _, micro = _micro_batches(data, N, B)
    seen = {"image": [], "text": []}
    v_fwd, s_fwd = n.vision.forward, n.second.forward

    def vision(x):
        f = v_fwd(x)
        seen["image"].append((f.clone(), n.vision.keep_idx.clone(), n.vision.L_run))
        return f

    def second(x):
        f = s_fwd(x)
        seen["text"].append(f.clone())
        return f
    monkeypatch.setattr(n.vision, "forward", vision)
    monkeypatch.setattr(n.second, "forward", second)
    n.patch_dropout_draw = 7
    m.cached_group_step(micro)
    torch.cuda.synchronize()
    assert n.patch_dropout_draw == 7 + N, "the draw counter advances by N per group, not 2N"
    assert len(seen["image"]) == 2 * N and len(seen["text"]) == 2 * N
    K = num_keep(16, 0.5)
    cache = m._group_caches
    for j in range(N):
        (f1, keep1, L1), (f2, keep2, L2) = seen["image"][j], seen["image"][N + j]
        assert L1 == L2 == K + 1 and tuple(keep1.shape) == (B, K), "the caching pass must drop patches like a training forward"
        assert torch.equal(keep1, keep2), f"micro-batch {j}: phase 2 kept other patches than the caching pass"
        assert torch.equal(f1, f2) and torch.equal(seen["text"][j], seen["text"][N + j])
        assert torch.equal(cache["image"][j * B:(j + 1) * B], f2) and torch.equal(cache["text"][j * B:(j + 1) * B], seen["text"][N + j])
    assert not torch.equal(seen["image"][0][1], seen["image"][1][1]), "every micro-batch has a draw of its own"
    # a second group goes on from the counter, and an evaluation forward in between still keeps every patch
    with torch.no_grad():
        n(micro[0]["images"], micro[0]["texts"])
    assert seen["image"][-1][2] == 17 and n.patch_dropout_draw == 7 + N
    m.cached_group_step(micro)
    assert n.patch_dropout_draw == 7 + 2 * N


# ---------------------------------------------------------------------------------------------- same build, two routes
def _oracle_grads(kind, n, full, ocfg):
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    f = O.net_forward(full["images"], full["texts"], p, ocfg)
    if kind == "clip":
        lo = O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"])
    else:       # open_clip SigLipLoss, one process: -sum logsigmoid(labels * (s z + b)) / B, labels = 2 I - 1
        G = f["image_features"].shape[0]
        logits = f["logit_scale"] * f["image_features"] @ f["text_features"].t()
        if "logit_bias" in p:
            logits = logits + p["logit_bias"]
        labels = 2 * torch.eye(G) - 1
        lo = -torch.nn.functional.logsigmoid(labels * logits).sum() / G
    lo.backward()
    return float(lo.detach()), {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in params}


@pytest.mark.parametrize("kind", ["clip", "siglip"])
def test_cached_and_plain_route_agree_within_their_oracle_distances(kind):
    """N = 3, B = 4 (G = 12: no power of two, no tile multiple) on the tiny gene-MLP model OF test_gpu_model.py
    (``tiny_cfgs()``, seed 3, ``perturb``: the model whose gradient bound is used, with no parameter it does not have -- the
    sigmoid loss runs without a ``logit_bias``, as ``SigLipLoss.forward`` allows): the gradient the cached group leaves against
    the gradient of one plain step at batch 12, each inside test_gpu_model.py's bound of the fp32 oracle for every tensor (4 % of
    the tensor's max-abs), so that their distance obeys the triangle inequality; the cached route twice, bit for bit.

    Loss: test_gpu_model.py's 6e-3 for ClipLoss on this model.  That figure is for a cross-entropy, whose sensitivity to a logit
    error dx is sum_j p_j dx_j - dx_pos per row and direction: weights that sum to 2.  The sigmoid loss of one process is
    sum_ij softplus(-y_ij x_ij) / G, per row sum_j sigma_j dx_j: without a bias and at a random start sigma_j is about 1/2, the
    weights sum to G / 2 = 6.  The same logit noise therefore moves it G / 4 = 3 times as far: 1.8e-2 for [siglip].

    An earlier form of the [siglip] case built a model of its own (``init_logit_bias=-10``, ``init_logit_scale=ln 10``), which
    test_gpu_model.py never bounds; there d logit_scale, a sum that cancels to 10 x the mean positive cosine 0.0104, was 5.0 % off
    the oracle on the plain and the cached route alike (-0.099182 both, oracle -0.104390).  The bias route
    of the group step has a test of its own below, with an exact expectation.

    Measured on an MI355X.  [clip]: loss 4.2e-03 from the oracle on both routes, worst |cached - plain| 4.4e-07 of a tensor's
    max-abs, d logit_scale 0.518042 on both against 0.512386 (1.1 %).  [siglip]: loss 1.79e-02 from the oracle on both routes
    (10.926748 against 10.944684), worst |cached - plain| 1.9e-07, d logit_scale 4.107535 on both against 4.124864 (0.4 %)."""
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    N, B = 3, 4
    sig = kind == "siglip"
    from tests.test_gpu_model import perturb, tiny_cfgs
    cfg, ocfg = tiny_cfgs()
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
    perturb(n)
    assert not n.has_logit_bias
    loss_fn = losses.SigLipLoss() if sig else losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    m = module.SpatialClipLitModule(n, loss_fn, None, None)
    full, micro = _micro_batches(data, N, B)
    lo, g_ref = _oracle_grads(kind, n, full, ocfg)

    def cached():
        loss = m.cached_group_step(micro)
        torch.cuda.synchronize()
        return float(loss.detach()), n.store.grad.detach().clone()

    l_c, flat_c = cached()
    g_c = {k: n.store.g(k).detach().cpu().clone() for k in g_ref}
    l_c2, flat_c2 = cached()
    assert l_c == l_c2 and torch.equal(flat_c, flat_c2), "the cached route is not bit-identical to itself"
    with streams.chain_stream():
        loss = m.training_step({k: v.cuda() for k, v in full.items()}, 0)
        loss.backward(m.root_gradient(loss))
    torch.cuda.synchronize()
    l_p = float(loss.detach())
    g_p = {k: n.store.g(k).detach().cpu().clone() for k in g_ref}
    print(f"  loss: oracle {lo:.6f} cached {l_c:.6f} plain {l_p:.6f}")
    loss_tol = 6e-3 * (N * B / 4 if sig else 1)
    assert abs(l_c - lo) < loss_tol and abs(l_p - lo) < loss_tol
    bad = []
    for k, ref in g_ref.items():
        tol = 0.04 * float(ref.abs().max()) + 1e-6
        d_c, d_p = float((g_c[k] - ref).abs().max()), float((g_p[k] - ref).abs().max())
        d_cp = float((g_c[k] - g_p[k]).abs().max())
        if d_c > tol or d_p > tol or d_cp > d_c + d_p:
            bad.append((k, d_c, d_p, d_cp, tol))
    worst = max((float((g_c[k] - g_p[k]).abs().max()) / (float(g_ref[k].abs().max()) + 1e-12)) for k in g_ref)
    print(f"  worst |cached - plain| / max|oracle| over the tensors: {worst:.3g}")
    # a figure, not an assertion: d logit_scale by the oracle's fp32 loss formula on THIS build's features (what the head is
    # given), beside the oracle's own -- it tells the towers' bf16 feature noise from an error of the head
    ls = n.store.p("logit_scale").detach().cpu().clone().requires_grad_(True)
    fi, ft = n.vision.f.detach().cpu(), n.second.f.detach().cpu()
    if sig:
        x = ls.exp() * fi @ ft.t()
        (-torch.nn.functional.logsigmoid((2 * torch.eye(N * B) - 1) * x).sum() / (N * B)).backward()
    else:
        O.clip_loss(fi, ft, ls.exp()).backward()
    print(f"  d logit_scale: oracle {float(g_ref['logit_scale']):.6f} cached {float(g_c['logit_scale']):.6f} plain "
          f"{float(g_p['logit_scale']):.6f}; fp32 formula on this build's features {float(ls.grad):.6f}")
    assert not bad, bad


def test_logit_scale_and_bias_take_the_group_gradient_on_one_micro_batch():
    """A net with a ``logit_bias`` (SigLIP's start point: bias -10, scale 10), N = 3: after the group step the flat gradient
    holds the head's d_bias bit for bit -- micro-batch 0 writes 1.0 * d_bias, the folds add the exact zeros of the other two --
    and d_scale times the device's exp(logit_scale) (the chain rule of the exponentiated scale; 4 ulp for the product), not N
    times either."""
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    N, B = 3, 4
    n = net.SpatialClipNet("custom", None, model_cfg=_gene_cfg(mc, bias=-10.0, scale=2.302585092994046), seed=3)
    m = module.SpatialClipLitModule(n, losses.SigLipLoss(), None, None)
    _, micro = _micro_batches(data, N, B)
    m.cached_group_step(micro)
    torch.cuda.synchronize()
    head = m.loss_fn.last
    d_b, d_s = head["d_bias"].detach().cpu(), head["d_scale"].detach().cpu()
    g_b, g_s = n.store.g("logit_bias").detach().cpu(), n.store.g("logit_scale").detach().cpu()
    assert float(d_b) != 0.0 and float(d_s) != 0.0
    assert torch.equal(g_b.reshape(()), d_b.reshape(())), (float(g_b), float(d_b))
    want = float(d_s.float() * n._scale.detach().cpu().reshape(()))      # fp32 product with the device's own exp(logit_scale)
    print(f"  d logit_bias {float(g_b):.8g} (head {float(d_b):.8g}); d logit_scale {float(g_s):.8g} (head x exp {want:.8g})")
    assert abs(float(g_s) - want) <= 4 * 2.0 ** -23 * abs(want)
    assert abs(float(g_s) - want) < abs(float(g_s) - N * want)


# ---------------------------------------------------------------------------------------------- memory
def test_activation_memory_is_one_micro_batch(monkeypatch):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    import gc
    monkeypatch.setenv("SC_OVERLAP", "0")
    N, B, image = 4, 8, 64
    L = (image // 8) ** 2 + 1
    full, micro = _micro_batches(data, N, B, image=image)

    def fresh():
        n = net.SpatialClipNet("custom", None, model_cfg=_gene_cfg(mc, image=image, layers=4), seed=3)
        return n, module.SpatialClipLitModule(n, losses.ClipLoss(), None, None)

    def peak(fn):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    big = {k: v.cuda() for k, v in full.items()}

    def plain_on(m):
        with streams.chain_stream():
            loss = m.training_step(big, 0)
            loss.backward(m.root_gradient(loss))

    # process-wide workspaces (split-K slabs, the streams' own) are allocated by whichever route runs first in the process and
    # kept: both routes once, unmeasured, on nets that are then dropped
    n, m = fresh()
    m.cached_group_step(micro)
    del n, m
    n, m = fresh()
    plain_on(m)
    del n, m
    n, m = fresh()
    cached = peak(lambda: m.cached_group_step(micro))
    bytes_cached = sum(o.bytes() for t in (n.vision, n.second) for o in (t.bufs, getattr(getattr(t, "stack", None), "bufs", None)) if o)
    rows = {}
    for name, tower in (("vision", n.vision), ("second", n.second)):
        for owner in (tower.bufs, getattr(getattr(tower, "stack", None), "bufs", None)):
            if owner is not None:
                for key, t in owner._b.items():
                    if t.dim() >= 2:
                        rows[f"{name}.{key}"] = t.shape[0]
    assert rows and max(rows.values()) <= B * L, {k: v for k, v in rows.items() if v > B * L}
    assert max(rows.values()) == B * L
    del n, m
    n, m = fresh()
    plain_peak = peak(lambda: plain_on(m))
    bytes_plain = sum(o.bytes() for t in (n.vision, n.second) for o in (t.bufs, getattr(getattr(t, "stack", None), "bufs", None)) if o)
    print(f"  peak device memory above the resident weights: cached group 4 x 8 {cached / 2**20:.2f} MiB, plain step at 32 "
          f"{plain_peak / 2**20:.2f} MiB; tower buffers {bytes_cached / 2**20:.2f} / {bytes_plain / 2**20:.2f} MiB")
    assert cached < plain_peak


# ---------------------------------------------------------------------------------------------- Trainer
def _dm(data):
    class TextDM(data.SyntheticSpatialDataModule):
        def _loader(self, n, offset):
            for s in range(n):
                b = data.synthetic_batch(self.batch_size, self.image_size, 64, self.k_neighbors, offset + s)
                b["texts"] = data.synthetic_captions(self.batch_size, 16, 97, seed=offset + s)
                yield b
    return TextDM(batch_size=8, image_size=32, n_genes=64, k_neighbors=4, steps_per_epoch=5, val_steps=1)


def _trainer_module(seed=5):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=mc.TextCfg(16, 97, 64, 2, 2), gene=None)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    m = module.SpatialClipLitModule(
        n, losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                              neighbor_alpha_scale=0.5, float32_logits=True),
        functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2))
    return n, m


def _fit(ckpt_path=None, max_epochs=1, **kw):
    data, *_ = _pkg()
    from spatial_clip_amd.trainer import Trainer
    n, m = _trainer_module()
    tr = Trainer(max_epochs=max_epochs, gradient_clip_val=1.0, log_every_n_steps=1, **kw)
    tr.fit(m, _dm(data), ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    return n, m, tr


def test_trainer_steps_once_per_group_and_drops_the_tail(monkeypatch):
    monkeypatch.setenv("SC_GRAPH", "1")         # asks for a captured step: a cached group stays eager
    calls = []
    n, m, tr = None, None, None
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    orig = module.SpatialClipLitModule.cached_group_step

    def counted(self, batches, partial=None):
        calls.append(len(batches))
        return orig(self, batches, partial=partial)
    monkeypatch.setattr(module.SpatialClipLitModule, "cached_group_step", counted)
    n, m, tr = _fit(accum_freq=2, callbacks={"weight_averaging": {"decay": 0.5}})
    assert calls == [2, 2], "5 batches at accum_freq=2: two groups, the fifth batch is dropped"
    assert tr.global_step == 2 and tr.optimizer.step_count == 2 and tr.scheduler.last_epoch == 2
    assert tr.estimated_stepping_batches == 2 and tr.graphed_step is None
    assert tr.accumulator is not None and tr.accumulator.scale == 1.0 and tr.accumulator.every == 2
    recs = [h for h in tr.history if "train/loss" in h and "epoch" not in h]
    assert [h["step"] for h in recs] == [1, 2]
    assert tr.weight_averager.n_averaged == 2 and tr.weight_averager.latest_update_step == 1    # once per optimiser step
    epoch = [h for h in tr.history if "epoch" in h][-1]
    assert "train/R@1" in epoch
    assert m.train_metrics.total == 2 * 16, "the train metrics see each group's 16 x 16 block once"


def test_trainer_accum_freq_one_is_the_plain_loop(monkeypatch):
    monkeypatch.setenv("SC_GRAPH", "0")
    n0, _, tr0 = _fit()
    n1, m1, tr1 = _fit(accum_freq=1)
    assert tr0.global_step == tr1.global_step == 5 and tr1.estimated_stepping_batches == 5
    assert torch.equal(n0.store.master.detach(), n1.store.master.detach())
    assert tr1.accumulator is None and getattr(m1, "_group_caches", None) is None and getattr(m1, "_group_accum", None) is None
    n2, _, tr2 = _fit(accum_freq=2)
    assert tr2.global_step == 2 and not torch.equal(n2.store.master.detach(), n1.store.master.detach())


def test_trainer_resumes_from_the_epoch_end_checkpoint(tmp_path):
    """Two epochs uninterrupted against one epoch, its epoch-end checkpoint, and a second run resumed from it.  The first
    leg's cosine schedule is sized for 2 steps and the uninterrupted run's for 4; both of the first leg's steps fall inside
    the 2-step warm-up, where the learning rate is step / warm-up and the total does not enter."""
    n, _, tr = _fit(accum_freq=2, max_epochs=2)
    assert tr.global_step == 4 and tr.optimizer.step_count == 4 and tr.scheduler.last_epoch == 4
    w = n.store.master.detach().clone()
    _, _, tr1 = _fit(accum_freq=2, max_epochs=1, enable_checkpointing=True, default_root_dir=str(tmp_path))
    assert tr1.global_step == 2
    last = tr1.checkpoint_callback.last_model_path
    assert os.path.isfile(last) and int(torch.load(last, map_location="cpu", weights_only=False)["global_step"]) == 2
    n2, _, tr2 = _fit(ckpt_path=last, accum_freq=2, max_epochs=2)
    assert tr2.global_step == 4 and tr2.optimizer.step_count == 4 and tr2.scheduler.last_epoch == 4
    assert torch.equal(n2.store.master.detach(), w)
