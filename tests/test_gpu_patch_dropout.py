"""FLIP patch dropout on the device: the selection kernel against its host restatement, the three ``keep`` stem kernels against
the full-length kernels they must agree with bit for bit, the dropping training step against the fp32 oracle and against the
reference's own PatchDropout (tests/golden/patch_dropout_tiny.npz), and the modes around it (evaluation, recomputation, the
graphed step, checkpoints)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O
from tests import _patchdrop_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_dropout_tiny.npz")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, ops, optim, patch_dropout as pd
    return data, graph, losses, mc, module, net, ops, optim, pd


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).cuda()


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("B,n,K", [(1, 4, 1), (3, 16, 8), (2, 49, 24), (5, 196, 98), (2, 196, 49), (7, 196, 195), (1, 576, 144),
                                   (2, 1024, 256)])
def test_patch_keep_kernel_equals_the_host_function(B, n, K):
    *_, ops, _, pd = _pkg()
    for seed, draw, sample0 in ((0, 0, 0), (3, 17, 5 * B), (0xFFFFFFF0, 2 ** 31 + 5, 0xFFFFFFFF)):
        keep, slot = ops.patch_keep(seed, draw, sample0, B, n, K)
        want = pd.keep_indices_host(seed, draw, sample0, B, n, K)
        assert np.array_equal(keep.cpu().numpy(), want)
        assert np.array_equal(slot.cpu().numpy(), pd.slots_from_keep(want, n))


# ------------------------------------------------------------------------------------------------ im2col
@pytest.mark.parametrize("P,S", [(8, 32), (14, 56), (16, 64), (32, 96)])
def test_im2col_keep_equals_the_kept_rows_of_the_full_im2col(P, S):
    *_, ops, _, pd = _pkg()
    B, G_ = 3, S // P
    n, kp = G_ * G_, 3 * P * P
    kpad = (kp + 63) // 64 * 64
    img = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(P)).cuda()
    full = torch.zeros(B * n, kpad, dtype=torch.bfloat16, device="cuda")
    ops.im2col(img, full, P)
    for K in (1, 7, n - 1):
        keep = pd.keep_indices_host(P, K, 0, B, n, K)
        got = torch.full((B * K, kpad), 5.0, dtype=torch.bfloat16, device="cuda")
        ops.im2col(img, got, P, keep=_dev(keep))
        rows = (torch.arange(B)[:, None] * n + torch.from_numpy(keep).long()).reshape(-1).cuda()
        assert torch.equal(got[:, :kp], full[rows, :kp])
        assert bool((got[:, kp:] == 5.0).all())                 # the K padding is not touched


# ------------------------------------------------------------------------------------------------ embedding forward
@pytest.mark.parametrize("d", [64, 192, 768, 1280, 2048])
@pytest.mark.parametrize("Lk", [2, 9, 50])
@pytest.mark.parametrize("x16", [False, True])
def test_embed_ln_fwd_keep_rows_are_the_full_kernels_rows(d, Lk, x16):
    *_, ops, _, pd = _pkg()
    B, n = 3, 60
    L, K = n + 1, Lk - 1
    g = torch.Generator().manual_seed(d + Lk)
    patch_out = torch.randn(B * n, d, generator=g).cuda()
    cls, pos = torch.randn(d, generator=g).cuda(), torch.randn(L, d, generator=g).cuda()
    gamma, beta = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    xd = torch.bfloat16 if x16 else torch.float32
    x = torch.empty(B * L, d, dtype=xd, device="cuda")
    mean, rstd = torch.empty(B * L, device="cuda"), torch.empty(B * L, device="cuda")
    ops.embed_ln_fwd(patch_out, cls, pos, gamma, beta, x, mean, rstd, B, L, d)
    keep = pd.keep_indices_host(d, Lk, 0, B, n, K)
    kl = torch.from_numpy(keep).long()
    prow = (torch.arange(B)[:, None] * n + kl).reshape(-1).cuda()                       # rows of patch_out
    trow = torch.cat([torch.arange(B)[:, None] * L, torch.arange(B)[:, None] * L + 1 + kl], 1).reshape(-1).cuda()   # token rows
    xk = torch.empty(B * Lk, d, dtype=xd, device="cuda")
    mk, rk = torch.empty(B * Lk, device="cuda"), torch.empty(B * Lk, device="cuda")
    ops.embed_ln_fwd(patch_out[prow].contiguous(), cls, pos, gamma, beta, xk, mk, rk, B, Lk, d, keep=_dev(keep))
    assert torch.equal(xk, x[trow]) and torch.equal(mk, mean[trow]) and torch.equal(rk, rstd[trow])


# ------------------------------------------------------------------------------------------------ embedding backward
def _close(a, b):
    """|a - b| <= 1e-5 |b| + 1e-6 max|b|: two fp32 summation orders of the same terms."""
    return bool(((a - b).abs() <= 1e-5 * b.abs() + 1e-6 * b.abs().max()).all())


def _forced_keep(B, n, K):
    """Explicit rows: patch 0 kept by every sample, patch n - 1 by none."""
    rows = [[0] + sorted(((7 * b + 3 * t) % (n - 2)) + 1 for t in range(K - 1)) for b in range(B)]
    keep = np.array(rows, dtype=np.int32)
    assert (np.diff(keep, axis=1) > 0).all() and keep.max() < n - 1
    return keep


@pytest.mark.parametrize("B,Lk,d,forced", [(1, 9, 192, False), (3, 9, 768, False), (90, 50, 64, False), (3, 6, 1280, True),
                                           (2, 4, 2048, False)])
def test_embed_ln_bwd_keep_against_the_full_kernel_on_zero_padded_gradients(B, Lk, d, forced):
    """B = 90, L' = 50: 4500 rows = 1125 row groups, more than the 1024 workgroups of the persistent row loop.  d = 2048: the
    workgroup's 64 KiB of LDS needs the raised dynamic-LDS limit."""
    *_, ops, _, pd = _pkg()
    n = 60
    L, K = n + 1, Lk - 1
    g = torch.Generator().manual_seed(B + d)
    patch_out = torch.randn(B * n, d, generator=g).cuda()
    cls, pos = torch.randn(d, generator=g).cuda(), torch.randn(L, d, generator=g).cuda()
    gamma, beta = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    keep = _forced_keep(B, n, K) if forced else pd.keep_indices_host(d, B, 0, B, n, K)
    slot = pd.slots_from_keep(keep, n)
    kl = torch.from_numpy(keep).long()
    prow = (torch.arange(B)[:, None] * n + kl).reshape(-1).cuda()
    trow = torch.cat([torch.arange(B)[:, None] * L, torch.arange(B)[:, None] * L + 1 + kl], 1).reshape(-1).cuda()
    # full-length forward statistics, full-length backward on a gradient that is zero outside the kept rows
    x = torch.empty(B * L, d, device="cuda")
    mean, rstd = torch.empty(B * L, device="cuda"), torch.empty(B * L, device="cuda")
    ops.embed_ln_fwd(patch_out, cls, pos, gamma, beta, x, mean, rstd, B, L, d)
    dx = torch.randn(B * Lk, d, generator=g).cuda()
    dres = torch.zeros(B * L, d, device="cuda")
    dres[trow] = dx
    dpatch = torch.zeros(B * n, d, dtype=torch.bfloat16, device="cuda")
    dg, db = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    dpos, dcls = torch.empty(L, d, device="cuda"), torch.empty(d, device="cuda")
    ops.embed_ln_bwd(dres, patch_out, cls, pos, mean, rstd, gamma, dpatch, dg, db, dpos, dcls, B, L, d)
    # the dropping backward, twice
    po_k = patch_out[prow].contiguous()
    outs = []
    for _ in range(2):
        dres_k = dx.clone()
        dpatch_k = torch.empty(B * K, d, dtype=torch.bfloat16, device="cuda")
        dg_k, db_k = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
        dpos_k, dcls_k = torch.full((L, d), 7.0, device="cuda"), torch.empty(d, device="cuda")
        ops.embed_ln_bwd(dres_k, po_k, cls, pos, mean[trow].contiguous(), rstd[trow].contiguous(), gamma, dpatch_k, dg_k, db_k,
                         dpos_k, dcls_k, B, Lk, d, keep=_dev(keep), slot=_dev(slot))
        outs.append((dres_k, dpatch_k, dg_k, db_k, dpos_k, dcls_k))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                # no atomics, fixed order: bit-reproducible
    dres_k, dpatch_k, dg_k, db_k, dpos_k, dcls_k = outs[0]
    assert torch.equal(dres_k, dres[trow])
    assert torch.equal(dpatch_k, dpatch[prow])
    assert _close(dg_k, dg) and _close(db_k, db) and _close(dpos_k, dpos) and _close(dcls_k, dcls)
    assert torch.equal(dcls_k, dpos_k[0])
    never = sorted(set(range(n)) - set(keep.reshape(-1).tolist()))
    if forced:
        assert n - 1 in never and bool((slot[:, 0] == 0).all())
    for j in never:
        assert float(dpos_k[1 + j].abs().max()) == 0.0          # exact zeros where no sample kept the patch


# ------------------------------------------------------------------------------------------------ the training step
def tiny_cfgs(width, head_width, layers, image, patch, embed=64, n_genes=200, hidden=64):
    *_, mc, _, _, _, _, _ = _pkg()
    cfg = mc.ModelCfg(embed_dim=embed, vision=mc.VisionCfg(image, patch, width, layers, head_width),
                      text=None, gene=mc.GeneCfg(n_genes, hidden))
    ocfg = O.ModelCfg(embed_dim=embed, vision=O.VisionCfg(image, patch, width, layers, head_width), text=None,
                      gene=O.GeneCfg(n_genes, hidden))
    return cfg, ocfg


def perturb(netobj, seed=11):
    g = torch.Generator().manual_seed(seed)
    sd = netobj.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    netobj.load_state_dict(sd)


# Cases of test_dropping_step_vs_oracle that miss the 4 % gradient bound, with the yardstick that replaces it there: the distance of
# the SAME oracle composition under torch.autocast(bfloat16) -- the reference's own precision policy -- from the fp32 oracle
# (tools/patch_dropout_parity.py -> profiles/patch_dropout_parity.txt).  The bound becomes 1.5 x that distance.
#   width 128, clip, fp32 stream, p = 0.5: visual.ln_post.bias (max|g| 6.5e-3, a sum of 12 bf16 rows): HIP 4.25 %, autocast 6.03 %
AUTOCAST_YARDSTICK = {(128, "clip", "fp32", 0.5): {"visual.ln_post.bias": 0.0603}}


def _bad_gradients(n, p, keep, n_patch, yardstick=None):
    """Names of the tensors whose gradient misses 4 % of the oracle tensor's max-abs; never-kept positions exact zeros."""
    bad = []
    for k in p:
        g_ref = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
        g = n.store.g(k).cpu()
        tol = max(0.04, 1.5 * (yardstick or {}).get(k, 0.0)) * float(g_ref.abs().max()) + 1e-6
        err = float((g - g_ref).abs().max())
        print(f"grad {k}: max|d| {err:.3e} of max|ref| {float(g_ref.abs().max()):.3e}")
        if err > tol:
            bad.append((k, err, float(g_ref.abs().max())))
    never = sorted(set(range(n_patch)) - set(np.asarray(keep).reshape(-1).tolist()))
    for j in never:
        assert float(n.store.g("visual.positional_embedding")[1 + j].abs().max()) == 0.0
        assert float(p["visual.positional_embedding"].grad[1 + j].abs().max()) == 0.0
    return bad


@pytest.mark.parametrize("width,head_width,image,patch", [(64, 32, 32, 8), (128, 64, 48, 16)])
@pytest.mark.parametrize("loss_kind", ["clip", "spatial"])
@pytest.mark.parametrize("stream,loss_tol", [("bf16", 6e-3), ("fp32", 4e-3)])
@pytest.mark.parametrize("drop", [0.5, 0.75])
def test_dropping_step_vs_oracle(width, head_width, image, patch, loss_kind, stream, loss_tol, drop):
    """The geometries and bounds of tests/test_gpu_model.py::test_forward_backward_vs_oracle; the oracle keeps the patches
    patch_dropout.keep_indices_host names for the net's seed and first draw."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    cfg, ocfg = tiny_cfgs(width, head_width, 2, image, patch)
    B, seed = 12, 3
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, residual_stream=stream, force_patch_dropout=drop)
    assert n.cfg.vision.patch_dropout == drop and n.patch_dropout_draw == 0
    perturb(n)
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    batch = data.synthetic_batch(B, image, cfg.gene.n_genes, K=4, step=0)
    n_patch = cfg.vision.tokens - 1
    keep = pd.keep_indices_host(seed, 0, 0, B, n_patch, pd.num_keep(n_patch, drop))
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    f = PO.net_forward_keep(batch["images"], batch["texts"], p, ocfg, keep)
    if loss_kind == "clip":
        lo = O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"])
        loss_fn = losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    else:
        lo = O.spatial_loss(f["image_features"], f["text_features"], f["logit_scale"], batch["image_tile_ids"],
                            batch["text_tile_ids"], batch["neighbor_tile_ids"], batch["neighbor_alphas"])
        loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0,
                                     temp_reg_weight=0.05, neighbor_alpha_scale=0.5, float32_logits=True)
    lo.backward()
    m = module.SpatialClipLitModule(n, loss_fn, None, None)
    out = m.model_step({k: v.cuda() for k, v in batch.items()})
    assert n.patch_dropout_draw == 1 and np.array_equal(n.vision.keep_idx.cpu().numpy(), keep)
    df = float((out["image_features"].cpu() - f["image_features"].detach()).abs().max())
    dl = abs(float(out["loss"].detach()) - float(lo.detach()))
    print(f"features max|d| {df:.3e}; loss |d| {dl:.3e}")
    assert df < 5e-3
    assert (out["text_features"].cpu() - f["text_features"].detach()).abs().max() < 5e-3
    assert dl < loss_tol
    out["loss"].backward()
    torch.cuda.synchronize()
    bad = _bad_gradients(n, p, keep, n_patch, AUTOCAST_YARDSTICK.get((width, loss_kind, stream, drop)))
    assert not bad, bad


def test_e4m3_path_drops_patches_within_its_stated_bounds():
    """precision="fp8" needs nothing of its own: the stack takes its length per call.  Geometry of tests/test_gpu_fp8.py::
    test_e4m3_mlp_weight_gradients_in_the_model (width 256, B = 128): at p = 0.5 the pass has 128 x 9 tokens = 9 K tiles of 128, so
    the e4m3 MLP weight gradients run too.  Second step at lr = 0 (the first primes the delayed scales) against the dropping fp32
    oracle, within the e4m3 path's stated distance: loss 1e-2, features 4e-2, gradients 35 % of max-abs."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 256, 3, 64), text=None, gene=mc.GeneCfg(200, 64))
    ocfg = O.ModelCfg(embed_dim=64, vision=O.VisionCfg(32, 8, 256, 3, 64), text=None, gene=O.GeneCfg(200, 64))
    B, seed = 128, 9
    batch = data.synthetic_batch(B, 32, 200, K=4, step=0)
    db = {k: v.cuda() for k, v in batch.items()}
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, precision="fp8", force_patch_dropout=0.5)
    m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    for _ in range(2):
        out = m.model_step(db)
        out["loss"].backward()
    torch.cuda.synchronize()
    assert n.vision.L_run == 9 and n.vision.stack.fwd.w8 and n.patch_dropout_draw == 2
    keep = pd.keep_indices_host(seed, 1, 0, B, 16, 8)
    assert np.array_equal(n.vision.keep_idx.cpu().numpy(), keep)
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in n.state_dict().items()}
    f = PO.net_forward_keep(batch["images"], batch["texts"], p, ocfg, keep)
    lo = O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"])
    lo.backward()
    dl = abs(float(out["loss"].detach()) - float(lo.detach()))
    df = float((out["image_features"].detach().cpu() - f["image_features"].detach()).abs().max())
    worst = max((float((n.store.g(k).cpu() - p[k].grad).abs().max() / p[k].grad.abs().max()), k)
                for k in p if p[k].grad is not None and float(p[k].grad.abs().max()) > 0)
    print(f"[fp8 + patch dropout] |d loss| {dl:.2e}, max|d feature| {df:.2e}, worst gradient {worst[0]:.3f} ({worst[1]})")
    assert dl < 1e-2 and df < 4e-2 and worst[0] < 0.35


@pytest.mark.parametrize("stream", ["bf16", "fp32"])
def test_reference_patch_dropout_fixture(stream):
    """The reference's own tower (vision_cfg.patch_dropout = 0.5, train mode, fp32) on the indices IT drew, sorted: features
    within 5e-3, every vision gradient of sum(features * target) within 4 % of its tensor's max-abs, exact zeros in the
    positional-embedding rows of patches no sample kept."""
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    z = np.load(GOLDEN)
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32, 2.0, 0.5), text=None, gene=mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=0, residual_stream=stream)
    sd = {k: v.cpu() for k, v in n.state_dict().items()}
    for k in z.files:
        if k.startswith("w."):
            assert k[2:] in sd and tuple(sd[k[2:]].shape) == z[k].shape, k
            sd[k[2:]] = torch.from_numpy(z[k])
    n.load_state_dict(sd)
    keep = np.sort(z["keep_topk_order"], axis=1)
    B = keep.shape[0]
    n.set_patch_keep(keep)
    texts = torch.randn(B, 200, generator=torch.Generator().manual_seed(1)).cuda()
    out = n(_dev(z["images"]), texts)
    assert np.array_equal(n.vision.keep_idx.cpu().numpy(), keep)
    df = float((out["image_features"].cpu() - torch.from_numpy(z["features"])).abs().max())
    print(f"features max|d| {df:.3e}")
    assert df < 5e-3
    (out["image_features"] * _dev(z["target"])).sum().backward()
    torch.cuda.synchronize()
    bad = []
    for k in z.files:
        if not k.startswith("g."):
            continue
        g_ref, g = torch.from_numpy(z[k]), n.store.g(k[2:]).cpu().reshape(z[k].shape)
        err, top = float((g - g_ref).abs().max()), float(g_ref.abs().max())
        print(f"grad {k[2:]}: max|d| {err:.3e} of max|ref| {top:.3e}")
        if err > 0.04 * top + 1e-6:
            bad.append((k, err, top))
    assert not bad, bad
    never = sorted(set(range(16)) - set(keep.reshape(-1).tolist()))
    assert never, "the fixture is meant to hold a patch no sample kept"
    for j in never:
        assert float(np.abs(z["g.visual.positional_embedding"][1 + j]).max()) == 0.0
        assert float(n.store.g("visual.positional_embedding")[1 + j].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ modes
def _cfg():
    *_, mc, _, _, _, _, _ = _pkg()
    return mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))


def _batch(B=12, step=0):
    data, *_ = _pkg()
    return {k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=step).items()}


@pytest.mark.parametrize("p", [1.0, -0.1])
def test_constructor_refuses_a_fraction_outside_the_interval(p):
    *_, net, _, _, _ = _pkg()
    with pytest.raises(ValueError):
        net.SpatialClipNet("custom", None, model_cfg=_cfg(), force_patch_dropout=p)


def test_evaluation_forwards_run_all_tokens():
    """no_grad forwards, encode_image and anything after net.eval() are bit-identical to a net without patch dropout."""
    *_, net, _, _, _ = _pkg()
    b = _batch()
    n0 = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3)
    n5 = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3, force_patch_dropout=0.5)
    with torch.no_grad():
        want = n0(b["images"], b["texts"])["image_features"].clone()
        assert torch.equal(n5(b["images"], b["texts"])["image_features"], want)
    assert torch.equal(n5.model.encode_image(b["images"], normalize=True), want)
    dropped = n5(b["images"], b["texts"])["image_features"]            # training mode, grad on: this one drops
    assert n5.patch_dropout_draw == 1 and n5.vision.L_run == 9 and not torch.equal(dropped, want)
    with torch.no_grad():                                               # ... and full length again right after it
        assert torch.equal(n5(b["images"], b["texts"])["image_features"], want)
    n5.eval()
    assert torch.equal(n5(b["images"], b["texts"])["image_features"], want)
    assert n5.patch_dropout_draw == 1 and n5.vision.L_run == 17
    # a net without patch dropout never selects anything
    n0(b["images"], b["texts"])
    assert n0.vision.keep_idx is None and n0.patch_dropout_draw == 0


def test_draws_follow_seed_and_counter():
    *_, net, _, _, pd = _pkg()
    b = _batch()
    a, c = (net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=5, force_patch_dropout=0.5) for _ in range(2))
    seq = []
    for n in (a, c):
        rows = []
        for _ in range(3):
            n(b["images"], b["texts"])
            rows.append(n.vision.keep_idx.cpu().numpy().copy())
        seq.append(rows)
    for draw in range(3):
        assert np.array_equal(seq[0][draw], seq[1][draw])
        assert np.array_equal(seq[0][draw], pd.keep_indices_host(5, draw, 0, 12, 16, 8))
    assert not np.array_equal(seq[0][0], seq[0][1]) and not np.array_equal(seq[0][1], seq[0][2])


def test_set_patch_keep_is_validated_and_consumed_once():
    *_, net, _, _, pd = _pkg()
    b = _batch()
    n = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=5, force_patch_dropout=0.5)
    for bad in (np.arange(8)[None, :].repeat(12, 0)[:, ::-1], np.arange(7)[None, :].repeat(12, 0), np.full((12, 8), 16)):
        with pytest.raises(ValueError):
            n.set_patch_keep(np.ascontiguousarray(bad))
    n.set_patch_keep(np.arange(8)[None, :].repeat(5, 0))                # right K, wrong batch: refused by the forward
    with pytest.raises(ValueError):
        n(b["images"], b["texts"])
    mine = np.arange(0, 16, 2)[None, :].repeat(12, 0)
    n.set_patch_keep(mine)
    n(b["images"], b["texts"])
    assert np.array_equal(n.vision.keep_idx.cpu().numpy(), mine)
    n(b["images"], b["texts"])                                           # the hook is spent: the next forward draws
    assert np.array_equal(n.vision.keep_idx.cpu().numpy(), pd.keep_indices_host(5, n.patch_dropout_draw - 1, 0, 12, 16, 8))
    with pytest.raises(ValueError):
        net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=5).set_patch_keep(mine)


def test_grad_checkpointing_is_bit_identical_under_patch_dropout():
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    b = _batch()
    got = []
    for rc in (False, True):
        n = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=3, force_patch_dropout=0.5, grad_checkpointing=rc)
        perturb(n)
        m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
        out = m.model_step(b)
        out["loss"].backward()
        torch.cuda.synchronize()
        got.append((out["image_features"].detach().clone(), {k: n.store.g(k).clone() for k in n.state_dict()}))
    assert torch.equal(got[0][0], got[1][0])
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k


def _trainable(seed=3, p=0.5, **kw):
    data, graph, losses, mc, module, net, ops, optim, pd = _pkg()
    n = net.SpatialClipNet("custom", None, model_cfg=_cfg(), seed=seed, force_patch_dropout=p, **kw)
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=1))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = 20, None, 20
    m.trainer = T()
    oc = m.configure_optimizers()
    return n, m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def test_graphed_step_declines_and_runs_eagerly(monkeypatch):
    data, graph, *_ = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")            # nothing else stands between this step and a capture
    n0, m0, opt0, _ = _trainable(p=None)
    assert graph.GraphedTrainStep(m0, opt0, max_norm=1.0).capturable() is None
    n, m, opt, sched = _trainable()
    step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
    assert "patch dropout" in step.capturable()
    losses_ = []
    for i in range(3):
        losses_.append(float(step(_batch(step=i)).detach()))
        sched.step()
        assert step.graph is None and step.failed is None
    assert n.patch_dropout_draw == 3 and all(np.isfinite(losses_))


def test_checkpoint_round_trip_resumes_the_draw_counter(tmp_path):
    from spatial_clip_amd.trainer import Trainer
    b = _batch()

    def steps(m, opt, sched, k):
        out = []
        for s in range(k):
            loss = m.training_step(b, s)
            loss.backward()
            opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
            out.append((float(loss.detach()), m.net.vision.keep_idx.cpu().numpy().copy()))
        return out

    n1, m1, opt1, sch1 = _trainable()
    ref = steps(m1, opt1, sch1, 4)
    n2, m2, opt2, sch2 = _trainable()
    first = steps(m2, opt2, sch2, 2)
    path = str(tmp_path / "flip.ckpt")
    Trainer.save_checkpoint(path, m2, opt2, sch2, 2)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["patch_dropout_draw"] == 2 and "patch_dropout_draw" not in ck["state_dict"]
    n3, m3, opt3, sch3 = _trainable()                       # same seed (the seed is configuration), fresh counter
    assert Trainer.load_checkpoint(path, m3, opt3, sch3) == 2 and n3.patch_dropout_draw == 2
    rest = steps(m3, opt3, sch3, 2)
    for (la, ka), (lb, kb) in zip(first + rest, ref):
        assert np.array_equal(ka, kb) and la == lb
    # a net without patch dropout writes no counter
    n0, m0, opt0, sch0 = _trainable(p=None)
    Trainer.save_checkpoint(path, m0, opt0, sch0, 0)
    assert "patch_dropout_draw" not in torch.load(path, map_location="cpu", weights_only=False)
