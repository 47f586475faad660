"""Distillation loss on the device against the REFERENCE's own numbers (tests/golden/make_golden_distill.py) and the float64
oracle (tests/_distill_oracle.py): the head, both row paths of the kernel, the two-output loss node, two emulated ranks, the
module with a frozen teacher, graph replay and the training entry point."""
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _distill_oracle as DO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ("c", "d")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import contrastive, data, graph, losses, model_configs as mc, module, net, ops, optim, trainer
    return contrastive, data, graph, losses, mc, module, net, ops, optim, trainer


# The bounds tests/test_gpu_loss.py and tests/test_gpu_siglip.py hold the CE head to for the same quantities.
def _num(x):
    return float(x.detach()) if isinstance(x, torch.Tensor) else float(x)


def _loss_ok(got, want):
    return abs(_num(got) - _num(want)) <= 5e-6 + 2e-6 * abs(_num(want))


def _scale_ok(got, want):
    return abs(_num(got) - _num(want)) <= 5e-6 + 1e-5 * abs(_num(want))


def _grad_close(got, want, tag, factor=1.0):
    np.testing.assert_allclose(np.asarray(got.detach().cpu(), dtype=np.float64), np.asarray(want, dtype=np.float64),
                               atol=2e-6 * factor, rtol=1e-4 * factor, err_msg=tag)


# Distillation-term feature gradients that cannot meet atol 2e-6 / rtol 1e-4, with the figure the issue's rule gives them: the
# EXISTING contrastive_forward_backward(mode="clip") measured against its float64 golden on the same inputs (the gimg_c / gtxt_c
# of the same file are ClipLoss's gradients), worst |got - want| / (2e-6 + 1e-4 |want|) on one MI355X, and TWICE that as the
# bound (the distill row does two exp-sums where CE does one).
#   B7_D16_s100_t1_ (saturated student, near-uniform teacher, B = 7): clip head 1.421 x the bound on d_image; the distill head
#   1.009 x on gimg_d (its contrastive term: 0.134 x), so gimg_d / gtxt_d of this one case are held to 2 * 1.421 = 2.842 x.
#   The entries that miss are near-zero sums of terms of magnitude s * 0.5 / B * |p_s - p_t| ~ 6: fp32 products summed in fp32.
# Every other case and quantity (31 of 32 cases; all losses, scale gradients and contrastive-term gradients) meets the CE
# head's own bounds as they stand; measured worst elsewhere: 0.84 x (B12_D16_s100_t1_ gimg_d).
CLIP_HEAD_MEASURED = {"B7_D16_s100_t1_": 1.421}


def _worst(got, want):
    """max of |got - want| / (atol + rtol |want|): <= 1 passes _grad_close (printed before the assertion)."""
    got, want = np.asarray(got.detach().cpu(), dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (2e-6 + 1e-4 * np.abs(want))).max())


def _cuda(a):
    return torch.from_numpy(np.asarray(a)).float().cuda()


# ---------------------------------------------------------------------------------------------------------- 1. the head
def _w1_cases(golden_dir):
    for path in sorted(glob.glob(os.path.join(golden_dir, "distill_w1_*.npz"))):
        z = np.load(path, allow_pickle=False)
        scales = json.loads(str(z["scales"]))
        for B, D, Dt, tag in json.loads(str(z["cases"])):
            yield z, B, D, Dt, tag, scales[tag]


def test_distill_head_matches_reference_and_is_bit_identical(golden_dir):
    """Every one-rank golden (B in {7, 12, 64, 300} x (D, D_t) x four scale pairs), join_local: both losses, grads_c and
    grads_d separately, two calls bitwise equal.  The bounds are the CE head's own (see _loss_ok / _grad_close / _scale_ok), but
    for the one case listed in CLIP_HEAD_MEASURED.  Every figure, the clip head's on the same inputs included, is printed first."""
    C = _pkg()[0]
    n_cases = 0
    for z, B, D, Dt, tag, (s, st) in _w1_cases(golden_dir):
        p = f"B{B}_D{D}_{tag}_"
        f = [_cuda(z[f"B{B}_D{D}_{k}"]) for k in ("img", "txt", "timg", "ttxt")]
        sc, tsc = torch.tensor(s, device="cuda"), torch.tensor(st, device="cuda")
        res = C.distill_forward_backward(f[0], f[1], sc, f[2], f[3], tsc, join_local=True)
        res2 = C.distill_forward_backward(f[0], f[1], sc, f[2], f[3], tsc, join_local=True)
        n = B * D
        ref = C.contrastive_forward_backward(f[0], f[1], sc, mode="clip", join_local=True, want_recall=False)
        fig = {"clip_head_gimg": _worst(ref["d_image"], z[p + "gimg_c"]), "clip_head_gtxt": _worst(ref["d_text"], z[p + "gtxt_c"]),
               "closs": abs(float(res["contrastive_loss"]) - float(z[p + "closs"])),
               "dloss": abs(float(res["distill_loss"]) - float(z[p + "dloss"]))}
        for k in TERMS:
            g = res["grads_" + k]
            assert g.shape == (2 * n + 2,) and g.is_contiguous() and float(g[-1]) == 0.0
            fig["gimg_" + k] = _worst(g[:n].view(B, D), z[p + "gimg_" + k])
            fig["gtxt_" + k] = _worst(g[n:2 * n].view(B, D), z[p + "gtxt_" + k])
            fig["gscale_" + k] = abs(float(g[2 * n]) - float(z[p + "gscale_" + k]))
        print(p, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
        assert _loss_ok(res["contrastive_loss"], z[p + "closs"]), (p, float(res["contrastive_loss"]), float(z[p + "closs"]))
        assert _loss_ok(res["distill_loss"], z[p + "dloss"]), (p, float(res["distill_loss"]), float(z[p + "dloss"]))
        for k in TERMS:
            g = res["grads_" + k]
            factor = max(1.0, 2.0 * CLIP_HEAD_MEASURED.get(p, 0.0)) if k == "d" else 1.0
            _grad_close(g[:n].view(B, D), z[p + "gimg_" + k], p + "gimg_" + k, factor)
            _grad_close(g[n:2 * n].view(B, D), z[p + "gtxt_" + k], p + "gtxt_" + k, factor)
            assert _scale_ok(g[2 * n], z[p + "gscale_" + k]), (p, k, float(g[2 * n]), float(z[p + "gscale_" + k]))
            assert torch.equal(g, res2["grads_" + k]), p                                                  # bitwise
        assert torch.equal(res["contrastive_loss"], res2["contrastive_loss"]) and torch.equal(res["distill_loss"],
                                                                                              res2["distill_loss"]), p
        assert bool(torch.isfinite(res["grads_d"]).all()) and bool(torch.isfinite(res["distill_loss"]))
        n_cases += 1
    assert n_cases == 32


def test_distill_head_contrastive_term_is_the_clip_head(golden_dir):
    """The contrastive term is ClipLoss: same loss and gradients as contrastive_forward_backward(mode="clip") to the bounds,
    and the R@k counters ride on the same similarity matrix."""
    C = _pkg()[0]
    z = np.load(os.path.join(golden_dir, "distill_w1_B64.npz"), allow_pickle=False)
    f = [_cuda(z[f"B64_D64_{k}"]) for k in ("img", "txt", "timg", "ttxt")]
    s = torch.tensor(14.3, device="cuda")
    hits, hits_ref = (torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(2))
    res = C.distill_forward_backward(f[0], f[1], s, f[2], f[3], s, join_local=True, recall_hits=hits)
    ref = C.contrastive_forward_backward(f[0], f[1], s, mode="clip", join_local=True, recall_hits=hits_ref)
    assert _loss_ok(res["contrastive_loss"], ref["loss"])
    _grad_close(res["grads_c"][:-1], ref["grads"][:-1].cpu(), "grads_c vs clip head")
    assert torch.equal(hits, hits_ref) and int(hits[2]) > 0


# ------------------------------------------------------------------------------------------------------- 2. row paths
@pytest.mark.parametrize("side", ["resident", "reread"])
def test_distill_row_paths_straddle_the_threshold(side):
    """B = 8 local rows of rank 1 against G gathered rows, G at the register-resident limit and one past it (the re-reading
    path), against the float64 oracle: losses, direct and gathered-feature gradients of both terms, scale gradients."""
    C, ops = _pkg()[0], _pkg()[7]
    limit = ops.distill_resident_max_g()
    G = limit if side == "resident" else limit + 1
    assert (G <= limit) == (side == "resident") and limit - 1 < G <= limit + 1      # the two cases straddle the threshold
    B, D, Dt, rank, s, st = 8, 32, 24, 1, 30.0, 40.0
    g = torch.Generator().manual_seed(G)
    unit = functools.partial(torch.nn.functional.normalize, dim=-1)
    img = unit(torch.randn(G, D, generator=g))
    txt = unit(img + 0.5 * torch.randn(G, D, generator=g))
    timg = unit(torch.randn(G, Dt, generator=g))
    ttxt = unit(timg + 0.3 * torch.randn(G, Dt, generator=g))
    sl = slice(rank * B, (rank + 1) * B)
    want = DO.distill_terms(img[sl], txt[sl], s, timg[sl], ttxt[sl], st, img, txt, timg, ttxt, rank=rank)
    dev = [t.cuda() for t in (img, txt, timg, ttxt)]
    res = C.distill_forward_backward(dev[0][sl].contiguous(), dev[1][sl].contiguous(), torch.tensor(s, device="cuda"),
                                     dev[2][sl].contiguous(), dev[3][sl].contiguous(), torch.tensor(st, device="cuda"),
                                     all_image=dev[0], all_text=dev[1], dist_all_image=dev[2], dist_all_text=dev[3], rank=rank)
    for k, name in zip(TERMS, ("contrastive_loss", "distill_loss")):
        print(side, name, float(res[name]), float(want[k]["loss"]), "d_scale", float(res["d_scale_" + k]),
              float(want[k]["d_scale"]), "worst d_image", _worst(res["d_image_" + k], want[k]["d_image"]))
        assert _loss_ok(res[name], want[k]["loss"]), (name, float(res[name]), float(want[k]["loss"]))
        assert _scale_ok(res["d_scale_" + k], want[k]["d_scale"]), k
        _grad_close(res["d_image_" + k], want[k]["d_image"], "d_image_" + k)
        _grad_close(res["d_text_" + k], want[k]["d_text"], "d_text_" + k)
        _grad_close(res["d_all_" + k][:, :D], want[k]["d_all_image"], "d_all_image_" + k)
        _grad_close(res["d_all_" + k][:, D:], want[k]["d_all_text"], "d_all_text_" + k)


# ------------------------------------------------------------------------------------------- 3. the loss node (autograd)
@pytest.mark.parametrize("upstream", [(1.0, 1.0), (-2.5, -2.5), (1.0, 0.25)])
def test_distill_loss_node_applies_each_upstream_gradient(golden_dir, upstream):
    """(1, 0.25) is the pair a single pre-summed gradient buffer would get wrong.  Teacher tensors get no gradient."""
    losses = _pkg()[3]
    z = np.load(os.path.join(golden_dir, "distill_w1_B12.npz"), allow_pickle=False)
    p, (s, st) = "B12_D64_s14_t14_", (14.3, 14.3)
    g_c, g_d = upstream
    i, t, ti, tt = (_cuda(z[f"B12_D64_{k}"]).requires_grad_(True) for k in ("img", "txt", "timg", "ttxt"))
    sc = torch.tensor(s, device="cuda", requires_grad=True)
    tsc = torch.tensor(st, device="cuda", requires_grad=True)
    out = losses.DistillClipLoss()(i, t, sc, ti, tt, tsc)
    assert isinstance(out, tuple) and len(out) == 2 and out[0].dim() == 0 and out[1].dim() == 0
    assert _loss_ok(out[0], z[p + "closs"]) and _loss_ok(out[1], z[p + "dloss"])
    (g_c * out[0] + g_d * out[1]).backward()
    _grad_close(i.grad, g_c * z[p + "gimg_c"] + g_d * z[p + "gimg_d"], "gimg")
    _grad_close(t.grad, g_c * z[p + "gtxt_c"] + g_d * z[p + "gtxt_d"], "gtxt")
    assert _scale_ok(sc.grad, g_c * float(z[p + "gscale_c"]) + g_d * float(z[p + "gscale_d"]))
    assert ti.grad is None and tt.grad is None and tsc.grad is None
    if g_c != g_d:      # the two terms really pull differently here: a shared factor would miss by far more than the bound
        mixed = g_c * (z[p + "gimg_c"] + z[p + "gimg_d"])
        assert np.abs(mixed - np.asarray(i.grad.cpu(), dtype=np.float64)).max() > 1e-3


def test_distill_loss_output_dict_and_single_term_backward(golden_dir):
    losses = _pkg()[3]
    z = np.load(os.path.join(golden_dir, "distill_w1_B7.npz"), allow_pickle=False)
    p = "B7_D16_s10_t100_"
    f = [_cuda(z[f"B7_D16_{k}"]) for k in ("img", "txt", "timg", "ttxt")]
    s, st = torch.tensor(10.0, device="cuda"), torch.tensor(100.0, device="cuda")
    crit = losses.DistillClipLoss(local_loss=True, gather_with_grad=True)
    d = crit(*f[:2], s, *f[2:], st, output_dict=True)
    assert isinstance(d, dict) and list(d) == ["contrastive_loss", "distill_loss"]
    tup = crit(*f[:2], s, *f[2:], st, output_dict=False)
    assert torch.equal(tup[0], d["contrastive_loss"]) and torch.equal(tup[1], d["distill_loss"])
    i = f[0].clone().requires_grad_(True)       # only the distillation term is differentiated: the other gets a zero gradient
    crit(i, f[1], s, *f[2:], st)[1].backward()
    _grad_close(i.grad, z[p + "gimg_d"], "gimg_d alone")


# --------------------------------------------------------------------------------------------------- 4. two emulated ranks
@pytest.mark.parametrize("layout", ["local", "global"])
def test_distill_two_emulated_ranks_match_reference(golden_dir, layout):
    """The 2-rank gloo golden with the ranks emulated on one GPU: the cross-rank d(all features) terms are summed by hand as the
    per-term reduce-scatter would (local_loss), or the [G, G] head's rows are taken W times (local_loss=False: every rank
    contributes the same full-loss term)."""
    C = _pkg()[0]
    z = np.load(os.path.join(golden_dir, "distill_w2.npz"), allow_pickle=False)
    W, G, D = int(z["world"]), z["img"].shape[0], z["img"].shape[1]
    B = G // W
    img, txt, timg, ttxt = (_cuda(z[k]) for k in ("img", "txt", "timg", "ttxt"))
    s = torch.tensor(float(z["scale"]), device="cuda")
    st = torch.tensor(float(z["dist_scale"]), device="cuda")
    outs = []
    for r in range(W):
        sl = slice(r * B, (r + 1) * B)
        if layout == "local":
            outs.append(C.distill_forward_backward(img[sl].contiguous(), txt[sl].contiguous(), s, timg[sl].contiguous(),
                                                   ttxt[sl].contiguous(), st, all_image=img, all_text=txt,
                                                   dist_all_image=timg, dist_all_text=ttxt, rank=r))
        else:
            outs.append(C.distill_forward_backward(img, txt, s, timg, ttxt, st, rank=0, recall_rows=(r * B, B)))
    for r in range(W):
        sl = slice(r * B, (r + 1) * B)
        o, pre = outs[r], f"r{r}_{layout}_"
        assert _loss_ok(o["contrastive_loss"], z[pre + "closs"]) and _loss_ok(o["distill_loss"], z[pre + "dloss"])
        for k in TERMS:
            if layout == "local":
                gi = o["d_image_" + k] + sum(x["d_all_" + k][sl, :D] for x in outs)
                gt = o["d_text_" + k] + sum(x["d_all_" + k][sl, D:] for x in outs)
            else:
                gi = W * (o["d_image_" + k] + o["d_all_" + k][:, :D])[sl]
                gt = W * (o["d_text_" + k] + o["d_all_" + k][:, D:])[sl]
            _grad_close(gi, z[pre + "gimg_" + k], pre + "gimg_" + k)
            _grad_close(gt, z[pre + "gtxt_" + k], pre + "gtxt_" + k)
            assert _scale_ok(o["d_scale_" + k], z[pre + "gscale_" + k]), (pre, k)


# ------------------------------------------------------------------------------------------------ 5. module with a teacher
def _cfgs(mc):
    student = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    teacher = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 96, 3, 32), text=None, gene=mc.GeneCfg(200, 64))
    return student, teacher


def _module(with_teacher=True, teacher_net=None, **student_kw):
    C, data, graph, losses, mc, module, net, ops, optim, trainer = _pkg()
    scfg, tcfg = _cfgs(mc)
    n = net.SpatialClipNet("custom", None, model_cfg=scfg, seed=3, **student_kw)
    t = None
    if with_teacher:
        t = teacher_net if teacher_net is not None else net.SpatialClipNet("custom", None, model_cfg=tcfg, seed=11)
    loss = losses.DistillClipLoss(local_loss=True, gather_with_grad=True) if with_teacher else \
        losses.ClipLoss(local_loss=True, gather_with_grad=True)
    m = module.SpatialClipLitModule(
        n, loss, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=3), dist_net=t)

    class T:
        max_steps, max_epochs, estimated_stepping_batches = 40, None, 40
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, n, t, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _batches(steps, B=24):
    data = _pkg()[1]
    return [{k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=s).items()} for s in range(steps)]


def test_module_trains_the_student_and_leaves_the_teacher_alone(tmp_path):
    C, data, graph, losses, mc, module, net, ops, optim, trainer = _pkg()
    m, n, t, opt, sched = _module()
    plain = _module(with_teacher=False)
    assert opt.exp_avg.numel() == plain[3].exp_avg.numel()                       # the optimiser holds the student alone
    assert len(list(m.parameters())) == len(list(plain[0].parameters()))
    assert not t.training and m.dist_net is t and all(mod is not t for mod in m.modules())
    m.train()
    assert not t.training and n.training                                         # module.train() cannot reach the teacher
    before_t = t.store.master.detach().clone()
    before_s = n.store.master.detach().clone()
    for step, batch in enumerate(_batches(3)):
        loss = m.training_step(batch, step)
        loss.backward()
        opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()
        c, d = m.logged["train/contrastive_loss"], m.logged["train/distill_loss"]
        assert torch.equal(m.logged["train/loss"], c + d) and torch.equal(loss.detach(), c + d)
        assert np.isfinite(float(c)) and np.isfinite(float(d)) and float(d) > 0.0
    n.store.wait_all()
    torch.cuda.synchronize()
    assert torch.equal(t.store.master, before_t)                                 # frozen, bit for bit
    assert not torch.equal(n.store.master, before_s)
    assert not any(k.startswith(("dist_net", "_teacher")) for k in m.state_dict())
    assert set(m.state_dict()) == set(plain[0].state_dict())
    path = str(tmp_path / "ck.ckpt")
    trainer.Trainer.save_checkpoint(path, m, opt, sched, 3)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck["state_dict"]) == set(n.state_dict()) and len(ck["state_dict"]) < len(t.state_dict())
    # validation and test steps run the teacher too and log the two terms beside their sum
    for prefix, step_fn in (("val/", m.validation_step), ("test/", m.test_step)):
        step_fn(_batches(1)[0], 0)
        assert torch.equal(m.logged[prefix + "loss"], m.logged[prefix + "contrastive_loss"] + m.logged[prefix + "distill_loss"])


def test_teacher_equal_to_the_student_gives_the_students_softmax_entropy():
    C, data, graph, losses, mc, module, net, ops, optim, trainer = _pkg()
    scfg, _ = _cfgs(mc)
    twin = net.SpatialClipNet("custom", None, model_cfg=scfg, seed=3)
    m, n, t, opt, sched = _module(teacher_net=twin)
    twin.load_state_dict(n.state_dict())
    batch = _batches(1)[0]
    m.validation_step(batch, 0)
    with torch.no_grad():
        f = n(batch["images"], batch["texts"])
    tf = m.teacher_features(batch)
    want = DO.distill_single(f["image_features"], f["text_features"], float(f["logit_scale"]), tf["dist_image_features"],
                             tf["dist_text_features"], float(tf["dist_logit_scale"]))
    assert _loss_ok(m.logged["val/distill_loss"], want["dloss"]), (float(m.logged["val/distill_loss"]), float(want["dloss"]))
    assert _loss_ok(m.logged["val/contrastive_loss"], want["closs"])
    # ... which is the entropy of the student's own softmax rows, averaged over the two directions
    fi, ft, s = f["image_features"].double().cpu(), f["text_features"].double().cpu(), float(f["logit_scale"])
    ent = 0.0
    for x in (s * fi @ ft.T, s * ft @ fi.T):
        lp = torch.log_softmax(x, dim=1)
        ent += 0.5 * float(-(lp.exp() * lp).sum(dim=1).mean())
    assert abs(float(want["dloss"]) - ent) <= 1e-4 * max(1.0, ent), (float(want["dloss"]), ent)


def test_teacher_sees_every_token_when_the_student_drops_patches():
    C, data, graph, losses, mc, module, net, ops, optim, trainer = _pkg()
    m, n, t, opt, sched = _module(force_patch_dropout=0.5)
    assert n.patch_dropout == 0.5 and t.patch_dropout == 0.0
    batch = _batches(1)[0]
    seen = {}
    inner = m.loss_fn.forward

    def spy(*a, **kw):
        seen.update({k: v.detach().clone() for k, v in kw.items() if k.startswith("dist_")})
        return inner(*a, **kw)
    m.loss_fn.forward = spy
    m.train()
    loss = m.training_step(batch, 0)
    loss.backward()
    assert n.patch_dropout_draw == 1 and t.patch_dropout_draw == 0              # the student dropped, the teacher did not
    with torch.no_grad():
        full = t(batch["images"], batch["texts"])                               # the teacher's own evaluation forward
    assert torch.equal(seen["dist_image_features"], full["image_features"])
    assert torch.equal(seen["dist_text_features"], full["text_features"])
    assert torch.equal(seen["dist_logit_scale"], full["logit_scale"])
    assert np.isfinite(float(loss.detach()))


# ---------------------------------------------------------------------------------------------------------- 6. graph replay
def test_graph_replay_of_a_distill_step_is_bit_identical(monkeypatch):
    """Eager against captured-and-replayed, 6 steps: losses, weights and optimiser state bit for bit.  If the runtime cannot
    capture the step, GraphedTrainStep stays eager by design: the test then reports ``step.failed`` and checks only the
    equality (no replay count) -- it says so in its output."""
    C, data, graph, losses, mc, module, net, ops, optim, trainer = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "0")
    steps = 6
    batches = _batches(steps)
    res = {}
    for mode in ("eager", "graph"):
        m, n, t, opt, sched = _module()
        t0 = t.store.master.detach().clone()
        step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        ls, terms = [], []
        for i in range(steps):
            loss = step.eager(batches[i]) if mode == "eager" else step(batches[i])
            sched.step()
            ls.append(float(loss.detach()))
            terms.append((float(m.logged["train/contrastive_loss"]), float(m.logged["train/distill_loss"])))
        n.store.wait_all()
        torch.cuda.synchronize()
        assert torch.equal(t.store.master, t0)
        res[mode] = dict(loss=ls, terms=terms, w=n.store.master.detach().clone(), m=opt.exp_avg.clone(),
                         v=opt.exp_avg_sq.clone(), replays=step.replays, failed=step.failed)
    if res["graph"]["failed"] is None:
        assert res["graph"]["replays"] == steps - 1
    else:
        print("capture failed inside the runtime, the step stayed eager:", res["graph"]["failed"])
    assert res["eager"]["loss"] == res["graph"]["loss"], (res["eager"]["loss"], res["graph"]["loss"])
    assert res["eager"]["terms"] == res["graph"]["terms"]
    for k in ("w", "m", "v"):
        assert torch.equal(res["eager"][k], res["graph"][k]), k
    assert all(np.isfinite(res["eager"]["loss"]))


# ------------------------------------------------------------------------------------------------------ 7. training entry
def test_train_entry_point_with_a_teacher(tmp_path):
    env = dict(os.environ, PROJECT_ROOT=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    net_target = "src.models.components.spatial_clip_net.SpatialClipNet"
    cmd = [sys.executable, "-m", "spatial_clip_amd.train", "experiment=smoke_shards", "loss=distill",
           f"+model.dist_net._target_={net_target}", "+model.dist_net.model_name=ViT-Ti-16-gene",
           "+model.dist_net.n_genes=2000", "+model.dist_net.seed=5", "trainer.max_steps=4", "trainer.fast_dev_run=False",
           "trainer.max_epochs=1", "data.steps_per_epoch=4", "data.val_steps=1", "save_ckpt=True", "callbacks=default",
           "test=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert last, r.stdout[-2000:]
    metrics = eval(last[-1], {"nan": float("nan"), "inf": float("inf")})      # the dict train.main prints
    assert all(np.isfinite(float(v)) for k, v in metrics.items() if "loss" in k and isinstance(v, (int, float))), metrics
    ckpts = glob.glob(os.path.join(str(tmp_path), "**", "last.ckpt"), recursive=True)
    assert ckpts, r.stdout[-2000:]
    sd = torch.load(ckpts[0], map_location="cpu", weights_only=False)["state_dict"]
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import model_configs as mc, params
    names = {s.name for s in params.build_specs(mc.get_model_config("ViT-Ti-16-gene", 2000))}
    assert set(sd) == names and not any("dist" in k for k in sd)               # the student's tensors, once; no teacher key
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
