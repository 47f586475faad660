"""Locked towers (LiT) through the HIP towers, the fused optimiser, the accumulator, the reducer and the graphed step.

1. the reference's three locked variants (tests/golden/make_golden_lock.py) with the bounds of
   tests/test_gpu_model.py::test_reference_three_training_steps_text_tower;
2. every floor position of a ``-gene`` model against the fp32 oracle with ``requires_grad`` set as the reference sets it;
3. bit-identity of the step forms (behind the forward / one launch / graphed / accumulated) with a lock;
4. the activation memory of a locked prefix does not grow with depth;
5. a one-rank process group with the distributed path forced on reduces 4 x trainable floats and changes no bit;
6. a net without a lock gives the bits and the library calls of the commit in front of the feature."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import spatial_clip_oracle as O
from tests import _pool_oracle as PO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
G0_ROUNDING = 2.0 ** -11        # the fixture's step-0 gradients are float16 of g / max|g| (make_golden_lock.py)


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, data, graph, losses, model_configs as mc, module, net, optim, patch_dropout as pd, streams
    return comm, data, graph, losses, mc, module, net, optim, pd, streams


def _spatial(losses):
    return losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                              neighbor_alpha_scale=0.5, float32_logits=True)


def _module(n, loss_fn, warmup=2, total=10):
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def perturb(netobj, seed=11):
    g = torch.Generator().manual_seed(seed)
    sd = netobj.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    netobj.load_state_dict(sd)


def _locked_mask(store):
    mask = torch.ones(store.total, dtype=torch.bool)
    for lo, hi in store.trainable_ranges():
        mask[lo:hi] = False
    return mask


def _locked_grad_is_zero(store):
    mask = _locked_mask(store)
    return (not bool(mask.any())) or float(store.grad.detach().cpu()[mask].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 1. the reference's variants
@functools.lru_cache(maxsize=None)
def _train3():
    z = np.load(os.path.join(GOLDEN, "train3_tiny_text.npz"), allow_pickle=False)
    sys.path.insert(0, GOLDEN)
    try:
        from make_golden_accum import p0_digest
    finally:
        sys.path.remove(GOLDEN)
    return {k: z[k] for k in z.files}, p0_digest(z)


def _tiny_text_cfg(c):
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    v, t = c["vision_cfg"], c["text_cfg"]
    return mc.ModelCfg(embed_dim=c["embed_dim"],
                       vision=mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64)),
                       text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)


VARIANTS = {"img0": (0, None), "img2": (2, None), "img0_txt1": (0, 1)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_reference_three_locked_training_steps(variant):
    """Bounds of test_reference_three_training_steps_text_tower: loss 4e-3 (steps 0, 1) / 2e-2 (step 2), pre-clip norm 5 %,
    trainable weights within 3e-3 of the reference's ``p3``; every locked tensor bit-identical to ``p0``; the locked part of the
    gradient buffer exactly zero; step-0 gradients of the trainable tensors within 4 % of the tensor's max-abs -- or, for a tensor
    that misses it, 1.5 x the distance of the reference's own bf16 autocast run from its fp32 run (the fixture's ``ac_rel``,
    profiles/lit_parity.txt) -- minus the 2^-11 the fixture's float16 storage may have moved the expected value by."""
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    z0, digest = _train3()
    z = np.load(os.path.join(GOLDEN, f"train3_tiny_text_lock_{variant}.npz"), allow_pickle=False)
    assert str(z["p0_sha256"]) == digest, "train3_tiny_text.npz was regenerated: regenerate the lock fixtures too"
    cfg = _tiny_text_cfg(json.loads(str(z["cfg"])))
    image, text = VARIANTS[variant]
    p0 = {k[3:]: torch.from_numpy(z0[k]) for k in z0 if k.startswith("p0.")}
    if variant == "img0":       # through the constructor (the Hydra keys); the others through the methods
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, lock_image=True, lock_image_unlocked_groups=image)
        n.load_state_dict(p0)
    else:
        n = net.SpatialClipNet("custom", None, model_cfg=cfg)
        n.load_state_dict(p0)
        n.lock_image_tower(unlocked_groups=image)
        if text is not None:
            n.lock_text_tower(unlocked_layers=text)
    trainable = json.loads(str(z["trainable"]))
    assert sorted(n.trainable_names()) == sorted(trainable)
    assert sorted(k for k, p in n.named_parameters() if p.requires_grad) == sorted(k.replace(".", "__") for k in trainable)
    assert len(list(n.parameters())) == len(n.state_dict()) == len(p0)        # parameters() / state_dict() keep every tensor
    m, opt, sched = _module(n, _spatial(losses), warmup=int(z["warmup"]), total=int(z["total"]))
    assert opt.exp_avg.numel() == n.store.trainable_floats() < n.store.total
    batch = {"images": torch.from_numpy(z0["images"]).cuda(), "texts": torch.from_numpy(z0["texts"]).cuda(),
             "image_tile_ids": torch.from_numpy(z0["ids"]).cuda(), "text_tile_ids": torch.from_numpy(z0["ids"]).cuda(),
             "neighbor_tile_ids": torch.from_numpy(z0["nb"]).cuda(), "neighbor_alphas": torch.from_numpy(z0["alpha"]).cuda()}
    ac_rel = json.loads(str(z["ac_rel"]))
    for step in range(3):
        loss = m.training_step(batch, step)
        loss.backward()
        torch.cuda.synchronize()
        assert _locked_grad_is_zero(n.store), step
        if step == 0:
            bad = []
            for k in trainable:
                top = float(z["g0s." + k])
                g_ref = torch.from_numpy(z["g0." + k].astype(np.float32)) * top
                err = float((n.store.g(k).cpu() - g_ref).abs().max())
                frac = 0.04
                if err > (0.04 - G0_ROUNDING) * top + 1e-6:
                    frac = max(0.04, 1.5 * ac_rel[k])
                print(f"grad {k}: max|d| {err:.3e} of max|ref| {top:.3e} ({err / max(top, 1e-30):.4f}; autocast {ac_rel[k]:.4f})")
                if err > (frac - G0_ROUNDING) * top + 1e-6:
                    bad.append((k, err, top, ac_rel[k]))
            assert not bad, bad
        nc = opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()
        dl, want_n = abs(float(loss.detach()) - float(z["losses"][step])), float(z["grad_norms"][step])
        print(f"step {step}: loss |d| {dl:.3e}; norm {float(nc[0]):.4f} vs {want_n:.4f}")
        assert dl < (4e-3 if step < 2 else 2e-2), (step, float(loss.detach()), float(z["losses"][step]))
        assert abs(float(nc[0]) - want_n) < 0.05 * want_n
    n.store.wait_all()
    torch.cuda.synchronize()
    for k, v in p0.items():
        got = n.store.p(k).cpu()
        if k in trainable:
            d = float((got - torch.from_numpy(z["p3." + k])).abs().max())
            assert d < 3e-3, (k, d)
        else:
            assert torch.equal(got, v), f"locked tensor {k} moved"
    moved = [k for k in trainable if not torch.equal(n.store.p(k).cpu(), p0[k])]
    assert len(moved) == len(trainable)


# ------------------------------------------------------------------------------------------------ 2. every floor position
def _reference_rule(layers, g, names, no_ln_pre=False):
    """requires_grad names after lock_image_tower(g), written out from VisionTransformer.lock (transformer.py:710-741) -- not
    from the package under test; held against the reference's own lists in test_reference_rule_equals_the_manifest."""
    stem = ["visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding"]
    stem += [] if no_ln_pre else ["visual.ln_pre.weight", "visual.ln_pre.bias"]
    block = lambda i: [k for k in names if k.startswith(f"visual.transformer.resblocks.{i}.")]
    groups = [stem] + [block(i) for i in range(layers - 1)] + [block(layers - 1) + ["visual.ln_post.weight", "visual.ln_post.bias"]]
    groups.append(["visual.proj"])
    free = set(k for k in names if not k.startswith("visual."))
    if g != 0:
        free |= set(k for grp in groups[-g:] for k in grp)
    return free


def test_reference_rule_equals_the_manifest():
    with open(os.path.join(GOLDEN, "lock_groups_manifest.json")) as f:
        man = json.load(f)
    layers = man["cfg"]["vision_cfg"]["layers"]
    names = man["image"][str(layers + 3)]
    for g in range(layers + 4):
        assert _reference_rule(layers, g, names) == set(man["image"][str(g)]), g


def _gene_cfgs(layers, flags, drop=None):
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, layers, 32, 4.0, **flags), text=None, gene=mc.GeneCfg(100, 64))
    ocfg = O.ModelCfg(embed_dim=32, vision=O.VisionCfg(32, 8, 64, layers, 32, 4.0), text=None, gene=O.GeneCfg(100, 64))
    return cfg, ocfg


class _OracleLoop:
    """O.OracleTrainer's step (clip 1.0, AdamW, cosine warm-up) over the pool oracle's forward, AdamW over the tensors with a
    gradient only -- what torch.optim.AdamW does with requires_grad=False parameters."""

    def __init__(self, ocfg, params, free, flags, warmup=2, total=10):
        self.ocfg, self.flags, self.warmup, self.total, self.t = ocfg, flags, warmup, total, 0
        self.p = {k: v.clone().float().requires_grad_(k in free) for k, v in params.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}

    def loss(self, batch, keep, autocast=False):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f = PO.net_forward(batch["images"], batch["texts"], self.p, self.ocfg, keep=keep, **self.flags)
            return O.spatial_loss(f["image_features"], f["text_features"], f["logit_scale"], batch["image_tile_ids"],
                                  batch["text_tile_ids"], batch["neighbor_tile_ids"], batch["neighbor_alphas"])

    def grads(self, batch, keep, autocast=False):
        for v in self.p.values():
            v.grad = None
        lo = self.loss(batch, keep, autocast)
        lo.backward()
        return lo, {k: v.grad.detach().clone().float() for k, v in self.p.items() if v.grad is not None}

    def step(self, batch, keep):
        lo, g = self.grads(batch, keep)
        assert all(self.p[k].grad is None for k in self.p if not self.p[k].requires_grad)
        norm = O.clip_grad_norm([self.p[k].grad for k in g], 1.0)
        lr = 1e-3 * O.cosine_warmup_lambda(self.t, self.warmup, self.total)
        self.t += 1
        with torch.no_grad():
            for k in g:
                O.adamw_step(self.p[k], self.p[k].grad, self.m[k], self.v[k], self.t, lr, 0.9, 0.98, 1e-6, 0.1)
        return float(lo.detach()), float(norm), g


FLOORS = [(2, g, "tok", "bf16", None, False) for g in range(5)] + [(2, g, "avg", "fp32", None, False) for g in range(5)]
FLOORS += [(4, 3, "tok", "fp32", None, False), (4, 4, "avg", "bf16", None, False),       # a floor in the middle of the stack
           (2, 2, "tok", "bf16", 0.5, False), (2, 3, "avg", "bf16", None, True), (4, 2, "tok", "bf16", None, True)]


@pytest.mark.parametrize("layers,g,pool,stream,drop,recompute", FLOORS)
def test_every_floor_position_vs_oracle(layers, g, pool, stream, drop, recompute):
    """``unlocked_groups`` 0 .. layers + 2 on a ``-gene`` model: three steps against the fp32 oracle whose ``requires_grad``
    follows the reference's rule, with the bounds of test 1.  A gradient that misses 4 % is held to 1.5 x the distance of the
    same oracle composition under torch.autocast(bfloat16) from fp32 (profiles/lit_parity.txt)."""
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    flags = {} if pool == "tok" else {"pool_type": "avg"}
    cfg, ocfg = _gene_cfgs(layers, flags)
    B, seed = 12, 3
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, residual_stream=stream, force_patch_dropout=drop,
                           grad_checkpointing=recompute, lock_image=True, lock_image_unlocked_groups=g)
    perturb(n)
    params = {k: v.cpu() for k, v in n.state_dict().items()}
    free = _reference_rule(layers, g, list(params))
    assert set(n.trainable_names()) == free
    assert n.vision.stack.floor == (max(0, layers + 1 - g) if g >= 2 else layers) and n.training
    tr = _OracleLoop(ocfg, params, free, flags)
    m, opt, sched = _module(n, _spatial(losses))
    n_patch = cfg.vision.tokens - 1
    for step in range(3):
        batch = data.synthetic_batch(B, 32, cfg.gene.n_genes, K=4, step=step)
        keep = pd.keep_indices_host(seed, step, 0, B, n_patch, pd.num_keep(n_patch, drop)) if drop else None
        ref_loss, ref_norm, g_ref = tr.step(batch, keep)
        loss = m.training_step({k: v.cuda() for k, v in batch.items()}, step)
        if drop:        # locking does not change train / eval mode: the locked tower still drops in a training forward
            assert n.vision.L_run == keep.shape[1] + 1 and np.array_equal(n.vision.keep_idx.cpu().numpy(), keep)
        loss.backward()
        torch.cuda.synchronize()
        assert _locked_grad_is_zero(n.store), step
        if step == 0:
            bad, yard = [], None
            for k in sorted(free):
                top = float(g_ref[k].abs().max())
                err = float((n.store.g(k).cpu() - g_ref[k]).abs().max())
                frac = 0.04
                if err > 0.04 * top + 1e-6:
                    if yard is None:        # the same oracle composition under the reference's own bf16 policy
                        _, g_ac = _OracleLoop(ocfg, params, free, flags).grads(batch, keep, autocast=True)
                        yard = {q: float((g_ac[q] - g_ref[q]).abs().max() / g_ref[q].abs().max().clamp_min(1e-30)) for q in g_ref}
                    frac = max(0.04, 1.5 * yard[k])
                    print(f"yardstick {k}: autocast distance {yard[k]:.4f}")
                print(f"grad {k}: max|d| {err:.3e} of max|ref| {top:.3e} ({err / max(top, 1e-30):.4f})")
                if err > frac * top + 1e-6:
                    bad.append((k, err, top))
            assert not bad, bad
        nc = opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()
        dl = abs(float(loss.detach()) - ref_loss)
        print(f"step {step}: loss |d| {dl:.3e}; norm {float(nc[0]):.4f} vs {ref_norm:.4f}")
        assert dl < (4e-3 if step < 2 else 2e-2), (step, float(loss.detach()), ref_loss)
        assert abs(float(nc[0]) - ref_norm) < 0.05 * ref_norm
    n.store.wait_all()
    torch.cuda.synchronize()
    for k, v in params.items():
        got = n.store.p(k).cpu()
        if k in free:
            d = float((got - tr.p[k].detach()).abs().max())
            assert d < 3e-3, (k, d)
        else:
            assert torch.equal(got, v), f"locked tensor {k} moved"
            assert torch.equal(tr.p[k].detach(), v)


# ------------------------------------------------------------------------------------------------ 3. step forms
def _locked_gene_net(g=2, layers=2, seed=3, **kw):
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    cfg, _ = _gene_cfgs(layers, {})
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed, **kw)
    perturb(n)
    if g is not None:
        n.lock_image_tower(g)
    return n


def _gene_batch(B, step):
    comm, data, *_ = _pkg()
    return {k: v.cuda() for k, v in data.synthetic_batch(B, 32, 100, K=4, step=step).items()}


@pytest.mark.parametrize("g", [0, 2])
def test_step_forms_are_bit_identical_with_a_lock(monkeypatch, g):
    """SC_ADAMW_BEHIND=1, SC_ADAMW_BEHIND=0 and the graphed step: the same weights and moments after four steps.  The loss is
    read after every step, as tests/test_gpu_graph.py does: replays with no host synchronisation between them are outside what
    FusedAdamW.refresh_hyper's single pinned staging triple holds, with or without a lock."""
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    steps = 4
    batches = [_gene_batch(12, s) for s in range(steps)]
    res, losses_of = {}, {}
    for form in ("behind", "one_launch", "graph"):
        monkeypatch.setenv("SC_ADAMW_BEHIND", "1" if form == "behind" else "0")
        n = _locked_gene_net(g)
        p0 = n.store.master.detach().clone()
        m, opt, sched = _module(n, _spatial(losses), warmup=1)
        gstep = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        assert gstep.capturable() is None
        ls = []
        for b in batches:
            loss = gstep(b) if form == "graph" else gstep.eager(b)
            sched.step()
            ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        if form == "graph":
            assert gstep.failed is None and gstep.replays == steps - 1, (gstep.failed, gstep.replays)
        mask = _locked_mask(n.store).cuda()
        assert torch.equal(n.store.master[mask], p0[mask]) and not torch.equal(n.store.master[~mask], p0[~mask])
        assert float(n.store.grad[mask].abs().max()) == 0.0
        res[form] = (n.store.master.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), n.store.master_bf16.clone())
        losses_of[form] = ls
    assert losses_of["behind"] == losses_of["one_launch"] == losses_of["graph"], losses_of
    for form in ("one_launch", "graph"):
        for a, b, what in zip(res["behind"], res[form], ("weights", "exp_avg", "exp_avg_sq", "bf16 mirror")):
            diff = (a != b).nonzero().flatten()
            where = "" if not diff.numel() else f": {diff.numel()} of {a.numel()} elements, first at {int(diff[0])}, " \
                f"max|d| {float((a.float() - b.float()).abs().max()):.3e}"
            assert not diff.numel(), f"{what}: {form} differs from the update behind the forward{where}"


def test_accumulated_step_equals_two_half_weighted_micro_batches_with_a_lock(monkeypatch):
    """accumulate_grad_batches = 2 with a lock, to the bound of tests/test_gpu_grad_accum.py::test_fold_composes_with_the_
    backward_of_a_real_net: the folded gradient is bit-equal to gA / 2 + gB / 2, the clip norm left by the fold is the norm of
    that sum, and neither the locked part of the gradient buffer nor of the running sum is written."""
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    n = _locked_gene_net(2)
    m, opt, sched = _module(n, _spatial(losses), warmup=0)
    A, B = _gene_batch(12, 11), _gene_batch(12, 23)
    store = n.store

    def backward(batch):
        with streams.chain_stream():
            loss = m.training_step(batch, 0)
            loss.backward(m.root_gradient(loss))

    def alone(batch):
        backward(batch)
        torch.cuda.synchronize()
        return store.grad.detach().cpu().clone()

    gA, gB = alone(A), alone(B)
    assert float(gA.abs().max()) > 0 and not torch.equal(gA, gB) and torch.equal(alone(A), gA)
    acc = optim.GradAccumulator(store, 2)
    partial = acc.sumsq_partial()
    assert partial.numel() == 1024 * len(store.trainable_ranges())
    with streams.chain_stream():
        backward(A)
        acc.fold(True, False)
        backward(B)
        acc.fold(False, True, partial=partial)
        torch.cuda.synchronize()
        half = torch.tensor(0.5)
        want = gA * half + gB * half
        assert torch.equal(store.grad.detach().cpu(), want)
        mask = _locked_mask(store)
        assert float(want[mask].abs().max()) == 0.0 and float(acc.acc.cpu()[mask].abs().max()) == 0.0
        p_before = store.master.detach().clone()
        nc = opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
    store.wait_all()
    torch.cuda.synchronize()
    ref_norm = float(want.double().norm())
    assert abs(float(nc[0]) - ref_norm) < 1e-5 * ref_norm
    assert torch.equal(store.master[mask.cuda()], p_before[mask.cuda()])
    # the same step from the gradient itself (no partials): same weights, bit for bit
    n2 = _locked_gene_net(2)
    m2, opt2, _ = _module(n2, _spatial(losses), warmup=0)
    n2.store.grad.copy_(want.cuda())
    opt2.step(grad_scale=1.0, max_norm=1.0)
    n2.store.wait_all()
    torch.cuda.synchronize()
    assert torch.equal(n2.store.master, store.master)


# ------------------------------------------------------------------------------------------------ 4. activation memory
def test_locked_prefix_keeps_no_activations_per_block():
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    b = _gene_batch(12, 0)

    def stack_bytes(layers, g):
        n = _locked_gene_net(g, layers)
        m, _, _ = _module(n, _spatial(losses))
        loss = m.training_step(b, 0)
        loss.backward()
        torch.cuda.synchronize()
        return n.vision.stack.bufs.bytes()

    locked2, locked6, free2 = stack_bytes(2, 0), stack_bytes(6, 0), stack_bytes(2, None)
    print(f"vision stack buffers: locked 2 layers {locked2} B, locked 6 layers {locked6} B, unlocked 2 layers {free2} B")
    assert locked2 == locked6 < free2
    # two trainable blocks on top of a locked prefix: the prefix still costs the same two rotating sets
    assert stack_bytes(6, 3) - stack_bytes(4, 3) == 0


# ------------------------------------------------------------------------------------------------ 5. forced distributed path
def _dist_worker(rank, world, port, force, ret):
    sys.path.insert(0, ROOT)
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1",
                       "SC_FORCE_DIST": "1" if force else "0", "SC_COMM_NATIVE": "0", "SC_GRAD_EXCHANGE": "allreduce"})
    comm, data, graph, losses, mc, module, net, optim, pd, streams = _pkg()
    comm.init_from_env()
    assert comm.is_dist() == bool(force)
    n = _locked_gene_net(2)
    m, opt, sched = _module(n, _spatial(losses), warmup=1)
    reducer = comm.make_grad_exchange(n.store, bucket_floats=20000)
    assert (reducer is not None) == bool(force)
    n.grad_bucket_hook = reducer.bucket_ready if reducer is not None else None
    opt.attach_exchange(reducer)
    comm.reset_stats()
    for s in range(3):
        loss = m.training_step(_gene_batch(12, s), s)
        loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()
    n.store.wait_all()
    torch.cuda.synchronize()
    ret[bool(force)] = {"w": n.store.master.detach().cpu(), "trainable": n.store.trainable_floats(), "total": n.store.total,
                        "stats": {k: list(v) for k, v in comm.STATS.items()}}
    comm.shutdown()


def test_forced_one_rank_group_reduces_the_trainable_floats_only():
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_dist_worker, args=(1, 29761, True, ret), nprocs=1, join=True)
        mp.spawn(_dist_worker, args=(1, 29762, False, ret), nprocs=1, join=True)
        res = dict(ret)
    launches, nbytes = res[True]["stats"]["all_reduce(gradient bucket)"]
    assert res[True]["trainable"] < res[True]["total"]
    assert nbytes == 3 * 4 * res[True]["trainable"], (nbytes, res[True]["trainable"])
    assert launches >= 3
    assert torch.equal(res[True]["w"], res[False]["w"])


# ------------------------------------------------------------------------------------------------ 6. the unlocked net
def test_unlocked_net_gives_the_parents_bits_and_launches():
    """tests/golden/lock_parent_bits.json was recorded on an MI355X from the commit in front of this feature
    (tests/golden/make_golden_lock_parent.py): three steps of a net without a lock give the same weights, moments, losses and
    norms, bit for bit, and the third step calls the same library entry points in the same order, in both step forms."""
    _pkg()
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_lock_parent as P
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "lock_parent_bits.json")) as f:
        want = json.load(f)
    log = P.CallLog()
    try:
        for behind in ("1", "0"):
            got, ref = P.three_steps(behind, log), want[f"behind={behind}"]
            assert got["calls"] == ref["calls"], [(i, a, b) for i, (a, b) in enumerate(zip(got["calls"], ref["calls"])) if a != b][:5]
            assert got["losses"] == ref["losses"] and got["norms"] == ref["norms"]
            for k in ("master", "exp_avg", "exp_avg_sq"):
                assert got[k] == ref[k], f"{k} after three steps (SC_ADAMW_BEHIND={behind}) differs from the parent commit's"
    finally:
        log.restore()
