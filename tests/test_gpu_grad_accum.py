"""Gradient accumulation on the device (Trainer accumulate_grad_batches): sc_grad_accumulate bit for bit against PyTorch's
fp32 ``acc + scale * g`` on a CPU, its sums of squares against float64, the fold composed with a real net's backward, the
reference's own accumulated run (tests/golden/make_golden_accum.py) and the Trainer's loop, counters and resume."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import _refbounds as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 8                      # NaN floats kept in front of and behind every slice
THIRD = 1.0 / 3.0


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, model_configs as mc, module, net, ops, optim, streams
    return data, losses, mc, module, net, ops, optim, streams


def _bits(t):
    return t.contiguous().view(torch.int32)


def _expected(acc, g, scale, mode, has_acc):
    """(acc after, grads after) by PyTorch's fp32 arithmetic on the CPU: the product and the sum are separate operations."""
    prod = g * torch.tensor(scale, dtype=torch.float32)
    if mode == 0:
        return prod, g
    if mode == 1:
        return acc + prod, g
    return acc, (acc + prod if has_acc else prod)


# ---------------------------------------------------------------------------------------------- kernel, bit-exact
KERNEL_N = [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 262144 * 4 + 7]   # the last: one element past a full stride of the capped grid
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0), (2, 3), (3, 0)]     # (acc, grads) start, in floats: alike and different
MODES = [(0, True), (1, True), (2, True), (2, False)]                          # (mode, acc given)


# past four full strides of the capped grid (1024 x 256 threads x 4 floats): one launch runs the 4x-unrolled vector loop (the loop
# a real model's fold spends its time in), then the single-vector remainder loop (300 vectors), then the scalar tail (3 floats)
UNROLLED_N = 4 * 262144 * 4 + 4 * 300 + 3


def _check_kernel(n, offsets, scales):
    *_, ops, _, _ = _pkg()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(n)
    a0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3.0
    a0d, g0d = a0.to(dev), g0.to(dev)
    size = n + 2 * GUARD + 3
    bad = []
    for oa, og in offsets:
        for scale in scales:
            for mode, has_acc in MODES:
                abuf = torch.full((size,), NAN, device=dev)
                gbuf = torch.full((size,), NAN, device=dev)
                sa, sg = slice(GUARD + oa, GUARD + oa + n), slice(GUARD + og, GUARD + og + n)
                abuf[sa] = a0d
                gbuf[sg] = g0d
                ops.grad_accumulate(abuf[sa] if has_acc else None, gbuf[sg], n, scale, mode)
                want_a, want_g = torch.full((size,), NAN), torch.full((size,), NAN)
                want_a[sa], want_g[sg] = _expected(a0, g0, scale, mode, has_acc)     # acc untouched in mode 2, grads in 0 / 1
                if not (torch.equal(_bits(abuf.cpu()), _bits(want_a)) and torch.equal(_bits(gbuf.cpu()), _bits(want_g))):
                    bad.append((oa, og, scale, mode, has_acc))
    assert not bad, f"n={n}: (acc offset, grads offset, scale, mode, acc given) with wrong bits or touched guards: {bad[:8]}"


@pytest.mark.parametrize("n", KERNEL_N)
def test_kernel_is_bit_exact_and_stays_inside_its_slice(n):
    _check_kernel(n, OFFSETS, (0.5, THIRD, 1.0))


def test_kernel_unrolled_vector_loop_is_bit_exact():
    """16-byte aligned slices (GUARD floats into a fresh allocation), every mode and acc=None: the vector kernel's three loops."""
    assert GUARD % 4 == 0 and UNROLLED_N // 4 > 4 * 1024 * 256
    _check_kernel(UNROLLED_N, [(0, 0)], (THIRD,))


def test_kernel_refusals_launch_nothing():
    *_, ops, _, _ = _pkg()
    from spatial_clip_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    a, g = torch.ones(8, device=dev), torch.full((8,), 2.0, device=dev)
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    assert l.sc_grad_accumulate(a.data_ptr(), g.data_ptr(), 8, 0.5, 3, None, st) != 0 and b"mode" in l.sc_last_error()
    assert l.sc_grad_accumulate(a.data_ptr(), g.data_ptr(), 8, 0.5, -1, None, st) != 0
    assert l.sc_grad_accumulate(a.data_ptr(), None, 8, 0.5, 1, None, st) != 0 and b"grads" in l.sc_last_error()
    assert l.sc_grad_accumulate(None, g.data_ptr(), 8, 0.5, 0, None, st) != 0
    assert l.sc_grad_accumulate(a.data_ptr(), g.data_ptr(), 0, 0.5, 1, None, st) == 0          # n == 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), torch.ones(8)) and torch.equal(g.cpu(), torch.full((8,), 2.0))


# ---------------------------------------------------------------------------------------------- partial sums of squares
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [5, 1025, 4097, 1_048_583, UNROLLED_N])      # the last: the unrolled loop's s4[] sums
def test_partials_give_the_norm_and_clip_of_the_summed_gradient(n, off):
    *_, ops, _, _ = _pkg()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(7 * n + off)
    a0, g0 = torch.randn(n, generator=gen) * 1e-2, torch.randn(n, generator=gen) * 1e-2
    if n % 4:                                   # a heavy tail: dropping or doubling it moves the norm far beyond the bound
        g0[n - (n % 4):] = 1e-2 * float(n) ** 0.5
    _, want = _expected(a0, g0, THIRD, 2, True)
    norm64 = float(want.double().norm())
    a = torch.full((n + 4,), NAN, device=dev)
    a[off:off + n] = a0.to(dev)
    parts = []
    for rep in range(2):
        g = torch.full((n + 4,), NAN, device=dev)
        g[off:off + n] = g0.to(dev)
        partial = torch.full((1024,), NAN, dtype=torch.float64, device=dev)
        ops.grad_accumulate(a[off:off + n], g[off:off + n], n, THIRD, 2, partial)
        parts.append(partial.clone())
        assert torch.equal(_bits(g[off:off + n].cpu()), _bits(want))          # the same gradient as without partials
    assert torch.equal(parts[0], parts[1]), "the partial sums must not depend on the run"
    assert bool(torch.isfinite(parts[0]).all())
    for gs, max_norm in ((1.0, 0.5 * norm64), (0.5, 2.0 * norm64), (1.0, 0.0)):      # clips / does not / clipping off
        out = torch.full((2,), NAN, device=dev)
        ops.grad_norm_final(parts[0], 1024, gs, max_norm, out)
        got_norm, got_clip = float(out[0]), float(out[1])
        ref_norm = norm64 * gs
        clip64 = 1.0 if max_norm <= 0 else min(1.0, max_norm / (ref_norm + 1e-6))
        rel, crel = abs(got_norm - ref_norm) / ref_norm, abs(got_clip - clip64) / clip64
        print(f"  n={n} off={off} gs={gs} max_norm={max_norm:.4g}: norm rel err {rel:.3g} (bound {R.GRAD_NORM_REL:g}), "
              f"clip {got_clip:.7g} rel err {crel:.3g} (bound {R.CLIP_REL:.3g})")
        assert rel <= R.GRAD_NORM_REL
        if clip64 == 1.0:
            assert got_clip == 1.0
        else:
            assert crel <= R.CLIP_REL and got_clip < 1.0


# ---------------------------------------------------------------------------------------------- composition on a real net
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}


def _p0_digest(golden_dir, name):
    """make_golden_accum.p0_digest: SHA-256 over the p0.* names and bytes, in name order."""
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


def _spatial_module(n, warmup=2, total=10):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                 neighbor_alpha_scale=0.5, float32_logits=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def test_fold_composes_with_the_backward_of_a_real_net(golden_dir, monkeypatch):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")       # weight gradients on the side stream: the fold must sit behind its join
    n, cfg = _tiny_text_net(golden_dir)
    m, _, _ = _spatial_module(n)
    batches = []
    for seed in (11, 23):
        b = data.synthetic_batch(6, cfg.vision.image_size, 64, K=4, step=seed)
        b["texts"] = data.synthetic_captions(6, cfg.text.context_length, cfg.text.vocab_size, seed=seed)
        batches.append({k: v.cuda() for k, v in b.items()})
    A, B = batches
    store = n.store

    def backward(batch):
        loss = m.training_step(batch, 0)
        loss.backward(m.root_gradient(loss))

    def alone(batch):
        with streams.chain_stream():
            backward(batch)
        torch.cuda.synchronize()
        return store.grad.detach().cpu().clone()

    gA, gB = alone(A), alone(B)
    assert float(gA.abs().max()) > 0 and not torch.equal(gA, gB)
    assert torch.equal(alone(A), gA), "the backward itself is not bit-reproducible: nothing below can hold"

    def group(every, members):
        acc = optim.GradAccumulator(store, every)
        with streams.chain_stream():
            for k, batch in enumerate(members):
                backward(batch)
                acc.fold(k == 0, k == len(members) - 1)
        torch.cuda.synchronize()
        return store.grad.detach().cpu().clone(), acc

    half, third = torch.tensor(0.5), torch.tensor(THIRD, dtype=torch.float32)
    got, acc = group(2, [A, B])
    assert torch.equal(got, gA * half + gB * half)
    assert acc.acc is not None and torch.equal(acc.acc.cpu(), gA * half)        # the last fold leaves the running sum alone
    got, _ = group(3, [A, B])                                                   # a short last group at N = 3: weights 1/3 each
    assert torch.equal(got, gA * third + gB * third)
    got, acc = group(2, [A])                                                    # a group of one at N = 2
    assert torch.equal(got, gA * half) and acc.acc is None


# ---------------------------------------------------------------------------------------------- the reference's accumulated run
BOUNDED = ("visual.proj", "text_projection", "token_embedding.weight", "visual.conv1.weight")


def _drive(golden_dir, z, every):
    """module + GradAccumulator + FusedAdamW + scheduler over the fixture's five batches; every = 1 is the plain loop."""
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    from spatial_clip_amd.trainer import accum_steps_after
    n, _ = _tiny_text_net(golden_dir)
    m, opt, sched = _spatial_module(n, warmup=int(z["warmup"]), total=int(z["total"]))
    acc = optim.GradAccumulator(n.store, every) if every > 1 else None
    steps_after = accum_steps_after(5, every)
    losses_, norms = [], []
    for i in range(5):
        batch = {"images": z[f"b{i}.images"].cuda(), "texts": z[f"b{i}.texts"].cuda(), "image_tile_ids": z[f"b{i}.ids"].cuda(),
                 "text_tile_ids": z[f"b{i}.ids"].cuda(), "neighbor_tile_ids": z[f"b{i}.nb"].cuda(),
                 "neighbor_alphas": z[f"b{i}.alpha"].cuda()}
        with streams.chain_stream():
            loss = m.training_step(batch, i)
            loss.backward(m.root_gradient(loss))
            if acc is not None:
                partial = acc.sumsq_partial() if steps_after[i] else None
                acc.fold(i % every == 0, steps_after[i], partial=partial)
                if steps_after[i]:
                    nc = opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
            else:
                nc = opt.step(grad_scale=1.0, max_norm=1.0)
        losses_.append(float(loss.detach()))
        if steps_after[i]:
            sched.step()
            norms.append(float(nc[0]))
    n.store.wait_all()
    torch.cuda.synchronize()
    return losses_, norms, {k: n.store.p(k).detach().cpu().clone() for k in BOUNDED}, opt, sched


def test_reference_accumulated_training_text_tower(golden_dir):
    """Five micro-batches at N = 2 against the reference's own classes in fp32 (Lightning's loop written out:
    tests/golden/make_golden_accum.py), bounded by the constants of test_reference_three_training_steps_text_tower or 1.5 x
    (parity.small_batch_loss_bound's factor) what the reference's bf16 autocast run deviates by, whichever is larger.

    Measured on an MI355X, this build / the autocast yardstick: see DESIGN.md "Gradient accumulation"."""
    z = _load(golden_dir, "train_accum2_tiny_text.npz")
    assert int(z["every"]) == 2 and str(z["p0_from"]) == "train3_tiny_text.npz"
    assert _p0_digest(golden_dir, "train3_tiny_text.npz") == str(z["p0_sha256"]), \
        "train3_tiny_text.npz no longer holds the starting weights this fixture was generated from: regenerate it too"
    losses_, norms, params, opt, sched = _drive(golden_dir, z, 2)
    assert opt.step_count == 3 and sched.last_epoch == 3 and len(norms) == 3
    steps_before = [0, 0, 1, 1, 2]              # optimiser steps taken before micro-batch i
    fails = []
    for i in range(5):
        ref, ac = float(z["losses"][i]), float(z["autocast_losses"][i])
        bound = max(4e-3 if steps_before[i] == 0 else 2e-2, 1.5 * abs(ac - ref))
        d = abs(losses_[i] - ref)
        print(f"  loss[{i}] {losses_[i]:.6f} ref {ref:.6f} |d| {d:.3g} autocast |d| {abs(ac - ref):.3g} bound {bound:.3g}")
        if d > bound:
            fails.append(("loss", i, d, bound))
    for s in range(3):
        ref, ac = float(z["grad_norms"][s]), float(z["autocast_grad_norms"][s])
        bound = max(0.05, 1.5 * abs(ac - ref) / ref)
        d = abs(norms[s] - ref) / ref
        print(f"  grad_norm[{s}] {norms[s]:.5f} ref {ref:.5f} rel {d:.3g} autocast rel {abs(ac - ref) / ref:.3g} bound {bound:.3g}")
        if d > bound:
            fails.append(("grad_norm", s, d, bound))
    bounds = {}
    for k in BOUNDED:
        ac_dev = float((z["autocast_pN." + k] - z["pN." + k]).abs().max())
        bounds[k] = max(3e-3, 1.5 * ac_dev)
        d = float((params[k] - z["pN." + k]).abs().max())
        print(f"  {k}: max|d| {d:.3g} autocast max|d| {ac_dev:.3g} bound {bounds[k]:.3g}")
        if d > bounds[k]:
            fails.append((k, d, bounds[k]))
    assert not fails, fails
    # the fixture tells the feature from its absence: the same HIP code stepping after every batch misses a parameter bound
    _, _, plain, opt1, _ = _drive(golden_dir, z, 1)
    assert opt1.step_count == 5
    dev1 = {k: float((plain[k] - z["pN." + k]).abs().max()) for k in BOUNDED}
    print("  N = 1 over the same batches:", {k: f"{v:.3g}" for k, v in dev1.items()})
    assert any(dev1[k] > bounds[k] for k in BOUNDED), (dev1, bounds)


# ---------------------------------------------------------------------------------------------- Trainer
def _text_dm(data):
    class TextDM(data.SyntheticSpatialDataModule):
        def _loader(self, n, offset):
            for s in range(n):
                B = self.batch_size if s + 1 < n else self.batch_size - 5           # ragged last batch of the epoch
                b = data.synthetic_batch(B, self.image_size, 64, self.k_neighbors, offset + s)
                b["texts"] = data.synthetic_captions(B, 16, 97, seed=offset + s)
                yield b
    return TextDM(batch_size=16, image_size=32, n_genes=64, k_neighbors=4, steps_per_epoch=5, val_steps=1)


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


def _fit(ckpt_path=None, **kw):
    data, *_ = _pkg()
    from spatial_clip_amd.trainer import Trainer
    n, m = _trainer_module()
    tr = Trainer(max_epochs=1, gradient_clip_val=1.0, log_every_n_steps=1, **kw)
    tr.fit(m, _text_dm(data), ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    return n, m, tr


@pytest.fixture(scope="module")
def accumulated_fit():
    """The uninterrupted run at N = 2 over five batches, shared (and left unchanged) by the trainer tests."""
    old = {k: os.environ.get(k) for k in ("SC_OVERLAP", "SC_GRAPH")}
    os.environ.update(SC_OVERLAP="1", SC_GRAPH="1")     # SC_GRAPH=1 asks for a captured step: an accumulated one stays eager
    try:
        n, m, tr = _fit(accumulate_grad_batches=2)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return n.store.master.detach().clone(), tr


def test_trainer_counts_optimiser_steps(accumulated_fit):
    w, tr = accumulated_fit
    assert tr.global_step == 3 and tr.optimizer.step_count == 3 and tr.scheduler.last_epoch == 3
    assert tr.estimated_stepping_batches == 3 and tr.graphed_step is None
    recs = [h for h in tr.history if "train/loss" in h and "epoch" not in h]
    assert [h["step"] for h in recs] == [1, 2, 3]
    assert tr.accumulator is not None and tr.accumulator.acc.numel() == tr.optimizer.store.total


def test_trainer_equals_the_hand_driven_loop(accumulated_fit, monkeypatch):
    data, losses, mc, module, net, ops, optim, streams = _pkg()
    from spatial_clip_amd.trainer import accum_steps_after
    monkeypatch.setenv("SC_OVERLAP", "1")
    w, tr = accumulated_fit
    n, m = _trainer_module()

    class T:
        max_steps, max_epochs, estimated_stepping_batches = -1, 1, 3
    m.trainer = T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    dm = _text_dm(data)
    dm.preprocess_fn, dm.tokenizer = n.preprocess_train, n.tokenizer
    dm.setup("fit")
    acc = optim.GradAccumulator(n.store, 2)
    steps_after = accum_steps_after(5, 2)
    last_loss = []
    for i, batch in enumerate(dm.train_dataloader()):
        batch = {k: v.cuda() for k, v in batch.items()}
        with streams.chain_stream():
            loss = m.training_step(batch, i)
            loss.backward(m.root_gradient(loss))
            partial = acc.sumsq_partial() if steps_after[i] else None
            acc.fold(i % 2 == 0, steps_after[i], partial=partial)
            if steps_after[i]:
                opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
        if steps_after[i]:
            sched.step()
            last_loss.append(float(loss.detach()))
    n.store.wait_all()
    torch.cuda.synchronize()
    assert torch.equal(n.store.master.detach(), w)
    recs = [h["train/loss"] for h in tr.history if "train/loss" in h and "epoch" not in h]
    assert recs == last_loss                    # the unscaled loss of each group's last micro-batch


def test_trainer_default_is_the_plain_loop(accumulated_fit, monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    w2, _ = accumulated_fit
    n0, _, tr0 = _fit()
    n1, _, tr1 = _fit(accumulate_grad_batches=1)
    assert tr0.global_step == tr1.global_step == 5 and tr1.estimated_stepping_batches == 5
    assert torch.equal(n0.store.master.detach(), n1.store.master.detach())
    assert tr1.accumulator is None and tr0.accumulator is None          # no running-sum buffer at N = 1
    assert not torch.equal(n1.store.master.detach(), w2)                # and accumulation is not a no-op


def test_trainer_resumes_between_groups(accumulated_fit, monkeypatch, tmp_path):
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    w, _ = accumulated_fit
    # max_steps=2 sizes the first leg's cosine schedule for 2 steps, the uninterrupted run's is sized for 3: the weights can
    # match only because both of the first leg's steps fall inside the 2-step warm-up (_trainer_module), where the LR is
    # step / warm-up and the total does not enter.  The second leg (max_steps=3) is sized like the uninterrupted run.
    n, m, tr = _fit(accumulate_grad_batches=2, max_steps=2)
    assert tr.global_step == 2 and tr.optimizer.step_count == 2
    path = str(tmp_path / "two_steps.ckpt")
    Trainer.save_checkpoint(path, m, tr.optimizer, tr.scheduler, tr.global_step)
    n2, _, tr2 = _fit(ckpt_path=path, accumulate_grad_batches=2, max_steps=3)
    assert tr2.global_step == 3 and tr2.optimizer.step_count == 3 and tr2.scheduler.last_epoch == 3
    assert torch.equal(n2.store.master.detach(), w)
