"""Lion on the device: the three launch forms of lion_kernel (spatial-clip_amd/csrc/sc_optim.hip) against the float64 formula,
then ``optim.FusedLion`` through a real net in every step form.

Kernel (tests/_lioncases.py states the rule and its tie band; tests/test_cpu_lion.py holds torch's fp32 evaluation to it on these
inputs): sizes of one slot, five slots and one past the 4096 x 256 x 4 grid cap, with and without a clip coefficient near 0.5,
with and without the bf16 mirror; exact zeros stay exact zeros under weight decay; ``lr = 0``; the device-``lr`` form and the
grouped form carry the bits of ``sc_lion_step``; every refusal writes nothing.

Through the net (width 64, 2 layers, image 32, patch 8, gene MLP, B = 12): one step against the host formula on the net's own
gradient (a plumbing check of scale, clip, ranges and mirror, not an oracle training run: a sign update turns the 4 % gradient
tolerance into whole ``lr`` steps); the step forms agree bit for bit; a locked tower; open_clip's no-decay groups; an
accumulated step of the Trainer; twenty steps on one batch lower the loss."""
import functools

import pytest
import torch

from tests import _groupcases as C
from tests import _lioncases as L

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _clip_coefficient(ops, gd, g, n):
    """norm_clip with a clip coefficient near 0.5: max_norm is half the norm of the scaled gradient."""
    nc = torch.full((2,), NAN, device=gd.device)
    ops.grad_norm(gd, n, L.GS, 0.5 * float(g.double().norm()) * L.GS, nc)
    return nc


# ================================================================================================ kernel
KERNEL_CASES = [(n, clip, mirror) for n in L.SIZES for clip in (False, True) for mirror in (True, False)]


@pytest.mark.parametrize("n,clip,with_mirror", KERNEL_CASES,
                         ids=[f"n{n}-" + ("clip" if c else "noclip") + ("-mirror" if m else "-nomirror") for n, c, m in KERNEL_CASES])
def test_lion_step_meets_the_float64_rule(n, clip, with_mirror):
    ops, dev = _ops(), _dev()
    p, m = L.start(n)
    pd, md = p.to(dev), m.to(dev)
    for k, lr in enumerate(L.STEPS):
        g = L.grad(n, k)
        gd = g.to(dev)
        nc = _clip_coefficient(ops, gd, g, n) if clip else None
        p0, m0 = pd.cpu(), md.cpu()
        mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        ops.lion_step(pd, gd, md, n, lr, L.B1, L.B2, L.WD, L.GS, nc, mirror if with_mirror else None)
        torch.cuda.synchronize()
        c = float(nc[1]) if clip else 1.0
        if clip:
            assert 0.4 < c < 0.6
        L.check_step(f"n={n} step {k}", pd, md, p0, m0, g, c, lr, L.WD)
        if with_mirror:
            assert torch.equal(_bits(mirror.cpu()), _bits(pd.cpu().to(torch.bfloat16))), f"step {k}: mirror != bf16(p)"
        else:
            assert bool((mirror == -1000.0).all()), f"step {k}: a buffer that was not passed was written"
        if n >= 5 * L.SLOT:
            s = L.slot(L.MOMENT_ONLY_SLOT)      # g = 0, m != 0: the weight moves against the sign of m by lr
            moved = pd[s].cpu().double() - p0[s].double() * (1.0 - L._f32(lr) * L._f32(L.WD))
            assert torch.equal(torch.sign(moved), -torch.sign(m0[s]).double()), f"step {k}: g = 0, the step follows sign(m)"
            assert float((moved.abs() - L._f32(lr)).abs().max()) < 2.0 ** -30       # |p| < 2^-7 here: two fp32 ulps of p
    if n >= 5 * L.SLOT:         # p = g = m = 0 (one slot with g = -0.0): bit-exact +0 after three steps with wd > 0
        for s in (L.ZERO_SLOT, L.NEG_ZERO_SLOT):
            for what, t in (("p", pd), ("m", md)) + ((("mirror", mirror),) if with_mirror else ()):
                assert not bool(_bits(t[L.slot(s)]).any()), f"slot {s}: {what} left zero"


def test_lr_zero_keeps_the_bits_of_p_and_advances_m():
    ops, dev = _ops(), _dev()
    n = 320
    p, m = L.start(n)
    g = L.grad(n, 0)
    pd, md, gd = p.to(dev), m.to(dev), g.to(dev)
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    ops.lion_step(pd, gd, md, n, 0.0, L.B1, L.B2, L.WD, L.GS, None, mirror)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pd.cpu()), _bits(p))
    assert torch.equal(_bits(mirror.cpu()), _bits(p.to(torch.bfloat16)))
    L.check_step("lr=0", pd, md, p, m, g, 1.0, 0.0, L.WD)
    live = torch.ones(n, dtype=torch.bool)
    for s in (L.ZERO_SLOT, L.NEG_ZERO_SLOT):
        live[L.slot(s)] = False
    assert bool((md.cpu() != m)[live].all())


@pytest.mark.parametrize("n", L.SIZES)
def test_device_lr_form_has_the_bits_of_the_host_scalar_form(n):
    ops, dev = _ops(), _dev()
    p, m = L.start(n)
    a = [p.to(dev), m.to(dev)]
    b = [t.clone() for t in a]
    for k, lr in enumerate(L.STEPS):
        g = L.grad(n, k)
        gd = g.to(dev)
        nc = _clip_coefficient(ops, gd, g, n)
        lr_dev = torch.tensor([lr], dtype=torch.float32).to(dev)
        ma = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        mb = ma.clone()
        ops.lion_step(a[0], gd, a[1], n, lr, L.B1, L.B2, L.WD, L.GS, nc, ma)
        ops.lion_step_dev(b[0], gd, b[1], n, lr_dev, L.B1, L.B2, L.WD, L.GS, nc, mb)
        torch.cuda.synchronize()
        for what, x, y in (("p", a[0], b[0]), ("m", a[1], b[1]), ("mirror", ma, mb)):
            assert torch.equal(_bits(x), _bits(y)), f"step {k}: {what}"
    assert not torch.equal(a[0].cpu(), p)


@functools.lru_cache(maxsize=None)
def _case(name):
    return C.CASES[name]()


GROUP_RANGES = {"one-range": None, "two-ranges": [(0, 128), (128, 320)]}
GROUP_RUNS = [("five-slots-three-groups", "one-range"), ("wrap-256-groups", "one-range"), ("five-slots-three-groups", "two-ranges")]


def _launch_groups(ops, case, state, gd, table, hyper_dev, nc, mirror, ranges):
    pd, md = state
    for lo, hi in ranges:
        ops.lion_step_groups(pd[lo:hi], gd[lo:hi], md[lo:hi], hi - lo, table[lo // C.SLOT:], hyper_dev, case.n_groups, L.B1, L.B2,
                             L.GS, nc, mirror[lo:hi])


@pytest.mark.parametrize("name,rng", GROUP_RUNS, ids=[f"{n}-{r}" for n, r in GROUP_RUNS])
def test_grouped_form_has_per_group_the_bits_of_the_ungrouped_kernel(name, rng):
    """Five slots in three groups (group 2 with lr = 0), the same five slots launched as two ranges with the table pointer
    offset, and 256 groups that change at every slot past the grid cap (the cases of tests/_groupcases.py)."""
    ops, dev = _ops(), _dev()
    case = _case(name)
    n = case.n
    ranges = GROUP_RANGES[rng] or [(0, n)]
    p, m = L.start(n)
    state = [p.to(dev), m.to(dev)]
    table = case.slot_group.to(dev)
    frozen = C.FROZEN_GROUP.get(name)
    for k, lr in enumerate(L.STEPS):
        g = L.grad(n, k)
        gd = g.to(dev)
        nc = _clip_coefficient(ops, gd, g, n)
        hyper = case.group_hyper(lr)
        host = torch.zeros(2 * case.n_groups, dtype=torch.float32)
        ops.lion_groups_hyper_host([a for a, _ in hyper], [b for _, b in hyper], host)
        assert host.tolist() == [x for pair in hyper for x in pair]
        hyper_dev = host.to(dev)
        before = [t.clone() for t in state]
        mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        _launch_groups(ops, case, state, gd, table, hyper_dev, nc, mirror, ranges)
        if rng != "one-range":      # the bits must not depend on how the buffer is cut into ranges
            whole, whole_mirror = [t.clone() for t in before], torch.full_like(mirror, -1000.0)
            _launch_groups(ops, case, whole, gd, table, hyper_dev, nc, whole_mirror, [(0, n)])
            for what, x, y in (("p", state[0], whole[0]), ("m", state[1], whole[1]), ("mirror", mirror, whole_mirror)):
                assert torch.equal(_bits(x), _bits(y)), f"step {k}: {what} depends on the range cut"
        for gi, (lr_g, wd_g) in enumerate(hyper):
            sub = [case.gather(t, gi) for t in before]
            sub_mirror = torch.full((sub[0].numel(),), -1000.0, dtype=torch.bfloat16, device=dev)
            ops.lion_step(sub[0], case.gather(gd, gi), sub[1], sub[0].numel(), lr_g, L.B1, L.B2, wd_g, L.GS, nc, sub_mirror)
            for what, got, want in (("p", state[0], sub[0]), ("m", state[1], sub[1]), ("mirror", mirror, sub_mirror)):
                assert torch.equal(_bits(case.gather(got, gi)), _bits(want)), \
                    f"step {k} group {gi} (lr {lr_g}, wd {wd_g}): {what} differs from sc_lion_step on the group's slots"
        torch.cuda.synchronize()
        if frozen is not None:      # lr = 0: weights and mirror keep their bits, the moment advances
            assert torch.equal(_bits(case.gather(state[0], frozen)), _bits(case.gather(before[0], frozen)))
            assert not torch.equal(case.gather(state[1], frozen), case.gather(before[1], frozen))
    assert not torch.equal(state[0].cpu(), p)


def test_argument_refusals_set_the_error_and_write_nothing():
    ops, dev = _ops(), _dev()
    from spatial_clip_amd import _lib
    lib = _lib.lib()
    n = 128
    bufs = [torch.full((n,), 0.5, device=dev) for _ in range(3)]
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    table = torch.zeros(n // 64, dtype=torch.uint8, device=dev)
    hyper = torch.full((2 * 256,), 1e-3, device=dev)
    lr_dev = torch.full((1,), 1e-3, device=dev)
    for bad_n in (0, 6, -4):
        with pytest.raises(_lib.SpatialClipHipError, match="sc_lion_step:"):
            ops.lion_step(*bufs, bad_n, 1e-3, L.B1, L.B2, L.WD, 1.0, None, mirror)
        with pytest.raises(_lib.SpatialClipHipError, match="sc_lion_step_dev:"):
            ops.lion_step_dev(*bufs, bad_n, lr_dev, L.B1, L.B2, L.WD, 1.0, None, mirror)
    with pytest.raises(_lib.SpatialClipHipError, match="sc_lion_step_dev: lr_dev"):
        ops.lion_step_dev(*bufs, n, None, L.B1, L.B2, L.WD, 1.0, None, mirror)
    for kw in (dict(n=100), dict(n=0), dict(n_groups=0), dict(n_groups=257), dict(chunk_group=None), dict(group_hyper=None)):
        a = dict(n=n, chunk_group=table, group_hyper=hyper, n_groups=2)
        a.update(kw)
        with pytest.raises(_lib.SpatialClipHipError, match="sc_lion_step_groups:"):
            ops.lion_step_groups(*bufs, a["n"], a["chunk_group"], a["group_hyper"], a["n_groups"], L.B1, L.B2, 1.0, None, mirror)
    # NULL buffers, straight at the C ABI
    ptrs = [b.data_ptr() for b in bufs]
    for i in range(3):
        a = list(ptrs)
        a[i] = None
        assert lib.sc_lion_step(*a, n, 1e-3, L.B1, L.B2, L.WD, 1.0, None, mirror.data_ptr(), None) != 0
        assert b"sc_lion_step: params, grads and exp_avg" in lib.sc_last_error()
        assert lib.sc_lion_step_dev(*a, n, lr_dev.data_ptr(), L.B1, L.B2, L.WD, 1.0, None, mirror.data_ptr(), None) != 0
        assert b"sc_lion_step_dev: params, grads and exp_avg" in lib.sc_last_error()
        assert lib.sc_lion_step_groups(*a, n, table.data_ptr(), hyper.data_ptr(), 2, L.B1, L.B2, 1.0, None, mirror.data_ptr(), None) != 0
        assert b"sc_lion_step_groups: params, grads and exp_avg" in lib.sc_last_error()
    for lrs in ([], [1e-3] * 257):
        with pytest.raises(_lib.SpatialClipHipError, match="sc_lion_groups_hyper_host"):
            ops.lion_groups_hyper_host(lrs, [0.0] * len(lrs), torch.zeros(2 * max(len(lrs), 1)))
    with pytest.raises(ValueError, match="lion_step_groups: chunk_group holds 1 slots"):
        ops.lion_step_groups(*bufs, n, table[:1], hyper, 2, L.B1, L.B2, 1.0, None, mirror)
    with pytest.raises(ValueError, match="lion_step: m holds 64 floats"):
        ops.lion_step(bufs[0], bufs[1], bufs[2][:64], n, 1e-3, L.B1, L.B2, L.WD, 1.0, None, mirror)
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs) and bool((mirror == -1000.0).all())


# ================================================================================================ through the net
LR, BETAS, WDECAY = 1.0e-4, (0.9, 0.99), 1.0        # configs/optimizer/lion.yaml


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, optim, streams
    return data, graph, losses, mc, module, net, optim, streams


def _net(seed=3, lock_image=False):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    g = torch.Generator().manual_seed(11)       # gains and biases off their ones and zeros: weight decay on them would show
    sd = n.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    n.load_state_dict(sd)
    if lock_image:      # what SpatialClipNet(lock_image=True) does, after the perturbation
        n.lock_image_tower(0)
    return n


def _module(n, param_groups=None, warmup=0, total=40, loss="clip"):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    if loss == "clip":
        loss_fn = losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    else:
        loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                     neighbor_alpha_scale=0.5, float32_logits=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedLion, lr=LR, betas=BETAS, weight_decay=WDECAY),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup), param_groups=param_groups)

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    assert isinstance(oc["optimizer"], optim.FusedLion)
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _batch(step, B=12):
    data, *_ = _pkg()
    return {k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=step).items()}


def _backward(m, batch):
    loss = m.training_step(batch, 0)
    loss.backward()
    return loss


def _full(opt, compact):
    return compact.clone() if opt.ranges == [(0, opt.store.total)] else opt._expand(compact)


def _trainable_mask(store):
    mask = torch.zeros(store.total, dtype=torch.bool, device=store.master.device)
    for lo, hi in store.trainable_ranges():
        mask[lo:hi] = True
    return mask


def _per_element(opt):
    """lr and weight decay of every float of the flat buffers (zeros where no group owns the slot)."""
    st = opt.store
    lr, wd = torch.zeros(st.total), torch.zeros(st.total)
    if len(opt.param_groups) == 1:
        return lr + opt.param_groups[0]["lr"], wd + opt.param_groups[0]["weight_decay"]
    for g in opt.param_groups:
        for name in g["param_names"]:
            sp = st.by_name[name]
            lr[sp.offset:sp.offset + sp.numel], wd[sp.offset:sp.offset + sp.numel] = g["lr"], g["weight_decay"]
    return lr, wd


def _check_against_the_formula(name, opt, p0, m0, grad_scale=1.0):
    """Masters and moments after ``opt.step`` against the host formula on the net's own gradient, the clip coefficient the
    step left in ``norm_clip`` and every element's group scalars; the locked part keeps its bits; the mirror is bf16(master)."""
    st = opt.store
    st.wait_all()
    torch.cuda.synchronize()
    mask = _trainable_mask(st).cpu()
    g = st.grad.detach().cpu()
    c = float(opt.norm_clip[1])
    lr, wd = _per_element(opt)
    ge = (g.double() * grad_scale * c, g * L._f32(grad_scale * 1.0) * L._f32(c))
    got_p, got_m = st.master.detach().cpu(), _full(opt, opt.exp_avg).cpu()
    b1, b2 = opt.param_groups[0]["betas"]
    fig = L.check_step(name, got_p[mask], got_m[mask], p0.cpu()[mask], m0.cpu()[mask], None, None, lr[mask], wd[mask], b1, b2,
                       ge=(ge[0][mask], ge[1][mask]))
    assert torch.equal(_bits(got_p[~mask]), _bits(p0.cpu()[~mask])), "a locked parameter moved"
    assert float(got_m[~mask].abs().max() if bool((~mask).any()) else 0.0) == 0.0
    assert torch.equal(_bits(st.master_bf16.detach().cpu()[mask]), _bits(got_p[mask].to(torch.bfloat16))), "mirror != bf16(master)"
    return fig, c


def _force_a_clip(store):
    """The plumbing check wants an active clip at max_norm = 1 and grad_scale = 0.5: a gradient of norm below 4 is scaled up
    to norm 4 (a clip coefficient of 0.5)."""
    norm = float(store.grad.double().norm())
    if norm < 4.0:
        store.grad.mul_(4.0 / norm)


def test_one_step_through_the_net_meets_the_kernel_rule(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    n = _net()
    m, opt, sched = _module(n)
    st = n.store
    assert opt.exp_avg.numel() == st.total and not hasattr(opt, "exp_avg_sq")
    m_init, gen = torch.zeros(st.total), torch.Generator().manual_seed(5)
    for sp in st.specs:         # a moment on the parameters, none on the padding between them
        m_init[sp.offset:sp.offset + sp.numel] = 0.01 * torch.randn(sp.numel, generator=gen)
    opt.exp_avg.copy_(m_init)
    _backward(m, _batch(0))
    st.wait_all()
    torch.cuda.synchronize()
    _force_a_clip(st)
    p0, m0 = st.master.detach().clone(), opt.exp_avg.clone()
    nc = opt.step(grad_scale=0.5, max_norm=1.0)
    fig, c = _check_against_the_formula("one step", opt, p0, m0, grad_scale=0.5)
    assert c < 1.0 and abs(float(nc[0]) - 0.5 * float(st.grad.double().norm())) < 1e-5 * float(nc[0])
    assert opt.step_count == 1 and not torch.equal(st.master, p0)


def _run_forms(forms, steps, make, monkeypatch):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    batches = [_batch(s) for s in range(steps)]
    res, losses_of = {}, {}
    for form in forms:
        monkeypatch.setenv("SC_ADAMW_BEHIND", "1" if form == "behind" else "0")
        n, m, opt, sched = make()
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
        res[form] = (n.store.master.detach().clone(), opt.exp_avg.clone(), n.store.master_bf16.clone())
        losses_of[form] = ls
    first = forms[0]
    for form in forms[1:]:
        assert losses_of[form] == losses_of[first], losses_of
        for a, b, what in zip(res[first], res[form], ("weights", "exp_avg", "bf16 mirror")):
            diff = (a != b).nonzero().flatten()
            where = "" if not diff.numel() else f": {diff.numel()} of {a.numel()} elements, first at {int(diff[0])}"
            assert not diff.numel(), f"{what}: {form} differs from {first}{where}"
    return res[first]


@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "no-decay-groups"])
def test_step_forms_are_bit_identical(monkeypatch, grouped):
    """Bucket by bucket behind the forward (4096-float buckets), one launch per range, and three graph replays against the
    eager steps, with the cosine schedule stepping (warm-up 2: the learning rate differs at every step)."""
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BUCKET", "4096")

    def make():
        n = _net()
        return (n, *_module(n, {"no_decay": "open_clip"} if grouped else None, warmup=2))
    w, _, _ = _run_forms(("behind", "one_launch", "graph"), 4, make, monkeypatch)
    assert not torch.equal(w, _net().store.master)


def test_locked_image_tower(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BEHIND", "0")
    batches = [_batch(s) for s in range(4)]

    def run(m, opt, sched, which):
        for s in which:
            _backward(m, batches[s])
            opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
        opt.store.wait_all()
        torch.cuda.synchronize()

    n = _net(lock_image=True)
    st = n.store
    m, opt, sched = _module(n, warmup=1)
    mask = _trainable_mask(st)
    assert 0 < int(mask.sum()) < st.total and opt.exp_avg.numel() == st.trainable_floats() == int(mask.sum())
    p0 = st.master.detach().clone()
    sched.step()        # past the lr = 0 of the first scheduler position
    _backward(m, batches[0])
    st.wait_all()
    torch.cuda.synchronize()
    before = st.master.detach().clone(), _full(opt, opt.exp_avg)
    opt.step(grad_scale=1.0, max_norm=1.0)
    _check_against_the_formula("locked step", opt, *before)
    sched.step()
    run(m, opt, sched, (1,))
    assert torch.equal(st.master[~mask], p0[~mask]) and not torch.equal(st.master[mask], p0[mask])
    ckpt = {"net": {k: v.cpu() for k, v in n.state_dict().items()}, "opt": opt.state_dict(), "sched": sched.last_epoch}
    assert list(ckpt["opt"]) == ["optimizer", "step", "exp_avg", "param_groups"] and ckpt["opt"]["exp_avg"].numel() == st.total
    assert float(ckpt["opt"]["exp_avg"][~mask].abs().max()) == 0.0
    run(m, opt, sched, (2, 3))
    want = (st.master.detach().clone(), opt.exp_avg.clone(), st.master_bf16.clone())
    # resumed with the lock: the uninterrupted run's bits
    n2 = _net(seed=5, lock_image=True)
    m2, opt2, sched2 = _module(n2, warmup=1)
    n2.load_state_dict(ckpt["net"])
    opt2.load_state_dict(ckpt["opt"])
    sched2.last_epoch = ckpt["sched"]
    sched2._apply()
    run(m2, opt2, sched2, (2, 3))
    for a, b, what in zip(want, (n2.store.master.detach(), opt2.exp_avg, n2.store.master_bf16), ("weights", "exp_avg", "mirror")):
        assert torch.equal(a, b), f"{what}: the resumed run differs from the uninterrupted one"
    # resumed without the lock: the full-layout moment is taken as it is and written back bit for bit
    n3 = _net(seed=5)
    m3, opt3, sched3 = _module(n3, warmup=1)
    n3.load_state_dict(ckpt["net"])
    opt3.load_state_dict(ckpt["opt"])
    assert opt3.exp_avg.numel() == st.total and opt3.step_count == 2
    assert torch.equal(_bits(opt3.exp_avg.cpu()), _bits(ckpt["opt"]["exp_avg"].cpu()))
    assert torch.equal(_bits(opt3.state_dict()["exp_avg"].cpu()), _bits(ckpt["opt"]["exp_avg"].cpu()))
    sched3.last_epoch = ckpt["sched"]
    sched3._apply()
    run(m3, opt3, sched3, (2,))
    assert not torch.equal(n3.store.master[~mask], p0[~mask])        # and now the image tower trains


def test_no_decay_groups_leave_gains_and_biases_undecayed(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    n = _net()
    m, opt, sched = _module(n, {"no_decay": "open_clip"})
    st = n.store
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(LR, 0.0), (LR, WDECAY)]
    _backward(m, _batch(0))
    st.wait_all()
    torch.cuda.synchronize()
    p0, m0 = st.master.detach().clone(), opt.exp_avg.clone()
    opt.step(grad_scale=1.0, max_norm=1.0)
    _check_against_the_formula("no-decay groups", opt, p0, m0)
    # the same said directly for one gain vector: p - lr * sign(c), no decay factor; a matrix carries the factor
    c = float(opt.norm_clip[1])
    for name, wd in (("visual.ln_post.weight", 0.0), ("gene.fc2.weight", WDECAY)):
        sp = st.by_name[name]
        s = slice(sp.offset, sp.offset + sp.numel)
        g = st.grad[s].cpu()
        L.check_step(name, st.master[s], opt.exp_avg[s], p0[s].cpu(), m0[s].cpu(), None, None, LR, wd, *BETAS,
                     ge=(g.double() * c, g * L._f32(c)))
        got = st.master[s].cpu().double()
        sign = torch.sign((1.0 - L._f32(BETAS[0])) * g.double() * c)         # m0 = 0: c is the gradient term alone
        undecayed = p0[s].cpu().double() - L._f32(LR) * sign
        near = float((got - undecayed).abs().max())
        assert (near < 1e-6) == (wd == 0.0), (name, near)


def test_trainer_accumulated_step_meets_the_kernel_rule(monkeypatch):
    """``Trainer(accumulate_grad_batches=2)`` over two batches: one optimiser step on the folded gradient (still in
    ``store.grad``), its norm finished from the fold's partial sums."""
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    n = _net()
    p0 = n.store.master.detach().clone()
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedLion, lr=LR, betas=BETAS, weight_decay=WDECAY),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=0))
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=2, val_steps=1)
    tr = Trainer(max_epochs=1, gradient_clip_val=1.0, log_every_n_steps=1, accumulate_grad_batches=2)
    tr.fit(m, dm)
    opt = tr.optimizer
    assert isinstance(opt, optim.FusedLion) and opt.step_count == 1 and tr.global_step == 1 and tr.accumulator is not None
    n.store.wait_all()
    torch.cuda.synchronize()
    norm = float(n.store.grad.double().norm())
    assert abs(float(opt.norm_clip[0]) - norm) < 1e-5 * norm, "norm_clip does not hold the norm of the folded gradient"
    opt.param_groups[0]["lr"] = opt.param_groups[0]["initial_lr"]      # the step ran at the schedule's first position: factor 1
    _check_against_the_formula("accumulated step", opt, p0, torch.zeros_like(p0))


def test_twenty_steps_on_one_batch_lower_the_loss(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    n = _net()
    m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    opt = optim.FusedLion(list(n.store.params.values()), lr=LR, betas=BETAS, weight_decay=WDECAY)
    batch = _batch(0)
    ls = []
    for _ in range(20):
        ls.append(float(_backward(m, batch).detach()))
        opt.step(grad_scale=1.0, max_norm=1.0)
    n.store.wait_all()
    torch.cuda.synchronize()
    print("  loss", " ".join(f"{x:.4f}" for x in ls))
    assert ls[-1] < ls[0], ls
