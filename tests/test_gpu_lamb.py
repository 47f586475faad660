"""LAMB on the device: the three kernels of a step (lamb_moments / lamb_trust / lamb_apply, spatial-clip_amd/csrc/sc_optim.hip)
against the float64 formula, then ``optim.FusedLamb`` through a real net in every step form.

Kernels (tests/_lambcases.py states the rule, the trust-ratio bound and the tensor table; tests/test_cpu_lamb.py holds torch's
fp32 evaluation in the kernels' summation order to them on these inputs): the full table with a tensor past the 4096 x 256 x 4
grid cap, with and without a clip coefficient near 0.5, with and without the bf16 mirror; the small table under
``always_adapt`` and ``trust_clip``; the same buffer as one piece and as three pieces cut inside tensors, launched in another
order, gives the same bits of p, m, v, mirror and r; the scalar table of the host function carries AdamW's bias corrections bit
for bit; ``lr = 0``; every refusal writes nothing.

Through the net (width 64, 2 layers, image 32, patch 8, gene MLP, B = 12): one step against the host formula per state-dict
tensor on the net's own gradient; the step forms agree bit for bit; open_clip's no-decay group gets r = 1; a locked tower; an
accumulated step of the Trainer; a checkpoint round trip; twenty steps on one batch lower the loss."""
import functools

import pytest
import torch

from tests import _lambcases as C

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
    ops.grad_norm(gd, n, C.GS, 0.5 * float(g.double().norm()) * C.GS, nc)
    return nc


# ================================================================================================ kernels
class _Run:
    """The device side of one table: state, tables, and one step as the optimiser issues it over ``pieces``."""

    def __init__(self, which, always_adapt=False, trust_clip=False):
        self.ops, self.dev = _ops(), _dev()
        self.tb = tb = C.table(which)
        self.which, self.flags = which, dict(always_adapt=always_adapt, trust_clip=trust_clip)
        self.state = [t.to(self.dev) for t in C.start(which)]
        self.slot_tensor, self.tensor_slots = tb.slot_tensor.to(self.dev), tb.tensor_slots.to(self.dev)
        self.slot_sums = torch.full((2 * (tb.n // 64),), NAN, device=self.dev)      # a slot of no tensor stays NaN: never summed
        self.trust = torch.full((tb.n_tensors,), NAN, device=self.dev)
        self.mirror = torch.full((tb.n,), -1000.0, dtype=torch.bfloat16, device=self.dev)

    def hyper(self, lr, t):
        host = torch.zeros(2 + 2 * self.tb.n_tensors, dtype=torch.float32)
        self.ops.lamb_hyper_host([lr * s for s in C.GROUP_LR], C.GROUP_WD, self.tb.tensor_group, C.B1, C.B2, t, host)
        return host

    def step(self, gd, lr, t, nc, with_mirror=True, pieces=None, hyper=None):
        ops, tb = self.ops, self.tb
        pd, md, vd = self.state
        hyper = (self.hyper(lr, t) if hyper is None else hyper).to(self.dev)
        pieces = pieces or [(0, tb.n)]
        for lo, hi in pieces:
            ops.lamb_moments(pd[lo:hi], gd[lo:hi], md[lo:hi], vd[lo:hi], hi - lo, self.slot_tensor[lo // 64:], hyper, tb.n_tensors,
                             C.B1, C.B2, C.EPS, C.GS, nc, self.slot_sums[2 * (lo // 64):])
        ops.lamb_trust(self.slot_sums, tb.n // 64, self.tensor_slots, hyper, tb.n_tensors, self.flags["always_adapt"],
                       self.flags["trust_clip"], self.trust)
        for lo, hi in pieces:
            ops.lamb_apply(pd[lo:hi], md[lo:hi], vd[lo:hi], hi - lo, self.slot_tensor[lo // 64:], hyper, self.trust, tb.n_tensors,
                           C.EPS, self.mirror[lo:hi] if with_mirror else None)
        torch.cuda.synchronize()

    def check_untouched(self, what, with_mirror=True):
        """Slots of no tensor keep their bits (the mirror its fill), the padding inside a tensor's last slot stays +0."""
        tb = self.tb
        pad = ~tb.owned
        for (lo, hi) in tb.holes:
            pad[lo:hi] = False
            for t, fill in zip(self.state, (C.HOLE_P, C.HOLE_M, C.HOLE_V)):
                assert bool((t[lo:hi] == fill).all()), f"{what}: a slot of no tensor was written"
            assert bool((self.mirror[lo:hi] == -1000.0).all()) and bool(torch.isnan(self.slot_sums[2 * lo // 64:2 * hi // 64]).all())
        for t in self.state + ([self.mirror] if with_mirror else []):
            assert not bool(_bits(t.cpu())[pad].any()), f"{what}: the padding of a tensor's last slot left zero"


KERNEL_CASES = [("full", clip, mirror, "plain") for clip in (False, True) for mirror in (True, False)] + \
               [("small", True, True, "always_adapt"), ("small", True, True, "trust_clip")]


@pytest.mark.parametrize("which,clip,with_mirror,variant", KERNEL_CASES,
                         ids=[f"{w}-" + ("clip" if c else "noclip") + ("-mirror-" if m else "-nomirror-") + v for w, c, m, v in KERNEL_CASES])
def test_lamb_step_meets_the_float64_rule(which, clip, with_mirror, variant):
    flags = {"plain": {}, "always_adapt": {"always_adapt": True}, "trust_clip": {"trust_clip": True}}[variant]
    run = _Run(which, **flags)
    tb = run.tb
    seen = {}
    for k, lr in enumerate(C.STEPS):
        g = C.grad(which, k)
        gd = g.to(run.dev)
        nc = _clip_coefficient(run.ops, gd, g, tb.n) if clip else None
        before = [t.cpu() for t in run.state]
        run.step(gd, lr, k + 1, nc, with_mirror)
        c = float(nc[1]) if clip else 1.0
        if clip:
            assert 0.4 < c < 0.6
        ge = (C.effective(g, c, torch.float64), C.effective(g, c, torch.float32))
        name = f"{which} {variant} step {k}"
        r64 = C.check_step(name, tb, run.state, before, ge, lr, k + 1, mirror=run.mirror if with_mirror else None, got_r=run.trust,
                           **flags)
        if which == "small":        # tensor by tensor, each with the E32 of its own elements
            C.check_step(name, tb, run.state, before, ge, lr, k + 1, per_tensor=True, **flags)
        if with_mirror:
            assert torch.equal(_bits(run.mirror.cpu())[tb.owned], _bits(run.state[0].cpu().to(torch.bfloat16))[tb.owned]), \
                f"step {k}: mirror != bf16(p)"
        else:
            assert bool((run.mirror == -1000.0).all()), f"step {k}: a buffer that was not passed was written"
        run.check_untouched(name, with_mirror)
        seen[k] = dict(zip(tb.names, run.trust.tolist()))
    # what the table is for: the cases of r, on the kernel's own output
    assert seen[0]["zero_p"] == 1.0 and all(s["still"] == 1.0 for s in seen.values())
    s = tb.elements(tb.index("still"))
    assert torch.equal(_bits(run.state[0][s].cpu()), _bits(C.start(which)[0][s])), "g = m = v = 0 without decay: p must not move"
    if variant == "always_adapt":
        assert all(s["nodecay"] != 1.0 for s in seen.values())
    else:
        assert all(s["nodecay"] == 1.0 for s in seen.values())
    if variant == "trust_clip":
        assert all(max(s.values()) == 1.0 and s["big_r"] == 1.0 for s in seen.values())
    else:
        assert all(s["big_r"] > 1.0 for s in seen.values())


PIECES = {"small": [(0, 384), (384, 768), (768, None)],
          "full": [(0, C.GRID_CAP_N // 2), (C.GRID_CAP_N // 2, C.GRID_CAP_N), (C.GRID_CAP_N, None)]}


@pytest.mark.parametrize("which", ["small", "full"])
def test_pieces_cut_inside_tensors_give_the_bits_of_one_piece(which):
    """Three pieces whose edges fall inside tensors (small: inside ``five`` and ``nodecay``; full: inside ``large``, the second
    at the end of the capped grid's first trip), launched last piece first, against one piece: p, m, v, the mirror, the slot
    sums and every tensor's r carry the same bits at every step."""
    one, cut = _Run(which), _Run(which)
    tb = one.tb
    pieces = [(lo, tb.n if hi is None else hi) for lo, hi in PIECES[which]][::-1]
    inside = {tb.names[ti] for lo, _ in pieces for ti in range(tb.n_tensors) if tb.offset[ti] < lo < tb.offset[ti] + tb.numel[ti]}
    assert inside == ({"five", "nodecay"} if which == "small" else {"large"}) and all(lo % 64 == 0 for lo, _ in pieces)
    for k, lr in enumerate(C.STEPS):
        g = C.grad(which, k)
        gd = g.to(one.dev)
        nc = _clip_coefficient(one.ops, gd, g, tb.n)
        one.step(gd, lr, k + 1, nc)
        cut.step(gd, lr, k + 1, nc, pieces=pieces)
        owned_slots = (tb.slot_tensor >= 0).repeat_interleave(2).to(one.dev)
        for what, x, y in (("p", one.state[0], cut.state[0]), ("m", one.state[1], cut.state[1]), ("v", one.state[2], cut.state[2]),
                           ("mirror", one.mirror, cut.mirror), ("r", one.trust, cut.trust),
                           ("slot sums", one.slot_sums[owned_slots], cut.slot_sums[owned_slots])):
            assert torch.equal(_bits(x), _bits(y)), f"step {k}: {what} depends on the cut"
        assert not bool(torch.isnan(one.trust).any())
    assert not torch.equal(one.state[0].cpu(), C.start(which)[0])


def test_the_scalar_table_is_adamws_and_a_relaunch_from_it_has_the_same_bits():
    """The device table is the one form of the step-dependent scalars, for the eager and the captured step alike: its bias
    corrections are the bits ``sc_adamw_hyper_host`` forms, each tensor reads its group's {lr, wd}, and a table built by hand
    from those bits (a captured step's refresh) gives the bits of the one the host function filled."""
    from spatial_clip_amd import _lib
    a, b = _Run("small"), _Run("small")
    tb = a.tb
    for k, lr in enumerate(C.STEPS):
        host = a.hyper(lr, k + 1)
        triple = torch.zeros(3, dtype=torch.float32)
        _lib.check(_lib.lib().sc_adamw_hyper_host(float(lr), C.B1, C.B2, k + 1, triple.data_ptr()), "sc_adamw_hyper_host")
        assert torch.equal(_bits(host[:2]), _bits(triple[1:]))
        assert torch.equal(_bits(torch.stack(C.bias_corrections(k + 1))), _bits(host[:2])), "the reference's scalars are not the kernel's"
        by_hand = torch.zeros_like(host)
        by_hand[:2] = triple[1:]
        for ti, gi in enumerate(tb.group):
            by_hand[2 + 2 * ti], by_hand[3 + 2 * ti] = lr * C.GROUP_LR[gi], C.GROUP_WD[gi]
        assert torch.equal(_bits(host), _bits(by_hand))
        g = C.grad("small", k)
        gd = g.to(a.dev)
        nc = _clip_coefficient(a.ops, gd, g, tb.n)
        a.step(gd, lr, k + 1, nc)
        b.step(gd, lr, k + 1, nc, hyper=by_hand)
        for what, x, y in zip(("p", "m", "v", "mirror", "r"), a.state + [a.mirror, a.trust], b.state + [b.mirror, b.trust]):
            assert torch.equal(_bits(x), _bits(y)), f"step {k}: {what}"


def test_lr_zero_keeps_the_bits_of_p_and_advances_the_moments():
    run = _Run("small")
    tb = run.tb
    p, m, v = C.start("small")
    g = C.grad("small", 0)
    run.step(g.to(run.dev), 0.0, 1, None)
    assert torch.equal(_bits(run.state[0].cpu()), _bits(p))
    assert torch.equal(_bits(run.mirror.cpu())[tb.owned], _bits(p.to(torch.bfloat16))[tb.owned])
    ge = (C.effective(g, 1.0, torch.float64), C.effective(g, 1.0, torch.float32))
    C.check_step("lr=0", tb, run.state, (p, m, v), ge, 0.0, 1, got_r=run.trust)
    live = tb.owned.clone()
    live[tb.elements(tb.index("still"))] = False
    assert bool((run.state[1].cpu() != m)[live].all()) and bool((run.state[2].cpu() != v)[live].all())


def test_argument_refusals_set_the_error_and_write_nothing():
    ops, dev = _ops(), _dev()
    from spatial_clip_amd import _lib
    lib = _lib.lib()
    n, n_t = 128, 2
    bufs = [torch.full((n,), 0.5, device=dev) for _ in range(4)]        # p, g, m, v
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    slot_tensor = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    tensor_slots = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32, device=dev)
    hyper = torch.full((2 + 2 * n_t,), 1e-3, device=dev)
    sums = torch.full((2 * (n // 64),), -7.0, device=dev)
    trust = torch.full((n_t,), -7.0, device=dev)
    E = _lib.SpatialClipHipError

    def moments(**kw):
        a = dict(n=n, slot_tensor=slot_tensor, hyper=hyper, n_tensors=n_t, slot_sums=sums)
        a.update(kw)
        ops.lamb_moments(*bufs, a["n"], a["slot_tensor"], a["hyper"], a["n_tensors"], C.B1, C.B2, C.EPS, 1.0, None, a["slot_sums"])

    def apply(**kw):
        a = dict(n=n, slot_tensor=slot_tensor, hyper=hyper, trust=trust, n_tensors=n_t)
        a.update(kw)
        ops.lamb_apply(bufs[0], bufs[2], bufs[3], a["n"], a["slot_tensor"], a["hyper"], a["trust"], a["n_tensors"], C.EPS, mirror)

    def trust_(**kw):
        a = dict(slot_sums=sums, n_slots=n // 64, tensor_slots=tensor_slots, hyper=hyper, n_tensors=n_t, trust=trust)
        a.update(kw)
        ops.lamb_trust(a["slot_sums"], a["n_slots"], a["tensor_slots"], a["hyper"], a["n_tensors"], False, False, a["trust"])

    for kw in (dict(n=0), dict(n=100), dict(n=-64), dict(n_tensors=0), dict(n_tensors=(1 << 20) + 1), dict(slot_tensor=None),
               dict(hyper=None), dict(slot_sums=None)):
        with pytest.raises(E, match="sc_lamb_moments:"):
            moments(**kw)
    for kw in (dict(n=0), dict(n=100), dict(n=-64), dict(n_tensors=0), dict(n_tensors=(1 << 20) + 1), dict(slot_tensor=None),
               dict(hyper=None), dict(trust=None)):
        with pytest.raises(E, match="sc_lamb_apply:"):
            apply(**kw)
    for kw in (dict(n_slots=0), dict(n_slots=-1), dict(n_tensors=0), dict(n_tensors=(1 << 20) + 1), dict(slot_sums=None),
               dict(tensor_slots=None), dict(hyper=None), dict(trust=None)):
        with pytest.raises(E, match="sc_lamb_trust:"):
            trust_(**kw)
    # tables too small for what the launch would read are refused before the library is called
    with pytest.raises(ValueError, match="lamb_moments: slot_tensor holds 1 elements, 2 are needed"):
        moments(slot_tensor=slot_tensor[:1])
    with pytest.raises(ValueError, match="lamb_moments: slot_sums holds 2 elements, 4 are needed"):
        moments(slot_sums=sums[:2])
    with pytest.raises(ValueError, match="lamb_apply: hyper holds 4 elements, 6 are needed"):
        apply(hyper=hyper[:4])
    with pytest.raises(ValueError, match="lamb_trust: tensor_slots holds 2 elements, 4 are needed"):
        trust_(tensor_slots=tensor_slots[:1])
    with pytest.raises(ValueError, match="lamb_trust: trust holds 1 elements, 2 are needed"):
        trust_(trust=trust[:1])
    with pytest.raises(ValueError, match="lamb_moments: v holds 64 floats"):
        ops.lamb_moments(bufs[0], bufs[1], bufs[2], bufs[3][:64], n, slot_tensor, hyper, n_t, C.B1, C.B2, C.EPS, 1.0, None, sums)
    with pytest.raises(TypeError, match="slot_tensor: expected torch.int32"):
        moments(slot_tensor=slot_tensor.to(torch.uint8))
    # NULL and misaligned buffers, straight at the C ABI
    ptrs = [b.data_ptr() for b in bufs]
    for i in range(4):
        a = list(ptrs)
        a[i] = None
        assert lib.sc_lamb_moments(*a, n, slot_tensor.data_ptr(), hyper.data_ptr(), n_t, C.B1, C.B2, C.EPS, 1.0, None,
                                   sums.data_ptr(), None) != 0
        assert b"sc_lamb_moments: params, grads and both moments" in lib.sc_last_error()
    for i in range(3):
        a = [ptrs[0], ptrs[2], ptrs[3]]
        a[i] = None
        assert lib.sc_lamb_apply(*a, n, slot_tensor.data_ptr(), hyper.data_ptr(), trust.data_ptr(), n_t, C.EPS, mirror.data_ptr(),
                                 None) != 0
        assert b"sc_lamb_apply: params and both moments" in lib.sc_last_error()
    assert lib.sc_lamb_moments(ptrs[0] + 4, *ptrs[1:], 64, slot_tensor.data_ptr(), hyper.data_ptr(), n_t, C.B1, C.B2, C.EPS, 1.0, None,
                               sums.data_ptr(), None) != 0
    assert b"16-byte aligned" in lib.sc_last_error()
    group = torch.zeros(n_t, dtype=torch.int32)
    for lrs, tg, step in (([], group, 1), ([1e-3] * 257, group, 1), ([1e-3], group, 0), ([1e-3], group + 1, 1), ([1e-3], group[:0], 1)):
        with pytest.raises(E, match="sc_lamb_hyper_host"):
            ops.lamb_hyper_host(lrs, [0.0] * len(lrs), tg, C.B1, C.B2, step, torch.zeros(2 + 2 * n_t))
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs) and bool((mirror == -1000.0).all())
    assert bool((sums == -7.0).all()) and bool((trust == -7.0).all())


def test_a_tensor_range_outside_the_buffer_is_not_followed():
    """``tensor_slots`` lives in device memory, out of the host's sight: a pair outside [0, n_slots] gives r = 1 and reads
    nothing; a slot whose tensor index is not below n_tensors is left alone."""
    ops, dev = _ops(), _dev()
    n = 192
    sums = torch.ones(2 * (n // 64), device=dev)
    sums[1::2] = 4.0            # every slot: sum p^2 = 1, sum u^2 = 4
    slots = torch.tensor([[0, 2], [2, 4], [-1, 1], [2, 1]], dtype=torch.int32, device=dev)
    hyper = torch.full((2 + 2 * 4,), 0.1, device=dev)
    trust = torch.full((4,), NAN, device=dev)
    ops.lamb_trust(sums, n // 64, slots, hyper, 4, False, False, trust)
    torch.cuda.synchronize()
    assert trust.tolist() == [0.5, 1.0, 1.0, 1.0]
    p, g, m, v = (torch.full((n,), 0.5, device=dev) for _ in range(4))
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    slot_tensor = torch.tensor([4, -1, 1 << 30], dtype=torch.int32, device=dev)
    ops.lamb_moments(p, g, m, v, n, slot_tensor, hyper, 4, C.B1, C.B2, C.EPS, 1.0, None, sums)
    ops.lamb_apply(p, m, v, n, slot_tensor, hyper, trust, 4, C.EPS, mirror)
    torch.cuda.synchronize()
    assert all(bool((t == 0.5).all()) for t in (p, m, v)) and bool((mirror == -1000.0).all())


# ================================================================================================ through the net
LR, BETAS, EPS, WDECAY = 2.0e-3, (0.9, 0.999), 1.0e-6, 0.05


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, optim, streams
    return data, graph, losses, mc, module, net, optim, streams


def _net(seed=3, lock_image=False):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    g = torch.Generator().manual_seed(11)       # gains and biases off their ones and zeros: a trust ratio on them would show
    sd = n.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    n.load_state_dict(sd)
    if lock_image:      # what SpatialClipNet(lock_image=True) does, after the perturbation
        n.lock_image_tower(0)
    return n


def _module(n, param_groups=None, warmup=0, total=40, **opt_kw):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WDECAY)
    kw.update(opt_kw)
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), functools.partial(optim.FusedLamb, **kw),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup), param_groups=param_groups)

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    assert isinstance(oc["optimizer"], optim.FusedLamb)
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


def _table_of(opt):
    st = opt.store
    items = [(n, st.by_name[n].offset, st.by_name[n].numel, int(opt.tensor_group[ti])) for ti, n in enumerate(opt.tensor_names)]
    return C.Table.from_layout(st.total, items)


def _state(opt):
    st = opt.store
    st.wait_all()
    torch.cuda.synchronize()
    return st.master.detach().cpu().clone(), _full(opt, opt.exp_avg).cpu(), _full(opt, opt.exp_avg_sq).cpu()


def _check_against_the_formula(name, opt, before, grad_scale=1.0, **kw):
    """Masters and moments after ``opt.step`` against the host formula, state-dict tensor by tensor, on the net's own gradient,
    the clip coefficient the step left in ``norm_clip`` and every tensor's group scalars; whatever is no trainable tensor keeps
    its bits; the mirror is bf16(master)."""
    st = opt.store
    tb = _table_of(opt)
    got = _state(opt)
    g = st.grad.detach().cpu()
    c = float(opt.norm_clip[1]) if opt._clip_threshold(kw.pop("max_norm", None)) is not None else 1.0
    ge = (g.double() * grad_scale * c, g * C._f32(grad_scale) * C._f32(c))
    lr_of = [opt.param_groups[gi]["lr"] for gi in tb.group]
    wd_of = [opt.param_groups[gi]["weight_decay"] for gi in tb.group]
    b1, b2 = opt.param_groups[0]["betas"]
    r64 = C.check_step(name, tb, got, before, ge, None, opt.step_count, got_r=opt.trust, per_tensor=True, lr_of=lr_of, wd_of=wd_of,
                       b1=b1, b2=b2, eps=opt.param_groups[0]["eps"], always_adapt=opt.always_adapt, trust_clip=opt.trust_clip)
    for lo, hi in tb.holes:
        for x, y in zip(got, before):
            assert torch.equal(_bits(x[lo:hi]), _bits(y[lo:hi])), "floats of no trainable tensor changed"
    mask = _trainable_mask(st).cpu()
    assert torch.equal(_bits(st.master_bf16.detach().cpu()[mask]), _bits(got[0][mask].to(torch.bfloat16))), "mirror != bf16(master)"
    return tb, r64, c


def _force_a_clip(store):
    """An active clip at max_norm = 1 and grad_scale = 0.5: a gradient of norm below 4 is scaled up to norm 4."""
    norm = float(store.grad.double().norm())
    if norm < 4.0:
        store.grad.mul_(4.0 / norm)


def test_one_step_through_the_net_meets_the_kernel_rule_per_tensor(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    n = _net()
    m, opt, sched = _module(n)
    st = n.store
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.total and len(opt.tensor_names) == len(st.specs)
    gen = torch.Generator().manual_seed(5)
    m_init, v_init = torch.zeros(st.total), torch.zeros(st.total)
    for sp in st.specs:         # moments on the parameters, none on the padding between them
        m_init[sp.offset:sp.offset + sp.numel] = 0.01 * torch.randn(sp.numel, generator=gen)
        v_init[sp.offset:sp.offset + sp.numel] = (0.01 * torch.randn(sp.numel, generator=gen)) ** 2
    opt.exp_avg.copy_(m_init)
    opt.exp_avg_sq.copy_(v_init)
    _backward(m, _batch(0))
    st.wait_all()
    torch.cuda.synchronize()
    _force_a_clip(st)
    before = _state(opt)
    nc = opt.step(grad_scale=0.5, max_norm=2.0)        # the optimiser's own max_grad_norm = 1 is the smaller threshold
    tb, r64, c = _check_against_the_formula("one step", opt, before, grad_scale=0.5, max_norm=2.0)
    norm = 0.5 * float(st.grad.double().norm())
    assert abs(float(nc[0]) - norm) < 1e-5 * norm and abs(c - 1.0 / norm) < 1e-5 * c, "the clip is not the one at max_grad_norm = 1"
    assert opt.step_count == 1 and not torch.equal(st.master.cpu(), before[0])
    assert float(r64.min()) < 1.0 and len({round(x, 4) for x in r64.tolist()}) > 10       # the ratios are per tensor


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
        res[form] = (n.store.master.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), n.store.master_bf16.clone(),
                     opt.trust.clone())
        losses_of[form] = ls
    first = forms[0]
    for form in forms[1:]:
        assert losses_of[form] == losses_of[first], losses_of
        for a, b, what in zip(res[first], res[form], ("weights", "exp_avg", "exp_avg_sq", "bf16 mirror", "trust ratios")):
            diff = (a != b).nonzero().flatten()
            where = "" if not diff.numel() else f": {diff.numel()} of {a.numel()} elements, first at {int(diff[0])}"
            assert not diff.numel(), f"{what}: {form} differs from {first}{where}"
    return res[first]


@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "no-decay-groups"])
def test_step_forms_are_bit_identical(monkeypatch, grouped):
    """Bucket by bucket behind the forward (4096-float buckets, cut inside the matrices), one pass per range, and three graph
    replays against the eager steps, with the cosine schedule stepping (warm-up 2: the learning rate differs at every step)."""
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BUCKET", "4096")

    def make():
        n = _net()
        return (n, *_module(n, {"no_decay": "open_clip"} if grouped else None, warmup=2))
    w, *_, trust = _run_forms(("behind", "one_launch", "graph"), 4, make, monkeypatch)
    assert not torch.equal(w, _net().store.master)
    assert bool((trust == 1.0).any()) == grouped and bool((trust != 1.0).any())


def test_no_decay_group_gets_a_trust_ratio_of_one(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    n = _net()
    m, opt, sched = _module(n, {"no_decay": "open_clip"})
    st = n.store
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(LR, 0.0), (LR, WDECAY)]
    _backward(m, _batch(0))
    before = _state(opt)
    opt.step(grad_scale=1.0, max_norm=1.0)
    tb, r64, c = _check_against_the_formula("no-decay groups", opt, before, max_norm=1.0)
    trust = dict(zip(opt.tensor_names, opt.trust.tolist()))
    no_decay = set(opt.param_groups[0]["param_names"])
    assert {"logit_scale", "visual.ln_post.weight", "visual.ln_post.bias"} <= no_decay and "gene.fc2.weight" not in no_decay
    assert all(trust[name] == 1.0 for name in no_decay) and all(trust[name] != 1.0 for name in trust if name not in no_decay)
    # against a reference that adapts the no-decay tensors too, the same step is far outside the rule: r = 1 is what ran
    ti = tb.index("visual.ln_post.bias")       # (a gain vector near 1 under a first Adam step of +-1 has r near 1 of itself)
    g = st.grad.detach().cpu()
    ge = g.double() * c
    adapted = C.step_ref(tb, *before, ge, None, 1, torch.float64, lr_of=[LR] * tb.n_tensors,
                         wd_of=[opt.param_groups[gi]["weight_decay"] for gi in tb.group], b1=BETAS[0], b2=BETAS[1], eps=EPS,
                         always_adapt=True)
    s = tb.elements(ti)
    assert float(adapted[3][ti]) != 1.0
    moved, would = st.master.detach().cpu()[s].double() - before[0][s].double(), adapted[0][s] - before[0][s].double()
    assert float((moved - would).abs().max()) > 0.1 * float(moved.abs().max()), "the no-decay gain moved as if it were adapted"


def test_locked_image_tower_and_checkpoint_round_trip(monkeypatch):
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
    m, opt, sched = _module(n, {"no_decay": "open_clip"}, warmup=1)
    mask = _trainable_mask(st)
    assert 0 < int(mask.sum()) < st.total
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.trainable_floats() == int(mask.sum())      # no moments for a locked float
    assert opt.tensor_names == st.trainable_names() and not any(name.startswith("visual.") for name in opt.tensor_names)
    p0 = st.master.detach().clone()
    sched.step()        # past the lr = 0 of the first scheduler position
    _backward(m, batches[0])
    before = _state(opt)
    opt.step(grad_scale=1.0, max_norm=1.0)
    _check_against_the_formula("locked step", opt, before, max_norm=1.0)
    sched.step()
    run(m, opt, sched, (1,))
    assert torch.equal(_bits(st.master[~mask]), _bits(p0[~mask])) and not torch.equal(st.master[mask], p0[mask])
    ckpt = {"net": {k: v.cpu() for k, v in n.state_dict().items()}, "opt": opt.state_dict(), "sched": sched.last_epoch}
    assert list(ckpt["opt"]) == ["optimizer", "step", "exp_avg", "exp_avg_sq", "param_groups"] and ckpt["opt"]["optimizer"] == "lamb"
    for key in ("exp_avg", "exp_avg_sq"):
        assert ckpt["opt"][key].numel() == st.total and float(ckpt["opt"][key][~mask].abs().max()) == 0.0
    run(m, opt, sched, (2, 3))
    want = (st.master.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), st.master_bf16.clone())
    # resumed with the lock: the uninterrupted run's bits
    n2 = _net(seed=5, lock_image=True)
    m2, opt2, sched2 = _module(n2, {"no_decay": "open_clip"}, warmup=1)
    n2.load_state_dict(ckpt["net"])
    opt2.load_state_dict(ckpt["opt"])
    sched2.last_epoch = ckpt["sched"]
    sched2._apply()
    run(m2, opt2, sched2, (2, 3))
    for a, b, what in zip(want, (n2.store.master.detach(), opt2.exp_avg, opt2.exp_avg_sq, n2.store.master_bf16),
                          ("weights", "exp_avg", "exp_avg_sq", "mirror")):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: the resumed run differs from the uninterrupted one"
    # resumed without the lock: the full-layout moments are taken as they are and written back bit for bit
    n3 = _net(seed=5)
    m3, opt3, sched3 = _module(n3, warmup=1)
    n3.load_state_dict(ckpt["net"])
    opt3.load_state_dict(ckpt["opt"])
    assert opt3.exp_avg.numel() == st.total and opt3.step_count == 2
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(opt3.state_dict()[key].cpu()), _bits(ckpt["opt"][key].cpu()))
    sched3.last_epoch = ckpt["sched"]
    sched3._apply()
    run(m3, opt3, sched3, (2,))
    assert not torch.equal(n3.store.master[~mask], p0[~mask])        # and now the image tower trains


def test_trainer_accumulated_step_meets_the_kernel_rule(monkeypatch):
    """``Trainer(accumulate_grad_batches=2)`` over two batches: one optimiser step on the folded gradient (still in
    ``store.grad``), its norm finished from the fold's partial sums."""
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    n = _net()
    p0 = n.store.master.detach().cpu().clone()
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedLamb, lr=LR, betas=BETAS, eps=EPS, weight_decay=WDECAY),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=0))
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=2, val_steps=1)
    tr = Trainer(max_epochs=1, gradient_clip_val=1.0, log_every_n_steps=1, accumulate_grad_batches=2)
    tr.fit(m, dm)
    opt = tr.optimizer
    assert isinstance(opt, optim.FusedLamb) and opt.step_count == 1 and tr.global_step == 1 and tr.accumulator is not None
    n.store.wait_all()
    torch.cuda.synchronize()
    norm = float(n.store.grad.double().norm())
    assert abs(float(opt.norm_clip[0]) - norm) < 1e-5 * norm, "norm_clip does not hold the norm of the folded gradient"
    opt.param_groups[0]["lr"] = opt.param_groups[0]["initial_lr"]      # the step ran at the schedule's first position: factor 1
    zeros = torch.zeros_like(p0)
    _check_against_the_formula("accumulated step", opt, (p0, zeros, zeros), max_norm=1.0)


def test_twenty_steps_on_one_batch_lower_the_loss(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    n = _net()
    m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    opt = optim.FusedLamb(list(n.store.params.values()), lr=LR, betas=BETAS, eps=EPS, weight_decay=WDECAY)
    batch = _batch(0)
    ls = []
    for _ in range(20):
        ls.append(float(_backward(m, batch).detach()))
        opt.step(grad_scale=1.0, max_norm=1.0)
    n.store.wait_all()
    torch.cuda.synchronize()
    print("  loss", " ".join(f"{x:.4f}" for x in ls))
    assert ls[-1] < ls[0], ls
