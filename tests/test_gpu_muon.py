"""Muon on the device: the epilogue kernel, the Newton-Schulz result against the rule of tests/_muoncases.py
(torch.optim.Muon on the CPU is the yardstick), three chained steps, pieces, refusals; then FusedMuon through a tiny net with an
image and a text tower: the default split, one step per tensor, the three step forms bit for bit, the AdamW part against
FusedAdamW, a locked tower with a checkpoint round trip, an accumulated Trainer step, weight averaging, and a short run."""
import functools

import pytest
import torch

from tests import _muoncases as C
from tests import _refbounds as R

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


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ================================================================================================ the epilogue kernel
@pytest.mark.parametrize("n", [8, 64, 72 * 200, 4096 * 256 * 8 + 8])
def test_axpby_is_one_rounding_of_the_fp32_expression(n):
    """out = bf16(fma(beta, cin, alpha * acc)); the last size crosses the end of the first trip of the capped grid."""
    ops, dev = _ops(), _dev()
    g = torch.Generator().manual_seed(n)
    acc = torch.randn(n, generator=g)
    cin = torch.randn(n, generator=g).to(torch.bfloat16)
    out = torch.full((n + 8,), -1000.0, dtype=torch.bfloat16, device=dev)
    alpha, beta = C.COEFFS[2], C.COEFFS[1]
    ops.muon_axpby(acc.to(dev), cin.to(dev), out, n, alpha, beta)
    torch.cuda.synchronize()
    want = (_f32(beta) * cin.double() + (_f32(alpha) * acc).double()).float().to(torch.bfloat16)      # the product rounded to fp32, the fma exact
    got = out.cpu()
    assert torch.equal(_bits(got[:n]), _bits(want)), int((got[:n] != want).sum())
    assert bool((got[n:] == -1000.0).all())


# ================================================================================================ the kernels of one step
class _Run:
    """The device side of the table: state, tables, scratch, and one step as the optimiser issues it over ``pieces``."""

    def __init__(self, adjust=None, zero_p=False):
        self.ops, self.dev = _ops(), _dev()
        self.tb = tb = C.table(adjust)
        dev = self.dev
        self.state = [t.clone().to(dev) for t in C.start(zero_p)]
        self.slot_tensor, self.info, self.ratio = tb.slot_tensor.to(dev), tb.info.to(dev), tb.ratio.to(dev)
        self.chunk_group = tb.chunk_group.to(dev)
        n_x = 64 * tb.compact_slots
        self.x0 = torch.full((n_x,), NAN, dtype=torch.bfloat16, device=dev)
        self.x1 = torch.full((n_x,), NAN, dtype=torch.bfloat16, device=dev)
        shapes = [tb.shape[i] for i in tb.muon]
        self.gbuf = torch.full((max(min(s) ** 2 for s in shapes),), NAN, dtype=torch.bfloat16, device=dev)
        self.pbuf = torch.full_like(self.gbuf, NAN)
        self.acc = torch.full((max(r * c for r, c in shapes),), NAN, device=dev)
        self.slot_sums = torch.full((tb.n // 64,), NAN, device=dev)       # an AdamW slot and a slot of no tensor stay NaN
        self.norms = torch.full((len(tb.muon),), NAN, device=dev)
        self.mirror = torch.full((tb.n,), -1000.0, dtype=torch.bfloat16, device=dev)

    def hyper(self, lrs, wds, t):
        host = torch.zeros(2 + 2 * len(lrs), dtype=torch.float32)
        self.ops.adamw_groups_hyper_host(lrs, wds, C.B1, C.B2, t, host)
        return host.to(self.dev)

    def obuf(self):
        return self.x1 if C.NS_STEPS & 1 else self.x0

    def step(self, gd, hyper, gs, nc, momentum, nesterov, pieces=None):
        ops, tb = self.ops, self.tb
        pd, md, vd = self.state
        pieces = pieces or [(0, tb.n)]
        n_mu = len(tb.muon)
        for lo, hi in pieces:
            ops.muon_momentum(gd[lo:hi], md[lo:hi], hi - lo, self.slot_tensor[lo // 64:], self.info, n_mu, lo // 64, momentum, nesterov,
                              gs, nc, self.x1, self.slot_sums[lo // 64:], tb.compact_slots)
        ops.muon_scale(self.slot_sums, tb.n // 64, self.info, n_mu, C.EPS_MUON, self.x1, self.x0, self.norms, tb.compact_slots)
        from spatial_clip_amd import optim
        for t, i in enumerate(tb.muon):
            r, c = tb.shape[i]
            out = optim.muon_newton_schulz(self.x0, self.x1, int(tb.info[t, 2]) * 64, r, c, self.gbuf, self.pbuf, self.acc, C.NS_STEPS,
                                           C.COEFFS)
            assert out is self.obuf()
        for lo, hi in pieces:
            ops.muon_apply(pd[lo:hi], gd[lo:hi], md[lo:hi], vd[lo:hi], hi - lo, self.chunk_group[lo // 64:], self.slot_tensor[lo // 64:],
                           self.info, self.ratio, n_mu, lo // 64, self.obuf(), hyper, len(C.GROUP_LR), C.B1, C.B2, C.EPS_ADAM, gs, nc,
                           self.mirror[lo:hi], tb.compact_slots)
        torch.cuda.synchronize()

    def adamw_reference(self, before, gd, hyper, gs, nc):
        """``ops.adamw_step_groups`` over the whole buffer from ``before``: what the AdamW slots must hold, bit for bit."""
        p, m, v = (t.clone().to(self.dev) for t in before)
        mirror = torch.full((self.tb.n,), -1000.0, dtype=torch.bfloat16, device=self.dev)
        self.ops.adamw_step_groups(p, gd, m, v, self.tb.n, self.chunk_group, hyper, len(C.GROUP_LR), C.B1, C.B2, C.EPS_ADAM, gs, nc, mirror)
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu(), mirror.cpu()

    def check_adamw_and_holes(self, what, before, gd, hyper, gs, nc):
        tb = self.tb
        want = self.adamw_reference(before, gd, hyper, gs, nc)
        got = [t.cpu() for t in self.state] + [self.mirror.cpu()]
        for i in tb.adamw:
            lo = tb.offset[i]
            s = slice(lo, lo + (max(tb.numel[i], 1) + 63) // 64 * 64)           # the tensor's whole slots, padding included
            for a, b, name in zip(got, want, ("p", "exp_avg", "exp_avg_sq", "mirror")):
                assert torch.equal(_bits(a[s]), _bits(b[s])), f"{what}: AdamW tensor {tb.names[i]}: {name} differs from adamw_step_groups"
            assert not torch.equal(got[0][s], before[0][s])
        for lo, hi in tb.holes:
            for t, fill in zip(self.state, (C.HOLE_P, C.HOLE_M, C.HOLE_V)):
                assert bool((t[lo:hi] == fill).all()), f"{what}: a slot of no tensor was written"
            assert bool((self.mirror[lo:hi] == -1000.0).all()) and bool(torch.isnan(self.slot_sums[lo // 64:hi // 64]).all())
        for i in tb.muon:           # Muon keeps no second moment: the slots' exp_avg_sq is not written
            s = tb.elements(i)
            assert torch.equal(_bits(got[2][s]), _bits(before[2][s])), f"{what}: exp_avg_sq of Muon tensor {tb.names[i]} changed"
            assert torch.equal(_bits(got[3][s]), _bits(got[0][s].to(torch.bfloat16))), f"{what}: mirror of {tb.names[i]} != bf16(p)"


@pytest.mark.parametrize("kind", C.KINDS)
def test_newton_schulz_alone_meets_the_rule(kind):
    """p = 0, lr = 1, wd = 0, momentum = 0, grad_scale = 1: U is the gradient, the compact result buffer holds O and the
    weights -lr_adj O.  Every matrix of the table carries an input of ``kind``."""
    run = _Run(zero_p=True)
    tb = run.tb
    g = C.grad(kind, 0)
    before = [t.cpu().clone() for t in run.state]
    hyper = run.hyper([1.0] * 4, [0.0] * 4, 1)
    run.step(g.to(run.dev), hyper, 1.0, None, 0.0, True)
    o_all, p, norms = run.obuf().cpu(), run.state[0].cpu(), run.norms.cpu()
    for t, i in enumerate(tb.muon):
        r, c = tb.shape[i]
        u = g[tb.elements(i)].reshape(r, c)
        o = o_all[tb.compact(t)].reshape(r, c)
        C.check_o(f"{kind} {tb.names[i]} [{r}, {c}]", o.double(), C.torch_o(u), C.ns64(u))
        want_norm = float(u.to(torch.bfloat16).double().norm())
        assert abs(float(norms[t]) - want_norm) <= 1e-6 * want_norm, (tb.names[i], float(norms[t]), want_norm)
        ratio = _f32(C.adjust_ratio(None, r, c))
        assert torch.equal(p[tb.elements(i)].reshape(r, c), -(ratio * o.float())), f"{tb.names[i]}: p is not -lr_adj O"
        assert torch.equal(_bits(run.state[1].cpu()[tb.elements(i)]), _bits(g[tb.elements(i)])), "momentum 0: B is the gradient"
    run.check_adamw_and_holes(kind, before, g.to(run.dev), hyper, 1.0, None)


CHAIN = [(True, None, False), (False, None, True), (True, "match_rms_adamw", True), (False, "original", False)]


@pytest.mark.parametrize("nesterov,adjust,clip", CHAIN, ids=[f"nesterov{int(a)}-{b}-clip{int(c)}" for a, b, c in CHAIN])
def test_three_chained_steps_meet_the_rules(nesterov, adjust, clip):
    """t = 1, 2, 3 with a changing learning rate, grad_scale 0.5; every reference step starts from the state the kernels left."""
    run = _Run(adjust)
    ops, tb, dev = run.ops, run.tb, run.dev
    for k, lr in enumerate(C.STEPS):
        g = C.grad("gauss", k)
        gd = g.to(dev)
        nc, cval = None, 1.0
        if clip:        # a clip coefficient near 0.5: max_norm is half the norm of the scaled gradient
            nc = torch.full((2,), NAN, device=dev)
            ops.grad_norm(gd, tb.n, C.GS, 0.5 * float(g.double().norm()) * C.GS, nc)
            cval = float(nc[1])
            assert 0.45 < cval < 0.55
        before = [t.cpu().clone() for t in run.state]
        lrs = [lr * s for s in C.GROUP_LR]
        hyper = run.hyper(lrs, C.GROUP_WD, k + 1)
        run.step(gd, hyper, C.GS, nc, C.MU, nesterov)
        got = [t.cpu() for t in run.state]
        ge64, ge32 = C.effective(g, cval, torch.float64), C.effective(g, cval, torch.float32)
        for t, i in enumerate(tb.muon):
            r, c = tb.shape[i]
            s = tb.elements(i)
            name = f"step {k} {tb.names[i]} [{r}, {c}]"
            lr_g, wd_g = lrs[tb.group[i]], C.GROUP_WD[tb.group[i]]
            p0, b0 = before[0][s].reshape(r, c), before[1][s].reshape(r, c)
            C.check_b(f"{name} B", got[1][s].reshape(r, c), b0, ge64[s].reshape(r, c), ge32[s].reshape(r, c), C.MU)
            _, u32 = C.update_of(b0, ge32[s].reshape(r, c), C.MU, nesterov, torch.float32)
            p_t, _ = C.torch_step(p0, b0, ge32[s].reshape(r, c), lr_g, wd_g, C.MU, nesterov, adjust)
            lr_adj = _f32(lr_g) * C.adjust_ratio(adjust, r, c)
            C.check_o(name, C.recover_o(p0, got[0][s].reshape(r, c), lr_g, wd_g, lr_adj), C.recover_o(p0, p_t, lr_g, wd_g, lr_adj),
                      C.ns64(u32))
        run.check_adamw_and_holes(f"step {k}", before, gd, hyper, C.GS, nc)


def test_pieces_cut_inside_tensors_give_the_bits_of_one_piece():
    tb = C.table()
    cuts = [tb.offset[tb.index("tall")] + 64 * 7, tb.offset[tb.index("odd")] + 64 * 100, tb.offset[tb.index("edge")] + 64]
    pieces = list(zip([0] + cuts, cuts + [tb.n]))
    res = []
    for pc in (None, pieces):
        run = _Run()
        for k, lr in enumerate(C.STEPS[:2]):
            hyper = run.hyper([lr * s for s in C.GROUP_LR], C.GROUP_WD, k + 1)
            run.step(C.grad("gauss", k).to(run.dev), hyper, C.GS, None, C.MU, True, pieces=pc)
        res.append([t.cpu() for t in run.state] + [run.mirror.cpu(), run.obuf().cpu(), run.norms.cpu()])
    for a, b, what in zip(res[0], res[1], ("p", "exp_avg", "exp_avg_sq", "mirror", "O", "norms")):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: the pieces differ from one piece"


def test_argument_refusals_set_the_error_and_write_nothing():
    ops, dev = _ops(), _dev()
    from spatial_clip_amd import _lib
    lib = _lib.lib()
    E = _lib.SpatialClipHipError
    n = 128
    bufs = [torch.full((n,), 0.5, device=dev) for _ in range(4)]        # p, g, m, v
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    slot_tensor = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    info = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=dev)
    chunk = torch.zeros(2, dtype=torch.uint8, device=dev)
    hyper = torch.full((4,), 1e-3, device=dev)
    ratio = torch.ones(1, device=dev)
    sums = torch.full((2,), -7.0, device=dev)
    norms = torch.full((1,), -7.0, device=dev)
    x = [torch.full((256,), -3.0, dtype=torch.bfloat16, device=dev) for _ in range(4)]         # x0, x1, g, p

    def momentum(**kw):
        a = dict(n=n, slot_tensor=slot_tensor, info=info, n_tensors=1, slot0=0, mu=0.95, ubuf=x[1], sums=sums)
        a.update(kw)
        ops.muon_momentum(bufs[1], bufs[2], a["n"], a["slot_tensor"], a["info"], a["n_tensors"], a["slot0"], a["mu"], True, 1.0, None,
                          a["ubuf"], a["sums"], 1)

    def scale(**kw):
        a = dict(sums=sums, n_slots=2, info=info, n_tensors=1, eps=1e-7, ubuf=x[1], xbuf=x[0], norms=norms)
        a.update(kw)
        ops.muon_scale(a["sums"], a["n_slots"], a["info"], a["n_tensors"], a["eps"], a["ubuf"], a["xbuf"], a["norms"], 1)

    def apply(**kw):
        a = dict(n=n, chunk=chunk, slot_tensor=slot_tensor, info=info, ratio=ratio, n_tensors=1, slot0=0, obuf=x[1], hyper=hyper, n_groups=1)
        a.update(kw)
        ops.muon_apply(*bufs, a["n"], a["chunk"], a["slot_tensor"], a["info"], a["ratio"], a["n_tensors"], a["slot0"], a["obuf"],
                       a["hyper"], a["n_groups"], C.B1, C.B2, C.EPS_ADAM, 1.0, None, mirror, 1)

    acc = torch.full((256,), 0.25, device=dev)

    def axpby(**kw):
        a = dict(acc=acc, cin=x[2], out=x[3], n=64)
        a.update(kw)
        ops.muon_axpby(a["acc"], a["cin"], a["out"], a["n"], 2.0, 3.0)

    for kw in (dict(n=0), dict(n=100), dict(n=-64), dict(n_tensors=0), dict(n_tensors=(1 << 20) + 1), dict(slot_tensor=None),
               dict(info=None), dict(ubuf=None), dict(sums=None), dict(slot0=-1), dict(mu=1.5), dict(mu=-0.1)):
        with pytest.raises(E, match="sc_muon_momentum:"):
            momentum(**kw)
    for kw in (dict(n_slots=0), dict(n_slots=-1), dict(n_tensors=0), dict(sums=None), dict(info=None),
               dict(eps=0.0), dict(ubuf=None), dict(xbuf=None), dict(norms=None), dict(xbuf=x[1])):
        with pytest.raises(E, match="sc_muon_scale:"):
            scale(**kw)
    for kw in (dict(n=0), dict(n=100), dict(n_groups=0), dict(n_groups=257), dict(n_tensors=-1), dict(n_tensors=(1 << 20) + 1),
               dict(chunk=None), dict(slot_tensor=None), dict(hyper=None), dict(info=None), dict(ratio=None), dict(obuf=None),
               dict(slot0=-1)):
        with pytest.raises(E, match="sc_muon_apply:"):
            apply(**kw)
    for kw in (dict(n=0), dict(n=-8), dict(n=12), dict(acc=None), dict(cin=None), dict(out=None)):
        with pytest.raises(E, match="sc_muon_axpby:"):
            axpby(**kw)
    # buffers too small for what a launch would touch are refused before the library is called
    with pytest.raises(ValueError, match="muon_momentum: slot_tensor holds 1 elements, 2 are needed"):
        momentum(slot_tensor=slot_tensor[:1])
    with pytest.raises(ValueError, match="muon_momentum: ubuf holds 32 elements, 64 are needed"):
        momentum(ubuf=x[1][:32])
    with pytest.raises(ValueError, match="muon_scale: norms holds 0 elements, 1 are needed"):
        scale(norms=norms[:0])
    with pytest.raises(ValueError, match="muon_apply: group_hyper holds 2 floats"):
        apply(hyper=hyper[:2])
    with pytest.raises(ValueError, match="muon_apply: v holds 64 floats"):
        ops.muon_apply(bufs[0], bufs[1], bufs[2], bufs[3][:64], n, chunk, slot_tensor, info, ratio, 1, 0, x[1], hyper, 1, C.B1, C.B2,
                       C.EPS_ADAM, 1.0, None, mirror, 1)
    with pytest.raises(ValueError, match="muon_axpby: out holds 32 elements, 64 are needed"):
        axpby(out=x[3][:32])
    with pytest.raises(ValueError, match="muon_axpby: acc holds 256 floats, n = 512"):
        axpby(n=512)
    with pytest.raises(ValueError, match="muon_axpby: out must not be cin"):
        axpby(out=x[2])
    with pytest.raises(TypeError, match="slot_tensor: expected torch.int32"):
        momentum(slot_tensor=slot_tensor.to(torch.uint8))
    # misaligned buffers, straight at the C ABI
    assert lib.sc_muon_momentum(bufs[1].data_ptr() + 4, bufs[2].data_ptr(), 64, slot_tensor.data_ptr(), info.data_ptr(), 1, 0, 0.95, 0.05,
                                1, 1.0, None, x[1].data_ptr(), sums.data_ptr(), None) != 0
    assert b"16-byte aligned" in lib.sc_last_error()
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs) and bool((mirror == -1000.0).all())
    assert bool((sums == -7.0).all()) and bool((norms == -7.0).all()) and all(bool((t == -3.0).all()) for t in x) and bool((acc == 0.25).all())


def test_a_table_outside_the_buffer_is_not_followed():
    """The tables live in device memory, out of the host's sight: a slot whose tensor index is not below n_tensors, or whose
    tensor's slot range does not hold it, is left alone; a tensor whose range lies outside the sums is not scaled."""
    ops, dev = _ops(), _dev()
    n = 192
    p, g, m, v = (torch.full((n,), 0.5, device=dev) for _ in range(4))
    mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
    slot_tensor = torch.tensor([4, 1 << 30, 0], dtype=torch.int32, device=dev)         # slot 2 names tensor 0, whose range is slot 0
    info = torch.tensor([[0, 1, 0, 0], [2, 9, 0, 0], [-1, 1, 0, 0], [2, 1, 0, 0]], dtype=torch.int32, device=dev)
    sums = torch.full((3,), 4.0, device=dev)
    norms = torch.full((4,), NAN, device=dev)
    x0 = torch.full((64 * 4,), -3.0, dtype=torch.bfloat16, device=dev)
    x1 = torch.full((64 * 4,), 2.0, dtype=torch.bfloat16, device=dev)
    chunk = torch.zeros(3, dtype=torch.uint8, device=dev)
    hyper = torch.full((4,), 1e-3, device=dev)
    ops.muon_momentum(g, m, n, slot_tensor, info, 4, 0, 0.95, True, 1.0, None, x1, sums, 4)
    ops.muon_scale(sums, 3, info, 4, 1e-7, x1, x0, norms, 4)
    ops.muon_apply(p, g, m, v, n, chunk, slot_tensor, info, torch.ones(4, device=dev), 4, 0, x1, hyper, 1, C.B1, C.B2, C.EPS_ADAM, 1.0,
                   None, mirror, 4)
    torch.cuda.synchronize()
    assert all(bool((t == 0.5).all()) for t in (p, m, v)) and bool((mirror == -1000.0).all()) and bool((sums == 4.0).all())
    assert float(norms[0]) == 2.0 and bool(torch.isnan(norms[1:]).all())
    assert bool((x0[:64] == 1.0).all()) and bool((x0[64:] == -3.0).all())        # tensor 0 alone was scaled: 2 / ||.|| = 2 / 2


# ================================================================================================ through the net
# The learning rate of the short run: torch.optim.Muon (adjust_lr_fn="match_rms_adamw", weight_decay 0.05) on the 16 block
# Linears plus torch.optim.AdamW on the rest, on the CPU oracle model (oracle/spatial_clip_oracle.py) of the same configuration,
# 20 steps on batch 0 with a clip at 1: lr 1e-3 takes the loss 3.131 -> 0.002, 3e-3 -> 0.001 (below 0.02 from step 8 on), 1e-2 ->
# 0.001, 3e-2 -> 0.006 with three rises on the way, 1e-1 stalls at 2.485.  3e-3 is the value used.
LR_RUN = 3.0e-3
LR, WDECAY, ADAM_BETAS, ADAM_EPS = 2.0e-2, 0.05, (0.9, 0.999), 1.0e-8      # LR: large enough to recover O from the weights
BLOCK_LEAVES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, optim, streams
    return data, graph, losses, mc, module, net, optim, streams


def _net(seed=3, lock_image=False, text=True):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=mc.TextCfg(16, 97, 64, 2, 2) if text else None,
                      gene=None if text else mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    if lock_image:
        n.lock_image_tower(0)
    return n


def _module(n, param_groups=None, warmup=0, total=40, cls="FusedMuon", **opt_kw):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    kw = dict(lr=LR, weight_decay=WDECAY, adamw_betas=ADAM_BETAS, adamw_eps=ADAM_EPS) if cls == "FusedMuon" else \
        dict(lr=LR, weight_decay=WDECAY, betas=ADAM_BETAS, eps=ADAM_EPS)
    kw.update(opt_kw)
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), functools.partial(getattr(optim, cls), **kw),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup), param_groups=param_groups)

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    assert isinstance(oc["optimizer"], getattr(optim, cls))
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _batch(step, B=12, text=True):
    data, *_ = _pkg()
    b = data.synthetic_batch(B, 32, 200, K=4, step=step)
    if text:
        b["texts"] = data.synthetic_captions(B, 16, 97, seed=step)
    return {k: v.cuda() for k, v in b.items()}


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


def _state(opt):
    st = opt.store
    st.wait_all()
    torch.cuda.synchronize()
    return st.master.detach().cpu().clone(), _full(opt, opt.exp_avg).cpu(), _full(opt, opt.exp_avg_sq).cpu()


def _check_against_the_rules(name, opt, before, grad_scale=1.0, clipped=True):
    """Masters and moments after ``opt.step`` from the state ``before``, on the net's own gradient and the clip coefficient the
    step left in ``norm_clip``: every Muon tensor under the rules for B and O with its group's scalars, every AdamW slot with the
    bits of ``ops.adamw_step_groups`` run on the same inputs; what is no trainable tensor keeps its bits; mirror = bf16(master)."""
    ops = _ops()
    st = opt.store
    dev = st.master.device
    got = _state(opt)
    g = st.grad.detach().cpu()
    c = float(opt.norm_clip[1]) if clipped else 1.0
    ge64, ge32 = C.effective(g, c, torch.float64, grad_scale), C.effective(g, c, torch.float32, grad_scale)
    group_of = {n: gi for gi, grp in enumerate(opt.param_groups) for n in grp["param_names"]}
    for name_t in opt.muon_names:
        sp = st.by_name[name_t]
        r, cc = sp.shape
        s = slice(sp.offset, sp.offset + sp.numel)
        grp = opt.param_groups[group_of[name_t]]
        assert grp["use_muon"]
        p0, b0 = before[0][s].reshape(r, cc), before[1][s].reshape(r, cc)
        C.check_b(f"{name} {name_t} B", got[1][s].reshape(r, cc), b0, ge64[s].reshape(r, cc), ge32[s].reshape(r, cc), opt.momentum)
        _, u32 = C.update_of(b0, ge32[s].reshape(r, cc), opt.momentum, opt.nesterov, torch.float32)
        p_t, _ = C.torch_step(p0, b0, ge32[s].reshape(r, cc), grp["lr"], grp["weight_decay"], opt.momentum, opt.nesterov,
                              opt.adjust_lr_fn, opt.ns_coefficients, opt.ns_steps, opt.muon_eps)
        lr_adj = _f32(grp["lr"]) * C.adjust_ratio(opt.adjust_lr_fn, r, cc)
        C.check_o(f"{name} {name_t}", C.recover_o(p0, got[0][s].reshape(r, cc), grp["lr"], grp["weight_decay"], lr_adj),
                  C.recover_o(p0, p_t, grp["lr"], grp["weight_decay"], lr_adj), C.ns64(u32, opt.ns_coefficients, opt.ns_steps, opt.muon_eps))
        assert torch.equal(_bits(got[2][s]), _bits(before[2][s])), f"{name_t}: exp_avg_sq of a Muon tensor changed"
    # the AdamW part: the grouped AdamW kernel on copies of the state before, with the scalar table of this step
    host = torch.zeros(opt.group_hyper.numel(), dtype=torch.float32)
    opt._fill_group_hyper(host)
    p, m, v = (t.clone().to(dev) for t in before)
    mirror = torch.zeros(st.total, dtype=torch.bfloat16, device=dev)
    b1, b2 = opt.param_groups[0]["betas"]
    ops.adamw_step_groups(p, st.grad, m, v, st.total, opt.chunk_group, host.to(dev), len(opt.param_groups), b1, b2,
                          opt.param_groups[0]["eps"], grad_scale, opt.norm_clip if clipped else None, mirror)
    torch.cuda.synchronize()
    mask = _trainable_mask(st).cpu()
    adamw = (opt.slot_tensor_host == -1).repeat_interleave(64) & mask
    assert 0 < int(adamw.sum()) < int(mask.sum()) or not opt.muon_names
    for a, b, what in zip(got, (p.cpu(), m.cpu(), v.cpu()), ("weights", "exp_avg", "exp_avg_sq")):
        assert torch.equal(_bits(a[adamw]), _bits(b[adamw])), f"{name}: {what} of the AdamW part differ from adamw_step_groups"
    for x, y in zip(got, before):
        assert torch.equal(_bits(x[~mask]), _bits(y[~mask])), "floats of no trainable tensor changed"
    assert torch.equal(_bits(st.master_bf16.detach().cpu()[mask]), _bits(got[0][mask].to(torch.bfloat16))), "mirror != bf16(master)"
    return c


def _force_a_clip(store):
    """An active clip at max_norm = 1 and grad_scale = 0.5: a gradient of norm below 4 is scaled up to norm 4."""
    norm = float(store.grad.double().norm())
    if norm < 4.0:
        store.grad.mul_(4.0 / norm)


def _random_moments(opt, seed=5):
    """Moments on the parameters, none on the padding between them.  With them the update U of a Muon tensor has full rank, and
    the O check through the net proves offsets, groups, ratios and the transposed products on the net's own layout.  The raw
    gradient of a 12-sample batch is rank-deficient (smallest / largest singular value 1e-8 and below), and there the iteration
    amplifies bf16 rounding noise to full size.  Recorded in profiles/muon_raw_gradient.txt (tools/muon_raw_gradient.py: this
    net, zero moments, inputs bit-identical): torch's own deviation from float64 is 0.04 - 0.25, the kernels' is 0.86 - 2.81 x
    of it (1.58 and 2.81 on two of 24 tensors), while the kernels' and the CPU emulation's (tests/_muoncases.ns_emulated)
    deviations agree to three digits on every tensor and the two results lie within 0.9 % of ||O|| of each other.  Like the
    shapes below 64, that is two correct bf16 implementations differing, and no ground for the rule.  The accumulated Trainer
    step below does run the rule on a raw gradient (the gene-MLP net's, ratios 0.95 - 1.05 there); the rank-deficient kinds
    the rule covers by construction (rows of zeros, an all-zero update) are in the kernel tests."""
    st = opt.store
    gen = torch.Generator().manual_seed(seed)
    m_init, v_init = torch.zeros(st.total), torch.zeros(st.total)
    for sp in st.specs:
        m_init[sp.offset:sp.offset + sp.numel] = 0.01 * torch.randn(sp.numel, generator=gen)
        v_init[sp.offset:sp.offset + sp.numel] = (0.01 * torch.randn(sp.numel, generator=gen)) ** 2
    for k, (lo, hi) in enumerate(opt.ranges):
        m, v = opt._moments(k, lo, hi)
        m.copy_(m_init[lo:hi])
        v.copy_(v_init[lo:hi])


def test_default_split_puts_exactly_the_block_linears_under_muon():
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    n = _net()
    st = n.store
    opt = optim.FusedMuon(list(st.params.values()), lr=LR)
    want = [sp.name for sp in st.specs if ".resblocks." in sp.name and sp.name.endswith(BLOCK_LEAVES)]
    assert len(want) == 16 and opt.muon_names == want           # two towers x two blocks x four Linears
    assert sum(n_.startswith("visual.") for n_ in want) == 8
    assert [g["use_muon"] for g in opt.param_groups] == [True, False]
    assert sorted(opt.param_groups[0]["param_names"]) == sorted(want)
    assert len(opt.param_groups[1]["param_names"]) == len(st.specs) - 16
    assert sorted(set(opt.muon_shapes)) == [(64, 64), (64, 256), (192, 64), (256, 64)] and len(opt.muon_shapes) == 16
    # through the module: parameters() un-grouped, as the reference's configure_optimizers passes them
    m, opt2, sched = _module(_net())
    assert opt2.muon_names == want and [g["use_muon"] for g in opt2.param_groups] == [True, False]


@pytest.mark.parametrize("adjust,nesterov", [(None, True), ("match_rms_adamw", False)])
def test_one_step_through_the_net_meets_the_rules_per_tensor(monkeypatch, adjust, nesterov):
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BEHIND", "0")
    n = _net()
    m, opt, sched = _module(n, {"no_decay": "open_clip"}, adjust_lr_fn=adjust, nesterov=nesterov, adamw_lr=1e-3)
    st = n.store
    assert [(g["use_muon"], g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(False, 1e-3, 0.0), (True, LR, WDECAY),
                                                                                      (False, 1e-3, WDECAY)]
    _random_moments(opt)
    _backward(m, _batch(0))
    st.wait_all()
    torch.cuda.synchronize()
    _force_a_clip(st)
    before = _state(opt)
    nc = opt.step(grad_scale=0.5, max_norm=1.0)
    c = _check_against_the_rules("one step", opt, before, grad_scale=0.5)
    norm = 0.5 * float(st.grad.double().norm())
    assert abs(float(nc[0]) - norm) < 1e-5 * norm and abs(c - 1.0 / norm) < 1e-5 * c
    assert opt.step_count == 1 and not torch.equal(st.master.cpu(), before[0])


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
                     opt.norms.clone())
        losses_of[form] = ls
    first = forms[0]
    for form in forms[1:]:
        assert losses_of[form] == losses_of[first], losses_of
        for a, b, what in zip(res[first], res[form], ("weights", "exp_avg", "exp_avg_sq", "bf16 mirror", "update norms")):
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
    w, *_, norms = _run_forms(("behind", "one_launch", "graph"), 4, make, monkeypatch)
    assert not torch.equal(w, _net().store.master) and bool((norms > 0).all()) and norms.numel() == 16


def test_with_every_group_on_adamw_the_bits_are_fused_adamws(monkeypatch):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BEHIND", "0")
    batches = [_batch(s) for s in range(3)]
    res = {}
    for cls in ("FusedAdamW", "FusedMuon"):
        n = _net()

        def groups(net_, cls=cls):
            gs = optim.open_clip_param_groups(net_.store.params.items(), WDECAY)
            return [dict(g, use_muon=False) for g in gs] if cls == "FusedMuon" else gs
        m, opt, sched = _module(n, groups, warmup=1, cls=cls, lr=1e-3)
        assert len(opt.param_groups) == 2
        if cls == "FusedMuon":
            assert opt.muon_names == [] and not any(g["use_muon"] for g in opt.param_groups)
        gstep = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        for b in batches:
            gstep.eager(b)
            sched.step()
        n.store.wait_all()
        torch.cuda.synchronize()
        res[cls] = (n.store.master.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), n.store.master_bf16.clone())
    for a, b, what in zip(res["FusedAdamW"], res["FusedMuon"], ("weights", "exp_avg", "exp_avg_sq", "mirror")):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: FusedMuon on AdamW alone differs from FusedAdamW"
    assert not torch.equal(res["FusedMuon"][0], _net().store.master)


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
    # a locked matrix is no tensor and runs no Newton-Schulz iteration
    assert len(opt.muon_names) == 8 and not any(name.startswith("visual.") for name in opt.muon_names)
    assert len(opt.muon_shapes) == 8 and opt.x0.numel() == sum(st.by_name[x].numel for x in opt.muon_names)
    p0 = st.master.detach().clone()
    sched.step()        # past the lr = 0 of the first scheduler position
    _random_moments(opt)
    _backward(m, batches[0])
    before = _state(opt)
    opt.step(grad_scale=1.0, max_norm=1.0)
    _check_against_the_rules("locked step", opt, before)
    sched.step()
    run(m, opt, sched, (1,))
    assert torch.equal(_bits(st.master[~mask]), _bits(p0[~mask])) and not torch.equal(st.master[mask], p0[mask])
    ckpt = {"net": {k: v.cpu() for k, v in n.state_dict().items()}, "opt": opt.state_dict(), "sched": sched.last_epoch}
    assert list(ckpt["opt"]) == ["optimizer", "step", "exp_avg", "exp_avg_sq", "param_groups"] and ckpt["opt"]["optimizer"] == "muon"
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
    # resumed without the lock: the full-layout moments are taken as they are, and now the image tower trains under Muon too
    n3 = _net(seed=5)
    m3, opt3, sched3 = _module(n3, warmup=1)
    n3.load_state_dict(ckpt["net"])
    opt3.load_state_dict(ckpt["opt"])
    assert opt3.exp_avg.numel() == st.total and opt3.step_count == 2 and len(opt3.muon_names) == 16
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(opt3.state_dict()[key].cpu()), _bits(ckpt["opt"][key].cpu()))
    sched3.last_epoch = ckpt["sched"]
    sched3._apply()
    run(m3, opt3, sched3, (2,))
    assert not torch.equal(n3.store.master[~mask], p0[~mask])
    # an AdamW optimiser refuses the file
    m4, opt4, sched4 = _module(_net(seed=5), cls="FusedAdamW")
    with pytest.raises(ValueError, match="(?s)FusedAdamW.*'muon'.*'adamw'"):
        opt4.load_state_dict(ckpt["opt"])


def test_trainer_accumulated_step_meets_the_rules(monkeypatch):
    """``Trainer(accumulate_grad_batches=2)`` over two batches: one optimiser step on the folded gradient (still in
    ``store.grad``), its norm finished from the fold's partial sums.  (The synthetic data module feeds the gene tower: the
    image tower's eight block Linears run Muon.)"""
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    n = _net(text=False)
    p0 = n.store.master.detach().cpu().clone()
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedMuon, lr=LR, weight_decay=WDECAY, adamw_lr=1e-3),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=0))
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=2, val_steps=1)
    tr = Trainer(max_epochs=1, gradient_clip_val=1.0, log_every_n_steps=1, accumulate_grad_batches=2)
    tr.fit(m, dm)
    opt = tr.optimizer
    assert isinstance(opt, optim.FusedMuon) and opt.step_count == 1 and tr.global_step == 1 and tr.accumulator is not None
    assert len(opt.muon_names) == 8
    n.store.wait_all()
    torch.cuda.synchronize()
    norm = float(n.store.grad.double().norm())
    assert abs(float(opt.norm_clip[0]) - norm) < 1e-5 * norm, "norm_clip does not hold the norm of the folded gradient"
    for g in opt.param_groups:      # the step ran at the schedule's first position: factor 1
        g["lr"] = g["initial_lr"]
    zeros = torch.zeros_like(p0)
    _check_against_the_rules("accumulated step", opt, (p0, zeros, zeros))


@pytest.mark.parametrize("form", ["behind", "graph"])
def test_the_weight_average_follows(monkeypatch, form):
    from tests import _wavgcases as W
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BUCKET", "4096")
    monkeypatch.setenv("SC_ADAMW_BEHIND", "1" if form == "behind" else "0")
    decay, every, start, steps = 0.9, 2, 2, 5
    n = _net()
    m, opt, sched = _module(n)
    st = n.store
    wa = optim.WeightAverager(st, decay=decay, update_every_n_steps=every, update_starting_at_step=start, kind="ema").attach(opt)
    initial = st.master.detach().clone().cpu()
    gstep = graph.GraphedTrainStep(m, opt, max_norm=1.0)
    snaps = []
    for s in range(steps):
        gstep(_batch(s)) if form == "graph" else gstep.eager(_batch(s))
        sched.step()
        st.wait_all()
        snaps.append(st.master.detach().clone().cpu())
        torch.cuda.synchronize()
    if form == "graph":
        assert gstep.failed is None and gstep.replays == steps - 1, (gstep.failed, gstep.replays)
    mask = _trainable_mask(st).cpu()
    want, n_avg = W.oracle_run(snaps, "ema", decay, every, start, initial, mask)
    assert wa.n_averaged == n_avg == 2
    W.assert_same_bits(wa.avg.detach().cpu(), want, f"{form}: average against the oracle over its own snapshots")
    assert not torch.equal(wa.avg.detach().cpu(), snaps[-1]) and not torch.equal(wa.avg.detach().cpu(), initial)


def test_twenty_steps_on_one_batch_lower_the_loss(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    n = _net()
    m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    opt = optim.FusedMuon(list(n.store.params.values()), lr=LR_RUN, weight_decay=WDECAY, adjust_lr_fn="match_rms_adamw")
    batch = _batch(0)
    ls = []
    for _ in range(20):
        ls.append(float(_backward(m, batch).detach()))
        opt.step(grad_scale=1.0, max_norm=1.0)
    n.store.wait_all()
    torch.cuda.synchronize()
    print("  loss", " ".join(f"{x:.4f}" for x in ls))
    assert ls[-1] < 0.5 * ls[0], ls
