"""sc_adamw_step_groups (spatial-clip_amd/csrc/sc_optim.hip): AdamW over a flat buffer of 64-float slots with a group per slot
and a learning rate and weight decay per group, one launch per range.

Every slot of group g must carry the BITS of sc_adamw_step run on a contiguous copy of exactly that group's slots with
(lr_g, wd_g) -- p, both moments and the bf16 mirror -- and p, m, v must meet the reference-relative rule of
tests/test_gpu_optim_kernels.py::test_adamw_step against float64 torch.optim.AdamW built with real parameter groups
(tests/_groupcases.py; tests/test_cpu_param_groups.py holds torch's own fp32 grouped step to the same rule on these inputs).
Shapes: one slot; five slots in three groups, one of them with lr = 0; the same five slots launched as two ranges with the
table pointer offset; past the 4096-block grid cap with 256 groups that change at every slot."""
import functools

import pytest
import torch

from tests import _groupcases as C
from tests import _refbounds as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _case(name):
    return C.CASES[name]()


def _hyper_dev(ops, case, base_lr, step):
    hyper = case.group_hyper(base_lr)
    host = torch.zeros(2 + 2 * case.n_groups, dtype=torch.float32)
    ops.adamw_groups_hyper_host([lr for lr, _ in hyper], [wd for _, wd in hyper], C.B1, C.B2, step, host)
    return host.to(_dev()), hyper


def _launch(ops, case, state, gd, table, hyper_dev, nc, mirror, ranges):
    pd, md, vd = state
    for lo, hi in ranges:
        ops.adamw_step_groups(pd[lo:hi], gd[lo:hi], md[lo:hi], vd[lo:hi], hi - lo, table[lo // C.SLOT:], hyper_dev, case.n_groups,
                              C.B1, C.B2, C.EPS, C.GS, nc, None if mirror is None else mirror[lo:hi])


RANGES = {"one-range": None, "two-ranges": [(0, 128), (128, 320)]}
RUNS = [(name, "one-range") for name in C.CASES] + [("five-slots-three-groups", "two-ranges")]
PARAMS = [(name, rng, clip, mirror) for name, rng in RUNS for clip in (False, True) for mirror in (True, False)]


@pytest.mark.parametrize("name,rng,clip,with_mirror", PARAMS,
                         ids=[f"{n}-{r}-" + ("clip" if c else "noclip") + ("-mirror" if m else "-nomirror") for n, r, c, m in PARAMS])
def test_grouped_step_has_the_bits_of_the_ungrouped_kernel_and_meets_the_float64_rule(name, rng, clip, with_mirror):
    ops = _ops()
    dev = _dev()
    case = _case(name)
    n = case.n
    ranges = RANGES[rng] or [(0, n)]
    p, m, v = C.start(n)
    state = [p.to(dev), m.to(dev), v.to(dev)]
    table = case.slot_group.to(dev)
    frozen = C.FROZEN_GROUP.get(name)
    ratios = []
    for step, lr in C.ADAM_STEPS:
        grad = C._adam_grad(n, step)
        gd = grad.to(dev)
        nc = None
        if clip:
            nc = torch.full((2,), NAN, device=dev)
            ops.grad_norm(gd, n, C.GS, 0.5 * float(grad.double().norm()) * C.GS, nc)        # clip coefficient ~0.5
        before = [t.clone() for t in state]
        p0, m0, v0 = (t.cpu() for t in before)
        mirror0 = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        mirror = mirror0.clone() if with_mirror else None
        hyper_dev, hyper = _hyper_dev(ops, case, lr, step)
        _launch(ops, case, state, gd, table, hyper_dev, nc, mirror, ranges)
        if rng != "one-range":      # the same buffer in ONE launch: the bits must not depend on how it is cut into ranges
            whole = [t.clone() for t in before]
            whole_mirror = mirror0.clone() if with_mirror else None
            _launch(ops, case, whole, gd, table, hyper_dev, nc, whole_mirror, [(0, n)])
            for what, a, b in zip("pmv", state, whole):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"step {step}: {what} depends on the range cut"
            if with_mirror:
                assert torch.equal(mirror.view(torch.int16), whole_mirror.view(torch.int16)), f"step {step}: mirror, range cut"
        # 1. per group: the bits of sc_adamw_step on a contiguous copy of exactly its slots
        for g, (lr_g, wd_g) in enumerate(hyper):
            sub = [case.gather(t, g) for t in before]
            sub_mirror = torch.full((sub[0].numel(),), -1000.0, dtype=torch.bfloat16, device=dev) if with_mirror else None
            ops.adamw_step(sub[0], case.gather(gd, g), sub[1], sub[2], sub[0].numel(), lr_g, C.B1, C.B2, C.EPS, wd_g, step, C.GS,
                           nc, sub_mirror)
            for what, got, want in zip("pmv", state, sub):
                assert torch.equal(case.gather(got, g).view(torch.int32), want.view(torch.int32)), \
                    f"step {step} group {g} (lr {lr_g}, wd {wd_g}): {what} differs from sc_adamw_step on the group's slots"
            if with_mirror:
                assert torch.equal(case.gather(mirror, g).view(torch.int16), sub_mirror.view(torch.int16)), \
                    f"step {step} group {g}: mirror differs from sc_adamw_step's"
        torch.cuda.synchronize()
        pd, md, vd = state
        # 2. float64 torch.optim.AdamW with real parameter groups, each step from the kernel's own state
        c = float(nc[1]) if clip else 1.0
        if clip:
            assert c < 1.0
        ref64 = C.torch_grouped(case, p0, m0, v0, grad.double() * C.GS * c, step, lr, torch.float64)
        ref32 = C.torch_grouped(case, p0, m0, v0, grad * C.GS * C._f32(c), step, lr, torch.float32)
        worst = 0.0
        for g in range(case.n_groups):
            for what, got, r64, r32 in zip("pmv", (pd, md, vd), ref64[g], ref32[g]):
                ref = R.Ref(r64, r32)
                got_g = case.gather(got, g).cpu().double()
                ratio = R._ratio((got_g - ref.r64).abs(), ref.allowed_f32())
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"step {step} group {g} {what}: error / allowed = {ratio} (E32 = {ref.e32})"
        ratios.append(worst)
        # 3. the mirror is bf16(p), bit for bit; without one nothing is written
        if with_mirror:
            assert torch.equal(mirror.cpu().view(torch.int16), pd.cpu().to(torch.bfloat16).view(torch.int16)), f"step {step}: mirror"
        assert bool((vd[1::97] == 0).all()) and bool((md[1::97] == 0).all())
        if frozen is not None:      # lr = 0: weights and mirror keep their bits, the moments advance
            assert torch.equal(case.gather(pd, frozen).view(torch.int32), case.gather(before[0], frozen).view(torch.int32))
            assert not torch.equal(case.gather(md, frozen), case.gather(before[1], frozen))
            assert not torch.equal(case.gather(vd, frozen), case.gather(before[2], frozen))
            if with_mirror:
                assert torch.equal(case.gather(mirror, frozen).cpu(), case.gather(before[0], frozen).cpu().to(torch.bfloat16))
    print(f"[adamw groups {name} {rng} clip={clip} mirror={with_mirror}] max ratio {max(ratios):.3g}")


def test_argument_errors_return_without_a_launch():
    """n that is no whole number of slots, n_groups outside 1 .. 256 and a null table or scalar buffer are refused by the
    library; nothing is written."""
    ops = _ops()
    from spatial_clip_amd import _lib
    dev = _dev()
    n = 128
    bufs = [torch.full((n,), 0.5, device=dev) for _ in range(4)]
    table = torch.zeros(n // 64, dtype=torch.uint8, device=dev)
    hyper = torch.zeros(2 + 2 * 256, device=dev)
    hyper[:2] = 0.5
    bad = [dict(n=100), dict(n=0), dict(n_groups=0), dict(n_groups=257), dict(chunk_group=None), dict(group_hyper=None)]
    for kw in bad:
        a = dict(n=n, chunk_group=table, group_hyper=hyper, n_groups=2)
        a.update(kw)
        with pytest.raises(_lib.SpatialClipHipError, match="sc_adamw_step_groups"):
            ops.adamw_step_groups(*bufs, a["n"], a["chunk_group"], a["group_hyper"], a["n_groups"], C.B1, C.B2, C.EPS, 1.0, None)
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs)
    host = torch.zeros(6)
    for lrs, step in (([], 1), ([1e-3] * 257, 1), ([1e-3], 0)):
        with pytest.raises(_lib.SpatialClipHipError, match="sc_adamw_groups_hyper_host"):
            ops.adamw_groups_hyper_host(lrs, [0.0] * len(lrs), C.B1, C.B2, step, torch.zeros(2 + 2 * max(len(lrs), 1)))
    # the bias corrections are the bits sc_adamw_hyper_host forms for the un-grouped captured step
    three = torch.zeros(3)
    _lib.check(_lib.lib().sc_adamw_hyper_host(1e-3, C.B1, C.B2, 7, three.data_ptr()), "sc_adamw_hyper_host")
    ops.adamw_groups_hyper_host([1e-3, 2e-3], [0.1, 0.0], C.B1, C.B2, 7, host)
    assert torch.equal(host[:2], three[1:]) and host[2:].tolist() == [C._f32(1e-3), C._f32(0.1), C._f32(2e-3), 0.0]
