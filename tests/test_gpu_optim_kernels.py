"""Optimiser kernels (spatial-clip_amd/csrc/sc_optim.hip) at the sizes where their loops change shape, against PyTorch in
float64 on the CPU (tests/_refbounds.py states the bounds).

sumsq_partial_kernel (1024 blocks x 256 threads = 262144-thread stride over float4s): the 4-way unrolled main loop runs only
above 3 145 728 floats (4 strides of float4s), the remainder loop below, and one thread adds the n % 4 tail.  adamw_kernel
caps its grid at 4096 blocks (4 194 304 floats): above that the grid-stride loop wraps."""
import functools
import math

import pytest
import torch

from tests import _refbounds as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNROLL_N = 4 * 3 * 262144         # the unrolled loop needs i + 3 * stride < n / 4 for some thread
ADAM_WRAP_N = 4096 * 256 * 4       # adamw grid cap in floats


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _sumsq_path(n):
    tags = ["unrolled" if n // 4 > UNROLL_N // 4 else "remainder-loop-only"]
    tags.append(f"tail{n % 4}" if n % 4 else "no-tail")
    return "-".join(tags)


# ---------------------------------------------------------------------------------------------------------- grad norm
GN_SIZES = [4, 5, 7, 4004, 3145728, 3145734, 50000003]
GN_TARGET = 4.0          # norm of every input: with grad_scale 1 the clip at max_norm 1 is active, with 1/8 it is not


@functools.lru_cache(maxsize=1)
def _gn_input(n):
    """randn with the n % 4 tail made heavy (each tail element carries as much square as the whole body), scaled to norm
    GN_TARGET: a dropped or doubled tail moves the norm by far more than the bound."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    t = n % 4
    if t:
        x[n - t:] = math.sqrt(n) * torch.tensor([1.0, -0.75, 0.5])[:t]
    x *= GN_TARGET / float(x.double().norm())
    return x, x.to(_dev())


@pytest.fixture(scope="module", autouse=True)
def _release_cached_input():
    """The last grad-norm input (up to 200 MB on the device plus its host copy) is not kept past this module."""
    yield
    _gn_input.cache_clear()


GN_CASES = [(n, gs, mn) for n in GN_SIZES for gs in (1.0, 0.125) for mn in (0.0, 1.0)]


def _clip_ref(norm64, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient, capped at 1; max_norm 0 means no clipping (the trainer's
    gradient_clip_val convention, and the kernel's)."""
    return 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm64 + 1e-6))


def _check_norm_clip(tag, out, norm64, max_norm):
    got_norm, got_clip = float(out[0]), float(out[1])
    rel = abs(got_norm - norm64) / norm64
    clip64 = _clip_ref(norm64, max_norm)
    crel = abs(got_clip - clip64) / clip64
    print(f"  {tag}: norm rel err {rel:.3g} (ratio {rel / R.GRAD_NORM_REL:.3g}), clip {got_clip:.7g} rel err {crel:.3g} "
          f"(ratio {crel / R.CLIP_REL:.3g})")
    assert rel <= R.GRAD_NORM_REL, f"{tag}: norm {got_norm} vs {norm64}"
    if clip64 == 1.0:
        assert got_clip == 1.0, f"{tag}: inactive clip must be exactly 1, got {got_clip}"
    else:
        assert crel <= R.CLIP_REL, f"{tag}: clip {got_clip} vs {clip64}"
    return max(rel / R.GRAD_NORM_REL, crel / R.CLIP_REL)


@pytest.mark.parametrize("n,gs,max_norm", GN_CASES,
                         ids=[f"n{n}-{_sumsq_path(n)}-gs{gs:g}-max{mn:g}" + ("-clip" if mn > 0 and GN_TARGET * gs > mn else "")
                              for n, gs, mn in GN_CASES])
def test_grad_norm(n, gs, max_norm):
    """sc_grad_norm: norm * grad_scale within GRAD_NORM_REL of float64, the clip coefficient as clip_grad_norm_ forms it."""
    ops = _ops()
    x, xd = _gn_input(n)
    norm64 = float(x.double().norm()) * gs
    out = torch.full((2,), NAN, device=xd.device)
    ops.workspace(1024, xd.device, "gn", torch.float64).fill_(NAN)
    ops.grad_norm(xd, n, gs, max_norm, out)
    _check_norm_clip(f"grad_norm n={n}", out.cpu(), norm64, max_norm)


SHARD_N = 16_000_004


def _pieces(n, w):
    """W contiguous pieces of unequal length, each a multiple of 4 (the last takes what remains)."""
    cuts = [0]
    for j in range(1, w):
        cuts.append(int(n * (j + 0.1 * (-1) ** j) / w) // 4 * 4)
    cuts.append(n)
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("w", [1, 2, 3, 8], ids=lambda w: f"W{w}")
def test_grad_norm_sharded(w):
    """sc_grad_sumsq_partial per piece into its own 1024 fp64 slots, then sc_grad_norm_final over 1024 * W slots: the same
    bound as one launch; a single piece gives the bits of sc_grad_norm.  Pieces of 8 M floats run the unrolled loop, those
    of the 8-way split only the remainder loop."""
    ops = _ops()
    dev = _dev()
    g = torch.Generator().manual_seed(w)
    x = torch.randn(SHARD_N, generator=g) * 1e-3
    xd = x.to(dev)
    norm64 = float(x.double().norm())
    max_norm = 0.5 * norm64
    partial = torch.full((1024 * w,), NAN, dtype=torch.float64, device=dev)
    for k, (a, b) in enumerate(_pieces(SHARD_N, w)):
        assert (b - a) % 4 == 0
        ops.grad_sumsq_partial(xd[a:b], b - a, partial[1024 * k:1024 * (k + 1)])
    out = torch.full((2,), NAN, device=dev)
    ops.grad_norm_final(partial, 1024 * w, 1.0, max_norm, out)
    _check_norm_clip(f"sharded W={w}", out.cpu(), norm64, max_norm)
    if w == 1:
        one = torch.full((2,), NAN, device=dev)
        ops.grad_norm(xd, SHARD_N, 1.0, max_norm, one)
        assert torch.equal(out, one)


# ---------------------------------------------------------------------------------------------------------- AdamW
ADAM_SIZES = [4, 4004, 4194304, 4194308, 33554436]
LR, B1, B2, EPS, WD, GS = 1e-3, 0.9, 0.98, 1e-6, 0.1, 0.5
# steps 1-3 at lr 1e-3, then step 1000 at a warm-up lr of 1e-7
ADAM_STEPS = [(1, 1e-3), (2, 1e-3), (3, 1e-3), (1000, 1e-7)]


def _adam_path(n):
    """Passes of the grid-stride loop: 4096 blocks x 256 threads, one float4 each per pass."""
    if n > ADAM_WRAP_N:
        return f"grid-wrap-{math.ceil(n / ADAM_WRAP_N)}-passes"
    return "grid-exactly-capped" if n == ADAM_WRAP_N else "no-wrap"


def _adam_grad(n, step):
    """Gradient of one step; elements 1, 98, 195, ... are zero at every step, so their v stays 0 and the denominator is eps
    alone."""
    g = torch.Generator().manual_seed(1000 * n + step)
    x = torch.randn(n, generator=g) * 0.1
    x[1::97] = 0.0
    return x


def _torch_adamw(p, m, v, grad, step, lr, dtype):
    """One torch.optim.AdamW(foreach=False) step in ``dtype`` from the given state; hyper-parameters at the fp32 values the
    kernel receives."""
    pp = p.to(dtype).clone()
    opt = torch.optim.AdamW([pp], lr=_f32(lr), betas=(_f32(B1), _f32(B2)), eps=_f32(EPS), weight_decay=_f32(WD), foreach=False)
    pp.grad = grad.to(dtype)
    opt.state[pp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    opt.step()
    st = opt.state[pp]
    return pp.detach(), st["exp_avg"], st["exp_avg_sq"]


ADAM_CASES = [(n, clip) for n in ADAM_SIZES for clip in (False, True)]


@pytest.mark.parametrize("n,clip", ADAM_CASES, ids=[f"n{n}-{_adam_path(n)}-" + ("clip" if c else "noclip") + "-mirror"
                                                  for n, c in ADAM_CASES])
def test_adamw_step(n, clip):
    """sc_adamw_step, each step judged on its own: the float64 reference starts from the kernel's p, m, v and gets the gradient
    times grad_scale times the clip coefficient read back from the kernel's norm_clip; p, m, v reference-relative; the bf16
    mirror is bf16(p) bit for bit."""
    ops = _ops()
    dev = _dev()
    g0 = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g0)
    pd, md, vd = p.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ratios = []
    for step, lr in ADAM_STEPS:
        grad = _adam_grad(n, step)
        gd = grad.to(dev)
        nc = None
        if clip:
            nc = torch.full((2,), NAN, device=dev)
            ops.grad_norm(gd, n, GS, 0.5 * float(grad.double().norm()) * GS, nc)       # max_norm: half the norm, clip ~0.5
        p0, m0, v0 = pd.cpu(), md.cpu(), vd.cpu()
        mirror = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        ops.adamw_step(pd, gd, md, vd, n, lr, B1, B2, EPS, WD, step, GS, nc, mirror)
        torch.cuda.synchronize()
        c = float(nc[1]) if clip else 1.0
        if clip:
            assert c < 1.0
        ref64 = _torch_adamw(p0, m0, v0, grad.double() * GS * c, step, lr, torch.float64)
        ref32 = _torch_adamw(p0, m0, v0, grad * GS * _f32(c), step, lr, torch.float32)
        for name, got, r64, r32 in zip(("p", "m", "v"), (pd, md, vd), ref64, ref32):
            ratios.append(R.check_f32(f"step {step} {name}", got, R.Ref(r64, r32)))
        assert torch.equal(mirror.cpu(), pd.cpu().to(torch.bfloat16)), f"step {step}: mirror != bf16(p)"
        assert bool((vd[1::97] == 0).all()) and bool((md[1::97] == 0).all())
    print(f"[adamw n={n} clip={clip}] max ratio {max(ratios):.3g}")


@pytest.mark.parametrize("n", ADAM_SIZES, ids=[f"n{n}-{_adam_path(n)}" for n in ADAM_SIZES])
def test_adamw_step_dev_same_bits(n):
    """sc_adamw_step_dev (the graph-captured form) with hyper from sc_adamw_hyper_host gives the bits of sc_adamw_step in p,
    m, v and the mirror at every step."""
    ops = _ops()
    from spatial_clip_amd import _lib
    dev = _dev()
    p = torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
    a = [p.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    b = [t.clone() for t in a]
    for step, lr in ADAM_STEPS:
        gd = _adam_grad(n, step).to(dev)
        nc = torch.full((2,), NAN, device=dev)
        ops.grad_norm(gd, n, GS, 0.5 * float(gd.double().norm()) * GS, nc)
        hyper_host = torch.zeros(3, dtype=torch.float32)
        _lib.check(_lib.lib().sc_adamw_hyper_host(float(lr), B1, B2, step, hyper_host.data_ptr()), "sc_adamw_hyper_host")
        hyper = hyper_host.to(dev)
        ma = torch.full((n,), -1000.0, dtype=torch.bfloat16, device=dev)
        mb = ma.clone()
        ops.adamw_step(a[0], gd, a[1], a[2], n, lr, B1, B2, EPS, WD, step, GS, nc, ma)
        ops.adamw_step_dev(b[0], gd, b[1], b[2], n, hyper, B1, B2, EPS, WD, GS, nc, mb)
        torch.cuda.synchronize()
        for name, x, y in zip(("p", "m", "v"), a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"step {step}: {name}"
        assert torch.equal(ma.view(torch.int16), mb.view(torch.int16)), f"step {step}: mirror"
