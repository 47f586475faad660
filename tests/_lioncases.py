"""Inputs, float64 / fp32 references and the element rule of the Lion kernel tests (tests/test_gpu_lion.py) and of their
CPU-side check (tests/test_cpu_lion.py).  CPU only: importing this module needs neither a GPU nor the HIP library.

The update (Chen et al. 2023, Algorithm 1), for the effective gradient ge = g * grad_scale * clip:

    c     = beta1 * m + (1 - beta1) * ge
    p_new = p * (1 - lr * wd) - lr * sign(c)        sign(0) = 0, also for -0.0
    m_new = beta2 * m + (1 - beta2) * ge

``step_ref`` is that formula through torch in float64 or fp32, scalars at the fp32 values the kernel receives.  Three chained
steps with a changing learning rate (``STEPS``); every reference step starts from the state the code under test left, as
tests/_groupcases.py does for the Adam moments.

The sign makes ``p`` discontinuous in ``c``: where c is a cancellation of its two terms, fp32 and float64 may land on
different sides of zero and then differ by ``2 * lr``.  Element i is NEAR A TIE when

    |c64| <= 2^-18 * (|beta1 * m| + |(1 - beta1) * ge|)      (and the two terms are not both zero)

An fp32 evaluation of c errs by about three roundings, 2^-22.4 relative to that magnitude, so 2^-18 is a 20x margin.  Where both
terms are zero, c is an exact zero in every precision: no tie, the update is 0.  Outside the band ``p`` and ``m`` meet the
reference-relative rule of tests/_refbounds.py (the rule sc_adamw_step is tested with; E32 taken outside the band).  Inside it
``p`` must be within that allowance of one of the three legal values -- the decayed p minus, plus or without lr -- and ``m``
meets the rule everywhere."""
import functools

import torch

from tests import _refbounds as R

SLOT = 64
B1, B2, WD, GS = 0.9, 0.99, 0.1, 0.5
STEPS = [1e-4, 3e-4, 1e-7]              # learning rate of the three chained steps (the last: a warm-up value)
GRID_CAP_N = 4096 * 256 * 4             # floats one pass of the capped grid covers
SIZES = [64, 320, GRID_CAP_N + 320]     # one slot; five slots; the grid-stride loop takes a second trip
BAND = 2.0 ** -18
BAND_SHARE_CAP = 1e-4                   # of the elements of the large case; about 80x what seeded runs at 4 M elements showed

# slots of the special elements (cases of five slots or more; the one-slot case has none)
ZERO_SLOT, NEG_ZERO_SLOT, MOMENT_ONLY_SLOT = 1, 2, 3


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def slot(k):
    return slice(k * SLOT, (k + 1) * SLOT)


@functools.lru_cache(maxsize=None)
def start(n):
    """p, m before the first step (m is not zero: c has two terms from the first step on).  Slot 1: p = m = 0 (the padding of
    the flat buffers); slot 2: the same, its gradient is -0.0; slot 3: m != 0 under a zero gradient, |p| ~ 1e-3."""
    g = torch.Generator().manual_seed(7 * n + 1)
    p = torch.randn(n, generator=g)
    m = 0.05 * torch.randn(n, generator=g)
    if n >= 5 * SLOT:
        for k in (ZERO_SLOT, NEG_ZERO_SLOT):
            p[slot(k)] = 0.0
            m[slot(k)] = 0.0
        p[slot(MOMENT_ONLY_SLOT)] *= 2.0 ** -10        # small weights: a step of lr = 1e-7 is far above their rounding
    return p, m


@functools.lru_cache(maxsize=None)
def grad(n, step):
    """Gradient of chained step ``step`` (0-based)."""
    g = torch.Generator().manual_seed(1000 * n + step)
    x = 0.1 * torch.randn(n, generator=g)
    if n >= 5 * SLOT:
        x[slot(ZERO_SLOT)] = 0.0
        x[slot(NEG_ZERO_SLOT)] = -0.0
        x[slot(MOMENT_ONLY_SLOT)] = 0.0
    return x


def effective(g, clip, dtype):
    """ge as the reference of ``dtype`` sees it: float64 from the exact product, fp32 with the clip coefficient at fp32."""
    if dtype == torch.float64:
        return g.double() * GS * float(clip)
    return g.float() * GS * _f32(clip)


def _scalar(v, dtype):
    """A Python float or a per-element tensor, at its fp32 value, in ``dtype``."""
    if isinstance(v, torch.Tensor):
        return v.float().to(dtype)
    return torch.tensor(_f32(v), dtype=dtype)


def step_ref(p, m, ge, lr, wd, dtype, b1=B1, b2=B2):
    """One step of the formula in ``dtype``; ``lr`` / ``wd``: floats or per-element tensors.  Returns p_new, m_new, c and
    |beta1 * m| + |(1 - beta1) * ge| (the magnitude the tie band is relative to)."""
    p, m, ge = p.to(dtype), m.to(dtype), ge.to(dtype)
    lr, wd, b1, b2 = (_scalar(v, dtype) for v in (lr, wd, b1, b2))
    one = torch.tensor(1.0, dtype=dtype)
    t1, t2 = b1 * m, (one - b1) * ge
    c = t1 + t2
    p_new = p * (one - lr * wd) - lr * torch.sign(c)
    m_new = b2 * m + (one - b2) * ge
    return p_new, m_new, c, t1.abs() + t2.abs()


def near_tie(c64, mag64):
    return (c64.abs() <= BAND * mag64) & (mag64 > 0)


def check_step(name, got_p, got_m, p0, m0, g, clip, lr, wd, b1=B1, b2=B2, ge=None):
    """The element rule for one step from the state (p0, m0): asserts it and returns a dict of figures (elements in the band,
    worst error / allowed of p and m, sign disagreements of the fp32 reference outside the band).  ``ge``: a pair (float64,
    fp32) of effective gradients instead of ``g`` and ``clip``."""
    ge64, ge32 = ge if ge is not None else (effective(g, clip, torch.float64), effective(g, clip, torch.float32))
    p64, m64, c64, mag = step_ref(p0, m0, ge64, lr, wd, torch.float64, b1, b2)
    p32, m32, c32, _ = step_ref(p0, m0, ge32, lr, wd, torch.float32, b1, b2)
    band = near_tie(c64, mag)
    out = ~band
    flips = int((torch.sign(c32).double() != torch.sign(c64))[out].sum())
    got_p, got_m = got_p.detach().cpu().double(), got_m.detach().cpu().double()
    ref_m = R.Ref(m64, m32)
    rm = R._ratio((got_m - m64).abs(), ref_m.allowed_f32())
    ref_p = R.Ref(p64[out], p32[out])
    rp = R._ratio((got_p[out] - ref_p.r64).abs(), ref_p.allowed_f32())
    rb = 0.0
    if bool(band.any()):
        lr64, wd64 = _scalar(lr, torch.float64), _scalar(wd, torch.float64)
        lr_b = lr64[band] if lr64.ndim else lr64
        decayed = (p0.double() * (1.0 - lr64 * wd64))[band]
        err = torch.stack([(got_p[band] - cand).abs() / (R.REF_FACTOR * ref_p.e32 + R.ulp(cand, torch.float32))
                           for cand in (decayed - lr_b, decayed, decayed + lr_b)]).min(0).values
        rb = float(err.max())
    fig = {"band": int(band.sum()), "p": rp, "p_band": rb, "m": rm, "flips": flips, "e32_p": ref_p.e32, "e32_m": ref_m.e32}
    print(f"  {name}: band {fig['band']} of {band.numel()}, p ratio {rp:.3g} (in band {rb:.3g}), m ratio {rm:.3g}, "
          f"fp32 sign flips outside the band {flips}")
    assert rm <= 1.0, f"{name}: m error / allowed = {rm} (E32 = {ref_m.e32})"
    assert rp <= 1.0, f"{name}: p error / allowed = {rp} outside the tie band (E32 = {ref_p.e32})"
    assert rb <= 1.0, f"{name}: p of an element near a tie is none of its three legal values (error / allowed = {rb})"
    return fig
