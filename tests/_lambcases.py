"""Inputs, float64 / fp32 references and the element rule of the LAMB kernel tests (tests/test_gpu_lamb.py) and of their
CPU-side check (tests/test_cpu_lamb.py).  CPU only: importing this module needs neither a GPU nor the HIP library.

The update (timm.optim.Lamb with its defaults), per tensor T of a group with (lr, wd), step t (1-based), for the effective
gradient ge = g * grad_scale * clip:

    m = b1 m + (1 - b1) ge;   v = b2 v + (1 - b2) ge^2
    u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p         (the wd term only when wd != 0)
    r = 1 if wd == 0 and not always_adapt, else ||p|| / ||u|| over T if both norms > 0, else 1;  min(r, 1) under trust_clip
    p = p - lr r u

``step_ref`` is that formula through torch in float64 or fp32, scalars at the fp32 values the kernel receives.  Three chained
steps with a changing learning rate (``STEPS``, t = 1, 2, 3); every reference step starts from the state the code under test
left.  The rule is the reference-relative one of tests/_refbounds.py: every element of p, m, v within
``REF_FACTOR * E32 + ulp_fp32``, the bf16 mirror within ``ulp_bf16 + REF_FACTOR * E32`` under ``SHARE_CAP``.

The trust ratio itself is held to ``TRUST_REL`` of the float64 value.  The kernels sum 64 non-negative fp32 squares per slot in
a tree of depth 6 after one rounding of each square (relative <= 7u on a sum of squares, 3.5u on its root; the fp64 sum over
slots adds nothing), every u carries at most about 4u of its own (two divisions, a root, an addition, one fma), the ratio adds
both norms' errors and the cast to fp32 half a u: 3.5 + 3.5 + 4 + 0.5 = 11.5u, held at 16u = 2^-20.  Where the rule gives r = 1
(no decay, a zero norm) the kernel must give exactly 1.

The tensor table holds the smallest shapes at which the kernels can go wrong: 1 element in a 64-slot; exactly 64; 65 (two
slots, 63 floats of padding); 320; a slot that belongs to no tensor (never read or written); a tensor without weight decay
(r = 1; adapted under always_adapt); p = 0 under a gradient (||p|| = 0); p != 0 with g = m = v = 0 and no decay (||u|| = 0
under always_adapt); a tensor whose r exceeds 1 (trust_clip); and, in the full table, a tensor across the end of the first trip
of the capped grid."""
import functools

import torch

from tests import _lioncases as L
from tests import _refbounds as R

SLOT = 64
B1, B2, EPS, WD, GS = 0.9, 0.999, 1e-6, 0.1, 0.5
STEPS = [1e-3, 3e-3, 1e-7]              # learning rate of the three chained steps (the last: a warm-up value)
GRID_CAP_N = L.GRID_CAP_N               # floats one pass of the capped grid covers (the same 4096 x 256 x 4 as Lion)
GROUP_WD = [WD, 0.0]                    # group 0 decays, group 1 does not
GROUP_LR = [1.0, 0.5]                   # ... and trains at half the learning rate
TRUST_REL = 2.0 ** -20

# (name, elements, group); name None: a slot of no tensor
SMALL = [("one", 1, 0), ("slot", 64, 0), ("two", 65, 0), ("five", 320, 0), (None, 64, 0), ("nodecay", 320, 1), ("zero_p", 128, 0),
         ("still", 64, 1), ("big_r", 64, 0), ("tail", 100, 0)]
FULL = SMALL[:-1] + [("large", GRID_CAP_N + 320, 0), ("tail", 100, 0)]


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


class Table:
    """The layout of a tensor list in a flat buffer of 64-float slots, and the device tables of the kernels as host tensors."""

    def __init__(self, entries):
        items, off = [], 0
        for name, numel, group in entries:
            if name is not None:
                items.append((name, off, numel, group))
            off += (max(numel, 1) + SLOT - 1) // SLOT * SLOT
        self._lay_out(off, items)

    @classmethod
    def from_layout(cls, n, items):
        """A table over a buffer that exists: ``items`` = (name, offset, elements, group) of its tensors, ``n`` its floats;
        every slot of no tensor (padding behind the last one, a locked parameter) is a hole."""
        tb = cls.__new__(cls)
        tb._lay_out(n, list(items))
        return tb

    def _lay_out(self, n, items):
        self.n, self.n_tensors = n, len(items)
        self.names, self.offset, self.numel, self.group = (list(x) for x in zip(*items))
        self.slot_tensor = torch.full((n // SLOT,), -1, dtype=torch.int32)
        self.tensor_slots = torch.zeros((self.n_tensors, 2), dtype=torch.int32)
        self.owned = torch.zeros(n, dtype=torch.bool)          # the elements of tensors (their slot padding is not)
        for ti in range(self.n_tensors):
            lo, hi = self.offset[ti] // SLOT, (self.offset[ti] + max(self.numel[ti], 1) + SLOT - 1) // SLOT
            self.slot_tensor[lo:hi] = ti
            self.tensor_slots[ti, 0], self.tensor_slots[ti, 1] = lo, hi
            self.owned[self.offset[ti]:self.offset[ti] + self.numel[ti]] = True
        self.tensor_group = torch.tensor(self.group, dtype=torch.int32)
        free = (self.slot_tensor < 0).tolist()
        self.holes, k = [], 0
        while k < len(free):        # maximal runs of slots that belong to no tensor
            if not free[k]:
                k += 1
                continue
            j = k
            while j < len(free) and free[j]:
                j += 1
            self.holes.append((k * SLOT, j * SLOT))
            k = j

    def index(self, name):
        return self.names.index(name)

    def elements(self, ti):
        return slice(self.offset[ti], self.offset[ti] + self.numel[ti])

    def slots(self, ti):
        """The tensor's whole slots: its elements and the zero padding of its last slot."""
        return slice(int(self.tensor_slots[ti, 0]) * SLOT, int(self.tensor_slots[ti, 1]) * SLOT)


@functools.lru_cache(maxsize=None)
def table(which):
    return Table({"small": SMALL, "full": FULL}[which])


HOLE_P, HOLE_M, HOLE_V = 777.0, 555.0, 333.0        # what a slot of no tensor holds, before and after


@functools.lru_cache(maxsize=None)
def start(which):
    """p, m, v before the first step (the moments are not zero: both terms of each are live from the first step on)."""
    tb = table(which)
    g = torch.Generator().manual_seed(13 * tb.n + 1)
    p = torch.randn(tb.n, generator=g)
    m = 0.05 * torch.randn(tb.n, generator=g)
    v = (0.05 * torch.randn(tb.n, generator=g)) ** 2
    for t in (p, m, v):
        t[~tb.owned] = 0.0
    p[tb.elements(tb.index("zero_p"))] = 0.0
    p[tb.elements(tb.index("big_r"))] *= 100.0
    for t in (m, v):
        t[tb.elements(tb.index("still"))] = 0.0
    for lo, hi in tb.holes:
        p[lo:hi], m[lo:hi], v[lo:hi] = HOLE_P, HOLE_M, HOLE_V
    return p, m, v


@functools.lru_cache(maxsize=None)
def grad(which, step):
    """Gradient of chained step ``step`` (0-based); zero on the padding and on the tensor that stands still."""
    tb = table(which)
    g = torch.Generator().manual_seed(1000 * tb.n + step)
    x = 0.1 * torch.randn(tb.n, generator=g)
    x[~tb.owned] = 0.0
    x[tb.elements(tb.index("still"))] = 0.0
    for lo, hi in tb.holes:
        x[lo:hi] = 1.0          # never read
    return x


effective = L.effective         # ge of a gradient under GS and a clip coefficient, as the reference of a dtype sees it


def bias_corrections(t, b1=B1, b2=B2):
    """1 - b1^t and sqrt(1 - b2^t) in fp32, as the library's host function forms them: ``powf`` is the correctly rounded power
    (taken here through float64), not a chain of fp32 products -- at b2 = 0.999, t = 3 the two differ in the last bit of b2^t and
    so by 2e-5 of 1 - b2^t.  tests/test_gpu_lamb.py holds these to the bits of the host function for the steps the tests run."""
    one = torch.tensor(1.0, dtype=torch.float32)
    bc1 = one - (torch.tensor(b1, dtype=torch.float32).double() ** t).float()
    bc2s = torch.sqrt(one - (torch.tensor(b2, dtype=torch.float32).double() ** t).float())
    return bc1, bc2s


def _norm(x, dtype, slot_order):
    """||x||: torch's norm in ``dtype``, or -- ``slot_order`` -- the kernels' order: fp32 sums of squares per 64-float slot,
    the slots summed in float64."""
    if not slot_order:
        return torch.linalg.vector_norm(x).double()
    sq = (x.float() * x.float()).view(-1, SLOT)
    while sq.shape[1] > 1:
        sq = sq[:, 0::2] + sq[:, 1::2]
    return sq.double().sum().sqrt()


def step_ref(tb, p, m, v, ge, lr, t, dtype, lr_of=None, wd_of=None, b1=B1, b2=B2, eps=EPS, always_adapt=False, trust_clip=False,
             slot_order=False):
    """One step of the formula in ``dtype`` over the tensors of ``tb``; ``lr_of`` / ``wd_of``: per-tensor lists (default: the
    table's groups under ``lr``).  Returns p_new, m_new, v_new and r (float64, one per tensor).  Slots of no tensor keep their
    values."""
    lr_of = [lr * GROUP_LR[g] for g in tb.group] if lr_of is None else lr_of
    wd_of = [GROUP_WD[g] for g in tb.group] if wd_of is None else wd_of
    p, m, v, ge = p.to(dtype), m.to(dtype), v.to(dtype), ge.to(dtype)
    sc = lambda x: torch.tensor(_f32(x), dtype=dtype)       # noqa: E731
    b1, b2, eps = sc(b1), sc(b2), sc(eps)
    bc1, bc2s = (x.to(dtype) for x in bias_corrections(t, float(b1), float(b2)))
    one = torch.tensor(1.0, dtype=dtype)
    m_new = b1 * m + (one - b1) * ge
    v_new = b2 * v + (one - b2) * ge * ge
    p_new = p.clone()
    r_out = torch.ones(tb.n_tensors, dtype=torch.float64)
    for ti in range(tb.n_tensors):
        s = tb.slots(ti)
        wd, lr_t = sc(wd_of[ti]), sc(lr_of[ti])
        u = (m_new[s] / bc1) / (v_new[s].sqrt() / bc2s + eps)
        if float(wd) != 0.0:
            u = u + wd * p[s]
        r = torch.tensor(1.0, dtype=torch.float64)
        if float(wd) != 0.0 or always_adapt:
            pn, un = _norm(p[s], dtype, slot_order), _norm(u, dtype, slot_order)
            if float(pn) > 0.0 and float(un) > 0.0:
                r = pn / un
        if trust_clip:
            r = r.clamp(max=1.0)
        r_out[ti] = r
        p_new[s] = p[s] - (lr_t * r.to(dtype)) * u
    for lo, hi in tb.holes:
        m_new[lo:hi], v_new[lo:hi] = m[lo:hi], v[lo:hi]
    return p_new, m_new, v_new, r_out


def check_trust(name, tb, got_r, r64, wd_of=None, always_adapt=False):
    got_r = got_r.detach().cpu().double()
    wd_of = [GROUP_WD[g] for g in tb.group] if wd_of is None else wd_of
    rel = float(((got_r - r64).abs() / r64).max())
    print(f"  {name}: trust ratios {[f'{x:.4g}' for x in got_r.tolist()]}, worst relative error {rel:.3g}")
    assert rel <= TRUST_REL, f"{name}: a trust ratio is {rel} (relative) off its float64 value (allowed {TRUST_REL})"
    for ti in range(tb.n_tensors):
        if float(r64[ti]) == 1.0:
            assert float(got_r[ti]) == 1.0, f"{name}: tensor {tb.names[ti]}: r = {float(got_r[ti])}, the rule gives exactly 1"
        if wd_of[ti] == 0.0 and not always_adapt:
            assert float(got_r[ti]) == 1.0, f"{name}: tensor {tb.names[ti]} has no decay: r = {float(got_r[ti])}"
    return rel


def check_step(name, tb, got, before, ge, lr, t, mirror=None, got_r=None, per_tensor=False, **kw):
    """The element rule for one step from the state ``before`` = (p0, m0, v0): asserts it for ``got`` = (p, m, v) over the
    elements of the table's tensors (``per_tensor``: tensor by tensor, each with the E32 of its own elements), for the bf16
    ``mirror`` and for the trust ratios ``got_r``; returns the float64 trust ratios.  ``ge``: the pair (float64, fp32) of
    effective gradients."""
    ref64 = step_ref(tb, *before, ge[0], lr, t, torch.float64, **kw)
    ref32 = step_ref(tb, *before, ge[1], lr, t, torch.float32, **kw)
    got = [x.detach().cpu() for x in got]
    parts = [(tb.names[ti], tb.elements(ti)) for ti in range(tb.n_tensors)] if per_tensor else [("all", tb.owned)]
    for part, sel in parts:
        for what, x, r64, r32 in zip("pmv", got, ref64, ref32):
            ref = R.Ref(r64[sel], r32[sel])
            R.check_f32(f"{name} {part} {what}", x[sel], ref)
            if what == "p" and mirror is not None:
                R.check_bf16(f"{name} {part} mirror", mirror.detach().cpu()[sel], ref)
    if got_r is not None:
        check_trust(name, tb, got_r, ref64[3], kw.get("wd_of"), kw.get("always_adapt", False))
    return ref64[3]
