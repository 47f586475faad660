"""Inputs, references and the rules of the Muon kernel tests (tests/test_gpu_muon.py) and of their CPU-side check
(tests/test_cpu_muon.py).  CPU only: importing this module needs neither a GPU nor the HIP library.

The update (torch.optim.Muon of the installed torch, torch/optim/_muon.py), per Muon tensor T of stored shape [r, c] in a group
with (lr, wd), for the effective gradient ge = g * grad_scale * clip:

    B = lerp(B, ge, 1 - mu);   U = lerp(ge, B, mu) if nesterov else B
    X = bf16(U), transposed if r > c;   X = X / max(||X||_F, eps)
    ns_steps times:  G = X X^T;  P = b G + c G G;  X = a X + P X
    O = X, transposed back;   p = p (1 - lr wd) - lr_adj O,   lr_adj = lr * ``adjust_ratio``

Every other tensor gets AdamW; its reference is ``ops.adamw_step_groups`` on the same inputs, bit for bit (the GPU tests).

The rule for O.  ``ns64`` -- the formula above in float64, started from the bf16 values of U -- is the truth; the yardstick is
``torch.optim.Muon`` on the CPU on the same input (``torch_step``).  With ``dev(O) = ||O - O_64||_F / ||O_64||_F`` a result
passes if ``dev(O) <= O_FACTOR * dev(O_torch)``; an all-zero input must give exactly 0.  Measured on a CPU at the shapes of
``MATRICES``: torch's own deviation is 1.2e-2 to 2.0e-2, ``ns_emulated`` (bf16 operands, fp32 accumulation, ONE rounding per
GEMM with the epilogue in fp32: what the kernels do) lands at 0.85 to 1.12 of it, and one element of a 64 x 64 result that is
off by 1 gives 10.5 (tests/test_cpu_muon.py holds all three).  Shapes with a dimension below 64 are not in the table: at [8, 8]
two correct bf16 implementations differ by 2.4 x.

O is recovered from the weights: ``O = (p0 (1 - lr wd) - p) / lr_adj`` in float64.  The weights are drawn at 0.02 and the
learning rates of ``STEPS`` are 1e-2 and above, so the fp32 rounding of p (2^-30 at |p| < 0.0625) and of the decay factor
(2^-24 |p|) put less than 1e-5 of a typical |O| = 1 / sqrt(max(r, c)) >= 0.07 into the recovered value: three orders below the
deviation the rule measures.

The momentum buffer B is held to the reference-relative rule of tests/_refbounds.py (torch's fp32 lerp against float64).

The matrix table holds the smallest shapes at which the kernels can go wrong: [64, 64]; [192, 64] (tall: the transposed
products, two row tiles); [64, 128] (wide); [72, 200] and [200, 72] (no dimension a multiple of a tile or of 64: edges in both
outer dimensions and a K tail in every product, wide and tall); [136, 136] (two tiles with an 8-wide edge); a class of three
[64, 128] at unequal offsets beside shapes that occur once.  AdamW tensors of 1, 64, 65 and 320 elements and a slot
of no tensor lie between them."""
import functools
import math

import torch

from tests import _refbounds as R

SLOT = 64
COEFFS = (3.4445, -4.7750, 2.0315)
NS_STEPS, EPS_MUON, MU = 5, 1e-7, 0.95
B1, B2, EPS_ADAM = 0.9, 0.999, 1e-8
GS = 0.5
O_FACTOR = 1.5
STEPS = [2e-2, 5e-2, 1e-2]                  # learning rate of the three chained steps (see the module docstring)
GROUP_USE_MUON = [True, True, False, False]
GROUP_LR = [1.0, 0.5, 1.0, 0.3]             # group learning rates as multiples of the step's
GROUP_WD = [0.1, 0.0, 0.05, 0.0]
KINDS = ("gauss", "half", "tiny", "zero")   # Gaussian; the upper half of the rows zero; Gaussian x 1e-6; all zero

# (name, shape, group); shape an int: an AdamW tensor of that many elements; name None: a slot of no tensor
ENTRIES = [("a1", 1, 2), ("sq", (64, 64), 0), ("a64", 64, 3), ("tall", (192, 64), 0), ("w0", (64, 128), 0), ("a65", 65, 2),
           ("odd", (72, 200), 1), ("w1", (64, 128), 0), (None, 64, 0), ("edge", (136, 136), 0), ("a320", 320, 3),
           ("w2", (64, 128), 1), ("oddtall", (200, 72), 0)]
MATRICES = [(n, s) for n, s, _ in ENTRIES if isinstance(s, tuple)]
HOLE_P, HOLE_M, HOLE_V = 777.0, 555.0, 333.0        # what a slot of no tensor holds, before and after


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def adjust_ratio(adjust_lr_fn, r, c):
    """lr_adj / lr of torch.optim._muon._adjust_lr."""
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(r, c))
    return math.sqrt(max(1, r / c))


class Table:
    """The layout of ``ENTRIES`` in a flat buffer of 64-float slots and the device tables of the kernels, as host tensors."""

    def __init__(self, entries=ENTRIES, adjust_lr_fn=None):
        self.names, self.offset, self.numel, self.group, self.shape = [], [], [], [], []
        off = 0
        holes = []
        for name, shape, group in entries:
            numel = shape[0] * shape[1] if isinstance(shape, tuple) else shape
            span = (max(numel, 1) + SLOT - 1) // SLOT * SLOT
            if name is None:
                holes.append((off, off + span))
            else:
                self.names.append(name)
                self.offset.append(off)
                self.numel.append(numel)
                self.group.append(group)
                self.shape.append(shape if isinstance(shape, tuple) else None)
            off += span
        self.n, self.holes = off, holes
        self.muon = [i for i, s in enumerate(self.shape) if s is not None]         # Muon tensor t is entry self.muon[t]
        self.adamw = [i for i, s in enumerate(self.shape) if s is None]
        self.slot_tensor = torch.full((off // SLOT,), -1, dtype=torch.int32)        # -1: AdamW
        for lo, hi in holes:
            self.slot_tensor[lo // SLOT:hi // SLOT] = -2                            # neither read nor written
        self.chunk_group = torch.zeros(off // SLOT, dtype=torch.uint8)
        self.owned = torch.zeros(off, dtype=torch.bool)
        self.info = torch.zeros((len(self.muon), 4), dtype=torch.int32)
        self.ratio = torch.ones(len(self.muon), dtype=torch.float32)
        x_slot = 0
        for i in range(len(self.names)):
            lo, hi = self.offset[i] // SLOT, (self.offset[i] + max(self.numel[i], 1) + SLOT - 1) // SLOT
            self.chunk_group[lo:hi] = self.group[i]
            self.owned[self.offset[i]:self.offset[i] + self.numel[i]] = True
            if self.shape[i] is not None:
                t = self.muon.index(i)
                self.slot_tensor[lo:hi] = t
                self.info[t, 0], self.info[t, 1], self.info[t, 2] = lo, hi, x_slot
                self.ratio[t] = adjust_ratio(adjust_lr_fn, *self.shape[i])
                x_slot += hi - lo
        self.compact_slots = x_slot
        self.classes = {}                    # (r, c) -> Muon tensor indices
        for t, i in enumerate(self.muon):
            self.classes.setdefault(self.shape[i], []).append(t)

    def index(self, name):
        return self.names.index(name)

    def elements(self, i):
        return slice(self.offset[i], self.offset[i] + self.numel[i])

    def compact(self, t):
        """Elements of Muon tensor t in the compact bf16 buffers."""
        lo = int(self.info[t, 2]) * SLOT
        return slice(lo, lo + self.numel[self.muon[t]])

    def class_offsets(self, shape):
        return torch.tensor([int(self.info[t, 2]) * SLOT for t in self.classes[shape]], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def table(adjust_lr_fn=None):
    return Table(ENTRIES, adjust_lr_fn)


def matrix_input(kind, r, c, seed):
    g = torch.Generator().manual_seed(7919 * r + 31 * c + seed)
    x = torch.randn(r, c, generator=g)
    if kind == "half":
        x[: r // 2] = 0.0
    elif kind == "tiny":
        x = x * 1e-6
    elif kind == "zero":
        x = torch.zeros(r, c)
    else:
        assert kind == "gauss", kind
    return x


@functools.lru_cache(maxsize=None)
def grad(kind, step):
    """The flat gradient of chained step ``step`` (0-based): every matrix of ``kind``, AdamW tensors Gaussian, padding zero."""
    tb = table()
    g = torch.Generator().manual_seed(1000 * tb.n + step)
    x = 0.1 * torch.randn(tb.n, generator=g)
    x[~tb.owned] = 0.0
    for i in tb.muon:
        x[tb.elements(i)] = matrix_input(kind, *tb.shape[i], seed=step).reshape(-1)
    for lo, hi in tb.holes:
        x[lo:hi] = 1.0          # never read
    return x


@functools.lru_cache(maxsize=None)
def start(zero_p=False):
    """p, m, v before the first step: weights at 0.02, moments not zero (both terms of each are live from the first step on)."""
    tb = table()
    g = torch.Generator().manual_seed(13 * tb.n + 1)
    p = 0.02 * torch.randn(tb.n, generator=g)
    m = 0.05 * torch.randn(tb.n, generator=g)
    v = (0.05 * torch.randn(tb.n, generator=g)) ** 2
    if zero_p:
        p, m, v = torch.zeros(tb.n), torch.zeros(tb.n), torch.zeros(tb.n)
    for t in (p, m, v):
        t[~tb.owned] = 0.0
    for lo, hi in tb.holes:
        p[lo:hi], m[lo:hi], v[lo:hi] = HOLE_P, HOLE_M, HOLE_V
    return p, m, v


def effective(g, clip, dtype, gs=GS):
    """ge = g * grad_scale * clip as a reference of ``dtype`` sees it (the kernel forms gs = grad_scale * clip in fp32 first)."""
    gs = torch.tensor(_f32(gs), dtype=torch.float32) * torch.tensor(_f32(clip), dtype=torch.float32)
    return g.to(dtype) * gs.to(dtype)


# ------------------------------------------------------------------------------------------------------------ Newton-Schulz
def ns64(u, coeffs=COEFFS, steps=NS_STEPS, eps=EPS_MUON):
    """The truth: the formula in float64 on the bf16 values of ``u`` ([r, c], any float dtype); returns O [r, c] float64."""
    a, b, c = coeffs
    x = u.to(torch.bfloat16).double()
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    x = x / x.norm().clamp(min=eps)
    for _ in range(steps):
        g = x @ x.T
        p = b * g + c * (g @ g)
        x = a * x + p @ x
    return (x.T if tall else x).contiguous()


def ns_emulated(u, coeffs=COEFFS, steps=NS_STEPS, eps=EPS_MUON):
    """What the kernels do, on the CPU: bf16 operands, fp32 accumulation, one rounding to bf16 per GEMM with the epilogue
    (beta Cin + alpha acc) in fp32; the norm in float64 from the bf16 values."""
    a, b, c = (_f32(x) for x in coeffs)
    x = u.to(torch.bfloat16)
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    den = max(float(x.double().norm()), eps)
    x = (x.float() / _f32(den)).to(torch.bfloat16)
    for _ in range(steps):
        g = (x.float() @ x.float().T).to(torch.bfloat16)
        p = (b * g.float() + c * (g.float() @ g.float())).to(torch.bfloat16)
        x = (a * x.float() + p.float() @ x.float()).to(torch.bfloat16)
    return (x.T if tall else x).contiguous()


def torch_step(p, buf, ge, lr, wd, momentum, nesterov, adjust_lr_fn, coeffs=COEFFS, steps=NS_STEPS, eps=EPS_MUON):
    """One step of torch.optim.Muon on the CPU for ONE matrix (fp32 tensors [r, c]); returns p_new, buf_new."""
    q = torch.nn.Parameter(p.clone().float())
    opt = torch.optim.Muon([q], lr=lr, weight_decay=wd, momentum=momentum, nesterov=nesterov, ns_coefficients=coeffs, eps=eps,
                           ns_steps=steps, adjust_lr_fn=adjust_lr_fn)
    opt.state[q]["momentum_buffer"] = buf.clone().float()
    q.grad = ge.clone().float()
    opt.step()
    return q.detach().clone(), opt.state[q]["momentum_buffer"].clone()


def torch_o(u, adjust_lr_fn=None):
    """O of torch.optim.Muon on the update ``u``: with p = 0, lr = 1, wd = 0, momentum = 0 its step gives -lr_adj O."""
    r, c = u.shape
    p, _ = torch_step(torch.zeros(r, c), torch.zeros(r, c), u.float(), 1.0, 0.0, 0.0, True, adjust_lr_fn)
    return -p.double() / adjust_ratio(adjust_lr_fn, r, c)


def update_of(buf, ge, momentum, nesterov, dtype):
    """(B_new, U) through torch's lerp in ``dtype``, as _single_tensor_muon forms them."""
    buf = buf.to(dtype).clone()
    ge = ge.to(dtype)
    buf.lerp_(ge, 1 - momentum)
    return buf, (ge.lerp(buf, momentum) if nesterov else buf)


def deviation(o, o64):
    d = float(o64.norm())
    return float((o.double() - o64).norm()) / d if d > 0.0 else float(o.double().norm())


def check_o(name, o, o_torch, o64):
    """The rule for O; prints the figures first; returns (dev, dev of torch)."""
    dk, dt = deviation(o, o64), deviation(o_torch, o64)
    print(f"  {name}: dev {dk:.4g}, torch {dt:.4g}, ratio {dk / dt if dt > 0 else float('nan'):.3g}")
    assert not bool(torch.isnan(o.double()).any()), f"{name}: NaN in O"
    if float(o64.abs().max()) == 0.0:
        assert float(o.double().abs().max()) == 0.0, f"{name}: O of an all-zero update is not exactly 0"
    else:
        assert dk <= O_FACTOR * dt, f"{name}: ||O - O_64|| / ||O_64|| = {dk}, torch's own is {dt} (allowed {O_FACTOR} x)"
    return dk, dt


def recover_o(p0, p, lr, wd, lr_adj):
    """O from the weights before and after, float64; lr, wd at the fp32 values the kernel reads."""
    return (p0.double() * (1.0 - _f32(lr) * _f32(wd)) - p.double()) / lr_adj


def check_b(name, got, buf, ge64, ge32, momentum):
    """The momentum buffer against float64 under the reference-relative rule (torch's fp32 lerp is the fp32 reference)."""
    b64, _ = update_of(buf, ge64, momentum, False, torch.float64)
    b32, _ = update_of(buf, ge32, momentum, False, torch.float32)
    return R.check_f32(name, got, R.Ref(b64, b32))
