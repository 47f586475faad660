"""Float64 references, their inputs and the error bounds of the row / reduction / optimiser kernel tests
(tests/test_gpu_norm_sweep.py, tests/test_gpu_optim_kernels.py) and of their CPU-side check
(tests/test_cpu_reference_bounds.py).  CPU only: importing this module needs neither a GPU nor the HIP library.

Every reference is PyTorch in float64 on the CPU, run on exactly the values the kernel received (bf16 and fp32 inputs are
widened exactly; scalar arguments are taken at the fp32 value the kernel sees).  Three kinds of bound:

* Reference-relative (fp32 outputs: LayerNorm mean / rstd / fp32 gradient, L2-norm, AdamW): the same operation through
  PyTorch in fp32 on the CPU, on the same inputs, has a maximum error E32 against float64 over the output tensor.  Every
  element of the kernel's output must lie within ``REF_FACTOR * E32 + ulp_fp32(|float64 value|)``.  The factor 4 allows for
  reduction orders (wave shuffles against sequential or pairwise sums) and rsqrtf, which differ from the CPU but are not bugs.
* bf16 outputs: within ``ulp_bf16(|float64 value|) + REF_FACTOR * E32`` (E32 of the fp32 value the bf16 copy rounds: the
  allowance near a cancellation), and at most ``SHARE_CAP`` of the elements of a tensor may differ from bf16(float64 value).
  On a CPU, PyTorch's fp32 LayerNorm differs from bf16(float64) on 2.5e-5 - 3.6e-5 of the elements: a 30x margin.
  tests/test_cpu_reference_bounds.py asserts that the fp32 CPU reference itself meets every cap on the exact inputs of the
  GPU tests.
* Derived (column sums, grad norm): from the kernel's own arithmetic, see ``ln_colsum_chain`` / ``colsum_chain`` and
  ``GRAD_NORM_REL``.
"""
import math

import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
REF_FACTOR = 4.0
SHARE_CAP = 1e-3
EPS_LN = float(torch.tensor(1e-5, dtype=torch.float32))      # the fp32 eps the LayerNorm kernels receive

# Grad norm (sumsq_partial_kernel + sumsq_final_kernel, spatial-clip_amd/csrc/sc_optim.hip:11-52): each float4 is squared and
# summed in fp32 in pairs (v0*v0 + v1*v1: two roundings, relative <= 2u each pair), the pairs and all further sums are fp64
# (relative 2^-53 per addition: negligible at n <= 5e7), then one sqrt in fp64, one cast to fp32 (u) and one multiply by
# grad_scale (u; exact for powers of two).  Relative error <= about 4u = 2.4e-7; 1e-6 is a 4x margin for sqrt / cast details
# and still ~60x tighter than PyTorch's own fp32 norm (6.4e-5 off at n = 3.5 M on a CPU).
GRAD_NORM_REL = 1e-6
# Clip coefficient min(1, max_norm / (norm + 1e-6)) in fp32 from that norm: the norm's relative error plus the roundings of
# the addition and the division (and of 1e-6 itself, far below them): GRAD_NORM_REL + 3u.
CLIP_REL = GRAD_NORM_REL + 3 * U32


# ---------------------------------------------------------------------------------------------------------- element rules
def ulp(x64: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` (fp32: 24 significant bits, bf16: 8) at |x| for a float64 tensor; at zero, the spacing at the
    smallest normal of ``dtype``."""
    bits = {torch.float32: 24, torch.bfloat16: 8}[dtype]
    a = x64.double().abs().clamp_min(torch.finfo(dtype).tiny)
    # biased float64 exponent E: a in the binade [2^(E-1023), 2^(E-1022)), whose dtype spacing is 2^(E-1022-bits) = the
    # float64 with biased exponent E + 1 - bits and a zero mantissa (bit arithmetic: a tenth of the time of frexp + pow)
    e = a.view(torch.int64) >> 52
    return ((e + 1 - bits) << 52).view(torch.float64)


def max_err(ref32: torch.Tensor, ref64: torch.Tensor) -> float:
    """E32: the largest |fp32 reference - float64 reference| over a tensor."""
    return float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0


def bf16_share(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """Share of the elements of a bf16 tensor that differ from bf16(float64 value)."""
    if ref64.numel() == 0:
        return 0.0
    want = ref64.to(torch.float32).to(torch.bfloat16)       # (double -> float is exact to far below a bf16 ulp)
    return float((got.cpu().to(torch.bfloat16).view(torch.int16) != want.view(torch.int16)).double().mean())


def _ratio(err: torch.Tensor, allowed: torch.Tensor) -> float:
    if err.numel() == 0:
        return 0.0
    r = err / allowed
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


class Ref:
    """A float64 reference with the fp32 reference's error E32; the allowances of both element rules are formed once."""

    def __init__(self, ref64: torch.Tensor, ref32: torch.Tensor):
        self.r64 = ref64.double()
        self.e32 = max_err(ref32, self.r64)
        self._a32 = self._a16 = self._w16 = None

    def allowed_f32(self) -> torch.Tensor:
        if self._a32 is None:
            self._a32 = REF_FACTOR * self.e32 + ulp(self.r64, torch.float32)
        return self._a32

    def allowed_bf16(self) -> torch.Tensor:
        if self._a16 is None:
            self._a16 = ulp(self.r64, torch.bfloat16) + REF_FACTOR * self.e32
        return self._a16

    def want_bf16(self) -> torch.Tensor:
        if self._w16 is None:
            self._w16 = self.r64.to(torch.float32).to(torch.bfloat16)    # (double -> float: exact far below a bf16 ulp)
        return self._w16


def check_f32(name: str, got: torch.Tensor, ref: Ref) -> float:
    """Reference-relative rule for an fp32 output; prints and returns the ratio (kernel error / allowed error)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.r64.shape, (name, got.shape, ref.r64.shape)
    ratio = _ratio((got - ref.r64).abs(), ref.allowed_f32())
    print(f"  {name}: ratio {ratio:.3g} (E32 {ref.e32:.3g})")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio} (E32 = {ref.e32})"
    return ratio


def check_bf16(name: str, got: torch.Tensor, ref: Ref) -> float:
    """bf16 rule: one bf16 ulp of the float64 value plus 4x the fp32 reference's error, and the share cap."""
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == ref.r64.shape, (name, got.dtype, got.shape, ref.r64.shape)
    ratio = _ratio((got.double() - ref.r64).abs(), ref.allowed_bf16())
    share = float((got.view(torch.int16) != ref.want_bf16().view(torch.int16)).double().mean()) if got.numel() else 0.0
    print(f"  {name}: ratio {ratio:.3g}, bf16 share {share:.3g} (E32 {ref.e32:.3g})")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio} (E32 = {ref.e32})"
    assert share <= SHARE_CAP, f"{name}: {share} of the elements differ from bf16(float64 value) (cap {SHARE_CAP})"
    return ratio


def check_sum(name: str, got: torch.Tensor, ref64: torch.Tensor, abs_sum: torch.Tensor, k: int) -> float:
    """Derived rule for a column sum: |err_c| <= k * u * sum_r |term_rc|, k the longest fp32 rounding chain of the kernel's
    summation order (each partial sum is at most sum_r |term_rc|, and each addition rounds it by at most u)."""
    got = got.detach().cpu().double()
    allowed = k * U32 * abs_sum.double()
    err = (got - ref64.double()).abs()
    ratio = _ratio(err, allowed.clamp_min(torch.finfo(torch.float64).tiny))
    print(f"  {name}: ratio {ratio:.3g} (k = {k})")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio} (k = {k})"
    return ratio


# ---------------------------------------------------------------------------------------------------------- summation chains
def colvec_chain(nblk: int) -> int:
    """colvec_finalize_kernel (sc_norm.hip:391-420): per column, 16 row groups (ty) each add their slots b = ty, ty + 16, ...
    round robin into 8 accumulators (:403-407, <= ceil(ceil(nblk / 16) / 8) additions each), a 3-level tree joins the 8
    (:408), and thread 0 adds the 16 group sums one after another (:413-415)."""
    return math.ceil(math.ceil(nblk / 16) / 8) + 3 + 16


def ln_nominal_blocks(rows: int, d: int) -> int:
    """ln_nominal_blocks (sc_norm.hip:718-722): partial-sum slots of a LayerNorm backward launch."""
    return min((rows + 3) // 4, 1280 if d <= 768 else 1024)


def ln_colsum_chain(rows: int, d: int, n_cu: int) -> int:
    """Longest fp32 addition chain of dgamma / dbeta / colsum in the LayerNorm backward (ln_bwd_kernel + colvec_finalize).
    Each wave adds its rows in turn (sc_norm.hip:167, row_ += 4 * gridDim.x; the sums at :202-203, :229, :293-294, :316):
    with the grid capped at the resident blocks (ln_resident_blocks, :733-752: at least one block per CU, never more than
    the nominal count) a wave takes at most ceil(rows / (4 * min(nominal, CUs))) rows; wave 0 then adds waves 1..3 in
    order (:370-374: 3); the zero-filled slots (:383-386) add exact zeros; colvec_finalize over the nominal slots
    (:820, :888)."""
    nominal = ln_nominal_blocks(rows, d)
    per_wave = math.ceil(rows / (4 * min(nominal, n_cu)))
    return per_wave + 3 + colvec_chain(nominal)


def colsum_slices(rows: int) -> int:
    """sc_colsum_bf16 (sc_norm.hip:902-903): row slices (grid.y) = ceil(rows / 64), capped at 256."""
    return max(1, min((rows + 63) // 64, 256))


def colsum_chain(rows: int) -> int:
    """colsum_kernel + colvec_finalize: a thread adds rows r = 4 * slice + lane, stepping 4 * slices (sc_norm.hip:431,
    ceil(rows / (4 * slices)) additions), the 4 row lanes are joined in order (:436: 3), then colvec_finalize over the
    slices (:908)."""
    ny = colsum_slices(rows)
    return math.ceil(rows / (4 * ny)) + 3 + colvec_chain(ny)


# ---------------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = [4, 64, 192, 320, 384, 640, 768, 1024, 1280, 1408, 1664, 2048]
# rows: one row, fewer rows than a block's four waves, 257; above the nominal-slot count in both cap classes
# (1280 slots for d <= 768: 6304 rows = 1576 blocks; 1024 slots above: 5140 rows = 1285 blocks)
LN_CASES = [(r, d) for d in LN_WIDTHS for r in (1, 3, 257)] + [(6304, 768), (5140, 1280)]
LN_SPARSE_P = 5


def ln_nv(d: int) -> int:
    """float4 slots per lane of the kernel instance that serves width d (ln_fwd_launch / ln_bwd_launch)."""
    nvv = (d // 4 + 63) // 64
    return nvv if nvv <= 4 else 8


def ln_case_id(rows: int, d: int) -> str:
    slots = d / 256
    tags = [f"d{d}", f"r{rows}", f"NV{ln_nv(d)}", f"{slots:g}slots"]
    tags.append("cap1280" if d <= 768 else "cap1024")
    if 36 * d > 48 * 1024:
        tags.append("lds>48K")
    if (rows + 3) // 4 > ln_nominal_blocks(rows, d):
        tags.append("over-nominal")
    return "-".join(tags)


def ln_inputs(rows: int, d: int):
    """x (fp32 holding bf16 values: the fp32-row and the bf16-row kernels get the same input), gamma, beta (fp32), dy
    (bf16), gin (bf16: the incoming residual gradient; the fp32-buffer forms start from float(gin)).  Below 1000 elements
    the share cap allows no element off bf16(float64 value) at all; tests/test_cpu_reference_bounds.py checks that the fp32
    reference meets it on exactly these seeds (a seed that puts an element on a bf16 rounding boundary is caught there)."""
    g = torch.Generator().manual_seed(1000003 * d + 17 * rows + 1)
    scale = torch.logspace(-1, 1, rows).view(-1, 1) if rows > 1 else torch.ones(1, 1)
    x = ((torch.randn(rows, d, generator=g) + 0.3 * torch.randn(rows, 1, generator=g)) * scale).bfloat16().float()
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g).bfloat16()
    gin = torch.randn(rows, d, generator=g).bfloat16()
    return x, gamma, beta, dy, gin


def ln_fwd_refs(x, gamma, beta):
    """{name: (float64 reference, fp32 reference)} for y, mean, rstd."""
    d = x.shape[1]
    y64, m64, r64 = torch.native_layer_norm(x.double(), [d], gamma.double(), beta.double(), EPS_LN)
    y32, m32, r32 = torch.native_layer_norm(x.float(), [d], gamma.float(), beta.float(), EPS_LN)
    return {"y": (y64, y32), "mean": (m64.view(-1), m32.view(-1)), "rstd": (r64.view(-1), r32.view(-1))}


def ln_incoming(gin, mode):
    """Incoming residual gradient as float32 rows for accumulate = mode (False: none, True: every row, -P: rows r % P == 0)."""
    if mode is False or mode == 0:
        return torch.zeros(gin.shape, dtype=torch.float32)
    if mode is True:
        return gin.float()
    inc = torch.zeros(gin.shape, dtype=torch.float32)
    inc[::-mode] = gin.float()[::-mode]
    return inc


def ln_bwd_refs(dy, x, mean, rstd, gamma, beta):
    """Backward references on the kernel's own mean / rstd (the values the backward kernel receives): the LayerNorm input
    gradient (float64, fp32 reference), dgamma / dbeta (float64) and their sums of |term| (dy * x_hat, dy)."""
    d = x.shape[1]
    m, r = mean.reshape(-1, 1), rstd.reshape(-1, 1)
    dx64, dg64, db64 = torch.ops.aten.native_layer_norm_backward(dy.double(), x.double(), [d], m.double(), r.double(),
                                                                 gamma.double(), beta.double(), [True, True, True])
    dx32, _, _ = torch.ops.aten.native_layer_norm_backward(dy.float(), x.float(), [d], m.float(), r.float(), gamma.float(),
                                                           beta.float(), [True, False, False])
    xh64 = (x.double() - m.double()) * r.double()
    return {"dx": (dx64, dx32), "dgamma": dg64, "dbeta": db64,
            "dgamma_abs": (dy.double() * xh64).abs().sum(0), "dbeta_abs": dy.double().abs().sum(0)}


def ln_dres_ref(bwd, gin, mode):
    """(float64, fp32 reference) of the new residual gradient for accumulate = mode: incoming gradient + LayerNorm gradient."""
    dx64, dx32 = bwd["dx"]
    inc = ln_incoming(gin, mode)
    return inc.double() + dx64, inc + dx32


# ---------------------------------------------------------------------------------------------------------- L2 norm
L2_WIDTHS = [64, 100, 512, 768, 1024, 1280]
L2_CASES = [(r, d) for d in L2_WIDTHS for r in (1, 3, 4097)]


def l2_inputs(rows: int, d: int):
    """x (one all-zero row when rows > 1: row rows // 2), dy."""
    g = torch.Generator().manual_seed(104729 + 31 * d + rows)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-2, 2, rows).view(-1, 1)
    zero = rows // 2 if rows > 1 else None
    if zero is not None:
        x[zero] = 0.0
    dy = torch.randn(rows, d, generator=g)
    return x, dy, zero


def l2_refs(x, dy):
    """{name: (float64, fp32 reference)} for y = F.normalize(x), inv = 1 / max(|x|, 1e-12) and dx (autograd of F.normalize)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        xx = x.to(dt).clone().requires_grad_(True)
        y = torch.nn.functional.normalize(xx, dim=-1, eps=1e-12)
        y.backward(dy.to(dt))
        inv = 1.0 / torch.linalg.vector_norm(x.to(dt), dim=-1).clamp_min(1e-12)
        out[dt] = (y.detach(), inv, xx.grad)
    return {k: (out[torch.float64][i], out[torch.float32][i]) for i, k in enumerate(("y", "inv", "dx"))}
