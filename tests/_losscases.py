"""Case lists, inputs, float64 / fp32 references and error bounds of the loss-kernel sweep (tests/test_gpu_loss_sweep.py: every
kernel of spatial-clip_amd/csrc/sc_loss.hip called directly) and of its CPU-side check (tests/test_cpu_loss_reference.py).
CPU only: importing this module needs neither a GPU nor the HIP library.

References are plain PyTorch on exactly the values the kernel receives: the fp32 ``z`` matrix is widened exactly; scale, bias,
cap and ``alpha * alpha_scale`` are taken at the fp32 value the kernel sees (``f32``) and then widened; the soft labels are
dense float64 matrices formed from those fp32 products.  Every reference function takes a ``dt``: float64 gives the
reference, float32 the same code as the fp32 CPU reference whose error E32 scales the bounds.

Bounds (none is a constant tuned to a kernel):

* Tensors (dz, the columns of rowstats / rowpart, exp_scalar): the reference-relative rule of tests/_refbounds.py, every
  element within ``REF_FACTOR * E32 + ulp_fp32(|float64 value|)`` (``check_f32``).
* Row reductions and scalars (rowstats, rowpart, rowgrad, loss, gap, d_scale, d_bias, PCC): that allowance plus the derived
  chain term of ``check_sum``, ``k * u * sum|term|`` (``check_red``): k is the longest fp32 addition chain of the kernel's own
  summation order (``block_chain`` and the functions after it, each citing its source lines) plus the roundings of the few
  operations that follow the sum, and sum|term| is taken over the finest terms of the sum.  The derived term keeps a scalar
  whose fp32 reference happens to be exact from being held to one ulp.
* Sums of terms that carry p = exp(x - max) weight each such term by ``expo`` = 1 + |exponent| / k: the exponent is one fma and
  its rounding, u * |exponent|, is relative in p.  Nothing is allowed for the exponential itself beyond one rounding.
* dz at G <= ``CANCEL_MAX_G`` = 2 only (``cancels``): there a whole dz tensor is a cancellation (G = 1: p = 1 = target, E32 = 0;
  G = 2: p - target of a saturated pair, E32 ~ 1e-28), the tensor rule collapses to one ulp of a residue, and fp32 cannot do
  better: p is known to u, a label column takes nlab subtractions.  Those tensors, and no others, add a per-element derived
  term over their uncancelled terms |s c| p + |s c| target, written down where it is formed.  At every G > 2 dz is held to the
  tensor rule alone.
* Label weights: ``(K + 2) * u`` relative (``check_sum`` with |value| as the term): the kernel adds the K neighbour weights one
  after another into the norm (sc_loss.hip:51-53: K additions) and divides once (:58, :62); the product alpha * alpha_scale
  is part of the input.  Columns are compared exactly.
* scale_by_scalar, exp_scalar_bwd: bit-equal to the fp32 expression.  axpby_scalars: see ``axpby_refs``.
"""
import collections
import math
import os
import re

import torch

from tests._refbounds import REF_FACTOR, U32, Ref, check_f32, check_sum, ulp  # noqa: F401  (re-exported to the tests)

CANCEL_MAX_G = 2


def cancels(G: int) -> bool:
    """Row lengths at which a whole dz tensor is a cancellation residue (see the module docstring)."""
    return G <= CANCEL_MAX_G


def _resident_max_g() -> int:
    """SC_DISTILL_RESIDENT_MAX_G as the public header defines it (what ops.distill_resident_max_g() returns; read from the
    source so that this module needs no library)."""
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spatial_clip_hip.h")
    with open(hdr) as f:
        return int(re.search(r"#define\s+SC_DISTILL_RESIDENT_MAX_G\s+(\d+)", f.read()).group(1))


RESIDENT_MAX_G = _resident_max_g()


def f32(v) -> float:
    """The fp32 value a kernel sees for a host scalar, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------- summation chains
def block_chain(n: int) -> int:
    """Longest fp32 addition chain of a 256-thread block reduction over n terms: a thread's stride-256 loop (ceil(n / 256)
    additions, e.g. sc_loss.hip:110-115), the 6 shuffle levels of sc_wave_sum and the 3 additions across sm[4]
    (block_sum, sc_loss.hip:74-80)."""
    return math.ceil(n / 256) + 6 + 3


def fwd_row_chain(G: int) -> int:
    """loss_rows_fwd_kernel (sc_loss.hip:109-133): the exp-sum and the exp * z sum over the row (block_chain each; the
    product e * zz rounds once per term: +1), then logf and the addition of the maximum (:130: +2) or the division (:131: +1)."""
    return block_chain(G) + 3


def label_chain(nlab: int) -> int:
    """Thread 0's loop over the row's labels (sc_loss.hip:120-128): per label the logit (one fma), the product with the
    weight and the addition (3 roundings, one after another)."""
    return 3 * nlab


def finalize_chain(B: int) -> int:
    """loss_finalize_kernel (sc_loss.hip:141-160): the difference of two row statistics (1), the block reduction over B,
    the division by B (1), the sum of the two directions and its half (1), the regulariser w * gap * gap and its addition
    (3).  siglip_finalize_kernel (:294-308) and distill_finalize_kernel (:411-436) have the same loop and fewer operations
    after it."""
    return block_chain(B) + 6


def bwd_row_chain(G: int, nlab: int) -> int:
    """loss_rows_bwd_kernel (sc_loss.hip:181-208): dl = c1*p + c2*p*(z - m) (4 roundings), dl * z (1), the block reduction,
    thread 0's nlab subtractions of c1 * q before it (:198) and the subtraction of c1 * rowstats[3] after it (:207: 2)."""
    return block_chain(G) + nlab + 7


def scalar_grads_chain(nrows: int) -> int:
    """loss_scalar_grads_kernel (sc_loss.hip:215-225): one block reduction over the 2B rows."""
    return block_chain(nrows)


def siglip_row_chain(G: int) -> int:
    """siglip_rows_kernel (sc_loss.hip:265-280): per term max(t, 0) + log1p(e) or dl * z (2 roundings), the block reduction."""
    return block_chain(G) + 2


def distill_row_chain(G: int) -> int:
    """distill_rows_kernel (sc_loss.hip:352-396): the exp-sum (block_chain), logf and lns - xs (2), the product with p_t and
    its own normalisation 1 / sum (3), then the block reduction of the terms (block_chain)."""
    return 2 * block_chain(G) + 5


def pcc_chain(cols: int) -> int:
    """pcc_rows_kernel (sc_loss.hip:459-479): the mean (a block reduction and a division), the centred products (2 roundings
    per term), their block reduction, two square roots, a product and a division (4)."""
    return 2 * block_chain(cols) + 7


# ---------------------------------------------------------------------------------------------------------- checking
# ref: the float64 reference with E32; r32: the fp32 CPU reference; abs_sum / k None: a tensor under the reference-relative rule
Out = collections.namedtuple("Out", "ref abs_sum k r32")


def out(r64, r32, abs_sum=None, k=None) -> Out:
    r64, r32 = r64.detach(), r32.detach().reshape(r64.shape)
    return Out(Ref(r64, r32), None if abs_sum is None else abs_sum.detach().double().reshape(r64.shape), k, r32)


def check_red(name: str, got: torch.Tensor, ref: Ref, abs_sum: torch.Tensor, k: int) -> float:
    """Row reductions and scalars: the allowance of ``check_f32`` plus the chain term of ``check_sum``."""
    got = got.detach().cpu().double().reshape(ref.r64.shape)
    allowed = ref.allowed_f32() + k * U32 * abs_sum
    r = (got - ref.r64).abs() / allowed
    ratio = float("nan") if bool(torch.isnan(r).any()) else float(r.max()) if r.numel() else 0.0
    print(f"  {name}: ratio {ratio:.3g} (E32 {ref.e32:.3g}, k = {k})")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio} (E32 = {ref.e32}, k = {k})"
    return ratio


def check(name: str, got: torch.Tensor, o: Out) -> float:
    if o.abs_sum is None:
        return check_f32(name, got.detach().reshape(o.ref.r64.shape), o.ref)
    return check_red(name, got, o.ref, o.abs_sum, o.k)


def finite(refs: dict) -> bool:
    """No NaN / Inf in any float64 reference or allowance of a family's outputs."""
    for o in refs.values():
        if not bool(torch.isfinite(o.ref.r64).all()) or not math.isfinite(o.ref.e32):
            return False
        if o.abs_sum is not None and not bool(torch.isfinite(o.abs_sum).all()):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------- z matrices
VALUES = ("cos", "equal", "peak", "max0", "maxlast", "ties")


def z_matrix(vals: str, lead: int, B: int, G: int, col0: int, seed: int) -> torch.Tensor:
    """fp32 [lead, B, G] with entries in [-1, 1].  cos: cosine-like random rows with a raised diagonal (column col0 + i);
    equal: every entry 0.3; peak: one entry at 1 per row (column (7 r + 3) % G), the rest at -1; max0 / maxlast: cos with
    the row maximum 1 at column 0 / G - 1; ties: cos rounded to quarters, so that rows hold exact ties with their diagonal."""
    g = torch.Generator().manual_seed(7919 * seed + 13 * G + B)
    rows = lead * B
    z = (0.25 * torch.randn(rows, G, generator=g)).clamp(-1.0, 1.0)
    r = torch.arange(rows)
    z[r, col0 + r % B] = 0.4 + 0.5 * torch.rand(rows, generator=g)
    if vals == "equal":
        z.fill_(0.3)
    elif vals == "peak":
        z.fill_(-1.0)
        z[r, (7 * r + 3) % G] = 1.0
    elif vals == "max0":
        z[:, 0] = 1.0
    elif vals == "maxlast":
        z[:, G - 1] = 1.0
    elif vals == "ties":
        z = torch.round(z * 4.0) / 4.0
    elif vals != "cos":
        raise ValueError(vals)
    return z.float().reshape(lead, B, G).contiguous()


# ---------------------------------------------------------------------------------------------------------- neighbour join
JoinCase = collections.namedtuple("JoinCase", "B G K rank flavor")
JOIN_K = (0, 1, 4, 5, 8, 63)
JOIN_G = (1, 63, 64, 65, 257, 1025)
JOIN_TAGS = {"perm", "dup_same_stride", "dup_other_stride", "col0", "own", "twice", "absent", "alpha0", "alpha_neg", "scale0",
             "high_word", "minus1"}
# flavor: "" ordinary, "scale0" alpha_scale = 0, "high" ids above 2^32 that differ only in the high word
JOIN_CASES = ([JoinCase(min(8, G), G, 8, 0, "") for G in JOIN_G] +
              [JoinCase(8, 257, K, 0, "") for K in JOIN_K if K != 8] +
              [JoinCase(8, 65, 5, 3, ""), JoinCase(8, 64, 4, 7, ""), JoinCase(5, 1025, 63, 204, ""),
               JoinCase(8, 257, 8, 1, "scale0"), JoinCase(8, 257, 8, 2, "high"), JoinCase(8, 257, 63, 0, "high"),
               JoinCase(3, 63, 1, 20, ""), JoinCase(1, 1, 4, 0, "")])


def join_case_id(c: JoinCase) -> str:
    tags = [f"B{c.B}", f"G{c.G}", f"K{c.K}", f"rank{c.rank}", f"{math.ceil(c.G / 64)}strides", f"{math.ceil(c.K / 4)}k-per-wave"]
    if c.flavor:
        tags.append(c.flavor)
    return "-".join(tags)


def join_inputs(c: JoinCase):
    """(all_image_ids, all_text_ids [G] int64, neighbour ids [B, K] int64, alphas [B, K] fp32, alpha_scale, tags): the
    structures of JOIN_TAGS are put in wherever G and K have room for them; ``tags`` names those present."""
    B, G, K, rank = c.B, c.G, c.K, c.rank
    g = torch.Generator().manual_seed(1009 * G + 31 * K + B)
    tags = set()
    perm = torch.randperm(G, generator=g).long()
    txt = 1000 + perm
    if c.flavor == "high":
        # unique ids whose low words repeat (97 values): a compare of the low 32 bits alone would take a later column
        txt = (perm % 97) + ((perm // 97 + 1) << 32)
        if G > 97:
            tags.add("high_word")
    if G > 2:
        txt[2] = -1
        tags.add("minus1")
    if G > 20:
        txt[20] = txt[10]            # both in the first 64-column stride: the wave maximum decides
        tags.add("dup_same_stride")
    if G > 69:
        txt[69] = txt[5]             # lane 5 meets the id again in its second stride
        txt[G - 1] = txt[7]          # another lane, a later stride
        tags.add("dup_other_stride")
    img = txt.clone()
    if G > 3:
        img = txt[torch.randperm(G, generator=g)]
        tags.add("perm")
    nbr = txt[torch.randint(0, G, (B, max(K, 1)), generator=g)][:, :K].contiguous()
    alpha = (0.05 + torch.rand(B, max(K, 1), generator=g))[:, :K].contiguous()
    specials = ["col0", "own", "twice", "absent", "alpha0", "alpha_neg", "minus1", "dup_a", "dup_b", "dup_c", "plain"]
    for i in range(B):
        for k in range(K):
            sp = specials[(3 * i + k) % len(specials)]
            if sp == "col0":
                nbr[i, k] = txt[0]; tags.add("col0")
            elif sp == "own":
                nbr[i, k] = txt[rank * B + i]; tags.add("own")
            elif sp == "twice" and k + 1 < K:
                nbr[i, k] = nbr[i, k + 1]                    # as the next column, unless that one becomes a special itself
            elif sp == "absent":
                nbr[i, k] = 999_999_999; tags.add("absent")
            elif sp == "alpha0":
                alpha[i, k] = 0.0; tags.add("alpha0")
            elif sp == "alpha_neg":
                alpha[i, k] = -0.5; tags.add("alpha_neg")
            elif sp == "minus1" and G > 2:
                nbr[i, k] = -1
            elif sp == "dup_a" and G > 20:
                nbr[i, k] = txt[10]
            elif sp == "dup_b" and G > 69:
                nbr[i, k] = txt[5]
            elif sp == "dup_c" and G > 69:
                nbr[i, k] = txt[7]
    # "twice": a pair (k, k + 2) of one row with the same present id and positive alphas, wherever K has room
    for i in range(B):
        if K >= 3:
            k = (2 * i) % (K - 2)
            nbr[i, k] = nbr[i, k + 2] = txt[(11 * i + 1) % G]
            alpha[i, k], alpha[i, k + 2] = 0.25, 0.5
            tags.add("twice")
    alpha_scale = 0.5
    if c.flavor == "scale0":
        alpha_scale = 0.0
        tags.add("scale0")
    return img.contiguous(), txt.contiguous(), nbr, alpha.float(), alpha_scale, tags


def join_sparse(img, txt, nbr, alpha, B, G, K, rank, alpha_scale, dt):
    """The join by the reference's rules (dict of id -> LAST column; alpha * scale <= 0 skipped before lookup; L1 norm with
    eps 1e-12) in the kernel's sparse form: col [2, B, K + 1] int32 (-1: no entry), w [2, B, K + 1] of ``dt``.  dt float32
    adds the norm in the kernel's order (1, then the K weights in turn): the fp32 reference; dt float64: exact to 2^-53."""
    a = (alpha.float() * torch.tensor(alpha_scale, dtype=torch.float32)).clamp_min(0.0)     # the fp32 product, as the kernel
    col = torch.full((2, B, K + 1), -1, dtype=torch.int32)
    col[:, :, 0] = rank * B + torch.arange(B, dtype=torch.int32)
    lut = [{int(t): j for j, t in enumerate(ids.tolist())} for ids in (txt, img)]      # direction 0 looks up text ids
    nb, al = nbr.tolist(), a.tolist()
    for d in range(2):
        for i in range(B):
            for k in range(K):
                if al[i][k] > 0.0:
                    col[d, i, 1 + k] = lut[d].get(int(nb[i][k]), -1)
    w = torch.zeros((2, B, K + 1), dtype=dt)
    w[:, :, 0] = 1.0
    w[:, :, 1:] = torch.where(col[:, :, 1:] >= 0, a.to(dt).unsqueeze(0).expand(2, B, K), torch.zeros((), dtype=dt))
    norm = torch.ones((2, B), dtype=dt)
    for k in range(K):
        norm = norm + w[:, :, 1 + k]
    return col, w / norm.clamp_min(1e-12).unsqueeze(-1)


def dense_labels(col, w, G, dt=torch.float64):
    """Dense [2, B, G] label matrices from (col, weight) pairs: scatter-add, repeated columns accumulate, col < 0 dropped."""
    q = torch.zeros(col.shape[:2] + (G,), dtype=dt)
    keep = col >= 0
    q.scatter_add_(2, col.clamp_min(0).long(), torch.where(keep, w.to(dt), torch.zeros((), dtype=dt)))
    return q


# ---------------------------------------------------------------------------------------------------------- loss cases
LOSS_G = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
LOSS_B = (1, 2, 3, 255, 256, 257, 513)
DISTILL_G = LOSS_G + (769, RESIDENT_MAX_G - 1, RESIDENT_MAX_G, RESIDENT_MAX_G + 1)
SCALES = (1.0, 14.2857, 100.0)
CAP_BELOW, CAP_ABOVE = 40.0, 120.0          # the project's default cap and one no scale of SCALES reaches
# (scale, cap, bias, temp_reg_weight): each scale, cap on either side of the scale, each bias, both weights
SCALARS = ((1.0, None, None, 0.0), (14.2857, None, None, 0.05), (100.0, None, None, 0.0), (100.0, CAP_BELOW, -10.0, 0.05),
           (14.2857, CAP_ABOVE, 3.0, 0.05), (100.0, CAP_ABOVE, -10.0, 0.0))

LossCase = collections.namedtuple("LossCase", "B G rank vals scale cap bias w K go")


def _smallest_g(B):
    return min(G for G in LOSS_G if G >= B)


def _shape_cases(g_list):
    """(B, G, rank): G swept at B = 3 (B = G below 3), B swept at its smallest G, multi-rank layouts first / middle / last."""
    shapes = [(min(3, G), G, 0) for G in g_list]
    shapes += [(B, _smallest_g(B), 0) for B in LOSS_B if (B, _smallest_g(B), 0) not in shapes]
    shapes += [(21, 63, 0), (21, 63, 1), (21, 63, 2), (3, 513, 170)]
    return shapes


VALUE_SHAPES = ((3, 65, 0), (2, 2, 0), (3, 513, 85))      # where the value cases are crossed with the scalars


def _loss_cases():
    cases, n = [], 0
    ks, gos = (5, 0, 1, 8), (None, -2.5)
    for B, G, rank in _shape_cases(LOSS_G):
        sc = SCALARS[n % len(SCALARS)]
        cases.append(LossCase(B, G, rank, "cos", *sc, ks[n % 4], gos[n % 2])); n += 1
    for B, G, rank in VALUE_SHAPES:
        for vals in VALUES:
            for sc in (SCALARS if G == 65 else SCALARS[2:4]):
                cases.append(LossCase(B, G, rank, vals, *sc, ks[n % 4], gos[(n // 2) % 2])); n += 1
    return cases


LOSS_CASES = _loss_cases()


def loss_case_id(c: LossCase) -> str:
    tags = [f"B{c.B}", f"G{c.G}", f"rank{c.rank}", c.vals, f"s{c.scale:g}", f"cap{c.cap:g}" if c.cap else "nocap",
            f"b{c.bias:g}" if c.bias is not None else "nobias", f"w{c.w:g}", f"nlab{c.K + 1}",
            "go1" if c.go is None else f"go{c.go:g}"]
    if c.G < 64:
        tags.append("one-wave")
    elif c.G < 256:
        tags.append("partial-block")
    elif c.G % 256:
        tags.append(f"{c.G // 256}x256+{c.G % 256}")
    if c.B > 256:
        tags.append("finalize-loops")
    return "-".join(tags)


def loss_inputs(c: LossCase):
    """z [2, B, G] fp32, sparse labels (col int32, w fp32 [2, B, K + 1]: the fp32 join of a small id problem, with -1
    columns and repeated columns), the effective scale and the bias at their fp32 values."""
    z = z_matrix(c.vals, 2, c.B, c.G, c.rank * c.B, 1)
    img, txt, nbr, alpha, a_scale, _ = join_inputs(JoinCase(c.B, c.G, c.K, c.rank, ""))
    col, w = join_sparse(img, txt, nbr, alpha, c.B, c.G, c.K, c.rank, a_scale, torch.float32)
    s = f32(c.scale)
    s_eff = min(s, f32(c.cap)) if c.cap else s
    return z, col.contiguous(), w.contiguous(), s_eff, (0.0 if c.bias is None else f32(c.bias))


def clip_fwd(z, q, s, b, wreg, dt):
    """Forward of ClipLoss / SpatialLoss on z [2, B, G] and dense labels q in ``dt``: rowstats [2B, 4] = (lse, E_p[z],
    sum q * logit, sum q * z) and loss_out [4] = (loss, gap, CE_image, CE_text), with the pieces the bounds need."""
    z, q = z.to(dt), q.to(dt)
    x = s * z + b
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse.unsqueeze(-1))
    epz, ql, qz = (p * z).sum(-1), (q * x).sum(-1), (q * z).sum(-1)
    ce = (lse - ql).mean(-1)
    gap = 0.5 * (epz - qz).mean(-1).sum()
    loss = 0.5 * ce.sum() + (wreg * gap * gap if wreg > 0 else 0.0)
    return {"rowstats": torch.stack([lse, epz, ql, qz], -1).reshape(-1, 4), "loss_out": torch.stack([loss, gap, ce[0], ce[1]]),
            "x": x, "p": p, "gap": gap}


def clip_fwd_refs(z, col, w, s, b, wreg):
    B, G, nlab = z.shape[1], z.shape[2], col.shape[2]
    q = dense_labels(col, w, G)
    r64, r32 = clip_fwd(z, q, s, b, wreg, torch.float64), clip_fwd(z, q, s, b, wreg, torch.float32)
    x, p, zz = r64["x"], r64["p"], z.double()
    rs = r64["rowstats"]
    a_lse = 1.0 + rs[:, 0].abs()                                    # d lse = d(sum e) / sum e; + the value's own rounding
    kr = fwd_row_chain(G)
    a_epz = 2.0 * (p * zz.abs() * expo(x - x.max(-1, keepdim=True).values, kr)).sum(-1).reshape(-1)    # sum(e z) / sum(e)
    a_ql, a_qz = (q * x.abs()).sum(-1).reshape(-1), (q * zz.abs()).sum(-1).reshape(-1)
    kl = label_chain(nlab)
    refs = {"lse": out(rs[:, 0], r32["rowstats"][:, 0], a_lse, kr), "E_p[z]": out(rs[:, 1], r32["rowstats"][:, 1], a_epz, kr),
            "sum q*logit": out(rs[:, 2], r32["rowstats"][:, 2], a_ql, kl), "sum q*z": out(rs[:, 3], r32["rowstats"][:, 3], a_qz, kl)}
    # loss_out: the finalize kernel sums the kernel's own row statistics; chain = the rows' chain + the finalize chain, the
    # terms those of the rows, averaged as the kernel averages them
    a_ce = (a_lse + a_ql).reshape(2, B).mean(-1)
    a_gap = 0.5 * (a_epz + a_qz).reshape(2, B).mean(-1).sum()
    gap = r64["gap"].abs()
    a_loss = 0.5 * a_ce.sum() + (2.0 * wreg * gap * a_gap + wreg * gap * gap if wreg > 0 else 0.0)
    k = max(kr, kl) + finalize_chain(B)
    lo64, lo32 = r64["loss_out"], r32["loss_out"]
    refs.update({"loss": out(lo64[0], lo32[0], a_loss, k), "gap": out(lo64[1], lo32[1], a_gap, k),
                 "CE_image": out(lo64[2], lo32[2], a_ce[0], k), "CE_text": out(lo64[3], lo32[3], a_ce[1], k)})
    return refs


BWD_ELEM_K = 8      # roundings of one dz element (sc_loss.hip:187-194): expf, c1*p, c2*p*(z - m) (3), their sum, s*dl + c2*p (2)


def expo(exponent, k):
    """Weight of a term that carries p = exp(exponent): 1 + |exponent| / k, so that k * u * weight * |term| allows, next to the
    k roundings of the chain, for the rounding of the exponent itself (one fma: u * |exponent|, relative in p)."""
    return 1.0 + exponent.abs() / k


def clip_bwd(z, q, s, b, wreg, go, lse, mi, gap, dt, nlab=1, kr=1):
    """Backward at the given row statistics (lse, E_p[z] per row) and gap: dz [2, B, G], rowgrad [2B, 2] = (sum dl * z, sum dl),
    d_scale, d_bias; dl = c1 (p - q) + c2 p (z - m), dz = s dl + c2 (p - q), c1 = go / 2B, c2 = go w gap / B."""
    z, q = z.to(dt), q.to(dt)
    B = z.shape[1]
    lse, mi = lse.to(dt).reshape(2, B, 1), mi.to(dt).reshape(2, B, 1)
    c1 = go * 0.5 / B
    c2 = go * wreg * float(gap) / B if wreg > 0 else 0.0
    p = torch.exp(s * z + b - lse)
    dense = c1 * p + c2 * p * (z - mi)
    dl = dense - c1 * q
    dz = s * dl + c2 * (p - q)
    rowgrad = torch.stack([(dl * z).sum(-1), dl.sum(-1)], -1).reshape(-1, 2)
    # uncancelled terms: T of the dense part of dz, each carrying p with the rounding of its exponent fma(s, z, b - lse) (the
    # rounding of b - lse itself: u |b - lse|, none without a bias) -- weight ``expo``; the label columns then take up to nlab
    # subtractions of (s c1 + c2) q one after another (sc_loss.hip:194-201)
    kp, nlab_ = BWD_ELEM_K, float(nlab)
    # (loss_rows_bwd_kernel rounds s * z + b at the size of the logit before it subtracts lse; the fp32 reference does the same,
    # so that error is E32's.  The term here is the part no evaluation order in fp32 avoids.)
    wp = expo((s * z + b - lse).abs() + ((b - lse).abs() if b != 0.0 else 0.0), kp)
    t_dz = (abs(s * c1) * p + abs(s * c2) * p * (z - mi).abs() + abs(c2) * p)
    a_dz = t_dz * wp + (q > 0).to(dt) * (t_dz + abs(s * c1 + c2) * q) * (nlab_ + 1.0) / kp
    wr = expo((s * z + b - lse).abs() + ((b - lse).abs() if b != 0.0 else 0.0), kr)
    return {"dz": dz, "rowgrad": rowgrad, "d_scale": rowgrad[:, 0].sum(), "d_bias": rowgrad[:, 1].sum(), "a_dz": a_dz,
            "a0": (dense * z * wr).abs().sum(-1) + abs(c1) * (q * z.abs()).sum(-1),
            "a1": (dense * wr).abs().sum(-1) + abs(c1) * q.sum(-1)}


def clip_bwd_refs(z, col, w, s, b, wreg, go, rowstats, loss_out):
    """``rowstats`` / ``loss_out``: the values the backward kernel receives (the forward kernel's own, as fp32 tensors)."""
    B, G, nlab = z.shape[1], z.shape[2], col.shape[2]
    q = dense_labels(col, w, G)
    go = 1.0 if go is None else f32(go)
    rs, gap = rowstats.detach().cpu().float(), float(loss_out.detach().cpu().float()[1])
    kr = bwd_row_chain(G, nlab)
    r64 = clip_bwd(z, q, s, b, wreg, go, rs[:, 0], rs[:, 1], gap, torch.float64, nlab, kr)
    r32 = clip_bwd(z, q, s, b, wreg, go, rs[:, 0], rs[:, 1], gap, torch.float32, nlab, kr)
    ks = kr + scalar_grads_chain(2 * B)
    a0, a1 = r64["a0"].reshape(-1), r64["a1"].reshape(-1)
    return {"dz": out(r64["dz"], r32["dz"], r64["a_dz"], BWD_ELEM_K) if cancels(G) else out(r64["dz"], r32["dz"]),
            "rowgrad sum dl*z": out(r64["rowgrad"][:, 0], r32["rowgrad"][:, 0], a0, kr),
            "rowgrad sum dl": out(r64["rowgrad"][:, 1], r32["rowgrad"][:, 1], a1, kr),
            "d_scale": out(r64["d_scale"], r32["d_scale"], a0.sum(), ks),
            "d_bias": out(r64["d_bias"], r32["d_bias"], a1.sum(), ks)}


# ---------------------------------------------------------------------------------------------------------- SigLIP
SigCase = collections.namedtuple("SigCase", "B G rank vals scale bias")


def _sig_cases():
    cases, n = [], 0
    sb = ((1.0, None), (14.2857, -10.0), (100.0, -10.0), (100.0, 3.0), (14.2857, None))
    for B, G, rank in _shape_cases(LOSS_G):
        cases.append(SigCase(B, G, rank, "cos", *sb[n % len(sb)])); n += 1
    for B, G, rank in VALUE_SHAPES:
        for vals in VALUES:
            for s_b in (sb if G == 65 else sb[2:4]):
                cases.append(SigCase(B, G, rank, vals, *s_b))
    return cases


SIG_CASES = _sig_cases()


def sig_case_id(c: SigCase) -> str:
    return "-".join([f"B{c.B}", f"G{c.G}", f"rank{c.rank}", c.vals, f"s{c.scale:g}", f"b{c.bias:g}" if c.bias is not None else "nobias"]
                    + (["finalize-loops"] if c.B > 256 else []) + (["one-wave"] if c.G < 64 else []))


SIG_ELEM_K = 6      # roundings of one dz element (sc_loss.hip:267-276): expf, 1 + e, the reciprocal, e * r, s / B, c * dl


def siglip(z, s, b, col0, dt):
    """z [B, G]: dz [B, G], rowpart [B, 3] = (sum loss, sum dl * z, sum dl), loss, d_scale, d_bias (softplus as logaddexp)."""
    z = z.to(dt)
    B, G = z.shape
    y = -torch.ones(B, G, dtype=dt)
    y[torch.arange(B), col0 + torch.arange(B)] = 1.0
    t = -y * (s * z + b)
    per = torch.logaddexp(t, torch.zeros((), dtype=dt))
    dl = -y * torch.sigmoid(t)
    rowpart = torch.stack([per.sum(-1), (dl * z).sum(-1), dl.sum(-1)], -1)
    # the logit x = fma(s, z, b) is rounded once, u |x|: softplus passes that on with its slope sigmoid(t), dl = +-sigmoid(t)
    # with sigmoid'(t) = sigmoid (1 - sigmoid) (nothing on a saturated element, all of it on a small one)
    kr = siglip_row_chain(G)
    sg = torch.sigmoid(t)
    dsg = sg * (1.0 - sg) * t.abs()
    return {"dz": (s / B) * dl, "rowpart": rowpart, "tot": rowpart.sum(0) / B,
            "a_dz": abs(s / B) * (dl.abs() + dsg / SIG_ELEM_K),
            "abs": torch.stack([(per + sg * t.abs() / kr).sum(-1), ((dl.abs() + dsg / kr) * z.abs()).sum(-1),
                                (dl.abs() + dsg / kr).sum(-1)], -1)}


def siglip_refs(z, s, b, col0):
    B, G = z.shape
    r64, r32 = siglip(z, s, b, col0, torch.float64), siglip(z, s, b, col0, torch.float32)
    kr = siglip_row_chain(G)
    k = kr + finalize_chain(B)
    refs = {"dz": out(r64["dz"], r32["dz"], r64["a_dz"], SIG_ELEM_K) if cancels(G) else out(r64["dz"], r32["dz"])}
    for j, (row, tot) in enumerate((("rowpart sum loss", "loss"), ("rowpart sum dl*z", "d_scale"), ("rowpart sum dl", "d_bias"))):
        refs[row] = out(r64["rowpart"][:, j], r32["rowpart"][:, j], r64["abs"][:, j], kr)
        refs[tot] = out(r64["tot"][j], r32["tot"][j], r64["abs"][:, j].sum() / B, k)
    return refs


# ---------------------------------------------------------------------------------------------------------- distillation
DistCase = collections.namedtuple("DistCase", "B G rank vals tvals scale tscale")


def _dist_cases():
    cases, n = [], 0
    st = ((14.2857, 25.0), (100.0, 60.0), (1.0, 100.0), (100.0, 100.0))
    for B, G, rank in _shape_cases(DISTILL_G):
        cases.append(DistCase(B, G, rank, "cos", ("cos", "peak")[n % 2], *st[n % len(st)])); n += 1
    for B, G, rank in VALUE_SHAPES:
        for vals in VALUES:
            for tvals, s_t in (("peak", st[1]), ("cos", st[0]), ("equal", st[2])):
                cases.append(DistCase(B, G, rank, vals, tvals, *s_t))
    return cases


DIST_CASES = _dist_cases()


def dist_case_id(c: DistCase) -> str:
    tags = [f"B{c.B}", f"G{c.G}", f"rank{c.rank}", c.vals, f"teacher-{c.tvals}", f"s{c.scale:g}", f"st{c.tscale:g}",
            "resident" if c.G <= RESIDENT_MAX_G else "streamed", f"slot{(c.G - 1) // 256}"]
    if c.B > 256:
        tags.append("finalize-loops")
    return "-".join(tags)


# roundings of one dz element at G <= 2 (sc_loss.hip:357-382): expf, the sum of at most two exponentials (the other additions of
# the block reduction add exact zeros), its reciprocal, e * inv, p - target, c * (..), s * (..)
DIST_ELEM_K = 7


def distill(zs, zt, s, st, col0, dt):
    """z_s, z_t [2, B, G]: dz_c, dz_d, rowpart [2B, 4] = (CE, D, sum dl_c * z_s, sum dl_d * z_s), loss_out [4] = (contrastive,
    distill, CE_image, CE_text), d_scale_c, d_scale_d.  D = sum p_t (lse - x_s): every term >= 0."""
    zs, zt = zs.to(dt), zt.to(dt)
    _, B, G = zs.shape
    x = s * zs
    lse = torch.logsumexp(x, -1, keepdim=True)
    ps, pt = torch.exp(x - lse), torch.softmax(st * zt, -1)
    on = torch.zeros(2, B, G, dtype=dt)
    on[:, torch.arange(B), col0 + torch.arange(B)] = 1.0
    nl = lse - x
    c = 0.5 / B
    dlc, dld = c * (ps - on), c * (ps - pt)
    ce, dd = (on * nl).sum(-1), (pt * nl).sum(-1)
    rowpart = torch.stack([ce, dd, (dlc * zs).sum(-1), (dld * zs).sum(-1)], -1).reshape(-1, 4)
    cem, ddm = ce.mean(-1), dd.mean(-1)
    # the kernel works on shifted exponents xs = x - max, xt (sc_loss.hip:357-372): uncancelled terms, p_s and p_t weighted by
    # the rounding of their exponents (``expo``); CE and D through lns = log(sum) (d lns = d sum / sum: the 1) and lns - xs
    kr = distill_row_chain(G)
    xs, xt = x - x.max(-1, keepdim=True).values, st * zt - (st * zt).max(-1, keepdim=True).values
    lns = lse - x.max(-1, keepdim=True).values
    ws, wt = ps * expo(xs, kr), pt * expo(xt, kr)
    nla = 1.0 + lns.abs() + xs.abs()
    return {"dz_c": s * dlc, "dz_d": s * dld, "rowpart": rowpart,
            "loss_out": torch.stack([0.5 * cem.sum(), 0.5 * ddm.sum(), cem[0], cem[1]]),
            "d_scale_c": rowpart[:, 2].sum(), "d_scale_d": rowpart[:, 3].sum(),
            "a_dz_c": abs(s * c) * (ps * expo(xs, DIST_ELEM_K) + on),
            "a_dz_d": abs(s * c) * (ps * expo(xs, DIST_ELEM_K) + pt * expo(xt, DIST_ELEM_K)),
            "abs": torch.stack([(on * nla).sum(-1), (wt * nla).sum(-1), c * ((ws + on) * zs.abs()).sum(-1),
                                c * ((ws + wt) * zs.abs()).sum(-1)], -1).reshape(-1, 4)}


def distill_refs(zs, zt, s, st, col0):
    _, B, G = zs.shape
    r64, r32 = distill(zs, zt, s, st, col0, torch.float64), distill(zs, zt, s, st, col0, torch.float32)
    kr = distill_row_chain(G)
    k = kr + finalize_chain(B)
    a = r64["abs"]
    if cancels(G):
        refs = {"dz_c": out(r64["dz_c"], r32["dz_c"], r64["a_dz_c"], DIST_ELEM_K),
                "dz_d": out(r64["dz_d"], r32["dz_d"], r64["a_dz_d"], DIST_ELEM_K)}
    else:
        refs = {"dz_c": out(r64["dz_c"], r32["dz_c"]), "dz_d": out(r64["dz_d"], r32["dz_d"])}
    for j, name in enumerate(("rowpart CE", "rowpart D", "rowpart sum dl_c*z", "rowpart sum dl_d*z")):
        refs[name] = out(r64["rowpart"][:, j], r32["rowpart"][:, j], a[:, j], kr)
    am = a.reshape(2, B, 4).mean(1)          # [2, 4]: per direction, the means the finalize kernel forms
    lo64, lo32 = r64["loss_out"], r32["loss_out"]
    refs.update({"contrastive": out(lo64[0], lo32[0], 0.5 * am[:, 0].sum(), k), "distill": out(lo64[1], lo32[1], 0.5 * am[:, 1].sum(), k),
                 "CE_image": out(lo64[2], lo32[2], am[0, 0], k), "CE_text": out(lo64[3], lo32[3], am[1, 0], k),
                 "d_scale_c": out(r64["d_scale_c"], r32["d_scale_c"], a[:, 2].sum(), k),
                 "d_scale_d": out(r64["d_scale_d"], r32["d_scale_d"], a[:, 3].sum(), k)})
    return refs


def distill_inputs(c: DistCase):
    zs = z_matrix(c.vals, 2, c.B, c.G, c.rank * c.B, 2)
    zt = z_matrix(c.tvals, 2, c.B, c.G, c.rank * c.B, 3)
    return zs, zt, f32(c.scale), f32(c.tscale)


# ---------------------------------------------------------------------------------------------------------- recall
RecallCase = collections.namedtuple("RecallCase", "n G row0 col0 rows vals init")      # z [rows, G]; window of n rows at row0
RECALL_B = (1, 4, 5, 9, 10, 11, 257)
RECALL_CASES = ([RecallCase(n, n, 0, 0, n, v, (0, 0, 0)) for n in RECALL_B for v in ("cos", "ties")] +
                [RecallCase(5, 16, 4, 4, 16, "ties", (3, 1, 4)),          # a window (row0, n) inside a [16, 16] matrix
                 RecallCase(9, 40, 20, 20, 40, "ties", (0, 7, 0)), RecallCase(11, 33, 0, 22, 11, "ties", (1, 2, 3)),   # rank 2 of 3
                 RecallCase(257, 514, 0, 257, 257, "ties", (100, 200, 300)), RecallCase(4, 9, 0, 5, 4, "equal", (0, 0, 0)),
                 RecallCase(10, 10, 0, 0, 10, "equal", (5, 5, 5)), RecallCase(11, 11, 0, 0, 11, "equal", (0, 0, 0))])


def recall_case_id(c: RecallCase) -> str:
    return f"n{c.n}-G{c.G}-row{c.row0}-col{c.col0}-{c.vals}-init{'.'.join(map(str, c.init))}"


def recall_inputs(c: RecallCase) -> torch.Tensor:
    """z [rows, G] fp32; the diagonal of the window's rows sits at column col0 + (row - row0)."""
    return z_matrix(c.vals, 1, c.rows, c.G, c.col0 - c.row0, 5)[0]


def recall_ref(z_rows: torch.Tensor, n: int, col0: int, init) -> list:
    """The kernel's documented rule on rows 0..n-1 of ``z_rows``: rank of row i's diagonal = the count of j in the window with
    z[j] > z[diag], or z[j] == z[diag] and j < i; a hit at k means rank < k.  Integer counters onto ``init``."""
    win = z_rows[:n, col0:col0 + n]
    d = win.diagonal().unsqueeze(1)
    j, i = torch.arange(n).unsqueeze(0), torch.arange(n).unsqueeze(1)
    rank = ((win > d) | ((win == d) & (j < i))).sum(1)
    return [int(init[t]) + int((rank < k).sum()) for t, k in enumerate((1, 5, 10))]


# ---------------------------------------------------------------------------------------------------------- PCC
PccCase = collections.namedtuple("PccCase", "rows cols ldp ldt want_pcc want_sum init")
PCC_COLS = (1, 3, 255, 256, 257, 1000)
PCC_CASES = ([PccCase(5, c, c, c, True, True, (0.0, 0.0)) for c in PCC_COLS] +
             [PccCase(5, 257, 300, 261, True, True, (1.5, 3.0)), PccCase(3, 1000, 1024, 1000, True, False, (0.0, 0.0)),
              PccCase(3, 255, 255, 256, False, True, (-2.0, 7.0)), PccCase(5, 3, 8, 8, True, True, (0.25, 1.0))])


def pcc_case_id(c: PccCase) -> str:
    return (f"rows{c.rows}-cols{c.cols}-ld{c.ldp}.{c.ldt}-{'pcc' if c.want_pcc else 'nopcc'}-"
            f"{'acc' if c.want_sum else 'noacc'}-init{c.init[0]:g}.{c.init[1]:g}")


def pcc_inputs(c: PccCase):
    """pred, target: [rows, cols] views of [rows, ld] buffers.  Row 0 of the prediction is constant (scores 0), row 1 has mean
    1e3 and unit spread (the two-pass form matters); the target rows are rank weights."""
    g = torch.Generator().manual_seed(97 * c.cols + c.rows)
    pb, tb = torch.randn(c.rows, c.ldp, generator=g), torch.rand(c.rows, c.ldt, generator=g)
    pb[0] = 0.75
    if c.rows > 1:
        pb[1] = 1000.0 + torch.randn(c.ldp, generator=g)
    return pb.float(), tb.float()


def pcc(pred, tgt, dt):
    p, t = pred.to(dt), tgt.to(dt)
    pc, tc = p - p.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
    num = (pc * tc).sum(1)
    den = torch.sqrt((pc * pc).sum(1)) * torch.sqrt((tc * tc).sum(1))
    ok = den > 1e-6
    r = torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num))
    return r, torch.where(ok, (pc * tc).abs().sum(1) / torch.where(ok, den, torch.ones_like(den)) + r.abs(), torch.zeros_like(num))


def pcc_refs(pred, tgt, init):
    """pcc [rows]; the accumulators: sum (float atomics in any order: chain = rows) and count (small integers: exact)."""
    (r64, a), (r32, _) = pcc(pred, tgt, torch.float64), pcc(pred, tgt, torch.float32)
    rows, cols = pred.shape
    k = pcc_chain(cols)
    i0 = torch.tensor(float(init[0]), dtype=torch.float64)
    return {"pcc": out(r64, r32, a, k),
            "sum": out(i0 + r64.sum(), (torch.tensor(init[0], dtype=torch.float32) + r32.sum()), i0.abs() + a.sum(), k + rows),
            "count": float(init[1]) + rows}


# ---------------------------------------------------------------------------------------------------------- scalar helpers
EXP_X = (0.0, math.log(14.2857), math.log(100.0), -2.0, 4.6052, 1.0)      # log scales around the ones of SCALES
HELPER_N = (1, 3, 255, 256, 257, 1025, 262145)         # 262145: above 1024 blocks of 256, the grid-stride loops turn


def helper_vectors(n: int):
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def axpby_refs(a, b, fa, fb):
    """out = fa * a + fb * b.  Plain C++ leaves the evaluation open: both products rounded and then added (``plain``), or one
    product kept exact inside a fused multiply-add: ``fma_a`` = fma(fa, a, rn(fb * b)) or ``fma_b`` = fma(fb, b, rn(fa * a)).
    Float64 holds an fp32 product exactly (48 bits), so each form is one float64 addition rounded to fp32 (a double rounding can
    differ from a true fma only when the float64 sum falls within 2^-53 of an fp32 tie).  axpby_scalars_kernel has the ``plain``
    order (the two products are one packed multiply, which no addition is fused into): asserted bitwise; every order lies
    within one rounding of each product and of the sum of the exact value (``slack``)."""
    a64, b64 = a.double(), b.double()
    pa, pb = fa * a64, fb * b64              # exact
    return {"plain": (pa.float().double() + pb.float().double()).float(), "fma_a": (pa + pb.float().double()).float(),
            "fma_b": (pb + pa.float().double()).float(), "exact": pa + pb,
            "slack": 0.5 * (ulp(pa + pb, torch.float32) + ulp(pa, torch.float32) + ulp(pb, torch.float32))}


# ---------------------------------------------------------------------------------------------------------- head level
HEAD_SHAPES = ((3, 9, 2, 8), (65, 130, 1, 33), (257, 257, 0, 96))         # (B, G, rank, D)
HEAD_K = 5


def head_inputs(B, G, rank, D):
    """Unit-norm gathered features [G, D] (image, text, teacher image, teacher text; the local rows are rank's block), ids."""
    g = torch.Generator().manual_seed(101 * G + D)
    nrm = torch.nn.functional.normalize
    img = nrm(torch.randn(G, D, generator=g), dim=-1)
    txt = nrm(img + 0.6 * torch.randn(G, D, generator=g), dim=-1)
    timg = nrm(img + 0.3 * torch.randn(G, D, generator=g), dim=-1)
    ttxt = nrm(txt + 0.3 * torch.randn(G, D, generator=g), dim=-1)
    img_ids, txt_ids, nbr, alpha, a_scale, _ = join_inputs(JoinCase(B, G, HEAD_K, rank, ""))
    return {"img": img, "txt": txt, "timg": timg, "ttxt": ttxt, "img_ids": img_ids, "txt_ids": txt_ids, "nbr": nbr,
            "alpha": alpha, "alpha_scale": a_scale}


def head_loss(kind, h, B, rank, s, b, dt, cap=CAP_BELOW, wreg=0.05, ts=25.0):
    """Autograd of the whole head in ``dt`` on leaf copies of the local rows and of the gathered features (the direct and the
    gathered terms of the gradient are separate outputs of the kernels' head): {loss(es), d_image, d_text, d_all_image,
    d_all_text, d_scale, d_bias}; distillation returns one such dict per term under "c" and "d"."""
    sl = slice(rank * B, (rank + 1) * B)
    leaf = lambda t: t.to(dt).clone().requires_grad_(True)                                  # noqa: E731
    fi, ft, ai, at = leaf(h["img"][sl]), leaf(h["txt"][sl]), leaf(h["img"]), leaf(h["txt"])
    sc, bi = leaf(torch.tensor(s)), leaf(torch.tensor(b))
    zi, zt = fi @ at.T, ft @ ai.T
    G = ai.shape[0]
    diag = rank * B + torch.arange(B)

    def grads(loss):
        g = torch.autograd.grad(loss, [fi, ft, ai, at, sc, bi], allow_unused=True, retain_graph=True)
        g = [torch.zeros_like(x) if y is None else y for x, y in zip([fi, ft, ai, at, sc, bi], g)]
        return dict(zip(("d_image", "d_text", "d_all_image", "d_all_text", "d_scale", "d_bias"), g), loss=loss.detach())
    if kind in ("clip", "spatial"):
        if kind == "clip":
            col = diag.to(torch.int32).reshape(1, B, 1).expand(2, B, 1)
            q = dense_labels(col, torch.ones(2, B, 1, dtype=dt), G, dt)
            s_eff, w = sc, 0.0
        else:
            col, wts = join_sparse(h["img_ids"], h["txt_ids"], h["nbr"], h["alpha"], B, G, HEAD_K, rank, h["alpha_scale"], dt)
            q = dense_labels(col, wts, G, dt)
            s_eff, w = sc + (sc.clamp(max=cap) - sc).detach(), wreg
        z = torch.stack([zi, zt])
        x = s_eff * z + bi
        lse = torch.logsumexp(x, -1)
        ce = (lse - (q * x).sum(-1)).mean(-1)
        gap = 0.5 * ((torch.softmax(x, -1) * z).sum(-1) - (q * z).sum(-1)).mean(-1).sum()
        return grads(0.5 * ce.sum() + (w * gap * gap if w > 0 else 0.0))
    if kind == "siglip":
        y = -torch.ones(B, G, dtype=dt)
        y[torch.arange(B), diag] = 1.0
        return grads(torch.logaddexp(-y * (sc * zi + bi), torch.zeros((), dtype=dt)).sum() / B)
    if kind == "distill":
        tz = torch.stack([h["timg"][sl].to(dt) @ h["ttxt"].to(dt).T, h["ttxt"][sl].to(dt) @ h["timg"].to(dt).T])
        x = sc * torch.stack([zi, zt])
        nl = torch.logsumexp(x, -1, keepdim=True) - x
        pt = torch.softmax(ts * tz, -1)
        closs = 0.5 * nl[:, torch.arange(B), diag].mean(-1).sum()
        dloss = 0.5 * (pt * nl).sum(-1).mean(-1).sum()
        return {"c": grads(closs), "d": grads(dloss)}
    raise ValueError(kind)


def head_refs(kind, h, B, rank, s, b, cap=CAP_BELOW, wreg=0.05, ts=25.0):
    """{name: Out}.  Tensors under the reference-relative rule (E32 of the fp32 autograd includes the GEMMs).  The scalars add the
    chain term of the row and finalize kernels: sum|term| and k as the kernel-level references form them, on the fp32 rounding
    of the float64 similarity matrix, with D more additions for the similarity products."""
    G, D = h["img"].shape
    kw = dict(cap=cap, wreg=wreg, ts=ts)
    r64, r32 = head_loss(kind, h, B, rank, s, b, torch.float64, **kw), head_loss(kind, h, B, rank, s, b, torch.float32, **kw)
    sl = slice(rank * B, (rank + 1) * B)
    sim = lambda i, t: torch.stack([i[sl].double() @ t.double().T, t[sl].double() @ i.double().T]).float()     # noqa: E731
    z = sim(h["img"], h["txt"])
    if kind in ("clip", "spatial"):
        K = HEAD_K if kind == "spatial" else 0
        col, w = join_sparse(h["img_ids"], h["txt_ids"], h["nbr"][:, :K], h["alpha"][:, :K], B, G, K, rank, h["alpha_scale"],
                             torch.float32)
        s_eff, wr = (min(s, cap), wreg) if kind == "spatial" else (s, 0.0)
        f = clip_fwd_refs(z, col, w, s_eff, b, wr)
        rs = torch.stack([f[n].ref.r64 for n in ("lse", "E_p[z]", "sum q*logit", "sum q*z")], -1)
        lo = torch.stack([f[n].ref.r64 for n in ("loss", "gap", "CE_image", "CE_text")])
        g = clip_bwd_refs(z, col, w, s_eff, b, wr, None, rs, lo)
        fam = {"": {"loss": f["loss"], "d_scale": g["d_scale"], "d_bias": g["d_bias"]}}
    elif kind == "siglip":
        fam = {"": siglip_refs(z[0], s, b, rank * B)}
    else:
        f = distill_refs(z, sim(h["timg"], h["ttxt"]), s, ts, rank * B)
        fam = {"_c": {"loss": f["contrastive"], "d_scale": f["d_scale_c"]}, "_d": {"loss": f["distill"], "d_scale": f["d_scale_d"]}}
    refs = {}
    for tag, terms in fam.items():
        a, c = (r64, r32) if tag == "" else (r64[tag[1]], r32[tag[1]])
        for name in ("d_image", "d_text", "d_all_image", "d_all_text"):
            refs[name + tag] = out(a[name], c[name])
        for name in ("loss", "d_scale", "d_bias"):
            if name in terms:
                refs[name + tag] = out(a[name], c[name], terms[name].abs_sum, terms[name].k + D)
    return refs
