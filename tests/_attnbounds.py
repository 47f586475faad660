"""Float64 references, inputs, rounding-point model and error bounds of the attention sweep (tests/test_gpu_attention_sweep.py)
and of its CPU-side check (tests/test_cpu_attention_bounds.py).  CPU only: importing this module needs neither a GPU nor
the HIP library.  The element rules (``REF_FACTOR``, ``ulp``, ``check_f32``, ``check_sum``) are those of tests/_refbounds.py.

References (no project kernel involved), on exactly the bf16 values the kernel receives, widened exactly; the softmax scale
is the fp32 value 1.0f / sqrtf(dh) the dispatcher passes (sc_attention.hip, ``scale``):

* ``ref64``: out, lse and d(qkv) of ``sum(out[:q_rows] * dout[:q_rows])`` by PyTorch autograd in float64, causal or not.
* ``delta``: rowsum(dO * O) in float64 on the bf16 ``out`` the backward kernel was given.

Rounding-point model (``model_fwd`` / ``model_bwd``): the same computation in PyTorch fp32 with the roundings every MFMA
attention kernel here has: P to bf16 before P V and P^T dO, dS to bf16 before dS K and dS^T Q, fp32 accumulation, bf16
results.  Its error against float64 is what bf16 attention costs on those inputs; it comes from the references alone.

Bounds:

* bf16 outputs (out, dQ, dK, dV), per element: ``|got - r64| <= ulp_bf16(|r64|) + REF_FACTOR * E_row``, E_row the model's
  largest error on that row (one token, one head's dh-slice): a sharp row or a row with few causal keys does not inherit
  the slack of a diffuse one.
  For the gradients the allowance has a third, derived term, ``fp32_floor``: the fp32 rounding of dP - delta where the two
  cancel exactly, and the GPU's flush of values below the smallest normal number; neither shows in a PyTorch model on a CPU.
* lse (fp32): ``check_f32`` against float64 with PyTorch's fp32 logsumexp of fp32 scores as the fp32 reference.
* delta (fp32): ``check_sum`` with k = dh and abs_sum = sum |dO * O|: any order of a dh-term fp32 dot product has at most dh
  roundings per chain.

The backward is tested on the model's own forward results (``model_fwd``: bf16 out, fp32 lse), not on a forward kernel's:
the backward kernel and the model then start from identical values, and E_row owes nothing to the code under test.  Rows
>= q_rows of that out / lse are NaN (a forward call leaves them unwritten: a backward kernel must not read them).
"""
import functools
import math

import torch

from tests._refbounds import REF_FACTOR, Ref, check_f32, check_sum, ulp

BF = torch.bfloat16
LOG2E = 1.4426950408889634

# lengths that end a 16- / 32- / 64-row tile or exceed one by a token, the path thresholds (224 / 257 / 288 / 320) and the
# project's model lengths (77, 197, 257)
BOUNDARY_LENGTHS = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77, 197, 223, 224, 225, 256, 257, 258, 288, 289, 304, 305, 319,
                    320]
STREAM_LONG_LENGTHS = (list(range(321, 331)) + [383, 384, 385, 447, 448, 449, 511, 512, 513, 575, 576, 577, 578, 640, 785,
                                                1023, 1024, 1025, 1370])
FAMILIES = ("diffuse", "mixed", "peaked")
MAXL = 320                                            # sc_attn_common.h:10


def q_rows_at(L: int):
    """q_rows values of the sweep at a boundary length: 1, around one 16-row tile, and all rows but the last."""
    return sorted({r for r in (1, 15, 16, 17, L - 1) if 1 <= r < L})


def scale_f32(dh: int) -> float:
    """1.0f / sqrtf((float)dh), as sc_attn_fwd / sc_attn_bwd compute it."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(dh), dtype=torch.float32).sqrt())


# ---------------------------------------------------------------------------------------------------------- layouts
def split_heads(qkv: torch.Tensor, B: int, L: int, H: int, dh: int):
    """q, k, v as [B, H, L, dh] views of the packed [B*L, 3*H*dh] rows."""
    x = qkv.view(B, L, 3, H, dh).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads(t: torch.Tensor, B: int, L: int, H: int, dh: int) -> torch.Tensor:
    """[B*L, H*dh] -> [B, H, L, dh]."""
    return t.view(B, L, H, dh).transpose(1, 2)


def grad_heads(dqkv: torch.Tensor, B: int, L: int, H: int, dh: int) -> torch.Tensor:
    """[B*L, 3*H*dh] -> [3 (dQ, dK, dV), B, H, L, dh]."""
    return dqkv.view(B, L, 3, H, dh).permute(2, 0, 3, 1, 4)


def allowed_keys(L: int, causal: bool, shift: int = 0, drop_last: bool = False) -> torch.Tensor:
    """[L, L] bool: may query i see key j.  ``shift`` moves the causal diagonal (mutants; row 0 keeps its own key),
    ``drop_last`` hides key L - 1 (mutants)."""
    i = torch.arange(L).view(-1, 1)
    j = torch.arange(L).view(1, -1)
    ok = torch.ones(L, L, dtype=torch.bool)
    if causal:
        ok = j <= (i + shift).clamp_min(0)
    if drop_last and L > 1:
        ok = ok & (j < L - 1)
    return ok


# ---------------------------------------------------------------------------------------------------------- inputs
def _peaked(g, B, L, H, dh, causal):
    """The construction of test_long_attention_large_scores_peak_in_last_tile at any L and dh: scaled scores span roughly
    -45 .. +70 and every row's maximum is at the last key it may see.  Non-causal: q = a u + noise, k = 4 noise, key L - 1
    = a u (u a unit vector, a^2 / sqrt(dh) = 72).  Causal: the peak has to move with the row, so q_i = a e_i + noise and
    k_j = a e_j + noise, e_i unit vectors of random Fourier features of the position (e_i . e_j is 1 on the diagonal and
    about 1 / sqrt(dh) rms off it)."""
    a = math.sqrt(72.0 * math.sqrt(dh))
    if not causal:
        u = torch.full((dh,), 1.0 / math.sqrt(dh))
        q = a * u + torch.randn(B, L, H, dh, generator=g)
        k = 4.0 * torch.randn(B, L, H, dh, generator=g)
        k[:, L - 1] = a * u
    else:
        w = math.pi * torch.rand(dh // 2, generator=g)
        ph = torch.arange(L).view(-1, 1) * w
        e = (torch.cat([ph.cos(), ph.sin()], 1) / math.sqrt(dh // 2)).view(1, L, 1, dh)
        q = a * e + torch.randn(B, L, H, dh, generator=g)
        k = a * e + torch.randn(B, L, H, dh, generator=g)
    return q, k


def peak_property(qkv, B, L, H, dh, causal) -> bool:
    """Every row's largest score is at the last key the row may see (key L - 1, or the diagonal when causal)."""
    q, k, _ = split_heads(qkv.double(), B, L, H, dh)
    s = q @ k.transpose(-1, -2)
    s = s.masked_fill(~allowed_keys(L, causal), -math.inf)
    want = torch.arange(L) if causal else torch.full((L,), L - 1)
    return bool((s.argmax(-1) == want).all())


@functools.lru_cache(maxsize=8)
def inputs(family: str, dh: int, L: int, causal: bool, B: int = 2, H: int = 3):
    """(qkv bf16 [B*L, 3*H*dh], dout bf16 [B*L, H*dh]) of a family, seeded from (dh, L, causal).

    diffuse: unit randn.  mixed: the query rows scaled by logspace(-1, 0.7) along the sequence (sharp and flat rows in one
    head), V with a fixed per-feature offset of order 1 (a wrong softmax denominator then shows in out).  peaked: see
    ``_peaked``; the first seed of the sequence seed, seed + 1, ... whose bf16 inputs have the peak property is taken."""
    seed = 7919 * L + 104729 * dh + (1 if causal else 0) + 31 * FAMILIES.index(family)
    for attempt in range(16):
        g = torch.Generator().manual_seed(seed + 1000003 * attempt)
        d = H * dh
        v = torch.randn(B, L, H, dh, generator=g)
        if family == "diffuse":
            q = torch.randn(B, L, H, dh, generator=g)
            k = torch.randn(B, L, H, dh, generator=g)
        elif family == "mixed":
            q = torch.randn(B, L, H, dh, generator=g) * torch.logspace(-1, 0.7, L).view(1, L, 1, 1)
            k = torch.randn(B, L, H, dh, generator=g)
            v = v + torch.linspace(-1.5, 1.5, dh)
        else:
            q, k = _peaked(g, B, L, H, dh, causal)
        qkv = torch.cat([q.reshape(B * L, d), k.reshape(B * L, d), v.reshape(B * L, d)], 1).to(BF)
        dout = torch.randn(B * L, d, generator=g).to(BF)
        if family != "peaked" or peak_property(qkv, B, L, H, dh, causal):
            return qkv, dout
    raise AssertionError(f"no seed gives the peak property at dh={dh} L={L} causal={causal}")


# ---------------------------------------------------------------------------------------------------------- float64 reference
def ref64(qkv, dout, B, L, H, dh, causal, q_rows=0, want_grads=True):
    """(out [B,H,L,dh], lse [B,H,L], d(qkv) [3,B,H,L,dh]) in float64 by autograd; rows >= q_rows of out / lse are computed too
    (the caller compares the first q_rows only), the loss takes the first q_rows query rows."""
    nq = q_rows if 0 < q_rows < L else L
    x = qkv.double().requires_grad_(want_grads)
    q, k, v = split_heads(x, B, L, H, dh)
    s = (q @ k.transpose(-1, -2)) * scale_f32(dh)
    s = s.masked_fill(~allowed_keys(L, causal), -math.inf)
    lse = torch.logsumexp(s, -1)
    out = torch.softmax(s, -1) @ v
    if not want_grads:
        return out, lse, None
    (out[:, :, :nq] * heads(dout, B, L, H, dh).double()[:, :, :nq]).sum().backward()
    return out.detach(), lse.detach(), grad_heads(x.grad, B, L, H, dh)


def lse_ref32(qkv, B, L, H, dh, causal):
    """PyTorch fp32 logsumexp of fp32 scores: the fp32 reference of the lse rule."""
    q, k, _ = split_heads(qkv.float(), B, L, H, dh)
    s = (q @ k.transpose(-1, -2)) * scale_f32(dh)
    return torch.logsumexp(s.masked_fill(~allowed_keys(L, causal), -math.inf), -1)


# ---------------------------------------------------------------------------------------------------------- the formulas by hand
def _bf(x, on):
    return x.to(BF).to(x.dtype) if on else x


def manual_fwd(qkv, B, L, H, dh, causal, dtype, rounded, mut=None):
    """out, lse [B,H,L(,dh)] in ``dtype`` by the textbook two-pass formula.  ``rounded``: the model's rounding points (P =
    exp(s - max) to bf16 before P V, the row sum from the unrounded fp32 P, the result to bf16).  ``mut``: a mutant of the
    mathematics (tests/test_cpu_attention_bounds.py)."""
    q, k, v = split_heads(qkv.to(dtype), B, L, H, dh)
    scale = scale_f32(dh) * (1.03 if mut == "scale" else 1.0)
    drop = mut == "drop_last" or (mut == "drop_stray" and L % 16 == 1)
    shift = {"mask+1": 1, "mask-1": -1}.get(mut, 0)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed_keys(L, causal, shift, drop), -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    lsum = p.sum(-1, keepdim=True)
    out = _bf((_bf(p, rounded) @ v) / lsum, rounded)
    lse = (m + torch.log(lsum)).squeeze(-1)
    if mut == "stale_max":
        lse = lse + 1e-3
    return out, lse


def manual_bwd(qkv, out, dout, lse, B, L, H, dh, causal, q_rows, dtype, rounded, mut=None):
    """(d(qkv) [3,B,H,L,dh], delta [B,H,L]) in ``dtype`` from out / lse [B,H,L(,dh)] (rows >= q_rows are never read) and the
    packed dout.  ``rounded``: P to bf16 before P^T dO, dS to bf16 before dS K and dS^T Q, bf16 results."""
    nq = q_rows if 0 < q_rows < L else L
    if mut == "ignore_q_rows":
        nq = L
    q, k, v = split_heads(qkv.to(dtype), B, L, H, dh)
    do = heads(dout, B, L, H, dh).to(dtype)
    scale = scale_f32(dh) * (1.03 if mut == "scale" else 1.0)
    drop = mut == "drop_last" or (mut == "drop_stray" and L % 16 == 1)
    shift = {"mask+1": 1, "mask-1": -1}.get(mut, 0)
    live = (torch.arange(L) < nq).view(L, 1)
    ok = allowed_keys(L, causal, shift, drop) & live
    s = (q @ k.transpose(-1, -2)) * scale
    lse_ = torch.where(live.view(L), lse.to(dtype), torch.zeros((), dtype=dtype)).unsqueeze(-1)
    p = torch.where(ok, torch.exp(s - lse_), torch.zeros((), dtype=dtype))
    o_ = torch.where(live, out.to(dtype), torch.zeros((), dtype=dtype))
    delta = (do * o_).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp if mut == "no_delta" else dp - delta)
    ds = torch.where(ok, ds, torch.zeros((), dtype=dtype))
    dv = _bf(p, rounded).transpose(-1, -2) @ torch.where(live, do, torch.zeros((), dtype=dtype))
    dq = (_bf(ds, rounded) @ k) * scale
    dk = (_bf(ds, rounded).transpose(-1, -2) @ q) * scale
    if mut == "zero_last_dkv":
        dk, dv = dk.clone(), dv.clone()
        dk[:, :, L - 1] = 0
        dv[:, :, L - 1] = 0
    return _bf(torch.stack([dq, dk, dv]), rounded), delta.squeeze(-1)


def model_fwd(qkv, B, L, H, dh, causal):
    """The rounding-point model's forward: (out bf16 [B,H,L,dh], lse fp32 [B,H,L])."""
    out, lse = manual_fwd(qkv, B, L, H, dh, causal, torch.float32, True)
    return out.to(BF), lse


def model_bwd(qkv, out, dout, lse, B, L, H, dh, causal, q_rows):
    return manual_bwd(qkv, out, dout, lse, B, L, H, dh, causal, q_rows, torch.float32, True)[0]


# ---------------------------------------------------------------------------------------------------------- a second emulation
def tiled_fwd(qkv, B, L, H, dh, causal, tile=64):
    """Flash-style forward in fp32: online softmax over ``tile``-key tiles in the exp2 domain, P to bf16 before P V, the
    accumulator rescaled when the running maximum moves.  (out bf16, lse fp32)."""
    q, k, v = split_heads(qkv.float(), B, L, H, dh)
    c2 = torch.tensor(scale_f32(dh), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    ok = allowed_keys(L, causal)
    m = torch.full((B, H, L, 1), -math.inf)
    lsum = torch.zeros(B, H, L, 1)
    acc = torch.zeros(B, H, L, dh)
    for j0 in range(0, L, tile):
        j1 = min(L, j0 + tile)
        s = (q @ k[:, :, j0:j1].transpose(-1, -2)) * c2
        s = s.masked_fill(~ok[:, j0:j1], -math.inf)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        safe = torch.where(torch.isinf(m_new), torch.zeros(()), m_new)       # a causal row before its first key
        alpha = torch.exp2(m - safe)
        p = torch.exp2(s - safe)
        lsum = lsum * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + p.to(BF).float() @ v[:, :, j0:j1]
        m = m_new
    out = (acc / lsum).to(BF)
    lse = ((m + torch.log2(lsum)) / torch.tensor(LOG2E, dtype=torch.float32)).squeeze(-1)
    return out, lse


def tiled_bwd(qkv, out, dout, lse, B, L, H, dh, causal, q_rows, tile=64):
    """Flash-style backward in fp32: P recomputed from lse tile by tile (exp2 domain), dQ summed over key tiles, dK / dV
    over query tiles, P and dS to bf16 before the products.  (d(qkv) bf16 [3,B,H,L,dh], delta fp32 [B,H,L])."""
    nq = q_rows if 0 < q_rows < L else L
    q, k, v = split_heads(qkv.float(), B, L, H, dh)
    do = heads(dout, B, L, H, dh).float()
    scale = torch.tensor(scale_f32(dh), dtype=torch.float32)
    c2 = scale * torch.tensor(LOG2E, dtype=torch.float32)
    ok = allowed_keys(L, causal)
    delta = torch.zeros(B, H, L)
    delta[:, :, :nq] = (do[:, :, :nq] * out[:, :, :nq].float()).sum(-1)
    nl2 = torch.zeros(B, H, L)
    nl2[:, :, :nq] = -lse[:, :, :nq] * torch.tensor(LOG2E, dtype=torch.float32)
    dq = torch.zeros(B, H, L, dh)
    dk = torch.zeros(B, H, L, dh)
    dv = torch.zeros(B, H, L, dh)
    for i0 in range(0, nq, tile):
        i1 = min(nq, i0 + tile)
        for j0 in range(0, L, tile):
            j1 = min(L, j0 + tile)
            live = ok[i0:i1, j0:j1]
            if not bool(live.any()):
                continue
            s = q[:, :, i0:i1] @ k[:, :, j0:j1].transpose(-1, -2)
            p = torch.where(live, torch.exp2(s * c2 + nl2[:, :, i0:i1, None]), torch.zeros(()))
            dp = do[:, :, i0:i1] @ v[:, :, j0:j1].transpose(-1, -2)
            ds = (p * (dp - delta[:, :, i0:i1, None])).to(BF).float()
            pb = p.to(BF).float()
            dv[:, :, j0:j1] += pb.transpose(-1, -2) @ do[:, :, i0:i1]
            dk[:, :, j0:j1] += ds.transpose(-1, -2) @ q[:, :, i0:i1]
            dq[:, :, i0:i1] += ds @ k[:, :, j0:j1]
    return torch.stack([dq * scale, dk * scale, dv]).to(BF), delta


def fp32_floor(qkv, dout, out64, lse64, B, L, H, dh, causal, nq):
    """Derived fp32 floors of dQ / dK / dV rows, [3, B, H, L]: two rounding points beyond the four bf16 ones, both far
    below E_row wherever a row's gradient is neither a pure cancellation nor below the normal range.

    * dS = P (dP - delta) subtracts two dh-term fp32 dot products that a kernel rounds separately (dP in the MFMA
      accumulator, delta in a lane sum: sc_attention.hip:437, ``pa * (p0[r] - sdel[qa])``), so where they cancel (a causal
      row with one key: dS is exactly zero) the difference keeps up to dh u (sum |dO V_j| + sum |dO O_i|) -- the
      ``check_sum`` chain rule -- while the PyTorch model, which happens to sum both in one order, shows no error at all.
      Carried through dS K and dS^T Q in float64.
    * The GPU flushes what lies below the smallest normal number T = 2^-126 (of fp32 and bf16 alike) to zero: P from the raw
      v_exp_f32 (sc_attn_common.h:171-173, ``fast_exp2``), bf16 P / dS operands of an MFMA, a bf16 result.  Each flushed P
      or dS moves a gradient by at most T times the factor it is multiplied with: T (1 + sum_i |dO_i|) for dV, T (1 + scale
      sum (1 + |dP - delta|) |Q or K|) for dK / dQ.  The peaked family has such gradients (keys 110 below the row maximum);
      a CPU keeps the denormals, so the model does not show it."""
    T = 2.0 ** -126
    scale = scale_f32(dh)
    q, k, v = split_heads(qkv.double(), B, L, H, dh)
    do = heads(dout, B, L, H, dh).double()
    live = (torch.arange(L) < nq).view(L, 1)
    ok = allowed_keys(L, causal) & live
    zero = torch.zeros((), dtype=torch.float64)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.where(ok, torch.exp(s - lse64.unsqueeze(-1)), zero)
    eps = dh * 2.0 ** -24 * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * out64.abs()).sum(-1, keepdim=True))
    w = p * eps
    f = torch.where(ok, 1.0 + (do @ v.transpose(-1, -2) - (do * out64).sum(-1, keepdim=True)).abs(), zero)
    dq = scale * (w @ k.abs()).amax(-1) + T * (1.0 + scale * (f @ k.abs()).amax(-1))
    dk = scale * (w.transpose(-1, -2) @ q.abs()).amax(-1) + T * (1.0 + scale * (f.transpose(-1, -2) @ q.abs()).amax(-1))
    dv = T * (1.0 + torch.where(live, do.abs(), zero).sum(2, keepdim=True).amax(-1).expand(B, H, L))
    return torch.stack([dq, dk, dv])


# ---------------------------------------------------------------------------------------------------------- one case's references
class Case:
    """References and allowances of one (family, dh, L, causal, q_rows, B, H): the inputs, the float64 results, the model's
    forward (the backward kernel's inputs ``out_in`` / ``lse_in``, packed, NaN in rows >= q_rows) and the per-row errors."""

    def __init__(self, family, dh, L, causal, q_rows=0, B=2, H=3, want_grads=True):
        self.family, self.dh, self.L, self.causal, self.B, self.H = family, dh, L, causal, B, H
        self.q_rows = q_rows if 0 < q_rows < L else 0
        self.nq = self.q_rows or L
        self.dims = (B, L, H, dh)
        self.qkv, self.dout = inputs(family, dh, L, causal, B, H)
        nq = self.nq
        self.out64, self.lse64, self.g64 = ref64(self.qkv, self.dout, B, L, H, dh, causal, self.q_rows, want_grads)
        self.m_out, self.m_lse = model_fwd(self.qkv, B, L, H, dh, causal)
        self.e_out = (self.m_out.double() - self.out64).abs().amax(-1)                      # [B,H,L]
        self.lse_ref = Ref(self.lse64[:, :, :nq], lse_ref32(self.qkv, B, L, H, dh, causal)[:, :, :nq])
        if want_grads:
            # what a forward call leaves for the backward: rows >= q_rows unwritten (NaN here)
            o = self.m_out.clone()
            l = self.m_lse.clone()
            o[:, :, nq:] = math.nan
            l[:, :, nq:] = math.nan
            self.out_in = o.transpose(1, 2).reshape(B * L, H * dh).contiguous()          # packed [B*L, H*dh]
            self.lse_in = l.contiguous()
            self.m_g = model_bwd(self.qkv, self.m_out, self.dout, self.m_lse, B, L, H, dh, causal, self.q_rows)
            self.e_g = (self.m_g.double() - self.g64).abs().amax(-1)                        # [3,B,H,L]
            self.floor_g = fp32_floor(self.qkv, self.dout, self.out64, self.lse64, B, L, H, dh, causal, nq)
            do = heads(self.dout, B, L, H, dh).double()[:, :, :nq]
            terms = do * self.m_out.double()[:, :, :nq]
            self.delta64, self.delta_abs = terms.sum(-1), terms.abs().sum(-1)

    def tag(self):
        return f"{self.family} dh{self.dh} L{self.L}{' causal' if self.causal else ''}" + \
            (f" q_rows{self.q_rows}" if self.q_rows else "")

    # ---- ratios (error / allowed); nothing asserted here: the callers collect
    def _rows(self, got, r64, e_row, floor=None):
        allowed = ulp(r64, BF) + REF_FACTOR * e_row.unsqueeze(-1)
        if floor is not None:
            allowed = allowed + floor.unsqueeze(-1)
        r = (got.double() - r64).abs() / allowed
        return math.nan if bool(torch.isnan(r).any()) else float(r.max()) if r.numel() else 0.0

    def ratio_out(self, out_heads):
        nq = self.nq
        return self._rows(out_heads[:, :, :nq], self.out64[:, :, :nq], self.e_out[:, :, :nq])

    def ratio_lse(self, lse):
        try:
            return check_f32("lse", lse[:, :, :self.nq], self.lse_ref)
        except AssertionError:
            r = (lse[:, :, :self.nq].double() - self.lse_ref.r64).abs() / self.lse_ref.allowed_f32()
            return math.nan if bool(torch.isnan(r).any()) else float(r.max())

    def ratio_grads(self, g_heads):
        """{dq, dk, dv: ratio}; dQ over the first q_rows rows (the rows behind them have the exact rule ``dq_tail``)."""
        nq = self.nq
        r = {"dq": self._rows(g_heads[0][:, :, :nq], self.g64[0][:, :, :nq], self.e_g[0][:, :, :nq], self.floor_g[0][:, :, :nq]),
             "dk": self._rows(g_heads[1], self.g64[1], self.e_g[1], self.floor_g[1]),
             "dv": self._rows(g_heads[2], self.g64[2], self.e_g[2], self.floor_g[2])}
        return r

    def dq_tail(self, g_heads, fill=None) -> bool:
        """dQ rows >= q_rows: all zero (the gradient), or, where the API does not promise that every element is written
        (``fill`` given), all still at the caller's fill."""
        t = g_heads[0][:, :, self.nq:]
        return bool((t == 0).all()) or (fill is not None and bool((t == fill).all()))

    def ratio_delta(self, delta):
        try:
            return check_sum("delta", delta[:, :, :self.nq], self.delta64, self.delta_abs, self.dh)
        except AssertionError as e:
            return float(str(e).split("= ")[1].split(" ")[0])

    def old_rule(self, out_heads=None, g_heads=None):
        """Worst |err| / (atol + rtol |ref|) under the rule the attention tests used before: 2e-2 on out, 4e-2 on d(qkv)."""
        worst = 0.0
        if out_heads is not None:
            r = self.out64[:, :, :self.nq]
            worst = max(worst, float(((out_heads[:, :, :self.nq].double() - r).abs() / (2e-2 + 2e-2 * r.abs())).max()))
        if g_heads is not None:
            worst = max(worst, float(((g_heads.double() - self.g64).abs() / (4e-2 + 4e-2 * self.g64.abs())).max()))
        return worst
