"""The stem kernels' "no LN" body (gamma == NULL; a tower built with no_ln_pre), full-length and with kept patches, both stream
dtypes, at the shapes of the stem tests of tests/test_gpu_patch_dropout.py.

Forward: the row is ``patch_out + pos`` (row 0: ``cls + pos[0]``), one fp32 add -- bit-equal to torch's fp32 add, and to its
``.to(bfloat16)`` for the bf16 stream; statistics buffers are not touched.  Backward: ``dres`` stays as it is, ``dpatch`` is
the bf16 rounding of its rows t > 0, ``dpos`` / ``dcls`` are fixed-order batch sums."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops, patch_dropout as pd
    return ops, pd


def _dev(a):
    return torch.as_tensor(a).cuda()


def _close(a, b):
    """|a - b| <= 1e-5 |b| + 1e-6 max|b|: two fp32 summation orders of the same terms (tests/test_gpu_patch_dropout.py)."""
    return bool(((a - b).abs() <= 1e-5 * b.abs() + 1e-6 * b.abs().max()).all())


def _forced_keep(B, n, K):
    """Explicit rows: patch 0 kept by every sample, patch n - 1 by none."""
    rows = [[0] + sorted(((7 * b + 3 * t) % (n - 2)) + 1 for t in range(K - 1)) for b in range(B)]
    keep = np.array(rows, dtype=np.int32)
    assert (np.diff(keep, axis=1) > 0).all() and keep.max() < n - 1
    return keep


@pytest.mark.parametrize("d", [64, 192, 768, 1280, 2048])
@pytest.mark.parametrize("Lk", [2, 9, 50])
@pytest.mark.parametrize("x16", [False, True])
def test_no_ln_forward_is_one_fp32_add(d, Lk, x16):
    ops, pd = _pkg()
    B, n = 3, 60
    L, K = n + 1, Lk - 1
    g = torch.Generator().manual_seed(d + Lk)
    patch_out = torch.randn(B * n, d, generator=g).cuda()
    cls, pos = torch.randn(d, generator=g).cuda(), torch.randn(L, d, generator=g).cuda()
    xd = torch.bfloat16 if x16 else torch.float32
    want = torch.cat([cls.expand(B, 1, d), patch_out.view(B, n, d)], dim=1) + pos          # fp32, one add per element
    x = torch.full((B * L, d), float("nan"), dtype=xd, device="cuda")
    mean, rstd = torch.full((B * L,), -7.0, device="cuda"), torch.full((B * L,), -9.0, device="cuda")
    ops.embed_ln_fwd(patch_out, cls, pos, None, None, x, mean, rstd, B, L, d)
    assert torch.equal(x, want.view(B * L, d).to(xd))
    assert bool((mean == -7.0).all()) and bool((rstd == -9.0).all())
    # kept rows equal the full kernel's rows
    keep = pd.keep_indices_host(d, Lk, 0, B, n, K)
    kl = torch.from_numpy(keep).long()
    prow = (torch.arange(B)[:, None] * n + kl).reshape(-1).cuda()
    trow = torch.cat([torch.arange(B)[:, None] * L, torch.arange(B)[:, None] * L + 1 + kl], 1).reshape(-1).cuda()
    xk = torch.full((B * Lk, d), float("nan"), dtype=xd, device="cuda")
    ops.embed_ln_fwd(patch_out[prow].contiguous(), cls, pos, None, None, xk, None, None, B, Lk, d, keep=_dev(keep))
    assert torch.equal(xk, x[trow])


@pytest.mark.parametrize("B,Lk,d,forced", [(1, 9, 192, False), (3, 9, 768, False), (90, 50, 64, False), (3, 6, 1280, True),
                                           (2, 4, 2048, False)])
def test_no_ln_backward_full_and_keep(B, Lk, d, forced):
    """B = 90, L' = 50: 4500 rows = 1125 row groups, more than the 1024 workgroups of the persistent row loop.  d = 2048: the
    width at which the LayerNorm body needs the raised dynamic-LDS limit (the "no LN" body uses no LDS)."""
    ops, pd = _pkg()
    n = 60
    K = Lk - 1
    g = torch.Generator().manual_seed(B + d)
    cls, pos = torch.randn(d, generator=g).cuda(), torch.randn(n + 1, d, generator=g).cuda()
    # ---- full length at L = Lk tokens (its own positions table of Lk rows)
    L = Lk
    patch_out = torch.randn(B * (L - 1), d, generator=g).cuda()
    dx = torch.randn(B * L, d, generator=g).cuda()
    outs = []
    for _ in range(2):
        dres = dx.clone()
        dpatch = torch.full((B * (L - 1), d), float("nan"), dtype=torch.bfloat16, device="cuda")
        dpos, dcls = torch.full((L, d), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
        ops.embed_ln_bwd(dres, patch_out, cls, pos[:L].contiguous(), None, None, None, dpatch, None, None, dpos, dcls, B, L, d)
        outs.append((dres, dpatch, dpos, dcls))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    dres, dpatch, dpos, dcls = outs[0]
    assert torch.equal(dres, dx)
    assert torch.equal(dpatch, dx.view(B, L, d)[:, 1:].reshape(-1, d).to(torch.bfloat16))
    want = dx.view(B, L, d).double().sum(0)
    assert _close(dpos.double(), want) and _close(dcls.double(), want[0]) and torch.equal(dcls, dpos[0])
    # ---- kept patches: L = Lk tokens of the n + 1 positions
    keep = _forced_keep(B, n, K) if forced else pd.keep_indices_host(d, B, 0, B, n, K)
    slot = pd.slots_from_keep(keep, n)
    outs = []
    for _ in range(2):
        dres = dx.clone()
        dpatch = torch.full((B * K, d), float("nan"), dtype=torch.bfloat16, device="cuda")
        dpos, dcls = torch.full((n + 1, d), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
        ops.embed_ln_bwd(dres, patch_out, cls, pos, None, None, None, dpatch, None, None, dpos, dcls, B, Lk, d,
                         keep=_dev(keep), slot=_dev(slot))
        outs.append((dres, dpatch, dpos, dcls))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    dres, dpatch, dpos, dcls = outs[0]
    assert torch.equal(dres, dx)
    assert torch.equal(dpatch, dx.view(B, Lk, d)[:, 1:].reshape(-1, d).to(torch.bfloat16))
    want = torch.zeros(n + 1, d, dtype=torch.float64)
    dx64 = dx.view(B, Lk, d).double().cpu()
    want[0] = dx64[:, 0].sum(0)
    for b in range(B):
        want[1 + torch.from_numpy(keep[b]).long()] += dx64[b, 1:]
    assert _close(dpos.double().cpu(), want) and torch.equal(dcls, dpos[0])
    never = sorted(set(range(n)) - set(keep.reshape(-1).tolist()))
    if forced:
        assert n - 1 in never and bool((slot[:, 0] == 0).all())
    for j in never:
        assert float(dpos[1 + j].abs().max()) == 0.0          # exact zeros where no sample kept the patch
