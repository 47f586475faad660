"""The bf16 share cap of tests/_refbounds.py is a condition on the inputs, not a measurement of a kernel: on the exact seeds
and shapes of tests/test_gpu_norm_sweep.py, PyTorch's fp32 CPU reference rounded to bf16 must itself differ from
bf16(float64 value) on at most SHARE_CAP of the elements of every tensor.  A cap that the reference alone breaks is caught
here, without a GPU.  (The derived bounds need no such check: they bound the kernel's own arithmetic, and the float64
reference is far more precise than they require.)"""
import pytest
import torch

from tests import _refbounds as R


def _assert_share(name, ref64, ref32):
    share = R.bf16_share(ref32.to(torch.bfloat16), ref64)
    print(f"  {name}: fp32 reference bf16 share {share:.3g}")
    assert share <= R.SHARE_CAP, f"{name}: the fp32 reference alone breaks the share cap ({share} > {R.SHARE_CAP})"


@pytest.mark.parametrize("rows,d", R.LN_CASES, ids=[R.ln_case_id(*c) for c in R.LN_CASES])
def test_layernorm_reference_meets_the_share_cap(rows, d):
    """Forward y, and the bf16 residual gradient of every accumulate mode (on the fp32 reference's mean / rstd, standing in
    for the kernel's)."""
    x, gamma, beta, dy, gin = R.ln_inputs(rows, d)
    fwd = R.ln_fwd_refs(x, gamma, beta)
    _assert_share("y", *fwd["y"])
    bwd = R.ln_bwd_refs(dy, x, fwd["mean"][1], fwd["rstd"][1], gamma, beta)
    for mode in (False, True, -R.LN_SPARSE_P):
        _assert_share(f"dres acc={mode}", *R.ln_dres_ref(bwd, gin, mode))


@pytest.mark.parametrize("rows,d", R.L2_CASES, ids=[f"d{d}-r{r}" for r, d in R.L2_CASES])
def test_l2norm_reference_meets_the_share_cap(rows, d):
    """y and dx of F.normalize, without the all-zero row (checked on its own by the GPU test)."""
    x, dy, zero = R.l2_inputs(rows, d)
    refs = R.l2_refs(x, dy)
    keep = torch.ones(rows, dtype=torch.bool)
    if zero is not None:
        keep[zero] = False
    for k in ("y", "dx"):
        _assert_share(k, refs[k][0][keep], refs[k][1][keep])


def test_ulp_and_chain_helpers():
    """The helpers the bounds are built from: fp32 / bf16 spacing, the colsum chain at the row-slice cap."""
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0], dtype=torch.float64)
    assert torch.equal(R.ulp(v, torch.float32), torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -22],
                                                               dtype=torch.float64))
    assert torch.equal(R.ulp(v, torch.bfloat16), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6],
                                                                dtype=torch.float64))
    assert R.colsum_slices(16385) == 256 and R.colsum_slices(63) == 1
    assert R.ln_nominal_blocks(6304, 768) == 1280 and R.ln_nominal_blocks(5140, 1280) == 1024
    assert R.ln_nv(1280) == 8 and R.ln_nv(320) == 2 and R.ln_nv(4) == 1
