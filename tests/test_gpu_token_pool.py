"""Token mean pooling kernels (sc_token_pool_fwd / sc_token_pool_bwd) against float64.

Forward bound: |got - want| <= (n - 1) * 2^-24 * max|x| -- what any fp32 summation order of n terms stays within (n = 1: the
mean is the row, bit for bit); the bf16 output is the rounding of the fp32 output.  Backward: outputs pre-filled with NaN,
rows below t0 exact zeros, the others within one ulp of float32(d_mean) / n, the bf16 copy the rounding of the fp32 one.
Two runs give equal bits.  Shapes outside the contract raise and launch nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, L, d, t0, bf16 input).  Every B of {1, 3, 130}, L of {2, 3, 10, 50, 257, 577}, d of {64, 192, 768, 1280, 2048}, both t0 and
# both dtypes appear; L = 2 / t0 = 1 pools ONE token; B = 1 / L = 577 splits the tokens of one sample over the 16 waves of a single
# workgroup; d = 64 bf16 has 128 token phases per workgroup, d = 2048 fp32 two; B = 130, L = 257, d = 768 gives the backward 2080
# work items, more than its 2048 workgroups: the grid loops.
POINTS = [
    (1, 2, 64, 1, True), (3, 2, 192, 1, False), (1, 2, 2048, 1, True), (3, 3, 64, 0, False), (3, 3, 768, 1, True),
    (1, 10, 192, 1, True), (3, 10, 1280, 0, True), (130, 10, 64, 1, False), (3, 50, 768, 1, False), (1, 50, 2048, 0, False),
    (130, 50, 192, 1, True), (1, 257, 1280, 1, True), (3, 257, 768, 1, True), (3, 257, 2048, 1, False),
    (130, 50, 2048, 1, False), (1, 577, 64, 1, False), (1, 577, 768, 1, True), (1, 577, 1280, 0, False), (3, 577, 192, 1, True),
    (130, 257, 768, 1, True), (130, 3, 1280, 1, True),
]


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, ops
    return ops, _lib


def test_points_cover_every_value():
    for i, vals in enumerate(({1, 3, 130}, {2, 3, 10, 50, 257, 577}, {64, 192, 768, 1280, 2048}, {0, 1}, {True, False})):
        assert {p[i] for p in POINTS} == vals


@pytest.mark.parametrize("B,L,d,t0,xb", POINTS)
def test_token_pool_fwd_against_float64(B, L, d, t0, xb):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(B * 1000 + L + d + t0)
    x = torch.randn(B, L, d, generator=g).to(torch.bfloat16 if xb else torch.float32).cuda()
    n = L - t0
    want = x[:, t0:].double().mean(dim=1)
    outs = []
    for _ in range(2):
        mf = torch.full((B, d), float("nan"), device="cuda")
        mb = torch.full((B, d), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.token_pool_fwd(x, B, L, t0, d, mean_f32=mf, mean_bf16=mb)
        outs.append((mf, mb))
    mf, mb = outs[0]
    err = float((mf.double() - want).abs().max())
    bound = (n - 1) * 2.0 ** -24 * float(x[:, t0:].abs().max())
    print(f"B={B} L={L} d={d} t0={t0} bf16={xb}: max|d| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if n == 1:
        assert torch.equal(mf, x[:, t0].float())
    assert torch.equal(mb, mf.to(torch.bfloat16))
    assert torch.equal(outs[1][0], mf) and torch.equal(outs[1][1], mb)
    # each output alone gives the same bits
    only_b = torch.empty_like(mb)
    ops.token_pool_fwd(x, B, L, t0, d, mean_bf16=only_b)
    assert torch.equal(only_b, mb)


@pytest.mark.parametrize("B,L,d,t0,db", POINTS)
def test_token_pool_bwd_against_float64(B, L, d, t0, db):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(B * 1000 + L + d + t0 + 7)
    dm = torch.randn(B, d, generator=g).to(torch.bfloat16 if db else torch.float32).cuda()
    n = L - t0
    outs = []
    for _ in range(2):
        df = torch.full((B, L, d), float("nan"), device="cuda")
        dbf = torch.full((B, L, d), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.token_pool_bwd(dm, B, L, t0, d, dx_f32=df, dx_bf16=dbf)
        outs.append((df, dbf))
    df, dbf = outs[0]
    assert not bool(torch.isnan(df).any()) and not bool(torch.isnan(dbf.float()).any())      # every element was written
    if t0:
        assert bool((df[:, :t0] == 0).all()) and bool((dbf[:, :t0] == 0).all())
        assert not bool(torch.signbit(df[:, :t0]).any())
    want = (dm.float().double() / n)[:, None, :].expand(B, n, d)
    assert bool(((df[:, t0:].double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
    assert torch.equal(dbf, df.to(torch.bfloat16))
    assert torch.equal(outs[1][0], df) and torch.equal(outs[1][1], dbf)
    only_b = torch.full((B, L, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.token_pool_bwd(dm, B, L, t0, d, dx_bf16=only_b)
    assert torch.equal(only_b, dbf)


@pytest.mark.parametrize("L,d,t0", [(5, 6, 1), (5, 2052, 1), (5, 64, 5)])
def test_bad_shapes_raise_and_launch_nothing(L, d, t0):
    ops, _lib = _ops()
    B = 2
    x = torch.ones(B, L, d, device="cuda")
    mean = torch.full((B, d), 3.0, device="cuda")
    with pytest.raises(_lib.SpatialClipHipError, match="sc_token_pool_fwd"):
        ops.token_pool_fwd(x, B, L, t0, d, mean_f32=mean)
    dx = torch.full((B, L, d), 5.0, device="cuda")
    with pytest.raises(_lib.SpatialClipHipError, match="sc_token_pool_bwd"):
        ops.token_pool_bwd(mean, B, L, t0, d, dx_f32=dx)
    torch.cuda.synchronize()
    assert bool((mean == 3.0).all()) and bool((dx == 5.0).all())
