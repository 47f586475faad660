"""The tail split of the 256x256 NT GEMM: the partial last round of tiles runs as 128-row half tiles (sc_gemm8p.hip).

Every output element is still produced by one workgroup from the same K order through the same epilogue arithmetic, so every
check here is ``torch.equal``: against the exact fp32 product on small integers, or against the same call with the switch
off.  ``SC_GEMM_TAIL=<n>`` applies the rule with n workgroup slots, which makes a tail appear at a few hundred tiles;
``ops.gemm_last_tail`` says what the launcher did, so a shape that silently went to another kernel fails instead of passing
vacuously.  (NT launches whose area M*N is below 100 tiles' worth go to the 128x128 kernel: sc_gemm8p_try.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _rand(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def _tail_of_last_launch(ops):
    return ops.gemm_last_tail(reset=True)


# ---------------------------------------------------------------------------------------------------- 1. ring exactness
# (M, N, SC_GEMM_TAIL, expected (nfull, rem)).  The first two are the shapes as first specified: 13 x 8 = 104 tiles, but an
# area of 97 tiles' worth, which the launcher sends to the 128x128 kernel (expected None: nothing to say about the tail; the
# product must be exact all the same).  The last two are the same layout one tile row taller, so that the area passes the
# 100-tile threshold: 14 x 8 = 112 tiles, S = 96 -> nfull = 96, rem = 16, 32 half tiles = one interior tile row and the ragged
# 40-row one, whose second halves lie wholly beyond M.
RING_SHAPES = [(256 * 12 + 40, 256 * 8, 88, None), (256 * 12 + 40, 256 * 8 - 24, 88, None),
               (256 * 13 + 40, 256 * 8, 96, (96, 16)), (256 * 13 + 40, 256 * 8 - 24, 96, (96, 16))]


@pytest.mark.parametrize("M,N,slots,want", RING_SHAPES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448, 576, 1024])
def test_half_tile_ring_exact(monkeypatch, M, N, slots, want, K):
    """The half tile keeps four images in flight ahead of the reading phase in a nine-slot LDS ring (three K tiles of three
    images).  Small-integer operands make every fp32 sum exact, so a fragment read from a stale or half-landed slot cannot
    hide in a tolerance.  K sweeps 1..16 K tiles: prologue only, every remainder of the ring's three, ring wrap.  The output
    is prefilled with a sentinel: an element no workgroup wrote shows."""
    ops = _ops()
    monkeypatch.setenv("SC_GEMM_TAIL", str(slots))
    g = torch.Generator().manual_seed(K + N)
    for rep in range(3):
        a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16).cuda()
        b = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16).cuda()
        ref = a.float() @ b.float().t()                        # exact in fp32: |sum| <= 9 K
        o32 = torch.full((M, N), 5.5, dtype=torch.float32, device="cuda")
        _tail_of_last_launch(ops)
        ops.gemm(ops.NT, ops.EPI_F32, a, b, o32, M=M, N=N, K=K)
        got = _tail_of_last_launch(ops)
        if want is not None:
            assert got == want, (got, want)
        assert torch.equal(o32, ref), (K, rep)


# ---------------------------------------------------------------------------------- 2. bit-identity with the switch off
EPIS = ["BF16", "BF16_BIAS", "F32_BIAS_RES", "GELU_PAIR", "BF16_DGELU", "F32", "BF16_BIAS_RES", "GELU_GRAD_PAIR",
        "GELU_GRAD_PAIR/formula", "BF16_MUL_AUX", "BF16_MUL_AUX/colgroup3"]
_operands = {}


def _identity_operands():
    """Random bf16 operands of the bit-identity tests, made once.  13 x 9 = 117 tiles, ragged M (40 rows) and ragged N (64)."""
    if not _operands:
        M, N, K = 256 * 12 + 40, 256 * 8 + 64, 192
        g = torch.Generator().manual_seed(1234)
        _operands.update(M=M, N=N, K=K, a=_rand((M, K), g).cuda(), b=_rand((N, K), g, 0.15).cuda(),
                         bias=torch.randn(N, generator=g).cuda(), res32=torch.randn(M, N, generator=g).cuda(),
                         res16=_rand((M, N), g).cuda(), aux=_rand((M, N), g).cuda())
    return _operands


def _run_epi(ops, name, d):
    M, N, K = d["M"], d["N"], d["K"]
    epi = getattr(ops, "EPI_" + name)
    f32 = name in ("F32", "F32_BIAS_RES")
    out = torch.full((M, N), 9.0, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
    kw = {}
    if name in ("BF16_BIAS", "F32_BIAS_RES", "GELU_PAIR", "BF16_BIAS_RES", "GELU_GRAD_PAIR"):
        kw["bias"] = d["bias"]
    if name == "F32_BIAS_RES":
        kw["res"] = d["res32"]
    if name == "BF16_BIAS_RES":
        kw["res"] = d["res16"]
    if name in ("BF16_DGELU", "BF16_MUL_AUX"):
        kw["aux"] = d["aux"]
    out2 = None
    if name in ("GELU_PAIR", "GELU_GRAD_PAIR"):
        out2 = torch.full((M, N), 9.0, dtype=torch.bfloat16, device="cuda")
        kw["out2"] = out2
    ops.gemm_last_tail(reset=True)
    ops.gemm(ops.NT, epi, d["a"], d["b"], out, M=M, N=N, K=K, **kw)
    return out, out2, ops.gemm_last_tail(reset=True)


@pytest.mark.parametrize("case", EPIS)
def test_tail_split_is_bit_identical_for_every_epilogue(monkeypatch, case):
    """S = 104 on 117 tiles: rem = 13, 26 half tiles -- the ragged last tile row and four tiles of the row above, the ragged
    last tile column among them.  Same call with the switch off and on: every output tensor must hold the same bits (the
    sentinel included where nothing is written: there is no such place, and both runs prefill alike)."""
    ops = _ops()
    d = _identity_operands()
    name, _, variant = case.partition("/")
    if variant == "formula":
        monkeypatch.setenv("SC_GELU_LUT", "0")
    if variant == "colgroup3":
        monkeypatch.setenv("SC_GEMM_COLGROUP", f"{getattr(ops, 'EPI_' + name)}:3")
    monkeypatch.setenv("SC_GEMM_TAIL", "0")
    off, off2, t_off = _run_epi(ops, name, d)
    monkeypatch.setenv("SC_GEMM_TAIL", "104")
    on, on2, t_on = _run_epi(ops, name, d)
    assert t_off == (117, 0) and t_on == (104, 13), (t_off, t_on)
    assert torch.equal(off, on)
    if off2 is not None:
        assert torch.equal(off2, on2)
    assert not bool((on.float() == 9.0).all())


# ------------------------------------------------------------------------------------------------- 3. the rule itself
@pytest.mark.parametrize("slots,want", [(39, (117, 0)),        # rem = 0: 117 = 3 x 39
                                        (100, (100, 17)),       # split: 2 x 17 <= 100
                                        (60, (117, 0)),         # rem = 57: 2 x 57 > 60
                                        (117, (117, 0)),        # T <= n
                                        (200, (117, 0))])       # T < n
def test_rule_through_the_launcher(monkeypatch, slots, want):
    """What the launcher did for 117 tiles on n slots (ops.gemm_last_tail), and the result next to the switch-off result."""
    ops = _ops()
    d = _identity_operands()
    monkeypatch.setenv("SC_GEMM_TAIL", "0")
    off, _, t_off = _run_epi(ops, "BF16_BIAS", d)
    monkeypatch.setenv("SC_GEMM_TAIL", str(slots))
    on, _, t_on = _run_epi(ops, "BF16_BIAS", d)
    assert t_off == (117, 0) and t_on == want, (t_off, t_on)
    assert t_on == ops.gemm_tail_rule(117, slots)
    assert torch.equal(off, on)


def test_split_k_launch_keeps_its_tiles(monkeypatch):
    """Split-K launches are outside the rule: exact, and no half tiles, whatever the switch says."""
    ops = _ops()
    monkeypatch.setenv("SC_GEMM_TAIL", "5")
    M, N, K = 1024, 768, 64 * 6
    g = torch.Generator().manual_seed(6)
    a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16).cuda()
    b = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16).cuda()
    o32 = torch.full((M, N), 5.5, dtype=torch.float32, device="cuda")
    ops.gemm_last_tail(reset=True)
    ops.gemm(ops.NT, ops.EPI_F32, a, b, o32, M=M, N=N, K=K, splitk=3)
    assert ops.gemm_last_tail(reset=True) == (36, 0)
    assert torch.equal(o32, a.float() @ b.float().t())


# -------------------------------------------------------------------------------------- 4. one launch at the real rule
def test_default_rule_with_the_device_cu_count(monkeypatch):
    """SC_GEMM_TAIL unset: the rule with the device's CU count.  95 x 3 = 285 tiles: rem = 29 and 58 half tiles on 256 CUs."""
    ops = _ops()
    M, N, K = 256 * 95, 768, 256
    g = torch.Generator().manual_seed(95)
    a, b = _rand((M, K), g).cuda(), _rand((N, K), g, 0.1).cuda()
    bias = torch.randn(N, generator=g).cuda()
    res = _rand((M, N), g).cuda()
    outs, tails = [], []
    for sw in ("0", None):
        if sw is None:
            monkeypatch.delenv("SC_GEMM_TAIL", raising=False)
        else:
            monkeypatch.setenv("SC_GEMM_TAIL", sw)
        o = torch.full((M, N), 9.0, dtype=torch.bfloat16, device="cuda")
        ops.gemm_last_tail(reset=True)
        ops.gemm(ops.NT, ops.EPI_BF16_BIAS_RES, a, b, o, M=M, N=N, K=K, bias=bias, res=res)
        tails.append(ops.gemm_last_tail(reset=True))
        outs.append(o)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tails[0] == (285, 0) and tails[1] == ops.gemm_tail_rule(285, cus), (tails, cus)
    if cus == 256:
        assert tails[1] == (256, 29)
    assert torch.equal(outs[0], outs[1])
