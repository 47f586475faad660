"""LayerNorm, L2-norm and column-sum kernels (spatial-clip_amd/csrc/sc_norm.hip) at every width the towers use and at the
row counts where their slots, caps and tails change, against PyTorch in float64 on the CPU (tests/_refbounds.py states
every bound and its derivation).

Case ids name the code path: NV = float4 slots per lane of the kernel instance (1, 2, 3, 4 or 8), the fill of those slots
(d / 256: 1.25 means the second slot is a quarter full), the cap class of the backward's partial-sum slots (1280 for
d <= 768, 1024 above), ``lds>48K`` where the backward needs the hipFuncSetAttribute opt-in (d > 1365) and ``over-nominal``
where the row count exceeds the nominal slots, so that a grid capped at the resident blocks leaves slots to the zero-fill.
Every workspace is filled with NaN before a call and every output with a sentinel, so that a slot left unwritten, a row
skipped or a padding column read shows as a failure, not as a stale value that happens to be right."""
import pytest
import torch

from tests import _refbounds as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -1000.0          # output sentinel (exact in bf16 and fp32; far outside every value these tests produce)
P = R.LN_SPARSE_P
TS = 16.0               # the per-tensor e4m3 scale handed to the t8 forms


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _e4m3(q8):
    return q8.cpu().view(torch.float8_e4m3fn).double()


def _check_e4m3_rows(name, q8, sinv, ref64):
    """Per-row e4m3 copy of a value the test only sees through its float64 reference (test_gpu_fp8.py's forward rule): the
    row scale is a power of two that puts the row maximum in the top binade of e4m3, and the dequantised value lies within
    e4m3's half ulp (2^-4 relative) of the reference, or its smallest subnormal."""
    sinv = sinv.cpu().double()
    s = 1.0 / sinv
    assert torch.equal(torch.log2(s).round(), torch.log2(s)), name
    top = ref64.abs().amax(1) * s
    assert bool((top <= 448.0 * 1.001).all()) and bool((top > 224.0 * 0.999).all()), name
    back = _e4m3(q8) * sinv[:, None]
    assert bool(((back - ref64).abs() <= ref64.abs() * 2.0 ** -4 + (sinv * 2.0 ** -9)[:, None] + 1e-5).all()), name


def _check_e4m3_exact(name, q8, sinv, val):
    """Per-row e4m3 copy of fp32 values the kernel also wrote (test_gpu_fp8.py's backward rule): same bits as torch's e4m3fn
    rounding of value * scale, the scale a power of two with the row maximum in (224, 448]."""
    s = 1.0 / sinv.cpu()
    top = val.abs().amax(1) * s
    assert bool((top <= 448.0).all()) and bool((top > 224.0).all()), name
    want = (val * s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q8.cpu(), want), name


def _amax_slots(absval, rows):
    """Per-tensor amax slots as ln_t8_amax fills them: slot s holds the maximum over rows r with r & 63 == s (0 if none)."""
    want = torch.zeros(64, dtype=absval.dtype)
    rmax = absval.amax(1)
    for s in range(min(rows, 64)):
        want[s] = rmax[s::64].max()
    return want


# ---------------------------------------------------------------------------------------------------------- LayerNorm forward
@pytest.mark.parametrize("rows,d", R.LN_CASES, ids=[R.ln_case_id(*c) for c in R.LN_CASES])
def test_layernorm_forward_forms(rows, d):
    """Every forward entry point (fp32 rows, bf16 rows, + per-row e4m3, + per-tensor e4m3, padded row strides) on one input:
    y (bf16 rule), mean and rstd (reference-relative), the e4m3 copies, and sentinels in the padding of strided rows."""
    ops = _ops()
    dev = _dev()
    x, gamma, beta, _, _ = R.ln_inputs(rows, d)
    refs = R.ln_fwd_refs(x, gamma, beta)
    ry, rm, rr = (R.Ref(*refs[k]) for k in ("y", "mean", "rstd"))
    xd, x16, gd, bd = x.to(dev), x.bfloat16().to(dev), gamma.to(dev), beta.to(dev)
    ratios = []

    def outs(ldy=d):
        return (torch.full((rows, ldy), SENT, dtype=torch.bfloat16, device=dev), torch.full((rows,), SENT, device=dev),
                torch.full((rows,), SENT, device=dev))

    def check(tag, y, m, r):
        torch.cuda.synchronize()
        ratios.extend([R.check_bf16(f"{tag} y", y, ry), R.check_f32(f"{tag} mean", m, rm), R.check_f32(f"{tag} rstd", r, rr)])

    for tag, xin in (("fp32", xd), ("x16", x16)):
        y, m, r = outs()
        ops.layernorm_fwd(xin, gd, bd, y, m, r, rows, d)
        check(tag, y, m, r)
        y, m, r = outs()
        q8 = torch.full((rows, d), 0x7F, dtype=torch.uint8, device=dev)
        sinv = torch.full((rows,), SENT, device=dev)
        ops.layernorm_fwd(xin, gd, bd, y, m, r, rows, d, q8=q8, q8_scale_inv=sinv)
        check(f"{tag}+q8", y, m, r)
        _check_e4m3_rows(f"{tag}+q8 e4m3", q8, sinv, ry.r64)
        # strided rows: padding of 4..64 floats; the input's padding is NaN (read = poisoned row), the output's must survive
        padx, pady = 4 * (1 + d % 16), 4 * (1 + (d // 4 + 7) % 16)
        xs = torch.full((rows, d + padx), NAN, dtype=xin.dtype, device=dev)
        xs[:, :d] = xin
        y, m, r = outs(d + pady)
        ops.layernorm_fwd(xs, gd, bd, y, m, r, rows, d, ldx=d + padx, ldy=d + pady)
        check(f"{tag} ldx={d + padx} ldy={d + pady}", y[:, :d], m, r)
        assert bool((y[:, d:] == SENT).all()), "row padding of the output overwritten"
    # bf16 rows + per-row e4m3 + per-tensor e4m3 (delayed scale TS, 64 amax slots)
    y, m, r = outs()
    q8 = torch.full((rows, d), 0x7F, dtype=torch.uint8, device=dev)
    sinv = torch.full((rows,), SENT, device=dev)
    t8 = (torch.full((rows, d), 0x7F, dtype=torch.uint8, device=dev), torch.full((1,), TS, device=dev),
          torch.zeros(64, device=dev))
    ops.layernorm_fwd(x16, gd, bd, y, m, r, rows, d, q8=q8, q8_scale_inv=sinv, t8=t8)
    check("x16+q8+t8", y, m, r)
    _check_e4m3_rows("x16+q8+t8 e4m3", q8, sinv, ry.r64)
    back = _e4m3(t8[0]) / TS
    assert bool(((back - ry.r64).abs() <= ry.r64.abs() * 2.0 ** -4 + 2.0 ** -9 / TS + 1e-5).all()), "t8 copy"
    want = _amax_slots(ry.r64.abs(), rows)
    slack = R.REF_FACTOR * ry.e32 + R.ulp(want, torch.float32)
    assert bool(((t8[2].cpu().double() - want).abs() <= slack).all()), "t8 amax slots"
    print(f"[ln fwd {R.ln_case_id(rows, d)}] max ratio {max(ratios):.3g}")


# ---------------------------------------------------------------------------------------------------------- LayerNorm backward
def _backward_forms(d):
    """(tag, accumulate, options) of every backward entry point the ops wrapper exposes.  A form with write_f32 = 0 runs
    after its twin with write_f32 = 1 (``twin``: the same kernel instance and grid, write_f32 is a runtime flag): the twin's
    fp32 gradient is the exact set of terms both runs add into colsum, and their other outputs must agree bit for bit."""
    forms = [
        ("fp32 acc=False", False, dict(xb16=False)),
        ("fp32 acc=True", True, dict(xb16=False)),
        (f"fp32 acc=-{P}", -P, dict(xb16=False)),
        ("g16 write_f32=1", True, dict(xb16=False, g16=True, write_f32=True)),
        ("g16 write_f32=0", True, dict(xb16=False, g16=True, write_f32=False, twin="g16 write_f32=1")),
        (f"x16 g16 acc=-{P} write_f32=1", -P, dict(xb16=True, g16=True, write_f32=True)),
        (f"x16 g16 acc=-{P} write_f32=0", -P, dict(xb16=True, g16=True, write_f32=False, twin=f"x16 g16 acc=-{P} write_f32=1")),
        ("x16", True, dict(xb16=True)),
        ("q8", True, dict(xb16=False, q8=True)),
        ("x16_t8", True, dict(xb16=True, g16=True, write_f32=True, q8=True, t8=True)),
        ("defer_reduce", True, dict(xb16=False, defer=True)),
    ]
    # SC_LN_BWD_LEAN (ln_bwd_launch): the register-lean row bodies (bf16 rows + bf16 gradient stream) exist at NV = 3 and 4.
    # 0 never selects them; 3 selects them at d = 768 and 1024; 4 selects the NV = 4 body only (at d = 768 it is the plain
    # body, the same as 0, so it runs at d = 1024 alone).
    if d == 768:
        forms += [("lean=0 (plain body)", True, dict(xb16=True, g16=True, write_f32=True, lean="0")),
                  ("lean=3 (NV=3 lean body)", True, dict(xb16=True, g16=True, write_f32=True, lean="3"))]
    if d == 1024:
        forms += [("lean=0 (plain body)", True, dict(xb16=True, g16=True, write_f32=True, lean="0")),
                  ("lean=3 (NV=4 lean body)", True, dict(xb16=True, g16=True, write_f32=True, lean="3")),
                  ("lean=4 (NV=4 lean body)", True, dict(xb16=True, g16=True, write_f32=True, lean="4"))]
    return forms


@pytest.mark.parametrize("rows,d", R.LN_CASES, ids=[R.ln_case_id(*c) for c in R.LN_CASES])
def test_layernorm_backward_forms(rows, d, monkeypatch):
    """Every backward entry point on one input, against the float64 gradient formed on the kernel's own mean / rstd: the fp32
    gradient (reference-relative), its bf16 copy (bf16 rule), dgamma / dbeta / colsum (derived chain bound), the e4m3
    copies (bits of the fp32 values written), buffers that must not be written (NaN survives), the deferred reduction on a
    side stream and the lean bodies through SC_LN_BWD_LEAN."""
    ops = _ops()
    dev = _dev()
    monkeypatch.delenv("SC_LN_BWD_LEAN", raising=False)
    x, gamma, beta, dy, gin = R.ln_inputs(rows, d)
    xd, x16, gd, bd = x.to(dev), x.bfloat16().to(dev), gamma.to(dev), beta.to(dev)
    dyd, gind = dy.to(dev), gin.to(dev)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    ops.layernorm_fwd(xd, gd, bd, torch.empty((rows, d), dtype=torch.bfloat16, device=dev), mean, rstd, rows, d)
    bwd = R.ln_bwd_refs(dy, x, mean.cpu(), rstd.cpu(), gamma, beta)
    dres_refs = {mode: R.Ref(*R.ln_dres_ref(bwd, gin, mode)) for mode in (False, True, -P)}
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    k = R.ln_colsum_chain(rows, d, n_cu)
    nws = ops.layernorm_bwd_ws_floats(rows, d)
    ratios = []
    runs = {}

    def run(tag, mode, xb16=False, g16=False, write_f32=True, q8=False, t8=False, defer=False, lean=None, twin=None):
        if lean is not None:
            monkeypatch.setenv("SC_LN_BWD_LEAN", lean)
        ref = dres_refs[mode]
        inc = R.ln_incoming(gin, mode)
        # the fp32 buffer: the incoming gradient where the form reads it, NaN where it must not be read
        dres = torch.full((rows, d), NAN, device=dev)
        if not g16 and mode is True:
            dres.copy_(inc)
        elif mode not in (True, False):
            dres[::-mode] = inc[::-mode].to(dev)
        dres_in = dres.clone()
        gout = torch.full((rows, d), SENT, dtype=torch.bfloat16, device=dev)
        dg, db, cs = (torch.full((d,), SENT, device=dev) for _ in range(3))
        kw = {}
        if q8:
            kw.update(q8=torch.full((rows, d), 0x7F, dtype=torch.uint8, device=dev),
                      q8_scale_inv=torch.full((rows,), SENT, device=dev))
        if t8:
            kw["t8"] = (torch.full((rows, d), 0x7F, dtype=torch.uint8, device=dev), torch.full((1,), TS, device=dev),
                        torch.zeros(64, device=dev))
        if defer:
            kw.update(ws=torch.full((nws,), NAN, device=dev), defer_reduce=True)
        else:
            ops.workspace(nws, dev, "ln").fill_(NAN)
        if g16:
            kw.update(g16=True, g_in=gind if mode is True else None, write_f32=write_f32)
        ops.layernorm_bwd(dyd, x16 if xb16 else xd, mean, rstd, gd, dres, gout, dg, db, cs, rows, d, accumulate=mode, **kw)
        if defer:
            torch.cuda.synchronize()
            assert bool((dg == SENT).all()) and bool((db == SENT).all()) and bool((cs == SENT).all()), "reduced too early"
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.layernorm_bwd_reduce(kw["ws"], dg, db, cs, rows, d)
            torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if lean is not None:
            monkeypatch.delenv("SC_LN_BWD_LEAN")
        gout, dg, db, cs = gout.cpu(), dg.cpu(), db.cpu(), cs.cpu()
        if write_f32:
            terms = dres.cpu()
            ratios.append(R.check_f32(f"{tag} dres", terms, ref))
        else:
            assert torch.equal(dres.isnan(), dres_in.isnan()) and torch.equal(dres.nan_to_num(), dres_in.nan_to_num()), \
                f"{tag}: fp32 buffer written"
            tw = runs[twin]
            for name, a, b in (("dres_bf16", gout, tw[1]), ("dgamma", dg, tw[2]), ("dbeta", db, tw[3]), ("colsum", cs, tw[4])):
                assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                                   b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)), \
                    f"{tag}: {name} differs from the write_f32 = 1 run of the same kernel"
            terms = tw[0]
        runs[tag] = (terms, gout, dg, db, cs)
        ratios.append(R.check_bf16(f"{tag} dres_bf16", gout, ref))
        # dgamma terms dy * x_hat carry three roundings of their own (x - mean, * rstd, * dy): k + 3; dbeta terms are the
        # exact bf16 dy: k.  colsum adds exactly the fp32 gradient the kernel wrote (ac += o, sc_norm.hip:316 and :229):
        # its float64 sum is the reference, k the bound (the gradient itself is held to the element rule above).
        ratios.append(R.check_sum(f"{tag} dgamma", dg, bwd["dgamma"], bwd["dgamma_abs"], k + 3))
        ratios.append(R.check_sum(f"{tag} dbeta", db, bwd["dbeta"], bwd["dbeta_abs"], k))
        t64 = terms.double()
        ratios.append(R.check_sum(f"{tag} colsum", cs, t64.sum(0), t64.abs().sum(0), k))
        if q8:
            _check_e4m3_exact(f"{tag} e4m3", kw["q8"], kw["q8_scale_inv"], dres.cpu())
        if t8:
            val = dres.cpu()
            assert torch.equal(kw["t8"][0].cpu(), (val * TS).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
            assert torch.equal(kw["t8"][2].cpu(), _amax_slots(val.abs(), rows)), f"{tag}: amax slots"

    for tag, mode, opt in _backward_forms(d):
        run(tag, mode, **opt)
    print(f"[ln bwd {R.ln_case_id(rows, d)}] k = {k}, max ratio {max(ratios):.3g}")


# ---------------------------------------------------------------------------------------------------------- L2 norm
@pytest.mark.parametrize("rows,d", R.L2_CASES, ids=[f"d{d}-r{r}" + ("-zero_row" if r > 1 else "") + ("-width_not_multiple_of_64" if d % 64 else "")
                                                   for r, d in R.L2_CASES])
def test_l2norm_fwd_bwd(rows, d):
    """sc_l2norm_fwd / _bwd against F.normalize (eps 1e-12) in float64 and its autograd: y and inv (reference-relative), the
    bf16 y and dx (bf16 rule).  The all-zero row gives y = 0 and dx = dy * 1e12, as F.normalize does; it is checked on its
    own (its dx is 1e12 times larger than every other row's and would swamp E32)."""
    ops = _ops()
    dev = _dev()
    x, dy, zero = R.l2_inputs(rows, d)
    refs = R.l2_refs(x, dy)
    keep = torch.ones(rows, dtype=torch.bool)
    if zero is not None:
        keep[zero] = False
    ry, rinv, rdx = (R.Ref(refs[k][0][keep], refs[k][1][keep]) for k in ("y", "inv", "dx"))
    y = torch.full((rows, d), SENT, device=dev)
    ybf = torch.full((rows, d), SENT, dtype=torch.bfloat16, device=dev)
    inv = torch.full((rows,), SENT, device=dev)
    ops.l2norm_fwd(x.to(dev), y, ybf, inv, rows, d)
    dx = torch.full((rows, d), SENT, dtype=torch.bfloat16, device=dev)
    ops.l2norm_bwd(dy.to(dev), y, inv, dx, rows, d)
    torch.cuda.synchronize()
    y, ybf, inv, dx = y.cpu(), ybf.cpu(), inv.cpu(), dx.cpu()
    ratios = [R.check_f32("y", y[keep], ry), R.check_bf16("y_bf16", ybf[keep], ry), R.check_f32("inv", inv[keep], rinv),
              R.check_bf16("dx", dx[keep], rdx)]
    if zero is not None:
        assert bool((y[zero] == 0).all()) and bool((ybf[zero] == 0).all())
        want = dy[zero].double() * 1e12
        assert bool(((dx[zero].double() - want).abs() <= R.ulp(want, torch.bfloat16)).all()), "zero row: dx = dy * 1e12"
        assert float(inv[zero]) == float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1e-12, dtype=torch.float32))
    print(f"[l2norm d{d} r{rows}] max ratio {max(ratios):.3g}")


# ---------------------------------------------------------------------------------------------------------- column sums
COLSUM_CASES = [(1, 4, 4), (63, 100, 104), (16385, 768, 768), (50432, 768, 776)]


@pytest.mark.parametrize("rows,n,ld", COLSUM_CASES,
                         ids=[f"r{r}-n{n}-ld{ld}-slices{R.colsum_slices(r)}" + ("-slice_cap" if (r + 63) // 64 > 256 else "")
                              + ("-padded" if ld > n else "") for r, n, ld in COLSUM_CASES])
def test_colsum_bf16(rows, n, ld):
    """sc_colsum_bf16 against the float64 column sums (derived chain bound): the cached workspace is poisoned with NaN, the
    padding columns of the rows hold NaN (read into a sum = NaN), and the output past n keeps its sentinel."""
    ops = _ops()
    dev = _dev()
    g = torch.Generator().manual_seed(rows + n)
    x = (torch.randn(rows, n, generator=g) + 0.5).bfloat16()
    xs = torch.full((rows, ld), NAN, dtype=torch.bfloat16)
    xs[:, :n] = x
    from spatial_clip_amd import _lib
    ops.workspace(_lib.lib().sc_colsum_ws_floats(rows, n), dev, "colsum").fill_(NAN)
    out = torch.full((n + 8,), SENT, device=dev)
    ops.colsum_bf16(xs.to(dev), rows, n, out[:n], ld=ld)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[n:] == SENT).all())
    ratio = R.check_sum("colsum", out[:n], x.double().sum(0), x.double().abs().sum(0), R.colsum_chain(rows))
    print(f"[colsum r{rows} n{n} ld{ld}] k = {R.colsum_chain(rows)}, ratio {ratio:.3g}")
