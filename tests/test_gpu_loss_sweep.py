"""Every kernel of spatial-clip_amd/csrc/sc_loss.hip called directly (``ops.*`` on a synthetic similarity matrix) and compared
with float64 at the shapes where its branches change: one-wave rows, partial blocks, 256 k +- 1, finalize loops over more than
256 rows, the distillation kernel's register slots and its resident / streamed straddle, every structure of the tile-id join.
Cases, references and bounds: tests/_losscases.py (its CPU-side check: tests/test_cpu_loss_reference.py).

Every output buffer is poisoned (NaN, or -7777 for integers) before the call and followed by 64 guard elements that must keep
their poison.  The backward tests feed the kernel its own forward outputs; the reference is taken at those values.  Each test
prints ``name: ratio`` lines (kernel error / allowed error) and one ``[loss-sweep]`` summary line."""
import math

import pytest
import torch

from tests import _losscases as L

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
INT_POISON = -7777


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, ops
    return ops, _lib


def _buf(shape, dtype=torch.float32, src=None):
    """(view, whole): a poisoned device buffer of ``shape`` followed by GUARD poisoned elements; ``src`` fills the payload (an
    input the kernel overwrites in place, or the start value of an accumulator)."""
    n = math.prod(shape)
    whole = torch.full((n + GUARD,), NAN if dtype.is_floating_point else INT_POISON, dtype=dtype, device="cuda")
    view = whole[:n].view(shape)
    if src is not None:
        view.copy_(torch.as_tensor(src, dtype=dtype).reshape(shape))
    return view, whole


def _guards_kept(*wholes):
    for w in wholes:
        g = w[-GUARD:]
        assert bool(torch.isnan(g).all() if w.dtype.is_floating_point else (g == INT_POISON).all()), "guard elements overwritten"


def _dev(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def _done(family, cid, ratios):
    name = max(ratios, key=lambda k: ratios[k])
    print(f"[loss-sweep] {family} {cid}: worst ratio {ratios[name]:.3g} ({name})")


def _check_all(refs, got):
    assert set(refs) == set(got), (sorted(refs), sorted(got))
    return {name: L.check(name, got[name], refs[name]) for name in refs}


# ---------------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("c", L.JOIN_CASES, ids=[L.join_case_id(c) for c in L.JOIN_CASES])
def test_neighbor_join_labels(c):
    ops, _ = _ops()
    img, txt, nbr, alpha, a_scale, _tags = L.join_inputs(c)
    col, col_w = _buf((2, c.B, c.K + 1), torch.int32)
    w, w_w = _buf((2, c.B, c.K + 1))
    ops.neighbor_join(img.cuda(), txt.cuda(), nbr.cuda(), alpha.cuda(), c.B, c.G, c.K, c.rank, a_scale, col, w)
    torch.cuda.synchronize()
    col64, w64 = L.join_sparse(img, txt, nbr, alpha, c.B, c.G, c.K, c.rank, a_scale, torch.float64)
    assert torch.equal(col.cpu(), col64)                                    # columns exactly (last column wins, skips, -1)
    assert not bool(torch.isnan(w).any())
    assert bool((w.cpu()[col64 < 0] == 0).all())
    q64 = L.dense_labels(col64, w64, c.G)
    ratios = {"label weights": L.check_sum("label weights", w.cpu(), w64, w64.abs(), c.K + 2),
              "dense labels": L.check_sum("dense labels", L.dense_labels(col.cpu(), w.cpu(), c.G), q64, q64.abs(), c.K + 2)}
    _guards_kept(col_w, w_w)
    _done("neighbor_join", L.join_case_id(c), ratios)


@pytest.mark.parametrize("B,rank", [(1, 0), (3, 2), (255, 1), (256, 0), (257, 3), (513, 1)])
def test_onehot_labels(B, rank):
    ops, _ = _ops()
    col, col_w = _buf((2, B, 1), torch.int32)
    w, w_w = _buf((2, B, 1))
    ops.onehot_labels(B, rank, col, w)
    torch.cuda.synchronize()
    assert torch.equal(col.cpu().view(2, B), (rank * B + torch.arange(B, dtype=torch.int32)).expand(2, B))
    assert bool((w == 1.0).all())
    _guards_kept(col_w, w_w)


def test_neighbor_join_refuses_64_neighbours_and_writes_nothing():
    """The kernel's s_col[2][64] / s_w[64] hold K <= 63 entries plus nothing else: K = 64 is refused by the host check, before
    any launch."""
    ops, _lib = _ops()
    B, G, K = 3, 65, 64
    ids = torch.arange(G, dtype=torch.int64, device="cuda")
    nbr = torch.zeros((B, K), dtype=torch.int64, device="cuda")
    alpha = torch.ones((B, K), device="cuda")
    col = torch.full((2, B, K + 1), 5, dtype=torch.int32, device="cuda")
    w = torch.full((2, B, K + 1), 3.0, device="cuda")
    with pytest.raises(_lib.SpatialClipHipError, match="sc_neighbor_join"):
        ops.neighbor_join(ids, ids, nbr, alpha, B, G, K, 0, 0.5, col, w)
    torch.cuda.synchronize()
    assert bool((col == 5).all()) and bool((w == 3.0).all())


# ---------------------------------------------------------------------------------------------------------- ClipLoss / SpatialLoss
def _run_fwd(ops, c, z, col, w):
    zd, cold, wd = z.cuda(), col.cuda(), w.cuda()
    rowstats, rs_w = _buf((2 * c.B, 4))
    loss_out, lo_w = _buf((4,))
    bias = None if c.bias is None else _dev(c.bias)
    ops.contrastive_loss_fwd(zd, c.B, c.G, _dev(c.scale), c.cap or 0.0, bias, cold, wd, c.K + 1, c.w, rowstats, loss_out)
    torch.cuda.synchronize()
    assert torch.equal(zd.cpu(), z)                                         # the forward leaves z alone
    _guards_kept(rs_w, lo_w)
    return cold, wd, bias, rowstats, loss_out


@pytest.mark.parametrize("c", L.LOSS_CASES, ids=[L.loss_case_id(c) for c in L.LOSS_CASES])
def test_contrastive_loss_fwd(c):
    ops, _ = _ops()
    z, col, w, s, b = L.loss_inputs(c)
    _, _, _, rowstats, loss_out = _run_fwd(ops, c, z, col, w)
    refs = L.clip_fwd_refs(z, col, w, s, b, c.w)
    rs, lo = rowstats.cpu(), loss_out.cpu()
    got = {"lse": rs[:, 0], "E_p[z]": rs[:, 1], "sum q*logit": rs[:, 2], "sum q*z": rs[:, 3],
           "loss": lo[0], "gap": lo[1], "CE_image": lo[2], "CE_text": lo[3]}
    _done("contrastive_loss_fwd", L.loss_case_id(c), _check_all(refs, got))


@pytest.mark.parametrize("c", L.LOSS_CASES, ids=[L.loss_case_id(c) for c in L.LOSS_CASES])
def test_contrastive_loss_bwd(c):
    ops, _ = _ops()
    z, col, w, s, b = L.loss_inputs(c)
    cold, wd, bias, rowstats, loss_out = _run_fwd(ops, c, z, col, w)
    dz, dz_w = _buf((2, c.B, c.G), src=z)
    rowgrad, rg_w = _buf((2 * c.B, 2))
    ds, ds_w = _buf((2,))
    go = None if c.go is None else _dev(c.go)
    ops.contrastive_loss_bwd(dz, c.B, c.G, _dev(c.scale), c.cap or 0.0, bias, cold, wd, c.K + 1, c.w, rowstats, loss_out, go,
                             rowgrad, ds[0:1], ds[1:2])
    torch.cuda.synchronize()
    refs = L.clip_bwd_refs(z, col, w, s, b, c.w, c.go, rowstats, loss_out)
    rg = rowgrad.cpu()
    got = {"dz": dz.cpu(), "rowgrad sum dl*z": rg[:, 0], "rowgrad sum dl": rg[:, 1], "d_scale": ds.cpu()[0], "d_bias": ds.cpu()[1]}
    ratios = _check_all(refs, got)
    _guards_kept(dz_w, rg_w, ds_w)
    _done("contrastive_loss_bwd", L.loss_case_id(c), ratios)


# ---------------------------------------------------------------------------------------------------------- SigLIP
@pytest.mark.parametrize("i,c", list(enumerate(L.SIG_CASES)), ids=[L.sig_case_id(c) for c in L.SIG_CASES])
def test_siglip_loss(i, c):
    ops, _ = _ops()
    z = L.z_matrix(c.vals, 1, c.B, c.G, c.rank * c.B, 4)[0]
    s, b, col0 = L.f32(c.scale), 0.0 if c.bias is None else L.f32(c.bias), c.rank * c.B
    dz, dz_w = _buf((c.B, c.G), src=z)
    rowpart, rp_w = _buf((c.B, 3))
    tot, tot_w = _buf((3,))
    init = (i % 3, 2, 5)
    hits, hits_w = _buf((3,), torch.int32, src=init) if i % 2 else (None, None)      # every other case also counts recall
    ops.siglip_loss(dz, c.B, c.G, col0, _dev(c.scale), None if c.bias is None else _dev(c.bias), rowpart, tot[0:1], tot[1:2],
                    tot[2:3], hits)
    torch.cuda.synchronize()
    refs = L.siglip_refs(z, s, b, col0)
    rp, t = rowpart.cpu(), tot.cpu()
    got = {"dz": dz.cpu(), "rowpart sum loss": rp[:, 0], "rowpart sum dl*z": rp[:, 1], "rowpart sum dl": rp[:, 2],
           "loss": t[0], "d_scale": t[1], "d_bias": t[2]}
    ratios = _check_all(refs, got)
    _guards_kept(dz_w, rp_w, tot_w)
    if hits is not None:                                    # read from z before it was overwritten with dz
        assert hits.cpu().tolist() == L.recall_ref(z, c.B, col0, init)
        _guards_kept(hits_w)
    _done("siglip_loss", L.sig_case_id(c), ratios)


# ---------------------------------------------------------------------------------------------------------- distillation
@pytest.mark.parametrize("i,c", list(enumerate(L.DIST_CASES)), ids=[L.dist_case_id(c) for c in L.DIST_CASES])
def test_distill_loss(i, c):
    ops, _ = _ops()
    assert ops.distill_resident_max_g() == L.RESIDENT_MAX_G          # the straddle of the case list sits where the kernel's does
    zs, zt, s, st = L.distill_inputs(c)
    col0 = c.rank * c.B
    dzc, dzc_w = _buf((2, c.B, c.G), src=zs)
    dzd, dzd_w = _buf((2, c.B, c.G), src=zt)
    rowpart, rp_w = _buf((2 * c.B, 4))
    loss_out, lo_w = _buf((4,))
    ds, ds_w = _buf((2,))
    init = (1, i % 4, 0)
    hits, hits_w = _buf((3,), torch.int32, src=init) if i % 2 else (None, None)
    ops.distill_loss(dzc, dzd, c.B, c.G, col0, _dev(c.scale), _dev(c.tscale), rowpart, loss_out, ds[0:1], ds[1:2], hits)
    torch.cuda.synchronize()
    refs = L.distill_refs(zs, zt, s, st, col0)
    rp, lo = rowpart.cpu(), loss_out.cpu()
    got = {"dz_c": dzc.cpu(), "dz_d": dzd.cpu(), "rowpart CE": rp[:, 0], "rowpart D": rp[:, 1], "rowpart sum dl_c*z": rp[:, 2],
           "rowpart sum dl_d*z": rp[:, 3], "contrastive": lo[0], "distill": lo[1], "CE_image": lo[2], "CE_text": lo[3],
           "d_scale_c": ds.cpu()[0], "d_scale_d": ds.cpu()[1]}
    ratios = _check_all(refs, got)
    _guards_kept(dzc_w, dzd_w, rp_w, lo_w, ds_w)
    if hits is not None:
        assert hits.cpu().tolist() == L.recall_ref(zs[0], c.B, col0, init)
        _guards_kept(hits_w)
    _done("distill_loss", L.dist_case_id(c), ratios)


# ---------------------------------------------------------------------------------------------------------- recall
@pytest.mark.parametrize("c", L.RECALL_CASES, ids=[L.recall_case_id(c) for c in L.RECALL_CASES])
def test_recall_hits(c):
    """The counters as integers, onto their start values; where the window is the whole matrix, the same counters through
    siglip_loss and distill_loss, which must read z before they overwrite it."""
    ops, _ = _ops()
    z = L.recall_inputs(c)
    want = L.recall_ref(z[c.row0:], c.n, c.col0, c.init)
    zd = z.cuda()
    hits, hits_w = _buf((3,), torch.int32, src=c.init)
    ops.recall_hits(zd[c.row0:], c.G, c.n, c.col0, hits)
    torch.cuda.synchronize()
    print(f"  recall hits {hits.cpu().tolist()} (reference {want}, start {list(c.init)})")
    assert hits.cpu().tolist() == want
    assert torch.equal(zd.cpu(), z)
    _guards_kept(hits_w)
    if c.row0 == 0 and c.rows == c.n:
        h1, h1_w = _buf((3,), torch.int32, src=c.init)
        ops.siglip_loss(zd.clone(), c.n, c.G, c.col0, _dev(14.2857), _dev(-10.0), torch.empty((c.n, 3), device="cuda"), None,
                        None, None, h1)
        h2, h2_w = _buf((3,), torch.int32, src=c.init)
        zs = torch.stack([zd, zd.flip(0)]).contiguous()                     # only the image rows z_s[0] are ranked
        ops.distill_loss(zs, zs.clone(), c.n, c.G, c.col0, _dev(14.2857), _dev(25.0), torch.empty((2 * c.n, 4), device="cuda"),
                         torch.empty(4, device="cuda"), None, None, h2)
        torch.cuda.synchronize()
        assert h1.cpu().tolist() == want and h2.cpu().tolist() == want
        _guards_kept(h1_w, h2_w)


# ---------------------------------------------------------------------------------------------------------- PCC
@pytest.mark.parametrize("c", L.PCC_CASES, ids=[L.pcc_case_id(c) for c in L.PCC_CASES])
def test_pcc_rows(c):
    ops, _ = _ops()
    pb, tb = L.pcc_inputs(c)
    pred, tgt = pb.cuda()[:, :c.cols], tb.cuda()[:, :c.cols]                # row strides ldp / ldt
    pcc, pcc_w = _buf((c.rows,)) if c.want_pcc else (None, None)
    acc, acc_w = _buf((2,), src=c.init) if c.want_sum else (None, None)
    ops.pcc_rows(pred, tgt, pcc, acc)
    torch.cuda.synchronize()
    refs = L.pcc_refs(pb[:, :c.cols], tb[:, :c.cols], c.init)
    ratios = {}
    if pcc is not None:
        ratios["pcc"] = L.check("pcc", pcc.cpu(), refs["pcc"])
        assert float(pcc[0]) == 0.0                                         # the constant row scores an exact 0
        _guards_kept(pcc_w)
    if acc is not None:
        ratios["sum"] = L.check("sum", acc.cpu()[0], refs["sum"])
        assert float(acc[1]) == refs["count"]
        _guards_kept(acc_w)
    _done("pcc_rows", L.pcc_case_id(c), ratios)


# ---------------------------------------------------------------------------------------------------------- scalar helpers
@pytest.mark.parametrize("n", L.HELPER_N)
def test_scalar_helpers(n):
    """scale_by_scalar: bit-equal to x * s.  axpby_scalars: fa * a + fb * b with both products rounded, then added (the ``plain``
    order of _losscases.axpby_refs): asserted bitwise, and within the roundings of any evaluation order of the exact value."""
    ops, _ = _ops()
    a, b = L.helper_vectors(n)
    fa, fb = L.f32(-2.5), L.f32(0.3)
    out, out_w = _buf((n,))
    ops.scale_by_scalar(a.cuda(), _dev(fa), out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), a * torch.tensor(fa))
    _guards_kept(out_w)
    out, out_w = _buf((n,))
    ops.axpby_scalars(a.cuda(), _dev(fa), b.cuda(), _dev(fb), out)
    torch.cuda.synchronize()
    r, got = L.axpby_refs(a, b, fa, fb), out.cpu()
    same = {k: bool(torch.equal(got, r[k])) for k in ("plain", "fma_a", "fma_b")}
    print(f"  axpby_scalars n={n}: bit-equal to {same}")
    assert bool(((got.double() - r["exact"]).abs() <= r["slack"]).all())
    assert same["plain"]
    _guards_kept(out_w)


def test_exp_scalar_and_its_backward():
    ops, _ = _ops()
    x = torch.tensor(L.EXP_X, dtype=torch.float32)
    ys = []
    for v in x.tolist():
        y, y_w = _buf((1,))
        ops.exp_scalar(_dev(v), y)
        torch.cuda.synchronize()
        _guards_kept(y_w)
        ys.append(float(y))
    L.check_f32("exp_scalar", torch.tensor(ys, dtype=torch.float32), L.Ref(torch.exp(x.double()), torch.exp(x)))
    for y, dy, mult in ((14.2857, -0.37, 1.0), (100.0, 2.5e-3, 0.5), (1.0, 7.0, -3.0)):
        dx, dx_w = _buf((1,))
        ops.exp_scalar_bwd(_dev(y), _dev(dy), dx, mult)
        torch.cuda.synchronize()
        t = lambda v: torch.tensor(v, dtype=torch.float32)                                  # noqa: E731
        assert float(dx) == float((t(dy) * t(y)) * t(mult))                 # (dy * y) * mult, each product rounded to fp32
        _guards_kept(dx_w)


# ---------------------------------------------------------------------------------------------------------- wrapper refusals
def _valid_args(name):
    """Valid arguments of one wrapper at B = 3, G = 5, K = 2 (tensors pre-filled: floats 3.0 or small ids, ints 5)."""
    B, G, K = 3, 5, 2
    f = lambda *shape: torch.full(shape, 3.0, device="cuda")                                 # noqa: E731
    i32 = lambda *shape: torch.full(shape, 1, dtype=torch.int32, device="cuda")              # noqa: E731
    i64 = lambda *shape: torch.full(shape, 5, dtype=torch.int64, device="cuda")              # noqa: E731
    one = lambda: torch.ones(1, device="cuda")                                               # noqa: E731
    if name == "neighbor_join":
        return dict(all_img_ids=i64(G), all_txt_ids=i64(G), nbr_ids=i64(B, K), nbr_alpha=f(B, K), B=B, G=G, K=K, rank=0,
                    alpha_scale=0.5, lab_col=i32(2, B, K + 1), lab_w=f(2, B, K + 1))
    if name == "contrastive_loss_fwd":
        return dict(z=f(2, B, G), B=B, G=G, scale=one(), cap=0.0, bias=one(), lab_col=i32(2, B, K + 1), lab_w=f(2, B, K + 1),
                    nlab=K + 1, w=0.05, rowstats=f(2 * B, 4), loss_out=f(4))
    if name == "contrastive_loss_bwd":
        return dict(z=f(2, B, G), B=B, G=G, scale=one(), cap=0.0, bias=one(), lab_col=i32(2, B, K + 1), lab_w=f(2, B, K + 1),
                    nlab=K + 1, w=0.05, rowstats=f(2 * B, 4), loss_out=f(4), grad_out=one(), rowgrad=f(2 * B, 2), dscale=f(1),
                    dbias=f(1))
    if name == "recall_hits":
        return dict(z_img_rows=f(B, G), G=G, B=B, col0=2, hits3=i32(3))
    if name == "siglip_loss":
        return dict(z=f(B, G), B=B, G=G, col0=2, scale=one(), bias=one(), rowpart=f(B, 3), loss_out=f(1), dscale=f(1), dbias=f(1),
                    hits3=i32(3))
    raise ValueError(name)


def _spoil(t, how):
    if how == "short":
        return t.flatten()[:-1]
    if how == "dtype":
        return t.double() if t.dtype.is_floating_point else (t.long() if t.dtype == torch.int32 else t.int())
    if how == "strided":
        return torch.stack([t, t], -1)[..., 0]                              # the same shape, inner stride 2
    if how == "two":
        return torch.ones(2, device="cuda")
    if how == "cpu":
        return t.cpu()
    raise ValueError(how)


REFUSALS = [("neighbor_join", a, h) for a, h in (("lab_col", "short"), ("lab_w", "short"), ("lab_col", "dtype"), ("nbr_ids", "short"),
                                                 ("nbr_alpha", "dtype"), ("nbr_alpha", "short"), ("all_img_ids", "short"),
                                                 ("all_txt_ids", "dtype"), ("all_txt_ids", "strided"))] + \
           [("contrastive_loss_fwd", a, h) for a, h in (("rowstats", "short"), ("z", "short"), ("z", "dtype"), ("z", "strided"),
                                                        ("lab_col", "short"), ("lab_w", "dtype"), ("scale", "two"), ("bias", "two"),
                                                        ("loss_out", "short"), ("rowstats", "cpu"))] + \
           [("contrastive_loss_bwd", a, h) for a, h in (("rowgrad", "short"), ("rowstats", "short"), ("z", "short"), ("grad_out", "two"),
                                                        ("lab_w", "short"), ("rowgrad", "dtype"), ("dscale", "dtype"))] + \
           [("recall_hits", a, h) for a, h in (("hits3", "short"), ("hits3", "dtype"), ("z_img_rows", "short"), ("z_img_rows", "dtype"))] + \
           [("siglip_loss", a, h) for a, h in (("rowpart", "short"), ("z", "short"), ("z", "strided"), ("scale", "two"), ("bias", "two"),
                                               ("hits3", "dtype"), ("hits3", "short"))]


@pytest.mark.parametrize("name,arg,how", REFUSALS, ids=[f"{n}-{a}-{h}" for n, a, h in REFUSALS])
def test_wrappers_refuse_bad_arguments_before_any_launch(name, arg, how):
    """A wrong-sized, wrong-typed or strided tensor raises from the host-side check; every tensor keeps its prefill."""
    ops, _lib = _ops()
    args = _valid_args(name)
    args[arg] = _spoil(args[arg], how)
    before = {k: v.clone() for k, v in args.items() if torch.is_tensor(v)}
    # the Python-side check must be the one that refuses: its own exception type per kind of fault (a host tensor is the one
    # fault the shared _req helper reports as SpatialClipHipError)
    expected = {"short": ValueError, "strided": ValueError, "two": ValueError, "dtype": TypeError,
                "cpu": _lib.SpatialClipHipError}[how]
    with pytest.raises(expected) as err:
        getattr(ops, name)(**args)
    assert "sc_" not in str(err.value)              # not the C host check's message
    assert type(err.value) is expected
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(args[k], v), k


@pytest.mark.parametrize("name", ["neighbor_join", "contrastive_loss_fwd", "contrastive_loss_bwd", "recall_hits", "siglip_loss"])
def test_wrappers_accept_their_valid_arguments(name):
    """The arguments the refusal test spoils one at a time are accepted as they stand."""
    ops, _ = _ops()
    getattr(ops, name)(**_valid_args(name))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- head level
def _padded(t):
    """[G, D] features as a view of a [G, D + 4] buffer: the layout of the all-gather's receive buffer, read in place."""
    buf = torch.zeros(t.shape[0], t.shape[1] + 4, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("kind", ["clip", "spatial", "siglip", "distill"])
@pytest.mark.parametrize("B,G,rank,D", L.HEAD_SHAPES)
def test_head_against_float64_autograd(kind, B, G, rank, D):
    """contrastive_forward_backward in both modes, siglip_forward_backward and distill_forward_backward against float64 autograd
    of the same loss, gathered features read in place from padded buffers; ``late_all_image`` at the middle shape, ``join_local``
    at the single-process one."""
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import contrastive as C
    h = L.head_inputs(B, G, rank, D)
    s, b = L.f32(14.2857), (0.0 if kind == "distill" else L.f32(-1.0))
    sl = slice(rank * B, (rank + 1) * B)
    fi, ft = h["img"][sl].contiguous().cuda(), h["txt"][sl].contiguous().cuda()
    ai, at = _padded(h["img"]), _padded(h["txt"])
    refs = L.head_refs(kind, h, B, rank, s, b)
    if kind in ("clip", "spatial"):
        kw = dict(mode=kind, all_text=at, rank=rank, logit_bias=_dev(b))
        if kind == "spatial":
            kw.update(image_tile_ids=h["img_ids"][sl].cuda(), text_tile_ids=h["txt_ids"][sl].cuda(),
                      all_image_tile_ids=h["img_ids"].cuda(), all_text_tile_ids=h["txt_ids"].cuda(),
                      neighbor_tile_ids=h["nbr"].cuda(), neighbor_alphas=h["alpha"].cuda(), cap_logit_scale=L.CAP_BELOW,
                      temp_reg_weight=0.05, neighbor_alpha_scale=h["alpha_scale"])
        if G == 130:
            kw.update(late_all_image=lambda: ai)
        else:
            kw.update(all_image=ai)
        res = C.contrastive_forward_backward(fi, ft, _dev(s), **kw)
        got = {k: res[k] for k in refs}
    elif kind == "siglip":
        res = C.siglip_forward_backward(fi, ft, _dev(s), _dev(b), all_text=at, rank=rank)
        for k in ("d_text", "d_all_image"):                 # the text rows' own gradient arrives through d_all_text
            assert float(refs.pop(k).ref.r64.abs().max()) == 0.0
        got = {k: res[k] for k in refs}
    else:
        ti, tt = h["timg"][sl].contiguous().cuda(), h["ttxt"][sl].contiguous().cuda()
        res = C.distill_forward_backward(fi, ft, _dev(s), ti, tt, _dev(25.0), all_image=ai, all_text=at,
                                         dist_all_image=_padded(h["timg"]), dist_all_text=_padded(h["ttxt"]), rank=rank)
        got = {}
        for j, t in enumerate(("c", "d")):
            got.update({f"loss_{t}": res[("contrastive_loss", "distill_loss")[j]], f"d_image_{t}": res[f"d_image_{t}"],
                        f"d_text_{t}": res[f"d_text_{t}"], f"d_all_image_{t}": res[f"d_all_{t}"][:, :D],
                        f"d_all_text_{t}": res[f"d_all_{t}"][:, D:], f"d_scale_{t}": res[f"d_scale_{t}"]})
    torch.cuda.synchronize()
    ratios = _check_all(refs, {k: v.detach().cpu() for k, v in got.items()})
    if kind == "clip" and G == B:               # single process: the GEMMs add the gathered terms onto the direct ones
        res = C.contrastive_forward_backward(fi, ft, _dev(s), mode="clip", logit_bias=_dev(b), join_local=True)
        torch.cuda.synchronize()
        for loc, gath in (("d_image", "d_all_image"), ("d_text", "d_all_text")):
            o = L.out(refs[loc].ref.r64 + refs[gath].ref.r64, refs[loc].r32 + refs[gath].r32)
            ratios[loc + " joined"] = L.check(loc + " joined", res[loc].cpu(), o)
        ratios["loss joined"] = L.check("loss joined", res["loss"].cpu(), refs["loss"])
    _done(f"head {kind}", f"B{B}-G{G}-rank{rank}-D{D}", ratios)
