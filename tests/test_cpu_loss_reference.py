"""CPU-side check of tests/_losscases.py, the references and bounds of the loss-kernel sweep (tests/test_gpu_loss_sweep.py).

The float64 references restate the losses in closed form (the forms the kernels implement), so they are pinned here against
three independent statements of the same losses: the oracle (oracle/spatial_clip_oracle.py) run in float64 with autograd,
the distillation oracle (tests/_distill_oracle.py) and the committed goldens (outputs of the reference implementation, fp32).
The label references are held to the oracle's ``spatial_labels`` on every join case; the fp32 CPU reference must itself meet
every bound on the exact inputs of the GPU tests; and the case lists must visit every listed size and value."""
import os

import numpy as np
import pytest
import torch

from oracle import spatial_clip_oracle as O
from tests import _distill_oracle as DO
from tests import _losscases as L

F64 = torch.float64


def _close(name, got, want, rel, floor=0.0):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    err = float((got - want).abs().max())
    allowed = rel * float(want.abs().max()) + floor
    print(f"  {name}: max|d| {err:.3g}, allowed {allowed:.3g}")
    assert err <= allowed, (name, err, allowed)


def _closed_form_head(h, B, rank, s, b, cap, wreg, K, dt=F64):
    """Loss and feature / scale / bias gradients of ClipLoss (K = 0, no cap, no regulariser) or SpatialLoss from the closed
    forms of _losscases (clip_fwd / clip_bwd) in ``dt``, on the similarity matrices formed in ``dt``."""
    sl = slice(rank * B, (rank + 1) * B)
    fi, ft, ai, at = h["img"][sl].to(dt), h["txt"][sl].to(dt), h["img"].to(dt), h["txt"].to(dt)
    G = ai.shape[0]
    z = torch.stack([fi @ at.T, ft @ ai.T])
    col, w = L.join_sparse(h["img_ids"], h["txt_ids"], h["nbr"][:, :K], h["alpha"][:, :K], B, G, K, rank, h["alpha_scale"], dt)
    q = L.dense_labels(col, w, G, dt)
    s_eff = min(s, cap) if cap else s
    fwd = L.clip_fwd(z, q, s_eff, b, wreg, dt)
    rs = fwd["rowstats"]
    bwd = L.clip_bwd(z, q, s_eff, b, wreg, 1.0, rs[:, 0], rs[:, 1], fwd["loss_out"][1], dt)
    dz = bwd["dz"]
    return {"loss": fwd["loss_out"][0], "d_image": dz[0] @ at, "d_all_text": dz[0].T @ fi, "d_text": dz[1] @ ai,
            "d_all_image": dz[1].T @ ft, "d_scale": bwd["d_scale"], "d_bias": bwd["d_bias"]}


@pytest.mark.parametrize("B,G,rank,D", L.HEAD_SHAPES)
@pytest.mark.parametrize("kind", ["clip", "spatial"])
def test_closed_forms_reproduce_the_oracle_in_float64(kind, B, G, rank, D, monkeypatch):
    """clip_fwd / clip_bwd and the autograd form head_loss against oracle.clip_loss / spatial_loss with float64 as the default
    dtype (the oracle builds its labels in the default dtype), scale above the cap, a bias, the regulariser on.  The oracle
    casts its logits with ``.float()`` (the reference's float32_logits); around the oracle's call alone that cast is made the
    identity, after this module's own references (which rely on ``.float()``) have been formed."""
    h = L.head_inputs(B, G, rank, D)
    s, b, cap, wreg = L.f32(100.0), L.f32(-1.0), L.CAP_BELOW, 0.05
    sl = slice(rank * B, (rank + 1) * B)
    closed = _closed_form_head(h, B, rank, s, b, cap if kind == "spatial" else None, wreg if kind == "spatial" else 0.0,
                               L.HEAD_K if kind == "spatial" else 0)
    auto = L.head_loss(kind, h, B, rank, s, b, F64, cap=cap, wreg=wreg)
    leaf = lambda t: t.double().clone().requires_grad_(True)                            # noqa: E731
    fi, ft, ai, at = leaf(h["img"][sl]), leaf(h["txt"][sl]), leaf(h["img"]), leaf(h["txt"])
    sc, bi = leaf(torch.tensor(s)), leaf(torch.tensor(b))
    alpha64 = h["alpha"].double()
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "float", lambda t: t)
            if kind == "clip":
                loss = O.clip_loss(fi, ft, sc, ai, at, rank=rank, logit_bias=bi)
            else:
                loss = O.spatial_loss(fi, ft, sc, h["img_ids"][sl], h["txt_ids"][sl], h["nbr"], alpha64, ai, at,
                                      h["img_ids"], h["txt_ids"], rank=rank, cap_logit_scale=cap, temp_reg_weight=wreg,
                                      neighbor_alpha_scale=h["alpha_scale"], logit_bias=bi)
        g = torch.autograd.grad(loss, [fi, ft, ai, at, sc, bi])
    finally:
        torch.set_default_dtype(old)
    want = dict(zip(("d_image", "d_text", "d_all_image", "d_all_text", "d_scale", "d_bias"), g), loss=loss.detach())
    for name, w in want.items():
        # float64 rounding of sums over G terms of size <= the result's largest element (the gradients cancel: floor from
        # the size of their terms, s / B)
        _close(f"closed {name}", closed[name], w, 1e-12, 1e-13)
        _close(f"autograd {name}", auto[name], w, 1e-12, 1e-13)


@pytest.mark.parametrize("B,G,rank,D", L.HEAD_SHAPES)
def test_distillation_closed_form_reproduces_its_oracle(B, G, rank, D):
    h = L.head_inputs(B, G, rank, D)
    s, ts = L.f32(14.2857), 25.0
    sl = slice(rank * B, (rank + 1) * B)
    want = DO.distill_terms(h["img"][sl], h["txt"][sl], s, h["timg"][sl], h["ttxt"][sl], ts, h["img"], h["txt"], h["timg"],
                            h["ttxt"], rank=rank)
    fi, ft, ai, at = h["img"][sl].double(), h["txt"][sl].double(), h["img"].double(), h["txt"].double()
    ti, tt, tai, tat = h["timg"][sl].double(), h["ttxt"][sl].double(), h["timg"].double(), h["ttxt"].double()
    got = L.distill(torch.stack([fi @ at.T, ft @ ai.T]), torch.stack([ti @ tat.T, tt @ tai.T]), s, ts, rank * B, F64)
    auto = L.head_loss("distill", h, B, rank, s, 0.0, F64, ts=ts)
    for j, k in enumerate(("c", "d")):
        dz = got["dz_" + k]
        mine = {"loss": got["loss_out"][j], "d_scale": got["d_scale_" + k], "d_image": dz[0] @ at, "d_all_text": dz[0].T @ fi,
                "d_text": dz[1] @ ai, "d_all_image": dz[1].T @ ft}
        for name, v in mine.items():
            _close(f"{k} closed {name}", v, want[k][name], 1e-12, 1e-13)
            _close(f"{k} autograd {name}", auto[k][name], want[k][name], 1e-12, 1e-13)


def _golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _golden_check(name, golden, got64, got32):
    """The goldens are fp32 outputs of the reference implementation, so they are held to the closed forms by the project's rule
    for an fp32 result: within ``REF_FACTOR * E32 + ulp``, E32 the error of the same closed form evaluated in fp32."""
    L.check_f32(name, torch.as_tensor(golden), L.Ref(torch.as_tensor(got64).double(), torch.as_tensor(got32)))


@pytest.mark.parametrize("tag", ["w1_default", "w1_edges", "w1_capped", "w1_noreg_nocap", "w1_bias"])
def test_closed_forms_reproduce_the_w1_goldens(golden_dir, tag):
    z = _golden(golden_dir, f"loss_{tag}.npz")
    B, K = z["img"].shape[0], z["nb"].shape[1]
    cap = float(z["cap"]) if float(z["cap"]) >= 0 else None
    b = L.f32(z["bias"]) if int(z["has_bias"]) else 0.0
    h = {"img": z["img"], "txt": z["txt"], "img_ids": z["ids"], "txt_ids": z["ids"], "nbr": z["nb"], "alpha": z["alpha"],
         "alpha_scale": 0.5}
    s = float(z["scale"].float())
    for which, pre, args in (("spatial", "sp", (cap, float(z["w"]), K)), ("clip", "cl", (None, 0.0, 0))):
        got, g32 = _closed_form_head(h, B, 0, s, b, *args), _closed_form_head(h, B, 0, s, b, *args, dt=torch.float32)
        _golden_check(f"{which} loss", z[f"{which}_loss"], got["loss"], g32["loss"])
        _golden_check(f"{which} gimg", z[f"{pre}_gimg"], got["d_image"] + got["d_all_image"], g32["d_image"] + g32["d_all_image"])
        _golden_check(f"{which} gtxt", z[f"{pre}_gtxt"], got["d_text"] + got["d_all_text"], g32["d_text"] + g32["d_all_text"])
        _golden_check(f"{which} gscale", z[f"{pre}_gscale"], got["d_scale"], g32["d_scale"])


def test_closed_forms_reproduce_the_w2_golden(golden_dir):
    z = _golden(golden_dir, "loss_w2.npz")
    W, G, K = 2, z["img"].shape[0], z["nb"].shape[1]
    B = G // W
    s = L.f32(z["scale"])
    for which, args in (("spatial", (40.0, 0.05, K)), ("clip", (None, 0.0, 0))):
        outs, o32 = [], []
        for r in range(W):
            sl = slice(r * B, (r + 1) * B)
            h = {"img": z["img"], "txt": z["txt"], "img_ids": z["ids"], "txt_ids": z["ids"], "nbr": z["nb"][sl],
                 "alpha": z["alpha"][sl], "alpha_scale": 0.5}
            outs.append(_closed_form_head(h, B, r, s, 0.0, *args))
            o32.append(_closed_form_head(h, B, r, s, 0.0, *args, dt=torch.float32))
        for r in range(W):
            sl = slice(r * B, (r + 1) * B)
            full = lambda os_, loc, gath: os_[r][loc] + sum(o[gath][sl] for o in os_)            # noqa: E731
            _golden_check(f"r{r} {which} loss", z[f"r{r}_{which}_loss"], outs[r]["loss"], o32[r]["loss"])
            _golden_check(f"r{r} {which} gimg", z[f"r{r}_{which}_gimg"], full(outs, "d_image", "d_all_image"),
                          full(o32, "d_image", "d_all_image"))
            _golden_check(f"r{r} {which} gtxt", z[f"r{r}_{which}_gtxt"], full(outs, "d_text", "d_all_text"),
                          full(o32, "d_text", "d_all_text"))
            _golden_check(f"r{r} {which} gscale", z[f"r{r}_{which}_gscale"], outs[r]["d_scale"], o32[r]["d_scale"])


@pytest.mark.parametrize("c", L.JOIN_CASES, ids=[L.join_case_id(c) for c in L.JOIN_CASES])
def test_label_references_agree_with_the_oracle(c):
    """oracle.spatial_labels (fp32, dict semantics: the last column wins, repeated neighbours accumulate) against the dense
    float64 labels, to fp32 label precision ((K + 2) * u relative, the bound of the kernel's labels; the oracle's own fp32
    normalisation is a sum of at most K + 1 terms and a division); the fp32 sparse reference meets the same bound."""
    img, txt, nbr, alpha, a_scale, _ = L.join_inputs(c)
    want = O.spatial_labels(img, txt, nbr, alpha, c.B, c.rank, a_scale)
    col64, w64 = L.join_sparse(img, txt, nbr, alpha, c.B, c.G, c.K, c.rank, a_scale, F64)
    col32, w32 = L.join_sparse(img, txt, nbr, alpha, c.B, c.G, c.K, c.rank, a_scale, torch.float32)
    q64 = L.dense_labels(col64, w64, c.G)
    assert torch.equal(col64, col32)
    assert bool(((q64.sum(-1) - 1.0).abs() < 1e-14).all())
    for d in range(2):
        assert torch.equal(want[d] > 0, q64[d] > 0)                       # the same columns carry weight
        L.check_sum(f"oracle labels dir {d}", want[d], q64[d], q64[d].abs(), c.K + 2)
    L.check_sum("fp32 sparse labels", L.dense_labels(col32, w32, c.G), q64, q64.abs(), c.K + 2)


def _assert_refs(refs):
    assert L.finite(refs)
    for name, o in refs.items():
        L.check(name, o.r32, o)


def _fwd_as_inputs(f):
    rs = torch.stack([f[n].r32 for n in ("lse", "E_p[z]", "sum q*logit", "sum q*z")], -1)
    return rs, torch.stack([f[n].r32 for n in ("loss", "gap", "CE_image", "CE_text")])


@pytest.mark.parametrize("c", L.LOSS_CASES, ids=[L.loss_case_id(c) for c in L.LOSS_CASES])
def test_fp32_reference_meets_the_cliploss_bounds(c):
    """Forward and backward (the fp32 reference's row statistics standing in for the kernel's)."""
    z, col, w, s, b = L.loss_inputs(c)
    f = L.clip_fwd_refs(z, col, w, s, b, c.w)
    _assert_refs(f)
    _assert_refs(L.clip_bwd_refs(z, col, w, s, b, c.w, c.go, *_fwd_as_inputs(f)))


@pytest.mark.parametrize("c", L.SIG_CASES, ids=[L.sig_case_id(c) for c in L.SIG_CASES])
def test_fp32_reference_meets_the_siglip_bounds(c):
    z = L.z_matrix(c.vals, 1, c.B, c.G, c.rank * c.B, 4)[0]
    _assert_refs(L.siglip_refs(z, L.f32(c.scale), 0.0 if c.bias is None else L.f32(c.bias), c.rank * c.B))


@pytest.mark.parametrize("c", L.DIST_CASES, ids=[L.dist_case_id(c) for c in L.DIST_CASES])
def test_fp32_reference_meets_the_distillation_bounds(c):
    zs, zt, s, st = L.distill_inputs(c)
    refs = L.distill_refs(zs, zt, s, st, c.rank * c.B)
    _assert_refs(refs)
    if c.tvals == "peak" and c.tscale >= 60.0 and c.G > 1:
        # off its peak the teacher's exponent is -2 * s_t <= -120: exp underflows to an exact 0 in fp32 (never in float64)
        assert float(torch.softmax(st * zt.float(), -1).min()) == 0.0 and float(torch.softmax(st * zt.double(), -1).min()) > 0.0


@pytest.mark.parametrize("c", L.PCC_CASES, ids=[L.pcc_case_id(c) for c in L.PCC_CASES])
def test_fp32_reference_meets_the_pcc_bounds(c):
    pb, tb = L.pcc_inputs(c)
    refs = L.pcc_refs(pb[:, :c.cols], tb[:, :c.cols], c.init)
    want = O.zero_shot_pcc_rows(pb[:, :c.cols].double(), tb[:, :c.cols].double())
    _close("pcc against the oracle in float64", refs["pcc"].ref.r64, want, 1e-12, 1e-15)
    assert float(refs["pcc"].ref.r64[0]) == 0.0                   # the constant row
    for name in ("pcc", "sum"):
        L.check(name, refs[name].r32, refs[name])


@pytest.mark.parametrize("kind", ["clip", "spatial", "siglip", "distill"])
@pytest.mark.parametrize("B,G,rank,D", L.HEAD_SHAPES)
def test_fp32_reference_meets_the_head_bounds(kind, B, G, rank, D):
    h = L.head_inputs(B, G, rank, D)
    _assert_refs(L.head_refs(kind, h, B, rank, L.f32(14.2857), 0.0 if kind == "distill" else L.f32(-1.0)))


def test_recall_reference_and_helper_expressions():
    """Recall: ties go to the lower column, so an all-equal window of n rows ranks row i at i.  Helpers: the fp32 expressions are
    finite, and the three evaluation orders of fa * a + fb * b lie within their roundings of the exact value."""
    for n in (1, 4, 5, 9, 10, 11):
        assert L.recall_ref(torch.full((n, n), 0.3), n, 0, (0, 0, 0)) == [1, min(n, 5), min(n, 10)]
    for c in L.RECALL_CASES:
        z = L.recall_inputs(c)
        hits = L.recall_ref(z[c.row0:], c.n, c.col0, c.init)
        assert all(c.init[t] <= hits[t] <= c.init[t] + c.n for t in range(3)) and hits[0] - c.init[0] <= hits[1] - c.init[1]
    x = torch.tensor(L.EXP_X, dtype=torch.float32)
    assert bool(torch.isfinite(torch.exp(x)).all())
    for n in L.HELPER_N:
        a, b = L.helper_vectors(n)
        r = L.axpby_refs(a, b, L.f32(-2.5), L.f32(0.3))
        for k in ("plain", "fma_a", "fma_b"):
            assert bool(torch.isfinite(r[k]).all())
            assert bool(((r[k].double() - r["exact"]).abs() <= r["slack"]).all())


def test_cases_cover_every_value():
    """Every listed G, B, K and value case occurs (the lists of the issue, restated here so that a shrunken list fails)."""
    g_all, b_all = {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025}, {1, 2, 3, 255, 256, 257, 513}
    assert set(L.LOSS_G) == g_all and set(L.LOSS_B) == b_all and set(L.SCALES) == {1.0, 14.2857, 100.0}
    assert set(L.DISTILL_G) == g_all | {769, L.RESIDENT_MAX_G - 1, L.RESIDENT_MAX_G, L.RESIDENT_MAX_G + 1}
    for cases, gs in ((L.LOSS_CASES, g_all), (L.SIG_CASES, g_all), (L.DIST_CASES, set(L.DISTILL_G))):
        assert gs <= {c.G for c in cases} and b_all <= {c.B for c in cases}
        assert {(3, G) for G in gs if G >= 3} <= {(c.B, c.G) for c in cases}                         # G swept at B = 3
        assert {(B, min(G for G in g_all if G >= B)) for B in b_all} <= {(c.B, c.G) for c in cases}   # B at its smallest G
        assert all(c.B <= c.G and (c.rank + 1) * c.B <= c.G for c in cases)
        last = {(c.B, c.G) for c in cases if c.rank > 0 and (c.rank + 1) * c.B == c.G}
        assert last and any(c.rank == 0 and (c.B, c.G) in last for c in cases)                       # first and last rank
        assert any(0 < c.rank and (c.rank + 1) * c.B < c.G and (c.B, c.G) in last for c in cases)    # a middle rank
        assert set(L.VALUES) <= {c.vals for c in cases}
        assert set(L.SCALES) <= {c.scale for c in cases}
        for B, G, _ in L.VALUE_SHAPES:                  # every value case at every crossing shape
            assert set(L.VALUES) <= {c.vals for c in cases if (c.B, c.G) == (B, G)}
    lc = L.LOSS_CASES
    assert any(c.cap is None for c in lc) and any(c.cap and c.cap < c.scale for c in lc) and any(c.cap and c.cap > c.scale for c in lc)
    assert {None, -10.0, 3.0} <= {c.bias for c in lc} and {0.0, 0.05} <= {c.w for c in lc} and {None, -2.5} <= {c.go for c in lc}
    assert {c.K + 1 for c in lc} >= {1, 2, 6, 9}
    assert any(c.w > 0 and c.go is not None for c in lc) and any(c.scale == 100.0 and c.vals == "peak" for c in lc)
    assert {None, -10.0, 3.0} <= {c.bias for c in L.SIG_CASES}
    dc = L.DIST_CASES
    assert any(c.scale != c.tscale for c in dc) and any(c.tvals == "peak" and c.tscale >= 60.0 for c in dc)
    assert {"resident", "streamed"} <= {("resident" if c.G <= L.RESIDENT_MAX_G else "streamed") for c in dc}
    jc = L.JOIN_CASES
    assert {0, 1, 4, 5, 8, 63} <= {c.K for c in jc} and {1, 63, 64, 65, 257, 1025} <= {c.G for c in jc}
    tags = set()
    for c in jc:
        tags |= L.join_inputs(c)[5]
    assert tags == L.JOIN_TAGS
    rc = L.RECALL_CASES
    assert {1, 4, 5, 9, 10, 11, 257} <= {c.n for c in rc}
    assert any(c.row0 > 0 and c.rows > c.n for c in rc) and any(c.col0 > 0 and c.row0 == 0 for c in rc)
    assert any(any(c.init) for c in rc) and any(c.vals == "ties" for c in rc)
    pc = L.PCC_CASES
    assert {1, 3, 255, 256, 257, 1000} <= {c.cols for c in pc}
    assert any(c.ldp > c.cols and c.ldt > c.cols for c in pc) and any(not c.want_pcc for c in pc)
    assert any(not c.want_sum for c in pc) and any(c.want_sum and any(c.init) for c in pc)
    assert {(3, 9, 2, 8), (65, 130, 1, 33), (257, 257, 0, 96)} == set(L.HEAD_SHAPES)
