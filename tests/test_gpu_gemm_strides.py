"""Strided, offset and aliased GEMM operands: the views the towers pass (``qkv[:, d:]``, ``wb[:, d:]``, the class-token rows
``x.view(B, L * d)[:, :d]``, a residual that is the output itself, ``gw[d:]`` / ``gb[d:]``), through every kernel they reach.

Every operand is a view into a larger parent allocation.  The parents of the inputs hold 2^60 outside the view (exact in bf16
and fp32, finite: a masked lane that is multiplied by zero is legal, but a padding element that enters a sum or an epilogue
shows grossly); the parents of the outputs hold random bits, and everything outside the [M, N] view must hold the same bits
after the call.  Each case is checked three ways: against a float64 reference (small-integer operands make every fp32 value
exact, so the linear epilogues compare with ``torch.equal``; the GELU-type ones take the tolerances of test_gpu_gemm.py), bit
for bit against the same call on dense copies of the same views with the same ``ops.gemm_last_path`` (strides must not change
the dispatch), and for unchanged bytes outside the view."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
PAD = 2.0 ** 60
LINEAR = ("BF16", "BF16_BIAS", "F32", "F32_BIAS_RES", "BF16_BIAS_RES", "BF16_MUL_AUX")
EPIS = LINEAR + ("GELU_PAIR", "BF16_DGELU", "GELU_GRAD_PAIR", "QGELU_PAIR", "BF16_DQGELU", "QGELU_GRAD_PAIR")
PERSISTENT_EPIS = ("BF16", "BF16_BIAS", "GELU_PAIR", "GELU_GRAD_PAIR", "QGELU_PAIR", "QGELU_GRAD_PAIR")
# (h, factor, dU) of test_nt_gelu_grad_pair_and_mul_aux / test_nt_residual_gelu_dgelu: (atol, rtol)
TOL_H, TOL_FACTOR, TOL_DU = (8e-3, 8e-3), (4e-3, 8e-3), (3e-2, 3e-2)


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def view_in(dense, ld, col0=8, row0=1, rows_after=2, pad=PAD):
    """A copy of ``dense`` [R, C] as the view [row0 : row0 + R, col0 : col0 + C] of a parent with ``ld`` columns that holds
    ``pad`` everywhere else."""
    R, C = dense.shape
    assert col0 + C <= ld
    parent = torch.full((row0 + R + rows_after, ld), pad, dtype=dense.dtype, device="cuda")
    v = parent[row0:row0 + R, col0:col0 + C]
    v.copy_(dense)
    assert v.data_ptr() % 16 == 0 and v.stride(0) == ld
    return v


def vec_in(dense, off=8):
    """The 1-D twin of view_in."""
    parent = torch.full((dense.numel() + 2 * off,), PAD, dtype=dense.dtype, device="cuda")
    v = parent[off:off + dense.numel()]
    v.copy_(dense)
    return v


class Out:
    """An output view into a parent of random bits; ``outside_untouched()`` compares everything around the view with a clone
    taken before the call."""

    def __init__(self, rows, cols, ld, dtype, col0=8, row0=1, rows_after=2, seed=0):
        g = torch.Generator(device="cuda").manual_seed(1000 + seed)
        shape = (row0 + rows + rows_after, ld) if ld else (row0 + rows + rows_after,)
        if dtype == BF16:
            self.bits = torch.randint(-2 ** 15, 2 ** 15 - 1, shape, dtype=torch.int16, device="cuda", generator=g)
        else:
            self.bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)
        self.before = self.bits.clone()
        self.sl = (slice(row0, row0 + rows), slice(col0, col0 + cols)) if ld else (slice(row0, row0 + rows),)
        self.view = self.bits.view(dtype)[self.sl]
        assert self.view.data_ptr() % 16 == 0

    def outside_untouched(self):
        after = self.bits.clone()
        after[self.sl] = self.before[self.sl]
        return torch.equal(after, self.before)

    def untouched(self):
        return torch.equal(self.bits, self.before)


def dense_out(like):
    return torch.full(tuple(like.shape), 3.0, dtype=like.dtype, device="cuda")


def gelu64(x):
    return torch.nn.functional.gelu(x)


def gelu_grad64(x):
    x = x.detach().clone().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    return x.grad


def qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad64(x):
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def _close(got, want64, tol):
    """A bf16 output against the float64 reference rounded once to bf16, as the erf tests of test_gpu_gemm.py compare."""
    torch.testing.assert_close(got.float(), want64.to(BF16).float(), atol=tol[0], rtol=tol[1])


# ------------------------------------------------------------------------------------------ operands of an NT problem
_data = {}


def nt_data(M, N, K, curved):
    """Dense operands of one NT problem and its float64 product, made once per shape (one shape is kept at a time).
    ``curved``: A in sixteenths and B in quarters of small integers, bias in quarters, so that u = A.B^T + bias stays exact
    in fp32 and lands in the curved range of the activations (|u| of order 1); otherwise plain small integers."""
    key = (M, N, K, curved)
    if key not in _data:
        _data.clear()
        g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + K + int(curved))

        def ints(shape, lo, hi, dtype=BF16, scale=1.0):
            return (torch.randint(lo, hi + 1, shape, generator=g, device="cuda").float() * scale).to(dtype)

        a = ints((M, K), -3, 3, scale=1.0 / 16 if curved else 1.0)
        b = ints((N, K), -3, 3, scale=0.25 if curved else 1.0)
        d = dict(a=a, b=b, bias=ints((N,), -4, 4, F32, 0.25 if curved else 1.0), res32=ints((M, N), -100, 100, F32),
                 res16=ints((M, N), -8, 8), aux_int=ints((M, N), -3, 3),
                 aux_u=torch.randn((M, N), generator=g, device="cuda").to(BF16))
        d["acc"] = a.double() @ b.double().t()
        _data[key] = d
    return _data[key]


def distinct_lds(N, K):
    """Non-dense, pairwise different leading dimensions: multiples of 8 for the bf16 tensors, of 4 (and not of 8) for the fp32
    ones."""
    ld = dict(a=K + 24, b=K + 40, c16=N + 16, c2=N + 32, res16=N + 48, aux=N + 64, c32=N + 12, res32=N + 20)
    for trio in (("a", "b", "c16", "c2", "res16", "aux"), ("a", "b", "c32", "res32")):
        assert len({ld[k] for k in trio}) == len(trio), ld
    return ld


def run_nt(ops, name, M, N, K, d, ld, a=None, b=None):
    """One NT call of epilogue ``name`` on views (leading dimensions ``ld``; ``a`` / ``b``: ready-made operand views) or, with
    ``ld`` None, on the dense tensors themselves.  Returns (outputs, path, tail, the Out objects)."""
    epi = getattr(ops, "EPI_" + name)
    f32 = name in ("F32", "F32_BIAS_RES")
    strided = ld is not None
    if a is None:
        a = view_in(d["a"], ld["a"]) if strided else d["a"]
    if b is None:
        b = view_in(d["b"], ld["b"]) if strided else d["b"]
    kw, outs = {}, []
    if name in ("BF16_BIAS", "F32_BIAS_RES", "BF16_BIAS_RES", "GELU_PAIR", "GELU_GRAD_PAIR", "QGELU_PAIR", "QGELU_GRAD_PAIR"):
        kw["bias"] = vec_in(d["bias"]) if strided else d["bias"]
    if name == "F32_BIAS_RES":
        kw["res"] = view_in(d["res32"], ld["res32"], col0=4) if strided else d["res32"]
    if name == "BF16_BIAS_RES":
        kw["res"] = view_in(d["res16"], ld["res16"]) if strided else d["res16"]
    if name == "BF16_MUL_AUX":
        kw["aux"] = view_in(d["aux_int"], ld["aux"]) if strided else d["aux_int"]
    if name in ("BF16_DGELU", "BF16_DQGELU"):
        kw["aux"] = view_in(d["aux_u"], ld["aux"]) if strided else d["aux_u"]
    if strided:
        outs.append(Out(M, N, ld["c32"] if f32 else ld["c16"], F32 if f32 else BF16, col0=4 if f32 else 8))
        out = outs[0].view
    else:
        out = torch.full((M, N), 3.0, dtype=F32 if f32 else BF16, device="cuda")
    out2 = None
    if name in ("GELU_PAIR", "GELU_GRAD_PAIR", "QGELU_PAIR", "QGELU_GRAD_PAIR"):
        if strided:
            outs.append(Out(M, N, ld["c2"], BF16, seed=1))
            out2 = outs[1].view
        else:
            out2 = torch.full((M, N), 3.0, dtype=BF16, device="cuda")
        kw["out2"] = out2
    ops.gemm_last_path(reset=True)
    ops.gemm_last_tail(reset=True)
    ops.gemm(ops.NT, epi, a, b, out, M=M, N=N, K=K, **kw)
    return (out, out2), ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True), outs


def check_nt_reference(name, d, out, out2):
    """Check 1: the float64 reference."""
    acc, bias = d["acc"], d["bias"].double()
    quick = "QGELU" in name
    act, act_grad = (qgelu64, qgelu_grad64) if quick else (gelu64, gelu_grad64)
    if name in LINEAR:
        want = {"BF16": acc, "F32": acc, "BF16_BIAS": acc + bias, "F32_BIAS_RES": acc + bias + d["res32"].double(),
                "BF16_BIAS_RES": acc + bias + d["res16"].double(), "BF16_MUL_AUX": acc * d["aux_int"].double()}[name]
        assert torch.equal(out.double(), want.to(out.dtype).double()), name           # rounded once
    elif name in ("GELU_PAIR", "QGELU_PAIR"):
        u = (acc + bias).to(BF16)
        assert torch.equal(out, u), name                                              # u is exact before its one rounding
        _close(out2, act(u.double()), TOL_H)
    elif name in ("GELU_GRAD_PAIR", "QGELU_GRAD_PAIR"):
        u = (acc + bias).to(BF16).double()
        _close(out2, act(u), TOL_H)
        _close(out, act_grad(u), TOL_FACTOR)
    else:                                                                             # BF16_DGELU / BF16_DQGELU
        _close(out, acc * act_grad(d["aux_u"].double()), TOL_DU)


def check_nt(ops, name, M, N, K, want_path, want_tail=None, curved=None, ld=None, a_of=None, b_of=None):
    """The three checks of one NT case.  ``a_of`` / ``b_of``: functions that build the operand view from the dense operand (the
    towers' forms); default: views with the all-distinct leading dimensions."""
    curved = name not in LINEAR if curved is None else curved
    d = nt_data(M, N, K, curved)
    ld = ld or distinct_lds(N, K)
    (o, o2), path, tail, outs = run_nt(ops, name, M, N, K, d, ld, a=a_of(d["a"]) if a_of else None,
                                       b=b_of(d["b"]) if b_of else None)
    assert path.path == want_path, path
    if want_tail is not None:
        assert tail == want_tail, tail
    check_nt_reference(name, d, o, o2)                                                # 1. float64
    (do, do2), dpath, dtail, _ = run_nt(ops, name, M, N, K, d, None)                  # 2. the dense call
    assert path == dpath and tail == dtail, (path, dpath, tail, dtail)
    assert _same_bits(o, do) and (o2 is None or _same_bits(o2, do2)), name
    for x in outs:                                                                    # 3. outside the view
        assert x.outside_untouched(), name
    return path


# -------------------------------------------------------------------------------- 1. all leading dimensions distinct
@pytest.mark.parametrize("K", [64, 40, 72, 200])
@pytest.mark.parametrize("name", EPIS)
def test_distinct_lds_128_kernel(name, K):
    """The 128x128 kernel (K = 64) and its partial last K tile (K = 40, 72, 200: less than one tile, one and a bit, three and
    a bit), 2 x 2 ragged tiles."""
    check_nt(_ops(), name, 200, 136, K, "nt128" if K % 64 == 0 else "nt128_ktail")


@pytest.mark.parametrize("slots,tail", [(0, (112, 0)), (96, (96, 16))])
@pytest.mark.parametrize("name", EPIS)
def test_distinct_lds_8phase_kernel(monkeypatch, name, slots, tail):
    """The 256x256 phase-interleaved kernel on 14 x 8 ragged tiles, as full tiles (SC_GEMM_TAIL=0) and with the last 16 tiles
    -- the ragged tile row among them -- as 32 half tiles (SC_GEMM_TAIL=96)."""
    monkeypatch.setenv("SC_GEMM_TAIL", str(slots))
    path = check_nt(_ops(), name, 3368, 2024, 192, "nt8p", tail)
    assert path.lut == (name in ("GELU_GRAD_PAIR", "QGELU_GRAD_PAIR"))


@pytest.mark.parametrize("name", PERSISTENT_EPIS)
def test_distinct_lds_persistent_kernel(monkeypatch, name):
    """The persistent tile walk: 172 x 6 = 1032 ragged tiles, three K tiles; the derivative-storing pairs reach it only
    without the table."""
    monkeypatch.setenv("SC_GELU_LUT", "0")
    check_nt(_ops(), name, 256 * 171 + 40, 1536, 192, "nt8p_persistent")


# ------------------------------------------------------------------------------------------ 2. the towers' own forms
@pytest.mark.parametrize("M,want", [(256 * 171 + 40, "nt8p_persistent"), (3368, "nt128")])
def test_kv_projection_writes_the_right_columns_of_qkv(M, want):
    """C = qkv[:, d:] (ldc = 3 d, column offset d) with B = wq[d:] and bias = bq[d:]: the k / v projection of the block whose
    q is computed for the class tokens only (d = 768, so N = 1536, ldc = 2304).  The q columns of qkv must keep their bits."""
    ops = _ops()
    d_, K, name = 768, 192, "BF16_BIAS"
    N = 2 * d_
    d = nt_data(M, N, K, False)
    wq = torch.full((3 * d_, K), PAD, dtype=BF16, device="cuda")
    wq[d_:] = d["b"]
    bq = torch.full((3 * d_,), PAD, dtype=F32, device="cuda")
    bq[d_:] = d["bias"]
    qkv = Out(M, N, 3 * d_, BF16, col0=d_, row0=0, rows_after=0)
    ops.gemm_last_path(reset=True)
    ops.gemm(ops.NT, ops.EPI_BF16_BIAS, d["a"], wq[d_:], qkv.view, M=M, N=N, K=K, bias=bq[d_:])
    path = ops.gemm_last_path(reset=True)
    assert path.path == want, path
    assert qkv.view.stride(0) == 2304 and torch.equal(qkv.view.double(), (d["acc"] + d["bias"].double()).to(BF16).double())
    dense = dense_out(qkv.view)
    ops.gemm(ops.NT, ops.EPI_BF16_BIAS, d["a"], d["b"], dense, M=M, N=N, K=K, bias=d["bias"])
    assert ops.gemm_last_path(reset=True) == path and _same_bits(qkv.view, dense)
    assert qkv.outside_untouched()


@pytest.mark.parametrize("M,slots,want,tail", [(256 * 134 + 40, 0, "nt8p", (135, 0)), (256 * 134 + 40, 96, "nt8p", (96, 39)),
                                                (256 * 1024 + 40, None, "nt8p_persistent", (-1, -1))])
def test_kv_data_gradient_reads_the_right_columns(monkeypatch, M, slots, want, tail):
    """A = dqkv[:, d:], B = wb[:, d:] (K = 2 d, lda = ldb = 3 d, both based d elements into their rows): the data gradient of the
    k / v projection, on the 256x256 kernel, on its half-tile tail and on the persistent walk (d = 192: one ragged tile
    column).  The q columns hold 2^60 in both operands."""
    if slots is not None:
        monkeypatch.setenv("SC_GEMM_TAIL", str(slots))
    d_ = 192
    check_nt(_ops(), "BF16", M, d_, 2 * d_, want, tail,
             a_of=lambda a: view_in(a, 3 * d_, col0=d_, row0=0, rows_after=1),
             b_of=lambda b: view_in(b, 3 * d_, col0=d_, row0=0, rows_after=1))


@pytest.mark.parametrize("L", [5, 197])
@pytest.mark.parametrize("form", ["a_and_c", "res_f32", "res_bf16", "res_is_c"])
def test_class_token_views(form, L):
    """The rows of the class tokens, x.view(B, L * d)[:, :d] (ld = L * d) and qkv.view(B, L * 3 d)[:, :d] (ld = L * 3 d), on the
    128x128 kernel: as A and C (the q projection), as the fp32 and the bf16 residual of out_proj, and as the residual that is
    the output itself (EPI_BF16_BIAS_RES in place: dA_c += dq_c . W_q)."""
    ops = _ops()
    B, d_ = 72, 128
    M, N, K = B, d_, d_
    d = nt_data(M, N, K, False)
    want = d["acc"] + d["bias"].double()
    kw = dict(col0=0, row0=0, rows_after=0)
    ops.gemm_last_path(reset=True)
    if form == "a_and_c":
        epi, a = ops.EPI_BF16_BIAS, view_in(d["a"], L * d_, **kw)
        out = Out(M, N, L * 3 * d_, BF16, **kw)
        ops.gemm(ops.NT, epi, a, d["b"], out.view, M=M, N=N, K=K, bias=d["bias"])
        dkw = dict(bias=d["bias"])
    elif form == "res_f32":
        epi, a = ops.EPI_F32_BIAS_RES, view_in(d["a"], L * d_, **kw)
        out = Out(M, N, N + 12, F32, col0=4)
        ops.gemm(ops.NT, epi, a, d["b"], out.view, M=M, N=N, K=K, bias=d["bias"], res=view_in(d["res32"], L * d_, **kw))
        want, dkw = want + d["res32"].double(), dict(bias=d["bias"], res=d["res32"])
    elif form == "res_bf16":
        epi, a = ops.EPI_BF16_BIAS_RES, view_in(d["a"], L * d_, **kw)
        out = Out(M, N, N + 16, BF16)
        ops.gemm(ops.NT, epi, a, d["b"], out.view, M=M, N=N, K=K, bias=d["bias"], res=view_in(d["res16"], L * d_, **kw))
        want, dkw = want + d["res16"].double(), dict(bias=d["bias"], res=d["res16"])
    else:
        epi, a = ops.EPI_BF16_BIAS_RES, view_in(d["a"], L * 3 * d_, **kw)           # dq_c
        wb = view_in(d["b"], 3 * d_, **kw)                                          # wb[:, :d]
        out = Out(M, N, L * d_, BF16, **kw)                                         # dA_c, holding the k / v part already
        out.view.copy_(d["res16"])
        out.before = out.bits.clone()
        ops.gemm(ops.NT, epi, a, wb, out.view, M=M, N=N, K=K, bias=d["bias"], res=out.view)
        want, dkw = want + d["res16"].double(), dict(bias=d["bias"], res=d["res16"].clone())
    path = ops.gemm_last_path(reset=True)
    assert path.path == "nt128", path
    assert torch.equal(out.view.double(), want.to(out.view.dtype).double())
    dense = dkw["res"] if form == "res_is_c" else dense_out(out.view)
    ops.gemm(ops.NT, epi, d["a"], d["b"], dense, M=M, N=N, K=K, **dkw)
    assert ops.gemm_last_path(reset=True) == path and _same_bits(out.view, dense)
    assert out.outside_untouched()


# ------------------------------------------------------------------------------------------------ weight gradients
def tn_data(M, N, K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(M + N * 3 + K * 5 + seed)
    dy = torch.randint(-3, 4, (K, M), generator=g, device="cuda").to(BF16)
    x = torch.randint(-3, 4, (K, N), generator=g, device="cuda").to(BF16)
    return dy, x, dy.double().t() @ x.double(), dy.double().sum(0)


@pytest.mark.parametrize("splitk", [1, 4])
def test_kv_weight_gradient_lands_in_the_right_rows(splitk):
    """gemm_wgrad_bias(dqkv[:, d:], a1, gw[d:], gb[d:]): dY with lddy = 3 d based d elements into its rows, dW / dbias the rows
    from d on of the whole in_proj gradient (d = 520: 1040 x 520 is above the 8 tiles' area of the 256x256 TN kernel), 13 K
    tiles, without and with split-K.  The q rows of gw / gb must keep their bits."""
    ops = _ops()
    d_, K = 520, 64 * 13
    M, N = 2 * d_, d_
    dy, x, want, want_b = tn_data(M, N, K)
    dqkv_kv = view_in(dy, 3 * d_, col0=d_, row0=0, rows_after=0)
    gw = Out(M, N, N, F32, col0=0, row0=d_, rows_after=0)
    gb = Out(M, 0, 0, F32, row0=d_, rows_after=0, seed=1)
    ops.gemm_last_path(reset=True)
    ops.gemm_wgrad_bias(dqkv_kv, x, gw.view, gb.view, M=M, N=N, K=K, splitk=splitk)
    path = ops.gemm_last_path(reset=True)
    assert (path.path, path.splitk, path.colsum) == ("tn8p", splitk, "fused"), path
    assert torch.equal(gw.view.double(), want) and torch.equal(gb.view.double(), want_b)
    dw, db = torch.full((M, N), 3.0, device="cuda"), torch.full((M,), 3.0, device="cuda")
    ops.gemm_wgrad_bias(dy, x, dw, db, M=M, N=N, K=K, splitk=splitk)
    assert ops.gemm_last_path(reset=True) == path and _same_bits(gw.view, dw) and _same_bits(gb.view, db)
    assert gw.outside_untouched() and gb.outside_untouched()


@pytest.mark.parametrize("K,L,want", [(64, 5, ("tn8p", "fused")), (256, 5, ("tn8p", "fused")), (48, 5, ("tn128", "separate")),
                                      (64, 197, ("tn8p", "fused"))])
def test_class_token_weight_gradient(K, L, want):
    """gemm_wgrad_bias(dq_c, a1_c, gw[:d], gb[:d]) over the K = B class-token rows: lddy = L * 3 d, ldx = L * d.  A batch that
    is a multiple of 64 reaches the 256x256 TN kernel with its fused column sums, any other the 128x128 kernel and the
    separate column-sum kernel (d = 728: 728^2 is above the 8 tiles' area)."""
    ops = _ops()
    d_ = 728
    M = N = d_
    dy, x, want_w, want_b = tn_data(M, N, K, seed=L)
    dq_c = view_in(dy, L * 3 * d_, col0=0, row0=0, rows_after=0)
    a1_c = view_in(x, L * d_, col0=0, row0=0, rows_after=0)
    gw = Out(M, N, N, F32, col0=0, row0=0, rows_after=2 * d_)
    gb = Out(M, 0, 0, F32, row0=0, rows_after=2 * d_, seed=1)
    ops.gemm_last_path(reset=True)
    ops.gemm_wgrad_bias(dq_c, a1_c, gw.view, gb.view, M=M, N=N, K=K)
    path = ops.gemm_last_path(reset=True)
    assert (path.path, path.colsum) == want, path
    assert torch.equal(gw.view.double(), want_w) and torch.equal(gb.view.double(), want_b)
    dw, db = torch.full((M, N), 3.0, device="cuda"), torch.full((M,), 3.0, device="cuda")
    ops.gemm_wgrad_bias(dy, x, dw, db, M=M, N=N, K=K)
    assert ops.gemm_last_path(reset=True) == path and _same_bits(gw.view, dw) and _same_bits(gb.view, db)
    assert gw.outside_untouched() and gb.outside_untouched()


@pytest.mark.parametrize("splitk", [1, 2])
def test_weight_gradient_group_with_strided_operands(splitk):
    """gemm_wgrad_group with strided dY / X and dW / dbias that are dense views into larger gradients: two problems over one
    token axis in one launch of the grouped TN kernel."""
    ops = _ops()
    K = 64 * 5
    shapes = [(1040, 520), (520, 1040)]
    probs, wants, outs, dense = [], [], [], []
    for i, (M, N) in enumerate(shapes):
        dy, x, want, want_b = tn_data(M, N, K, seed=i)
        dw = Out(M, N, N, F32, col0=0, row0=8, rows_after=8, seed=2 * i)
        db = Out(M, 0, 0, F32, row0=8, rows_after=8, seed=2 * i + 1)
        probs.append((view_in(dy, M + 24 + 16 * i, row0=0), view_in(x, N + 48 + 16 * i, row0=0), dw.view, db.view, M, N))
        dense.append((dy, x, torch.full((M, N), 3.0, device="cuda"), torch.full((M,), 3.0, device="cuda"), M, N))
        wants.append((want, want_b))
        outs += [dw, db]
    ops.gemm_last_path(reset=True)
    ops.gemm_wgrad_group(probs, K=K, splitk=splitk)
    path = ops.gemm_last_path(reset=True)
    assert (path.path, path.group, path.splitk, path.colsum) == ("tn8p_group", "one_launch", splitk, "fused"), path
    ops.gemm_wgrad_group(dense, K=K, splitk=splitk)
    assert ops.gemm_last_path(reset=True) == path
    for p, q, (want, want_b) in zip(probs, dense, wants):
        assert torch.equal(p[2].double(), want) and torch.equal(p[3].double(), want_b)
        assert _same_bits(p[2], q[2]) and _same_bits(p[3], q[3])
    for o in outs:
        assert o.outside_untouched()


@pytest.mark.parametrize("M,N,K,want", [(808, 792, 192, "tn8p"), (200, 136, 100, "tn128")])
def test_plain_tn_with_a_strided_output(M, N, K, want):
    """Plain TN (EPI_F32) with ldw != N at split-K 1, every leading dimension non-dense and different."""
    ops = _ops()
    dy, x, want_w, _ = tn_data(M, N, K)
    out = Out(M, N, N + 12, F32, col0=4)
    ops.gemm_last_path(reset=True)
    ops.gemm(ops.TN, ops.EPI_F32, view_in(dy, M + 24), view_in(x, N + 56), out.view, M=M, N=N, K=K)
    path = ops.gemm_last_path(reset=True)
    assert path.path == want, path
    assert torch.equal(out.view.double(), want_w)
    dense = dense_out(out.view)
    ops.gemm(ops.TN, ops.EPI_F32, dy, x, dense, M=M, N=N, K=K)
    assert ops.gemm_last_path(reset=True) == path and _same_bits(out.view, dense)
    assert out.outside_untouched()


@pytest.mark.parametrize("mode", ["NT", "TN", "wgrad_bias"])
def test_split_k_refuses_a_strided_output(mode):
    """Split-K sums dense [M, N] slabs into C: with ldc != N the call must raise, before any launch, and leave the whole output
    parent as it was."""
    ops = _ops()
    M, N, K = 808, 792, 64 * 4
    dy, x, _, _ = tn_data(M, N, K)
    out = Out(M, N, N + 12, F32, col0=4)
    db = Out(M, 0, 0, F32, row0=8, seed=1)
    with pytest.raises(Exception, match="sc_gemm_bf16: split-K needs a dense C"):
        if mode == "wgrad_bias":
            ops.gemm_wgrad_bias(dy, x, out.view, db.view, M=M, N=N, K=K, splitk=2)
        elif mode == "TN":
            ops.gemm(ops.TN, ops.EPI_F32, dy, x, out.view, M=M, N=N, K=K, splitk=2)
        else:
            ops.gemm(ops.NT, ops.EPI_F32, dy.t().contiguous(), x.t().contiguous(), out.view, M=M, N=N, K=K, splitk=2)
    torch.cuda.synchronize()
    assert out.untouched() and db.untouched()


# ------------------------------------------------------------------------------------------------------- e4m3 NT
FP8_EPIS = ("BF16", "BF16_BIAS", "F32_BIAS_RES", "GELU_PAIR", "BF16_DGELU", "F32", "BF16_BIAS_RES", "GELU_GRAD_PAIR", "BF16_MUL_AUX")
_fp8 = {}


def fp8_data(ops, M, N, K):
    """Integers in [-7, 7] times power-of-two row scales (every product and partial sum exact in fp32), quantised; the
    epilogue inputs of nt_data.  ``curve``: a factor on A's scales that brings u into the activations' curved range."""
    if not _fp8:
        g = torch.Generator(device="cuda").manual_seed(88)

        def rows(n):
            v = torch.randint(-7, 8, (n, K), generator=g, device="cuda").float()
            return v * torch.pow(2.0, torch.randint(-3, 4, (n, 1), generator=g, device="cuda").float())

        a, b = rows(M), rows(N)
        a8, sa = ops.quantize_rows_fp8(a)
        b8, sb = ops.quantize_rows_fp8(b)
        assert torch.equal(a8.view(torch.float8_e4m3fn).float() * sa[:, None], a)
        _fp8.update(nt_data(M, N, K, False))
        _fp8.update(a8=a8, sa=sa, b8=b8, sb=sb, acc=a.double() @ b.double().t(), curve=2.0 ** -12)
    return _fp8


def run_fp8(ops, name, M, N, K, d, ld):
    strided = ld is not None
    f32 = name in ("F32", "F32_BIAS_RES")
    curved = name in ("GELU_PAIR", "GELU_GRAD_PAIR")
    a8 = view_in(d["a8"], ld["a"], col0=16, pad=0x7E) if strided else d["a8"]      # 0x7E = 448, the largest finite e4m3
    b8 = view_in(d["b8"], ld["b"], col0=16, pad=0x7E) if strided else d["b8"]
    sa = d["sa"] * d["curve"] if curved else d["sa"]
    sa, sb = (vec_in(sa), vec_in(d["sb"])) if strided else (sa, d["sb"])
    kw, outs = {}, []
    if name in ("BF16_BIAS", "F32_BIAS_RES", "BF16_BIAS_RES", "GELU_PAIR", "GELU_GRAD_PAIR"):
        kw["bias"] = vec_in(d["bias"]) if strided else d["bias"]
    if name == "F32_BIAS_RES":
        kw["res"] = view_in(d["res32"], ld["res32"], col0=4) if strided else d["res32"]
    if name == "BF16_BIAS_RES":
        kw["res"] = view_in(d["res16"], ld["res16"]) if strided else d["res16"]
    if name == "BF16_MUL_AUX":
        kw["aux"] = view_in(d["aux_int"], ld["aux"]) if strided else d["aux_int"]
    if name == "BF16_DGELU":
        kw["aux"] = view_in(d["aux_u"], ld["aux"]) if strided else d["aux_u"]
    if strided:
        outs.append(Out(M, N, ld["c32"] if f32 else ld["c16"], F32 if f32 else BF16, col0=4 if f32 else 8))
        out = outs[0].view
    else:
        out = torch.full((M, N), 3.0, dtype=F32 if f32 else BF16, device="cuda")
    out2 = None
    if name in ("GELU_PAIR", "GELU_GRAD_PAIR"):
        if strided:
            outs.append(Out(M, N, ld["c2"], BF16, seed=1))
        out2 = outs[1].view if strided else torch.full((M, N), 3.0, dtype=BF16, device="cuda")
        kw["out2"] = out2
    ops.gemm_last_path(reset=True)
    ops.gemm_fp8(getattr(ops, "EPI_" + name), a8, sa, b8, sb, out, M=M, N=N, K=K, **kw)
    return (out, out2), ops.gemm_last_path(reset=True), outs


@pytest.mark.parametrize("name", FP8_EPIS)
def test_distinct_lds_fp8_kernel(name):
    """The e4m3 NT kernel with every byte / element stride non-dense and different (operand strides multiples of 16 bytes),
    scale vectors and bias based into larger buffers: 2 x 1 ragged tiles, three K tiles of 128."""
    ops = _ops()
    M, N, K = 300, 200, 384
    d = fp8_data(ops, M, N, K)
    ld = dict(distinct_lds(N, K), a=K + 48, b=K + 80)
    (o, o2), path, outs = run_fp8(ops, name, M, N, K, d, ld)
    assert path.path == "fp8_nt", path
    if name in ("GELU_PAIR", "GELU_GRAD_PAIR"):
        check_nt_reference(name, dict(d, acc=d["acc"] * d["curve"]), o, o2)
    else:
        check_nt_reference(name, d, o, o2)
    (do, do2), dpath, _ = run_fp8(ops, name, M, N, K, d, None)
    assert path == dpath and _same_bits(o, do) and (o2 is None or _same_bits(o2, do2))
    for x in outs:
        assert x.outside_untouched(), name
