"""Thin, validated wrappers over the C ABI.  Tensors in / tensors out, raw pointers underneath.
Every function enqueues on the current HIP stream and never synchronises."""
from __future__ import annotations

import collections
import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import check

NT, TN = 0, 1
(EPI_BF16, EPI_BF16_BIAS, EPI_F32_BIAS_RES, EPI_GELU_PAIR, EPI_BF16_DGELU, EPI_F32, EPI_BF16_BIAS_RES, EPI_GELU_GRAD_PAIR,
 EPI_BF16_MUL_AUX, EPI_QGELU_PAIR, EPI_BF16_DQGELU, EPI_QGELU_GRAD_PAIR) = range(12)


def act_epilogues(quick_gelu: bool):
    """(pair, grad_pair, dgelu) epilogues of a block's activation: exact-erf GELU (nn.GELU) or, for towers built with
    ``quick_gelu: true`` (src/open_clip/model.py:142-145), QuickGELU x * sigmoid(1.702 x)."""
    if quick_gelu:
        return EPI_QGELU_PAIR, EPI_QGELU_GRAD_PAIR, EPI_BF16_DQGELU
    return EPI_GELU_PAIR, EPI_GELU_GRAD_PAIR, EPI_BF16_DGELU


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str) -> None:
    if not t.is_cuda:
        raise _lib.SpatialClipHipError(f"{name}: expected a device tensor (no CPU path exists)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


_slab_cache = {}


def _slabs(nfloat: int, device) -> torch.Tensor:
    # scratch is per STREAM: two streams of one step (the towers side by side, net.py; the weight-gradient side stream) must
    # never share a split-K slab buffer -- launches of one stream are ordered, launches of two are not
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _slab_cache.get(key)
    if buf is None or buf.numel() < nfloat:
        buf = torch.empty(max(nfloat, 1 << 22), dtype=torch.float32, device=device)
        _slab_cache[key] = buf
    return buf


def gemm(mode: int, epi: int, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int,
         out2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None, splitk: int = 1) -> torch.Tensor:
    """C[M,N] = A.B^T (NT: a[M,K], b[N,K]) or At^T.Bt (TN: a[K,M], b[K,N]) with a fused epilogue."""
    _req(a, torch.bfloat16, "a"); _req(b, torch.bfloat16, "b")
    want = torch.float32 if epi in (EPI_F32, EPI_F32_BIAS_RES) else torch.bfloat16
    _req(out, want, "out")
    if bias is not None: _req(bias, torch.float32, "bias")
    if res is not None: _req(res, torch.bfloat16 if epi == EPI_BF16_BIAS_RES else torch.float32, "res")
    if aux is not None: _req(aux, torch.bfloat16, "aux")
    if out2 is not None: _req(out2, torch.bfloat16, "out2")
    l = _lib.lib()
    slabs = None
    if splitk > 1:
        n = l.sc_gemm_slab_floats(M, N, K, splitk)
        slabs = _slabs(n, out.device) if n else None
        if slabs is None:
            splitk = 1
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    rc = l.sc_gemm_bf16(mode, epi, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), M, N, K,
                        out.data_ptr(), out.stride(0), _ptr(out2), out2.stride(0) if out2 is not None else 0,
                        _ptr(bias), _ptr(res), res.stride(0) if res is not None else 0,
                        _ptr(aux), aux.stride(0) if aux is not None else 0, splitk, _ptr(slabs), _stream())
    if ev is not None:
        ev[1].record()
        # algorithmic bytes of the launch: both operands once, every output once, every epilogue input once
        ob = 4 if want == torch.float32 else 2
        nbytes = 2.0 * M * K + 2.0 * N * K + float(ob) * M * N
        nbytes += (2.0 * M * N if out2 is not None else 0.0) + (float(res.element_size()) * M * N if res is not None else 0.0)
        nbytes += (2.0 * M * N if aux is not None else 0.0) + (4.0 * N if bias is not None else 0.0)
        KERNEL_EVENTS.append(("gemm_nt" if mode == NT else "gemm_tn", 2.0 * M * N * K, ev, nbytes))
    check(rc, "sc_gemm_bf16")
    return out


def gemm_wgrad_bias(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, dbias: torch.Tensor, *, M: int, N: int, K: int,
                    splitk: int = 1) -> None:
    """dW[M,N] = dY[K,M]^T . X[K,N] (fp32) and dbias[M] = column sums of dY, one fused pass."""
    _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw")
    _req(dbias, torch.float32, "dbias")
    l = _lib.lib()
    ws = workspace(l.sc_gemm_wgrad_ws_floats(M, N, K, splitk), dw.device, "wgrad")
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    rc = l.sc_gemm_wgrad_bias(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), M, N, K, dw.data_ptr(),
                              dw.stride(0), dbias.data_ptr(), splitk, ws.data_ptr(), _stream())
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append(("gemm_tn", 2.0 * M * N * K, ev))
    check(rc, "sc_gemm_wgrad_bias")


class _WgradDesc(ctypes.Structure):
    """``sc_wgrad_desc`` of include/spatial_clip_hip.h."""
    _fields_ = [("dY", ctypes.c_void_p), ("lddy", ctypes.c_longlong), ("X", ctypes.c_void_p), ("ldx", ctypes.c_longlong),
                ("dW", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("M", ctypes.c_int), ("N", ctypes.c_int)]


WGRAD_GROUP_MAX = 4


def gemm_wgrad_group(problems, *, K: int, splitk: int = 1) -> None:
    """Several weight (+ bias) gradients over ONE token axis in one launch: ``problems`` = iterable of
    (dy [K, M], x [K, N], dw [M, N] fp32 dense, dbias [M] or None, M, N); dW = dY^T . X, dbias = column sums of dY."""
    problems = list(problems)
    if not 1 <= len(problems) <= WGRAD_GROUP_MAX:
        raise ValueError(f"gemm_wgrad_group: 1..{WGRAD_GROUP_MAX} problems, got {len(problems)}")
    arr = (_WgradDesc * len(problems))()
    flops = 0.0
    for d, (dy, x, dw, dbias, M, N) in zip(arr, problems):
        _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw")
        if dbias is not None: _req(dbias, torch.float32, "dbias")
        if not dw.is_contiguous() or dw.numel() != M * N:
            raise ValueError("gemm_wgrad_group: dw must be a dense [M, N] tensor")
        d.dY, d.lddy, d.X, d.ldx = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0)
        d.dW, d.dbias, d.M, d.N = dw.data_ptr(), _ptr(dbias), M, N
        flops += 2.0 * M * N * K
    l = _lib.lib()
    p = ctypes.cast(arr, ctypes.c_void_p)
    ws = workspace(l.sc_gemm_wgrad_group_ws_floats(p, len(problems), K, splitk), problems[0][0].device, "wgrad")
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    rc = l.sc_gemm_wgrad_group(p, len(problems), K, splitk, ws.data_ptr(), _stream())
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append(("gemm_tn", flops, ev))
    check(rc, "sc_gemm_wgrad_group")


# bench.py sets this to a list to bracket every GEMM launch with HIP events on the launch stream
KERNEL_EVENTS = None


# ------------------------------------------------------------------------------------------ workspace
_ws_cache = {}


def workspace(nfloat: int, device, tag: str = "ws", dtype=torch.float32) -> torch.Tensor:
    """Scratch of at least ``nfloat`` elements for the launch being enqueued: one buffer per (device, purpose, dtype, STREAM) --
    see ``_slabs``."""
    key = (device.index, tag, dtype, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nfloat:
        buf = torch.empty(max(int(nfloat), 1024), dtype=dtype, device=device)
        _ws_cache[key] = buf
    return buf


# ------------------------------------------------------------------------------------------ attention
def attn_fwd(qkv: torch.Tensor, B: int, L: int, H: int, dh: int, causal: bool = False,
             out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None, q_rows: int = 0):
    """softmax(q k^T / sqrt(dh)) v on the packed bf16 ``qkv`` [B*L, 3*H*dh]: (out bf16 [B*L, H*dh], lse fp32 [B, H, L]).
    Head dims 32 / 64 / 80 up to 320 tokens, causal or not (80: ViT-H, sc_attention_stream.hip); head dim 64 non-causal at any
    length.  Anything else raises RuntimeError naming the limit, before a launch.  ``q_rows`` > 0: only the first ``q_rows``
    query rows of every sequence are computed."""
    _req(qkv, torch.bfloat16, "qkv")
    if out is None:
        out = torch.empty((B * L, H * dh), dtype=torch.bfloat16, device=qkv.device)
    if lse is None:
        lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    check(_lib.lib().sc_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, dh, int(causal), q_rows,
                                 _stream()), "sc_attn_fwd")
    return out, lse


def attn_bwd(qkv, out, dout, lse, B: int, L: int, H: int, dh: int, causal: bool = False,
             dqkv: Optional[torch.Tensor] = None, delta: Optional[torch.Tensor] = None, q_rows: int = 0):
    """d(qkv) (bf16, the layout of ``qkv``) from ``out``, ``dout`` and the forward's ``lse``; the shapes of ``attn_fwd``
    (head dims 32 / 64 / 80 up to 320 tokens; 64 non-causal at any length).  No float atomics: two calls give identical
    bits.  At head dim 80, on the long-sequence path and with ``q_rows == 1`` every element of ``dqkv`` is written."""
    for t_, n in ((qkv, "qkv"), (out, "out"), (dout, "dout")):
        _req(t_, torch.bfloat16, n)
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    if delta is None:
        delta = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    check(_lib.lib().sc_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                 dqkv.data_ptr(), B, L, H, dh, int(causal), q_rows, _stream()), "sc_attn_bwd")
    return dqkv


# enum sc_attn_path (csrc/sc_kernels.h), in order
ATTN_FWD_PATHS = ("persistent", "persistent2", "per_head", "stream")
ATTN_BWD_PATHS = ("cls", "ring", "ring8", "single_pass", "persistent", "fused", "dq_dkv", "stream")


def attn_last_path():
    """(forward, backward): the names of the kernels that the last ``attn_fwd`` and the last ``attn_bwd`` of this process
    dispatched to (``ATTN_FWD_PATHS`` / ``ATTN_BWD_PATHS``; ``"none"`` before the first call).  A debug hook
    (``sc_debug_attn_last_path``): host-side bookkeeping, no device work."""
    fn = getattr(_lib.lib(), "sc_debug_attn_last_path")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2
    f, b = ctypes.c_int(-1), ctypes.c_int(-1)
    check(fn(ctypes.byref(f), ctypes.byref(b)), "sc_debug_attn_last_path")
    return (ATTN_FWD_PATHS[f.value] if f.value >= 0 else "none", ATTN_BWD_PATHS[b.value] if b.value >= 0 else "none")


def attn_plan(B: int, L: int, H: int, dh: int, causal: bool = False, q_rows: int = 0):
    """(forward, backward): the names of the kernels that ``attn_fwd`` / ``attn_bwd`` would dispatch this shape to under the
    current environment switches, without launching anything (``sc_debug_attn_plan``: host arithmetic only, so it runs
    without a GPU).  A shape the library refuses raises RuntimeError with ``sc_attn_fwd``'s own message."""
    fn = getattr(_lib.lib(), "sc_debug_attn_plan")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)] * 2
    f, b = ctypes.c_int(-1), ctypes.c_int(-1)
    check(fn(B, L, H, dh, int(causal), q_rows, ctypes.byref(f), ctypes.byref(b)), "sc_debug_attn_plan")
    return ATTN_FWD_PATHS[f.value], ATTN_BWD_PATHS[b.value]


def gemm_tail_rule(T: int, S: int):
    """(nfull, rem) of the NT GEMM's tail split for ``T`` 256x256 tiles on ``S`` workgroup slots: the first ``nfull`` tiles run
    as full tiles and the last ``rem`` as ``2 * rem`` half tiles; ``(T, 0)`` when the launch is not split
    (``sc_debug_gemm_tail_rule``: host arithmetic only, so it runs without a GPU)."""
    fn = getattr(_lib.lib(), "sc_debug_gemm_tail_rule")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 2 + [ctypes.POINTER(ctypes.c_int)] * 2
    nfull, rem = ctypes.c_int(-1), ctypes.c_int(-1)
    split = fn(T, S, ctypes.byref(nfull), ctypes.byref(rem))
    assert bool(split) == (rem.value > 0)
    return nfull.value, rem.value


def gemm_last_tail(reset: bool = False):
    """(nfull, rem) of the last launch of the non-persistent 256x256 NT kernel by this process: ``(tiles, 0)`` when its tail
    was not split, ``(-1, -1)`` when there was none since the last ``reset`` (the launch went to another kernel).  A debug
    hook (``sc_debug_gemm_last_tail``): host-side bookkeeping, no device work."""
    fn = getattr(_lib.lib(), "sc_debug_gemm_last_tail")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.c_int]
    nfull, rem = ctypes.c_int(-1), ctypes.c_int(-1)
    fn(ctypes.byref(nfull), ctypes.byref(rem), int(reset))
    return nfull.value, rem.value


# enum sc_gemm_path / sc_gemm_colsum / sc_gemm_group (csrc/sc_kernels.h), in order
GEMM_PATHS = ("nt128", "nt128_ktail", "tn128", "nt8p", "nt8p_persistent", "tn8p", "tn8p_group", "nt256", "tn256", "fp8_nt",
              "fp8_tn")
GEMM_COLSUMS = ("none", "fused", "separate")
GEMM_GROUPS = ("none", "one_launch", "per_problem")
GemmPath = collections.namedtuple("GemmPath", "path lut col_group splitk colsum group")


def gemm_last_path(reset: bool = False) -> GemmPath:
    """What the last ``gemm`` / ``gemm_wgrad_bias`` / ``gemm_wgrad_group`` / ``gemm_fp8*`` / ``gemm_wgrad_fp8`` of this process
    dispatched to: ``path`` (one of ``GEMM_PATHS``; ``"none"`` before the first call or after a ``reset``), ``lut`` (the GELU
    table was attached), ``col_group`` (column group of the tile walk in effect, 0 = row-major), ``splitk`` (the split-K
    actually used), ``colsum`` (bias-gradient column sums: ``"fused"`` into the TN kernel, a ``"separate"`` kernel, or
    ``"none"``) and ``group`` (``gemm_wgrad_group``: ``"one_launch"``, or ``"per_problem"`` with the other fields those of the
    last problem; ``"none"`` for the other entry points).  Whether the 256x256 NT kernel split its tail is
    ``gemm_last_tail``'s.  A debug hook (``sc_debug_gemm_last_path``): host-side bookkeeping, no device work."""
    fn = getattr(_lib.lib(), "sc_debug_gemm_last_path")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]
    out = (ctypes.c_int * 6)()
    assert fn(out, 6, int(reset)) == 6
    return GemmPath(GEMM_PATHS[out[0]] if out[0] >= 0 else "none", bool(out[1]), out[2], out[3], GEMM_COLSUMS[out[4]],
                    GEMM_GROUPS[out[5]])


def gemm_plan(mode: int, epi: int, M: int, N: int, K: int, *, ldc: Optional[int] = None, splitk: int = 1,
              has_slabs: bool = False, colsum: bool = False, slots: int = 0):
    """(GemmPath, (nfull, rem)): what ``gemm_last_path`` / ``gemm_last_tail`` would report after ``gemm`` (``colsum``:
    ``gemm_wgrad_bias``) of this problem under the current environment switches on a device of ``slots`` CUs (0: no tail
    split), without launching anything (``sc_debug_gemm_plan``: the planner the entry points call, host arithmetic only, so
    it runs without a GPU).  ``ldc`` defaults to a dense ``N``.  A problem the library refuses raises RuntimeError with the
    entry point's own message."""
    fn = getattr(_lib.lib(), "sc_debug_gemm_plan")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    out = (ctypes.c_int * 8)()
    check(fn(mode, epi, M, N, K, N if ldc is None else ldc, splitk, int(has_slabs), int(colsum), slots, out, 8),
          "sc_debug_gemm_plan")
    return (GemmPath(GEMM_PATHS[out[0]], bool(out[1]), out[2], out[3], GEMM_COLSUMS[out[4]], GEMM_GROUPS[out[5]]),
            (out[6], out[7]))


# ------------------------------------------------------------------------------------------ norms
def _t8_args(t8, rows: int, d: int, what: str):
    """(buffer uint8 [rows, >= d], scale fp32 [1], amax fp32 [64]) -> ctypes arguments of a per-tensor e4m3 second output."""
    buf, scale, amax = t8
    if buf.dtype != torch.uint8 or not buf.is_cuda or buf.stride(-1) != 1 or buf.shape[0] < rows or buf.shape[1] < d:
        raise TypeError(f"{what}: t8 buffer must be a device uint8 matrix of at least [{rows}, {d}]")
    _req(scale, torch.float32, "t8 scale"); _req(amax, torch.float32, "t8 amax")
    if scale.numel() != 1 or amax.numel() != 64:
        raise ValueError(f"{what}: t8 needs a one-element scale and 64 amax slots")
    return buf.data_ptr(), buf.stride(0), scale.data_ptr(), amax.data_ptr()


def layernorm_fwd(x, gamma, beta, y, mean, rstd, rows: int, d: int, ldx: Optional[int] = None,
                  ldy: Optional[int] = None, eps: float = 1e-5, q8: Optional[torch.Tensor] = None,
                  q8_scale_inv: Optional[torch.Tensor] = None, t8=None):
    """``q8`` (uint8 [rows, d]) + ``q8_scale_inv`` (fp32 [rows]): also emit the e4m3 copy of the output with its
    per-row power-of-two scale (the fp8 forward GEMM's A operand) from the same kernel.  ``t8`` = (uint8 [rows, d], scale
    [1], amax [64]): a SECOND e4m3 copy with one delayed scale for the whole tensor (the e4m3 weight gradient's X operand;
    bf16 rows + q8 only)."""
    _req(y, torch.bfloat16, "y")
    if q8 is not None:
        if q8.dtype != torch.uint8 or not q8.is_cuda or q8.stride(-1) != 1:
            raise TypeError("layernorm_fwd: q8 must be a device uint8 matrix")
        _req(q8_scale_inv, torch.float32, "q8_scale_inv")
    if t8 is not None and (x.dtype != torch.bfloat16 or q8 is None):
        raise _lib.SpatialClipHipError("layernorm_fwd: the per-tensor e4m3 copy exists for bf16 rows with the per-row copy (q8)")
    if x.dtype == torch.bfloat16 and t8 is not None:
        tp, tld, tsc, tam = _t8_args(t8, rows, d, "layernorm_fwd")
        check(_lib.lib().sc_layernorm_fwd_x16_t8(x.data_ptr(), ldx if ldx is not None else d, gamma.data_ptr(), beta.data_ptr(),
                                                 y.data_ptr(), ldy if ldy is not None else d, q8.data_ptr(), q8.stride(0),
                                                 q8_scale_inv.data_ptr(), tp, tld, tsc, tam, _ptr(mean), _ptr(rstd), rows, d, eps,
                                                 _stream()), "sc_layernorm_fwd_x16_t8")
        return y
    if x.dtype == torch.bfloat16:           # residual stream kept in bf16 (EPI_BF16_BIAS_RES)
        _req(x, torch.bfloat16, "x")
        check(_lib.lib().sc_layernorm_fwd_x16(x.data_ptr(), ldx if ldx is not None else d, gamma.data_ptr(), beta.data_ptr(),
                                              y.data_ptr(), ldy if ldy is not None else d, _ptr(q8),
                                              q8.stride(0) if q8 is not None else 0, _ptr(q8_scale_inv), _ptr(mean),
                                              _ptr(rstd), rows, d, eps, _stream()), "sc_layernorm_fwd_x16")
        return y
    _req(x, torch.float32, "x")
    if q8 is not None:
        check(_lib.lib().sc_layernorm_fwd_q8(x.data_ptr(), ldx if ldx is not None else d, gamma.data_ptr(),
                                             beta.data_ptr(), y.data_ptr(), ldy if ldy is not None else d, q8.data_ptr(),
                                             q8.stride(0), q8_scale_inv.data_ptr(), _ptr(mean), _ptr(rstd), rows, d, eps,
                                             _stream()), "sc_layernorm_fwd_q8")
        return y
    check(_lib.lib().sc_layernorm_fwd(x.data_ptr(), ldx if ldx is not None else d, gamma.data_ptr(), beta.data_ptr(),
                                      y.data_ptr(), ldy if ldy is not None else d, _ptr(mean), _ptr(rstd), rows, d, eps,
                                      _stream()), "sc_layernorm_fwd")
    return y


def gelu_bf16(u: torch.Tensor, h: torch.Tensor, quick: bool = False) -> torch.Tensor:
    """h = gelu(u) (bf16 -> bf16, contiguous), bit-identical to the GELU-pair GEMM epilogue's second output; ``quick``:
    QuickGELU (the SC_EPI_QGELU_PAIR epilogue's)."""
    _req(u, torch.bfloat16, "u"); _req(h, torch.bfloat16, "h")
    if not (u.is_contiguous() and h.is_contiguous()) or u.numel() != h.numel():
        raise ValueError("gelu_bf16: contiguous tensors of equal size required")
    fn = _lib.lib().sc_quick_gelu_bf16 if quick else _lib.lib().sc_gelu_bf16
    check(fn(u.data_ptr(), h.data_ptr(), u.numel(), _stream()), "sc_gelu_bf16")
    return h


def layernorm_bwd(dy, x, mean, rstd, gamma, dres, dres_bf16, dgamma, dbeta, colsum, rows: int, d: int, *,
                  accumulate, lddy=None, ldx=None, lddres=None, lddbf=None, ws=None, defer_reduce: bool = False,
                  q8: Optional[torch.Tensor] = None, q8_scale_inv: Optional[torch.Tensor] = None,
                  g_in: Optional[torch.Tensor] = None, ldgin=None, write_f32: bool = True, g16: bool = False, t8=None):
    """``accumulate``: False / True, or a negative int -P: only rows r % P == 0 of ``dres`` carry an incoming gradient.
    ``defer_reduce``: leave the per-block partial sums of dgamma / dbeta / colsum in ``ws`` (caller-owned, at least
    layernorm_bwd_ws_floats floats) and finish them with layernorm_bwd_reduce -- e.g. on the weight-gradient stream.
    ``g16`` (sc_layernorm_bwd_g16): the residual gradient travels in bf16 -- the incoming one is ``g_in`` (bf16) when
    ``accumulate`` is True, the outgoing one ``dres_bf16``; the fp32 ``dres`` is written only if ``write_f32``."""
    _req(dy, torch.bfloat16, "dy"); _req(dres, torch.float32, "dres")
    xb = x.dtype == torch.bfloat16          # residual stream kept in bf16
    _req(x, torch.bfloat16 if xb else torch.float32, "x")
    l = _lib.lib()
    if ws is None:
        if defer_reduce:
            raise _lib.SpatialClipHipError("layernorm_bwd: defer_reduce needs a caller-owned workspace")
        ws = workspace(l.sc_layernorm_bwd_ws_floats(rows, d), dy.device, "ln")
    legacy = xb and not g16                 # bf16 rows, fp32 gradient buffer read-modify-written as in sc_layernorm_bwd
    if legacy:
        g16, g_in, write_f32 = True, None, True
    if g16:
        if int(accumulate) > 0 and not legacy:
            _req(g_in, torch.bfloat16, "g_in")
        if dres_bf16 is not None or not legacy:
            _req(dres_bf16, torch.bfloat16, "dres_bf16")
        if q8 is not None:
            _req(q8_scale_inv, torch.float32, "q8_scale_inv")
        if t8 is not None:
            if not xb or q8 is None:
                raise _lib.SpatialClipHipError("layernorm_bwd: the per-tensor e4m3 copy exists for bf16 rows with the per-row copy (q8)")
            tp, tld, tsc, tam = _t8_args(t8, rows, d, "layernorm_bwd")
            check(l.sc_layernorm_bwd_x16_t8(dy.data_ptr(), lddy or d, x.data_ptr(), ldx or d, mean.data_ptr(), rstd.data_ptr(),
                                            gamma.data_ptr(), _ptr(g_in), ldgin or d, dres.data_ptr(), lddres or d, int(write_f32),
                                            _ptr(dres_bf16), lddbf or d, q8.data_ptr(), q8.stride(0), q8_scale_inv.data_ptr(),
                                            tp, tld, tsc, tam, int(accumulate), None if defer_reduce else dgamma.data_ptr(),
                                            dbeta.data_ptr(), _ptr(colsum), ws.data_ptr(), rows, d, _stream()),
                  "sc_layernorm_bwd_x16_t8")
            return
        fn = l.sc_layernorm_bwd_x16 if xb else l.sc_layernorm_bwd_g16
        check(fn(dy.data_ptr(), lddy or d, x.data_ptr(), ldx or d, mean.data_ptr(), rstd.data_ptr(),
                                     gamma.data_ptr(), _ptr(g_in), ldgin or d, dres.data_ptr(), lddres or d, int(write_f32),
                                     _ptr(dres_bf16), lddbf or d, _ptr(q8), q8.stride(0) if q8 is not None else 0,
                                     _ptr(q8_scale_inv), int(accumulate),
                                     None if defer_reduce else dgamma.data_ptr(), dbeta.data_ptr(), _ptr(colsum),
                                     ws.data_ptr(), rows, d, _stream()), "sc_layernorm_bwd_x16" if xb else "sc_layernorm_bwd_g16")
        return
    if q8 is not None:          # e4m3 copy of the new residual gradient + per-row 1/scale (A operand of the fp8 dgrad GEMMs)
        if q8.dtype != torch.uint8 or not q8.is_cuda or q8.stride(-1) != 1:
            raise TypeError("layernorm_bwd: q8 must be a device uint8 matrix")
        _req(q8_scale_inv, torch.float32, "q8_scale_inv")
        check(l.sc_layernorm_bwd_q8(dy.data_ptr(), lddy or d, x.data_ptr(), ldx or d, mean.data_ptr(), rstd.data_ptr(),
                                    gamma.data_ptr(), dres.data_ptr(), lddres or d, _ptr(dres_bf16), lddbf or d,
                                    q8.data_ptr(), q8.stride(0), q8_scale_inv.data_ptr(), int(accumulate),
                                    None if defer_reduce else dgamma.data_ptr(), dbeta.data_ptr(), _ptr(colsum),
                                    ws.data_ptr(), rows, d, _stream()), "sc_layernorm_bwd_q8")
        return
    check(l.sc_layernorm_bwd(dy.data_ptr(), lddy or d, x.data_ptr(), ldx or d, mean.data_ptr(), rstd.data_ptr(),
                             gamma.data_ptr(), dres.data_ptr(), lddres or d, _ptr(dres_bf16), lddbf or d,
                             int(accumulate), None if defer_reduce else dgamma.data_ptr(), dbeta.data_ptr(), _ptr(colsum),
                             ws.data_ptr(), rows, d, _stream()), "sc_layernorm_bwd")


def layernorm_bwd_ws_floats(rows: int, d: int) -> int:
    return int(_lib.lib().sc_layernorm_bwd_ws_floats(rows, d))


def layernorm_bwd_reduce(ws, dgamma, dbeta, colsum, rows: int, d: int):
    _req(ws, torch.float32, "ws")
    check(_lib.lib().sc_layernorm_bwd_reduce(ws.data_ptr(), rows, d, dgamma.data_ptr(), dbeta.data_ptr(), _ptr(colsum),
                                             _stream()), "sc_layernorm_bwd_reduce")


def bias_gelu_pair(x, bias, u, h, rows: int, n: int):
    _req(x, torch.float32, "x"); _req(u, torch.bfloat16, "u"); _req(h, torch.bfloat16, "h")
    check(_lib.lib().sc_bias_gelu_pair(x.data_ptr(), bias.data_ptr(), u.data_ptr(), h.data_ptr(), rows, n, _stream()),
          "sc_bias_gelu_pair")


def colsum_bf16(x, rows: int, n: int, out, ld: Optional[int] = None):
    _req(x, torch.bfloat16, "x"); _req(out, torch.float32, "out")
    l = _lib.lib()
    ws = workspace(l.sc_colsum_ws_floats(rows, n), x.device, "colsum")
    check(l.sc_colsum_bf16(x.data_ptr(), ld or x.stride(0), rows, n, out.data_ptr(), ws.data_ptr(), _stream()),
          "sc_colsum_bf16")
    return out


def l2norm_fwd(x, y, y_bf16, inv, rows: int, d: int):
    check(_lib.lib().sc_l2norm_fwd(x.data_ptr(), y.data_ptr(), _ptr(y_bf16), _ptr(inv), rows, d, _stream()),
          "sc_l2norm_fwd")
    return y


def l2norm_bwd(dy, y, inv, dx_bf16, rows: int, d: int):
    check(_lib.lib().sc_l2norm_bwd(dy.data_ptr(), y.data_ptr(), inv.data_ptr(), dx_bf16.data_ptr(), rows, d, _stream()),
          "sc_l2norm_bwd")
    return dx_bf16


def cast_pad_bf16(src, dst, rows: int, cols: int, cols_pad: int, ld_src=None, ld_dst=None):
    _req(src, torch.float32, "src"); _req(dst, torch.bfloat16, "dst")
    check(_lib.lib().sc_cast_pad_bf16(src.data_ptr(), ld_src or cols, dst.data_ptr(), ld_dst or cols_pad, rows, cols,
                                      cols_pad, _stream()), "sc_cast_pad_bf16")
    return dst


def cast_transpose_bf16(src, dst, rows: int, cols: int, ld_dst=None):
    _req(src, torch.float32, "src"); _req(dst, torch.bfloat16, "dst")
    check(_lib.lib().sc_cast_transpose_bf16(src.data_ptr(), dst.data_ptr(), rows, cols, ld_dst or rows, _stream()),
          "sc_cast_transpose_bf16")
    return dst


# ------------------------------------------------------------------------------------------ patch embedding
def _req_keep(keep, B: int, K: int, name: str = "keep") -> None:
    _req(keep, torch.int32, name)
    if tuple(keep.shape) != (B, K) or not keep.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 [{B}, {K}] tensor, got {tuple(keep.shape)}")


def patch_keep(seed: int, draw: int, sample0: int, B: int, n: int, K: int, keep=None, slot=None, device=None):
    """FLIP patch dropout: (keep int32 [B, K] ascending, slot int32 [B, n]) of draw ``draw`` for samples sample0 .. sample0 + B - 1
    (sc_patch_keep; patch_dropout.keep_indices_host gives the same bits on the host)."""
    if keep is None:
        keep = torch.empty((B, K), dtype=torch.int32, device=device or "cuda")
    if slot is None:
        slot = torch.empty((B, n), dtype=torch.int32, device=keep.device)
    _req_keep(keep, B, K)
    _req_keep(slot, B, n, "slot")
    check(_lib.lib().sc_patch_keep(keep.data_ptr(), slot.data_ptr(), int(seed), int(draw), int(sample0), B, n, K, _stream()),
          "sc_patch_keep")
    return keep, slot


def im2col(images, patches, P: int, ld_out: Optional[int] = None, keep=None):
    """``keep`` (int32 [B, K], FLIP patch dropout): only the kept patches' rows, [B*K, ld_out] (sc_im2col_keep)."""
    _req(images, torch.float32, "images"); _req(patches, torch.bfloat16, "patches")
    B, C, H, W = images.shape
    if not images.is_contiguous():
        raise ValueError("images must be contiguous NCHW")
    if keep is not None:
        K = keep.shape[1]
        _req_keep(keep, B, K)
        if patches.shape[0] < B * K:
            raise ValueError(f"patches: {B * K} rows needed, got {patches.shape[0]}")
        check(_lib.lib().sc_im2col_keep(images.data_ptr(), keep.data_ptr(), patches.data_ptr(), B, K, C, H, W, P,
                                        ld_out or patches.stride(0), _stream()), "sc_im2col_keep")
        return patches
    check(_lib.lib().sc_im2col(images.data_ptr(), patches.data_ptr(), B, C, H, W, P, ld_out or patches.stride(0),
                               _stream()), "sc_im2col")
    return patches


def embed_ln_fwd(patch_out, cls, pos, gamma, beta, x, mean, rstd, B: int, L: int, d: int, eps: float = 1e-5, keep=None):
    """class token + positional embedding + ln_pre -> the residual stream ``x`` [B*L, d]: fp32, or bf16 (sc_embed_ln_fwd_x16)
    when the stream is kept in bf16.  ``keep`` (int32 [B, L - 1], FLIP patch dropout): ``patch_out`` holds the kept patches'
    rows only and token t > 0 takes position keep[b, t - 1] + 1 of ``pos`` (sc_embed_ln_fwd_keep / _keep_x16).
    ``gamma`` None (a tower built with ``no_ln_pre``): no LayerNorm, ``x`` = class token / patch rows + positions; ``beta``,
    ``mean`` and ``rstd`` are ignored (may be None) and never written."""
    x16 = x.dtype == torch.bfloat16
    if gamma is None:
        beta = None
    _req(x, torch.bfloat16 if x16 else torch.float32, "x")
    if keep is not None:
        _req_keep(keep, B, L - 1)
        what = "sc_embed_ln_fwd_keep_x16" if x16 else "sc_embed_ln_fwd_keep"
        check(getattr(_lib.lib(), what)(patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), keep.data_ptr(), _ptr(gamma),
                                        _ptr(beta), x.data_ptr(), _ptr(mean), _ptr(rstd), B, L,
                                        pos.shape[0] - 1, d, float(eps), _stream()), what)
        return x
    if x16:
        fn, what = _lib.lib().sc_embed_ln_fwd_x16, "sc_embed_ln_fwd_x16"
    else:
        fn, what = _lib.lib().sc_embed_ln_fwd, "sc_embed_ln_fwd"
    check(fn(patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), _ptr(gamma), _ptr(beta), x.data_ptr(),
             _ptr(mean), _ptr(rstd), B, L, d, float(eps), _stream()), what)
    return x


def embed_ln_bwd(dres, patch_out, cls, pos, mean, rstd, gamma, dpatch_bf16, dgamma, dbeta, dpos, dcls, B, L, d, keep=None,
                 slot=None):
    """``keep`` / ``slot`` (int32 [B, L - 1] / [B, n], FLIP patch dropout): the backward of the dropping forward at L = K + 1
    tokens; ``dpos`` has all n + 1 rows, exact zeros where no sample kept the patch (sc_embed_ln_bwd_keep).
    ``gamma`` None (``no_ln_pre``): d(token) is ``dres`` itself, left untouched; ``dpatch_bf16`` is the bf16 rounding of its
    rows t > 0; ``mean`` / ``rstd`` / ``dgamma`` / ``dbeta`` are ignored (may be None), no workspace is used."""
    l = _lib.lib()
    if gamma is None:
        mean = rstd = dgamma = dbeta = ws = None
    else:
        ws = workspace(l.sc_embed_ln_bwd_ws_floats(B, L, d), dres.device, "embed")
    if keep is not None:
        n = pos.shape[0] - 1
        _req_keep(keep, B, L - 1)
        if slot is None:
            raise ValueError("embed_ln_bwd(keep=...) needs the inverse map slot [B, n] as well")
        _req_keep(slot, B, n, "slot")
        if dpos.numel() != (n + 1) * d:
            raise ValueError(f"dpos: expected {(n + 1) * d} elements, got {dpos.numel()}")
        check(l.sc_embed_ln_bwd_keep(dres.data_ptr(), patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), keep.data_ptr(),
                                     slot.data_ptr(), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                     dpatch_bf16.data_ptr(), _ptr(dgamma), _ptr(dbeta), dpos.data_ptr(),
                                     dcls.data_ptr(), _ptr(ws), B, L, n, d, _stream()), "sc_embed_ln_bwd_keep")
        return
    check(l.sc_embed_ln_bwd(dres.data_ptr(), patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), _ptr(mean),
                            _ptr(rstd), _ptr(gamma), dpatch_bf16.data_ptr(), _ptr(dgamma),
                            _ptr(dbeta), dpos.data_ptr(), dcls.data_ptr(), _ptr(ws), B, L, d, _stream()),
          "sc_embed_ln_bwd")


# ------------------------------------------------------------------------------------------ token mean pooling
def _req_rows(t: torch.Tensor, name: str) -> bool:
    """bf16 or fp32 contiguous device rows -> is it bf16?"""
    if t.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: expected bfloat16 or float32, got {t.dtype}")
    _req(t, t.dtype, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t.dtype == torch.bfloat16


def token_pool_fwd(x, B: int, L: int, t0: int, d: int, mean_f32=None, mean_bf16=None):
    """mean[b] = mean over tokens t >= t0 of the contiguous rows ``x`` [B, L, d] (bf16 or fp32), fp32 accumulation in a fixed
    order; written to ``mean_f32`` [B, d] and / or ``mean_bf16`` [B, d] (sc_token_pool_fwd)."""
    xb = _req_rows(x, "x")
    if x.numel() != B * L * d:
        raise ValueError(f"x: expected {B * L * d} elements, got {x.numel()}")
    for t, dt, name in ((mean_f32, torch.float32, "mean_f32"), (mean_bf16, torch.bfloat16, "mean_bf16")):
        if t is not None:
            _req(t, dt, name)
            if t.numel() != B * d or not t.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous [{B}, {d}] tensor")
    check(_lib.lib().sc_token_pool_fwd(x.data_ptr(), int(xb), B, L, t0, d, _ptr(mean_f32), _ptr(mean_bf16), _stream()),
          "sc_token_pool_fwd")
    return mean_f32 if mean_f32 is not None else mean_bf16


def token_pool_bwd(d_mean, B: int, L: int, t0: int, d: int, dx_f32=None, dx_bf16=None):
    """Backward of token_pool_fwd into contiguous [B, L, d] rows: exact zeros for t < t0, ``d_mean / (L - t0)`` elsewhere, as
    fp32 (``dx_f32``) and / or its bf16 rounding (``dx_bf16``).  Every element is written (sc_token_pool_bwd)."""
    db = _req_rows(d_mean, "d_mean")
    if d_mean.numel() != B * d:
        raise ValueError(f"d_mean: expected {B * d} elements, got {d_mean.numel()}")
    for t, dt, name in ((dx_f32, torch.float32, "dx_f32"), (dx_bf16, torch.bfloat16, "dx_bf16")):
        if t is not None:
            _req(t, dt, name)
            if t.numel() != B * L * d or not t.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous [{B}, {L}, {d}] tensor")
    check(_lib.lib().sc_token_pool_bwd(d_mean.data_ptr(), int(db), B, L, t0, d, _ptr(dx_f32), _ptr(dx_bf16), _stream()),
          "sc_token_pool_bwd")


# ------------------------------------------------------------------------------------------ contrastive head
def sgemm(a, sam, sak, b, sbn, sbk, c, ldc, M, N, K, accumulate=False):
    check(_lib.lib().sc_sgemm_f32(a.data_ptr(), sam, sak, b.data_ptr(), sbn, sbk, c.data_ptr(), ldc, M, N, K,
                                  int(accumulate), _stream()), "sc_sgemm_f32")
    return c


class _SgemmDesc(ctypes.Structure):
    """``sc_sgemm_desc`` of include/spatial_clip_hip.h (host-side problem descriptor)."""
    _fields_ = [("A", ctypes.c_void_p), ("sam", ctypes.c_longlong), ("sak", ctypes.c_longlong),
                ("B", ctypes.c_void_p), ("sbn", ctypes.c_longlong), ("sbk", ctypes.c_longlong),
                ("C", ctypes.c_void_p), ("ldc", ctypes.c_longlong),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("accumulate", ctypes.c_int)]


SGEMM_MAX_GROUP = 6


def sgemm_grouped(problems) -> None:
    """Several independent fp32 GEMMs in one launch.  ``problems``: iterable of
    (a, sam, sak, b, sbn, sbk, c, ldc, M, N, K[, accumulate]) exactly as for :func:`sgemm`."""
    problems = list(problems)
    if not 1 <= len(problems) <= SGEMM_MAX_GROUP:
        raise ValueError(f"sgemm_grouped: 1..{SGEMM_MAX_GROUP} problems, got {len(problems)}")
    arr = (_SgemmDesc * len(problems))()
    for d, p in zip(arr, problems):
        a, sam, sak, b, sbn, sbk, c, ldc, M, N, K = p[:11]
        for t_, n in ((a, "a"), (b, "b"), (c, "c")):
            if not t_.is_cuda or t_.dtype != torch.float32:
                raise TypeError(f"sgemm_grouped: {n} must be a device fp32 tensor")
        d.A, d.sam, d.sak = a.data_ptr(), sam, sak
        d.B, d.sbn, d.sbk = b.data_ptr(), sbn, sbk
        d.C, d.ldc = c.data_ptr(), ldc
        d.M, d.N, d.K, d.accumulate = M, N, K, int(p[11]) if len(p) > 11 else 0
    check(_lib.lib().sc_sgemm_f32_grouped(ctypes.cast(arr, ctypes.c_void_p), len(problems), _stream()),
          "sc_sgemm_f32_grouped")


def pack_rows(feat: torch.Tensor, ids_a: Optional[torch.Tensor], ids_b: Optional[torch.Tensor],
              out: torch.Tensor) -> torch.Tensor:
    """out[B, D(+4)] = feat | ids_a | ids_b (int64 through two float slots each): all-gather send buffer."""
    _req(feat, torch.float32, "feat"); _req(out, torch.float32, "out")
    if ids_a is not None:
        _req(ids_a, torch.int64, "ids_a"); _req(ids_b, torch.int64, "ids_b")
        if not (ids_a.is_contiguous() and ids_b.is_contiguous()):
            raise ValueError("pack_rows: id vectors must be contiguous")
    B, D = feat.shape
    check(_lib.lib().sc_pack_rows(feat.data_ptr(), feat.stride(0), _ptr(ids_a), _ptr(ids_b), out.data_ptr(),
                                  out.stride(0), B, D, _stream()), "sc_pack_rows")
    return out


def _req_buf(what: str, t: torch.Tensor, dtype, n: int, name: str) -> None:
    """What a raw pointer of the loss kernels stands for: a contiguous device tensor of ``dtype`` with at least ``n`` elements
    (host shape arithmetic only: nothing is launched and nothing synchronises)."""
    _req(t, dtype, name)
    if not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of at least {n} elements, got shape "
                         f"{tuple(t.shape)}, strides {tuple(t.stride())}")


def _req_scalar(what: str, t: Optional[torch.Tensor], name: str, optional: bool = False, exact: bool = True) -> None:
    """A device scalar: fp32, one element (``exact``) or a slot of at least one element the kernel writes its result to."""
    if t is None:
        if optional:
            return
        raise ValueError(f"{what}: {name} is missing")
    _req(t, torch.float32, name)
    if (t.numel() != 1) if exact else (t.numel() < 1 or not t.is_contiguous()):
        raise ValueError(f"{what}: {name} must be a one-element fp32 tensor, got shape {tuple(t.shape)}")


def _req_dims(what: str, **dims) -> None:
    for k, v in dims.items():
        if int(v) != v or v < 0:
            raise ValueError(f"{what}: {k} must be a non-negative int, got {v!r}")


def _req_labels(what: str, lab_col, lab_w, B: int, nlab: int) -> None:
    _req_buf(what, lab_col, torch.int32, 2 * B * nlab, "lab_col")
    _req_buf(what, lab_w, torch.float32, 2 * B * nlab, "lab_w")


def neighbor_join(all_img_ids, all_txt_ids, nbr_ids, nbr_alpha, B, G, K, rank, alpha_scale, lab_col, lab_w):
    """Sparse soft labels lab_col / lab_w [2, B, K + 1] from the tile-id join (``sc_neighbor_join``): the gathered id vectors hold
    G int64 ids, ``nbr_ids`` (int64) and ``nbr_alpha`` (fp32) are [B, K]."""
    what = "neighbor_join"
    _req_dims(what, B=B, G=G, K=K, rank=rank)
    _req_buf(what, all_img_ids, torch.int64, G, "all_image_tile_ids")
    _req_buf(what, all_txt_ids, torch.int64, G, "all_text_tile_ids")
    _req_buf(what, nbr_ids, torch.int64, B * K, "neighbor_tile_ids")
    _req_buf(what, nbr_alpha, torch.float32, B * K, "neighbor_alphas")
    _req_labels(what, lab_col, lab_w, B, K + 1)
    check(_lib.lib().sc_neighbor_join(all_img_ids.data_ptr(), all_txt_ids.data_ptr(), nbr_ids.data_ptr(),
                                      nbr_alpha.data_ptr(), B, G, K, rank, float(alpha_scale), lab_col.data_ptr(),
                                      lab_w.data_ptr(), _stream()), "sc_neighbor_join")


def onehot_labels(B, rank, lab_col, lab_w):
    _req_dims("onehot_labels", B=B, rank=rank)
    _req_labels("onehot_labels", lab_col, lab_w, B, 1)
    check(_lib.lib().sc_onehot_labels(B, rank, lab_col.data_ptr(), lab_w.data_ptr(), _stream()), "sc_onehot_labels")


def contrastive_loss_fwd(z, B, G, scale, cap, bias, lab_col, lab_w, nlab, w, rowstats, loss_out):
    """ClipLoss / SpatialLoss rows pass + finalize on z [2, B, G]: rowstats [2B, 4], loss_out [4] (all fp32, contiguous)."""
    what = "contrastive_loss_fwd"
    _req_dims(what, B=B, G=G, nlab=nlab)
    _req_buf(what, z, torch.float32, 2 * B * G, "z")
    _req_scalar(what, scale, "logit_scale"); _req_scalar(what, bias, "logit_bias", optional=True)
    _req_labels(what, lab_col, lab_w, B, nlab)
    _req_buf(what, rowstats, torch.float32, 8 * B, "rowstats")
    _req_buf(what, loss_out, torch.float32, 4, "loss_out")
    check(_lib.lib().sc_contrastive_loss_fwd(z.data_ptr(), B, G, scale.data_ptr(), float(cap), _ptr(bias),
                                             lab_col.data_ptr(), lab_w.data_ptr(), nlab, float(w),
                                             rowstats.data_ptr(), loss_out.data_ptr(), _stream()),
          "sc_contrastive_loss_fwd")


def contrastive_loss_bwd(z, B, G, scale, cap, bias, lab_col, lab_w, nlab, w, rowstats, loss_out, grad_out, rowgrad,
                         dscale, dbias):
    """Backward of ``contrastive_loss_fwd``: z <- dz in place, rowgrad [2B, 2], d_scale / d_bias (optional one-element slots);
    ``grad_out``: the upstream gradient as a one-element device tensor, or None for 1."""
    what = "contrastive_loss_bwd"
    _req_dims(what, B=B, G=G, nlab=nlab)
    _req_buf(what, z, torch.float32, 2 * B * G, "z")
    _req_scalar(what, scale, "logit_scale"); _req_scalar(what, bias, "logit_bias", optional=True)
    _req_scalar(what, grad_out, "grad_out", optional=True)
    _req_labels(what, lab_col, lab_w, B, nlab)
    _req_buf(what, rowstats, torch.float32, 8 * B, "rowstats")
    _req_buf(what, loss_out, torch.float32, 4, "loss_out")
    _req_buf(what, rowgrad, torch.float32, 4 * B, "rowgrad")
    _req_scalar(what, dscale, "dscale", optional=True, exact=False); _req_scalar(what, dbias, "dbias", optional=True, exact=False)
    check(_lib.lib().sc_contrastive_loss_bwd(z.data_ptr(), B, G, scale.data_ptr(), float(cap), _ptr(bias),
                                             lab_col.data_ptr(), lab_w.data_ptr(), nlab, float(w),
                                             rowstats.data_ptr(), loss_out.data_ptr(), _ptr(grad_out),
                                             rowgrad.data_ptr(), _ptr(dscale), _ptr(dbias), _stream()),
          "sc_contrastive_loss_bwd")


def recall_hits(z_img_rows, G, B, col0, hits3):
    """R@1/5/10 hit counters (int32 [3], added onto) of B rows of row stride G whose diagonal block starts at column col0."""
    what = "recall_hits"
    _req_dims(what, G=G, B=B, col0=col0)
    _req_buf(what, z_img_rows, torch.float32, max(B - 1, 0) * G + col0 + B, "z_image_rows")
    _req_buf(what, hits3, torch.int32, 3, "hits3")
    check(_lib.lib().sc_recall_hits(z_img_rows.data_ptr(), G, B, col0, hits3.data_ptr(), _stream()), "sc_recall_hits")


def retrieval_ranks(image_feat, text_feat, row0: int = 0, M: Optional[int] = None, rank_i2t=None, cnt_t2i=None):
    """Full-set retrieval ranks of the pairs (image_feat[i], text_feat[i]), both fp32 [N, D] with any row stride >= D
    (``sc_retrieval_ranks``; the N x N similarities are never stored).  For the rows i of [row0, row0 + M) (M None: up to N)
    against all N columns, with z_ij = <image_i, text_j> and d_i = z_ii:
    ``rank_i2t`` (int32 [M], written) = #{j != i: z_ij > d_i or (z_ij == d_i and j < i)}; ``cnt_t2i`` (int32 [N], ADDED onto;
    a zeroed one is made when None) += #{i in block, i != j: z_ij > d_j or (z_ij == d_j and i < j)}: summed over row blocks
    that partition [0, N) it is the text->image rank.  Returns ``(rank_i2t, cnt_t2i)``."""
    what = "retrieval_ranks"
    _req(image_feat, torch.float32, "image_feat"); _req(text_feat, torch.float32, "text_feat")
    if image_feat.dim() != 2 or text_feat.shape != image_feat.shape or image_feat.shape[0] < 1 or image_feat.shape[1] < 1:
        raise ValueError(f"{what}: image_feat and text_feat must be [N, D] of one shape with N, D >= 1, got "
                         f"{tuple(image_feat.shape)} and {tuple(text_feat.shape)}")
    N, D = image_feat.shape
    for t_, n in ((image_feat, "image_feat"), (text_feat, "text_feat")):
        if N > 1 and t_.stride(0) < D:
            raise ValueError(f"{what}: {n} rows overlap (row stride {t_.stride(0)} < D = {D})")
    if M is None:
        M = N - row0
    _req_dims(what, row0=row0, M=M)
    if rank_i2t is None:
        rank_i2t = torch.empty(M, dtype=torch.int32, device=image_feat.device)
    if cnt_t2i is None:
        cnt_t2i = torch.zeros(N, dtype=torch.int32, device=image_feat.device)
    _req_buf(what, rank_i2t, torch.int32, M, "rank_i2t")
    _req_buf(what, cnt_t2i, torch.int32, N, "cnt_t2i")
    ld_i = image_feat.stride(0) if N > 1 else D
    ld_t = text_feat.stride(0) if N > 1 else D
    check(_lib.lib().sc_retrieval_ranks(image_feat.data_ptr(), ld_i, text_feat.data_ptr(), ld_t, N, D, row0, M,
                                        rank_i2t.data_ptr(), cnt_t2i.data_ptr(), _stream()), "sc_retrieval_ranks")
    return rank_i2t, cnt_t2i


def group_cache_put(image_features, text_features, image_cache, text_cache, j: int, N: int, image_tile_ids=None,
                    text_tile_ids=None, neighbor_tile_ids=None, neighbor_alphas=None, image_id_cache=None, text_id_cache=None,
                    neighbor_id_cache=None, neighbor_alpha_cache=None) -> None:
    """Row block ``j`` of the group caches of ``Trainer(accum_freq=N)`` <- one micro-batch (``sc_group_cache_put``, one
    launch): ``image_features`` / ``text_features`` fp32 [B, D] (any row stride >= D) into ``image_cache`` / ``text_cache``
    [N*B, D]; the int64 id vectors [B] into ``*_id_cache`` [N*B]; ``neighbor_tile_ids`` (int64) / ``neighbor_alphas`` (fp32)
    [B, K] into their [N*B, K] caches.  Ids and neighbours may be None (ClipLoss, SigLipLoss); K may be 0."""
    _req(image_features, torch.float32, "image_features"); _req(text_features, torch.float32, "text_features")
    B, D = image_features.shape
    if tuple(text_features.shape) != (B, D):
        raise ValueError(f"group_cache_put: text_features {tuple(text_features.shape)} against image_features {(B, D)}")
    G = int(N) * B
    K = 0 if neighbor_tile_ids is None else int(neighbor_tile_ids.shape[1])
    if K == 0:      # [B, 0] matrices carry nothing: the neighbour caches are not touched
        neighbor_tile_ids = neighbor_alphas = neighbor_id_cache = neighbor_alpha_cache = None

    def want(t, dtype, shape, name, optional=False):
        if t is None:
            if optional:
                return
            raise ValueError(f"group_cache_put: {name} is missing")
        _req(t, dtype, name)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"group_cache_put: {name}: expected a contiguous {dtype} {shape}, got {tuple(t.shape)}")
    want(image_cache, torch.float32, (G, D), "image_cache"); want(text_cache, torch.float32, (G, D), "text_cache")
    for src, cache, dtype, shp, name in ((image_tile_ids, image_id_cache, torch.int64, (), "image_tile_ids"),
                                         (text_tile_ids, text_id_cache, torch.int64, (), "text_tile_ids"),
                                         (neighbor_tile_ids, neighbor_id_cache, torch.int64, (K,), "neighbor_tile_ids"),
                                         (neighbor_alphas, neighbor_alpha_cache, torch.float32, (K,), "neighbor_alphas")):
        want(src, dtype, (B,) + shp, name, optional=True)
        if src is not None and (K > 0 or not shp):
            want(cache, dtype, (G,) + shp, name + " cache")
    check(_lib.lib().sc_group_cache_put(
        image_features.data_ptr(), image_features.stride(0), text_features.data_ptr(), text_features.stride(0),
        _ptr(image_tile_ids), _ptr(text_tile_ids), _ptr(neighbor_tile_ids), _ptr(neighbor_alphas), image_cache.data_ptr(),
        text_cache.data_ptr(), _ptr(image_id_cache), _ptr(text_id_cache), _ptr(neighbor_id_cache), _ptr(neighbor_alpha_cache),
        B, D, K, int(j), int(N), _stream()), "sc_group_cache_put")


def siglip_loss(z, B, G, col0, scale, bias, rowpart, loss_out, dscale, dbias, hits3=None):
    """SigLIP rows pass + finalize: z [B, G] <- dz in place, rowpart [B, 3]; loss_out / dscale / dbias: optional one-element
    slots; ``hits3``: optional int32 [3] recall counters, read from z before it is overwritten."""
    what = "siglip_loss"
    _req_dims(what, B=B, G=G, col0=col0)
    _req_buf(what, z, torch.float32, B * G, "z")
    _req_scalar(what, scale, "logit_scale"); _req_scalar(what, bias, "logit_bias", optional=True)
    _req_buf(what, rowpart, torch.float32, 3 * B, "rowpart")
    for t_, n in ((loss_out, "loss_out"), (dscale, "dscale"), (dbias, "dbias")):
        _req_scalar(what, t_, n, optional=True, exact=False)
    if hits3 is not None:
        _req_buf(what, hits3, torch.int32, 3, "hits3")
    check(_lib.lib().sc_siglip_loss(z.data_ptr(), B, G, col0, scale.data_ptr(), _ptr(bias), rowpart.data_ptr(),
                                    _ptr(loss_out), _ptr(dscale), _ptr(dbias), _ptr(hits3), _stream()),
          "sc_siglip_loss")


def distill_resident_max_g() -> int:
    """Longest row (G) the distillation rows kernel keeps in registers (SC_DISTILL_RESIDENT_MAX_G); longer rows are re-read."""
    return int(_lib.lib().sc_distill_resident_max_g())


def distill_loss(z_s, z_t, B, G, col0, scale, dist_scale, rowpart, loss_out, dscale_c, dscale_d, hits3=None):
    """DistillClipLoss rows pass + finalize: z_s <- dz_c, z_t <- dz_d (both [2, B, G] fp32, contiguous)."""
    _req(z_s, torch.float32, "z_s"); _req(z_t, torch.float32, "z_t"); _req(rowpart, torch.float32, "rowpart")
    _req(scale, torch.float32, "logit_scale"); _req(dist_scale, torch.float32, "dist_logit_scale")
    _req(loss_out, torch.float32, "loss_out")
    if tuple(z_s.shape) != (2, B, G) or tuple(z_t.shape) != (2, B, G) or not (z_s.is_contiguous() and z_t.is_contiguous()):
        raise ValueError(f"distill_loss: z_s and z_t must be contiguous [2, {B}, {G}] tensors")
    if rowpart.numel() < 8 * B or not rowpart.is_contiguous() or loss_out.numel() < 4 or not loss_out.is_contiguous():
        raise ValueError("distill_loss: rowpart must hold [2B, 4] and loss_out 4 contiguous floats")
    if scale.numel() != 1 or dist_scale.numel() != 1:
        raise ValueError("distill_loss: the scales are one-element tensors")
    if hits3 is not None:
        _req(hits3, torch.int32, "recall_hits")
    check(_lib.lib().sc_distill_loss(z_s.data_ptr(), z_t.data_ptr(), B, G, col0, scale.data_ptr(), dist_scale.data_ptr(),
                                     rowpart.data_ptr(), loss_out.data_ptr(), _ptr(dscale_c), _ptr(dscale_d),
                                     _ptr(hits3), _stream()), "sc_distill_loss")


def axpby_scalars(a: torch.Tensor, ga: torch.Tensor, b: torch.Tensor, gb: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = ga * a + gb * b (ga, gb: one-element device tensors); contiguous fp32 of equal size."""
    for t_, n in ((a, "a"), (ga, "ga"), (b, "b"), (gb, "gb"), (out, "out")):
        _req(t_, torch.float32, n)
    if not (a.is_contiguous() and b.is_contiguous() and out.is_contiguous()) or a.numel() != out.numel() \
            or b.numel() != out.numel() or ga.numel() != 1 or gb.numel() != 1:
        raise ValueError("axpby_scalars: contiguous tensors of equal size and one-element factors required")
    check(_lib.lib().sc_axpby_scalars(a.data_ptr(), ga.data_ptr(), b.data_ptr(), gb.data_ptr(), out.data_ptr(),
                                      a.numel(), _stream()), "sc_axpby_scalars")
    return out


def exp_scalar(x, y):
    check(_lib.lib().sc_exp_scalar(x.data_ptr(), y.data_ptr(), _stream()), "sc_exp_scalar")
    return y


def scale_by_scalar(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = x * s (s: one-element device tensor); contiguous fp32."""
    _req(x, torch.float32, "x"); _req(s, torch.float32, "s"); _req(out, torch.float32, "out")
    if not (x.is_contiguous() and out.is_contiguous()) or x.numel() != out.numel() or s.numel() != 1:
        raise ValueError("scale_by_scalar: contiguous tensors of equal size and a one-element scale required")
    check(_lib.lib().sc_scale_by_scalar(x.data_ptr(), s.data_ptr(), out.data_ptr(), x.numel(), _stream()), "sc_scale_by_scalar")
    return out


def exp_scalar_bwd(y, dy, dx, mult: float = 1.0):
    check(_lib.lib().sc_exp_scalar_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), float(mult), _stream()),
          "sc_exp_scalar_bwd")


# ------------------------------------------------------------------------------------------ optimiser
def grad_norm(grads, n, grad_scale, max_norm, out2):
    ws = workspace(1024, grads.device, "gn", torch.float64)
    check(_lib.lib().sc_grad_norm(grads.data_ptr(), n, float(grad_scale), float(max_norm), ws.data_ptr(),
                                  out2.data_ptr(), _stream()), "sc_grad_norm")
    return out2


def grad_sumsq_partial(grads, n, partial1024):
    """1024 fp64 partial sums of squares of grads[:n] (one contiguous piece of a rank's gradient shard)."""
    _req(grads, torch.float32, "grads"); _req(partial1024, torch.float64, "partial")
    check(_lib.lib().sc_grad_sumsq_partial(grads.data_ptr(), int(n), partial1024.data_ptr(), _stream()), "sc_grad_sumsq_partial")


def grad_norm_final(partial, n_partial, grad_scale, max_norm, out2):
    """out2 = {norm * grad_scale, clip coefficient} from (all-reduced) fp64 partial sums of squares."""
    _req(partial, torch.float64, "partial")
    check(_lib.lib().sc_grad_norm_final(partial.data_ptr(), int(n_partial), float(grad_scale), float(max_norm), out2.data_ptr(),
                                        _stream()), "sc_grad_norm_final")
    return out2


def grad_accumulate(acc, grads, n, scale, mode, partial=None):
    """One micro-batch folded into the running gradient sum (``sc_grad_accumulate``): mode 0 ``acc = scale * grads``, mode 1
    ``acc += scale * grads``, mode 2 ``grads = acc + scale * grads`` (``acc=None``: ``grads *= scale``) with, if ``partial``
    (1024 fp64) is given, the partial sums of squares of the new ``grads`` for ``grad_norm_final``.  Product and sum are rounded
    separately.  Host tensors evaluate the same expressions with torch (tests of the schedule and of the gloo route; not a
    product path: no model runs on the host)."""
    n, mode = int(n), int(mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"grad_accumulate: mode {mode!r}: 0 (first), 1 (add) or 2 (last)")
    if acc is None and mode != 2:
        raise ValueError(f"grad_accumulate: mode {mode} writes acc, which is None")
    if partial is not None and mode != 2:
        raise ValueError("grad_accumulate: partial sums of squares belong to the summed gradient (mode 2)")
    for t, name in ((grads, "grads"), (acc, "acc")):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError(f"grad_accumulate: {name}: expected torch.float32, got {t.dtype}")
        if not t.is_contiguous() or t.numel() < n or n < 0:
            raise ValueError(f"grad_accumulate: {name} must be contiguous and hold n = {n} floats")
        if t.device != grads.device:
            raise ValueError("grad_accumulate: acc and grads live on different devices")
    if partial is not None and (partial.dtype != torch.float64 or partial.numel() < 1024 or not partial.is_contiguous()
                                or partial.device != grads.device):
        raise ValueError("grad_accumulate: partial must be 1024 contiguous float64 on the gradient's device")
    if not grads.is_cuda:
        g = grads.view(-1)[:n]
        prod = g * float(scale)                         # one rounding ...
        if mode == 2:
            g.copy_(prod if acc is None else acc.view(-1)[:n] + prod)     # ... and the other
            if partial is not None:
                partial[:1024].zero_()
                partial[0] = g.double().square().sum()
        else:
            acc.view(-1)[:n].copy_(prod if mode == 0 else acc.view(-1)[:n] + prod)
        return
    check(_lib.lib().sc_grad_accumulate(_ptr(acc), grads.data_ptr(), n, float(scale), mode, _ptr(partial), _stream()),
          "sc_grad_accumulate")


WAVG_SKIP, WAVG_COPY, WAVG_EMA, WAVG_MEAN = range(4)


def _wavg_pair(what: str, x, y, n: int, names) -> None:
    for t, name in ((x, names[0]), (y, names[1])):
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name}: expected torch.float32, got {t.dtype}")
        if not t.is_contiguous() or n < 0 or t.numel() < n:
            raise ValueError(f"{what}: {name} must be contiguous and hold n = {n} floats")
    if x.device != y.device:
        raise ValueError(f"{what}: {names[0]} and {names[1]} live on different devices")


def weight_average(avg, params, n, op, a=0.0, b=0.0):
    """One update of the averaged weights (``sc_weight_average``): ``WAVG_COPY`` ``avg = params``, ``WAVG_EMA``
    ``avg = a * avg + b * params`` (a = decay, b = 1 - decay), ``WAVG_MEAN`` ``avg = avg + (params - avg) / a``
    (a = n_averaged + 1), ``WAVG_SKIP`` nothing.  Every operation is rounded to fp32 on its own.  Host tensors evaluate the same
    expressions with torch (tests of the schedule and the checkpoint layout; not a product path)."""
    n, op = int(n), int(op)
    if op not in (WAVG_SKIP, WAVG_COPY, WAVG_EMA, WAVG_MEAN):
        raise ValueError(f"weight_average: op {op!r}: WAVG_SKIP, WAVG_COPY, WAVG_EMA or WAVG_MEAN")
    _wavg_pair("weight_average", avg, params, n, ("avg", "params"))
    if not avg.is_cuda:
        if op == WAVG_SKIP or n == 0:
            return
        v, p = avg.view(-1)[:n], params.view(-1)[:n]
        if op == WAVG_COPY:
            v.copy_(p)
        elif op == WAVG_EMA:
            a32, b32 = torch.tensor(float(a), dtype=torch.float32), torch.tensor(float(b), dtype=torch.float32)
            v.copy_(a32 * v + b32 * p)
        else:
            v.copy_(v + (p - v) / torch.tensor(float(a), dtype=torch.float32))
        return
    check(_lib.lib().sc_weight_average(avg.data_ptr(), params.data_ptr(), n, op, float(a), float(b), _stream()),
          "sc_weight_average")


def weight_average_dev(avg, params, n, ctl):
    """The same update with ``{int32 op, float32 a, float32 b}`` read from the device block ``ctl`` (3 x 4 bytes; an int32
    tensor whose second and third word hold the floats' bits): the launch a captured graph replays.  ``op == WAVG_SKIP``
    touches nothing."""
    n = int(n)
    _wavg_pair("weight_average_dev", avg, params, n, ("avg", "params"))
    _req(avg, torch.float32, "avg")
    if ctl.dtype != torch.int32 or ctl.numel() < 3 or not ctl.is_contiguous() or ctl.device != avg.device:
        raise ValueError("weight_average_dev: ctl must be 3 contiguous int32 on the device of avg")
    check(_lib.lib().sc_weight_average_dev(avg.data_ptr(), params.data_ptr(), n, ctl.data_ptr(), _stream()),
          "sc_weight_average_dev")


def swap_f32(a, b, n):
    """Exchange ``a[:n]`` and ``b[:n]`` in place (``sc_swap_f32``); overlapping buffers are refused.  Host tensors: with torch."""
    n = int(n)
    _wavg_pair("swap_f32", a, b, n, ("a", "b"))
    if not a.is_cuda:
        x, y = a.view(-1)[:n], b.view(-1)[:n]
        if n and x.data_ptr() < y.data_ptr() + 4 * n and y.data_ptr() < x.data_ptr() + 4 * n:
            raise ValueError("swap_f32: a and b must not overlap")
        t = x.clone()
        x.copy_(y)
        y.copy_(t)
        return
    check(_lib.lib().sc_swap_f32(a.data_ptr(), b.data_ptr(), n, _stream()), "sc_swap_f32")


def weight_average_pass_floats() -> int:
    """Floats that one trip of the full grid of the weight-averaging kernels covers (their launch constants)."""
    return int(_lib.lib().sc_weight_average_pass_floats())


def adamw_step(p, g, m, v, n, lr, beta1, beta2, eps, wd, step, grad_scale, norm_clip, p_bf16=None):
    check(_lib.lib().sc_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(lr), float(beta1),
                                   float(beta2), float(eps), float(wd), int(step), float(grad_scale), _ptr(norm_clip),
                                   _ptr(p_bf16), _stream()), "sc_adamw_step")


def adamw_step_dev(p, g, m, v, n, hyper, beta1, beta2, eps, wd, grad_scale, norm_clip, p_bf16=None):
    """AdamW with {lr, 1 - beta1^step, sqrt(1 - beta2^step)} read from the device tensor ``hyper`` (graph-captured steps)."""
    _req(hyper, torch.float32, "hyper")
    check(_lib.lib().sc_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), float(beta1),
                                       float(beta2), float(eps), float(wd), float(grad_scale), _ptr(norm_clip), _ptr(p_bf16),
                                       _stream()), "sc_adamw_step_dev")


def adamw_groups_hyper_host(lr, wd, beta1, beta2, step, out_host):
    """Fill the HOST fp32 tensor ``out_host`` (2 + 2 * len(lr) floats, pinned for an async copy) with
    {1 - beta1^step, sqrt(1 - beta2^step)} and then {lr_g, wd_g} per group: what ``adamw_step_groups`` reads from its device
    copy.  The bias corrections are formed by the library with ``sc_adamw_step``'s expressions."""
    n_groups = len(lr)
    if len(wd) != n_groups:
        raise ValueError(f"adamw_groups_hyper_host: {n_groups} learning rates, {len(wd)} weight decays")
    if out_host.is_cuda or out_host.dtype != torch.float32 or not out_host.is_contiguous() or out_host.numel() < 2 + 2 * n_groups:
        raise ValueError(f"adamw_groups_hyper_host: out_host must be {2 + 2 * n_groups} contiguous float32 in host memory")
    arr = ctypes.c_float * max(n_groups, 1)
    check(_lib.lib().sc_adamw_groups_hyper_host(arr(*[float(x) for x in lr]), arr(*[float(x) for x in wd]), n_groups,
                                                float(beta1), float(beta2), int(step), out_host.data_ptr()),
          "sc_adamw_groups_hyper_host")
    return out_host


def adamw_step_groups(p, g, m, v, n, chunk_group, group_hyper, n_groups, beta1, beta2, eps, grad_scale, norm_clip, p_bf16=None):
    """AdamW over one range of the flat buffers with per-group lr / weight decay, one launch: ``chunk_group`` (uint8, device)
    names the group of each 64-float slot of the range, ``group_hyper`` (fp32, device) is ``adamw_groups_hyper_host``'s
    layout.  ``None`` for either is passed on as NULL, which the library refuses."""
    n, n_groups = int(n), int(n_groups)
    if chunk_group is not None:
        _req(chunk_group, torch.uint8, "chunk_group")
        if n > 0 and chunk_group.numel() < n // 64:
            raise ValueError(f"adamw_step_groups: chunk_group holds {chunk_group.numel()} slots, the range has {n // 64}")
    if group_hyper is not None:
        _req(group_hyper, torch.float32, "group_hyper")
        if 1 <= n_groups <= 256 and group_hyper.numel() < 2 + 2 * n_groups:
            raise ValueError(f"adamw_step_groups: group_hyper holds {group_hyper.numel()} floats, {n_groups} groups need "
                             f"{2 + 2 * n_groups}")
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"adamw_step_groups: {name} holds {t.numel()} floats, n = {n}")
    if p_bf16 is not None and p_bf16.numel() < n:
        raise ValueError(f"adamw_step_groups: the bf16 mirror holds {p_bf16.numel()} elements, n = {n}")
    check(_lib.lib().sc_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, _ptr(chunk_group),
                                          _ptr(group_hyper), n_groups, float(beta1), float(beta2), float(eps), float(grad_scale),
                                          _ptr(norm_clip), _ptr(p_bf16), _stream()), "sc_adamw_step_groups")


def _lion_buffers(what, p, g, m, n, p_bf16):
    for t, name in ((p, "p"), (g, "g"), (m, "m")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"{what}: {name} holds {t.numel()} floats, n = {n}")
    if p_bf16 is not None and p_bf16.numel() < n:
        raise ValueError(f"{what}: the bf16 mirror holds {p_bf16.numel()} elements, n = {n}")


def lion_step(p, g, m, n, lr, beta1, beta2, wd, grad_scale, norm_clip, p_bf16=None):
    """Lion over flat[:n] (``sc_lion_step``): ``c = b1 m + (1 - b1) ge; p = p (1 - lr wd) - lr sign(c); m = b2 m + (1 - b2) ge``
    with ``ge = g * grad_scale * norm_clip[1]``; one moment, ``sign(0) = 0``; the bf16 mirror is written when given."""
    n = int(n)
    _lion_buffers("lion_step", p, g, m, n, p_bf16)
    check(_lib.lib().sc_lion_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, float(lr), float(beta1), float(beta2), float(wd),
                                  float(grad_scale), _ptr(norm_clip), _ptr(p_bf16), _stream()), "sc_lion_step")


def lion_step_dev(p, g, m, n, lr_dev, beta1, beta2, wd, grad_scale, norm_clip, p_bf16=None):
    """``lion_step`` with the learning rate read from the one-float device tensor ``lr_dev`` (graph-captured steps); ``None``
    is passed on as NULL, which the library refuses."""
    n = int(n)
    if lr_dev is not None:
        _req(lr_dev, torch.float32, "lr_dev")
        if lr_dev.numel() < 1:
            raise ValueError("lion_step_dev: lr_dev holds no float")
    _lion_buffers("lion_step_dev", p, g, m, n, p_bf16)
    check(_lib.lib().sc_lion_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, _ptr(lr_dev), float(beta1), float(beta2),
                                      float(wd), float(grad_scale), _ptr(norm_clip), _ptr(p_bf16), _stream()),
          "sc_lion_step_dev")


def lion_groups_hyper_host(lr, wd, out_host):
    """Fill the HOST fp32 tensor ``out_host`` (2 * len(lr) floats, pinned for an async copy) with {lr_g, wd_g} per group: what
    ``lion_step_groups`` reads from its device copy."""
    n_groups = len(lr)
    if len(wd) != n_groups:
        raise ValueError(f"lion_groups_hyper_host: {n_groups} learning rates, {len(wd)} weight decays")
    if out_host.is_cuda or out_host.dtype != torch.float32 or not out_host.is_contiguous() or out_host.numel() < 2 * n_groups:
        raise ValueError(f"lion_groups_hyper_host: out_host must be {2 * n_groups} contiguous float32 in host memory")
    arr = ctypes.c_float * max(n_groups, 1)
    check(_lib.lib().sc_lion_groups_hyper_host(arr(*[float(x) for x in lr]), arr(*[float(x) for x in wd]), n_groups,
                                               out_host.data_ptr()), "sc_lion_groups_hyper_host")
    return out_host


def lion_step_groups(p, g, m, n, chunk_group, group_hyper, n_groups, beta1, beta2, grad_scale, norm_clip, p_bf16=None):
    """Lion over one range of the flat buffers with per-group lr / weight decay, one launch: ``chunk_group`` (uint8, device)
    names the group of each 64-float slot of the range, ``group_hyper`` (fp32, device) is ``lion_groups_hyper_host``'s layout.
    ``None`` for either is passed on as NULL, which the library refuses."""
    n, n_groups = int(n), int(n_groups)
    if chunk_group is not None:
        _req(chunk_group, torch.uint8, "chunk_group")
        if n > 0 and chunk_group.numel() < n // 64:
            raise ValueError(f"lion_step_groups: chunk_group holds {chunk_group.numel()} slots, the range has {n // 64}")
    if group_hyper is not None:
        _req(group_hyper, torch.float32, "group_hyper")
        if 1 <= n_groups <= 256 and group_hyper.numel() < 2 * n_groups:
            raise ValueError(f"lion_step_groups: group_hyper holds {group_hyper.numel()} floats, {n_groups} groups need "
                             f"{2 * n_groups}")
    _lion_buffers("lion_step_groups", p, g, m, n, p_bf16)
    check(_lib.lib().sc_lion_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, _ptr(chunk_group), _ptr(group_hyper),
                                         n_groups, float(beta1), float(beta2), float(grad_scale), _ptr(norm_clip), _ptr(p_bf16),
                                         _stream()), "sc_lion_step_groups")


def _lamb_tables(what, n_slots, n_tensors, slot_tensor=None, hyper=None, trust=None, slot_sums=None, tensor_slots=None):
    """Dtype, device and size of the LAMB tables that are given (``None`` is passed on as NULL, which the library refuses)."""
    ok = 1 <= n_tensors <= (1 << 20)        # outside: the library refuses before anything is read
    for t, dtype, name, need in ((slot_tensor, torch.int32, "slot_tensor", n_slots), (hyper, torch.float32, "hyper", 2 + 2 * n_tensors),
                                 (trust, torch.float32, "trust", n_tensors), (slot_sums, torch.float32, "slot_sums", 2 * n_slots),
                                 (tensor_slots, torch.int32, "tensor_slots", 2 * n_tensors)):
        if t is None:
            continue
        _req(t, dtype, name)
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if ok and n_slots > 0 and t.numel() < need:
            raise ValueError(f"{what}: {name} holds {t.numel()} elements, {need} are needed")


def lamb_hyper_host(lr, wd, tensor_group, beta1, beta2, step, out_host):
    """Fill the HOST fp32 tensor ``out_host`` (2 + 2 * len(tensor_group) floats, pinned for an async copy) with
    {1 - beta1^step, sqrt(1 - beta2^step)} and then {lr, wd} of every tensor's group: what the ``lamb_*`` launches read from its
    device copy.  ``lr`` / ``wd``: one per group; ``tensor_group``: int32 host tensor, the group of each tensor."""
    n_groups, n_tensors = len(lr), int(tensor_group.numel())
    if len(wd) != n_groups:
        raise ValueError(f"lamb_hyper_host: {n_groups} learning rates, {len(wd)} weight decays")
    if tensor_group.is_cuda or tensor_group.dtype != torch.int32 or not tensor_group.is_contiguous():
        raise ValueError("lamb_hyper_host: tensor_group must be contiguous int32 in host memory")
    if out_host.is_cuda or out_host.dtype != torch.float32 or not out_host.is_contiguous() or out_host.numel() < 2 + 2 * n_tensors:
        raise ValueError(f"lamb_hyper_host: out_host must be {2 + 2 * n_tensors} contiguous float32 in host memory")
    arr = ctypes.c_float * max(n_groups, 1)
    check(_lib.lib().sc_lamb_hyper_host(arr(*[float(x) for x in lr]), arr(*[float(x) for x in wd]), n_groups,
                                        tensor_group.data_ptr(), n_tensors, float(beta1), float(beta2), int(step),
                                        out_host.data_ptr()), "sc_lamb_hyper_host")
    return out_host


def lamb_moments(p, g, m, v, n, slot_tensor, hyper, n_tensors, beta1, beta2, eps, grad_scale, norm_clip, slot_sums):
    """LAMB, first pass over flat[:n] (``sc_lamb_moments``): Adam's moments, and {sum p^2, sum u^2} of every 64-float slot into
    ``slot_sums`` (fp32, 2 per slot).  ``slot_tensor`` (int32, one per slot) names each slot's tensor, ``hyper`` is
    ``lamb_hyper_host``'s layout on the device.  p is not written."""
    n, n_tensors = int(n), int(n_tensors)
    _lamb_tables("lamb_moments", n // 64, n_tensors, slot_tensor=slot_tensor, hyper=hyper, slot_sums=slot_sums)
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"lamb_moments: {name} holds {t.numel()} floats, n = {n}")
    check(_lib.lib().sc_lamb_moments(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, _ptr(slot_tensor), _ptr(hyper),
                                     n_tensors, float(beta1), float(beta2), float(eps), float(grad_scale), _ptr(norm_clip),
                                     _ptr(slot_sums), _stream()), "sc_lamb_moments")


def lamb_trust(slot_sums, n_slots, tensor_slots, hyper, n_tensors, always_adapt, trust_clip, trust):
    """LAMB, between the passes (``sc_lamb_trust``): ``trust[T]`` from the slot sums of the WHOLE buffer (``n_slots`` pairs);
    ``tensor_slots`` (int32, 2 per tensor): first slot and one past the last."""
    n_slots, n_tensors = int(n_slots), int(n_tensors)
    _lamb_tables("lamb_trust", n_slots, n_tensors, hyper=hyper, trust=trust, slot_sums=slot_sums, tensor_slots=tensor_slots)
    check(_lib.lib().sc_lamb_trust(_ptr(slot_sums), n_slots, _ptr(tensor_slots), _ptr(hyper), n_tensors, int(bool(always_adapt)),
                                   int(bool(trust_clip)), _ptr(trust), _stream()), "sc_lamb_trust")


def lamb_apply(p, m, v, n, slot_tensor, hyper, trust, n_tensors, eps, p_bf16=None):
    """LAMB, second pass over flat[:n] (``sc_lamb_apply``): ``p -= lr_T * trust[T] * u`` with u formed again from (p, m, v); the
    bf16 mirror is written when given."""
    n, n_tensors = int(n), int(n_tensors)
    _lamb_tables("lamb_apply", n // 64, n_tensors, slot_tensor=slot_tensor, hyper=hyper, trust=trust)
    for t, name in ((p, "p"), (m, "m"), (v, "v")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"lamb_apply: {name} holds {t.numel()} floats, n = {n}")
    if p_bf16 is not None and p_bf16.numel() < n:
        raise ValueError(f"lamb_apply: the bf16 mirror holds {p_bf16.numel()} elements, n = {n}")
    check(_lib.lib().sc_lamb_apply(p.data_ptr(), m.data_ptr(), v.data_ptr(), n, _ptr(slot_tensor), _ptr(hyper), _ptr(trust),
                                   n_tensors, float(eps), _ptr(p_bf16), _stream()), "sc_lamb_apply")


def _muon_tables(what, n_slots, n_tensors, slot_tensor=None, tensor_info=None, slot_sums=None, ratio=None, norms=None):
    """Dtype, device and size of the Muon tables that are given (``None`` is passed on as NULL, which the library refuses)."""
    ok = 1 <= n_tensors <= (1 << 20)
    for t, dtype, name, need in ((slot_tensor, torch.int32, "slot_tensor", n_slots), (tensor_info, torch.int32, "tensor_info", 4 * n_tensors),
                                 (slot_sums, torch.float32, "slot_sums", n_slots), (ratio, torch.float32, "ratio", n_tensors),
                                 (norms, torch.float32, "norms", n_tensors)):
        if t is None:
            continue
        _req(t, dtype, name)
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if ok and n_slots > 0 and t.numel() < need:
            raise ValueError(f"{what}: {name} holds {t.numel()} elements, {need} are needed")


def _muon_bf16(what, t, name, need):
    if t is None:
        return
    _req(t, torch.bfloat16, name)
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    if t.numel() < need:
        raise ValueError(f"{what}: {name} holds {t.numel()} elements, {need} are needed")


def muon_momentum(g, m, n, slot_tensor, tensor_info, n_tensors, slot0, momentum, nesterov, grad_scale, norm_clip, ubuf, slot_sums,
                  compact_slots):
    """Muon, first pass over flat[:n] (``sc_muon_momentum``): on the slots of a Muon tensor ``m = lerp(m, ge, 1 - momentum)``,
    ``bf16(U)`` into the compact buffer ``ubuf`` and the slot's sum of squares of it into ``slot_sums`` (fp32, one per slot of
    the range); every other slot is neither read nor written.  ``slot_tensor`` (int32, one per slot of the range),
    ``tensor_info`` (int32 [n_tensors, 4]: first slot, one past the last, first compact slot, 0), ``slot0``: the slot at which
    the range starts; ``compact_slots``: what the caller's tables address in ``ubuf`` at the most (host-side size check)."""
    n, n_tensors = int(n), int(n_tensors)
    _muon_tables("muon_momentum", n // 64, n_tensors, slot_tensor=slot_tensor, tensor_info=tensor_info, slot_sums=slot_sums)
    _muon_bf16("muon_momentum", ubuf, "ubuf", 64 * int(compact_slots))
    for t, name in ((g, "g"), (m, "m")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"muon_momentum: {name} holds {t.numel()} floats, n = {n}")
    check(_lib.lib().sc_muon_momentum(g.data_ptr(), m.data_ptr(), n, _ptr(slot_tensor), _ptr(tensor_info), n_tensors, int(slot0),
                                      float(momentum), 1.0 - float(momentum), int(bool(nesterov)), float(grad_scale), _ptr(norm_clip),
                                      _ptr(ubuf),
                                      _ptr(slot_sums), _stream()), "sc_muon_momentum")


def muon_scale(slot_sums, n_slots, tensor_info, n_tensors, eps, ubuf, xbuf, norms, compact_slots):
    """Muon, between the passes (``sc_muon_scale``): each tensor's Frobenius norm from the slot sums of the WHOLE buffer in fp64
    (fixed order) into ``norms`` and ``xbuf = bf16(ubuf / max(norm, eps))`` (compact bf16 buffers)."""
    n_slots, n_tensors = int(n_slots), int(n_tensors)
    _muon_tables("muon_scale", n_slots, n_tensors, tensor_info=tensor_info, slot_sums=slot_sums, norms=norms)
    _muon_bf16("muon_scale", ubuf, "ubuf", 64 * int(compact_slots))
    _muon_bf16("muon_scale", xbuf, "xbuf", 64 * int(compact_slots))
    check(_lib.lib().sc_muon_scale(_ptr(slot_sums), n_slots, _ptr(tensor_info), n_tensors, float(eps), _ptr(ubuf), _ptr(xbuf),
                                   _ptr(norms), _stream()), "sc_muon_scale")


def muon_axpby(acc, cin, out, n, alpha, beta):
    """``out[:n] = bf16(beta * cin[:n] + alpha * acc[:n])`` (``sc_muon_axpby``): the epilogue of a Newton-Schulz product whose fp32
    accumulators ``gemm(..., EPI_F32, ...)`` left in ``acc``; ``cin`` and ``out`` bf16, distinct buffers."""
    n = int(n)
    if acc is not None:
        _req(acc, torch.float32, "acc")
        if acc.numel() < n:
            raise ValueError(f"muon_axpby: acc holds {acc.numel()} floats, n = {n}")
    _muon_bf16("muon_axpby", cin, "cin", n)
    _muon_bf16("muon_axpby", out, "out", n)
    if out is not None and cin is not None and out.data_ptr() == cin.data_ptr():
        raise ValueError("muon_axpby: out must not be cin")
    check(_lib.lib().sc_muon_axpby(_ptr(acc), _ptr(cin), _ptr(out), n, float(alpha), float(beta), _stream()), "sc_muon_axpby")


def muon_apply(p, g, m, v, n, chunk_group, slot_tensor, tensor_info, ratio, n_tensors, slot0, obuf, group_hyper, n_groups, beta1,
               beta2, eps, grad_scale, norm_clip, p_bf16=None, compact_slots=0):
    """Muon, last pass over flat[:n] (``sc_muon_apply``): ``p = p (1 - lr wd) - lr ratio[T] O`` on the slots of Muon tensor T
    (``obuf``: the Newton-Schulz result, compact bf16), the update of ``adamw_step_groups`` on the slots marked -1, nothing
    on a slot marked otherwise.  ``chunk_group`` / ``group_hyper`` as for ``adamw_step_groups``."""
    n, n_tensors, n_groups = int(n), int(n_tensors), int(n_groups)
    _muon_tables("muon_apply", n // 64, max(n_tensors, 1), slot_tensor=slot_tensor,
                 tensor_info=tensor_info if n_tensors else None, ratio=ratio if n_tensors else None)
    if n_tensors:
        _muon_bf16("muon_apply", obuf, "obuf", 64 * int(compact_slots))
    if chunk_group is not None:
        _req(chunk_group, torch.uint8, "chunk_group")
        if n > 0 and chunk_group.numel() < n // 64:
            raise ValueError(f"muon_apply: chunk_group holds {chunk_group.numel()} slots, the range has {n // 64}")
    if group_hyper is not None:
        _req(group_hyper, torch.float32, "group_hyper")
        if 1 <= n_groups <= 256 and group_hyper.numel() < 2 + 2 * n_groups:
            raise ValueError(f"muon_apply: group_hyper holds {group_hyper.numel()} floats, {n_groups} groups need {2 + 2 * n_groups}")
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, name)
        if t.numel() < n:
            raise ValueError(f"muon_apply: {name} holds {t.numel()} floats, n = {n}")
    if p_bf16 is not None and p_bf16.numel() < n:
        raise ValueError(f"muon_apply: the bf16 mirror holds {p_bf16.numel()} elements, n = {n}")
    check(_lib.lib().sc_muon_apply(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, _ptr(chunk_group), _ptr(slot_tensor),
                                   _ptr(tensor_info), _ptr(ratio), n_tensors, int(slot0), _ptr(obuf), _ptr(group_hyper), n_groups,
                                   float(beta1), float(beta2), float(eps), float(grad_scale), _ptr(norm_clip), _ptr(p_bf16),
                                   _stream()), "sc_muon_apply")


def cast_transpose_batched(master, desc, tile_prefix, n, total_tiles, mirror_bf16=None):
    check(_lib.lib().sc_cast_transpose_batched(master.data_ptr(), _ptr(mirror_bf16), desc.data_ptr(),
                                               tile_prefix.data_ptr(), n, total_tiles, _stream()),
          "sc_cast_transpose_batched")


# ------------------------------------------------------------------------------------------ text tower glue
def token_embed_fwd(tokens, table, pos, x, B, L, d, V):
    _req(tokens, torch.int64, "tokens")
    check(_lib.lib().sc_token_embed_fwd(tokens.data_ptr(), table.data_ptr(), pos.data_ptr(), x.data_ptr(), B, L, d, V,
                                        _stream()), "sc_token_embed_fwd")
    return x


def token_embed_bwd(tokens, dres, dtable, dpos, B, L, d, V, eot=None, deterministic=True):
    """Gradient of the embedding gather + positional embedding.  ``deterministic`` (default): every table row summed in
    position order by one wave per column slab (bit-reproducible); ``eot`` int32 [B] = pooled positions (rows behind them are
    skipped: exactly zero in the causal tower).  ``deterministic=False``: float atomics (order-dependent last bit)."""
    if deterministic:
        if eot is not None:
            _req(eot, torch.int32, "eot")
        check(_lib.lib().sc_token_embed_bwd_det(tokens.data_ptr(), _ptr(eot), dres.data_ptr(), dtable.data_ptr(), dpos.data_ptr(),
                                                B, L, d, V, _stream()), "sc_token_embed_bwd_det")
        return
    check(_lib.lib().sc_token_embed_bwd(tokens.data_ptr(), dres.data_ptr(), dtable.data_ptr(), dpos.data_ptr(), B, L, d,
                                        V, _stream()), "sc_token_embed_bwd")


def argmax_rows(tokens, out_idx, B, L):
    _req(tokens, torch.int64, "tokens")
    check(_lib.lib().sc_argmax_rows_i64(tokens.data_ptr(), out_idx.data_ptr(), B, L, _stream()), "sc_argmax_rows_i64")
    return out_idx


def gather_rows(src, idx, L, dst, B, d):
    check(_lib.lib().sc_gather_rows_f32(src.data_ptr(), idx.data_ptr(), L, dst.data_ptr(), B, d, _stream()),
          "sc_gather_rows_f32")
    return dst


def scatter_rows(src, idx, L, dst, dst_bf16, B, d):
    check(_lib.lib().sc_scatter_rows_f32(src.data_ptr(), idx.data_ptr(), L, dst.data_ptr(), _ptr(dst_bf16), B, d,
                                         _stream()), "sc_scatter_rows_f32")


def pcc_rows(pred: torch.Tensor, target: torch.Tensor, pcc: Optional[torch.Tensor] = None,
             sum_count: Optional[torch.Tensor] = None) -> None:
    """Row-wise Pearson correlation with the reference metric's guards (src/metrics/zero_shot.py:72-88)."""
    _req(pred, torch.float32, "pred"); _req(target, torch.float32, "target")
    rows, cols = pred.shape
    if tuple(target.shape) != (rows, cols):
        raise _lib.SpatialClipHipError(f"pcc_rows: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
    check(_lib.lib().sc_pcc_rows(pred.data_ptr(), pred.stride(0), target.data_ptr(), target.stride(0), rows, cols,
                                 _ptr(pcc), _ptr(sum_count), _stream()), "sc_pcc_rows")


# ------------------------------------------------------------------------------------------ input pipeline
def knn_alpha(xy: torch.Tensor, K: int, mode: str = "inverse", sigma: float = 1.0):
    """Spatial neighbours + loss weights of the tiles of one slide: xy fp32 [N,2] -> (nbr_index int32 [N,K], alpha [N,K])."""
    _req(xy, torch.float32, "xy")
    if xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous():
        raise ValueError("knn_alpha: xy must be a contiguous [N, 2] tensor")
    N = xy.shape[0]
    nbr = torch.empty((N, K), dtype=torch.int32, device=xy.device)
    alpha = torch.empty((N, K), dtype=torch.float32, device=xy.device)
    check(_lib.lib().sc_knn_alpha(xy.data_ptr(), N, K, {"inverse": 0, "gaussian": 1}[mode], float(sigma), nbr.data_ptr(),
                                  alpha.data_ptr(), _stream()), "sc_knn_alpha")
    return nbr, alpha


def png_decode(files: torch.Tensor, offsets: torch.Tensor, H: int, W: int):
    """Concatenated PNG files (device uint8 [total]) + int64 offsets [B + 1] -> (uint8 [B, H, W, 3], int32 status [B])."""
    if not files.is_cuda or files.dtype != torch.uint8 or files.dim() != 1 or not files.is_contiguous():
        raise TypeError("png_decode: files must be a contiguous device uint8 vector")
    _req(offsets, torch.int64, "offsets")
    B = offsets.numel() - 1
    if B < 1:
        raise ValueError("png_decode: offsets must hold B + 1 entries")
    l = _lib.lib()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=files.device)
    status = torch.full((B,), -1, dtype=torch.int32, device=files.device)
    scratch = workspace(l.sc_png_decode_scratch_bytes(B, H, W), files.device, "png", torch.uint8)
    check(l.sc_png_decode(files.data_ptr(), offsets.data_ptr(), B, out.data_ptr(), H, W, scratch.data_ptr(),
                          status.data_ptr(), _stream()), "sc_png_decode")
    return out, status


def augment_tiles(src_u8: torch.Tensor, params: torch.Tensor, out_size: int, mean, std) -> torch.Tensor:
    """uint8 [B,H,W,3] + params fp32 [B,12] -> normalised fp32 [B,3,S,S] (crop, resize, colour jitter, normalise)."""
    if not src_u8.is_cuda or src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 \
            or not src_u8.is_contiguous():
        raise TypeError("augment_tiles: src must be a contiguous device uint8 [B,H,W,3] tensor")
    _req(params, torch.float32, "params")
    B, H, W, _ = src_u8.shape
    if tuple(params.shape) != (B, 12) or not params.is_contiguous():
        raise ValueError("augment_tiles: params must be [B, 12]")
    out = torch.empty((B, 3, out_size, out_size), dtype=torch.float32, device=src_u8.device)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().sc_augment_tiles(src_u8.data_ptr(), B, H, W, params.data_ptr(), out.data_ptr(), out_size,
                                      ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), _stream()),
          "sc_augment_tiles")
    return out


AUG_ROW = 36      # SC_AUG_ROW of include/spatial_clip_hip.h


def augment_tiles_ex(src_u8: torch.Tensor, params: torch.Tensor, out_size: int, mean, std,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,H,W,3] + HOST params fp32 [B, stride >= AUG_ROW] -> normalised fp32 [B,3,S,S]: ``augment_tiles`` plus vertical
    flip, hue, the jitter switch, grayscale and erase boxes (row layout: include/spatial_clip_hip.h).  The rows stay on the
    host: the entry checks them and copies them to the device on the current stream itself."""
    if not src_u8.is_cuda or src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 \
            or not src_u8.is_contiguous():
        raise TypeError("augment_tiles_ex: src must be a contiguous device uint8 [B,H,W,3] tensor")
    B, H, W, _ = src_u8.shape
    if params.is_cuda or params.dtype != torch.float32 or params.dim() != 2 or params.shape[0] != B \
            or params.shape[1] < AUG_ROW or not params.is_contiguous():
        raise ValueError(f"augment_tiles_ex: params must be a contiguous host fp32 [B, >= {AUG_ROW}] tensor")
    if out is None:
        out = torch.empty((B, 3, out_size, out_size), dtype=torch.float32, device=src_u8.device)
    elif tuple(out.shape) != (B, 3, out_size, out_size) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != src_u8.device:
        raise ValueError("augment_tiles_ex: out must be a contiguous fp32 [B,3,S,S] tensor on the source's device")
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().sc_augment_tiles_ex(src_u8.data_ptr(), B, H, W, params.data_ptr(), int(params.shape[1]), out.data_ptr(),
                                         out_size, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p),
                                         _stream()), "sc_augment_tiles_ex")
    return out


# ------------------------------------------------------------------------------------------ fp8 forward path
def quantize_rows_fp8_batched(desc: torch.Tensor, block_prefix: torch.Tensor, n: int, total_blocks: int) -> None:
    """Row-wise e4m3 copies of ``n`` matrices in one launch (params.ParamStore._q8_plan builds the device tables)."""
    check(_lib.lib().sc_quantize_rows_fp8_batched(desc.data_ptr(), block_prefix.data_ptr(), n, total_blocks, _stream()),
          "sc_quantize_rows_fp8_batched")


def quantize_rows_fp8(src: torch.Tensor, dst: Optional[torch.Tensor] = None, scale_inv: Optional[torch.Tensor] = None,
                      fixed_scale: float = 0.0):
    """Row-wise e4m3 quantisation with a power-of-two scale per row: -> (fp8 bytes as uint8 [rows, cols], 1/scale [rows])."""
    if not src.is_cuda or src.dtype not in (torch.float32, torch.bfloat16) or src.dim() != 2 or src.stride(1) != 1:
        raise TypeError("quantize_rows_fp8: src must be a device fp32 / bf16 matrix with unit inner stride")
    rows, cols = src.shape
    if dst is None:
        dst = torch.empty((rows, cols), dtype=torch.uint8, device=src.device)
    if scale_inv is None:
        scale_inv = torch.empty(rows, dtype=torch.float32, device=src.device)
    check(_lib.lib().sc_quantize_rows_fp8(src.data_ptr(), int(src.dtype == torch.float32), src.stride(0), rows, cols,
                                          dst.data_ptr(), dst.stride(0), scale_inv.data_ptr(), float(fixed_scale),
                                          _stream()), "sc_quantize_rows_fp8")
    return dst, scale_inv


def fp8_scale_update(amax_slots: torch.Tensor, scale: torch.Tensor, scale_inv: torch.Tensor, margin_bits: int = 1,
                     hist: Optional[torch.Tensor] = None, slot: int = 0) -> None:
    """Delayed scaling: next step's per-tensor e4m3 scales from the maxima the epilogues recorded ([n, 64] slots, cleared).
    ``hist`` (fp32 [H, n]) + ``slot``: keep the maxima of the last H steps and scale for their maximum."""
    _req(amax_slots, torch.float32, "amax_slots"); _req(scale, torch.float32, "scale"); _req(scale_inv, torch.float32, "scale_inv")
    n = scale.numel()
    if amax_slots.numel() != n * 64 or scale_inv.numel() != n:
        raise ValueError("fp8_scale_update: amax_slots must be [n, 64] for n scales")
    if hist is not None:
        _req(hist, torch.float32, "hist")
        if hist.dim() != 2 or hist.shape[1] != n or not hist.is_contiguous():
            raise ValueError("fp8_scale_update: hist must be a contiguous [H, n] tensor")
        check(_lib.lib().sc_fp8_scale_update_hist(amax_slots.data_ptr(), hist.data_ptr(), hist.shape[0], int(slot) % hist.shape[0],
                                                  scale.data_ptr(), scale_inv.data_ptr(), n, int(margin_bits), _stream()),
              "sc_fp8_scale_update_hist")
        return
    check(_lib.lib().sc_fp8_scale_update(amax_slots.data_ptr(), scale.data_ptr(), scale_inv.data_ptr(), n, int(margin_bits),
                                         _stream()), "sc_fp8_scale_update")


def gemm_wgrad_fp8(dy8: torch.Tensor, dy_scale_inv: torch.Tensor, x8: torch.Tensor, x_scale_inv: torch.Tensor, dw: torch.Tensor,
                   dbias: Optional[torch.Tensor], *, M: int, N: int, K: int, splitk: int = 1) -> None:
    """dW[M,N] = s_dy s_x dY8[K,M]^T . X8[K,N] (fp32) and dbias[M] = s_dy column sums of dY8: e4m3 operands with ONE scale per
    tensor (``*_scale_inv``: one-element device tensors)."""
    for t_, n in ((dy8, "dy8"), (x8, "x8")):
        if not t_.is_cuda or t_.dtype != torch.uint8 or t_.stride(-1) != 1:
            raise TypeError(f"gemm_wgrad_fp8: {n} must be a device uint8 (e4m3 bytes) matrix")
    _req(dy_scale_inv, torch.float32, "dy_scale_inv"); _req(x_scale_inv, torch.float32, "x_scale_inv"); _req(dw, torch.float32, "dw")
    if dbias is not None: _req(dbias, torch.float32, "dbias")
    if not dw.is_contiguous() or dw.numel() != M * N:
        raise ValueError("gemm_wgrad_fp8: dw must be a dense [M, N] tensor")
    l = _lib.lib()
    ws = workspace(l.sc_gemm_wgrad_ws_floats(M, N, K, splitk), dw.device, "wgrad")
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    rc = l.sc_gemm_wgrad_fp8(dy8.data_ptr(), dy8.stride(0), dy_scale_inv.data_ptr(), x8.data_ptr(), x8.stride(0),
                             x_scale_inv.data_ptr(), M, N, K, dw.data_ptr(), N, _ptr(dbias), splitk, ws.data_ptr(), _stream())
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append(("gemm_tn_fp8", 2.0 * M * N * K, ev))
    check(rc, "sc_gemm_wgrad_fp8")


def gemm_fp8(epi: int, a8: torch.Tensor, a_scale_inv: torch.Tensor, b8: torch.Tensor, b_scale_inv: torch.Tensor,
             out: torch.Tensor, *, M: int, N: int, K: int, out2: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
             aux: Optional[torch.Tensor] = None, a_scale_scalar: bool = False, q8_out: Optional[torch.Tensor] = None,
             q8_scale: Optional[torch.Tensor] = None, q8_amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[M,N] = dequant(A8[M,K] . B8[N,K]^T) with the bf16 GEMM's epilogues (see sc_gemm_fp8); ``aux`` = the pre-GELU
    tensor of EPI_BF16_DGELU (the c_proj data-gradient GEMM)."""
    for t_, n in ((a8, "a8"), (b8, "b8")):
        if not t_.is_cuda or t_.dtype != torch.uint8 or t_.stride(-1) != 1:
            raise TypeError(f"gemm_fp8: {n} must be a device uint8 (e4m3 bytes) matrix")
    _req(a_scale_inv, torch.float32, "a_scale_inv"); _req(b_scale_inv, torch.float32, "b_scale_inv")
    want = torch.float32 if epi in (EPI_F32, EPI_F32_BIAS_RES) else torch.bfloat16
    _req(out, want, "out")
    if res is not None: _req(res, torch.bfloat16 if epi == EPI_BF16_BIAS_RES else torch.float32, "res")
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    if q8_out is not None and (q8_out.dtype != torch.uint8 or not q8_out.is_cuda or q8_out.stride(-1) != 1):
        raise TypeError("gemm_fp8: q8_out must be a device uint8 matrix")
    rc = _lib.lib().sc_gemm_fp8_q(epi, a8.data_ptr(), a8.stride(0), a_scale_inv.data_ptr(), int(a_scale_scalar),
                                  b8.data_ptr(), b8.stride(0), b_scale_inv.data_ptr(), M, N, K, out.data_ptr(),
                                  out.stride(0), _ptr(out2), out2.stride(0) if out2 is not None else 0, _ptr(bias),
                                  _ptr(res), res.stride(0) if res is not None else 0, _ptr(aux),
                                  aux.stride(0) if aux is not None else 0, _ptr(q8_out),
                                  q8_out.stride(0) if q8_out is not None else 0, _ptr(q8_scale), _ptr(q8_amax), _stream())
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append(("gemm_nt_fp8", 2.0 * M * N * K, ev))
    check(rc, "sc_gemm_fp8")
    return out
