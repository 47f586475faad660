"""Attention above 320 tokens (sc_attention_stream.hip at head dim 64): parity with the fp32 formula, q_rows, many heads,
determinism, the SC_ATTN_LONG=1 switch at short lengths and the shapes the build rejects above 320 tokens."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DH = 64


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def ref_attn(qkv, B, L, H, dh):
    """The fp32 formula of tests/test_gpu_ops.py's ref_attn (non-causal): out [B*L, H*dh] and lse [B, H, L]."""
    d = H * dh
    q, k, v = qkv.float().view(B, L, 3 * d).split(d, dim=-1)
    q = q.view(B, L, H, dh).transpose(1, 2)
    k = k.view(B, L, H, dh).transpose(1, 2)
    v = v.view(B, L, H, dh).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    a = torch.softmax(s, -1)
    return (a @ v).transpose(1, 2).reshape(B * L, d), torch.logsumexp(s, -1)


def _inputs(B, L, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = H * DH
    qkv = torch.randn(B * L, 3 * d, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B * L, d, device="cuda", generator=g).bfloat16()
    return qkv, dout


def _reference(qkv, dout, B, L, H, rows=None):
    """fp32 out, lse and d(loss)/d(qkv) of loss = sum(out * dout) over the first `rows` query rows (all when None)."""
    x = qkv.float().requires_grad_(True)
    o, lse = ref_attn(x, B, L, H, DH)
    w = dout.float()
    if rows is not None:
        keep = (torch.arange(L, device=qkv.device) < rows).float().repeat(B)[:, None]
        w = w * keep
    (o * w).sum().backward()
    return o.detach(), lse.detach(), x.grad


def _check(out, lse, dqkv, o_ref, lse_ref, g_ref):
    torch.testing.assert_close(out.float(), o_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(lse, lse_ref, atol=2e-3, rtol=1e-3)
    if dqkv is not None:
        torch.testing.assert_close(dqkv.float(), g_ref, atol=4e-2, rtol=4e-2)


@pytest.mark.parametrize("B,L,H", [(2, 321, 2), (1, 401, 4), (2, 577, 3), (3, 600, 2), (1, 785, 2), (1, 1025, 1)])
def test_long_attention_matches_fp32_formula(B, L, H):
    ops = _ops()
    qkv, dout = _inputs(B, L, H, seed=L + H)
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H)
    out, lse = ops.attn_fwd(qkv, B, L, H, DH)
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH)
    torch.cuda.synchronize()
    _check(out, lse, dqkv, o_ref, lse_ref, g_ref)


def test_long_attention_large_scores_peak_in_last_tile():
    """Scaled scores span about -45..+72, every row's maximum at the last key (577 = 9 * 64 + 1: alone in its tile), so
    the running max moves in the last step of the online softmax and the rescale must be exact."""
    ops = _ops()
    B, L, H = 2, 577, 2
    d = H * DH
    g = torch.Generator(device="cuda").manual_seed(5)
    u = torch.full((DH,), 1.0 / 8.0, device="cuda")                            # unit vector
    q = 24.0 * u + torch.randn(B * L, H, DH, device="cuda", generator=g)
    k = 4.0 * torch.randn(B * L, H, DH, device="cuda", generator=g)
    k.view(B, L, H, DH)[:, L - 1] = 24.0 * u
    v = torch.randn(B * L, H, DH, device="cuda", generator=g)
    qkv = torch.cat([q.reshape(B * L, d), k.reshape(B * L, d), v.reshape(B * L, d)], 1).bfloat16()
    dout = torch.randn(B * L, d, device="cuda", generator=g).bfloat16()
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H)
    s = (qkv.float().view(B, L, 3, H, DH)[:, :, 0].transpose(1, 2) @
         qkv.float().view(B, L, 3, H, DH)[:, :, 1].permute(0, 2, 3, 1)) / 8.0
    assert s.max() > 55 and s.min() < -35 and bool((s.argmax(-1) == L - 1).all())
    out, lse = ops.attn_fwd(qkv, B, L, H, DH)
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    _check(out, lse, dqkv, o_ref, lse_ref, g_ref)


@pytest.mark.parametrize("q_rows", [1, 30])
def test_long_attention_q_rows(q_rows):
    ops = _ops()
    B, L, H = 2, 577, 2
    d = H * DH
    qkv, dout = _inputs(B, L, H, seed=q_rows)
    out_all, lse_all = ops.attn_fwd(qkv, B, L, H, DH)
    out, lse = ops.attn_fwd(qkv, B, L, H, DH, q_rows=q_rows)
    torch.cuda.synchronize()
    rows = (torch.arange(L, device="cuda") < q_rows).repeat(B)
    assert torch.equal(out[rows], out_all[rows])
    assert torch.equal(lse[:, :, :q_rows], lse_all[:, :, :q_rows])
    # the backward writes every element of dqkv (no memset by the caller): start from NaNs
    dqkv = torch.full_like(qkv, float("nan"))
    ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH, dqkv=dqkv, q_rows=q_rows)
    torch.cuda.synchronize()
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H, rows=q_rows)
    assert torch.isfinite(dqkv.float()).all()
    g = dqkv.float().view(B, L, 3 * d)
    gr = g_ref.view(B, L, 3 * d)
    torch.testing.assert_close(g[:, :, d:], gr[:, :, d:], atol=4e-2, rtol=4e-2)             # dK, dV
    torch.testing.assert_close(g[:, :q_rows, :d], gr[:, :q_rows, :d], atol=4e-2, rtol=4e-2)
    assert bool((g[:, q_rows:, :d] == 0).all())                                            # dQ of unconsumed rows


def test_long_attention_many_heads_and_determinism():
    """B * H = 640 heads (far more than the 256 CUs); two launches give bit-identical out, lse and dqkv."""
    ops = _ops()
    B, L, H = 40, 577, 16
    qkv, dout = _inputs(B, L, H, seed=40)
    out, lse = ops.attn_fwd(qkv, B, L, H, DH)
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH)
    out2, lse2 = ops.attn_fwd(qkv, B, L, H, DH)
    dqkv2 = ops.attn_bwd(qkv, out2, dout, lse2, B, L, H, DH)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H)
    _check(out, lse, dqkv, o_ref, lse_ref, g_ref)


@pytest.mark.parametrize("L", [197, 257, 300])
def test_forced_long_kernels_at_short_lengths(L, monkeypatch):
    ops = _ops()
    B, H = 3, 4
    qkv, dout = _inputs(B, L, H, seed=L)
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H)
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("SC_ATTN_LONG", sw)
        # what runs at these lengths without the switch: the persistent kernels up to 224 / 288 tokens forward, the ring
        # kernels up to 224 / 257 backward, then the per-head kernels (300 tokens are past the fused backward's 288)
        fwd, bwd = ("stream", "stream") if sw == "1" else {197: ("persistent", "ring"), 257: ("persistent2", "ring8"),
                                                           300: ("per_head", "dq_dkv")}[L]
        out, lse = ops.attn_fwd(qkv, B, L, H, DH)
        assert ops.attn_last_path()[0] == fwd
        out30, lse30 = ops.attn_fwd(qkv, B, L, H, DH, q_rows=30)
        assert ops.attn_last_path()[0] == fwd
        dqkv = ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH)
        assert ops.attn_last_path()[1] == bwd
        torch.cuda.synchronize()
        _check(out, lse, dqkv, o_ref, lse_ref, g_ref)
        rows = (torch.arange(L, device="cuda") < 30).repeat(B)
        torch.testing.assert_close(out30[rows].float(), o_ref[rows], atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(lse30[:, :, :30], lse_ref[:, :, :30], atol=2e-3, rtol=1e-3)
        res[sw] = (out, lse, dqkv, out30[rows], lse30[:, :, :30])
    for a, b in zip(res["0"], res["1"]):
        torch.testing.assert_close(a.float(), b.float(), atol=2e-2, rtol=2e-2)


def test_long_attention_rejects_unsupported_shapes():
    """Above 320 tokens only dh = 64, non-causal has a kernel: other shapes raise (naming the limit) and launch nothing;
    the next valid call works."""
    ops = _ops()
    B, L, H = 1, 400, 2
    qkv, dout = _inputs(B, L, H, seed=1)
    with pytest.raises(RuntimeError, match="320"):
        ops.attn_fwd(qkv, B, L, H, DH, causal=True)
    out0 = torch.zeros(B * L, H * DH, device="cuda", dtype=torch.bfloat16)
    lse0 = torch.zeros(B, H, L, device="cuda")
    with pytest.raises(RuntimeError, match="320"):
        ops.attn_bwd(qkv, out0, dout, lse0, B, L, H, DH, causal=True, dqkv=torch.zeros_like(qkv))
    qkv32 = qkv[:, : 3 * H * 32].contiguous()
    with pytest.raises(RuntimeError, match="320"):
        ops.attn_fwd(qkv32, B, L, H, 32, out=out0[:, : H * 32].contiguous())
    with pytest.raises(RuntimeError, match="320"):
        ops.attn_bwd(qkv32, out0[:, : H * 32].contiguous(), dout[:, : H * 32].contiguous(), lse0, B, L, H, 32)
    torch.cuda.synchronize()
    o_ref, lse_ref, g_ref = _reference(qkv, dout, B, L, H)
    out, lse = ops.attn_fwd(qkv, B, L, H, DH)
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH)
    torch.cuda.synchronize()
    _check(out, lse, dqkv, o_ref, lse_ref, g_ref)
