"""Which kernel sc_attn_fwd / sc_attn_bwd dispatch a shape to, restated by hand from each path's acceptance predicate
(file:line beside each) and the order of the two path tables (attn_fwd_paths / attn_bwd_paths, sc_attention.hip).  Nothing
here asks the library: tests/test_gpu_attention_sweep.py asserts these names against the kernel that ran, and
tests/test_cpu_attention_dispatch.py against ``ops.attn_plan``.  No GPU.

Left out: the LDS limits of the persistent kernels (never the binding limit inside their token ranges) and the 2^31-workgroup
limit of the streamed kernels."""

from tests._attnbounds import MAXL                     # sc_attn_common.h:10

BUFFER_LIMIT = 0xFFFFFFF0                              # attn_fits_buffer, sc_attn_host.h:51

SWITCHES = ("SC_ATTN_PERSIST", "SC_ATTN_PERSIST2", "SC_ATTN_LONG", "SC_ATTN_BWD3", "SC_ATTN_BWD4", "SC_ATTN_BWD1",
            "SC_ATTN_BWD2", "SC_ATTN_FUSED")
DEFAULT = {"SC_ATTN_PERSIST": "1", "SC_ATTN_PERSIST2": "1", "SC_ATTN_LONG": "0", "SC_ATTN_BWD3": "1", "SC_ATTN_BWD4": "1",
           "SC_ATTN_BWD1": "1", "SC_ATTN_BWD2": "1", "SC_ATTN_FUSED": "1"}
_NO_BWD = {"SC_ATTN_BWD3": "0", "SC_ATTN_BWD4": "0", "SC_ATTN_BWD1": "0", "SC_ATTN_BWD2": "0"}
FWD_ENV = {"persistent": {"SC_ATTN_PERSIST2": "0"}, "persistent2": {}, "per_head": {"SC_ATTN_PERSIST": "0"},
           "stream": {"SC_ATTN_LONG": "1"}}
BWD_ENV = {"ring": {**_NO_BWD, "SC_ATTN_BWD3": "1"}, "ring8": {**_NO_BWD, "SC_ATTN_BWD4": "1"},
           "single_pass": {**_NO_BWD, "SC_ATTN_BWD1": "1"}, "persistent": {**_NO_BWD, "SC_ATTN_BWD2": "1"},
           "fused": dict(_NO_BWD), "dq_dkv": {**_NO_BWD, "SC_ATTN_FUSED": "0"}, "stream": {"SC_ATTN_LONG": "1"}, "cls": {}}


def out_bytes(B, L, H, dh):
    """out [B*L, H*dh] bf16 (AttnShape::out_bytes, sc_attn_host.h:15); dqkv is three times that (:17)."""
    return B * L * H * dh * 2


def _streams(env, dh, L, causal):
    """stream_only (sc_attention.hip:525) and stream_shape (sc_attention_stream.hip:569): head dim 80 up to MAXL; head dim
    64 non-causal above MAXL or with SC_ATTN_LONG=1."""
    if dh == 80:
        return L <= MAXL
    return dh == 64 and not causal and (L > MAXL or env["SC_ATTN_LONG"] == "1")


def expected_fwd(env, dh, L, causal, nq, B=2, H=3):
    if _streams(env, dh, L, causal):
        return "stream"
    on = env["SC_ATTN_PERSIST"] != "0"
    fits = out_bytes(B, L, H, dh) < BUFFER_LIMIT
    # sc_attention_p.hip:259-260: dh 64, L <= 224, one compute wave per 16-query tile beside 3 loader waves, 16 waves at most
    if on and dh == 64 and L <= 224 and (nq + 15) // 16 + 3 <= 16 and fits:
        return "persistent"
    # sc_attention_p2.hip:231-233: 224 < L <= 288 (one compute wave per two query tiles: always within its 12 waves)
    if on and env["SC_ATTN_PERSIST2"] != "0" and dh == 64 and 224 < L <= 288 and fits:
        return "persistent2"
    return "per_head"


def fused_fits(dh, L):
    """bwd_fused_accepts (sc_attention.hip:486): Q, K, V, dO images of Lp = L rounded up to 32 rows plus two fp32 row vectors
    in 160 KiB."""
    Lp = (L + 31) & ~31
    return 4 * Lp * dh * 2 + 2 * Lp * 4 <= 160 * 1024


def expected_bwd(env, dh, L, causal, nq, B=2, H=3):
    cls = nq == 1 and L >= 2                                             # sc_attention_cls.hip:109
    if _streams(env, dh, L, causal):
        return "cls" if cls else "stream"
    if cls:
        return "cls"
    full64 = dh == 64 and nq == L and 3 * out_bytes(B, L, H, dh) < BUFFER_LIMIT
    if env["SC_ATTN_BWD3"] != "0" and full64 and L <= 224 and not causal:            # sc_attention_bwd3.hip:391
        return "ring"
    if env["SC_ATTN_BWD4"] != "0" and full64 and 224 < L <= 257 and not causal:      # sc_attention_bwd4.hip:725-726
        return "ring8"
    if env["SC_ATTN_BWD1"] != "0" and full64 and L <= 224 and not causal:            # sc_attention_bwd1.hip:362
        return "single_pass"
    if env["SC_ATTN_BWD2"] != "0" and full64 and L <= 224:                           # sc_attention_bwd2.hip:336-337
        return "persistent"
    if env["SC_ATTN_FUSED"] != "0" and fused_fits(dh, L):
        return "fused"
    return "dq_dkv"
