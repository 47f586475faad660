"""The attention dispatcher without a GPU: ``ops.attn_plan`` (sc_debug_attn_plan: the planner sc_attn_fwd / sc_attn_bwd use,
host arithmetic only) against the hand restatement of tests/_attnpaths.py at every length, head dim, causal flag, q_rows
and switch setting of the GPU sweep; the byte limits of the persistent kernels; the shapes the library refuses; null operands."""
import pytest

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import _lib, ops
from tests import _attnpaths as P
from tests._attnbounds import STREAM_LONG_LENGTHS, q_rows_at


def _envs():
    """Every environment of the sweep, and every single switch flipped alone from DEFAULT."""
    envs = [dict(P.DEFAULT)]
    envs += [{**P.DEFAULT, **e} for e in list(P.FWD_ENV.values()) + list(P.BWD_ENV.values())]
    envs += [{**P.DEFAULT, k: "0" if P.DEFAULT[k] == "1" else "1"} for k in P.SWITCHES]
    seen, out = set(), []
    for e in envs:
        key = tuple(e[k] for k in P.SWITCHES)
        if key not in seen:
            seen.add(key)
            out.append(e)
    return out


def _set(monkeypatch, env):
    for k in P.SWITCHES:
        monkeypatch.setenv(k, env[k])


@pytest.mark.parametrize("dh", [32, 64, 80])
def test_plan_matches_the_restatement(dh, monkeypatch):
    B, H = 2, 3
    bad, n = [], 0
    for env in _envs():
        _set(monkeypatch, env)
        for L in list(range(1, P.MAXL + 1)) + STREAM_LONG_LENGTHS:
            for causal in (False, True):
                for r in [0] + q_rows_at(L):
                    if L > P.MAXL and (dh != 64 or causal):
                        with pytest.raises(RuntimeError, match="above 320 tokens"):
                            ops.attn_plan(B, L, H, dh, causal, r)
                        continue
                    nq = r if r else L
                    want = (P.expected_fwd(env, dh, L, causal, nq, B, H), P.expected_bwd(env, dh, L, causal, nq, B, H))
                    got = ops.attn_plan(B, L, H, dh, causal, r)
                    n += 1
                    if got != want:
                        bad.append((env, L, causal, r, got, want))
    assert n > 10000 and not bad, (len(bad), bad[:10])


def test_unset_switches_are_the_default(monkeypatch):
    for k in P.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for dh, L, causal, r in [(64, 197, False, 0), (64, 77, True, 0), (64, 257, False, 0), (64, 300, False, 0), (32, 50, False, 0),
                             (80, 257, True, 0), (64, 577, False, 0), (64, 197, False, 1), (64, 197, False, 16)]:
        nq = r if r else L
        assert ops.attn_plan(2, L, 3, dh, causal, r) == (P.expected_fwd(P.DEFAULT, dh, L, causal, nq),
                                                         P.expected_bwd(P.DEFAULT, dh, L, causal, nq))


def test_byte_limits_of_the_persistent_kernels(monkeypatch):
    """out (forward) and dqkv (backward) are addressed with 32-bit byte offsets by the persistent kernels: the largest batch
    that stays under the limit takes them, one more falls to the per-head kernels.  Nothing is allocated."""
    _set(monkeypatch, P.DEFAULT)
    dh, L, H = 64, 197, 12
    B = (P.BUFFER_LIMIT - 1) // P.out_bytes(1, L, H, dh)
    assert P.out_bytes(B, L, H, dh) < P.BUFFER_LIMIT <= P.out_bytes(B + 1, L, H, dh)
    assert ops.attn_plan(B, L, H, dh)[0] == "persistent" and ops.attn_plan(B + 1, L, H, dh)[0] == "per_head"
    assert (P.expected_fwd(P.DEFAULT, dh, L, False, L, B, H), P.expected_fwd(P.DEFAULT, dh, L, False, L, B + 1, H)) == \
        ("persistent", "per_head")
    B = (P.BUFFER_LIMIT - 1) // (3 * P.out_bytes(1, L, H, dh))
    assert 3 * P.out_bytes(B, L, H, dh) < P.BUFFER_LIMIT <= 3 * P.out_bytes(B + 1, L, H, dh)
    assert ops.attn_plan(B, L, H, dh)[1] == "ring" and ops.attn_plan(B + 1, L, H, dh)[1] == "fused"
    assert (P.expected_bwd(P.DEFAULT, dh, L, False, L, B, H), P.expected_bwd(P.DEFAULT, dh, L, False, L, B + 1, H)) == \
        ("ring", "fused")
    for env, path in ((P.BWD_ENV["single_pass"], "single_pass"), (P.BWD_ENV["persistent"], "persistent")):
        _set(monkeypatch, {**P.DEFAULT, **env})
        assert ops.attn_plan(B, L, H, dh)[1] == path and ops.attn_plan(B + 1, L, H, dh)[1] == "fused"
    _set(monkeypatch, P.DEFAULT)
    L = 257
    B = (P.BUFFER_LIMIT - 1) // P.out_bytes(1, L, H, dh)
    assert ops.attn_plan(B, L, H, dh)[0] == "persistent2" and ops.attn_plan(B + 1, L, H, dh)[0] == "per_head"
    B = (P.BUFFER_LIMIT - 1) // (3 * P.out_bytes(1, L, H, dh))
    assert ops.attn_plan(B, L, H, dh)[1] == "ring8" and ops.attn_plan(B + 1, L, H, dh)[1] == "fused"


@pytest.mark.parametrize("args,msg", [((1, 400, 2, 64, True), "above 320 tokens"), ((1, 400, 2, 32, False), "above 320 tokens"),
                                      ((1, 321, 2, 80, False), "above 320 tokens"), ((1, 0, 2, 64, False), "need 0 < L <= 320"),
                                      ((0, 100, 2, 64, False), "need 0 < L <= 320"), ((1, 100, 0, 64, False), "need 0 < L <= 320"),
                                      ((0, 1000, 2, 64, False), "need 0 < L <= 320"),
                                      ((1, 100, 2, 48, False), "head dim must be 32, 64 or 80"),
                                      ((1 << 20, 1 << 20, 1 << 10, 64, False), "grid too large")])
def test_refused_shapes_return_the_library_message(args, msg):
    l = _lib.lib()
    fn = l.sc_debug_attn_plan
    rc = fn(*[int(a) for a in args], 0, None, None)
    assert rc == -1 and msg.encode() in l.sc_last_error() and b"sc_attn_fwd" in l.sc_last_error()
    with pytest.raises(RuntimeError, match=msg):
        ops.attn_plan(*args)
    B, L, H, dh, causal = args
    if msg != "grid too large":           # sc_attn_fwd / sc_attn_bwd say the same, before they look at the operands
        assert l.sc_attn_fwd(None, None, None, B, L, H, dh, int(causal), 0, None) < 0 and msg.encode() in l.sc_last_error()
        assert l.sc_attn_bwd(None, None, None, None, None, None, B, L, H, dh, int(causal), 0, None) < 0
        assert msg.encode() in l.sc_last_error() and b"sc_attn_bwd" in l.sc_last_error()


def test_null_operands_are_refused_on_every_path():
    """A launch on a null pointer would fault the device: every path refuses it, not only the streamed one."""
    l = _lib.lib()
    for L, dh, causal in [(100, 64, 0), (257, 64, 0), (300, 64, 1), (50, 32, 0), (100, 80, 0), (1000, 64, 0)]:
        assert l.sc_attn_fwd(None, None, None, 1, L, 1, dh, causal, 0, None) < 0 and b"null operand" in l.sc_last_error()
        for q_rows in (0, 1):
            assert l.sc_attn_bwd(None, None, None, None, None, None, 1, L, 1, dh, causal, q_rows, None) < 0
            assert b"null operand" in l.sc_last_error() and b"sc_attn_bwd" in l.sc_last_error()
