"""The GEMM dispatcher without a GPU: ``ops.gemm_plan`` (sc_debug_gemm_plan: the planner sc_gemm_bf16 / sc_gemm_wgrad_bias
call, host arithmetic only) against the hand restatement of tests/_gemmpaths.py over both modes, every epilogue, split-K
requests, slabs or none, dense and strided C, CU counts, every switch flipped alone, and shapes on both sides of every
boundary of the rule; the shapes the library refuses."""
import re

import pytest

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import _lib, ops
from tests import _gemmpaths as P


def _set(monkeypatch, env):
    for k in P.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _plan(mode, epi, M, N, K, ldc, splitk, has_slabs, colsum, slots):
    """The library's answer in the restatement's form: the record, or the refusal's message."""
    try:
        path, tail = ops.gemm_plan(mode, epi, M, N, K, ldc=ldc, splitk=splitk, has_slabs=has_slabs, colsum=colsum, slots=slots)
    except RuntimeError as e:
        return str(e)
    return tuple(path), tail


def _same(got, want):
    return (want in got) if isinstance(want, str) else (not isinstance(got, str) and got == want)


@pytest.mark.parametrize("env", P.ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_plan_matches_the_restatement(env, monkeypatch):
    _set(monkeypatch, env)
    bad, n, paths = [], 0, set()
    for M, N, K in P.SHAPES:
        for mode in (P.NT, P.TN):
            for epi in P.EPIS:
                for splitk in P.SPLITKS:
                    for has_slabs in (False, True):
                        for ldc in P.ldcs(N):
                            # the CU count matters to the tail rule alone: every count where it can, two elsewhere
                            tailed = mode == P.NT and splitk == 1
                            for slots in (P.SLOTS if tailed else (0, 256)):
                                want = P.expected(env, slots, mode, epi, M, N, K, ldc, splitk, has_slabs)
                                got = _plan(mode, epi, M, N, K, ldc, splitk, has_slabs, False, slots)
                                n += 1
                                if not isinstance(want, str):
                                    paths.add(want[0][0])
                                if not _same(got, want):
                                    bad.append((mode, epi, M, N, K, ldc, splitk, has_slabs, slots, got, want))
        for splitk in P.SPLITKS:                               # sc_gemm_wgrad_bias
            for ldc in P.ldcs(N):
                want = P.expected(env, 256, P.TN, P.F32, M, N, K, ldc, splitk, True, colsum=True)
                got = _plan(P.TN, P.F32, M, N, K, ldc, splitk, True, True, 256)
                n += 1
                if not _same(got, want):
                    bad.append(("wgrad_bias", M, N, K, ldc, splitk, got, want))
    assert n > 8000 and not bad, (n, len(bad), bad[:10])
    force = env.get("SC_GEMM_FORCE")
    want_paths = {"nt128", "nt128_ktail", "tn128"} | ({"nt256", "tn256"} if force == "256" else set()) | \
        ({"nt8p", "tn8p"} if force is None else set()) | \
        ({"nt8p_persistent"} if force is None and env.get("SC_GEMM_PERSIST") != "0" else set())
    assert paths == want_paths, paths


def test_boundaries_one_by_one(monkeypatch):
    """The boundary shapes the sweep exists for, spelled out (default switches, 256 CUs)."""
    _set(monkeypatch, {})

    def path(mode, epi, M, N, K, **kw):
        p, tail = ops.gemm_plan(mode, epi, M, N, K, slots=256, **kw)
        return p.path, p.splitk, tail

    assert path(P.NT, P.F32, 248, 4096 * 4, 128, splitk=2, has_slabs=True)[0] == "nt128"          # M 248 / 256
    assert path(P.NT, P.F32, 256, 4096 * 4, 128, splitk=2, has_slabs=True)[0] == "nt8p"
    assert path(P.NT, P.BF16, 40960, 184, 128)[0] == "nt128" and path(P.NT, P.BF16, 40960, 192, 128)[0] == "nt8p"
    assert path(P.NT, P.BF16, 2560, 2560, 136)[0] == "nt128_ktail" and path(P.NT, P.BF16, 2560, 2560, 128)[0] == "nt8p"
    assert path(P.TN, P.F32, 512, 1024, 128)[0] == "tn8p" and path(P.TN, P.F32, 504, 1024, 128)[0] == "tn128"     # 8 tiles
    assert path(P.NT, P.BF16, 2560, 2560, 128)[0] == "nt8p" and path(P.NT, P.BF16, 2552, 2560, 128)[0] == "nt128"  # 100 tiles
    assert path(P.TN, P.F32, 2564, 2560, 128)[0] == "tn128" and path(P.TN, P.BF16, 2560, 2560, 128)[0] == "tn128"
    assert path(P.NT, P.BF16, 8192, 8192, 192)[0] == "nt8p_persistent"
    assert path(P.NT, P.BF16, 8192, 7936, 192) == ("nt8p", 1, (992, 0))                            # 992 tiles: 2 rem > S
    assert path(P.NT, P.BF16, 8192, 8192, 128) == ("nt8p", 1, (1024, 0))
    assert path(P.NT, P.BF16, 6144, 4096, 64) == ("nt8p", 1, (256, 128))                          # 2 rem == S
    assert path(P.NT, P.BF16, 6400, 4096, 64) == ("nt8p", 1, (400, 0))                            # 2 rem > S
    assert path(P.NT, P.F32, 1024, 768, 128, splitk=64, has_slabs=True) == ("nt8p", 2, (24, 0))   # more slices than K tiles
    with pytest.raises(RuntimeError, match="sc_gemm_bf16: split-K needs a dense C"):
        ops.gemm_plan(P.NT, P.F32, 1024, 768, 128, ldc=776, splitk=2, has_slabs=True)
    monkeypatch.setenv("SC_GEMM_COLGROUP", "-1:3")
    assert ops.gemm_plan(P.NT, P.BF16, 25600, 1024, 128)[0].col_group == 3                        # ntn 4
    assert ops.gemm_plan(P.NT, P.BF16, 25600, 768, 128)[0].col_group == 0                         # col_group >= ntn
    assert ops.gemm_plan(P.NT, P.BF16, 25600 * 4, 256, 128)[0].col_group == 0                     # ntn == 1


def test_unset_switches_are_the_default(monkeypatch):
    _set(monkeypatch, {})
    base = [ops.gemm_plan(P.NT, e, 8192, 8192, 192, slots=256) for e in range(9)]
    _set(monkeypatch, {"SC_GEMM_SMALL_TILES": "100", "SC_GEMM_PERSIST": "1", "SC_GEMM_TAIL": "256", "SC_GEMM_COLGROUP": "-1:0",
                       "SC_GELU_LUT": "1"})
    assert base == [ops.gemm_plan(P.NT, e, 8192, 8192, 192, slots=0) for e in range(9)]


@pytest.mark.parametrize("args,msg", [
    ((2, P.BF16, 256, 256, 64, 256, 1, 0, 0), "sc_gemm_bf16: bad mode 2"),
    ((P.NT, P.BF16, 0, 256, 64, 256, 1, 0, 0), "sc_gemm_bf16: empty problem"),
    ((P.NT, P.BF16, 256, 252, 64, 252, 1, 0, 0), "must be a multiple of 8"),
    ((P.NT, P.F32, 256, 254, 64, 256, 1, 0, 0), "must be a multiple of 4"),
    ((P.NT, P.F32, 256, 256, 64, 258, 1, 0, 0), "ldc (258) of 4"),
    ((P.NT, P.BF16, 256, 256, 68, 256, 1, 0, 0), "NT needs K % 8 == 0"),
    ((P.NT, P.BF16, 256, 256, 64, 256, 2, 1, 0), "split-K needs EPI_F32 + slabs"),
    ((P.NT, P.F32, 256, 256, 64, 256, 2, 0, 0), "split-K needs EPI_F32 + slabs"),
    ((P.NT, P.F32, 256, 256, 128, 264, 2, 1, 0), "sc_gemm_bf16: split-K needs a dense C"),
    ((P.TN, P.BF16_BIAS, 256, 256, 64, 256, 1, 0, 0), "sc_gemm_bf16: unsupported (mode=1, epi=1)"),
    ((P.NT, 12, 256, 256, 64, 256, 1, 0, 0), "sc_gemm_bf16: unsupported"),
    ((P.TN, P.F32, 258, 256, 64, 256, 1, 1, 1), "sc_gemm_wgrad_bias: bad shape")])
def test_refused_shapes_return_the_entry_points_message(args, msg):
    l = _lib.lib()
    mode, epi, M, N, K, ldc, splitk, has_slabs, colsum = args
    rc = l.sc_debug_gemm_plan(mode, epi, M, N, K, ldc, splitk, has_slabs, colsum, 256, None, 0)
    assert rc == -1 and msg.encode() in l.sc_last_error(), l.sc_last_error()
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        ops.gemm_plan(mode, epi, M, N, K, ldc=ldc, splitk=splitk, has_slabs=bool(has_slabs), colsum=bool(colsum))
    # sc_gemm_wgrad_bias / sc_gemm_bf16 say the same, before they look at the operands (no slab buffer is passed here)
    if colsum:
        assert l.sc_gemm_wgrad_bias(None, M, None, N, M, N, K, None, ldc, None, splitk, None, None) < 0
        assert msg.encode() in l.sc_last_error(), l.sc_last_error()
    elif not has_slabs:
        assert l.sc_gemm_bf16(mode, epi, None, K, None, K, M, N, K, None, ldc, None, 0, None, None, 0, None, 0, splitk,
                              None, None) < 0
        assert msg.encode() in l.sc_last_error(), l.sc_last_error()
