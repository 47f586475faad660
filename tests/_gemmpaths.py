"""Which kernel sc_gemm_bf16 / sc_gemm_wgrad_bias dispatch a problem to, restated by hand from the entry points and the
launchers as they stood before the planner existed (sc_gemm_bf16 and sc_gemm_wgrad_bias in sc_gemm.hip, sc_gemm8p_try in
sc_gemm8p.hip, sc_gemm256_try in sc_gemm256.hip), and the shape lists the dispatch tests share.  Nothing here asks the
library: tests/test_cpu_gemm_dispatch.py asserts these records against ``ops.gemm_plan`` and tests/test_gpu_gemm_plan.py
asserts ``ops.gemm_plan`` against the kernel that ran.  No GPU.

Left out: the operand checks (alignment, leading dimensions of A / B / aux / C2), which do not depend on the shape."""
import re

NT, TN = 0, 1
(BF16, BF16_BIAS, F32_BIAS_RES, GELU_PAIR, BF16_DGELU, F32, BF16_BIAS_RES, GELU_GRAD_PAIR, BF16_MUL_AUX, QGELU_PAIR,
 BF16_DQGELU, QGELU_GRAD_PAIR) = range(12)
EPIS = tuple(range(12))
_BASE = {QGELU_PAIR: GELU_PAIR, BF16_DQGELU: BF16_DGELU, QGELU_GRAD_PAIR: GELU_GRAD_PAIR}     # sc_epi_base

SWITCHES = ("SC_GEMM_FORCE", "SC_GEMM_SMALL_TILES", "SC_GEMM_PERSIST", "SC_GEMM_TAIL", "SC_GEMM_COLGROUP", "SC_GELU_LUT")
# every switch flipped alone from its default (unset)
ENVS = [{}, {"SC_GEMM_FORCE": "128"}, {"SC_GEMM_FORCE": "256"}, {"SC_GEMM_SMALL_TILES": "0"}, {"SC_GEMM_SMALL_TILES": "8"},
        {"SC_GEMM_PERSIST": "0"}, {"SC_GEMM_TAIL": "0"}, {"SC_GEMM_TAIL": "7"}, {"SC_GEMM_COLGROUP": "-1:3"},
        {"SC_GELU_LUT": "0"}]

TILE = 256 * 256


def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def _off(env, name):
    """An opt-out switch: off when its value starts with 0."""
    return env.get(name, "")[:1] == "0"


def tail_rule(T, S):
    """sc_debug_gemm_tail_rule: (nfull, rem), (T, 0) when the last round is not split."""
    r = T % S if (S > 0 and T > S) else 0
    return (T - r, r) if (r > 0 and 2 * r <= S) else (T, 0)


def splitk_plan(ktiles, req, has_slabs):
    """splitk_plan (sc_gemm8p.hip), and its inline copies in sc_gemm256_try and sc_gemm_bf16."""
    sk = 1 if (req < 1 or not has_slabs) else req
    sk = min(sk, ktiles)
    per = -(-ktiles // sk)
    return -(-ktiles // per)


def big_tile(env, mode, M, N, K, splitk_req):
    """What sc_gemm8p_try, sc_gemm256_try and sc_gemm8p_tn_group_plan each ask first: enough work for 256x256 tiles, whole K
    tiles, and for NT without split-K an area of at least SC_GEMM_SMALL_TILES (100) tiles."""
    if M < 256 or N < 192 or K % 64:
        return False
    if mode == TN and (M % 8 or N % 8):
        return False
    if M * N < 8 * TILE:
        return False
    if mode == NT and splitk_req <= 1:
        small = _atoi(env["SC_GEMM_SMALL_TILES"]) if "SC_GEMM_SMALL_TILES" in env else 100
        if M * N < small * TILE:
            return False
    return True


def _colgroup(env, epi, ntn):
    gc = 0
    p = env.get("SC_GEMM_COLGROUP")
    while p:
        m = re.match(r"\s*([+-]?\d+):", p)
        if not m:
            break
        v = re.match(r"\s*[+-]?\d+", p[m.end():])
        val, rest = (int(v.group()), p[m.end() + v.end():]) if v else (0, p[m.end():])
        if int(m.group(1)) in (epi, -1):
            gc = val
        if not rest.startswith(","):
            break
        p = rest[1:]
    return gc if 0 < gc < ntn else 0


def _rec(path, lut=False, col_group=0, splitk=1, colsum="none", tail=(-1, -1)):
    return (path, lut, col_group, splitk, colsum, "none"), tail


def expected(env, slots, mode, epi, M, N, K, ldc, splitk, has_slabs, colsum=False):
    """((path, lut, col_group, splitk, colsum, group), (nfull, rem)) as ``ops.gemm_last_path`` / ``ops.gemm_last_tail`` report
    them after the call ((-1, -1): the non-persistent 256x256 NT kernel did not run), or the refusal's message as a string.
    ``colsum``: the call is sc_gemm_wgrad_bias (TN, fp32 out, workspace always there), else sc_gemm_bf16."""
    if colsum:
        if not (M > 0 and N > 0 and K > 0 and M % 4 == 0 and N % 4 == 0):
            return "sc_gemm_wgrad_bias: bad shape"
        mode, epi, has_slabs = TN, F32, True
    epi = _BASE.get(epi, epi)
    if mode not in (NT, TN):
        return "sc_gemm_bf16: bad mode"
    if not (M > 0 and N > 0 and K > 0):
        return "sc_gemm_bf16: empty problem"
    if N % (4 if epi in (F32, F32_BIAS_RES) else 8) or ldc % 4:
        return "must be a multiple of"
    if mode == NT and K % 8:
        return "NT needs K % 8 == 0"
    splitk = max(splitk, 1)
    if splitk > 1 and not (epi == F32 and has_slabs):
        return "split-K needs EPI_F32 + slabs"
    fused = "fused" if colsum else "none"
    force = env.get("SC_GEMM_FORCE")
    slabs_ok = epi == F32 and has_slabs
    ntm, ntn = -(-M // 256), -(-N // 256)
    big = big_tile(env, mode, M, N, K, splitk)
    sk = splitk_plan(K // 64, splitk, slabs_ok) if big else 1
    dense = sk == 1 or ldc == N
    # 1. the phase-interleaved 256x256 kernels, unless a kernel is pinned
    if force is None and big and dense and (mode == NT or epi == F32):
        T = ntm * ntn * sk
        if mode == TN:
            return _rec("tn8p", splitk=sk, colsum=fused)
        lut = epi == GELU_GRAD_PAIR and not _off(env, "SC_GELU_LUT")
        if (not lut and not _off(env, "SC_GEMM_PERSIST") and sk == 1 and T >= 1024 and K // 64 >= 3
                and epi in (BF16, BF16_BIAS, GELU_PAIR, GELU_GRAD_PAIR)):
            return _rec("nt8p_persistent")
        cg = _colgroup(env, epi, ntn) if (sk == 1 and ntn > 1) else 0
        tail = (T, 0)
        if sk == 1:
            tail = tail_rule(T, _atoi(env["SC_GEMM_TAIL"]) if "SC_GEMM_TAIL" in env else slots)
        return _rec("nt8p", lut, cg, sk, tail=tail)
    # 2. the two-stage 256x256 kernel: SC_GEMM_FORCE=256 (unpinned it sees only what the first kernel also refuses)
    if (force is None or force[:1] == "2") and big and dense and (mode == NT or epi == F32):
        return _rec("nt256" if mode == NT else "tn256", splitk=sk, colsum=fused)
    # 3. the 128x128 general kernel
    if mode == TN and epi not in (F32, BF16):
        return "sc_gemm_bf16: unsupported"
    sk = splitk_plan(-(-K // 64), splitk, True)
    if sk > 1 and ldc != N:
        return "split-K needs a dense C"
    path = "tn128" if mode == TN else "nt128_ktail" if K % 64 else "nt128"
    return _rec(path, splitk=sk, colsum="separate" if colsum else "none")


# ---------------------------------------------------------------------------------------------------- shapes
# (M, N, K): both sides of every boundary of the rule.  K is 1-3 K tiles unless the boundary is about K.
SHAPES = [
    (248, 1024, 128), (256, 2048, 128),              # M 248 / 256 (256 x 2048: 8 tiles exactly)
    (2816, 184, 128), (2816, 192, 128),              # N 184 / 192
    (2560, 2560, 136), (2560, 2560, 128),            # K % 64 != 0 with K % 8 == 0 (the NT K-tail kernel) / whole K tiles
    (504, 1024, 128), (512, 1024, 128),              # one step below 8 tiles' area, and 8 tiles exactly
    (2552, 2560, 128), (2560, 2560, 192),            # one step below the 100-tile threshold, and 100 tiles exactly
    (2564, 2564, 128), (2560, 2572, 128),            # TN with M % 8 != 0 / N % 8 != 0
    (8192, 8192, 192), (8192, 7936, 192), (8192, 8192, 128),     # persistent: 1024 tiles x 3 K tiles, 992 tiles, 2 K tiles
    (25600, 256, 128), (25600, 768, 128),            # ntn == 1; ntn == 3: col_group 3 >= ntn
    (25600, 1024, 128),                              # ntn == 4: col_group 3 in effect
    (6656, 4096, 64), (6400, 4096, 64),              # 416 / 400 tiles: on 256 slots rem = 160 / 144, 2 rem > S
    (6144, 4096, 64), (6912, 4096, 64),              # 384 tiles: rem = 128, 2 rem == S exactly; 432 tiles: rem = 176
    (2560, 2816, 64), (2816, 2816, 64),              # 110 / 121 tiles: rem = 6 / 17 on 104 slots, 14 / 25 on 96, 0 / 1 on 5
    (1024, 768, 384), (1024, 768, 64),               # split-K: 6 K tiles; more slices asked than K tiles
    (128, 64, 64), (8, 8, 8),                        # toy shapes
]
SPLITKS = (1, 2, 4, 64)
SLOTS = (0, 5, 96, 104, 256)


def ldcs(N):
    return (N, N + 8)


# ---------------------------------------------------------------------------------------------------- launch list
# What tests/test_gpu_gemm_plan.py launches and tests/golden/gemm_paths_parent.json records:
# (entry point, mode, epilogue name, M, N, K, split-K, environment).  entry: "gemm", "wgrad_bias", or "wgrad_group" (two
# problems: this one and its transpose-shaped twin N x M, the first with a bias gradient).
def _l(entry, mode, epi, M, N, K, splitk=1, **env):
    return (entry, mode, epi, M, N, K, splitk, env)


LAUNCHES = [
    _l("gemm", NT, "BF16", 248, 1024, 128), _l("gemm", NT, "BF16", 2560, 2560, 128), _l("gemm", NT, "BF16", 2552, 2560, 128),
    _l("gemm", NT, "BF16_BIAS", 2560, 2560, 136), _l("gemm", NT, "F32", 2816, 184, 128), _l("gemm", NT, "F32", 2816, 192, 128, 2),
    _l("gemm", NT, "F32", 512, 1024, 192, 2), _l("gemm", NT, "F32", 504, 1024, 192, 2), _l("gemm", NT, "F32", 1024, 768, 64, 4),
    _l("gemm", NT, "GELU_GRAD_PAIR", 2560, 2816, 64), _l("gemm", NT, "GELU_GRAD_PAIR", 2560, 2816, 64, SC_GELU_LUT="0"),
    _l("gemm", NT, "BF16", 8192, 8192, 192), _l("gemm", NT, "BF16", 8192, 7936, 192), _l("gemm", NT, "BF16_BIAS", 8192, 8192, 128),
    _l("gemm", NT, "BF16", 8192, 8192, 192, SC_GEMM_PERSIST="0"),
    _l("gemm", NT, "BF16", 6656, 4096, 64), _l("gemm", NT, "BF16", 6144, 4096, 64),
    _l("gemm", NT, "BF16", 25600, 1024, 128, SC_GEMM_COLGROUP="-1:3"), _l("gemm", NT, "BF16", 25600, 768, 128, SC_GEMM_COLGROUP="-1:3"),
    _l("gemm", NT, "BF16", 2560, 2816, 64, SC_GEMM_TAIL="104"), _l("gemm", NT, "BF16", 2560, 2816, 64, SC_GEMM_TAIL="0"),
    _l("gemm", NT, "BF16", 2552, 2560, 128, SC_GEMM_SMALL_TILES="0"), _l("gemm", NT, "BF16", 512, 1024, 128, SC_GEMM_SMALL_TILES="8"),
    _l("gemm", NT, "BF16", 2560, 2560, 128, SC_GEMM_FORCE="128"), _l("gemm", NT, "BF16_BIAS", 2560, 2560, 128, SC_GEMM_FORCE="256"),
    _l("gemm", TN, "F32", 2560, 2560, 128), _l("gemm", TN, "F32", 2564, 2564, 128), _l("gemm", TN, "BF16", 2560, 2560, 128),
    _l("gemm", TN, "F32", 512, 1024, 192, 2), _l("gemm", TN, "F32", 504, 1024, 192, 2),
    _l("gemm", TN, "F32", 512, 1024, 192, 2, SC_GEMM_FORCE="256"), _l("gemm", TN, "F32", 512, 1024, 192, 2, SC_GEMM_FORCE="128"),
    _l("wgrad_bias", TN, "F32", 768, 2304, 192, 2), _l("wgrad_bias", TN, "F32", 248, 1024, 192, 2),
    _l("wgrad_bias", TN, "F32", 768, 2304, 192, 2, SC_GEMM_FORCE="256"), _l("wgrad_bias", TN, "F32", 768, 2304, 192, 2, SC_GEMM_FORCE="128"),
    _l("wgrad_group", TN, "F32", 768, 2304, 192, 2), _l("wgrad_group", TN, "F32", 768, 184, 192, 2),
    _l("wgrad_group", TN, "F32", 768, 2304, 192, 2, SC_GEMM_FORCE="128"),
]


def launch_key(case):
    entry, mode, epi, M, N, K, splitk, env = case
    return "%s %s %s %dx%dx%d sk%d %s" % (entry, "NT" if mode == NT else "TN", epi, M, N, K, splitk,
                                          ",".join("%s=%s" % kv for kv in sorted(env.items())) or "-")
