"""The tail-split rule of the 256x256 NT GEMM without a GPU (``ops.gemm_tail_rule`` -> sc_debug_gemm_tail_rule, the function
the launcher itself calls): T tiles on S workgroup slots are split into ``nfull`` full tiles and ``2 * rem`` half tiles when
T > S, rem = T % S > 0 and 2 rem <= S; otherwise the launch stays as it is."""
import pytest

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import ops


@pytest.mark.parametrize("T,S,want", [
    (591, 256, (512, 79)),        # the step's N = 768 launches: 2.31 rounds
    (2364, 256, (2304, 60)),      # the step's N = 3072 launches: 9.23 rounds
    (285, 256, (256, 29)),
    (104, 88, (88, 16)), (112, 96, (96, 16)), (117, 104, (104, 13)),
    (384, 256, (256, 128)),       # 2 rem == S: every CU gets one half tile
    (385, 256, (385, 0)),         # 2 rem > S
    (512, 256, (512, 0)),         # rem == 0
    (256, 256, (256, 0)), (200, 256, (200, 0)), (1, 256, (1, 0)),     # T <= S: one round
    (591, 0, (591, 0)), (591, -3, (591, 0)),                          # switched off
    (7, 2, (6, 1)), (3, 2, (2, 1)), (5, 3, (5, 0)),
])
def test_rule_cases(T, S, want):
    assert ops.gemm_tail_rule(T, S) == want


def test_rule_properties_over_a_sweep():
    for S in (1, 2, 3, 8, 88, 104, 255, 256, 304):
        for T in range(1, 4 * S + 3):
            nfull, rem = ops.gemm_tail_rule(T, S)
            assert nfull + rem == T and rem >= 0
            if rem:
                assert T > S and nfull % S == 0 and rem == T % S and 2 * rem <= S
                assert nfull + 2 * rem <= (T // S) * S + S            # the half tiles fit in one round of slots
            else:
                assert T <= S or T % S == 0 or 2 * (T % S) > S


def test_last_path_record_names_match_the_enums():
    """``ops.gemm_last_path`` without a GPU: no launch yet, so the record is empty, and the name tables have one entry per
    value of enum sc_gemm_path / sc_gemm_colsum / sc_gemm_group (csrc/sc_kernels.h)."""
    import os
    import re
    p = ops.gemm_last_path(reset=True)
    assert p == ops.GemmPath("none", False, 0, 0, "none", "none") and ops.gemm_last_path() == p
    src = open(os.path.join(os.path.dirname(ops.__file__), "csrc", "sc_kernels.h")).read()
    for enum, prefix, names in (("sc_gemm_path", "SC_GEMM_PATH_", ("none",) + ops.GEMM_PATHS),
                                ("sc_gemm_colsum", "SC_GEMM_COLSUM_", ops.GEMM_COLSUMS),
                                ("sc_gemm_group", "SC_GEMM_GROUP_", ops.GEMM_GROUPS)):
        body = re.search(r"enum %s \{(.*?)\};" % enum, src, re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        assert tuple(n.lower() for n in re.findall(prefix + r"(\w+)", body)) == names, enum
