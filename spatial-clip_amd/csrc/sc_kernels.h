// Internal alias of the public C ABI header (include/spatial_clip_hip.h).
#pragma once
#include "../../include/spatial_clip_hip.h"

// Which kernel the last sc_attn_fwd / sc_attn_bwd of this process dispatched to (sc_debug_attn_last_path; tests assert that
// a forced path really ran).  Host-side bookkeeping only: one int store per call.
enum sc_attn_path {
    SC_ATTN_PATH_NONE = -1,
    // forward
    SC_ATTN_FWD_PERSISTENT = 0, SC_ATTN_FWD_PERSISTENT2, SC_ATTN_FWD_PER_HEAD, SC_ATTN_FWD_STREAM,
    // backward
    SC_ATTN_BWD_CLS = 0, SC_ATTN_BWD_RING, SC_ATTN_BWD_RING8, SC_ATTN_BWD_SINGLE_PASS, SC_ATTN_BWD_PERSISTENT,
    SC_ATTN_BWD_FUSED, SC_ATTN_BWD_DQ_DKV, SC_ATTN_BWD_STREAM
};

// Debug exports (not in the public header).  sc_debug_attn_plan: the paths the next sc_attn_fwd / sc_attn_bwd of this shape would
// take under the current environment switches; -1 with sc_attn_fwd's own message for a shape they refuse.  No HIP call.
extern "C" int sc_debug_attn_last_path(int* fwd, int* bwd);
extern "C" int sc_debug_attn_plan(int B, int L, int H, int dh, int causal, int q_rows, int* fwd, int* bwd);
// sc_debug_gemm_tail_rule: the tail-split rule of the 256x256 NT kernel for T tiles on S workgroup slots (sc_gemm8p.hip).  Returns 1
// and (nfull, rem) = (T - T % S, T % S) when the last round is split into 2 rem half tiles, else 0 and (T, 0).  Host arithmetic only.
extern "C" int sc_debug_gemm_tail_rule(int T, int S, int* nfull, int* rem);
// sc_debug_gemm_last_tail: (nfull, rem) of this process's last launch of the non-persistent 256x256 NT kernel ((T, 0): not split;
// (-1, -1): none since the last reset); reset != 0 clears the record.
extern "C" int sc_debug_gemm_last_tail(int* nfull, int* rem, int reset);
