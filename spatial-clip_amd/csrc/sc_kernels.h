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
// sc_debug_gemm_tail_rule: the tail-split rule of the 256x256 NT kernel for T tiles on S workgroup slots (sc_gemm_dispatch.hip).  Returns 1
// and (nfull, rem) = (T - T % S, T % S) when the last round is split into 2 rem half tiles, else 0 and (T, 0).  Host arithmetic only.
extern "C" int sc_debug_gemm_tail_rule(int T, int S, int* nfull, int* rem);
// sc_debug_gemm_last_tail: (nfull, rem) of this process's last launch of the non-persistent 256x256 NT kernel ((T, 0): not split;
// (-1, -1): none since the last reset); reset != 0 clears the record.
extern "C" int sc_debug_gemm_last_tail(int* nfull, int* rem, int reset);

// Which kernel the last GEMM entry point of this process (sc_gemm_bf16, sc_gemm_wgrad_bias, sc_gemm_wgrad_group, sc_gemm_fp8*,
// sc_gemm_wgrad_fp8) dispatched to.  Written by the entry points after the launch, host-side bookkeeping only (a few int stores per call); the
// tests assert with it that a shape reached the kernel they are named for.
enum sc_gemm_path {
    SC_GEMM_PATH_NONE = -1,
    SC_GEMM_PATH_NT128 = 0,        // 128x128 general kernel, K a multiple of 64
    SC_GEMM_PATH_NT128_KTAIL,      // the same with a partial last K tile
    SC_GEMM_PATH_TN128,
    SC_GEMM_PATH_NT8P,             // 256x256 phase-interleaved kernel, one workgroup per tile (its tail split: sc_debug_gemm_last_tail)
    SC_GEMM_PATH_NT8P_PERSISTENT,  // the persistent tile walk of the same kernel
    SC_GEMM_PATH_TN8P,
    SC_GEMM_PATH_TN8P_GROUP,       // sc_gemm_wgrad_group: several problems in one launch
    SC_GEMM_PATH_NT256,            // two-stage LDS-DMA kernel (SC_GEMM_FORCE=256 only)
    SC_GEMM_PATH_TN256,
    SC_GEMM_PATH_FP8_NT,
    SC_GEMM_PATH_FP8_TN
};
enum sc_gemm_colsum { SC_GEMM_COLSUM_NONE = 0, SC_GEMM_COLSUM_FUSED, SC_GEMM_COLSUM_SEPARATE };   // bias-gradient column sums
enum sc_gemm_group { SC_GEMM_GROUP_NONE = 0, SC_GEMM_GROUP_ONE_LAUNCH, SC_GEMM_GROUP_PER_PROBLEM };   // sc_gemm_wgrad_group
// sc_debug_gemm_last_path: out[0 .. n) = {path, GELU table attached (0 / 1), column group in effect (0: row-major walk), split-K
// actually used, sc_gemm_colsum, sc_gemm_group} of the last GEMM call (of the last problem, for a group that ran per problem);
// path SC_GEMM_PATH_NONE before the first call or after a reset.  reset != 0 clears the record.  Returns the number of fields.
extern "C" int sc_debug_gemm_last_path(int* out, int n, int reset);
// sc_debug_gemm_plan: what sc_gemm_bf16 (colsum == 0) or sc_gemm_wgrad_bias (colsum != 0: TN, fp32 out) would launch for this problem
// under the current environment switches on a device of `slots` CUs (<= 0: no tail split): out[0 .. n) = the six fields of
// sc_debug_gemm_last_path, then (nfull, rem) of sc_debug_gemm_last_tail.  The planner the entry points call; no HIP call.  -1 with
// the entry point's own message for a problem it refuses.
extern "C" int sc_debug_gemm_plan(int mode, int epi, int M, int N, int K, int ldc, int splitk, int has_slabs, int colsum,
                                  int slots, int* out, int n);
