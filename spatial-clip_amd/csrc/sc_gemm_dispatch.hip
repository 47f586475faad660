// Which kernel a matrix product runs on: the switches, the planner, the path table, the C entry points of the bf16 / e4m3 GEMMs
// and the debug records.  The kernels and their launch functions are in sc_gemm.hip (128x128 general kernel, slab reduction),
// sc_gemm256.hip (256x256 two-stage LDS-DMA kernel) and sc_gemm8p.hip (256x256 phase-interleaved kernels).
// Part 1 (switches, planner) is host arithmetic: no HIP call, nothing written outside its result; sc_debug_gemm_plan runs it
// without a device (tools/gemm_plan_host.cpp: the same under the host sanitizers).
#include "sc_gemm_common.h"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------------------------------------- part 1: switches
// The environment, parsed once per entry-point call (tests and A/B runs flip a switch inside one process).
struct GemmSwitches {
    enum { UNPINNED = 1, PIN256 = 2, PIN128 = 4 };
    int force = UNPINNED;             // SC_GEMM_FORCE: 256 pins the two-stage kernel, any other value the 128x128 kernel
    int small_tiles = 100;            // SC_GEMM_SMALL_TILES: big_tile() below; 0 = never
    bool persist = true;              // SC_GEMM_PERSIST=0: no persistent tile walk
    bool tail_set = false;            // SC_GEMM_TAIL: unset = the tail rule with the device's CU count for every launch class,
    int tail = 0;                     //   0 = off, <n> = the rule with S = n (the result does not depend on S);
    bool tail256 = false;             //   =1 also opts gemm256_kernel into its own tail split (below)
    int col_group[9] = {};            // SC_GEMM_COLGROUP="<epi>:<Gc>[,<epi>:<Gc>...]" (<epi> -1: all): column groups of Gc tiles
    bool gelu_lut = true;             // SC_GELU_LUT=0: the GELU epilogues evaluate the formula
};

GemmSwitches gemm_switches() {
    GemmSwitches s;
    if (const char* e = getenv("SC_GEMM_FORCE")) s.force = e[0] == '2' ? GemmSwitches::PIN256 : GemmSwitches::PIN128;
    if (const char* e = getenv("SC_GEMM_SMALL_TILES")) s.small_tiles = atoi(e);
    if (const char* e = getenv("SC_GEMM_PERSIST")) s.persist = e[0] != '0';
    if (const char* e = getenv("SC_GEMM_TAIL")) { s.tail_set = true; s.tail = atoi(e); s.tail256 = e[0] == '1'; }
    if (const char* e = getenv("SC_GELU_LUT")) s.gelu_lut = e[0] != '0';
    // Which launches take the column-group walk by default (measured per launch class: profiles/r05_gemm_colgroup.txt): none.
    if (const char* sw = getenv("SC_GEMM_COLGROUP")) {
        for (const char* p = sw; *p;) {
            char* e = nullptr;
            const long ep = strtol(p, &e, 10);
            if (e == p || *e != ':') break;
            const long v = strtol(e + 1, &e, 10);
            for (int i = 0; i < 9; ++i)
                if (ep == i || ep == -1) s.col_group[i] = (int)v;
            p = (*e == ',') ? e + 1 : e;
            if (*e != ',') break;
        }
    }
    return s;
}

// ---------------------------------------------------------------------------------------------- part 1: the planner
struct GemmProblem {
    int mode, epi, M, N, K, ldc;      // epi: a base epilogue (sc_epi_base)
    int splitk;                       // as requested, >= 1
    bool has_slabs;                   // there is a slab buffer to split K through
    bool colsum;                      // column sums of the At operand are wanted (sc_gemm_wgrad_bias)
};

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Split-K plan: `req` slices (one without slabs to reduce through) over ktiles K tiles, evened out so that no slice is empty.
// Returns the slice count; *tiles_per = K tiles per slice.
int splitk_plan(int ktiles, int req, bool has_slabs, int* tiles_per) {
    int splitk = (req < 1 || !has_slabs) ? 1 : req;
    if (splitk > ktiles) splitk = ktiles;
    *tiles_per = ceil_div(ktiles, splitk);
    return ceil_div(ktiles, *tiles_per);
}

// Tail split of the non-persistent NT kernel.  T tiles on S workgroup slots (one 140-KiB workgroup per CU) run in ceil(T / S)
// rounds, and the last one keeps only rem = T % S of the S CUs busy.  When rem <= S / 2 those rem tiles are launched as 2 rem
// half tiles (128 rows each, dispatched last), one per CU: the last round then costs a half tile's time instead of a tile's.
// With more than S / 2 tiles in the last round the halves would not all find a free CU at once; with T <= S there is one round.
bool tail_rule(int T, int S, int* nfull, int* rem) {
    const int r = (S > 0 && T > S) ? T % S : 0;
    const bool split = r > 0 && 2 * r <= S;
    if (nfull) *nfull = split ? T - r : T;
    if (rem) *rem = split ? r : 0;
    return split;
}

// The 256x256 kernels' common condition: enough work for their tiles, whole K tiles, operands that allow clamped 16-byte chunks.
// NT launches with fewer 256x256 tiles than ~0.4 of the chip's CUs go to the 128x128 general kernel: four times the
// workgroups, two of them per CU.  Measured (tools/bench_small_m.py, profiles/r06_small_m_kernel_choice.txt; the token
// counts of ViT-B-32 + CLIP text tower at the reference's batch 32): 20-84 tiles 1.08-1.52x faster on the small kernel,
// 150 tiles and more 1.1-1.5x faster on the big ones.  SC_GEMM_SMALL_TILES=<n> moves the threshold (0: never).
bool big_tile(int mode, int M, int N, int K, int splitk_req, const GemmSwitches& sw) {
    if (M < 256 || N < 192 || (K % 64) != 0) return false;
    if (mode == SC_GEMM_TN && ((M % 8) != 0 || (N % 8) != 0)) return false;
    const long long work = (long long)M * N;
    if (work < 256LL * 256 * 8) return false;
    return !(mode == SC_GEMM_NT && splitk_req <= 1 && work < 256LL * 256 * sw.small_tiles);
}

// one workgroup per tile and split-K slice; false = more than a grid holds
bool plan_grid(GemmPlan& p) {
    const long long tiles = (long long)p.ntm * p.ntn * p.splitk;
    p.tiles = p.grid = (int)tiles;
    return tiles <= 0x7fffffffLL;
}

// What the three 256x256 families share: the condition above, the tile counts and the split-K plan
bool plan_tiles256(const GemmProblem& q, const GemmSwitches& sw, int, GemmPlan& p) {
    if (!big_tile(q.mode, q.M, q.N, q.K, q.splitk, sw) || (q.mode == SC_GEMM_TN && q.epi != SC_EPI_F32)) return false;
    p.ntm = ceil_div(q.M, 256);
    p.ntn = ceil_div(q.N, 256);
    int tiles_per = 0;
    p.splitk = splitk_plan(q.K / 64, q.splitk, q.epi == SC_EPI_F32 && q.has_slabs, &tiles_per);
    p.k_per_split = tiles_per * 64;
    if (p.splitk > 1 && q.ldc != q.N) return false;              // the slabs are dense
    if (!plan_grid(p)) return false;
    p.lds = p.lds_max = SC_GEMM256_LDS;
    p.colsum = q.colsum ? SC_GEMM_COLSUM_FUSED : SC_GEMM_COLSUM_NONE;
    return true;
}

// GELU by table: only the non-persistent kernel has LDS to spare for it (the persistent one fills all 160 KiB)
bool lut_wanted(const GemmProblem& q, const GemmSwitches& sw) { return q.epi == SC_EPI_GELU_GRAD_PAIR && sw.gelu_lut; }

// persistent walk of the tile list for the store-only bf16 epilogues once there are >= 4 rounds of tiles (measured: +7 % at 7
// rounds, -3 % at 2.3; GELU pair: +1.5 % at 9.2 rounds)
bool plan_nt8p_persistent(const GemmProblem& q, const GemmSwitches& sw, int, GemmPlan& p) {
    if (!sw.persist || lut_wanted(q, sw) || !plan_tiles256(q, sw, 0, p)) return false;
    if (p.splitk != 1 || p.tiles < 1024 || q.K / 64 < 3) return false;
    if (q.epi != SC_EPI_BF16 && q.epi != SC_EPI_BF16_BIAS && q.epi != SC_EPI_GELU_PAIR && q.epi != SC_EPI_GELU_GRAD_PAIR) return false;
    p.grid = 256;
    p.lds = p.lds_max = SC_GEMM8PP_LDS;
    return true;
}

bool plan_nt8p(const GemmProblem& q, const GemmSwitches& sw, int slots, GemmPlan& p) {
    if (!plan_tiles256(q, sw, 0, p)) return false;
    p.lut = lut_wanted(q, sw);
    // tile walk: column groups of Gc tiles inside per-XCD row bands (sc_tile_colgroup)
    const int gc = sw.col_group[q.epi];
    if (p.splitk == 1 && gc > 0 && gc < p.ntn) {
        p.col_group = gc;
        p.band_rows = ceil_div(p.ntm, 8);                        // an XCD's contiguous share of the remapped tile list
    }
    // Tail split.  Which launch classes take it by default: measured per class on the step's shapes (M = 50 432, alone on the
    // chip, switch off -> on, profiles/gemm_tail_summary.txt): N = 768 (591 tiles, 2.31 rounds) plain K = 768 / 2304 / 3072
    // 67.6 -> 61.2 / 165.2 -> 153.4 / 213.7 -> 199.4 us, bf16 residual K = 768 / 3072 82.6 -> 72.0 / 237.2 -> 215.2, fp32
    // residual K = 768 117.2 -> 108.8; N = 3072 (2 364 tiles, 9.23 rounds) act-pair 303.1 -> 295.9, x act' 278.8 -> 274.6.
    // Every class gains, the short-K ones (where a half tile's fixed prologue and epilogue weigh most) the most: none is excluded.
    p.lds_max = SC_GEMM8P_HALF_LDS;
    int nfull = 0, rem = 0;
    if (p.splitk == 1 && tail_rule(p.tiles, sw.tail_set ? sw.tail : slots, &nfull, &rem)) {
        p.tail_first = nfull;
        p.tail_rem = rem;
        p.grid = nfull + 2 * rem;
        p.lds = SC_GEMM8P_HALF_LDS;                              // a launch with half tiles needs their nine-slot ring
    }
    return true;
}


// full rounds with whole tiles, then the remainder cut into halves / quarters so that it still covers the chip.  Measured
// (interleaved A/B on one MI355X, ViT-B/16 step): splitting the last round is 0.4 ms/step SLOWER than leaving it whole --
// workgroups are not in lockstep rounds, the hardware backfills; opt-in only (SC_GEMM_TAIL=1)
bool plan_256(const GemmProblem& q, const GemmSwitches& sw, int, GemmPlan& p) {
    if (!plan_tiles256(q, sw, 0, p)) return false;
    const int CUS = 256, rem = p.tiles % CUS;
    if (sw.tail256 && p.splitk == 1 && !q.colsum && p.tiles > CUS && rem > 0) {
        p.tail_parts = rem * 4 <= CUS ? 4 : rem * 2 <= CUS + 64 ? 2 : 0;
        if (p.tail_parts) { p.tail_first = p.tiles - rem; p.tail_rem = rem; }
    }
    return true;
}

// the 128x128 general kernel: any shape; the column sums of a weight gradient come from a kernel of their own
bool plan_128(const GemmProblem& q, const GemmSwitches&, int, GemmPlan& p) {
    if (q.mode == SC_GEMM_TN && q.epi != SC_EPI_F32 && q.epi != SC_EPI_BF16) return false;
    p.ntm = ceil_div(q.M, 128);
    p.ntn = ceil_div(q.N, 128);
    int tiles_per = 0;
    p.splitk = splitk_plan(ceil_div(q.K, 64), q.splitk, true, &tiles_per);
    p.k_per_split = tiles_per * 64;
    if (p.splitk > 1 && q.ldc != q.N) {
        p.refused = "split-K needs a dense C (ldc == N)";
        return false;
    }
    if (!plan_grid(p)) return false;
    p.lds = p.lds_max = SC_GEMM128_LDS;
    p.colsum = q.colsum ? SC_GEMM_COLSUM_SEPARATE : SC_GEMM_COLSUM_NONE;
    return true;
}
bool plan_128_ktail(const GemmProblem& q, const GemmSwitches& sw, int s, GemmPlan& p) { return (q.K % 64) != 0 && plan_128(q, sw, s, p); }

// ---------------------------------------------------------------------------------------------- part 1: the path table
// Which kernel runs a problem: the first row, in table order, of the problem's mode that SC_GEMM_FORCE admits and whose `accepts`
// takes the problem (filling the plan).  Phase-interleaved 256x256 kernels -> two-stage 256x256 kernel (which takes nothing the first would not:
// it runs when pinned, for A/B benchmarking) -> 128x128 general kernel.
struct GemmPath {
    int id;                           // enum sc_gemm_path
    int force;                        // the SC_GEMM_FORCE settings under which the row is tried
    int mode;
    bool (*accepts)(const GemmProblem&, const GemmSwitches&, int slots, GemmPlan&);
    int (*launch)(int mode, int epi, const GemmPlan&, const GemmArgs&, hipStream_t);
};
constexpr int UNPINNED = GemmSwitches::UNPINNED, OR_256 = UNPINNED | GemmSwitches::PIN256, ANY = OR_256 | GemmSwitches::PIN128;
const GemmPath gemm_paths[] = {
    {SC_GEMM_PATH_NT8P_PERSISTENT, UNPINNED, SC_GEMM_NT, plan_nt8p_persistent, sc_gemm8p_launch},
    {SC_GEMM_PATH_NT8P, UNPINNED, SC_GEMM_NT, plan_nt8p, sc_gemm8p_launch},
    {SC_GEMM_PATH_TN8P, UNPINNED, SC_GEMM_TN, plan_tiles256, sc_gemm8p_launch},
    {SC_GEMM_PATH_NT256, OR_256, SC_GEMM_NT, plan_256, sc_gemm256_launch},
    {SC_GEMM_PATH_TN256, OR_256, SC_GEMM_TN, plan_256, sc_gemm256_launch},
    {SC_GEMM_PATH_NT128_KTAIL, ANY, SC_GEMM_NT, plan_128_ktail, sc_gemm128_launch},
    {SC_GEMM_PATH_NT128, ANY, SC_GEMM_NT, plan_128, sc_gemm128_launch},
    {SC_GEMM_PATH_TN128, ANY, SC_GEMM_TN, plan_128, sc_gemm128_launch},
};

// `slots`: the workgroup slots the tail rule counts with (<= 0: no tail split) unless SC_GEMM_TAIL names a count
GemmPlan gemm_plan(const GemmProblem& q, const GemmSwitches& sw, int slots, const GemmPath** row = nullptr) {
    const char* refused = "unsupported";
    for (const GemmPath& e : gemm_paths) {
        GemmPlan p;
        if ((e.force & sw.force) && e.mode == q.mode && e.accepts(q, sw, slots, p)) {
            p.path = e.id;
            if (row) *row = &e;
            return p;
        }
        if (p.refused) refused = p.refused;
    }
    GemmPlan none;
    none.refused = refused;
    return none;
}

// (nfull, rem) as sc_debug_gemm_last_tail reports a launch of this plan
void plan_tail(const GemmPlan& p, int* tail) {
    const bool nt8p = p.path == SC_GEMM_PATH_NT8P;
    tail[0] = !nt8p ? -1 : p.tail_first > 0 ? p.tail_first : p.tiles;
    tail[1] = nt8p ? p.tail_rem : -1;
}

// what sc_gemm_bf16 asks of a shape before it looks at the operands (sc_debug_gemm_plan asks the same)
int gemm_validate(const char* who, int mode, int epi, int M, int N, int K, int ldc, int splitk, bool has_slabs) {
    SC_CHECK(mode == SC_GEMM_NT || mode == SC_GEMM_TN, "%s: bad mode %d", who, mode);
    SC_CHECK(M > 0 && N > 0 && K > 0, "%s: empty problem M=%d N=%d K=%d", who, M, N, K);
    SC_CHECK(epi >= 0 && epi <= SC_EPI_BF16_MUL_AUX, "%s: unsupported (mode=%d, epi=%d)", who, mode, epi);
    const bool f32out = (epi == SC_EPI_F32 || epi == SC_EPI_F32_BIAS_RES);
    SC_CHECK((N % (f32out ? 4 : 8)) == 0 && (ldc % 4) == 0, "%s: N (%d) must be a multiple of %d, ldc (%d) of 4", who, N,
             f32out ? 4 : 8, ldc);
    if (mode == SC_GEMM_NT) SC_CHECK((K % 8) == 0, "%s: NT needs K %% 8 == 0 (K=%d)", who, K);
    SC_CHECK(splitk <= 1 || (epi == SC_EPI_F32 && has_slabs), "%s: split-K needs EPI_F32 + slabs", who);
    return 0;
}
// ... and of the operands: whole 16-byte chunks
int gemm_check_operands(const char* who, const void* A, long long lda, const void* B, long long ldb, const void* C) {
    SC_CHECK((lda % 8) == 0 && (ldb % 8) == 0, "%s: lda/ldb (%lld,%lld) must be multiples of 8", who, lda, ldb);
    SC_CHECK(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && ((uintptr_t)C % 16) == 0, "%s: operands must be 16-byte aligned", who);
    return 0;
}
int wgrad_validate(int M, int N, int K) {
    SC_CHECK(M > 0 && N > 0 && K > 0 && (M % 4) == 0 && (N % 4) == 0, "sc_gemm_wgrad_bias: bad shape M=%d N=%d K=%d", M, N, K);
    return 0;
}

// the records behind sc_debug_gemm_last_path / sc_debug_gemm_last_tail (sc_kernels.h): host-side bookkeeping for tests, written
// after a launch succeeded
int sc_last_path[6] = {SC_GEMM_PATH_NONE, 0, 0, 0, SC_GEMM_COLSUM_NONE, SC_GEMM_GROUP_NONE};
int sc_last_tail[2] = {-1, -1};

}  // namespace

extern "C" int sc_debug_gemm_tail_rule(int T, int S, int* nfull, int* rem) { return tail_rule(T, S, nfull, rem) ? 1 : 0; }

extern "C" int sc_debug_gemm_last_tail(int* nfull, int* rem, int reset) {
    if (nfull) *nfull = sc_last_tail[0];
    if (rem) *rem = sc_last_tail[1];
    if (reset) sc_last_tail[0] = sc_last_tail[1] = -1;
    return 0;
}

void sc_gemm_note_path(int path, int lut, int col_group, int splitk, int colsum) {
    sc_last_path[0] = path; sc_last_path[1] = lut; sc_last_path[2] = col_group; sc_last_path[3] = splitk;
    sc_last_path[4] = colsum; sc_last_path[5] = SC_GEMM_GROUP_NONE;
}
extern "C" int sc_debug_gemm_last_path(int* out, int n, int reset) {
    for (int i = 0; i < n && i < 6; ++i) out[i] = sc_last_path[i];
    if (reset) sc_gemm_note_path(SC_GEMM_PATH_NONE, 0, 0, 0, SC_GEMM_COLSUM_NONE);
    return 6;
}

bool sc_gemm_lut_wanted() { return gemm_switches().gelu_lut; }

// The plan sc_gemm_bf16 (colsum == 0) or sc_gemm_wgrad_bias (colsum != 0) would launch under the current environment on a device
// of `slots` CUs: out[0 .. n) = the six fields of sc_debug_gemm_last_path, then nfull and rem of sc_debug_gemm_last_tail.
extern "C" int sc_debug_gemm_plan(int mode, int epi, int M, int N, int K, int ldc, int splitk, int has_slabs, int colsum,
                                  int slots, int* out, int n) {
    const char* who = colsum ? "sc_gemm_wgrad_bias" : "sc_gemm_bf16";
    if (colsum) {
        if (wgrad_validate(M, N, K)) return -1;
        mode = SC_GEMM_TN; epi = SC_EPI_F32; has_slabs = 1;
    }
    epi = sc_epi_base(epi);
    if (splitk < 1) splitk = 1;
    if (gemm_validate(who, mode, epi, M, N, K, ldc, splitk, has_slabs != 0)) return -1;
    const GemmPlan p = gemm_plan({mode, epi, M, N, K, ldc, splitk, has_slabs != 0, colsum != 0}, gemm_switches(), slots);
    SC_CHECK(p.path != SC_GEMM_PATH_NONE, "sc_gemm_bf16: %s (mode=%d, epi=%d)", p.refused, mode, epi);
    int rec[8] = {p.path, p.lut, p.col_group, p.splitk, p.colsum, SC_GEMM_GROUP_NONE, 0, 0};
    plan_tail(p, rec + 6);
    for (int i = 0; i < n && i < 8; ++i) out[i] = rec[i];
    return 0;
}

// ---------------------------------------------------------------------------------------------- part 2: launch from a plan
// workgroup slots of the current device = its CU count (queried once per device)
static int sc_gemm_slots() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = -1;
        cus[dev] = n;
    }
    return cus[dev] > 0 ? cus[dev] : 0;
}

// tile counts and split-K plan into g; with more than one slice the kernel writes the slabs
static void gemm_args_plan(GemmArgs& g, int ntm, int ntn, int splitk, int k_per_split, float* slabs) {
    g.ntm = ntm; g.ntn = ntn; g.splitk = splitk; g.k_per_split = k_per_split;
    if (splitk > 1) { g.C = slabs; g.slab_stride = (long long)g.M * g.N; }
}

// Plan, launch and record one problem.  g holds the operands (g.C the final output); with more than one split-K slice the
// kernel writes the slabs and the caller reduces them (*plan says how many).
static int gemm_run(const GemmProblem& q, const GemmSwitches& sw, GemmArgs g, float* slabs, float* cs_part, hipStream_t st,
                    GemmPlan* plan) {
    const GemmPath* row = nullptr;
    // the CU count matters to the tail rule alone, which only an unpinned NT launch without SC_GEMM_TAIL asks
    const bool count = q.mode == SC_GEMM_NT && !sw.tail_set && sw.force == GemmSwitches::UNPINNED;
    const GemmPlan p = gemm_plan(q, sw, count ? sc_gemm_slots() : 0, &row);
    // (a refusal by the planner names sc_gemm_bf16 for every entry point, as it always has: callers match on it)
    SC_CHECK(p.path != SC_GEMM_PATH_NONE, "sc_gemm_bf16: %s (mode=%d, epi=%d)", p.refused, q.mode, q.epi);
    gemm_args_plan(g, p.ntm, p.ntn, p.splitk, p.k_per_split, slabs);
    g.col_group = p.col_group; g.band_rows = p.band_rows; g.tail_first = p.tail_first; g.tail_rem = p.tail_rem;
    if (p.colsum == SC_GEMM_COLSUM_FUSED) g.colsum = cs_part;
    if (p.lut) g.gelu_lut = sc_gelu_lut_device(st, g.act);
    if (const int rc = row->launch(q.mode, q.epi, p, g, st)) return rc;
    sc_gemm_note_path(p.path, g.gelu_lut != nullptr, p.col_group, p.splitk, p.colsum);
    if (p.path == SC_GEMM_PATH_NT8P) plan_tail(p, sc_last_tail);
    *plan = p;
    return 0;
}

// ---------------------------------------------------------------------------------------------- the C ABI
extern "C" int sc_gemm_bf16(int mode, int epi, const void* A, int lda, const void* B, int ldb, int M, int N, int K,
                            void* C, int ldc, void* C2, int ldc2, const float* bias, const void* res, int ldres,
                            const void* aux, int ldaux, int splitk, float* slabs, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int act = sc_epi_act(epi);          // SC_EPI_QGELU_*: the erf twin's kernel instance with the activation flag set
    epi = sc_epi_base(epi);
    if (splitk < 1) splitk = 1;
    if (gemm_validate("sc_gemm_bf16", mode, epi, M, N, K, ldc, splitk, slabs != nullptr)) return -1;
    if (gemm_check_operands("sc_gemm_bf16", A, lda, B, ldb, C)) return -1;
    SC_CHECK(!sc_epi_aux_mul(epi) || (aux != nullptr && (ldaux % 8) == 0), "sc_gemm_bf16: epilogue %d needs aux (ldaux %% 8 == 0)", epi);
    SC_CHECK(!sc_epi_gelu_fwd(epi) || (C2 != nullptr && (ldc2 % 8) == 0), "sc_gemm_bf16: epilogue %d needs the second output C2", epi);
    GemmArgs g = sc_gemm_args(A, lda, B, ldb, M, N, K, C, ldc);
    g.C2 = C2; g.ldc2 = ldc2; g.bias = bias; g.res = (const float*)res; g.ldres = ldres;
    g.aux = (const bf16*)aux; g.ldaux = ldaux; g.act = act;
    GemmPlan p;
    if (const int rc = gemm_run({mode, epi, M, N, K, ldc, splitk, slabs != nullptr, false}, gemm_switches(), g, slabs, nullptr, st, &p))
        return rc;
    return p.splitk > 1 ? sc_reduce_slabs_launch({(float*)C, slabs, M, N, nullptr, nullptr}, p.splitk, st) : 0;
}

extern "C" long long sc_gemm_slab_floats(int M, int N, int K, int splitk) {
    int ktiles = (K + 63) / 64;
    if (splitk < 1) splitk = 1;
    if (splitk > ktiles) splitk = ktiles;
    return splitk > 1 ? (long long)splitk * M * N : 0;
}

// Weight gradient + bias gradient of one Linear in one pass: dW[M,N] = dY[K,M]^T . X[K,N] (fp32) and
// dbias[M] = column sums of dY, fused into the TN kernel when a 256x256 kernel takes the problem.
extern "C" long long sc_gemm_wgrad_ws_floats(int M, int N, int K, int splitk) {
    long long a = sc_gemm_slab_floats(M, N, K, splitk);
    int sk = splitk < 1 ? 1 : splitk;
    long long b = (long long)sk * M + sc_colsum_ws_floats(K, M);
    return a + b + 64;
}

extern "C" int sc_gemm_wgrad_bias(const void* dY, int lddy, const void* X, int ldx, int M, int N, int K, float* dW,
                                  int ldw, float* dbias, int splitk, float* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (wgrad_validate(M, N, K)) return -1;
    SC_CHECK(ws != nullptr && dbias != nullptr, "sc_gemm_wgrad_bias: workspace / dbias required");
    if (splitk < 1) splitk = 1;
    // every kernel moves whole 16-byte chunks: asked on the fused path too, which used to launch unchecked
    if (gemm_validate("sc_gemm_wgrad_bias", SC_GEMM_TN, SC_EPI_F32, M, N, K, ldw, splitk, true)) return -1;
    if (gemm_check_operands("sc_gemm_wgrad_bias", dY, lddy, X, ldx, dW)) return -1;
    float* slabs = ws;
    float* cs_part = ws + ((sc_gemm_slab_floats(M, N, K, splitk) + 15) / 16) * 16;
    GemmPlan p;
    if (const int rc = gemm_run({SC_GEMM_TN, SC_EPI_F32, M, N, K, ldw, splitk, true, true}, gemm_switches(),
                                sc_gemm_args(dY, lddy, X, ldx, M, N, K, dW, ldw), slabs, cs_part, st, &p))
        return rc;
    const float* red = p.splitk > 1 ? slabs : nullptr;
    if (p.colsum == SC_GEMM_COLSUM_FUSED) return sc_reduce_slabs_launch({dW, red, M, N, dbias, cs_part}, p.splitk, st);
    // general kernel: separate GEMM and column-sum kernels
    if (red)
        if (const int rc = sc_reduce_slabs_launch({dW, red, M, N, nullptr, nullptr}, p.splitk, st)) return rc;
    return sc_colsum_bf16(dY, lddy, K, M, dbias, cs_part, stream);
}

// ---- e4m3 weight (+ bias) gradient: dW[M,N] = s_dy s_x sum_k dY8[k,m] X8[k,n], per-tensor scales (include/spatial_clip_hip.h) ----
extern "C" int sc_gemm_wgrad_fp8(const void* dY8, long long lddy, const float* dy_scale_inv, const void* X8, long long ldx,
                                 const float* x_scale_inv, int M, int N, int K, float* dW, int ldw, float* dbias, int splitk,
                                 float* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SC_CHECK(M > 0 && N > 0 && K > 0 && dY8 && X8 && dW && ws && dy_scale_inv && x_scale_inv, "sc_gemm_wgrad_fp8: null / empty argument");
    SC_CHECK((lddy % 16) == 0 && (ldx % 16) == 0 && ((uintptr_t)dY8 % 16) == 0 && ((uintptr_t)X8 % 16) == 0 && ((uintptr_t)dW % 16) == 0,
             "sc_gemm_wgrad_fp8: operand rows must be 16-byte aligned (lddy=%lld ldx=%lld)", lddy, ldx);
    SC_CHECK(ldw == N, "sc_gemm_wgrad_fp8: dW must be dense (ldw == N)");
    SC_CHECK(M >= 256 && N >= 192 && (K % 128) == 0 && (M % 16) == 0 && (N % 16) == 0,
             "sc_gemm_wgrad_fp8: shape outside the kernel's range (M=%d N=%d K=%d: M >= 256, N >= 192, M %% 16 == N %% 16 == 0, K %% 128 == 0)", M, N, K);
    const long long slab_floats = sc_gemm_slab_floats(M, N, K, splitk);
    float* slabs = ws;
    float* cs_part = ws + ((slab_floats + 15) / 16) * 16;
    GemmArgs g = sc_gemm_args(dY8, lddy, X8, ldx, M, N, K, dW, ldw);             // lda / ldb in bytes
    int tiles_per = 0;
    const int sk = splitk_plan(K / 128, splitk, slab_floats != 0, &tiles_per);
    gemm_args_plan(g, ceil_div(M, 256), ceil_div(N, 256), sk, tiles_per * 128, slabs);
    g.colsum = dbias ? cs_part : nullptr;
    g.a_scale = dy_scale_inv; g.b_scale = x_scale_inv;
    if (const int rc = sc_gemm8p_tn_fp8_launch(g, st)) return rc;
    sc_gemm_note_path(SC_GEMM_PATH_FP8_TN, 0, 0, g.splitk, dbias ? SC_GEMM_COLSUM_FUSED : SC_GEMM_COLSUM_NONE);
    if (g.splitk > 1 || dbias != nullptr)
        return sc_reduce_slabs_launch({dW, g.splitk > 1 ? slabs : nullptr, M, N, dbias, cs_part}, g.splitk, st);
    return 0;
}

// ---- several weight (+ bias) gradients over one token axis in one launch (include/spatial_clip_hip.h) ----
static long long wgrad_group_layout(const sc_wgrad_desc* d, int n, int K, int splitk, long long* slab_off, long long* cs_off) {
    // workspace = per problem [splitk slabs of M x N | splitk partial column sums of M], 16-float aligned; the plain
    // per-problem path (sc_gemm_wgrad_bias) must fit too
    long long off = 0, worst_single = 0;
    const int sk = splitk < 1 ? 1 : splitk;
    for (int p = 0; p < n; ++p) {
        if (slab_off) slab_off[p] = off;
        off += ((long long)sk * d[p].M * d[p].N + 15) / 16 * 16;
        if (cs_off) cs_off[p] = off;
        off += ((long long)sk * d[p].M + 15) / 16 * 16;
        const long long single = sc_gemm_wgrad_ws_floats(d[p].M, d[p].N, K, splitk);
        if (single > worst_single) worst_single = single;
    }
    return (off > worst_single ? off : worst_single) + 64;
}

extern "C" long long sc_gemm_wgrad_group_ws_floats(const sc_wgrad_desc* descs, int n, int K, int splitk) {
    if (descs == nullptr || n < 1 || n > SC_WGRAD_GROUP_MAX) return 0;
    return wgrad_group_layout(descs, n, K, splitk, nullptr, nullptr);
}

extern "C" int sc_gemm_wgrad_group(const sc_wgrad_desc* descs, int n, int K, int splitk, float* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SC_CHECK(descs != nullptr && n >= 1 && n <= SC_WGRAD_GROUP_MAX, "sc_gemm_wgrad_group: 1..%d problems (n=%d)", SC_WGRAD_GROUP_MAX, n);
    SC_CHECK(K > 0 && ws != nullptr, "sc_gemm_wgrad_group: K=%d, workspace required", K);
    const GemmSwitches sw = gemm_switches();
    // one launch: more than one problem, no kernel pinned, every problem inside the 256x256 kernels' range (dW is dense)
    bool grouped = n > 1 && sw.force == GemmSwitches::UNPINNED;
    bool sums = false;
    for (int p = 0; p < n; ++p) {
        const sc_wgrad_desc& d = descs[p];
        SC_CHECK(d.M > 0 && d.N > 0 && (d.M % 4) == 0 && (d.N % 4) == 0 && d.dY && d.X && d.dW,
                 "sc_gemm_wgrad_group: problem %d: bad shape M=%d N=%d", p, d.M, d.N);
        if (gemm_check_operands("sc_gemm_wgrad_group", d.dY, d.lddy, d.X, d.ldx, d.dW)) return -1;
        grouped = grouped && big_tile(SC_GEMM_TN, d.M, d.N, K, splitk, sw);
        sums = sums || d.dbias != nullptr;
    }
    if (grouped) {
        int tiles_per = 0;
        const int sk = splitk_plan(K / 64, splitk, true, &tiles_per);
        long long slab_off[SC_WGRAD_GROUP_MAX], cs_off[SC_WGRAD_GROUP_MAX];
        (void)wgrad_group_layout(descs, n, K, sk, slab_off, cs_off);
        GemmArgs g[SC_WGRAD_GROUP_MAX] = {};
        ReduceOne r[SC_WGRAD_GROUP_MAX] = {};
        for (int p = 0; p < n; ++p) {
            const sc_wgrad_desc& d = descs[p];
            float* slabs = sk > 1 ? ws + slab_off[p] : nullptr;
            g[p] = sc_gemm_args(d.dY, d.lddy, d.X, d.ldx, d.M, d.N, K, d.dW, d.N);
            gemm_args_plan(g[p], ceil_div(d.M, 256), ceil_div(d.N, 256), sk, tiles_per * 64, slabs);
            g[p].colsum = d.dbias ? ws + cs_off[p] : nullptr;
            r[p] = {d.dW, slabs, d.M, d.N, d.dbias, ws + cs_off[p]};
        }
        if (const int rc = sc_gemm8p_tn_group_launch(g, n, st)) return rc;
        sc_gemm_note_path(SC_GEMM_PATH_TN8P_GROUP, 0, 0, sk, sums ? SC_GEMM_COLSUM_FUSED : SC_GEMM_COLSUM_NONE);
        sc_last_path[5] = SC_GEMM_GROUP_ONE_LAUNCH;
        return (sk > 1 || sums) ? sc_reduce_slabs_group_launch(r, n, sk, st) : 0;
    }
    // outside the 256x256 kernel's range (toy shapes) or a single problem: one by one through the per-Linear entry points
    for (int p = 0; p < n; ++p) {
        const sc_wgrad_desc& d = descs[p];
        int rc;
        if (d.dbias) {
            rc = sc_gemm_wgrad_bias(d.dY, (int)d.lddy, d.X, (int)d.ldx, d.M, d.N, K, d.dW, d.N, d.dbias, splitk, ws, stream);
        } else {
            const long long sf = sc_gemm_slab_floats(d.M, d.N, K, splitk);
            rc = sc_gemm_bf16(SC_GEMM_TN, SC_EPI_F32, d.dY, (int)d.lddy, d.X, (int)d.ldx, d.M, d.N, K, d.dW, d.N, nullptr, 0,
                              nullptr, nullptr, 0, nullptr, 0, sf ? splitk : 1, sf ? ws : nullptr, stream);
        }
        if (rc != 0) return rc;
    }
    sc_last_path[5] = SC_GEMM_GROUP_PER_PROBLEM;
    return 0;
}
