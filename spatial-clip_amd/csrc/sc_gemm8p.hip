// 256x256x64 MFMA GEMMs with a phase-interleaved ("ping-pong") main loop, gfx950: bf16 and e4m3 operands, NT and TN layouts.
// The schedule is described for the bf16 NT kernel; the others differ in their operand policy only.
//
//   8 waves (2 x 4), each wave a 128x64 output tile (128 accumulator VGPRs) cut into four 64x32 quadrants.
//   A K tile (64 deep) is four phases, one quadrant each: {fragment ds_reads + 2 LDS-DMA of a later half-tile ->
//   s_barrier -> 16 MFMA -> s_barrier}.  Waves 4-7 run one barrier behind waves 0-3, and wave w shares its SIMD
//   with wave w+4, so on every SIMD one wave is in its MFMA section while its partner reads LDS / issues DMA:
//   the matrix pipe never waits for a fragment read, and the DMA never waits for the matrix pipe.
//
//   Operand tiles live in LDS as HALF-TILES of 128 rows x 64 k (16 KiB, 128-B rows, same XOR swizzle as
//   sc_gemm256.hip): A half i holds, for each of the two M-waves, rows [64 i, 64 i + 64) of its 128 rows; B half j
//   holds, for each of the four N-waves, columns [32 j, 32 j + 32) of its 64.  Ring = 2 K tiles x 4 half-tiles
//   = 128 KiB.  Half-tiles are staged in the order they are consumed (A0, B0, B1, A1), six half-tiles ahead of the
//   phase that issues them, with a counted `s_waitcnt vmcnt(8)` (four half-tiles stay in flight across the barriers).
//
//   Ordering rules the schedule is built on:
//     RAW: a half-tile is read one phase after the phase whose load section waited for it (every wave waits for its
//          own DMA, the barrier that follows publishes it to the other waves -- including the staggered group);
//     WAR: a ring slot is restaged at the earliest two phases after the phase that read it (the staggered group
//          retires its reads one barrier later than the leading group).
//   Epilogue: bf16 outputs without an extra input tile take a bf16 LDS strip (epilogue_bf16_lds); the others the
//   fp32 LDS staging shared with sc_gemm256.hip (sc_gemm_common.h).
//
//   Layout of this file: the operand policies (bf16 NT, e4m3 NT, bf16 TN, e4m3 TN: fragment types, reads, waits, MFMAs,
//   staging), then the schedules written once over them (phase / ktile, hphase, pphase), then the six kernels
//   (gemm8p_kernel, gemm8pp_kernel, gemm8p_tn_kernel, gemm8p_tn_group_kernel, gemm8p_tn_f8_kernel, gemm8p_f8_kernel), then
//   the host side (launch_lds, epi_dispatch, splitk_plan and the entry points).
//
//   Tail split (non-persistent kernel, splitk == 1): the tiles of a launch's partial last round run as HALF TILES of 128 rows
//   (half_tile below: two phases and three images per K tile, nine-slot ring -- the same two rules, derived there), one per
//   CU, so the round costs a half tile's time.  Which launches: tail_rule / plan_nt8p in sc_gemm_dispatch.hip.
#include "sc_gemm_common.h"
#include <map>
#include <mutex>
#include <type_traits>

namespace {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int HALF = 128 * 64 * 2;                  // 16 KiB half-tile
constexpr int RING = 8 * HALF;                      // 128 KiB
constexpr int EPI_BYTES = 8 * 64 * SC_EPI_LD * 4;   // 139264 (LDS-staged epilogues)
constexpr int LDS_BYTES = EPI_BYTES > RING ? EPI_BYTES : RING;

// bf16 epilogue through a small wave-private LDS strip (4 KiB: 32 rows x 128 B), four passes per 128x64 wave tile.
// Why: a store instruction that writes whole 128-B lines (8 rows x 128 B) retires 3.7x faster than the 16 rows x 64 B
// an accumulator-layout store touches (tools/micro/store_pattern.hip: 1.0 vs 3.8 us per 256x256 bf16 tile on one CU),
// and an un-retired store holds back every later LDS-DMA of the same wave (vmcnt retires in order).  The accumulators
// are packed to bf16 BEFORE the LDS trip (half the LDS bytes of the fp32 staging in sc_gemm_common.h), 16-B chunks
// XOR-swizzled by row so the 8-B writes (2-way at worst) and 16-B reads spread over the banks.
//   BF16 / BF16_BIAS: C = bf16(acc (+ bias));  GELU_PAIR: C = u = bf16(acc + bias), C2 = bf16(gelu(float(u)));
//   GELU_GRAD_PAIR: C = bf16(gelu'(float(u))), C2 as before, u itself is not stored.
// NI = 16-row accumulator blocks of the wave tile: 8 (128 rows, four passes) or 4 (the 64 rows of a half tile, two passes).
template <int EPI, bool Q8 = false, bool LUT = false, int NI = 8>
SC_DEVICE void epilogue_bf16_lds(f32x4 (&acc)[NI][4], const GemmArgs& g, char* strip, int row0, int col0, int lane,
                                 const unsigned* lut = nullptr) {
    float amax_lane = 0.f;
    const float q8s = (Q8 && sc_epi_gelu_fwd(EPI) && g.q8) ? *g.q8_scale : 0.f;
    const int li = lane & 15, lg = lane >> 4;
    constexpr bool kBias = (EPI == SC_EPI_BF16_BIAS || sc_epi_gelu_fwd(EPI));
    f32x4 bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bj[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int c = col0 + j * 16 + lg * 4;
        if (kBias && g.bias && c < g.N) bj[j] = *reinterpret_cast<const f32x4*>(g.bias + c);
    }
    bf16* C = reinterpret_cast<bf16*>(g.C);
    bf16* C2 = reinterpret_cast<bf16*>(g.C2);
    const int rr = lane >> 3, rc = lane & 7;                      // read side: row (+ 8 s), 16-B chunk
    const int gcol = col0 + rc * 8;
#pragma unroll
    for (int p = 0; p < NI / 2; ++p) {
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) {
            const int r = ib * 16 + li;                           // strip row
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = acc[p * 2 + ib][j] + bj[j];
                const int chunk = (j * 2 + (lg >> 1)) ^ (r & 7);
                *reinterpret_cast<u32x2*>(strip + r * 128 + chunk * 16 + (lg & 1) * 8) = sc_pack4(v[0], v[1], v[2], v[3]);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int r = s4 * 8 + rr;
            const u32x4 u = *reinterpret_cast<const u32x4*>(strip + r * 128 + ((rc ^ (r & 7)) << 4));
            const int grow = row0 + p * 32 + r;
            if (grow < g.M && gcol < g.N) {
                if (EPI != SC_EPI_GELU_GRAD_PAIR) *reinterpret_cast<u32x4*>(C + (size_t)grow * g.ldc + gcol) = u;
                if (sc_epi_gelu_fwd(EPI)) {
                    union { u32x4 w; bf16x8 h; } x;
                    x.w = u;
                    bf16x8 o;
                    if (EPI == SC_EPI_GELU_PAIR) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[e] = (bf16)sc_act((float)x.h[e], g.act);
                    } else {                             // the backward's factor gelu'(u) instead of u
                        bf16x8 gd;
                        bool formula = true;
                        if (LUT) {                       // both values by table (SC_GELU_LUT_*): same bits as the formula
                            unsigned ent[8];
                            bool inside = true;
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const unsigned bits = (u[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
                                const unsigned rel = (bits & 0x7FFFu) - (unsigned)SC_GELU_LUT_LO;
                                inside = inside && rel < (unsigned)SC_GELU_LUT_HALF;
                                const unsigned idx = min(rel, (unsigned)SC_GELU_LUT_HALF - 1u) + (bits >> 15) * (unsigned)SC_GELU_LUT_HALF;
                                ent[e] = lut[idx];
                            }
                            formula = __builtin_amdgcn_ballot_w64(!inside) != 0;      // wave-uniform
                            if (!formula) {
                                union { u32x4 w; bf16x8 h; } lo, hi;
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    lo.w[q] = __builtin_amdgcn_perm(ent[2 * q + 1], ent[2 * q], 0x05040100u);
                                    hi.w[q] = __builtin_amdgcn_perm(ent[2 * q + 1], ent[2 * q], 0x07060302u);
                                }
                                o = lo.h;
                                gd = hi.h;
                            }
                        }
                        if (formula) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                float hv, gv;
                                sc_act_both((float)x.h[e], g.act, hv, gv);
                                o[e] = (bf16)hv;
                                gd[e] = (bf16)gv;
                            }
                        }
                        *reinterpret_cast<bf16x8*>(C + (size_t)grow * g.ldc + gcol) = gd;
                    }
                    *reinterpret_cast<bf16x8*>(C2 + (size_t)grow * g.ldc2 + gcol) = o;
                    if (Q8 && g.q8) {                    // e4m3 copy of h for the c_proj forward GEMM (GemmArgs::q8)
                        float r[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) { r[e] = (float)o[e]; amax_lane = fmaxf(amax_lane, fabsf(r[e])); }
                        *reinterpret_cast<u32x2*>(g.q8 + (size_t)grow * g.ldq8 + gcol) = sc_pack8_fp8(r, q8s);
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
    if (Q8 && sc_epi_gelu_fwd(EPI) && g.q8) sc_amax_publish(amax_lane, g.q8_amax);
}

// ring slot of half-tile q (0: A half 0, 1: B half 0, 2: B half 1, 3: A half 1) of the K tile with parity D
constexpr int slot(int D, int q) { return D * 4 * HALF + q * HALF; }

// the barrier the two wave groups meet at, fenced so that the compiler moves nothing across it
SC_DEVICE void fenced_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// =====================================================================================================================
// Operand policies: what really differs between the kernels of this file.  A policy names its fragment types and supplies
//   read_a<Q> / read_b<Q>   the fragment reads from half-tile Q of the K tile image set at `par`,
//   wait_a / wait_b         the hand-written lgkmcnt wait that names the registers it retires (empty where the compiler
//                           sees the reads),
//   mfma<MI, NJ, NEWA>      the MFMAs of quadrant (MI, NJ); NEWA = the A fragments are used for the first time, which is when
//                           the TN policies take their fused column sum (their extra arguments do_cs, wc, cs: the `hook`
//                           pack of the schedules, empty for NT),
//   stage(S, q, ts, dst)    the two LDS-DMA pieces of half-tile q of K tile ts, with its source addressing.
// The schedules below (phase / hphase / pphase) are written once over these pieces.
struct Stager {
    const bf16* src[4][2];      // [q][p] : this lane's source of the two 1-KiB pieces it copies per half-tile
    int nt;
    int wave;
};

struct OpsNT {                  // NT layout: what the bf16 and the e4m3 kernel share (per-lane source pointers, visible reads)
    typedef Stager Src;
    typedef const char* Ring;
    typedef int Off;
    static constexpr int NOA = 2, NOB = 2;
    static SC_DEVICE Ring ring(char* smem) { return smem; }
    // the two 1-KiB pieces of one half-tile, `eoff` elements along K behind the lane's sources
    static SC_DEVICE void stage_pair(const bf16* s0, const bf16* s1, long long eoff, char* dst, int wave) {
        dma16(s0 + eoff, dst + wave * 1024);
        dma16(s1 + eoff, dst + (8 + wave) * 1024);
    }
    static SC_DEVICE void stage(const Stager& S, int q, int ts, char* dst) {
        stage_pair(S.src[q][0], S.src[q][1], (size_t)ts * BK, dst, S.wave);
    }
    template <class F>
    static SC_DEVICE void wait_a(F&) {}
    template <class F>
    static SC_DEVICE void wait_b(F&) {}
};

struct OpsNT16 : OpsNT {        // bf16 NT
    typedef bf16x8 Frag;
    static constexpr int NA = 8, NB = 4;
    template <int Q>
    static SC_DEVICE void read_a(const char* par, const int (&a_off)[2], bf16x8 (&a)[8]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
                a[kk * 4 + ii] = *reinterpret_cast<const bf16x8*>(par + Q * HALF + a_off[kk] + ii * 2048);
    }
    template <int Q>
    static SC_DEVICE void read_b(const char* par, const int (&b_off)[2], bf16x8 (&b)[4]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
                b[kk * 2 + jj] = *reinterpret_cast<const bf16x8*>(par + Q * HALF + b_off[kk] + jj * 2048);
    }
    template <int MI, int NJ, bool NEWA, int NI>
    static SC_DEVICE void mfma(const bf16x8 (&a)[8], const bf16x8 (&b)[4], f32x4 (&acc)[NI][4]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
                    acc[MI * 4 + ii][NJ * 2 + jj] = sc_mfma16(b[kk * 2 + jj], a[kk * 4 + ii], acc[MI * 4 + ii][NJ * 2 + jj]);
    }
};

// FP8 (OCP e4m3) NT: the same tile, ring, phase schedule and epilogues on one-byte operands.  A half-tile row
// is still 128 bytes, i.e. 128 k values instead of 64, so the staging stream, swizzle and waits are byte-for-byte the
// bf16 kernel's; the caller passes K / 2, lda / 2, ldb / 2 ("bf16 elements") and the MFMA section issues ONE
// v_mfma_scale_f32_16x16x128_f8f6f4 per fragment pair where the bf16 kernel issues two 16x16x32: half the MFMA count
// for twice the k per tile = 2x the matrix rate.  Operand layout (probed with integer data, tools/micro/
// mfma_fp8_layout.hip): lane (g = lane >> 4, r = lane & 15) supplies row r and the 32 consecutive k of bytes
// [32 g, 32 g + 32) of the 128-byte row = the two 16-byte chunks 2g, 2g + 1; the block scales are E8M0 1.0 -- the real
// scales are per-row floats applied to the accumulators before the epilogue:
//     C[m][n] = a_scale[m] * b_scale[n] * sum_k A8[m][k] B8[n][k]   (+ bias, residual, GELU as in the bf16 kernel).
// Block scales of the f8f6f4 MFMA.  Unit scales two ways: E8M0 127 (= 2^0) in the scale registers of the SCALED opcode
// (v_mfma_scale_..., a 16-byte encoding that loads the scales in front of every MFMA), or the constant 0, for which the compiler
// selects the UNSCALED opcode v_mfma_f32_16x16x128_f8f6f4 (8-byte encoding, no scale load; the scales are implicitly one).
// -DSC_F8_SCALED_OPCODE keeps the first form (A/B; tests/test_gpu_fp8.py's exact-integer tests pin the arithmetic of either).
#ifdef SC_F8_SCALED_OPCODE
#define SC_F8_UNIT_SCALE 0x7F7F7F7F
#else
#define SC_F8_UNIT_SCALE 0
#endif
typedef __attribute__((ext_vector_type(8))) int i32x8;
SC_DEVICE f32x4 mfma_f8(i32x8 b, i32x8 a, f32x4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, 0, 0, 0, SC_F8_UNIT_SCALE, 0, SC_F8_UNIT_SCALE);
}
struct Frag8 {
    union { i32x8 v; u32x4 h[2]; };
};

struct OpsNT8 : OpsNT {         // e4m3 NT
    typedef Frag8 Frag;
    static constexpr int NA = 4, NB = 2;
    template <int Q>
    static SC_DEVICE void read_a(const char* par, const int (&a_off)[2], Frag8 (&a)[4]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
                a[ii].h[kk] = *reinterpret_cast<const u32x4*>(par + Q * HALF + a_off[kk] + ii * 2048);
    }
    template <int Q>
    static SC_DEVICE void read_b(const char* par, const int (&b_off)[2], Frag8 (&b)[2]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
                b[jj].h[kk] = *reinterpret_cast<const u32x4*>(par + Q * HALF + b_off[kk] + jj * 2048);
    }
    template <int MI, int NJ, bool NEWA, int NI>
    static SC_DEVICE void mfma(const Frag8 (&a)[4], const Frag8 (&b)[2], f32x4 (&acc)[NI][4]) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
                acc[MI * 4 + ii][NJ * 2 + jj] = mfma_f8(b[jj].v, a[ii].v, acc[MI * 4 + ii][NJ * 2 + jj]);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// TN layout (weight gradients): C[m,n] = sum_k At[k,m] Bt[k,n], both operands k-major in global memory.
//   Half-tile image = [64 k][128 columns] bf16 (256-B rows); A half i = tile columns [128 i, 128 i + 128), of which
//   M-wave wr owns [64 wr, 64 wr + 64); B half j likewise with N-wave wc owning [32 wc, 32 wc + 32) -- so a wave's
//   128x64 output is rows {128 i + 64 wr + ..} x columns {128 j + 32 wc + ..} (2 x 2 blocks of 64 x 32), and every
//   DMA row is one contiguous 256-B run of the source.  Fragments come out of LDS through ds_read_b64_tr_b16 (inline
//   asm + hand-placed lgkmcnt: see sc_gemm_common.h), 32-B chunk ^= (k & 3) | ((k >> 3) & 1) << 2 keeps the 8 rows a
//   32-lane half touches on distinct banks.  Phase / ring schedule identical to the NT kernel.
struct StagerTN {
    // wave-uniform base (SGPRs) + 32-bit per-lane byte offset: the DMA takes the scalar-base addressing form (no address VALU, 4
    // VGPRs instead of 16; with 64-bit pointers the e4m3 kernel spilled them and reloaded one before every DMA); piece 1 of a
    // half-tile is half a K tile of source rows behind piece 0 = a scalar addend (step / 2)
    const char* base[4];
    unsigned off[4];
    long long step[4];          // BYTES per K tile (bf16: 64 source rows, e4m3: 128) for each half-tile kind
    int nt;
    int wave;
};
struct OpsTN {                  // TN layout: what the bf16 and the e4m3 kernel share (scalar-base sources, asm reads)
    typedef StagerTN Src;
    typedef unsigned Ring;      // LDS byte address: the operand of the asm reads
    typedef unsigned Off;
    static constexpr int NOA = 4, NOB = 2;
    static SC_DEVICE Ring ring(char* smem) { return (unsigned)(uintptr_t)(lptr_t)smem; }
    // PIN = false: the prologue's DMAs, which run once and never needed the pin
    template <bool PIN = true>
    static SC_DEVICE void stage(const StagerTN& S, int q, int ts, char* dst) {
        const char* kb = S.base[q] + ts * S.step[q];
        unsigned o0 = S.off[q];
        if (PIN) asm volatile("" : "+v"(o0));      // keep (scalar base + 32-bit offset): no hoisted 64-bit sums, which cost 2 VGPRs each
        dma16(kb + o0, dst + S.wave * 1024);
        dma16(kb + (S.step[q] >> 1) + o0, dst + (8 + S.wave) * 1024);
    }
};

struct FragTN {                 // one operand fragment set: [kk][f] as two 64-bit halves
    u32x2 lo, hi;
};
struct OpsTN16 : OpsTN {        // bf16 TN
    typedef FragTN Frag;
    static constexpr int NA = 8, NB = 4;
    template <int NF>
    static SC_DEVICE void read(unsigned base, const unsigned (&off)[NF], FragTN (&f)[2 * NF]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int x = 0; x < NF; ++x) {
                if (kk == 0) {
                    f[x].lo = tr16_asm<0>(base + off[x]);
                    f[x].hi = tr16_asm<1024>(base + off[x]);
                } else {
                    f[NF + x].lo = tr16_asm<8192>(base + off[x]);
                    f[NF + x].hi = tr16_asm<8192 + 1024>(base + off[x]);
                }
            }
    }
    template <int Q>
    static SC_DEVICE void read_a(unsigned par, const unsigned (&a_off)[4], FragTN (&a)[8]) { read<4>(par + Q * HALF, a_off, a); }
    template <int Q>
    static SC_DEVICE void read_b(unsigned par, const unsigned (&b_off)[2], FragTN (&b)[4]) { read<2>(par + Q * HALF, b_off, b); }
    // The asm reads above are invisible to hipcc's waitcnt pass, so the wait is written by hand -- and it must NAME the
    // registers it retires ("+v"): a clobber-only `s_waitcnt` orders memory, not registers, and the compiler may copy or
    // consume an asm-loaded register in front of it (seen in the attention kernels).  Same pattern as
    // tr_wait / tr_wait_b in sc_gemm256.hip.
    static SC_DEVICE void wait_b(FragTN (&f)[4]) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi), "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo),
                       "+v"(f[3].hi)
                     :: "memory");
    }
    static SC_DEVICE void wait_a(FragTN (&f)[8]) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi), "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo),
                       "+v"(f[3].hi), "+v"(f[4].lo), "+v"(f[4].hi), "+v"(f[5].lo), "+v"(f[5].hi), "+v"(f[6].lo), "+v"(f[6].hi),
                       "+v"(f[7].lo), "+v"(f[7].hi)
                     :: "memory");
    }
    template <int MI, int NJ, bool NEWA>
    static SC_DEVICE void mfma(const FragTN (&a)[8], const FragTN (&b)[4], f32x4 (&acc)[8][4], bool do_cs, int wc, float* cs) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const bf16x8 af = tr_cat(a[kk * 4 + ii].lo, a[kk * 4 + ii].hi);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const FragTN& bf = b[kk * 2 + jj];
                    acc[MI * 4 + ii][NJ * 2 + jj] = sc_mfma16(tr_cat(bf.lo, bf.hi), af, acc[MI * 4 + ii][NJ * 2 + jj]);
                }
                // fused bias gradient: column sums of At over this K tile, one 16-column fragment per wave (ii == wc),
                // taken from the A fragments when they are first used (PH 1: half 0, PH 3: half 1); the VALU adds sit
                // between the MFMAs so they issue in the matrix pipe's shadow
                if (NEWA && do_cs && ii == wc) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) cs[MI] += (float)af[e];
                }
            }
    }
};

// FP8 (OCP e4m3) TN: weight gradients dW[m, n] = sum_k A8[k, m] B8[k, n] with both operands token-major bytes
// quantised with ONE scale per tensor (the reduction runs over the tokens, so a per-token scale cannot be pulled out of it).
//   K tile = 128 tokens; half-tile image = [128 k][128 columns] bytes (16 KiB, 128-B rows): the ring, the DMA piece count and the
//   phase schedule are byte-for-byte those of the bf16 TN kernel above, with twice the k per tile.
//   Fragments: the MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) wants, in lane (g = lane >> 4, r = lane & 15), the 32 consecutive k
//   [32 g, 32 g + 32) of output row r, one per byte.  ds_read_b64_tr_b8 (layout probed with tools/micro/tr_b8_layout.hip: lane
//   2 q + p of a 16-lane group supplies the address of (row q, byte columns 8 p .. 8 p + 7); lane i receives column i of rows
//   0 .. 7) delivers 8 of them: four reads per fragment at k offsets 0, 8, 16, 24 (+1024 B each in the image).
//   Swizzle: 16-byte chunk ^= ((k >> 1) & 3) | ((k >> 5) & 1) << 2 -- the four same-parity rows of an 8-row block and the two
//   row blocks a 32-lane half reads land on eight different 16-byte bank windows; the per-lane swizzle term does not depend on
//   which of the four reads it is, so they are immediate offsets off one address.
//   C = a_scale_inv * b_scale_inv * sum (fp32 slabs as above); the fused bias gradient sums the e4m3 A fragments (x a_scale_inv).
struct FragT8 {
    union {
        i32x8 v;                // the MFMA operand: 8 consecutive registers
        u32x2 q[4];             // k blocks 0..7, 8..15, 16..23, 24..31 of this lane's group (one transposed read each)
    };
};
template <int OFF>
SC_DEVICE u32x2 tr8_asm(unsigned lds_addr) {
    u32x2 r;
    asm volatile("ds_read_b64_tr_b8 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF) : "memory");
    return r;
}
struct OpsTN8 : OpsTN {         // e4m3 TN
    typedef FragT8 Frag;
    static constexpr int NA = 4, NB = 2;
    // Q = half-tile index inside one ring parity: its byte offset (<= 48 KiB) rides in the instruction's 16-bit offset field, so a
    // fragment needs ONE address register per ring parity instead of one per ring slot (with the slot folded into the address the
    // compiler keeps ~24 hoisted address registers and spills); the ring parity base is part of the (hoisted) address
    template <int Q>
    static SC_DEVICE void read(unsigned addr, FragT8& f) {
        f.q[0] = tr8_asm<Q * HALF>(addr);
        f.q[1] = tr8_asm<Q * HALF + 1024>(addr);
        f.q[2] = tr8_asm<Q * HALF + 2048>(addr);
        f.q[3] = tr8_asm<Q * HALF + 3072>(addr);
    }
    template <int Q>
    static SC_DEVICE void read_a(unsigned par, const unsigned (&a_off)[4], FragT8 (&a)[4]) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) read<Q>(par + a_off[ii], a[ii]);
    }
    template <int Q>
    static SC_DEVICE void read_b(unsigned par, const unsigned (&b_off)[2], FragT8 (&b)[2]) {
        read<Q>(par + b_off[0], b[0]);
        read<Q>(par + b_off[1], b[1]);
    }
    // retire every register the asm reads above wrote (see OpsTN16::wait_b)
    static SC_DEVICE void wait_b(FragT8 (&f)[2]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0].v), "+v"(f[1].v)::"memory"); }
    static SC_DEVICE void wait_a(FragT8 (&f)[4]) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0].v), "+v"(f[1].v), "+v"(f[2].v), "+v"(f[3].v)::"memory");
    }
    static SC_DEVICE float sum(const FragT8& f) {       // sum of this lane's 32 e4m3 values
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int v = (int)f.q[j][w];
                s += __builtin_amdgcn_cvt_f32_fp8(v, 0) + __builtin_amdgcn_cvt_f32_fp8(v, 1) + __builtin_amdgcn_cvt_f32_fp8(v, 2) +
                     __builtin_amdgcn_cvt_f32_fp8(v, 3);
            }
        return s;
    }
    template <int MI, int NJ, bool NEWA>
    static SC_DEVICE void mfma(const FragT8 (&a)[4], const FragT8 (&b)[2], f32x4 (&acc)[8][4], bool do_cs, int wc, float* cs) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const i32x8 af = a[ii].v;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) acc[MI * 4 + ii][NJ * 2 + jj] = mfma_f8(b[jj].v, af, acc[MI * 4 + ii][NJ * 2 + jj]);
            if (NEWA && do_cs && ii == wc) cs[MI] += sum(a[ii]);      // fused bias gradient, as in the bf16 kernel
        }
    }
};

// =====================================================================================================================
// Schedules: phase / ktile (standard 8-slot ring, every operand policy), hphase (half tile: three images, nine slots) and
// pphase (persistent: staging cursor across tiles, post-epilogue waits) share the load section, the MFMA section and the
// fenced barrier below.
// What is shared is straight-line code over register arrays, which inlines to the text it replaced.  The tile frame around
// the K loop -- per-lane sources and offsets, accumulator zeroing, prologue, ring loop, re-align, epilogue choice -- stays
// written out in each kernel on purpose: the compiler simplifies a helper on its own before it inlines it, without what the
// kernel knows (lane < 64, m0 a multiple of 256, ...), and every attempt to share one of those pieces (also the wait and
// barrier tail of the prologue alone) changed the instruction stream of the kernels it touched (profiles/gemm8p_fold_isa.txt).
//
// The LDS offsets a wave reads its fragments at (inside a half-tile image), and its fragment registers:
template <class Ops>
struct FragOffs {
    typename Ops::Off a[Ops::NOA], b[Ops::NOB];
};
template <class Ops>
struct Frags {
    typename Ops::Frag a[Ops::NA], b0[Ops::NB], b1[Ops::NB];
};

// Load section of phase PH (1..4  <->  quadrant (0,0) (0,1) (1,1) (1,0)): the fragments of this quadrant that are not in
// registers yet, from the K tile whose images start at `par`.
template <class Ops, int PH>
SC_DEVICE void load_section(typename Ops::Ring par, const FragOffs<Ops>& O, Frags<Ops>& F) {
    if (PH == 1) Ops::template read_b<1>(par, O.b, F.b0);
    if (PH == 2) Ops::template read_b<2>(par, O.b, F.b1);
    if (PH == 1) Ops::template read_a<0>(par, O.a, F.a);
    if (PH == 3) Ops::template read_a<3>(par, O.a, F.a);
}

// MFMA section of quadrant (MI, NJ), and the barrier that ends the phase
template <class Ops, int MI, int NJ, bool NEWA, int NI, class... Hook>
SC_DEVICE void mfma_section(Frags<Ops>& F, f32x4 (&acc)[NI][4], Hook... hook) {
    __builtin_amdgcn_s_setprio(1);
    Ops::template mfma<MI, NJ, NEWA>(F.a, NJ ? F.b1 : F.b0, acc, hook...);
    __builtin_amdgcn_s_setprio(0);
    fenced_barrier();
}

// One phase of K tile `t` (ring parity D) on the standard 8-slot schedule.
template <class Ops, int D, int PH, class... Hook>
SC_DEVICE void phase(char* smem, const typename Ops::Src& S, int t, const FragOffs<Ops>& O, Frags<Ops>& F, f32x4 (&acc)[8][4], Hook... hook) {
    load_section<Ops, PH>(Ops::ring(smem) + D * 4 * HALF, O, F);
    // ---- stage the half-tile six positions ahead (consumption order A0 B0 B1 A1) ----
    constexpr int q = (PH + 1) & 3;
    constexpr int DS = PH <= 2 ? (D ^ 1) : D;
    const int ts = t + (PH <= 2 ? 1 : 2);
    if (ts < S.nt) {
        Ops::stage(S, q, ts, smem + slot(DS, q));
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");      // retires the half-tile read in the NEXT phase
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // ring is draining: fewer than four in flight
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    // every fragment register this phase's asm reads wrote is tied to the wait that retires it
    if (PH == 1) { Ops::wait_b(F.b0); Ops::wait_a(F.a); }
    if (PH == 2) Ops::wait_b(F.b1);
    if (PH == 3) Ops::wait_a(F.a);
    __builtin_amdgcn_sched_barrier(0);
    mfma_section<Ops, (PH >= 3), (PH == 2 || PH == 3), (PH == 1 || PH == 3)>(F, acc, hook...);
}

template <class Ops, int D, class... Hook>
SC_DEVICE void ktile(char* smem, const typename Ops::Src& S, int t, const FragOffs<Ops>& O, Frags<Ops>& F, f32x4 (&acc)[8][4], Hook... hook) {
    phase<Ops, D, 1>(smem, S, t, O, F, acc, hook...);
    phase<Ops, D, 2>(smem, S, t, O, F, acc, hook...);
    phase<Ops, D, 3>(smem, S, t, O, F, acc, hook...);
    phase<Ops, D, 4>(smem, S, t, O, F, acc, hook...);
}

// (z, tm, tn) of tile index idx = (z * ntm + tm) * ntn + tn
SC_DEVICE void tile_decode(int idx, const GemmArgs& g, int& z, int& tm, int& tn) {
    tn = idx % g.ntn;
    idx /= g.ntn;
    tm = idx % g.ntm;
    z = idx / g.ntm;
}

// ---------------------------------------------------------------------------------------------------------------------
// Half tile (128 rows x 256 columns): the workgroups of a launch's partial last round (GemmArgs::tail_first).
// Half h of tile (tm, tn) is rows tm 256 + 128 h + [0, 128).  Same 2 x 4 wave layout; wave (wr, wc) owns 64 x 64 -- what the full
// tile calls quadrants (0,0) and (0,1): acc[0..3][*] over the images A0', B0, B1, where A0' holds the half tile's 128 rows
// (M-wave wr: rows [64 wr, 64 wr + 64)) and B0 / B1 are the full tile's.  A K tile is two phases (the full tile's phases 1
// and 2, same fragment reads, same 16 MFMAs in the same order, so every output element sees the same sums) over THREE images.
//
// Schedule, in the terms of the RAW / WAR rules of the file header.  Number the phases 2 t (PH 1) and 2 t + 1 (PH 2) of K tile t.
//   reads:  A0'(t), B0(t) in phase 2 t;  B1(t) in phase 2 t + 1.
//   ring:   R K tiles x 3 images; image x(t + R) takes the slot of x(t).
//   WAR:    x(t + R) may be issued two phases after x(t) was read:  A0' / B0 (t + R) from phase 2 t + 2, B1(t + R) from 2 t + 3.
//           So the issue-to-read distance is 2 R - 2 phases whatever the order: R = 3 (nine slots, 144 KiB -- R = 4 does not
//           fit in 160 KiB) gives four phases = two K tiles, against the full tile's six phases with its 8-slot ring.
//   issue:  PH 1 of K tile t stages A0'(t + 2) and B0(t + 2) (two DMA pairs), PH 2 stages B1(t + 2) (one pair): each exactly
//           two phases after the read of the slot's previous image, the earliest the WAR rule allows.
//   RAW:    per-lane issue order is ... B1(t) | A0' B0 (t+1) | B1(t+1) | A0' B0 (t+2) | B1(t+2) ...
//           PH 1 (t) must retire B1(t), read in the next phase: 5 younger images = vmcnt(10);
//           PH 2 (t) must retire A0' B0 (t+1): 4 younger images (B1(t+1), A0' B0 (t+2), B1(t+2)) = vmcnt(8).
//           A phase that stages nothing (t + 2 >= nt: the ring drains) waits for vmcnt(0), as in the full tile.
//   prologue: K tiles 0 and 1 whole (six images); A0' B0 (0) have landed at vmcnt(8) (vmcnt(0) when nt == 1), and PH 1 (0)
//           then finds exactly the steady-state queue.
// The two wave groups stay staggered by one barrier; a half tile passes 4 nt + 2 (+ 1 for the trailing group) barriers.
constexpr int HRING = 9 * HALF;                     // 144 KiB
constexpr int hslot(int D, int q) { return (D * 3 + q) * HALF; }      // q: 0 A0', 1 B0, 2 B1 of the K tile with t % 3 == D

template <int D, int PH>
SC_DEVICE void hphase(char* smem, const Stager& S, int t, const FragOffs<OpsNT16>& O, Frags<OpsNT16>& F, f32x4 (&acc)[4][4]) {
    load_section<OpsNT16, PH>(smem + hslot(D, 0), O, F);
    constexpr int DS = (D + 2) % 3;
    const int ts = t + 2;
    if (ts < S.nt) {
        if (PH == 1) {
            OpsNT16::stage(S, 0, ts, smem + hslot(DS, 0));
            OpsNT16::stage(S, 1, ts, smem + hslot(DS, 1));
            asm volatile("s_waitcnt vmcnt(10)" ::: "memory");     // retires B1(t), read in the NEXT phase
        } else {
            OpsNT16::stage(S, 2, ts, smem + hslot(DS, 2));
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");      // retires A0', B0 of K tile t + 1
        }
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    fenced_barrier();
    mfma_section<OpsNT16, 0, PH - 1, false>(F, acc);
}

// rows [mh, mh + 128) x columns [n0, n0 + 256) of the product (splitk == 1); the caller has checked mh < g.M
template <int EPI>
SC_DEVICE void half_tile(const GemmArgs& g, char* smem, int mh, int n0) {
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;

    Stager S;
    S.nt = g.K / BK;
    S.wave = wave;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (p * 8 + wave) * 8 + (lane >> 3);          // row of the half-tile image, 128 B per row
        const int lc = (lane & 7) ^ ((r >> 1) & 7);              // logical 16-byte chunk stored at physical lane&7
        const int ga = min(mh + r, g.M - 1);
        S.src[0][p] = g.A + (size_t)ga * g.lda + lc * 8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int gb = min(n0 + (r >> 5) * 64 + h * 32 + (r & 31), g.N - 1);
            S.src[1 + h][p] = g.B + (size_t)gb * g.ldb + lc * 8;
        }
    }
    FragOffs<OpsNT16> O;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int coff = ((kk * 4 + lg) ^ ((li >> 1) & 7)) << 4;
        O.a[kk] = (wr * 64 + li) * 128 + coff;
        O.b[kk] = (wc * 32 + li) * 128 + coff;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue: K tiles 0 and 1 (six images)
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int ts = s / 3, q = s % 3;
        if (ts < S.nt) OpsNT16::stage(S, q, ts, smem + hslot(ts, q));
    }
    if (S.nt > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsNT16> F;
    for (int kt = 0; kt < S.nt; kt += 3) {
        hphase<0, 1>(smem, S, kt, O, F, acc);
        hphase<0, 2>(smem, S, kt, O, F, acc);
        if (kt + 1 < S.nt) { hphase<1, 1>(smem, S, kt + 1, O, F, acc); hphase<1, 2>(smem, S, kt + 1, O, F, acc); }
        if (kt + 2 < S.nt) { hphase<2, 1>(smem, S, kt + 2, O, F, acc); hphase<2, 2>(smem, S, kt + 2, O, F, acc); }
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                   // re-align the two wave groups
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // the full tile's epilogues on a 64-row wave tile: two strip passes / one fp32 staging block
    const int row0 = mh + wr * 64, col0 = n0 + wc * 64;
    if (EPI == SC_EPI_GELU_GRAD_PAIR && g.gelu_lut != nullptr) {
        // the table moves into the dead operand ring (behind the eight 4-KiB strips) while the first strip pass is packed
        unsigned* lut = reinterpret_cast<unsigned*>(smem + 8 * 4096);
        for (int c = t; c < SC_GELU_LUT_N / 4; c += 512)
            reinterpret_cast<u32x4*>(lut)[c] = reinterpret_cast<const u32x4*>(g.gelu_lut)[c];
        __syncthreads();
        epilogue_bf16_lds<EPI, false, true>(acc, g, smem + wave * 4096, row0, col0, lane, lut);
    } else if (EPI == SC_EPI_BF16 || EPI == SC_EPI_BF16_BIAS || sc_epi_gelu_fwd(EPI)) {
        epilogue_bf16_lds<EPI>(acc, g, smem + wave * 4096, row0, col0, lane);
    } else {
        float* ep = reinterpret_cast<float*>(smem) + wave * 64 * SC_EPI_LD;
        EpiRegs<EPI> er;
        sc_epi_load<EPI>(er, row0, col0, lane, g, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sc_epi_put(ep, i, j, li, lg, acc[i][j]);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        sc_epilogue_store<EPI>(ep, er, row0, col0, lane, g, 0, -1, 64);
    }
}

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm8p_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Tail split (plan_nt8p, sc_gemm_dispatch.hip): workgroups [0, tail_first) compute the first tail_first tiles of the walk as full tiles, XCD
    // remap over those alone; the last 2 tail_rem workgroups compute the remaining tail_rem tiles as half tiles.  Their own
    // XCD remap gives an XCD a contiguous run of (tile, half) pairs, so the two halves of a tile share their B panel in one L2.
    int idx, hh = -1;
    if (g.tail_first > 0) {
        const int b = (int)blockIdx.x - g.tail_first;
        if (b >= 0) {
            const int r = sc_xcd_remap(b, 2 * g.tail_rem);
            idx = g.tail_first + (r >> 1);
            hh = r & 1;
        } else {
            idx = sc_xcd_remap(blockIdx.x, g.tail_first);
        }
    } else {
        idx = sc_xcd_remap(blockIdx.x, gridDim.x);
    }
    int tn, tm, z;
    if (g.col_group > 0) {                                       // column-group walk (splitk == 1): sc_gemm_common.h
        sc_tile_colgroup(idx, g, tm, tn);
        z = 0;
    } else {
        tile_decode(idx, g, z, tm, tn);
    }
    if (hh >= 0) {                                               // workgroup-uniform: every wave takes the same path
        const int mh = tm * BM + hh * 128;
        if (mh < g.M) half_tile<EPI>(g, smem, mh, tn * BN);      // second half of a ragged last tile row: nothing to do
        return;
    }
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;

    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = z * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    Stager S;
    S.nt = (kend - kbeg) / BK;
    S.wave = wave;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (p * 8 + wave) * 8 + (lane >> 3);          // row of the half-tile image, 128 B per row
        const int lc = (lane & 7) ^ ((r >> 1) & 7);              // logical 16-byte chunk stored at physical lane&7
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ga = min(m0 + (r >> 6) * 128 + h * 64 + (r & 63), g.M - 1);
            const int gb = min(n0 + (r >> 5) * 64 + h * 32 + (r & 31), g.N - 1);
            S.src[h ? 3 : 0][p] = g.A + (size_t)ga * g.lda + kbeg + lc * 8;
            S.src[h ? 2 : 1][p] = g.B + (size_t)gb * g.ldb + kbeg + lc * 8;
        }
    }
    FragOffs<OpsNT16> O;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int coff = ((kk * 4 + lg) ^ ((li >> 1) & 7)) << 4;
        O.a[kk] = (wr * 64 + li) * 128 + coff;
        O.b[kk] = (wc * 32 + li) * 128 + coff;
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue: the first six half-tiles (all of K tile 0, A0 and B0 of K tile 1)
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int ts = s >> 2, q = s & 3;
        if (ts < S.nt) OpsNT16::stage(S, q, ts, smem + slot(ts & 1, q));
    }
    if (S.nt > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsNT16> F;
    for (int kt = 0; kt < S.nt; kt += 2) {
        ktile<OpsNT16, 0>(smem, S, kt, O, F, acc);
        if (kt + 1 < S.nt) ktile<OpsNT16, 1>(smem, S, kt + 1, O, F, acc);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                   // re-align the two wave groups
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);

    // Epilogue: bf16 outputs without an extra input tile go through the bf16 LDS strip (full-line stores, half the LDS
    // bytes); the fp32-residual, GELU' and fp32 epilogues keep the fp32 staging shared with sc_gemm256.hip.
    if (EPI == SC_EPI_GELU_GRAD_PAIR && g.gelu_lut != nullptr) {
        // the table moves into the dead operand ring (behind the eight 4-KiB strips) while the first strip pass is packed
        unsigned* lut = reinterpret_cast<unsigned*>(smem + 8 * 4096);
        for (int c = t; c < SC_GELU_LUT_N / 4; c += 512)
            reinterpret_cast<u32x4*>(lut)[c] = reinterpret_cast<const u32x4*>(g.gelu_lut)[c];
        __syncthreads();
        epilogue_bf16_lds<EPI, false, true>(acc, g, smem + wave * 4096, m0 + wr * 128, n0 + wc * 64, lane, lut);
    } else if (EPI == SC_EPI_BF16 || EPI == SC_EPI_BF16_BIAS || sc_epi_gelu_fwd(EPI)) {
        epilogue_bf16_lds<EPI>(acc, g, smem + wave * 4096, m0 + wr * 128, n0 + wc * 64, lane);
    } else {
        const int mw = wr * 128;
        float* ep = reinterpret_cast<float*>(smem) + wave * 64 * SC_EPI_LD;
        EpiRegs<EPI> er;
        sc_epi_load<EPI>(er, m0 + mw, n0 + wc * 64, lane, g, 64);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sc_epi_put(ep, i, j, li, lg, acc[h * 4 + i][j]);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            sc_epilogue_store<EPI>(ep, er, m0 + mw + h * 64, n0 + wc * 64, lane, g, z, (h + 1 < 2) ? m0 + mw + 64 : -1, 64);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

__global__ void sc_gelu_lut_fill_kernel(unsigned* lut, int act) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= SC_GELU_LUT_N) return;
    const unsigned bits = (unsigned)(SC_GELU_LUT_LO + i % SC_GELU_LUT_HALF) | (i >= SC_GELU_LUT_HALF ? 0x8000u : 0u);
    const float u = __uint_as_float(bits << 16);
    float hv, gv;
    sc_act_both(u, act, hv, gv);
    union { bf16 b; unsigned short s; } h, gq;
    h.b = (bf16)hv;
    gq.b = (bf16)gv;
    lut[i] = ((unsigned)gq.s << 16) | (unsigned)h.s;
}

// =====================================================================================================================
// Persistent NT variant: one workgroup per CU walks a list of output tiles (tile = first + r * gridDim).  The staging
// stream never stops at a tile boundary -- the first six half-tiles of the next tile are issued during the last K
// tiles of the current one -- so a new tile starts without the DMA round trip, without a workgroup launch and without
// waiting for the previous tile's stores to drain.  At a boundary the two wave groups re-align (one extra barrier
// for waves 0-3), every wave writes its 128x64 result through its 4-KiB LDS strip behind the ring (epilogue_bf16_lds), and the
// stagger is restored (one extra barrier for waves 4-7).  The epilogue's stores enter the vmcnt stream between two half-tile DMAs: the
// three phases that follow allow for them in their counted waits (kind POSTEPI, interior tiles: every store is
// issued); tiles that touch the M / N edge, where a fully masked store may be skipped, drain to zero instead.
enum { PW_STEADY = 0, PW_POSTEPI = 1, PW_DRAIN0 = 2 };      // counted-wait flavour of the K tile that follows an epilogue

struct PStager {
    const bf16* src[4][2];
    long long koff;             // element offset of the K tile being staged
    int sk;                     // K tile (within the staging tile) being staged
    int stile;                  // staging tile index, >= total when the list is exhausted
    int nt, wave, total, stride;
};

SC_DEVICE void pstage_set_tile(PStager& S, const GemmArgs& g, int lane) {
    const int tn = S.stile % g.ntn, tm = S.stile / g.ntn;
    const int m0 = tm * BM, n0 = tn * BN;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (p * 8 + S.wave) * 8 + (lane >> 3);
        const int lc = (lane & 7) ^ ((r >> 1) & 7);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ga = min(m0 + (r >> 6) * 128 + h * 64 + (r & 63), g.M - 1);
            const int gb = min(n0 + (r >> 5) * 64 + h * 32 + (r & 31), g.N - 1);
            S.src[h ? 3 : 0][p] = g.A + (size_t)ga * g.lda + lc * 8;
            S.src[h ? 2 : 1][p] = g.B + (size_t)gb * g.ldb + lc * 8;
        }
    }
}
// move the staging cursor to the next K tile (possibly the first one of the next tile of this workgroup's list)
SC_DEVICE void pstage_advance(PStager& S, const GemmArgs& g, int lane) {
    S.sk += 1;
    S.koff += BK;
    if (S.sk == S.nt) {
        S.sk = 0;
        S.koff = 0;
        S.stile += S.stride;
        if (S.stile < S.total) pstage_set_tile(S, g, lane);
    }
}

// One phase; `doff` = byte offset of the ring half (parity) that holds the K tile being computed.
template <int PH, int ESTORES>
SC_DEVICE void pphase(char* smem, int doff, PStager& S, const GemmArgs& g, int lane, int pw, const FragOffs<OpsNT16>& O,
                      Frags<OpsNT16>& F, f32x4 (&acc)[8][4]) {
    load_section<OpsNT16, PH>(smem + doff, O, F);
    // staging: the K tile under the cursor is (compute K tile + 1) in phases 1-2 and (+ 2) in phases 3-4
    constexpr int q = (PH + 1) & 3;
    char* dst = smem + (PH <= 2 ? (doff ^ (4 * HALF)) : doff) + q * HALF;
    if (PH == 3) pstage_advance(S, g, lane);
    if (S.stile < S.total) {
        OpsNT16::stage_pair(S.src[q][0], S.src[q][1], S.koff, dst, S.wave);
        if (PH <= 3 && pw == PW_POSTEPI) {
            constexpr int N = 8 + ESTORES > 63 ? 63 : 8 + ESTORES;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
        } else if (PH == 1 && pw == PW_DRAIN0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        }
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    fenced_barrier();
    mfma_section<OpsNT16, (PH >= 3), (PH == 2 || PH == 3), false>(F, acc);
}

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm8pp_kernel(const GemmArgs g, int total_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;
    // stores one wave issues per interior tile (every lane in bounds): 4 passes x 4 full-line stores, two tensors -> 32
    constexpr int ESTORES = sc_epi_gelu_fwd(EPI) ? 32 : 16;

    PStager S;
    S.nt = g.K / BK;
    S.wave = wave;
    S.total = total_tiles;
    S.stride = gridDim.x;
    S.stile = sc_xcd_remap(blockIdx.x, gridDim.x);
    S.sk = 0;
    S.koff = 0;
    pstage_set_tile(S, g, lane);
    int ctile = S.stile;                                         // tile being computed

    FragOffs<OpsNT16> O;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int coff = ((kk * 4 + lg) ^ ((li >> 1) & 7)) << 4;
        O.a[kk] = (wr * 64 + li) * 128 + coff;
        O.b[kk] = (wc * 32 + li) * 128 + coff;
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue: K tile 0 (four half-tiles) and A0, B0 of K tile 1.  The launcher guarantees nt >= 3, so every image exists:
    // the constant stands for that, and the cursor moves to K tile 1 in front of its first image
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int q = s & 3;
        if (s == 4) pstage_advance(S, g, lane);
        OpsNT16::stage_pair(S.src[q][0], S.src[q][1], S.koff, smem + slot(s >> 2, q), wave);
    }
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsNT16> F;
    int k = 0;                                                   // K tile inside the tile being computed
    int pw = PW_STEADY;
    int doff = 0;                                                // ring half of the K tile being computed
    while (ctile < total_tiles) {
        pphase<1, ESTORES>(smem, doff, S, g, lane, pw, O, F, acc);
        pphase<2, ESTORES>(smem, doff, S, g, lane, pw, O, F, acc);
        pphase<3, ESTORES>(smem, doff, S, g, lane, pw, O, F, acc);
        pphase<4, ESTORES>(smem, doff, S, g, lane, pw, O, F, acc);
        doff ^= 4 * HALF;
        pw = PW_STEADY;
        if (++k == S.nt) {
            k = 0;
            const int tn = ctile % g.ntn, tm = ctile / g.ntn;
            const int m0 = tm * BM, n0 = tn * BN;
            if (wr == 0) __builtin_amdgcn_s_barrier();           // waves 0-3 wait for 4-7: groups aligned
            __builtin_amdgcn_sched_barrier(0);
            epilogue_bf16_lds<EPI>(acc, g, smem + RING + wave * 4096, m0 + wr * 128, n0 + wc * 64, lane);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_sched_barrier(0);
            pw = ((m0 + BM <= g.M) && (n0 + BN <= g.N)) ? PW_POSTEPI : PW_DRAIN0;
            ctile += gridDim.x;
            if (ctile < total_tiles && wr == 1) __builtin_amdgcn_s_barrier();   // restore the stagger
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// =====================================================================================================================
// TN kernels (weight gradients; layouts: OpsTN16 / OpsTN8 above).
// one 256x256 output tile (or split-K slab tile) of the TN product described by g; idx = (z * ntm + tm) * ntn + tn
SC_DEVICE void tn_tile(const GemmArgs& g, int idx, char* smem) {
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;

    int z, tm, tn;
    tile_decode(idx, g, z, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = z * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    StagerTN S;
    S.nt = (kend - kbeg) / BK;
    S.wave = wave;
    S.step[0] = S.step[3] = (long long)BK * g.lda * 2;
    S.step[1] = S.step[2] = (long long)BK * g.ldb * 2;
    {
        // piece p = k rows [32 p + 4 wave, + 4): rows kr and kr + 32 share the swizzle term (bits 0, 1, 3 of k)
        const int kr = wave * 4 + (lane >> 4);                          // k row of the half-tile image, 256 B per row
        const int s = (kr & 3) | (((kr >> 3) & 1) << 2);
        const int c = ((((lane & 15) >> 1) ^ s) << 4) + (lane & 1) * 8;  // logical column held at physical lane&15
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ca = min(m0 + h * 128 + c, g.M - 8), cb = min(n0 + h * 128 + c, g.N - 8);
            S.off[h ? 3 : 0] = ((unsigned)kr * (unsigned)g.lda + (unsigned)ca) * 2u;
            S.off[h ? 2 : 1] = ((unsigned)kr * (unsigned)g.ldb + (unsigned)cb) * 2u;
        }
    }
    S.base[0] = S.base[3] = reinterpret_cast<const char*>(g.A + (size_t)kbeg * g.lda);
    S.base[1] = S.base[2] = reinterpret_cast<const char*>(g.B + (size_t)kbeg * g.ldb);

    FragOffs<OpsTN16> O;
    {
        const int q = li >> 2, p = li & 3;
        const int s = q | ((lg & 1) << 2);
        const int row = (lg * 8 + q) * 256 + p * 8;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) O.a[ii] = row + (((wr * 4 + ii) ^ s) << 5);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) O.b[jj] = row + (((wc * 2 + jj) ^ s) << 5);
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool do_cs = g.colsum != nullptr && tn == 0;
    float cs[2] = {0.f, 0.f};

    // prologue: the first six half-tiles (all of K tile 0, A0 and B0 of K tile 1)
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int ts = s >> 2, q = s & 3;
        if (ts < S.nt) OpsTN16::stage<false>(S, q, ts, smem + slot(ts & 1, q));
    }
    if (S.nt > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsTN16> F;
    for (int kt = 0; kt < S.nt; kt += 2) {
        ktile<OpsTN16, 0>(smem, S, kt, O, F, acc, do_cs, wc, cs);
        if (kt + 1 < S.nt) ktile<OpsTN16, 1>(smem, S, kt + 1, O, F, acc, do_cs, wc, cs);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                   // re-align the two wave groups
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (do_cs) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v = cs[h];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int m = m0 + h * 128 + wr * 64 + wc * 16 + li;
            if (lg == 0 && m < g.M) g.colsum[(size_t)z * g.M + m] = v;
        }
    }
    float* ep = reinterpret_cast<float*>(smem) + wave * 64 * SC_EPI_LD;
    EpiRegs<SC_EPI_F32> er;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sc_epi_put(ep, i, j, li, lg, acc[h * 4 + i][j]);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        sc_epilogue_store<SC_EPI_F32>(ep, er, m0 + h * 128 + wr * 64, n0 + wc * 32, lane, g, z, -1, 64, 128 - 32);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(512, 2) void gemm8p_tn_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tn_tile(g, sc_xcd_remap(blockIdx.x, gridDim.x), smem);
}

// Several weight gradients that share the reduction length (one Linear's token axis) in ONE launch: problem p owns the
// remapped block ids [first[p], first[p + 1]).  Why (round 4): the four weight gradients of a transformer block were four
// launches of about one round of workgroups each; out_proj (9 output tiles) needed split-K 28 to fill the chip -- 66 MB of
// fp32 slabs for a 2.4 MB result and 28-K-tile workgroups that are mostly prologue and epilogue (820 TFLOP/s against
// 1 100-1 190 for its siblings).  Grouped, every problem runs at the group's split-K.
struct GemmGroup {
    GemmArgs g[SC_WGRAD_GROUP_MAX];
    int first[SC_WGRAD_GROUP_MAX + 1];
    int n;
};
__global__ __launch_bounds__(512, 2) void gemm8p_tn_group_kernel(const GemmGroup gg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int idx = sc_xcd_remap(blockIdx.x, gridDim.x);
    int p = 0;
    while (p + 1 < gg.n && idx >= gg.first[p + 1]) ++p;
    tn_tile(gg.g[p], idx - gg.first[p], smem);
}

// g.A / g.B: e4m3 bytes [K tokens][M] / [K][N], lda / ldb in BYTES; g.K tokens (k_per_split a multiple of 128);
// g.a_scale / g.b_scale: ONE dequantisation factor each (device scalars)
__global__ __launch_bounds__(512, 2) void gemm8p_tn_f8_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BK8 = 128;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;

    int z, tm, tn;
    tile_decode(sc_xcd_remap(blockIdx.x, gridDim.x), g, z, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = z * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const char* A8 = reinterpret_cast<const char*>(g.A);
    const char* B8 = reinterpret_cast<const char*>(g.B);

    StagerTN S;
    S.nt = (kend - kbeg) / BK8;
    S.wave = wave;
    S.step[0] = S.step[3] = (long long)BK8 * g.lda;
    S.step[1] = S.step[2] = (long long)BK8 * g.ldb;
    {
        // piece p of a half-tile = k rows [8 (8 p + wave), + 8): rows kr and kr + 64 have the same swizzle term (bits 1, 2, 5 of k)
        const int kr = wave * 8 + (lane >> 3);                           // k row of the half-tile image, 128 B per row
        const int sw = ((kr >> 1) & 3) | (((kr >> 5) & 1) << 2);
        const int c = ((lane & 7) ^ sw) << 4;                            // logical byte column held at physical chunk lane & 7
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ca = min(m0 + h * 128 + c, g.M - 16), cb = min(n0 + h * 128 + c, g.N - 16);
            S.off[h ? 3 : 0] = (unsigned)kr * (unsigned)g.lda + (unsigned)ca;
            S.off[h ? 2 : 1] = (unsigned)kr * (unsigned)g.ldb + (unsigned)cb;
        }
    }
    S.base[0] = S.base[3] = A8 + (size_t)kbeg * g.lda;
    S.base[1] = S.base[2] = B8 + (size_t)kbeg * g.ldb;

    FragOffs<OpsTN8> O;
    {
        const int sw = ((li >> 2) & 3) | ((lg & 1) << 2);                // swizzle term of rows 32 lg + 8 j + (li >> 1), any j
        const int row = (32 * lg + (li >> 1)) * 128 + (li & 1) * 8;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) O.a[ii] = row + (((wr * 4 + ii) ^ sw) << 4);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) O.b[jj] = row + (((wc * 2 + jj) ^ sw) << 4);
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool do_cs = g.colsum != nullptr && tn == 0;
    float cs[2] = {0.f, 0.f};

    // prologue: the first six half-tiles (all of K tile 0, A0 and B0 of K tile 1)
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int ts = s >> 2, q = s & 3;
        if (ts < S.nt) OpsTN8::stage<false>(S, q, ts, smem + slot(ts & 1, q));
    }
    if (S.nt > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsTN8> F;
    for (int kt = 0; kt < S.nt; kt += 2) {
        ktile<OpsTN8, 0>(smem, S, kt, O, F, acc, do_cs, wc, cs);
        if (kt + 1 < S.nt) ktile<OpsTN8, 1>(smem, S, kt + 1, O, F, acc, do_cs, wc, cs);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                   // re-align the two wave groups
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const float sa = g.a_scale ? *g.a_scale : 1.0f, sb = g.b_scale ? *g.b_scale : 1.0f;
    if (do_cs) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v = cs[h];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int m = m0 + h * 128 + wr * 64 + wc * 16 + li;
            if (lg == 0 && m < g.M) g.colsum[(size_t)z * g.M + m] = v * sa;
        }
    }
    const float sab = sa * sb;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] *= sab;
    float* ep = reinterpret_cast<float*>(smem) + wave * 64 * SC_EPI_LD;
    EpiRegs<SC_EPI_F32> er;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sc_epi_put(ep, i, j, li, lg, acc[h * 4 + i][j]);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        sc_epilogue_store<SC_EPI_F32>(ep, er, m0 + h * 128 + wr * 64, n0 + wc * 32, lane, g, z, -1, 64, 128 - 32);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
}

// FP8 NT (OpsNT8 above): g.K / lda / ldb are in 2-byte units; g.a_scale [M] and g.b_scale [N] are the dequantisation factors
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm8p_f8_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 15, lg = lane >> 4;

    int idx = sc_xcd_remap(blockIdx.x, gridDim.x);
    const int tn = idx % g.ntn;
    const int tm = idx / g.ntn;
    const int m0 = tm * BM, n0 = tn * BN;

    Stager S;
    S.nt = g.K / BK;
    S.wave = wave;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (p * 8 + wave) * 8 + (lane >> 3);          // row of the half-tile image, 128 B per row
        const int lc = (lane & 7) ^ ((r >> 1) & 7);              // logical 16-byte chunk stored at physical lane&7
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ga = min(m0 + (r >> 6) * 128 + h * 64 + (r & 63), g.M - 1);
            const int gb = min(n0 + (r >> 5) * 64 + h * 32 + (r & 31), g.N - 1);
            S.src[h ? 3 : 0][p] = g.A + (size_t)ga * g.lda + lc * 8;
            S.src[h ? 2 : 1][p] = g.B + (size_t)gb * g.ldb + lc * 8;
        }
    }
    FragOffs<OpsNT8> O;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        // Which two 16-byte chunks of the 128-byte row lane group lg takes is free -- the MFMA sums over all 128 k, and A and B
        // fragments use the same map -- but not for the LDS: a ds_read_b128 is served in groups of 16 lanes
        // ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS table) that mix rows of lg and lg + 1, and with the staging
        // swizzle chunk ^ ((row >> 1) & 7) the obvious map 2 lg + kk put both halves of such a group on the same bank windows:
        // SQ_LDS_BANK_CONFLICT 29.5 M cycles against the bf16 kernel's 4.2 M on the same bytes (profiles/r06_fp8_ktile_probe.txt).
        // Conflict-free needs c(lg, kk) ^ c(lg ^ 1, kk) in {1, 6, 7}: c = 4 (lg >> 1) + 2 kk + (lg & 1).
        const int coff = (((lg >> 1) * 4 + 2 * kk + (lg & 1)) ^ ((li >> 1) & 7)) << 4;
        O.a[kk] = (wr * 64 + li) * 128 + coff;
        O.b[kk] = (wc * 32 + li) * 128 + coff;
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue: the first six half-tiles (all of K tile 0, A0 and B0 of K tile 1)
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int ts = s >> 2, q = s & 3;
        if (ts < S.nt) OpsNT8::stage(S, q, ts, smem + slot(ts & 1, q));
    }
    if (S.nt > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                   // waves 4-7 run one barrier behind
    __builtin_amdgcn_sched_barrier(0);

    Frags<OpsNT8> F;
    for (int kt = 0; kt < S.nt; kt += 2) {
        ktile<OpsNT8, 0>(smem, S, kt, O, F, acc);
        if (kt + 1 < S.nt) ktile<OpsNT8, 1>(smem, S, kt + 1, O, F, acc);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                   // re-align the two wave groups
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);

    // dequantise: lane owns C[m = .. + 16 i + li][n = .. + 16 j + 4 lg .. + 3]
    {
        const int mrow = m0 + wr * 128 + li, ncol = n0 + wc * 64 + lg * 4;
        f32x4 sb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sb[j] = (f32x4){1.f, 1.f, 1.f, 1.f};
            if (g.b_scale && ncol + j * 16 < g.N) sb[j] = *reinterpret_cast<const f32x4*>(g.b_scale + ncol + j * 16);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float sa = g.a_scale ? g.a_scale[g.a_scale_scalar ? 0 : min(mrow + i * 16, g.M - 1)] : 1.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] *= sb[j] * sa;
        }
    }
    if (EPI == SC_EPI_GELU_GRAD_PAIR && g.gelu_lut != nullptr) {
        // the table moves into the dead operand ring (behind the eight 4-KiB strips) while the first strip pass is packed
        unsigned* lut = reinterpret_cast<unsigned*>(smem + 8 * 4096);
        for (int c = t; c < SC_GELU_LUT_N / 4; c += 512)
            reinterpret_cast<u32x4*>(lut)[c] = reinterpret_cast<const u32x4*>(g.gelu_lut)[c];
        __syncthreads();
        epilogue_bf16_lds<EPI, true, true>(acc, g, smem + wave * 4096, m0 + wr * 128, n0 + wc * 64, lane, lut);
    } else if (EPI == SC_EPI_BF16 || EPI == SC_EPI_BF16_BIAS || sc_epi_gelu_fwd(EPI)) {
        epilogue_bf16_lds<EPI, true>(acc, g, smem + wave * 4096, m0 + wr * 128, n0 + wc * 64, lane);
    } else {
        const int mw = wr * 128;
        float* ep = reinterpret_cast<float*>(smem) + wave * 64 * SC_EPI_LD;
        EpiRegs<EPI> er;
        float amax_lane = 0.f;
        sc_epi_load<EPI>(er, m0 + mw, n0 + wc * 64, lane, g, 64);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sc_epi_put(ep, i, j, li, lg, acc[h * 4 + i][j]);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            sc_epilogue_store<EPI, true>(ep, er, m0 + mw + h * 64, n0 + wc * 64, lane, g, 0, (h + 1 < 2) ? m0 + mw + 64 : -1,
                                         64, 0, &amax_lane);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        }
        if (sc_epi_aux_mul(EPI) && g.q8) sc_amax_publish(amax_lane, g.q8_amax);
    }
}

// Launch of one of this file's 512-thread kernels with `lds` bytes of dynamic LDS; the kernel's limit (lds_max) is raised on its
// first launch, once per kernel: Kernel is a template argument, so every kernel has its own flag.
template <auto Kernel, class... Args>
int launch_lds(int grid, int lds_max, int lds, hipStream_t st, const Args&... args) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        attr_done = true;
    }
    Kernel<<<grid, 512, lds, st>>>(args...);
    SC_LAUNCH_CHECK();
    return 0;
}

static_assert(LDS_BYTES == SC_GEMM256_LDS && HRING == SC_GEMM8P_HALF_LDS && HRING >= LDS_BYTES && RING + 8 * 4096 == SC_GEMM8PP_LDS,
              "the planner's LDS figures; gemm8p_kernel's limit is raised once, to the half tiles' ring");

}  // namespace

int sc_gemm8p_launch(int mode, int epi, const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
    if (mode == SC_GEMM_TN) return launch_lds<&gemm8p_tn_kernel>(p.grid, p.lds_max, p.lds, st, g);
    if (p.path == SC_GEMM_PATH_NT8P_PERSISTENT) {
        if (epi == SC_EPI_BF16) return launch_lds<&gemm8pp_kernel<SC_EPI_BF16>>(p.grid, p.lds_max, p.lds, st, g, p.tiles);
        if (epi == SC_EPI_BF16_BIAS) return launch_lds<&gemm8pp_kernel<SC_EPI_BF16_BIAS>>(p.grid, p.lds_max, p.lds, st, g, p.tiles);
        if (epi == SC_EPI_GELU_PAIR) return launch_lds<&gemm8pp_kernel<SC_EPI_GELU_PAIR>>(p.grid, p.lds_max, p.lds, st, g, p.tiles);
        return launch_lds<&gemm8pp_kernel<SC_EPI_GELU_GRAD_PAIR>>(p.grid, p.lds_max, p.lds, st, g, p.tiles);
    }
    return sc_epi_dispatch(epi, [&](auto E) {
        return launch_lds<&gemm8p_kernel<decltype(E)::value>>(p.grid, p.lds_max, p.lds, st, g);
    });
}

// every g[p] describes dW_p[M_p, N_p] = A_p[K, M_p]^T . B_p[K, N_p] with the SAME K and split-K
int sc_gemm8p_tn_group_launch(const GemmArgs* g, int n, hipStream_t st) {
    GemmGroup gg{};
    gg.n = n;
    int total = 0;
    for (int p = 0; p < n; ++p) {
        gg.g[p] = g[p];
        gg.first[p] = total;
        total += g[p].ntm * g[p].ntn * g[p].splitk;
    }
    for (int p = n; p <= SC_WGRAD_GROUP_MAX; ++p) gg.first[p] = total;
    return launch_lds<&gemm8p_tn_group_kernel>(total, LDS_BYTES, LDS_BYTES, st, gg);
}

int sc_gemm8p_tn_fp8_launch(const GemmArgs& g, hipStream_t st) {
    return launch_lds<&gemm8p_tn_f8_kernel>(g.ntm * g.ntn * g.splitk, LDS_BYTES, LDS_BYTES, st, g);
}

int sc_gemm8p_fp8_launch(int epi, GemmArgs g, hipStream_t st) {
    g.ntm = (g.M + BM - 1) / BM;
    g.ntn = (g.N + BN - 1) / BN;
    g.splitk = 1;
    g.k_per_split = g.K;
    const int rc = (g.M < 1 || g.N < 8 || (g.K % BK) != 0) ? -1 : sc_epi_dispatch(epi, [&](auto E) {
        return launch_lds<&gemm8p_f8_kernel<decltype(E)::value>>(g.ntm * g.ntn, LDS_BYTES, LDS_BYTES, st, g);
    });
    SC_CHECK(rc != -1, "sc_gemm_fp8: shape not supported (M=%d N=%d K=%d epi=%d)", g.M, g.N, 2 * g.K, epi);
    return rc;
}

// device copy of the GELU table, one per device and activation, filled on first use by the formula itself (sc_gemm_common.h)
const unsigned* sc_gelu_lut_device(hipStream_t st, int act) {
    static std::mutex mu;
    static std::map<int, unsigned*> all;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const int key = dev * 2 + (act ? 1 : 0);
    std::lock_guard<std::mutex> lock(mu);
    auto it = all.find(key);
    if (it != all.end()) return it->second;
    unsigned* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), SC_GELU_LUT_N * sizeof(unsigned)) != hipSuccess) p = nullptr;
    if (p) {
        sc_gelu_lut_fill_kernel<<<(SC_GELU_LUT_N + 255) / 256, 256, 0, st>>>(p, act ? 1 : 0);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {     // once per device: later launches may use any stream
            (void)hipFree(p);
            p = nullptr;
        }
    }
    all[key] = p;
    return p;
}
