// Streamed attention: K / V (forward, dq) or Q / dO (dkv) pass through LDS in 64-row tiles, so nothing limits L but the
// instances built.  Two of them: head dim 64, non-causal, any L (ViT-L/14 at 336 px = 577 tokens, at 280 px = 401,
// ViT-B/16 towers above 284 px: the head-in-LDS kernels of sc_attention.hip stop at L = 320), and head dim 80, L <= 320,
// causal or not (ViT-H: width 1280 = 16 heads of 80).  One set of kernel templates over <head dim, CAUSAL>; what the head
// dim changes (LDS image, fragment over the head dim, tuning constants) is struct Head below and the kernels do not know it.
//
// Why streamed and not head-resident at 80: K and V of a 257-token head are 90 KiB at 160-byte rows, so two head-resident
// workgroups do not share a CU (160 KiB) and the fused backward (four images, 182 KiB) fits not at all; 64-row tiles
// through two LDS buffers cost 40 KiB per workgroup and keep two workgroups on a CU.
//
// Forward: one workgroup (4 waves) = 128 query rows of one (batch, head), 32 per wave as two 16-query MFMA column tiles
// whose Q fragments stay in registers.  K and V tiles (one LDS image each, read by rows for S and by ds_read_b64_tr_b16
// for P.V) are double buffered: the global loads of tile j + 1 are in flight while tile j is computed, and one barrier per
// tile separates the LDS write of one buffer from the reads of the other.  Products are transposed as in sc_attention.hip
// (key on the MFMA row, query on the column), so a query's running max and sum live in the lanes of its accumulators and
// P / dS feed the next MFMA from registers: online softmax in fp32, O rescaled only when some row's max moves.  A tile is
// walked in 32-key halves and a half past L is skipped (577 = 9 * 64 + 1 costs one 32-key half, not a 64-key tile).
//
// Backward: two kernels, no float atomics, a fixed summation order everywhere (bit-reproducible):
//   dq kernel : the forward's structure (128 queries per workgroup, K/V streamed): P recomputed from Q, K and lse,
//               dP^T = V.dO^T, dS^T, dQ^T += K^T.dS^T; also writes delta = rowsum(dO * O).  Rows from q_rows on: zeros.
//   dkv kernel: 32 (dh 64) or 16 (dh 80) keys per wave with K and V fragments in registers, Q / dO / lse / delta streamed
//               in 64-query tiles: S = Q.K^T and dP = dO.V^T with the key on the lane, so P and dS are directly the B
//               operands of dV^T += dO^T.P and dK^T += Q^T.dS.
// Workgroups of one head are mapped onto one XCD so that its K / V (forward, dq) or Q / dO (dkv) is fetched into one L2.
// Causal: a workgroup stops (forward, dq) or starts (dkv) its tile loop at the diagonal and a wave skips 32-row halves that
// lie wholly above it; with CAUSAL false every such term folds away.
#include "sc_attn_common.h"

namespace {

constexpr int LT = 64;                  // rows per streamed tile
constexpr int LB = 128;                 // queries per workgroup of the forward and dq kernels: 4 waves x 32
constexpr float LOG2E = 1.4426950408889634f;

// What the head dim decides.  A 16-row fragment over the whole head dim is NK steps of K = 32: lane (g, i) holds row i,
// columns 32 ks + 8g .. + 7 (lds_step from an LDS image, global_step from a row in HBM); where the head dim is an M extent
// (O^T, dQ^T, dK^T, dV^T) it is DH / 16 tiles read by tr().
//   FWD_WAVES: amdgpu_waves_per_eu of the forward (dq and dkv: two everywhere)
//   DKV_KT   : 16-key tiles per wave in the dkv kernel; DKV_KEYS: keys per workgroup of it (4 waves)
//   DQ_K_OUTER: source order of the dq kernel's four products per step (dot4 below)
template <int DH_>
struct Head;

// dh 64: the swizzled image of the head-in-LDS kernels (sc_attn_common.h), two K steps
template <>
struct Head<64> {
    static constexpr int DH = 64, NK = 2, FWD_WAVES = 3, DKV_KT = 2, DKV_KEYS = 4 * 16 * DKV_KT;
    static constexpr bool DQ_K_OUTER = true;
    static constexpr float SCALE = 0.125f;
    static SC_DEVICE int off(int row, int ch) { return Img<64>::off(row, ch); }
    static SC_DEVICE bf16x8 lds_step(const char* img, int row, int ks, int lg) { return frag_row<64>(img, row, ks, 0, lg); }
    static SC_DEVICE bf16x8 global_step(const bf16* row, int ks, int lg) {
        return *reinterpret_cast<const bf16x8*>(row + ks * 32 + lg * 8);
    }
    static SC_DEVICE bf16x8 tr(const char* img, int row0, int c0, int li, int lg) { return frag_tr<64>(img, row0, c0, li, lg); }
};

// dh 80 = 2 x 32 + 16: three K steps, the third on columns 64..79 (lane (g, i): columns 64 + 8 (g & 1) .. + 7) with the
// upper half of its K extent padded IN REGISTERS: the register-side operand of every product (Q, dO in the forward and dq
// kernels, K, V in the dkv kernel; loaded once per wave by global_step) holds zeros in lanes g >= 2, so whatever finite
// values the LDS-side operand repeats there (it re-reads columns 64..79, a broadcast) contribute nothing.  Nothing is
// padded in HBM or LDS.  The K = 16 instruction (v_mfma_f32_16x16x16_bf16) would save half an MFMA per product, but chained
// behind a 16x16x32 through SrcC with a different destination the toolchain emits no wait states between the two and the
// sums came out wrong intermittently on the device; one instruction type keeps the chains on the path every other kernel
// here uses.
//
// LDS image: dense rows of 160 B, no swizzle.  160 B = 40 banks and 40 r mod 64 takes the eight values 0, 8, ..., 56 over
// 16 consecutive rows, so rows r and r + 8 start on the same bank; the lane groups of the kinds of read never put
// two such rows on one 16-byte slot:
//   * ds_read_b128 row fragments (lane (g, i): row i, chunk 4 ks + g) are served in the four 16-lane groups
//     {rows 0-3, 12-15 of chunk c; rows 4-11 of chunk c + 1}: the second set starts 4 banks further and rows r, r + 8 fall
//     in different sets -> 16 slots on 16 different bank quads, conflict free (4 LDS cycles, the minimum);
//   * ds_read_b64_tr_b16 (lane (g, 4q + p): row 4g + q, 32 contiguous bytes per row) is served in 32-lane halves = 8
//     consecutive rows x 32 B, starting 8 banks apart -> 64 different banks, conflict free (2 cycles);
//   * the third row fragment (lane (g, i): row i, chunk 8 + (g & 1)) is a ds_read_b128 like the first two with lanes g and
//     g + 2 on one address (a broadcast): conflict free.
//
// DKV_KT = 1: with 32 keys per wave the K / V fragments, ten accumulator tiles per 16 keys and the Q / dO fragments of a
// half tile need more than the 256 registers of two waves per SIMD; the forward at three waves per SIMD (168 registers)
// spills 1-2, hence FWD_WAVES = 2.
template <>
struct Head<80> {
    static constexpr int DH = 80, NK = 3, FWD_WAVES = 2, DKV_KT = 1, DKV_KEYS = 4 * 16 * DKV_KT, ROWB = 160;
    static constexpr bool DQ_K_OUTER = false;
    static constexpr float SCALE = 0.11180339887498949f;               // 1 / sqrt(80)
    static SC_DEVICE int off(int row, int ch) { return row * ROWB + ch * 16; }
    static SC_DEVICE bf16x8 lds_step(const char* img, int row, int ks, int lg) {
        return *reinterpret_cast<const bf16x8*>(img + row * ROWB + ks * 64 + (ks < 2 ? lg : (lg & 1)) * 16);
    }
    static SC_DEVICE bf16x8 global_step(const bf16* row, int ks, int lg) {
        if (ks < 2) return *reinterpret_cast<const bf16x8*>(row + ks * 32 + lg * 8);
        const u32x4 tail = *reinterpret_cast<const u32x4*>(row + 64 + (lg & 1) * 8);
        const unsigned keep = lg < 2 ? 0xffffffffu : 0u;                // lanes g >= 2: the zero padding of the K extent
        return sc_as_bf16x8((u32x4){tail[0] & keep, tail[1] & keep, tail[2] & keep, tail[3] & keep});
    }
    static SC_DEVICE bf16x8 tr(const char* img, int row0, int c0, int li, int lg) {
        const int q = li >> 2, p = li & 3;
        const char* a = img + (row0 + 4 * lg + q) * ROWB + c0 * 2 + p * 8;
        return sc_cat(sc_lds_tr16(a), sc_lds_tr16(a + 16 * ROWB));
    }
};

// a 16-row fragment over the whole head dim, and the product of two of them
template <class HD>
struct Frag {
    bf16x8 k32[HD::NK];
    static SC_DEVICE Frag lds(const char* img, int row0, int li, int lg) {
        Frag f;
#pragma unroll
        for (int ks = 0; ks < HD::NK; ++ks) f.k32[ks] = HD::lds_step(img, row0 + li, ks, lg);
        return f;
    }
    static SC_DEVICE Frag global(const bf16* row, int lg) {
        Frag f;
#pragma unroll
        for (int ks = 0; ks < HD::NK; ++ks) f.k32[ks] = HD::global_step(row, ks, lg);
        return f;
    }
};
template <class HD>
SC_DEVICE f32x4 dot(const Frag<HD>& a, const Frag<HD>& b) {
    f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HD::NK; ++ks) c = sc_mfma16(a.k32[ks], b.k32[ks], c);
    return c;
}

// the four products of a dq step: s0 = a0.b, s1 = a1.b, p0 = c0.d, p1 = c1.d.  Per accumulator the order of MFMAs is the
// same either way; HD::DQ_K_OUTER only chooses the order in the source, which the scheduler largely keeps: K step by K
// step (four independent accumulators in turn; at dh 64 a ten instructions shorter tile loop with five waits fewer) or
// product by product (at dh 80, where the K-outer order needs 256 registers and spills in the causal instance)
template <class HD>
SC_DEVICE void dot4(const Frag<HD>& a0, const Frag<HD>& a1, const Frag<HD>& b, const Frag<HD>& c0, const Frag<HD>& c1,
                    const Frag<HD>& d, f32x4& s0, f32x4& s1, f32x4& p0, f32x4& p1) {
    if (!HD::DQ_K_OUTER) {
        s0 = dot(a0, b), s1 = dot(a1, b), p0 = dot(c0, d), p1 = dot(c1, d);
        return;
    }
    s0 = s1 = p0 = p1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HD::NK; ++ks) {
        s0 = sc_mfma16(a0.k32[ks], b.k32[ks], s0);
        s1 = sc_mfma16(a1.k32[ks], b.k32[ks], s1);
        p0 = sc_mfma16(c0.k32[ks], d.k32[ks], p0);
        p1 = sc_mfma16(c1.k32[ks], d.k32[ks], p1);
    }
}

// blockIdx -> logical block such that consecutive logical blocks (the row blocks of one head) share an XCD: hardware
// hands block i to XCD i % 8
SC_DEVICE int xcd_block() {
    const int G = gridDim.x, per = G >> 3, rem = G & 7;
    const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
    return x < rem ? x * (per + 1) + i : rem * (per + 1) + (x - rem) * per + i;
}

// register stage of one 64-row tile of two images (256 threads, 512 or 640 16-byte chunks per image); rows at or past
// `lim` are zeros.  The compiler does not know threadIdx.x < 256: the chunk guard is spelt so that it folds when every
// thread has a chunk in every round (dh 64)
template <class HD>
struct Stage {
    static constexpr int CH = HD::DH / 8, NCHUNK = LT * CH, NST = (NCHUNK + 255) / 256;
    static constexpr bool FULL = NCHUNK % 256 == 0;
    u32x4 a[NST], b[NST];
    SC_DEVICE void load(const bf16* src_a, long long stride_a, const bf16* src_b, long long stride_b, int row0, int lim,
                        int t) {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int c = t + u * 256, row = c / CH, ch = c % CH;
            a[u] = b[u] = (u32x4){0u, 0u, 0u, 0u};
            if ((FULL || c < NCHUNK) && row0 + row < lim) {
                a[u] = *reinterpret_cast<const u32x4*>(src_a + (long long)(row0 + row) * stride_a + ch * 8);
                b[u] = *reinterpret_cast<const u32x4*>(src_b + (long long)(row0 + row) * stride_b + ch * 8);
            }
        }
    }
    SC_DEVICE void store(char* img_a, char* img_b, int t) const {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int c = t + u * 256, row = c / CH, ch = c % CH;
            if (FULL || c < NCHUNK) {
                *reinterpret_cast<u32x4*>(img_a + HD::off(row, ch)) = a[u];
                *reinterpret_cast<u32x4*>(img_b + HD::off(row, ch)) = b[u];
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------- forward
// dh 64: 148 VGPRs, three waves per SIMD, i.e. three workgroups per CU; dh 80: 176 (causal: 180), two
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Head<DH>::FWD_WAVES, Head<DH>::FWD_WAVES))) void
attn_fwd_stream_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out, float* __restrict__ lse, int L, int Lq, int H,
                       float scale) {
    using HD = Head<DH>;
    constexpr int DT = DH / 16, IMG = LT * DH * 2;
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];      // [buffer][K image | V image]
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);           // scalar: every per-wave decision is a scalar branch
    const int nqb = (Lq + LB - 1) / LB;
    const int blk = xcd_block();
    const int bh = blk / nqb, qblk = blk % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int q0 = qblk * LB + wave * 32;                              // this wave's first query
    const bool active = q0 < Lq;
    const float c2 = scale * LOG2E;                                     // exp(x*scale) = exp2(x*c2)

    Frag<HD> qf[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) qf[u] = Frag<HD>::global(base + (long long)min(q0 + u * 16 + li, Lq - 1) * rs, lg);
    f32x4 o[2][DT];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m[2] = {-1e30f, -1e30f}, lsum[2] = {0.f, 0.f};

    // keys this workgroup needs: all, or up to its last query under the causal mask
    const int kend = CAUSAL ? min(L, qblk * LB + LB) : L;
    const int nkt = (kend + LT - 1) / LT;
    Stage<HD> st;
    st.load(base + d, rs, base + 2 * d, rs, 0, L, t);
    st.store(smem[0], smem[0] + IMG, t);
    __syncthreads();
    for (int j = 0; j < nkt; ++j) {
        const bool more = j + 1 < nkt;
        if (more) st.load(base + d, rs, base + 2 * d, rs, (j + 1) * LT, L, t);
        const char* Kimg = smem[j & 1];
        const char* Vimg = Kimg + IMG;
        if (active) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int k0 = j * LT + half * 32;
                if (k0 >= L || (CAUSAL && k0 > q0 + 31)) break;
                const Frag<HD> ka = Frag<HD>::lds(Kimg, half * 32, li, lg), kb = Frag<HD>::lds(Kimg, half * 32 + 16, li, lg);
                f32x4 s0[2], s1[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    s0[u] = dot(ka, qf[u]);
                    s1[u] = dot(kb, qf[u]);
                }
                bf16x8 vt[DT];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) vt[dt] = HD::tr(Vimg, half * 32, dt * 16, li, lg);
                if (k0 + 32 > L || (CAUSAL && k0 + 31 > q0)) {          // ragged end / diagonal: masked keys never count
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ka_ = k0 + 4 * lg + r, kb_ = ka_ + 16;
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int q = q0 + u * 16 + li;
                            if (ka_ >= L || (CAUSAL && ka_ > q)) s0[u][r] = -1e30f;
                            if (kb_ >= L || (CAUSAL && kb_ > q)) s1[u][r] = -1e30f;
                        }
                    }
                }
                bf16x8 pf[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float mx = fmaxf(fmaxf(fmaxf(s0[u][0], s0[u][1]), fmaxf(s0[u][2], s0[u][3])),
                                     fmaxf(fmaxf(s1[u][0], s1[u][1]), fmaxf(s1[u][2], s1[u][3])));
                    mx = quad_max(mx);
                    const float mn = fmaxf(m[u], mx);
                    const float nb = -mn * c2;
                    const f32x4 e0 = exp2_affine(s0[u], c2, nb), e1 = exp2_affine(s1[u], c2, nb);
                    const f32x4 pv = e0 + e1;
                    const float ps = (pv[0] + pv[1]) + (pv[2] + pv[3]);
                    pf[u] = pack8(e0, e1);
                    if (__any(mn != m[u])) {                            // running max moved for some query of the tile
                        const float alpha = fast_exp2((m[u] - mn) * c2);
                        lsum[u] *= alpha;
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt) o[u][dt] *= alpha;
                    }
                    m[u] = mn;
                    lsum[u] += ps;
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int u = 0; u < 2; ++u) o[u][dt] = sc_mfma16(vt[dt], pf[u], o[u][dt]);
            }
        }
        if (more) st.store(smem[(j + 1) & 1], smem[(j + 1) & 1] + IMG, t);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = q0 + u * 16 + li;
        const float ls = quad_sum(lsum[u]);
        const float inv = 1.0f / ls;
        if (q < Lq) {
            bf16* orow = out + ((long long)b * L + q) * d + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                *reinterpret_cast<u32x2*>(orow + dt * 16 + lg * 4) =
                    sc_pack4(o[u][dt][0] * inv, o[u][dt][1] * inv, o[u][dt][2] * inv, o[u][dt][3] * inv);
            if (lg == 0) lse[(long long)bh * L + q] = m[u] * scale + __logf(ls);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward: dQ (+ delta)
// dh 64: 202 VGPRs (without the bound on waves: 258 registers, one wave per SIMD); dh 80: 253 (causal: 254), the instance
// with no register to spare.  No scratch, two waves per SIMD
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dq_stream_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ out, const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    using HD = Head<DH>;
    constexpr int DT = DH / 16, CH = DH / 8, IMG = LT * DH * 2;
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nqb = (L + LB - 1) / LB;                                 // every row of dQ is written (zeros past q_rows)
    const int blk = xcd_block();
    const int bh = blk / nqb, qblk = blk % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    bf16* dbase = dqkv + (long long)b * L * rs + h * DH;
    if (qblk * LB >= Lq) {                                              // no consumed query in this block: zeros only
        const int r0 = qblk * LB, nr = min(LB, L - r0);
        for (int c = t; c < nr * CH; c += 256) {
            const int row = c / CH, ch = c % CH;
            *reinterpret_cast<u32x4*>(dbase + (long long)(r0 + row) * rs + ch * 8) = (u32x4){0u, 0u, 0u, 0u};
        }
        return;
    }
    const int q0 = qblk * LB + wave * 32;
    const bool active = q0 < Lq;
    const float c2 = scale * LOG2E;

    Frag<HD> qf[2], gf[2];
    float dl[2], nl2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qc = min(q0 + u * 16 + li, Lq - 1);
        qf[u] = Frag<HD>::global(base + (long long)qc * rs, lg);
        gf[u] = Frag<HD>::global(dout + ((long long)b * L + qc) * d + h * DH, lg);
        const Frag<HD> of = Frag<HD>::global(out + ((long long)b * L + qc) * d + h * DH, lg);
        float acc = 0.f;
#pragma unroll
        for (int ks = 0; ks < HD::NK; ++ks)                             // zero-padded lanes of a fragment add nothing
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += (float)gf[u].k32[ks][e] * (float)of.k32[ks][e];
        dl[u] = quad_sum(acc);
        nl2[u] = -lse[(long long)bh * L + qc] * LOG2E;
        const int q = q0 + u * 16 + li;
        if (active && q < Lq && lg == 0) delta[(long long)bh * L + q] = dl[u];
    }
    f32x4 dq[2][DT];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int kend = CAUSAL ? min(L, qblk * LB + LB) : L;
    const int nkt = (kend + LT - 1) / LT;
    Stage<HD> st;
    st.load(base + d, rs, base + 2 * d, rs, 0, L, t);
    st.store(smem[0], smem[0] + IMG, t);
    __syncthreads();
    for (int j = 0; j < nkt; ++j) {
        const bool more = j + 1 < nkt;
        if (more) st.load(base + d, rs, base + 2 * d, rs, (j + 1) * LT, L, t);
        const char* Kimg = smem[j & 1];
        const char* Vimg = Kimg + IMG;
        if (active) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int k0 = j * LT + half * 32;
                if (k0 >= L || (CAUSAL && k0 > q0 + 31)) break;
                const Frag<HD> ka = Frag<HD>::lds(Kimg, half * 32, li, lg), kb = Frag<HD>::lds(Kimg, half * 32 + 16, li, lg);
                const Frag<HD> va = Frag<HD>::lds(Vimg, half * 32, li, lg), vb = Frag<HD>::lds(Vimg, half * 32 + 16, li, lg);
                bf16x8 kt[DT];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) kt[dt] = HD::tr(Kimg, half * 32, dt * 16, li, lg);
                const bool edge = k0 + 32 > L || (CAUSAL && k0 + 31 > q0);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    f32x4 s0, s1, p0, p1;
                    dot4(ka, kb, qf[u], va, vb, gf[u], s0, s1, p0, p1);
                    f32x4 e0 = exp2_affine(s0, c2, nl2[u]), e1 = exp2_affine(s1, c2, nl2[u]);
                    if (edge) {
                        const int q = q0 + u * 16 + li;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ka_ = k0 + 4 * lg + r, kb_ = ka_ + 16;
                            if (ka_ >= L || (CAUSAL && ka_ > q)) e0[r] = 0.f;
                            if (kb_ >= L || (CAUSAL && kb_ > q)) e1[r] = 0.f;
                        }
                    }
                    const bf16x8 dsf = pack8(e0 * (p0 - dl[u]), e1 * (p1 - dl[u]));
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) dq[u][dt] = sc_mfma16(kt[dt], dsf, dq[u][dt]);
                }
            }
        }
        if (more) st.store(smem[(j + 1) & 1], smem[(j + 1) & 1] + IMG, t);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = q0 + u * 16 + li;
        if (q >= L) continue;
        const float sc = q < Lq ? scale : 0.f;                          // rows past q_rows: zeros
        bf16* drow = dbase + (long long)q * rs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            *reinterpret_cast<u32x2*>(drow + dt * 16 + lg * 4) =
                sc_pack4(dq[u][dt][0] * sc, dq[u][dt][1] * sc, dq[u][dt][2] * sc, dq[u][dt][3] * sc);
    }
}

// ---------------------------------------------------------------------------------------------- backward: dK, dV
// 4 waves x DKV_KT 16-key tiles per workgroup.  dh 64: 254 VGPRs (without the bound on waves: 268 registers, one wave
// per SIMD); dh 80: 176 (causal: 170; three waves per SIMD, 168 registers, would spill 6 to 10).  No scratch, two waves
// per SIMD
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dkv_stream_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    using HD = Head<DH>;
    constexpr int DT = DH / 16, IMG = LT * DH * 2, KT = HD::DKV_KT, KW = 16 * KT, LBK = HD::DKV_KEYS;
    constexpr int BUF = 2 * IMG + 2 * LT * 4;                           // Q image | dO image | -lse*log2e | delta
    __shared__ __attribute__((aligned(16))) char smem[2][BUF];
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nkb = (L + LBK - 1) / LBK;
    const int blk = xcd_block();
    const int bh = blk / nkb, kblk = blk % nkb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const bf16* gbase = dout + (long long)b * L * d + h * DH;
    const float* lrow = lse + (long long)bh * L;
    const float* drow_ = delta + (long long)bh * L;
    const int k0w = kblk * LBK + wave * KW;                             // this wave's first key
    const bool active = k0w < L;
    const float c2 = scale * LOG2E;

    Frag<HD> kf[KT], vf[KT];
    f32x4 dk[KT][DT], dv[KT][DT];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        const int kc = min(k0w + u * 16 + li, L - 1);
        kf[u] = Frag<HD>::global(base + d + (long long)kc * rs, lg);
        vf[u] = Frag<HD>::global(base + 2 * d + (long long)kc * rs, lg);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[u][dt] = dv[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // queries this workgroup needs: all consumed ones, or from its first key on under the causal mask
    const int j0 = CAUSAL ? (kblk * LBK) / LT : 0;
    const int nqt = (Lq + LT - 1) / LT;
    Stage<HD> st;
    float rl = 0.f, rd = 0.f;                                           // thread t < 64: row t of the tile's lse / delta
    auto load_rows = [&](int r0) {
        st.load(base, rs, gbase, d, r0, Lq, t);
        if (t < LT) {
            const bool ok = r0 + t < Lq;
            rl = ok ? -lrow[r0 + t] * LOG2E : 0.f;
            rd = ok ? drow_[r0 + t] : 0.f;
        }
    };
    auto store_rows = [&](char* buf) {
        st.store(buf, buf + IMG, t);
        if (t < LT) {
            reinterpret_cast<float*>(buf + 2 * IMG)[t] = rl;
            reinterpret_cast<float*>(buf + 2 * IMG + LT * 4)[t] = rd;
        }
    };
    if (!CAUSAL || j0 < nqt) {                                          // j0 = 0 < nqt without the mask
        load_rows(j0 * LT);
        store_rows(smem[j0 & 1]);
    }
    __syncthreads();
    const bool kedge = k0w + KW > L;
    for (int j = j0; j < nqt; ++j) {
        const bool more = j + 1 < nqt;
        if (more) load_rows((j + 1) * LT);
        const char* Qimg = smem[j & 1];
        const char* Gimg = Qimg + IMG;
        const float* slse = reinterpret_cast<const float*>(Qimg + 2 * IMG);
        const float* sdel = slse + LT;
        if (active) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int qb0 = j * LT + half * 32;
                if (qb0 >= Lq) break;
                if (CAUSAL && qb0 + 31 < k0w) continue;                 // every query of the half precedes every key
                const Frag<HD> qa = Frag<HD>::lds(Qimg, half * 32, li, lg), qb = Frag<HD>::lds(Qimg, half * 32 + 16, li, lg);
                const Frag<HD> ga = Frag<HD>::lds(Gimg, half * 32, li, lg), gb = Frag<HD>::lds(Gimg, half * 32 + 16, li, lg);
                // transposed dO / Q tiles: a wave with two key tiles reads them once for both; with one tile they are read
                // where they are used, which keeps 40 registers free across the softmax (dh 80: 176 instead of 216)
                bf16x8 gt[DT], qt[DT];
                if (KT > 1) {
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        gt[dt] = HD::tr(Gimg, half * 32, dt * 16, li, lg);
                        qt[dt] = HD::tr(Qimg, half * 32, dt * 16, li, lg);
                    }
                }
                f32x4 la, lb, da, db;                                   // row constants of queries 4g+r and 16+4g+r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    la[r] = slse[half * 32 + 4 * lg + r];
                    lb[r] = slse[half * 32 + 16 + 4 * lg + r];
                    da[r] = sdel[half * 32 + 4 * lg + r];
                    db[r] = sdel[half * 32 + 16 + 4 * lg + r];
                }
                const bool edge = qb0 + 32 > Lq || kedge || (CAUSAL && qb0 < k0w + KW);
#pragma unroll
                for (int u = 0; u < KT; ++u) {
                    const int key = k0w + u * 16 + li;
                    const f32x4 s0 = dot(qa, kf[u]), s1 = dot(qb, kf[u]);
                    const f32x4 p0 = dot(ga, vf[u]), p1 = dot(gb, vf[u]);
                    f32x4 e0, e1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        e0[r] = fast_exp2(fmaf(s0[r], c2, la[r]));
                        e1[r] = fast_exp2(fmaf(s1[r], c2, lb[r]));
                    }
                    if (edge) {                                         // masked entries are exact zeros
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int qa_ = qb0 + 4 * lg + r, qb_ = qa_ + 16;
                            if (qa_ >= Lq || key >= L || (CAUSAL && key > qa_)) e0[r] = 0.f;
                            if (qb_ >= Lq || key >= L || (CAUSAL && key > qb_)) e1[r] = 0.f;
                        }
                    }
                    const bf16x8 pf = pack8(e0, e1), dsf = pack8(e0 * (p0 - da), e1 * (p1 - db));
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        dv[u][dt] = sc_mfma16(KT > 1 ? gt[dt] : HD::tr(Gimg, half * 32, dt * 16, li, lg), pf, dv[u][dt]);
                        dk[u][dt] = sc_mfma16(KT > 1 ? qt[dt] : HD::tr(Qimg, half * 32, dt * 16, li, lg), dsf, dk[u][dt]);
                    }
                }
            }
        }
        if (more) store_rows(smem[(j + 1) & 1]);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        const int key = k0w + u * 16 + li;
        if (key >= L) continue;
        bf16* drow = dqkv + ((long long)b * L + key) * rs + h * DH;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            *reinterpret_cast<u32x2*>(drow + d + dt * 16 + lg * 4) =
                sc_pack4(dk[u][dt][0] * scale, dk[u][dt][1] * scale, dk[u][dt][2] * scale, dk[u][dt][3] * scale);
            *reinterpret_cast<u32x2*>(drow + 2 * d + dt * 16 + lg * 4) =
                sc_pack4(dv[u][dt][0], dv[u][dt][1], dv[u][dt][2], dv[u][dt][3]);
        }
    }
}

// the instances that exist: (64, non-causal) at any L, (80, either) up to MAXL
bool stream_shape(const AttnShape& s) { return s.dh == 64 ? !s.causal : s.dh == 80 && s.L <= MAXL; }

template <class F>
void stream_instance(const AttnShape& s, F&& f) {
    if (s.dh == 64) f(std::integral_constant<int, 64>{}, std::false_type{});
    else attn_dispatch(attn_causal{}, s.causal != 0, [&](auto C) { f(std::integral_constant<int, 80>{}, C); });
}

// number of workgroups for `rows` rows in blocks of `per`, or 0 when it does not fit a grid
unsigned stream_grid(const AttnShape& s, int rows, int per) {
    const long long g = (long long)s.B * s.H * ((rows + per - 1) / per);
    return g > 0x7fffffffLL ? 0u : (unsigned)g;
}
unsigned stream_grid_dkv(const AttnShape& s) {
    return stream_grid(s, s.L, s.dh == 64 ? Head<64>::DKV_KEYS : Head<80>::DKV_KEYS);
}

}  // namespace

bool sc_attn_fwd_stream_accepts(const AttnShape& s) { return stream_shape(s) && stream_grid(s, s.Lq, LB); }

int sc_attn_fwd_stream_launch(const AttnShape& s, const AttnFwdOps& o, hipStream_t st) {
    stream_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_fwd_stream_kernel<DH.value, C.value != 0>, stream_grid(s, s.Lq, LB), 256, 0, st, o.qkv, o.out, o.lse,
                    s.L, s.Lq, s.H, Head<DH.value>::SCALE);
    });
    return 0;
}

bool sc_attn_bwd_stream_accepts(const AttnShape& s) { return stream_shape(s) && stream_grid(s, s.L, LB) && stream_grid_dkv(s); }

int sc_attn_bwd_stream_launch(const AttnShape& s, const AttnBwdOps& o, hipStream_t st) {
    stream_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_bwd_dq_stream_kernel<DH.value, C.value != 0>, stream_grid(s, s.L, LB), 256, 0, st, o.qkv, o.out,
                    o.dout, o.lse, o.delta, o.dqkv, s.L, s.Lq, s.H, Head<DH.value>::SCALE);
        attn_launch(attn_bwd_dkv_stream_kernel<DH.value, C.value != 0>, stream_grid_dkv(s), 256, 0, st, o.qkv, o.dout, o.lse,
                    o.delta, o.dqkv, s.L, s.Lq, s.H, Head<DH.value>::SCALE);
    });
    return 0;
}
