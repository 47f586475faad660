// Attention at head dim 80 (ViT-H: width 1280 = 16 heads of 80), 0 < L <= 320, causal or not.
//
// Structure: the streamed one of sc_attention_long.hip, not the head-in-LDS one of sc_attention.hip.  K and V of a
// 257-token head are 90 KiB at 160-byte rows, so two head-resident workgroups do not share a CU (160 KiB) and the fused
// backward (four images, 182 KiB) fits not at all; 64-row tiles through two LDS buffers cost 40 KiB per workgroup and keep
// two workgroups on a CU (176-254 registers per lane: two waves per SIMD), each loading its next tile while it computes the
// current one.
//
// 80 = 2 x 32 + 16.  Where dh is the K extent (S^T = K.Q^T, dP^T = V.dO^T and their dkv-kernel forms) the K loop is three
// 16x16x32 bf16 MFMAs, the third on columns 64..79 with the upper half of its K extent zero in the REGISTER-side operand
// (struct Frag below); nothing is padded in HBM or LDS.  The K = 16 instruction (v_mfma_f32_16x16x16_bf16) would save
// half an MFMA per product, but chained behind a 16x16x32 through SrcC with a different destination the toolchain emits
// no wait states between the two and the sums came out wrong intermittently on the device; one instruction type keeps the
// chains on the path every other kernel here uses.  Where dh is an M extent (O^T = V^T.P^T, dQ^T, dK^T, dV^T) it is five
// 16-row tiles instead of four.
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
// Products are transposed as in the other attention kernels (key on the MFMA row, query on the column), so that the
// softmax statistics of a query live in the lanes of its accumulators and P / dS feed the next MFMA from registers.
// No float atomics; every sum has a fixed order (bit-reproducible).  Causal: a workgroup stops (forward, dq) or starts
// (dkv) its tile loop at the diagonal and a wave skips 32-row halves that lie wholly above it.
#include "sc_attn_common.h"

namespace {

constexpr int DH = 80;
constexpr int CH = DH / 8;              // 16-byte chunks per row
constexpr int DT = DH / 16;             // 16-row output tiles
constexpr int ROWB = DH * 2;            // bytes per LDS image row (dense)
constexpr int LT = 64;                  // rows per streamed tile
constexpr int LB = 128;                 // queries per workgroup of the forward and dq kernels: 4 waves x 32
constexpr int IMG = LT * ROWB;          // one 64 x 80 bf16 image: 10 KiB
constexpr int NCHUNK = LT * CH;         // 640 chunks per image and tile
constexpr int NST = (NCHUNK + 255) / 256;
constexpr float LOG2E = 1.4426950408889634f;

// a 16-row fragment over the whole head dim as three K = 32 steps: lane (g, i) holds row i, columns 32 ks + 8g .. + 7 for
// ks = 0, 1, and in the third step columns 64 + 8 (g & 1) .. + 7.  The third step covers 80 = 64 + 16 with the upper
// half of its K extent padded IN REGISTERS: the register-side operand of every product (Q, dO in the forward and dq
// kernels, K, V in the dkv kernel; loaded once per wave) holds zeros in lanes g >= 2, so whatever finite values the
// LDS-side operand repeats there (it re-reads columns 64..79, a broadcast) contribute nothing.
struct Frag {
    bf16x8 k32[3];
};
SC_DEVICE Frag frag_lds(const char* img, int row0, int li, int lg) {
    const char* p = img + (row0 + li) * ROWB;
    Frag f;
    f.k32[0] = *reinterpret_cast<const bf16x8*>(p + lg * 16);
    f.k32[1] = *reinterpret_cast<const bf16x8*>(p + 64 + lg * 16);
    f.k32[2] = *reinterpret_cast<const bf16x8*>(p + 128 + (lg & 1) * 16);
    return f;
}
SC_DEVICE Frag frag_global(const bf16* row, int lg) {
    Frag f;
    f.k32[0] = *reinterpret_cast<const bf16x8*>(row + lg * 8);
    f.k32[1] = *reinterpret_cast<const bf16x8*>(row + 32 + lg * 8);
    const u32x4 tail = *reinterpret_cast<const u32x4*>(row + 64 + (lg & 1) * 8);
    const unsigned keep = lg < 2 ? 0xffffffffu : 0u;                    // lanes g >= 2: the zero padding of the K extent
    f.k32[2] = sc_as_bf16x8((u32x4){tail[0] & keep, tail[1] & keep, tail[2] & keep, tail[3] & keep});
    return f;
}
SC_DEVICE f32x4 dot80(const Frag& a, const Frag& b, f32x4 c) {
    c = sc_mfma16(a.k32[0], b.k32[0], c);
    c = sc_mfma16(a.k32[1], b.k32[1], c);
    return sc_mfma16(a.k32[2], b.k32[2], c);
}
// transposed fragment over a 32-row block for the 16 columns [c0, c0 + 16): lane (g, i) gets img[row0 + slot(g, j)][c0 + i]
SC_DEVICE bf16x8 frag_tr80(const char* img, int row0, int c0, int li, int lg) {
    const int q = li >> 2, p = li & 3;
    const char* a = img + (row0 + 4 * lg + q) * ROWB + c0 * 2 + p * 8;
    return sc_cat(sc_lds_tr16(a), sc_lds_tr16(a + 16 * ROWB));
}

SC_DEVICE int xcd_block80() {
    const int G = gridDim.x, per = G >> 3, rem = G & 7;
    const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
    return x < rem ? x * (per + 1) + i : rem * (per + 1) + (x - rem) * per + i;
}

// register stage of one 64-row tile of two images (256 threads, 640 chunks per image); rows at or past `lim` are zeros
struct Stage80 {
    u32x4 a[NST], b[NST];
    SC_DEVICE void load(const bf16* src_a, long long stride_a, const bf16* src_b, long long stride_b, int row0, int lim,
                        int t) {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int c = t + u * 256, row = c / CH, ch = c % CH;
            a[u] = b[u] = (u32x4){0u, 0u, 0u, 0u};
            if (c < NCHUNK && row0 + row < lim) {
                a[u] = *reinterpret_cast<const u32x4*>(src_a + (long long)(row0 + row) * stride_a + ch * 8);
                b[u] = *reinterpret_cast<const u32x4*>(src_b + (long long)(row0 + row) * stride_b + ch * 8);
            }
        }
    }
    SC_DEVICE void store(char* img_a, char* img_b, int t) const {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int c = t + u * 256;
            if (c < NCHUNK) {                                           // dense image: chunk c sits at byte 16 c
                *reinterpret_cast<u32x4*>(img_a + c * 16) = a[u];
                *reinterpret_cast<u32x4*>(img_b + c * 16) = b[u];
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------- forward
// 176-180 VGPRs: two waves per SIMD (at three, 168 registers, it spills 1-2)
template <bool CAUSAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_fwd_d80_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ out, float* __restrict__ lse, int L, int Lq, int H, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];      // [buffer][K image | V image]
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);           // scalar: every per-wave decision is a scalar branch
    const int nqb = (Lq + LB - 1) / LB;
    const int blk = xcd_block80();
    const int bh = blk / nqb, qblk = blk % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int q0 = qblk * LB + wave * 32;                              // this wave's first query
    const bool active = q0 < Lq;
    const float c2 = scale * LOG2E;                                     // exp(x*scale) = exp2(x*c2)

    Frag qf[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) qf[u] = frag_global(base + (long long)min(q0 + u * 16 + li, Lq - 1) * rs, lg);
    f32x4 o[2][DT];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m[2] = {-1e30f, -1e30f}, lsum[2] = {0.f, 0.f};

    // keys this workgroup needs: all, or up to its last query under the causal mask
    const int kend = CAUSAL ? min(L, qblk * LB + LB) : L;
    const int nkt = (kend + LT - 1) / LT;
    Stage80 st;
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
                const Frag ka = frag_lds(Kimg, half * 32, li, lg), kb = frag_lds(Kimg, half * 32 + 16, li, lg);
                f32x4 s0[2], s1[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    s0[u] = dot80(ka, qf[u], (f32x4){0.f, 0.f, 0.f, 0.f});
                    s1[u] = dot80(kb, qf[u], (f32x4){0.f, 0.f, 0.f, 0.f});
                }
                bf16x8 vt[DT];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) vt[dt] = frag_tr80(Vimg, half * 32, dt * 16, li, lg);
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
// 253-254 VGPRs, no scratch: two waves per SIMD
template <bool CAUSAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dq_d80_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ out, const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);           // scalar: every per-wave decision is a scalar branch
    const int nqb = (L + LB - 1) / LB;                                 // every row of dQ is written (zeros past q_rows)
    const int blk = xcd_block80();
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

    Frag qf[2], gf[2];
    float dl[2], nl2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qc = min(q0 + u * 16 + li, Lq - 1);
        qf[u] = frag_global(base + (long long)qc * rs, lg);
        gf[u] = frag_global(dout + ((long long)b * L + qc) * d + h * DH, lg);
        const Frag of = frag_global(out + ((long long)b * L + qc) * d + h * DH, lg);
        float acc = 0.f;
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)                                  // the zero lanes of the third step add nothing
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
    Stage80 st;
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
                const Frag ka = frag_lds(Kimg, half * 32, li, lg), kb = frag_lds(Kimg, half * 32 + 16, li, lg);
                const Frag va = frag_lds(Vimg, half * 32, li, lg), vb = frag_lds(Vimg, half * 32 + 16, li, lg);
                bf16x8 kt[DT];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) kt[dt] = frag_tr80(Kimg, half * 32, dt * 16, li, lg);
                const bool edge = k0 + 32 > L || (CAUSAL && k0 + 31 > q0);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const f32x4 s0 = dot80(ka, qf[u], z), s1 = dot80(kb, qf[u], z);
                    const f32x4 p0 = dot80(va, gf[u], z), p1 = dot80(vb, gf[u], z);
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
// 4 waves x 16 keys per workgroup: with 32 keys per wave the K / V fragments, ten accumulator tiles per 16 keys and the
// Q / dO fragments of a half tile need more than the 256 registers of two waves per SIMD; with 16 keys it is about 180
// (three waves per SIMD, 168 registers, would spill 6 to 10 of them)
constexpr int KVT = 256;                // threads of the dkv kernel
constexpr int LBK = KVT / 64 * 16;      // keys per workgroup of the dkv kernel
constexpr int NSK = (NCHUNK + KVT - 1) / KVT;
template <bool CAUSAL>
__global__ __launch_bounds__(KVT) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dkv_d80_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    constexpr int BUF = 2 * IMG + 2 * LT * 4;                           // Q image | dO image | -lse*log2e | delta
    __shared__ __attribute__((aligned(16))) char smem[2][BUF];
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);           // scalar: every per-wave decision is a scalar branch
    const int nkb = (L + LBK - 1) / LBK;
    const int blk = xcd_block80();
    const int bh = blk / nkb, kblk = blk % nkb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const bf16* gbase = dout + (long long)b * L * d + h * DH;
    const float* lrow = lse + (long long)bh * L;
    const float* drow_ = delta + (long long)bh * L;
    const int k0w = kblk * LBK + wave * 16;                              // this wave's first key
    const bool active = k0w < L;
    const float c2 = scale * LOG2E;
    const int key = k0w + li;

    const int kc = min(key, L - 1);
    const Frag kf = frag_global(base + d + (long long)kc * rs, lg), vf = frag_global(base + 2 * d + (long long)kc * rs, lg);
    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // queries this workgroup needs: all consumed ones, or from its first key on under the causal mask
    const int j0 = CAUSAL ? (kblk * LBK) / LT : 0;
    const int nqt = (Lq + LT - 1) / LT;
    u32x4 sa[NSK], sb[NSK];
    float rl = 0.f, rd = 0.f;                                           // thread t < 64: row t of the tile's lse / delta
    auto load_rows = [&](int r0) {
#pragma unroll
        for (int u = 0; u < NSK; ++u) {
            const int c = t + u * KVT, row = c / CH, ch = c % CH;
            sa[u] = sb[u] = (u32x4){0u, 0u, 0u, 0u};
            if (c < NCHUNK && r0 + row < Lq) {
                sa[u] = *reinterpret_cast<const u32x4*>(base + (long long)(r0 + row) * rs + ch * 8);
                sb[u] = *reinterpret_cast<const u32x4*>(gbase + (long long)(r0 + row) * d + ch * 8);
            }
        }
        if (t < LT) {
            const bool ok = r0 + t < Lq;
            rl = ok ? -lrow[r0 + t] * LOG2E : 0.f;
            rd = ok ? drow_[r0 + t] : 0.f;
        }
    };
    auto store_rows = [&](char* buf) {
#pragma unroll
        for (int u = 0; u < NSK; ++u) {
            const int c = t + u * KVT;
            if (c < NCHUNK) {
                *reinterpret_cast<u32x4*>(buf + c * 16) = sa[u];
                *reinterpret_cast<u32x4*>(buf + IMG + c * 16) = sb[u];
            }
        }
        if (t < LT) {
            reinterpret_cast<float*>(buf + 2 * IMG)[t] = rl;
            reinterpret_cast<float*>(buf + 2 * IMG + LT * 4)[t] = rd;
        }
    };
    if (j0 < nqt) {
        load_rows(j0 * LT);
        store_rows(smem[j0 & 1]);
    }
    __syncthreads();
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
                const Frag qa = frag_lds(Qimg, half * 32, li, lg), qb = frag_lds(Qimg, half * 32 + 16, li, lg);
                const Frag ga = frag_lds(Gimg, half * 32, li, lg), gb = frag_lds(Gimg, half * 32 + 16, li, lg);
                f32x4 la, lb, da, db;                                   // row constants of queries 4g+r and 16+4g+r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    la[r] = slse[half * 32 + 4 * lg + r];
                    lb[r] = slse[half * 32 + 16 + 4 * lg + r];
                    da[r] = sdel[half * 32 + 4 * lg + r];
                    db[r] = sdel[half * 32 + 16 + 4 * lg + r];
                }
                const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
                const f32x4 s0 = dot80(qa, kf, z), s1 = dot80(qb, kf, z);
                const f32x4 p0 = dot80(ga, vf, z), p1 = dot80(gb, vf, z);
                f32x4 e0, e1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e0[r] = fast_exp2(fmaf(s0[r], c2, la[r]));
                    e1[r] = fast_exp2(fmaf(s1[r], c2, lb[r]));
                }
                if (qb0 + 32 > Lq || key >= L || (CAUSAL && qb0 < k0w + 16)) {      // masked entries are exact zeros
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
                    dv[dt] = sc_mfma16(frag_tr80(Gimg, half * 32, dt * 16, li, lg), pf, dv[dt]);
                    dk[dt] = sc_mfma16(frag_tr80(Qimg, half * 32, dt * 16, li, lg), dsf, dk[dt]);
                }
            }
        }
        if (more) store_rows(smem[(j + 1) & 1]);
        __syncthreads();
    }
    if (!active || key >= L) return;
    bf16* drow = dqkv + ((long long)b * L + key) * rs + h * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        *reinterpret_cast<u32x2*>(drow + d + dt * 16 + lg * 4) =
            sc_pack4(dk[dt][0] * scale, dk[dt][1] * scale, dk[dt][2] * scale, dk[dt][3] * scale);
        *reinterpret_cast<u32x2*>(drow + 2 * d + dt * 16 + lg * 4) = sc_pack4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
    }
}

constexpr float SCALE80 = 0.11180339887498949f;                        // 1 / sqrt(80)

bool d80_shape(int B, int L, int Lq, int H, int dh) {
    return dh == DH && B > 0 && H > 0 && L > 0 && L <= MAXL && Lq > 0 && Lq <= L;
}

}  // namespace

int sc_attn_fwd_d80(const void* qkv, void* out, float* lse, int B, int L, int Lq, int H, int dh, int causal,
                    hipStream_t st) {
    if (!d80_shape(B, L, Lq, H, dh)) return 0;
    const long long grid = (long long)B * H * ((Lq + LB - 1) / LB);
    if (grid > 0x7fffffffLL) return 0;
    if (causal)
        attn_fwd_d80_kernel<true><<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (bf16*)out, lse, L, Lq, H, SCALE80);
    else
        attn_fwd_d80_kernel<false><<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (bf16*)out, lse, L, Lq, H, SCALE80);
    return 1;
}

int sc_attn_bwd_d80(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv, int B,
                    int L, int Lq, int H, int dh, int causal, hipStream_t st) {
    if (!d80_shape(B, L, Lq, H, dh)) return 0;
    const long long grid = (long long)B * H * ((L + LB - 1) / LB), gkv = (long long)B * H * ((L + LBK - 1) / LBK);
    if (grid > 0x7fffffffLL || gkv > 0x7fffffffLL) return 0;
    if (causal) {
        attn_bwd_dq_d80_kernel<true><<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (const bf16*)out, (const bf16*)dout,
                                                                     lse, delta, (bf16*)dqkv, L, Lq, H, SCALE80);
        attn_bwd_dkv_d80_kernel<true><<<(unsigned)gkv, KVT, 0, st>>>((const bf16*)qkv, (const bf16*)dout, lse, delta,
                                                                      (bf16*)dqkv, L, Lq, H, SCALE80);
    } else {
        attn_bwd_dq_d80_kernel<false><<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (const bf16*)out, (const bf16*)dout,
                                                                      lse, delta, (bf16*)dqkv, L, Lq, H, SCALE80);
        attn_bwd_dkv_d80_kernel<false><<<(unsigned)gkv, KVT, 0, st>>>((const bf16*)qkv, (const bf16*)dout, lse, delta,
                                                                       (bf16*)dqkv, L, Lq, H, SCALE80);
    }
    return 1;
}
