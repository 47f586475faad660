// Attention for sequences of any length (dh = 64, non-causal): ViT-L/14 at 336 px (577 tokens), 280 px (401), ViT-B/16
// towers above 284 px.  The per-head kernels keep a whole head in LDS and stop at L = 320; these stream it.
//
// Forward: one workgroup (4 waves) = 128 query rows of one (batch, head), 32 per wave as two 16-query MFMA column tiles
// whose Q fragments stay in registers.  K and V pass through LDS in 64-key tiles (one swizzled Img<64> each, read by rows
// for S and by ds_read_b64_tr_b16 for P.V), double buffered: the global loads of tile j + 1 are in flight while tile j is
// computed, and one barrier per tile separates the LDS write of one buffer from the reads of the other.  Products are
// transposed as in sc_attention.hip (key on the MFMA row, query on the column), so a query's running max and sum live in
// the lanes of its accumulators: online softmax in fp32, O rescaled only when some row's max moves.  The last tile is
// walked in 32-key halves and a half past L is skipped (577 = 9 * 64 + 1 costs one 32-key half, not a 64-key tile).
//
// Backward: two kernels, no float atomics, a fixed summation order everywhere (bit-reproducible):
//   dq kernel : the forward's structure (128 queries per workgroup, K/V streamed): P recomputed from Q, K and lse,
//               dP^T = V.dO^T, dS^T, dQ^T += K^T.dS^T; also writes delta = rowsum(dO * O).  Rows from q_rows on: zeros.
//   dkv kernel: 128 keys per workgroup, 32 per wave with K and V fragments in registers, Q / dO / lse / delta streamed in
//               64-query tiles: S = Q.K^T and dP = dO.V^T with the key on the lane, so P and dS are directly the B
//               operands of dV^T += dO^T.P and dK^T += Q^T.dS.
// Workgroups of one head are mapped onto one XCD so that its K / V (forward, dq) or Q / dO (dkv) is fetched into one L2.
#include "sc_attn_common.h"

namespace {

constexpr int LT = 64;                  // rows per streamed tile
constexpr int LB = 128;                 // rows (queries or keys) per workgroup: 4 waves x 32
constexpr int IMG = LT * 64 * 2;        // one 64 x 64 bf16 image: 8 KiB
constexpr float LOG2E = 1.4426950408889634f;

// blockIdx -> logical block such that consecutive logical blocks (the row blocks of one head) share an XCD: hardware
// hands block i to XCD i % 8
SC_DEVICE int xcd_block() {
    const int G = gridDim.x, per = G >> 3, rem = G & 7;
    const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
    return x < rem ? x * (per + 1) + i : rem * (per + 1) + (x - rem) * per + i;
}

// register stage of one 64-row tile of two images (256 threads, two 16-byte chunks per image and thread); rows at or
// past `lim` are zeros
struct Stage2 {
    u32x4 a[2], b[2];
    SC_DEVICE void load(const bf16* src_a, long long stride_a, const bf16* src_b, long long stride_b, int row0, int lim,
                        int t) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = t + u * 256, row = c >> 3, ch = c & 7;
            a[u] = b[u] = (u32x4){0u, 0u, 0u, 0u};
            if (row0 + row < lim) {
                a[u] = *reinterpret_cast<const u32x4*>(src_a + (long long)(row0 + row) * stride_a + ch * 8);
                b[u] = *reinterpret_cast<const u32x4*>(src_b + (long long)(row0 + row) * stride_b + ch * 8);
            }
        }
    }
    SC_DEVICE void store(char* img_a, char* img_b, int t) const {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = t + u * 256, row = c >> 3, ch = c & 7;
            *reinterpret_cast<u32x4*>(img_a + Img<64>::off(row, ch)) = a[u];
            *reinterpret_cast<u32x4*>(img_b + Img<64>::off(row, ch)) = b[u];
        }
    }
};

// ---------------------------------------------------------------------------------------------- forward
// 148 VGPRs: three waves per SIMD, i.e. three workgroups per CU
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_fwd_long_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ out, float* __restrict__ lse, int L, int Lq, int H, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];      // [buffer][K image | V image]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int nqb = (Lq + LB - 1) / LB;
    const int blk = xcd_block();
    const int bh = blk / nqb, qblk = blk % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * 64;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * 64;
    const int q0 = qblk * LB + wave * 32;                              // this wave's first query
    const bool active = q0 < Lq;
    const float c2 = scale * LOG2E;                                     // exp(x*scale) = exp2(x*c2)

    bf16x8 qf[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qc = min(q0 + u * 16 + li, Lq - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            qf[u][ks] = *reinterpret_cast<const bf16x8*>(base + (long long)qc * rs + ks * 32 + lg * 8);
    }
    f32x4 o[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m[2] = {-1e30f, -1e30f}, lsum[2] = {0.f, 0.f};

    const int nkt = (L + LT - 1) / LT;
    Stage2 st;
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
                if (k0 >= L) break;
                bf16x8 ka[2], kb[2], vt[4];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    ka[ks] = frag_row<64>(Kimg, half * 32, ks, li, lg);
                    kb[ks] = frag_row<64>(Kimg, half * 32 + 16, ks, li, lg);
                }
                f32x4 s0[2], s1[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    s0[u] = s1[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        s0[u] = sc_mfma16(ka[ks], qf[u][ks], s0[u]);
                        s1[u] = sc_mfma16(kb[ks], qf[u][ks], s1[u]);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) vt[dt] = frag_tr<64>(Vimg, half * 32, dt * 16, li, lg);
                if (k0 + 32 > L) {                                      // ragged end: keys past L never count
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ka_ = k0 + 4 * lg + r, kb_ = ka_ + 16;
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            if (ka_ >= L) s0[u][r] = -1e30f;
                            if (kb_ >= L) s1[u][r] = -1e30f;
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
                        for (int dt = 0; dt < 4; ++dt) o[u][dt] *= alpha;
                    }
                    m[u] = mn;
                    lsum[u] += ps;
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
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
            bf16* orow = out + ((long long)b * L + q) * d + h * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<u32x2*>(orow + dt * 16 + lg * 4) =
                    sc_pack4(o[u][dt][0] * inv, o[u][dt][1] * inv, o[u][dt][2] * inv, o[u][dt][3] * inv);
            if (lg == 0) lse[(long long)bh * L + q] = m[u] * scale + __logf(ls);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward: dQ (+ delta)
// 202 VGPRs: two waves per SIMD (without the bound: 258 registers, one wave)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dq_long_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ out, const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int nqb = (L + LB - 1) / LB;                                 // every row of dQ is written (zeros past q_rows)
    const int blk = xcd_block();
    const int bh = blk / nqb, qblk = blk % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * 64;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * 64;
    bf16* dbase = dqkv + (long long)b * L * rs + h * 64;
    if (qblk * LB >= Lq) {                                              // no consumed query in this block: zeros only
        const int r0 = qblk * LB, nr = min(LB, L - r0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = t + u * 256, row = c >> 3, ch = c & 7;
            if (row < nr) *reinterpret_cast<u32x4*>(dbase + (long long)(r0 + row) * rs + ch * 8) = (u32x4){0u, 0u, 0u, 0u};
        }
        return;
    }
    const int q0 = qblk * LB + wave * 32;
    const bool active = q0 < Lq;
    const float c2 = scale * LOG2E;

    bf16x8 qf[2][2], gf[2][2];
    float dl[2], nl2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qc = min(q0 + u * 16 + li, Lq - 1);
        const bf16* orow = out + ((long long)b * L + qc) * d + h * 64;
        const bf16* grow = dout + ((long long)b * L + qc) * d + h * 64;
        float acc = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[u][ks] = *reinterpret_cast<const bf16x8*>(base + (long long)qc * rs + ks * 32 + lg * 8);
            gf[u][ks] = *reinterpret_cast<const bf16x8*>(grow + ks * 32 + lg * 8);
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(orow + ks * 32 + lg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += (float)gf[u][ks][e] * (float)of[e];
        }
        dl[u] = quad_sum(acc);
        nl2[u] = -lse[(long long)bh * L + qc] * LOG2E;
        const int q = q0 + u * 16 + li;
        if (active && q < Lq && lg == 0) delta[(long long)bh * L + q] = dl[u];
    }
    f32x4 dq[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nkt = (L + LT - 1) / LT;
    Stage2 st;
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
                if (k0 >= L) break;
                bf16x8 ka[2], kb[2], va[2], vb[2], kt[4];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    ka[ks] = frag_row<64>(Kimg, half * 32, ks, li, lg);
                    kb[ks] = frag_row<64>(Kimg, half * 32 + 16, ks, li, lg);
                    va[ks] = frag_row<64>(Vimg, half * 32, ks, li, lg);
                    vb[ks] = frag_row<64>(Vimg, half * 32 + 16, ks, li, lg);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) kt[dt] = frag_tr<64>(Kimg, half * 32, dt * 16, li, lg);
                const bool edge = k0 + 32 > L;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        s0 = sc_mfma16(ka[ks], qf[u][ks], s0);
                        s1 = sc_mfma16(kb[ks], qf[u][ks], s1);
                        p0 = sc_mfma16(va[ks], gf[u][ks], p0);
                        p1 = sc_mfma16(vb[ks], gf[u][ks], p1);
                    }
                    f32x4 e0 = exp2_affine(s0, c2, nl2[u]), e1 = exp2_affine(s1, c2, nl2[u]);
                    if (edge) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ka_ = k0 + 4 * lg + r, kb_ = ka_ + 16;
                            if (ka_ >= L) e0[r] = 0.f;
                            if (kb_ >= L) e1[r] = 0.f;
                        }
                    }
                    const bf16x8 dsf = pack8(e0 * (p0 - dl[u]), e1 * (p1 - dl[u]));
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) dq[u][dt] = sc_mfma16(kt[dt], dsf, dq[u][dt]);
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
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<u32x2*>(drow + dt * 16 + lg * 4) =
                sc_pack4(dq[u][dt][0] * sc, dq[u][dt][1] * sc, dq[u][dt][2] * sc, dq[u][dt][3] * sc);
    }
}

// ---------------------------------------------------------------------------------------------- backward: dK, dV
// 252 VGPRs: two waves per SIMD (without the bound: 268 registers, one wave)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dkv_long_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dqkv, int L, int Lq, int H, float scale) {
    constexpr int BUF = 2 * IMG + 2 * LT * 4;                           // Q image | dO image | -lse*log2e | delta
    __shared__ __attribute__((aligned(16))) char smem[2][BUF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int nkb = (L + LB - 1) / LB;
    const int blk = xcd_block();
    const int bh = blk / nkb, kblk = blk % nkb;
    const int b = bh / H, h = bh % H;
    const int d = H * 64;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * 64;
    const bf16* gbase = dout + (long long)b * L * d + h * 64;
    const float* lrow = lse + (long long)bh * L;
    const float* drow_ = delta + (long long)bh * L;
    const int k0w = kblk * LB + wave * 32;                              // this wave's first key
    const bool active = k0w < L;
    const float c2 = scale * LOG2E;

    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int kc = min(k0w + u * 16 + li, L - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[u][ks] = *reinterpret_cast<const bf16x8*>(base + d + (long long)kc * rs + ks * 32 + lg * 8);
            vf[u][ks] = *reinterpret_cast<const bf16x8*>(base + 2 * d + (long long)kc * rs + ks * 32 + lg * 8);
        }
    }
    f32x4 dk[2][4], dv[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dk[u][dt] = dv[u][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nqt = (Lq + LT - 1) / LT;
    Stage2 st;
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
    load_rows(0);
    store_rows(smem[0]);
    __syncthreads();
    const bool kedge = k0w + 32 > L;
    for (int j = 0; j < nqt; ++j) {
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
                bf16x8 qa[2], qb[2], ga[2], gb[2], gt[4], qt[4];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    qa[ks] = frag_row<64>(Qimg, half * 32, ks, li, lg);
                    qb[ks] = frag_row<64>(Qimg, half * 32 + 16, ks, li, lg);
                    ga[ks] = frag_row<64>(Gimg, half * 32, ks, li, lg);
                    gb[ks] = frag_row<64>(Gimg, half * 32 + 16, ks, li, lg);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    gt[dt] = frag_tr<64>(Gimg, half * 32, dt * 16, li, lg);
                    qt[dt] = frag_tr<64>(Qimg, half * 32, dt * 16, li, lg);
                }
                f32x4 la, lb, da, db;                                   // row constants of queries 4g+r and 16+4g+r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    la[r] = slse[half * 32 + 4 * lg + r];
                    lb[r] = slse[half * 32 + 16 + 4 * lg + r];
                    da[r] = sdel[half * 32 + 4 * lg + r];
                    db[r] = sdel[half * 32 + 16 + 4 * lg + r];
                }
                const bool edge = qb0 + 32 > Lq || kedge;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int key = k0w + u * 16 + li;
                    f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        s0 = sc_mfma16(qa[ks], kf[u][ks], s0);
                        s1 = sc_mfma16(qb[ks], kf[u][ks], s1);
                        p0 = sc_mfma16(ga[ks], vf[u][ks], p0);
                        p1 = sc_mfma16(gb[ks], vf[u][ks], p1);
                    }
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
                            if (qa_ >= Lq || key >= L) e0[r] = 0.f;
                            if (qb_ >= Lq || key >= L) e1[r] = 0.f;
                        }
                    }
                    const bf16x8 pf = pack8(e0, e1), dsf = pack8(e0 * (p0 - da), e1 * (p1 - db));
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        dv[u][dt] = sc_mfma16(gt[dt], pf, dv[u][dt]);
                        dk[u][dt] = sc_mfma16(qt[dt], dsf, dk[u][dt]);
                    }
                }
            }
        }
        if (more) store_rows(smem[(j + 1) & 1]);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int key = k0w + u * 16 + li;
        if (key >= L) continue;
        bf16* drow = dqkv + ((long long)b * L + key) * rs + h * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            *reinterpret_cast<u32x2*>(drow + d + dt * 16 + lg * 4) =
                sc_pack4(dk[u][dt][0] * scale, dk[u][dt][1] * scale, dk[u][dt][2] * scale, dk[u][dt][3] * scale);
            *reinterpret_cast<u32x2*>(drow + 2 * d + dt * 16 + lg * 4) =
                sc_pack4(dv[u][dt][0], dv[u][dt][1], dv[u][dt][2], dv[u][dt][3]);
        }
    }
}

}  // namespace

int sc_attn_fwd_long(const void* qkv, void* out, float* lse, int B, int L, int Lq, int H, int dh, int causal,
                     hipStream_t st) {
    if (dh != 64 || causal || B <= 0 || H <= 0 || L <= 0 || Lq <= 0 || Lq > L) return 0;
    const long long grid = (long long)B * H * ((Lq + LB - 1) / LB);
    if (grid > 0x7fffffffLL) return 0;
    attn_fwd_long_kernel<<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (bf16*)out, lse, L, Lq, H, 0.125f);
    return 1;
}

int sc_attn_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                     int B, int L, int Lq, int H, int dh, int causal, hipStream_t st) {
    if (dh != 64 || causal || B <= 0 || H <= 0 || L <= 0 || Lq <= 0 || Lq > L) return 0;
    const long long grid = (long long)B * H * ((L + LB - 1) / LB);
    if (grid > 0x7fffffffLL) return 0;
    attn_bwd_dq_long_kernel<<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (const bf16*)out, (const bf16*)dout, lse,
                                                            delta, (bf16*)dqkv, L, Lq, H, 0.125f);
    attn_bwd_dkv_long_kernel<<<(unsigned)grid, 256, 0, st>>>((const bf16*)qkv, (const bf16*)dout, lse, delta, (bf16*)dqkv,
                                                             L, Lq, H, 0.125f);
    return 1;
}
