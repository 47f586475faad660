// Multi-head self-attention for short sequences (L <= 320: ViT 197/257 tokens, CLIP text 77) on gfx950; longer ones go to
// sc_attention_stream.hip, head dim 80 too (see sc_attn_fwd / sc_attn_bwd at the end).
// One workgroup (4 waves) owns one (batch, head).  The whole K and V of that head sit in LDS (<= 80 KiB at
// L=320, dh=64) in ONE swizzled image each that serves both row reads (ds_read_b128) and transposed reads
// (ds_read_b64_tr_b16), so there is no multi-block online softmax and no [L,L] matrix in HBM.
//
// All products keep the query on the MFMA *column* (lane & 15), i.e. they are computed transposed:
//   S^T[key][q]  = K . Q^T          (A = K rows from LDS,   B = Q rows from registers)
//   O^T[d][q]    = V^T . P^T        (A = V by tr-read,       B = P^T = the S^T accumulators, in place)
// so the softmax statistics of a query live in the same lanes as its accumulators (no cross-lane moves
// except a 4-lane max/sum), and the probabilities feed the second MFMA without touching LDS.
// k-slot convention for "accumulator as operand": for a 32-key block, element j of lane group g is
// key 4g+j (j<4) or 16+4g+(j-4) (j>=4) -- both operands use the same order.
//
// Backward = two kernels with the same structure:
//   dq kernel : per query tile, loop key blocks : S^T, dP^T = V.dO^T, dS^T, dQ^T += K^T . dS^T  (+ delta)
//   dkv kernel: per key tile,   loop query blocks: S = Q.K^T, dP = dO.V^T, dV^T += dO^T.P, dK^T += Q^T.dS
// Reference semantics: nn.MultiheadAttention via src/open_clip/transformer.py:253,272-287 (scale 1/sqrt(dh)
// on q.k, fp32 softmax, optional additive causal mask :1080-1086).
#include "sc_attn_common.h"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------------------------------------- forward
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(7, 8))) void attn_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out,
                                                          float* __restrict__ lse, int L, int Lq, int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = DH / 32, DT = DH / 16;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int Lp = (L + 31) & ~31;
    char* Kimg = smem;
    char* Vimg = smem + Lp * DH * 2;
    // the first query tile's fragments travel together with the K/V images (one memory round trip, not two)
    bf16x8 qnext[KS];
    {
        const int qc0 = min(wave * 16 + li, L - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qnext[ks] = *reinterpret_cast<const bf16x8*>(base + (long long)qc0 * rs + ks * 32 + lg * 8);
    }
    load_images2<DH>(Kimg, base + d, rs, Vimg, base + 2 * d, rs, L, Lp, t);
    __syncthreads();
    const float c2 = scale * 1.4426950408889634f;  // exp(x*scale) = exp2(x*c2)
    const int nqt = (Lq + 15) >> 4;        // only the first Lq query rows are needed
    const int nwaves = blockDim.x >> 6;
    for (int qt = wave; qt < nqt; qt += nwaves) {
        const int q = qt * 16 + li;           // this lane's query (B-operand column)
        bf16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qnext[ks];
        if (qt + nwaves < nqt) {              // prefetch the next tile of this wave (L > 16 * waves only)
            const int qc1 = min((qt + nwaves) * 16 + li, L - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                qnext[ks] = *reinterpret_cast<const bf16x8*>(base + (long long)qc1 * rs + ks * 32 + lg * 8);
        }
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float m = -1e30f, lsum = 0.f;
        const int kend = CAUSAL ? min(Lp, ((qt * 16 + 15) / 32 + 1) * 32) : Lp;
        for (int k0 = 0; k0 < kend; k0 += 32) {
            f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s0 = sc_mfma16(frag_row<DH>(Kimg, k0, ks, li, lg), qf[ks], s0);
                s1 = sc_mfma16(frag_row<DH>(Kimg, k0 + 16, ks, li, lg), qf[ks], s1);
            }
            // masking is needed only where the block touches the padding (last block) or the causal diagonal
            if (k0 + 32 > L || CAUSAL) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ka = k0 + 4 * lg + r, kb = ka + 16;
                    if (ka >= L || (CAUSAL && ka > q)) s0[r] = -1e30f;
                    if (kb >= L || (CAUSAL && kb > q)) s1[r] = -1e30f;
                }
            }
            float mx = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])),
                             fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
            mx = quad_max(mx);
            const float mn = fmaxf(m, mx);
            const float nb = -mn * c2;                      // exp(scale*(s - mn)) = exp2(s*c2 + nb)
            s0 = exp2_affine(s0, c2, nb);
            s1 = exp2_affine(s1, c2, nb);
            const f32x4 pv = s0 + s1;
            const float ps = (pv[0] + pv[1]) + (pv[2] + pv[3]);
            const bf16x8 pf = pack8(s0, s1);
            if (__any(mn != m)) {                           // running max moved for some query: rescale (rare after
                const float alpha = fast_exp2((m - mn) * c2);   // the first blocks), otherwise alpha == 1 exactly
                lsum *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
            }
            m = mn;
            lsum += ps;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = sc_mfma16(frag_tr<DH>(Vimg, k0, dt * 16, li, lg), pf, o[dt]);
        }
        lsum = quad_sum(lsum);
        const float inv = 1.0f / lsum;
        if (q < Lq) {
            bf16* orow = out + ((long long)b * L + q) * d + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                *reinterpret_cast<u32x2*>(orow + dt * 16 + lg * 4) =
                    sc_pack4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
            if (lg == 0) lse[((long long)b * H + h) * L + q] = m * scale + __logf(lsum);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward: dQ (+ delta)
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(1024) void attn_bwd_dq_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ out,
                                                             const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                             float* __restrict__ delta, bf16* __restrict__ dqkv, int L,
                                                             int Lq, int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = DH / 32, DT = DH / 16;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int Lp = (L + 31) & ~31;
    char* Kimg = smem;
    char* Vimg = smem + Lp * DH * 2;
    load_images2<DH>(Kimg, base + d, rs, Vimg, base + 2 * d, rs, L, Lp, t);
    __syncthreads();
    const float c2 = scale * 1.4426950408889634f;
    const int nqt = (Lq + 15) >> 4;        // only the first Lq query rows are needed
    for (int qt = wave; qt < nqt; qt += (blockDim.x >> 6)) {
        const int q = qt * 16 + li;
        const int qc = min(q, L - 1);
        bf16x8 qf[KS], dof[KS];
        float dl = 0.f;
        const bf16* orow = out + ((long long)b * L + qc) * d + h * DH;
        const bf16* grow = dout + ((long long)b * L + qc) * d + h * DH;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8*>(base + (long long)qc * rs + ks * 32 + lg * 8);
            dof[ks] = *reinterpret_cast<const bf16x8*>(grow + ks * 32 + lg * 8);
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(orow + ks * 32 + lg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl += (float)dof[ks][e] * (float)of[e];
        }
        dl = quad_sum(dl);
        const float nl2 = -lse[((long long)b * H + h) * L + qc] * 1.4426950408889634f;
        if (q < Lq && lg == 0) delta[((long long)b * H + h) * L + q] = dl;
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int kend = CAUSAL ? min(Lp, ((qt * 16 + 15) / 32 + 1) * 32) : Lp;
        for (int k0 = 0; k0 < kend; k0 += 32) {
            f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s0 = sc_mfma16(frag_row<DH>(Kimg, k0, ks, li, lg), qf[ks], s0);
                s1 = sc_mfma16(frag_row<DH>(Kimg, k0 + 16, ks, li, lg), qf[ks], s1);
                p0 = sc_mfma16(frag_row<DH>(Vimg, k0, ks, li, lg), dof[ks], p0);
                p1 = sc_mfma16(frag_row<DH>(Vimg, k0 + 16, ks, li, lg), dof[ks], p1);
            }
            const bool edge = (k0 + 32 > L) || CAUSAL;      // masks only where the block touches padding / diagonal
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pa = fast_exp2(fmaf(s0[r], c2, nl2)), pb = fast_exp2(fmaf(s1[r], c2, nl2));
                if (edge) {
                    const int ka = k0 + 4 * lg + r, kb = ka + 16;
                    if (ka >= L || (CAUSAL && ka > q)) pa = 0.f;
                    if (kb >= L || (CAUSAL && kb > q)) pb = 0.f;
                }
                s0[r] = pa * (p0[r] - dl);
                s1[r] = pb * (p1[r] - dl);
            }
            const bf16x8 dsf = pack8(s0, s1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                dq[dt] = sc_mfma16(frag_tr<DH>(Kimg, k0, dt * 16, li, lg), dsf, dq[dt]);
        }
        if (q < Lq) {
            bf16* drow = dqkv + ((long long)b * L + q) * rs + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                *reinterpret_cast<u32x2*>(drow + dt * 16 + lg * 4) =
                    sc_pack4(dq[dt][0] * scale, dq[dt][1] * scale, dq[dt][2] * scale, dq[dt][3] * scale);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward: dK, dV
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(1024) void attn_bwd_dkv_kernel(const bf16* __restrict__ qkv,
                                                              const bf16* __restrict__ dout,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ delta, bf16* __restrict__ dqkv,
                                                              int L, int Lq, int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = DH / 32, DT = DH / 16;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int Lp = (L + 31) & ~31;
    char* Qimg = smem;
    char* Gimg = smem + Lp * DH * 2;
    float* slse = reinterpret_cast<float*>(smem + 2 * Lp * DH * 2);
    float* sdel = slse + Lp;
    load_images2<DH>(Qimg, base, rs, Gimg, dout + (long long)b * L * d + h * DH, d, L, Lp, t);
    for (int i = t; i < Lp; i += blockDim.x) {
        slse[i] = i < L ? -lse[((long long)b * H + h) * L + i] * 1.4426950408889634f : 0.f;
        sdel[i] = i < L ? delta[((long long)b * H + h) * L + i] : 0.f;
    }
    __syncthreads();
    const float c2 = scale * 1.4426950408889634f;
    const int nkt = (L + 15) >> 4;
    for (int kt = wave; kt < nkt; kt += (blockDim.x >> 6)) {
        const int key = kt * 16 + li;  // this lane's key (B-operand column)
        const int kc = min(key, L - 1);
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = *reinterpret_cast<const bf16x8*>(base + d + (long long)kc * rs + ks * 32 + lg * 8);
            vf[ks] = *reinterpret_cast<const bf16x8*>(base + 2 * d + (long long)kc * rs + ks * 32 + lg * 8);
        }
        f32x4 dk[DT], dv[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int qbeg = CAUSAL ? ((kt * 16) / 32) * 32 : 0;
        for (int q0 = qbeg; q0 < ((Lq + 31) & ~31); q0 += 32) {
            // S[q][key], dP[q][key]: rows = queries 4g+r (+16), col = key
            f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s0 = sc_mfma16(frag_row<DH>(Qimg, q0, ks, li, lg), kf[ks], s0);
                s1 = sc_mfma16(frag_row<DH>(Qimg, q0 + 16, ks, li, lg), kf[ks], s1);
                p0 = sc_mfma16(frag_row<DH>(Gimg, q0, ks, li, lg), vf[ks], p0);
                p1 = sc_mfma16(frag_row<DH>(Gimg, q0 + 16, ks, li, lg), vf[ks], p1);
            }
            f32x4 pr0, pr1;
            const bool edge = (q0 + 32 > Lq) || (kt * 16 + 16 > L) || CAUSAL;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // masked entries are forced to exact zeros (lse / delta of unused query rows may hold anything);
                // interior blocks (no padding, no diagonal) skip the comparisons
                const int qa = q0 + 4 * lg + r, qb = qa + 16;
                float pa = fast_exp2(fmaf(s0[r], c2, slse[qa])), pb = fast_exp2(fmaf(s1[r], c2, slse[qb]));
                float da = pa * (p0[r] - sdel[qa]), db = pb * (p1[r] - sdel[qb]);
                if (edge) {
                    const bool ma = (qa >= Lq || key >= L || (CAUSAL && key > qa));
                    const bool mb = (qb >= Lq || key >= L || (CAUSAL && key > qb));
                    pa = ma ? 0.f : pa; da = ma ? 0.f : da;
                    pb = mb ? 0.f : pb; db = mb ? 0.f : db;
                }
                pr0[r] = pa;
                pr1[r] = pb;
                s0[r] = da;
                s1[r] = db;
            }
            const bf16x8 pf = pack8(pr0, pr1), dsf = pack8(s0, s1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                dv[dt] = sc_mfma16(frag_tr<DH>(Gimg, q0, dt * 16, li, lg), pf, dv[dt]);
                dk[dt] = sc_mfma16(frag_tr<DH>(Qimg, q0, dt * 16, li, lg), dsf, dk[dt]);
            }
        }
        if (key < L) {
            bf16* drow = dqkv + ((long long)b * L + key) * rs + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                *reinterpret_cast<u32x2*>(drow + d + dt * 16 + lg * 4) =
                    sc_pack4(dk[dt][0] * scale, dk[dt][1] * scale, dk[dt][2] * scale, dk[dt][3] * scale);
                *reinterpret_cast<u32x2*>(drow + 2 * d + dt * 16 + lg * 4) =
                    sc_pack4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward, fused
// dQ, dK and dV of one (batch, head) in ONE workgroup: Q, K, V and dO all sit in LDS (4 x Lp x dh bf16 = 112 KiB at
// L = 197, dh = 64; one workgroup per CU), loaded once.  Pass A (wave = query tile) is the dq kernel above with its
// per-tile operands read from the LDS images and delta = rowsum(dO * O) left in LDS; pass B (wave = key tile) is the
// dkv kernel.  Against the two-kernel form this reads qkv / dO once instead of twice and needs no delta round trip
// through HBM (618 MB instead of 1.0 GB per ViT-B/16 layer at B = 256).  Same arithmetic, same results.
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(1024) void attn_bwd_fused_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ out,
                                                                const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                                float* __restrict__ delta, bf16* __restrict__ dqkv, int L,
                                                                int Lq, int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = DH / 32, DT = DH / 16;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int d = H * DH;
    const long long rs = 3LL * d;
    const bf16* base = qkv + (long long)b * L * rs + h * DH;
    const int Lp = (L + 31) & ~31;
    const int isz = Lp * DH * 2;
    char* Qimg = smem;
    char* Kimg = smem + isz;
    char* Vimg = smem + 2 * isz;
    char* Gimg = smem + 3 * isz;
    float* slse = reinterpret_cast<float*>(smem + 4 * isz);
    float* sdel = slse + Lp;
    {
        char* const imgs[4] = {Qimg, Kimg, Vimg, Gimg};
        const bf16* const srcs[4] = {base, base + d, base + 2 * d, dout + (long long)b * L * d + h * DH};
        const long long strides[4] = {rs, rs, rs, (long long)d};
        load_images4<DH>(imgs, srcs, strides, L, Lp, t);
    }
    for (int i = t; i < Lp; i += blockDim.x) {
        slse[i] = i < L ? -lse[((long long)b * H + h) * L + i] * 1.4426950408889634f : 0.f;
        sdel[i] = 0.f;
    }
    __syncthreads();
    const float c2 = scale * 1.4426950408889634f;
    // ---------------- pass A: dQ (+ delta) ----------------
    const int nqt = (Lq + 15) >> 4;
    for (int qt = wave; qt < nqt; qt += nwaves) {
        const int q = qt * 16 + li;
        const int qc = min(q, L - 1);
        bf16x8 qf[KS], dof[KS];
        float dl = 0.f;
        const bf16* orow = out + ((long long)b * L + qc) * d + h * DH;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = frag_row<DH>(Qimg, qt * 16, ks, li, lg);
            dof[ks] = frag_row<DH>(Gimg, qt * 16, ks, li, lg);
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(orow + ks * 32 + lg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl += (float)dof[ks][e] * (float)of[e];
        }
        dl = quad_sum(dl);
        const float nl2 = slse[qc];
        if (q < Lq && lg == 0) {
            sdel[q] = dl;
            delta[((long long)b * H + h) * L + q] = dl;
        }
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int kend = CAUSAL ? min(Lp, ((qt * 16 + 15) / 32 + 1) * 32) : Lp;
        for (int k0 = 0; k0 < kend; k0 += 32) {
            // all row fragments of the block in flight before the first MFMA, the transposed ones issued before the
            // VALU section: two LDS round trips per block instead of one per fragment
            bf16x8 ka[KS], kb[KS], va[KS], vb[KS], ktr[DT];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                ka[ks] = frag_row<DH>(Kimg, k0, ks, li, lg);
                kb[ks] = frag_row<DH>(Kimg, k0 + 16, ks, li, lg);
                va[ks] = frag_row<DH>(Vimg, k0, ks, li, lg);
                vb[ks] = frag_row<DH>(Vimg, k0 + 16, ks, li, lg);
            }
            f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s0 = sc_mfma16(ka[ks], qf[ks], s0);
                s1 = sc_mfma16(kb[ks], qf[ks], s1);
                p0 = sc_mfma16(va[ks], dof[ks], p0);
                p1 = sc_mfma16(vb[ks], dof[ks], p1);
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) ktr[dt] = frag_tr<DH>(Kimg, k0, dt * 16, li, lg);
            const bool edge = (k0 + 32 > L) || CAUSAL;
            f32x4 e0 = exp2_affine(s0, c2, nl2), e1 = exp2_affine(s1, c2, nl2);
            if (edge) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ka = k0 + 4 * lg + r, kb = ka + 16;
                    if (ka >= L || (CAUSAL && ka > q)) e0[r] = 0.f;
                    if (kb >= L || (CAUSAL && kb > q)) e1[r] = 0.f;
                }
            }
            s0 = e0 * (p0 - dl);
            s1 = e1 * (p1 - dl);
            const bf16x8 dsf = pack8(s0, s1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                dq[dt] = sc_mfma16(ktr[dt], dsf, dq[dt]);
        }
        if (q < Lq) {
            bf16* drow = dqkv + ((long long)b * L + q) * rs + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                *reinterpret_cast<u32x2*>(drow + dt * 16 + lg * 4) =
                    sc_pack4(dq[dt][0] * scale, dq[dt][1] * scale, dq[dt][2] * scale, dq[dt][3] * scale);
        }
    }
    __syncthreads();                                  // every query's delta is in LDS
    // ---------------- pass B: dK, dV ----------------
    const int nkt = (L + 15) >> 4;
    for (int kt = wave; kt < nkt; kt += nwaves) {
        const int key = kt * 16 + li;
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = frag_row<DH>(Kimg, kt * 16, ks, li, lg);
            vf[ks] = frag_row<DH>(Vimg, kt * 16, ks, li, lg);
        }
        f32x4 dk[DT], dv[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int qbeg = CAUSAL ? ((kt * 16) / 32) * 32 : 0;
        for (int q0 = qbeg; q0 < ((Lq + 31) & ~31); q0 += 32) {
            bf16x8 qa_[KS], qb_[KS], ga_[KS], gb_[KS], gtr[DT];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                qa_[ks] = frag_row<DH>(Qimg, q0, ks, li, lg);
                qb_[ks] = frag_row<DH>(Qimg, q0 + 16, ks, li, lg);
                ga_[ks] = frag_row<DH>(Gimg, q0, ks, li, lg);
                gb_[ks] = frag_row<DH>(Gimg, q0 + 16, ks, li, lg);
            }
            f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s0 = sc_mfma16(qa_[ks], kf[ks], s0);
                s1 = sc_mfma16(qb_[ks], kf[ks], s1);
                p0 = sc_mfma16(ga_[ks], vf[ks], p0);
                p1 = sc_mfma16(gb_[ks], vf[ks], p1);
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) gtr[dt] = frag_tr<DH>(Gimg, q0, dt * 16, li, lg);     // lands under the VALU section
            f32x4 pr0, pr1;
            const bool edge = (q0 + 32 > Lq) || (kt * 16 + 16 > L) || CAUSAL;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qa = q0 + 4 * lg + r, qb = qa + 16;
                float pa = fast_exp2(fmaf(s0[r], c2, slse[qa])), pb = fast_exp2(fmaf(s1[r], c2, slse[qb]));
                float da = pa * (p0[r] - sdel[qa]), db = pb * (p1[r] - sdel[qb]);
                if (edge) {
                    const bool ma = (qa >= Lq || key >= L || (CAUSAL && key > qa));
                    const bool mb = (qb >= Lq || key >= L || (CAUSAL && key > qb));
                    pa = ma ? 0.f : pa; da = ma ? 0.f : da;
                    pb = mb ? 0.f : pb; db = mb ? 0.f : db;
                }
                pr0[r] = pa;
                pr1[r] = pb;
                s0[r] = da;
                s1[r] = db;
            }
            const bf16x8 pf = pack8(pr0, pr1), dsf = pack8(s0, s1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                dv[dt] = sc_mfma16(gtr[dt], pf, dv[dt]);
                dk[dt] = sc_mfma16(frag_tr<DH>(Qimg, q0, dt * 16, li, lg), dsf, dk[dt]);
            }
        }
        if (key < L) {
            bf16* drow = dqkv + ((long long)b * L + key) * rs + h * DH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                *reinterpret_cast<u32x2*>(drow + d + dt * 16 + lg * 4) =
                    sc_pack4(dk[dt][0] * scale, dk[dt][1] * scale, dk[dt][2] * scale, dk[dt][3] * scale);
                *reinterpret_cast<u32x2*>(drow + 2 * d + dt * 16 + lg * 4) =
                    sc_pack4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
            }
        }
    }
}

template <typename K>
void set_lds(K kern, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

}  // namespace

#define SC_ATTN_DISPATCH(KERNEL, ...)                                                         \
    do {                                                                                      \
        if (dh == 64 && !causal) { set_lds(KERNEL<64, false>, lds); KERNEL<64, false><<<B * H, nthreads, lds, st>>>(__VA_ARGS__); } \
        else if (dh == 64 && causal) { set_lds(KERNEL<64, true>, lds); KERNEL<64, true><<<B * H, nthreads, lds, st>>>(__VA_ARGS__); } \
        else if (dh == 32 && !causal) { set_lds(KERNEL<32, false>, lds); KERNEL<32, false><<<B * H, nthreads, lds, st>>>(__VA_ARGS__); } \
        else { set_lds(KERNEL<32, true>, lds); KERNEL<32, true><<<B * H, nthreads, lds, st>>>(__VA_ARGS__); } \
    } while (0)

// one wave per 16-row tile, all tiles of a head in flight at once when they fit (13 waves at L=197): balanced work
// max_waves: 13 for forward (68 VGPRs -> 7 waves/SIMD, two 13-wave workgroups per CU so that one workgroup's K/V load
// overlaps the other's compute); 7 for backward (114-120 VGPRs -> 4 waves/SIMD: two 7-wave workgroups per CU)
static int attn_threads(int L, int max_waves) {
    const int tiles = (L + 15) / 16;
    const int rounds = (tiles + max_waves - 1) / max_waves;
    return ((tiles + rounds - 1) / rounds) * 64;
}

// the streamed kernels of sc_attention_stream.hip take the call at head dim 80 (their only path, up to MAXL tokens) and
// at head dim 64, non-causal, above MAXL tokens (the only path there) or at any L with SC_ATTN_LONG=1 (A/B runs and
// tests; read per call, off by default)
static bool attn_stream(int B, int L, int H, int dh, int causal) {
    if (B <= 0 || H <= 0 || L <= 0) return false;
    if (dh == 80) return L <= MAXL;
    if (dh != 64 || causal) return false;
    if (L > MAXL) return true;
    const char* e = getenv("SC_ATTN_LONG");
    return e && e[0] == '1';
}

static int attn_check_long(const char* who, int L, int dh, int causal) {
    SC_CHECK(L <= MAXL || (dh == 64 && !causal),
             "%s: above %d tokens only non-causal attention with head dim 64 is supported; head dims 32 / 64 / 80, causal or "
             "not, up to %d tokens (L=%d, dh=%d, causal=%d)", who, MAXL, MAXL, L, dh, causal);
    return 0;
}

// a launch on a null operand would fault the device: refused before anything is enqueued
static int attn_check_ptrs(const char* who, bool ok, int L) {
    SC_CHECK(ok, "%s: null operand pointer (supported: 0 < L <= %d with dh 32 / 64 / 80, causal or not; any L with dh 64, "
                 "non-causal; got L=%d)", who, MAXL, L);
    return 0;
}

static int attn_check(const char* who, int B, int L, int H, int dh) {
    SC_CHECK(B > 0 && H > 0 && L > 0 && L <= MAXL, "%s: need 0 < L <= %d (L=%d), B=%d H=%d", who, MAXL, L, B, H);
    SC_CHECK(dh == 64 || dh == 32 || dh == 80, "%s: head dim must be 32, 64 or 80 (got %d)", who, dh);
    return 0;
}

// the kernel the last call of each direction dispatched to (enum sc_attn_path); written at each `return 0` below
static int attn_last_fwd = SC_ATTN_PATH_NONE, attn_last_bwd = SC_ATTN_PATH_NONE;

extern "C" int sc_debug_attn_last_path(int* fwd, int* bwd) {
    if (fwd) *fwd = attn_last_fwd;
    if (bwd) *bwd = attn_last_bwd;
    return 0;
}

extern "C" int sc_attn_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dh, int causal,
                           int q_rows, void* stream) {
    const int Lq = (q_rows > 0 && q_rows < L) ? q_rows : L;
    hipStream_t st = (hipStream_t)stream;
    if (attn_stream(B, L, H, dh, causal)) {
        if (attn_check_ptrs("sc_attn_fwd", qkv && out && lse, L)) return -1;
        SC_CHECK(sc_attn_fwd_stream(qkv, out, lse, B, L, Lq, H, dh, causal, st),
                 "sc_attn_fwd: grid too large (B=%d L=%d H=%d)", B, L, H);
        SC_LAUNCH_CHECK();
        attn_last_fwd = SC_ATTN_FWD_STREAM;
        return 0;
    }
    if (attn_check_long("sc_attn_fwd", L, dh, causal)) return -1;
    if (attn_check("sc_attn_fwd", B, L, H, dh)) return -1;
    const char* pe = getenv("SC_ATTN_PERSIST");                  // read per call, like SC_ATTN_BWD1 / SC_ATTN_BWD2
    const bool persist_on = !(pe && pe[0] == '0');
    if (persist_on && sc_attn_fwd_persistent(qkv, out, lse, B, L, Lq, H, dh, causal, st)) {
        SC_LAUNCH_CHECK();
        attn_last_fwd = SC_ATTN_FWD_PERSISTENT;
        return 0;
    }
    const char* p2 = getenv("SC_ATTN_PERSIST2");                 // A/B switch of the 225..288-token persistent kernel
    if (persist_on && !(p2 && p2[0] == '0') && sc_attn_fwd_persistent2(qkv, out, lse, B, L, Lq, H, dh, causal, st)) {
        SC_LAUNCH_CHECK();
        attn_last_fwd = SC_ATTN_FWD_PERSISTENT2;
        return 0;
    }
    const int Lp = (L + 31) & ~31;
    const size_t lds = (size_t)2 * Lp * dh * 2;
    const float scale = 1.0f / sqrtf((float)dh);
    const int nthreads = attn_threads(L, 13);
    SC_ATTN_DISPATCH(attn_fwd_kernel, (const bf16*)qkv, (bf16*)out, lse, L, Lq, H, scale);
    SC_LAUNCH_CHECK();
    attn_last_fwd = SC_ATTN_FWD_PER_HEAD;
    return 0;
}

extern "C" int sc_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                           void* dqkv, int B, int L, int H, int dh, int causal, int q_rows, void* stream) {
    const int Lq = (q_rows > 0 && q_rows < L) ? q_rows : L;
    hipStream_t st = (hipStream_t)stream;
    if (attn_stream(B, L, H, dh, causal)) {
        if (attn_check_ptrs("sc_attn_bwd", qkv && out && dout && lse && delta && dqkv, L)) return -1;
        // q_rows == 1 (class-token-only last block): the rank-one kernel streams the keys at any L
        const bool cls = sc_attn_bwd_cls(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st) != 0;
        if (!cls)
            SC_CHECK(sc_attn_bwd_stream(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st),
                     "sc_attn_bwd: grid too large (B=%d L=%d H=%d)", B, L, H);
        SC_LAUNCH_CHECK();
        attn_last_bwd = cls ? SC_ATTN_BWD_CLS : SC_ATTN_BWD_STREAM;
        return 0;
    }
    if (attn_check_long("sc_attn_bwd", L, dh, causal)) return -1;
    if (attn_check("sc_attn_bwd", B, L, H, dh)) return -1;
    const int Lp = (L + 31) & ~31;
    const float scale = 1.0f / sqrtf((float)dh);
    if (sc_attn_bwd_cls(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st)) {      // q_rows == 1
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_CLS;
        return 0;
    }
    // 1) single-pass (non-causal, L <= 224): 232-256 us per ViT-B/16 layer; 2) persistent two-pass with loader waves
    // (also causal): 254 us; 3) one workgroup per head: 268-296 us.  The switches are read per call (tests select a path).
    const bool ring_on = !(getenv("SC_ATTN_BWD3") && getenv("SC_ATTN_BWD3")[0] == '0');
    if (ring_on && sc_attn_bwd_ring(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st)) {   // round 4: dS ring + MFMA-chain dQ
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_RING;
        return 0;
    }
    // round 5: 225..257 tokens (ViT-L/14): the ring design with eight key waves and no helper wave
    const bool ring8_on = !(getenv("SC_ATTN_BWD4") && getenv("SC_ATTN_BWD4")[0] == '0');
    if (ring8_on && sc_attn_bwd_ring8(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st)) {
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_RING8;
        return 0;
    }
    const bool single_on = !(getenv("SC_ATTN_BWD1") && getenv("SC_ATTN_BWD1")[0] == '0');
    if (single_on && sc_attn_bwd_single_pass(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st)) {
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_SINGLE_PASS;
        return 0;
    }
    const bool persist_on = !(getenv("SC_ATTN_BWD2") && getenv("SC_ATTN_BWD2")[0] == '0');
    if (persist_on && sc_attn_bwd_persistent(qkv, out, dout, lse, delta, dqkv, B, L, Lq, H, dh, causal, st)) {
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_PERSISTENT;
        return 0;
    }
    // fused two-pass kernel when Q, K, V and dO of a head fit LDS together (Lp = L rounded up to 32 rows: L <= 288 at
    // dh = 64, every L <= MAXL at dh = 32); beyond that the dq + dkv pair
    const bool fused_on = !(getenv("SC_ATTN_FUSED") && getenv("SC_ATTN_FUSED")[0] == '0');
    const size_t lds_fused = (size_t)4 * Lp * dh * 2 + (size_t)2 * Lp * 4;
    if (fused_on && lds_fused <= 160 * 1024) {
        const size_t lds = lds_fused;
        const int nthreads = attn_threads(L, 13);
        SC_ATTN_DISPATCH(attn_bwd_fused_kernel, (const bf16*)qkv, (const bf16*)out, (const bf16*)dout, lse, delta,
                         (bf16*)dqkv, L, Lq, H, scale);
        SC_LAUNCH_CHECK();
        attn_last_bwd = SC_ATTN_BWD_FUSED;
        return 0;
    }
    const int nthreads = attn_threads(L, 7);
    {
        const size_t lds = (size_t)2 * Lp * dh * 2;
        SC_ATTN_DISPATCH(attn_bwd_dq_kernel, (const bf16*)qkv, (const bf16*)out, (const bf16*)dout, lse, delta,
                         (bf16*)dqkv, L, Lq, H, scale);
        SC_LAUNCH_CHECK();
    }
    {
        const size_t lds = (size_t)2 * Lp * dh * 2 + (size_t)2 * Lp * 4;
        SC_ATTN_DISPATCH(attn_bwd_dkv_kernel, (const bf16*)qkv, (const bf16*)dout, lse, delta, (bf16*)dqkv, L, Lq, H,
                         scale);
        SC_LAUNCH_CHECK();
    }
    attn_last_bwd = SC_ATTN_BWD_DQ_DKV;
    return 0;
}
