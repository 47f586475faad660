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

// one wave per 16-row tile, all tiles of a head in flight at once when they fit (13 waves at L=197): balanced work
// max_waves: 13 for forward (68 VGPRs -> 7 waves/SIMD, two 13-wave workgroups per CU so that one workgroup's K/V load
// overlaps the other's compute); 7 for backward (114-120 VGPRs -> 4 waves/SIMD: two 7-wave workgroups per CU)
int attn_threads(int L, int max_waves) {
    const int tiles = (L + 15) / 16;
    const int rounds = (tiles + max_waves - 1) / max_waves;
    return ((tiles + rounds - 1) / rounds) * 64;
}

// ---------------------------------------------------------------------------------------------- the paths of this file
// One workgroup per head: `images` LDS images of Lp = L rounded up to 32 rows and `vectors` fp32 row vectors.  The fused
// backward holds Q, K, V and dO of a head (L <= 288 at dh = 64, every L <= MAXL at dh = 32); beyond that the dq + dkv pair.
size_t per_head_lds(const AttnShape& s, int images, int vectors) {
    const int Lp = (s.L + 31) & ~31;
    return (size_t)images * Lp * s.dh * 2 + (size_t)vectors * Lp * 4;
}
bool per_head_accepts(const AttnShape& s) { return (s.dh == 64 || s.dh == 32) && s.L <= MAXL; }
bool bwd_fused_accepts(const AttnShape& s) { return per_head_accepts(s) && per_head_lds(s, 4, 2) <= ATTN_LDS_MAX; }

template <class F>
void per_head_instance(const AttnShape& s, F&& f) {
    attn_dispatch(attn_vals<32, 64>{}, s.dh, attn_vals<1, 0>{}, s.causal != 0, f);
}

int fwd_per_head_launch(const AttnShape& s, const AttnFwdOps& o, hipStream_t st) {
    per_head_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_fwd_kernel<DH.value, C.value != 0>, s.nheads(), attn_threads(s.L, 13), per_head_lds(s, 2, 0), st, o.qkv,
                    o.out, o.lse, s.L, s.Lq, s.H, s.scale());
    });
    return 0;
}

int bwd_fused_launch(const AttnShape& s, const AttnBwdOps& o, hipStream_t st) {
    per_head_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_bwd_fused_kernel<DH.value, C.value != 0>, s.nheads(), attn_threads(s.L, 13), per_head_lds(s, 4, 2), st,
                    o.qkv, o.out, o.dout, o.lse, o.delta, o.dqkv, s.L, s.Lq, s.H, s.scale());
    });
    return 0;
}

int bwd_dq_dkv_launch(const AttnShape& s, const AttnBwdOps& o, hipStream_t st) {
    const int threads = attn_threads(s.L, 7);
    per_head_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_bwd_dq_kernel<DH.value, C.value != 0>, s.nheads(), threads, per_head_lds(s, 2, 0), st, o.qkv, o.out,
                    o.dout, o.lse, o.delta, o.dqkv, s.L, s.Lq, s.H, s.scale());
    });
    SC_LAUNCH_CHECK();
    per_head_instance(s, [&](auto DH, auto C) {
        attn_launch(attn_bwd_dkv_kernel<DH.value, C.value != 0>, s.nheads(), threads, per_head_lds(s, 2, 2), st, o.qkv, o.dout,
                    o.lse, o.delta, o.dqkv, s.L, s.Lq, s.H, s.scale());
    });
    return 0;
}

// The streamed kernels of sc_attention_stream.hip are the only path at head dim 80 and above MAXL tokens; SC_ATTN_LONG=1
// sends them the rest of their range too (head dim 64, non-causal, any L: A/B runs and tests).
bool stream_only(const AttnShape& s) { return s.dh == 80 || s.L > MAXL; }
bool fwd_stream_only(const AttnShape& s) { return stream_only(s) && sc_attn_fwd_stream_accepts(s); }
bool bwd_stream_only(const AttnShape& s) { return stream_only(s) && sc_attn_bwd_stream_accepts(s); }

// ---------------------------------------------------------------------------------------------- the path tables
// Which kernel runs for a shape: the first entry, in table order, whose switches are on and whose predicate accepts it.
// A switch is an environment variable read per call (tests select a path): opt-out ones are on unless set to 0, the opt-in
// one is on when set to 1.
struct AttnSwitch {
    const char* name;
    bool opt_in;
};
template <class Ops>
struct AttnPath {
    int id;                                   // enum sc_attn_path
    AttnSwitch sw[2];
    bool (*accepts)(const AttnShape&);
    int (*launch)(const AttnShape&, const Ops&, hipStream_t);
};

const AttnPath<AttnFwdOps> attn_fwd_paths[] = {
    {SC_ATTN_FWD_STREAM, {}, fwd_stream_only, sc_attn_fwd_stream_launch},
    {SC_ATTN_FWD_STREAM, {{"SC_ATTN_LONG", true}}, sc_attn_fwd_stream_accepts, sc_attn_fwd_stream_launch},
    {SC_ATTN_FWD_PERSISTENT, {{"SC_ATTN_PERSIST"}}, sc_attn_fwd_persistent_accepts, sc_attn_fwd_persistent_launch},
    {SC_ATTN_FWD_PERSISTENT2, {{"SC_ATTN_PERSIST"}, {"SC_ATTN_PERSIST2"}}, sc_attn_fwd_persistent2_accepts,
     sc_attn_fwd_persistent2_launch},
    {SC_ATTN_FWD_PER_HEAD, {}, per_head_accepts, fwd_per_head_launch},
};

// the per-layer times behind this order (ViT-B/16, 197 tokens): ring 180-183 us, single pass 232-256 us, persistent two-pass
// (also causal) 254 us, one workgroup per head 268-296 us
const AttnPath<AttnBwdOps> attn_bwd_paths[] = {
    {SC_ATTN_BWD_CLS, {}, sc_attn_bwd_cls_accepts, sc_attn_bwd_cls_launch},
    {SC_ATTN_BWD_STREAM, {}, bwd_stream_only, sc_attn_bwd_stream_launch},
    {SC_ATTN_BWD_STREAM, {{"SC_ATTN_LONG", true}}, sc_attn_bwd_stream_accepts, sc_attn_bwd_stream_launch},
    {SC_ATTN_BWD_RING, {{"SC_ATTN_BWD3"}}, sc_attn_bwd_ring_accepts, sc_attn_bwd_ring_launch},
    {SC_ATTN_BWD_RING8, {{"SC_ATTN_BWD4"}}, sc_attn_bwd_ring8_accepts, sc_attn_bwd_ring8_launch},
    {SC_ATTN_BWD_SINGLE_PASS, {{"SC_ATTN_BWD1"}}, sc_attn_bwd_single_pass_accepts, sc_attn_bwd_single_pass_launch},
    {SC_ATTN_BWD_PERSISTENT, {{"SC_ATTN_BWD2"}}, sc_attn_bwd_persistent_accepts, sc_attn_bwd_persistent_launch},
    {SC_ATTN_BWD_FUSED, {{"SC_ATTN_FUSED"}}, bwd_fused_accepts, bwd_fused_launch},
    {SC_ATTN_BWD_DQ_DKV, {}, per_head_accepts, bwd_dq_dkv_launch},
};

bool attn_switch_on(const AttnSwitch& w) {
    const char* e = w.name ? getenv(w.name) : nullptr;
    return w.opt_in ? (e && e[0] == '1') : !(e && e[0] == '0');
}

// the chosen entry, or nullptr: a streamed shape whose grid does not fit (every other valid shape has a per-head kernel)
template <class Ops, size_t N>
const AttnPath<Ops>* attn_plan(const AttnPath<Ops> (&table)[N], const AttnShape& s) {
    for (const AttnPath<Ops>& e : table)
        if (e.accepts(s) && attn_switch_on(e.sw[0]) && attn_switch_on(e.sw[1])) return &e;
    return nullptr;
}
const AttnPath<AttnFwdOps>* attn_plan_fwd(const AttnShape& s) { return attn_plan(attn_fwd_paths, s); }
const AttnPath<AttnBwdOps>* attn_plan_bwd(const AttnShape& s) { return attn_plan(attn_bwd_paths, s); }

// ---------------------------------------------------------------------------------------------- validation
int attn_validate(const char* who, int B, int L, int H, int dh, int causal) {
    SC_CHECK(L <= MAXL || (dh == 64 && !causal),
             "%s: above %d tokens only non-causal attention with head dim 64 is supported; head dims 32 / 64 / 80, causal or "
             "not, up to %d tokens (L=%d, dh=%d, causal=%d)", who, MAXL, MAXL, L, dh, causal);
    SC_CHECK(B > 0 && H > 0 && L > 0, "%s: need 0 < L <= %d (L=%d), B=%d H=%d", who, MAXL, L, B, H);
    SC_CHECK(dh == 64 || dh == 32 || dh == 80, "%s: head dim must be 32, 64 or 80 (got %d)", who, dh);
    return 0;
}

// a launch on a null operand would fault the device: refused before anything is enqueued
int attn_check_ptrs(const char* who, bool ok, int L) {
    SC_CHECK(ok, "%s: null operand pointer (supported: 0 < L <= %d with dh 32 / 64 / 80, causal or not; any L with dh 64, "
                 "non-causal; got L=%d)", who, MAXL, L);
    return 0;
}

AttnShape attn_shape(int B, int L, int H, int dh, int causal, int q_rows) {
    return {B, L, (q_rows > 0 && q_rows < L) ? q_rows : L, H, dh, causal};
}

// the kernel the last call of each direction dispatched to (enum sc_attn_path)
int attn_last_fwd = SC_ATTN_PATH_NONE, attn_last_bwd = SC_ATTN_PATH_NONE;

}  // namespace

// ---------------------------------------------------------------------------------------------- shared launch helpers
static int attn_cu_count() {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
        ncu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    }
    return ncu;
}

int attn_persistent_grid(int nheads) {
    const int ncu = attn_cu_count();
    if (!ncu) sc_set_error("attention: the device's compute-unit count cannot be read (the device query failed)");
    return nheads < ncu ? nheads : ncu;
}

int attn_grid_cap(int grid) {
    const char* e = getenv("SC_ATTN_GRID");
    const int cap = e ? atoi(e) : 0;
    return cap > 0 && cap < grid ? cap : grid;
}

// ---------------------------------------------------------------------------------------------- the C ABI
extern "C" int sc_debug_attn_last_path(int* fwd, int* bwd) {
    if (fwd) *fwd = attn_last_fwd;
    if (bwd) *bwd = attn_last_bwd;
    return 0;
}

// the paths the next sc_attn_fwd / sc_attn_bwd of this shape would take under the current environment; no HIP call
extern "C" int sc_debug_attn_plan(int B, int L, int H, int dh, int causal, int q_rows, int* fwd, int* bwd) {
    if (attn_validate("sc_attn_fwd", B, L, H, dh, causal)) return -1;
    const AttnShape s = attn_shape(B, L, H, dh, causal, q_rows);
    const AttnPath<AttnFwdOps>* f = attn_plan_fwd(s);
    SC_CHECK(f, "sc_attn_fwd: grid too large (B=%d L=%d H=%d)", B, L, H);
    const AttnPath<AttnBwdOps>* b = attn_plan_bwd(s);
    SC_CHECK(b, "sc_attn_bwd: grid too large (B=%d L=%d H=%d)", B, L, H);
    if (fwd) *fwd = f->id;
    if (bwd) *bwd = b->id;
    return 0;
}

extern "C" int sc_attn_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dh, int causal,
                           int q_rows, void* stream) {
    if (attn_validate("sc_attn_fwd", B, L, H, dh, causal)) return -1;
    if (attn_check_ptrs("sc_attn_fwd", qkv && out && lse, L)) return -1;
    const AttnShape s = attn_shape(B, L, H, dh, causal, q_rows);
    const AttnPath<AttnFwdOps>* e = attn_plan_fwd(s);
    SC_CHECK(e, "sc_attn_fwd: grid too large (B=%d L=%d H=%d)", B, L, H);
    if (const int rc = e->launch(s, {(const bf16*)qkv, (bf16*)out, lse}, (hipStream_t)stream)) return rc;
    SC_LAUNCH_CHECK();
    attn_last_fwd = e->id;
    return 0;
}

extern "C" int sc_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                           void* dqkv, int B, int L, int H, int dh, int causal, int q_rows, void* stream) {
    if (attn_validate("sc_attn_bwd", B, L, H, dh, causal)) return -1;
    if (attn_check_ptrs("sc_attn_bwd", qkv && out && dout && lse && delta && dqkv, L)) return -1;
    const AttnShape s = attn_shape(B, L, H, dh, causal, q_rows);
    const AttnPath<AttnBwdOps>* e = attn_plan_bwd(s);
    SC_CHECK(e, "sc_attn_bwd: grid too large (B=%d L=%d H=%d)", B, L, H);
    const AttnBwdOps o{(const bf16*)qkv, (const bf16*)out, (const bf16*)dout, lse, delta, (bf16*)dqkv};
    if (const int rc = e->launch(s, o, (hipStream_t)stream)) return rc;
    SC_LAUNCH_CHECK();
    attn_last_bwd = e->id;
    return 0;
}
