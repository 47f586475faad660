// bf16 MFMA GEMM for gfx950 with fused epilogues.  Two operand layouts:
//   NT : C[M,N] = A[M,K] . B[N,K]^T      (both operands K-contiguous: forward linears and dgrads,
//                                          the latter against a transposed bf16 weight copy)
//   TN : C[M,N] = At[K,M]^T . Bt[K,N]     (both operands reduction-major: weight gradients
//                                          dW = dY^T X straight from the row-major activations,
//                                          fragments fetched with ds_read_b64_tr_b16)
// 128x128x64 block tile, 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 tiles, fp32 accumulate.
// Register-staged double buffering (global -> VGPR -> swizzled LDS), one barrier per K tile.
// Edge handling: buffer loads return 0 beyond the operand (outer dims), stores are guarded.
// The accumulators are produced "swapped" (D = B.A^T) so that every lane owns 4 consecutive columns
// of C; they are then bounced through LDS once so that global stores / residual loads are full
// 128..256-byte row segments.
#include "sc_gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * 64 * 2;          // 16 KiB per operand tile
constexpr int EPI_LD = SC_EPI_LD;
constexpr int LDS_BYTES = 4 * 64 * EPI_LD * 4;     // 69632 >= 4 * TILE_BYTES

template <int MODE, bool KTAIL>
SC_DEVICE void stage_load(u32x4 (&ra)[4], u32x4 (&rb)[4], __amdgpu_buffer_rsrc_t rsA, __amdgpu_buffer_rsrc_t rsB,
                          int lda, int ldb, int k0, int t, int kend) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int c = p * 256 + t;
        if (MODE == SC_GEMM_NT) {
            const int row = c >> 3, kc = c & 7;
            ra[p] = sc_buf_load16(rsA, (uint32_t)(row * lda + k0 + kc * 8) * 2u);
            rb[p] = sc_buf_load16(rsB, (uint32_t)(row * ldb + k0 + kc * 8) * 2u);
            if (KTAIL && k0 + kc * 8 >= kend) {   // K not a multiple of 64: zero the chunks past the row end
                ra[p] = (u32x4){0u, 0u, 0u, 0u};
                rb[p] = (u32x4){0u, 0u, 0u, 0u};
            }
        } else {
            const int krow = c >> 4, mc = c & 15;
            ra[p] = sc_buf_load16(rsA, (uint32_t)((k0 + krow) * lda + mc * 8) * 2u);
            rb[p] = sc_buf_load16(rsB, (uint32_t)((k0 + krow) * ldb + mc * 8) * 2u);
        }
    }
}

template <int MODE>
SC_DEVICE void stage_store(const u32x4 (&ra)[4], const u32x4 (&rb)[4], char* sA, char* sB, int t) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int c = p * 256 + t;
        int off;
        if (MODE == SC_GEMM_NT) {
            const int row = c >> 3, kc = c & 7;
            off = row * 128 + ((kc ^ ((row >> 1) & 7)) << 4);
        } else {
            const int krow = c >> 4, mc = c & 15;
            const int s = (krow & 3) | (((krow >> 3) & 1) << 2);
            off = krow * 256 + ((((mc >> 1) ^ s)) << 5) + ((mc & 1) << 4);
        }
        *reinterpret_cast<u32x4*>(sA + off) = ra[p];
        *reinterpret_cast<u32x4*>(sB + off) = rb[p];
    }
}

template <int MODE, int EPI, bool KTAIL>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 15, lg = lane >> 4;

    int idx = sc_xcd_remap(blockIdx.x, gridDim.x);
    const int tn = idx % g.ntn;
    idx /= g.ntn;
    const int tm = idx % g.ntm;
    const int z = idx / g.ntm;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = z * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nt = (kend - kbeg + BK - 1) / BK;

    __amdgpu_buffer_rsrc_t rsA, rsB;
    if (MODE == SC_GEMM_NT) {
        rsA = sc_make_rsrc(g.A + (size_t)m0 * g.lda, sc_clamp_bytes((uint64_t)max(g.M - m0, 0) * g.lda * 2));
        rsB = sc_make_rsrc(g.B + (size_t)n0 * g.ldb, sc_clamp_bytes((uint64_t)max(g.N - n0, 0) * g.ldb * 2));
    } else {
        // base at (kbeg, m0); everything past the last reduction row is out of range -> 0
        rsA = sc_make_rsrc(g.A + (size_t)kbeg * g.lda + m0,
                           sc_clamp_bytes(((uint64_t)(g.K - kbeg) * g.lda - m0) * 2));
        rsB = sc_make_rsrc(g.B + (size_t)kbeg * g.ldb + n0,
                           sc_clamp_bytes(((uint64_t)(g.K - kbeg) * g.ldb - n0) * 2));
    }
    const int kb = (MODE == SC_GEMM_NT) ? kbeg : 0;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 ra[4], rb[4];
    if (nt > 0) {
        stage_load<MODE, KTAIL>(ra, rb, rsA, rsB, g.lda, g.ldb, kb, t, kend);
        stage_store<MODE>(ra, rb, smem, smem + TILE_BYTES, t);
    }
    __syncthreads();

    for (int it = 0; it < nt; ++it) {
        const int cur = it & 1;
        char* sA = smem + cur * 2 * TILE_BYTES;
        char* sB = sA + TILE_BYTES;
        const bool more = (it + 1 < nt);
        if (more) stage_load<MODE, KTAIL>(ra, rb, rsA, rsB, g.lda, g.ldb, kb + (it + 1) * BK, t, kend);

#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[4], bfr[4];
            if (MODE == SC_GEMM_NT) {
                const int sw = (li >> 1) & 7;
                const int coff = ((kk * 4 + lg) ^ sw) << 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rowa = wm * 64 + i * 16 + li;
                    const int rowb = wn * 64 + i * 16 + li;
                    af[i] = *reinterpret_cast<const bf16x8*>(sA + rowa * 128 + coff);
                    bfr[i] = *reinterpret_cast<const bf16x8*>(sB + rowb * 128 + coff);
                }
            } else {
                const int q = li >> 2, p = li & 3;
                const int krow = kk * 32 + lg * 8 + q;
                const int s = q | ((lg & 1) << 2);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ca = ((wm * 4 + i) ^ s) << 5;
                    const int cb = ((wn * 4 + i) ^ s) << 5;
                    const char* pa = sA + krow * 256 + ca + p * 8;
                    const char* pb = sB + krow * 256 + cb + p * 8;
                    af[i] = sc_cat(sc_lds_tr16(pa), sc_lds_tr16(pa + 4 * 256));
                    bfr[i] = sc_cat(sc_lds_tr16(pb), sc_lds_tr16(pb + 4 * 256));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = sc_mfma16(bfr[j], af[i], acc[i][j]);
        }
        if (more) {
            char* nA = smem + (cur ^ 1) * 2 * TILE_BYTES;
            stage_store<MODE>(ra, rb, nA, nA + TILE_BYTES, t);
        }
        __syncthreads();
    }

    // ---------------- epilogue: bounce the wave's 64x64 tile through LDS ----------------
    EpiRegs<EPI> er;
    sc_epi_load<EPI>(er, m0 + wm * 64, n0 + wn * 64, lane, g);
    float* ep = reinterpret_cast<float*>(smem) + wave * 64 * EPI_LD;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(ep + (i * 16 + li) * EPI_LD + j * 16 + lg * 4) = acc[i][j];
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): a wave only reads back its own region
    __builtin_amdgcn_wave_barrier();

    sc_epilogue_store<EPI>(ep, er, m0 + wm * 64, n0 + wn * 64, lane, g, z);
}

// Blocks [b of nb] sum the split-K slabs of one output into it, and its partial column sums (the fused bias gradient:
// [nslab][cs_n] -> [cs_n]); each in the order z = 0 .. nslab - 1
SC_DEVICE void reduce_slabs_body(long long b, long long nb, float* __restrict__ out, const float* __restrict__ slabs, int nslab,
                                 long long slab_stride, long long n4, float* __restrict__ cs_out,
                                 const float* __restrict__ cs_part, int cs_n) {
    if (slabs != nullptr) {
        for (long long i = b * blockDim.x + threadIdx.x; i < n4; i += nb * blockDim.x) {
            f32x4 s = reinterpret_cast<const f32x4*>(slabs)[i];
            for (int z = 1; z < nslab; ++z) s += reinterpret_cast<const f32x4*>(slabs + z * slab_stride)[i];
            reinterpret_cast<f32x4*>(out)[i] = s;
        }
    }
    if (cs_out != nullptr) {
        for (long long i = b * blockDim.x + threadIdx.x; i < cs_n; i += nb * blockDim.x) {
            float s = 0.f;
            for (int z = 0; z < nslab; ++z) s += cs_part[(long long)z * cs_n + i];
            cs_out[i] = s;
        }
    }
}

SC_DEVICE void reduce_slabs_one(long long b, long long nb, const ReduceOne& o, int nslab) {
    const long long mn = (long long)o.M * o.N;
    reduce_slabs_body(b, nb, o.out, o.slabs, nslab, mn, mn / 4, o.cs_out, o.cs_part, o.M);
}
__global__ void reduce_slabs_kernel(const ReduceOne o, int nslab) { reduce_slabs_one(blockIdx.x, gridDim.x, o, nslab); }

// reduce_slabs_kernel for several outputs in one launch: output p owns blocks [first[p], first[p + 1])
struct ReduceGroup {
    ReduceOne one[SC_WGRAD_GROUP_MAX];
    int first[SC_WGRAD_GROUP_MAX + 1];
    int n, nslab;
};
__global__ void reduce_slabs_group_kernel(const ReduceGroup r) {
    int p = 0;
    while (p + 1 < r.n && (int)blockIdx.x >= r.first[p + 1]) ++p;
    reduce_slabs_one(blockIdx.x - r.first[p], r.first[p + 1] - r.first[p], r.one[p], r.nslab);
}

// 256 threads per four floats, at most `cap` blocks; with column sums to reduce, at least one thread per column
int reduce_blocks(long long n4, int cap, int cs_n) {
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > cap) blocks = cap;
    if (blocks < (cs_n + 255) / 256) blocks = (cs_n + 255) / 256;
    return blocks;
}

template <int MODE, int EPI, bool KTAIL>
int launch1(const GemmArgs& g, int nblocks, hipStream_t st) {
    static_assert(LDS_BYTES == SC_GEMM128_LDS, "the planner's LDS figure");
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<MODE, EPI, KTAIL>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        attr_done = true;
    }
    gemm_kernel<MODE, EPI, KTAIL><<<nblocks, 256, LDS_BYTES, st>>>(g);
    SC_LAUNCH_CHECK();
    return 0;
}
template <int MODE, int EPI>
int launch(const GemmArgs& g, int nblocks, hipStream_t st) {
    if (MODE == SC_GEMM_NT && (g.K % BK) != 0) return launch1<MODE, EPI, true>(g, nblocks, st);
    return launch1<MODE, EPI, false>(g, nblocks, st);
}

}  // namespace

int sc_gemm128_launch(int mode, int epi, const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
    return sc_mode_epi_dispatch<SC_EPI_F32, SC_EPI_BF16>(
        mode, epi, [&](auto MODE, auto EPI) { return launch<decltype(MODE)::value, decltype(EPI)::value>(g, p.grid, st); });
}

int sc_reduce_slabs_launch(const ReduceOne& o, int nslab, hipStream_t st) {
    const int blocks = reduce_blocks((long long)o.M * o.N / 4, 2048, o.cs_part ? o.M : 0);
    reduce_slabs_kernel<<<blocks, 256, 0, st>>>(o, nslab);
    SC_LAUNCH_CHECK();
    return 0;
}

int sc_reduce_slabs_group_launch(const ReduceOne* o, int n, int nslab, hipStream_t st) {
    ReduceGroup r{};
    r.n = n; r.nslab = nslab;
    int total = 0;
    for (int p = 0; p <= SC_WGRAD_GROUP_MAX; ++p) {
        r.first[p] = total;
        if (p < n) { r.one[p] = o[p]; total += reduce_blocks((long long)o[p].M * o[p].N / 4, 1024, 0); }
    }
    reduce_slabs_group_kernel<<<total, 256, 0, st>>>(r);
    SC_LAUNCH_CHECK();
    return 0;
}
