// Full-set retrieval ranks (gfx950): the rank of every pair's ground truth among ALL N candidates, image->text and
// text->image, without ever storing the N x N similarity matrix.
//   reference op site: src/open_clip_train/train.py:383-400 (get_clip_metrics: N x N logits on the CPU + argsort).
//   z_ij = <image_i, text_j> (fp32, v_mfma_f32_16x16x4_f32), d_i = z_ii, rows i of the block [row0, row0 + M):
//   rank_i2t[i - row0]  = #{ j != i          : z_ij > d_i or (z_ij == d_i and j < i) }
//   cnt_t2i[j]         += #{ i in block, != j : z_ij > d_j or (z_ij == d_j and i < j) }
// (recall_kernel's tie rule: the 0-based position of the ground truth under a stable descending sort).
//
// One workgroup owns a 128-row panel of the block and walks 128-column tiles; the tile body, the LDS layout and the K
// assignment are those of sc_head_gemm.hip (k-contiguous operands, [row][32 k + 4 pad], lane group g feeds k = 4g + j to
// MFMA j of a 16-k chunk).  Operands are zero-filled past the M / N / K edge, and a product 0 * 0 added to an accumulator
// leaves it unchanged, so z_ij is ONE function of (image row i, text row j): the same bits in every tile position, on the
// 16-byte and on the guarded staging path, at every row stride.
// The diagonals come from that same function.  Beside the panel x tile product, the K loop of a column tile at n0 forms
// the eight 16 x 16 fragments (image rows n0 + 16f.., text rows n0 + 16f..) whose diagonals are d_j of the tile's columns
// (a third staged operand, 1/8 more MFMAs); a first K loop of the same body at n0 = m0 gives d_i of the panel's rows.
// Nothing but the operand panels is read and nothing but integers is written.
// Counting: the accumulators are compared in registers.  The row counts of the panel stay in LDS over the whole walk;
// the column counts of a tile are summed in LDS and leave as one integer atomic per column per tile (contiguous ints).
// The walk of a panel is split over several workgroups when there are few panels, so the row counts leave as integer
// atomics too (rank_i2t is cleared first on the same stream).  Integer adds commute: the result does not depend on the
// order of arrival.
// Non-finite diagonal: every comparison against it counts as "ranked above".  Row i then gets N - 1 from its own
// workgroups, and column j gets (rows of the block other than j) from each block, N - 1 over any partition of [0, N).
#include "sc_common.h"
#include "sc_kernels.h"

namespace {

constexpr int RT = 128;           // tile: RT rows x RT columns, 256 threads = 2 x 2 waves of 64 x 64
constexpr int RK = 32;            // K depth of an LDS tile
constexpr int RLD = RK + 4;       // LDS row stride (floats)
constexpr int RF = RT / 32;       // 16x16 fragments per wave in each direction
constexpr int RP = RT / 32;       // float4 per thread per staged operand tile

// RT rows x 32 k of a k-contiguous operand -> registers (rows >= `rows` and k >= K read as 0)
SC_DEVICE void rt_stage_load(const float* __restrict__ base, long long ld, int r0, int k0, int rows, int K, bool fast,
                             int t, f32x4 (&reg)[RP]) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
        const int idx = p * 256 + t;
        const int r = idx >> 3, k = (idx & 7) * 4;
        if (fast) {
            reg[p] = *reinterpret_cast<const f32x4*>(base + (long long)(r0 + r) * ld + (k0 + k));
        } else {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < rows) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + k + e < K) v[e] = base[(long long)(r0 + r) * ld + (k0 + k + e)];
            }
            reg[p] = v;
        }
    }
}

SC_DEVICE void rt_stage_store(float* __restrict__ lds, int t, const f32x4 (&reg)[RP]) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
        const int idx = p * 256 + t;
        *reinterpret_cast<f32x4*>(lds + (idx >> 3) * RLD + (idx & 7) * 4) = reg[p];
    }
}

SC_DEVICE bool rt_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

struct Operands {
    const float* img; long long ld_img; bool img_al;
    const float* txt; long long ld_txt; bool txt_al;
    int N, D;
};

// One K loop.  MAIN: acc = image rows [m0, m0 + RT) x text rows [n0, n0 + RT).  Always: the diagonals z_jj of
// j in [n0, n0 + RT) into dl[RT] (LDS), from image rows [n0, ..) x text rows [n0, ..) with the same fragment arithmetic.
template <bool MAIN>
SC_DEVICE void rt_tile(const Operands& P, int m0, int n0, float* As, float* Bs, float* Ds, float* dl,
                       f32x4 (&acc)[RF][RF]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * (RT / 2), wn = (wave & 1) * (RT / 2);
    const int l15 = lane & 15, g = lane >> 4;
    const int N = P.N, K = P.D;
    const bool a_fast = P.img_al && m0 + RT <= N, b_fast = P.txt_al && n0 + RT <= N, d_fast = P.img_al && n0 + RT <= N;

    f32x4 dacc[2];
    dacc[0] = dacc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (MAIN) {
#pragma unroll
        for (int i = 0; i < RF; ++i)
#pragma unroll
            for (int n = 0; n < RF; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    f32x4 ra[RP], rb[RP], rd[RP];
    const int nk = (K + RK - 1) / RK;
    {
        const bool kin = RK <= K;
        if (MAIN) rt_stage_load(P.img, P.ld_img, m0, 0, N, K, a_fast && kin, t, ra);
        rt_stage_load(P.txt, P.ld_txt, n0, 0, N, K, b_fast && kin, t, rb);
        rt_stage_load(P.img, P.ld_img, n0, 0, N, K, d_fast && kin, t, rd);
    }
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                                   // previous tile's fragment reads are done
        if (MAIN) rt_stage_store(As, t, ra);
        rt_stage_store(Bs, t, rb);
        rt_stage_store(Ds, t, rd);
        __syncthreads();
        if (kt + 1 < nk) {                                 // prefetch the next tile under this tile's MFMAs
            const int k0 = (kt + 1) * RK;
            const bool kin = k0 + RK <= K;
            if (MAIN) rt_stage_load(P.img, P.ld_img, m0, k0, N, K, a_fast && kin, t, ra);
            rt_stage_load(P.txt, P.ld_txt, n0, k0, N, K, b_fast && kin, t, rb);
            rt_stage_load(P.img, P.ld_img, n0, k0, N, K, d_fast && kin, t, rd);
        }
#pragma unroll
        for (int ks = 0; ks < RK / 16; ++ks) {
            const int ko = ks * 16 + 4 * g;
            // diagonal fragments 2 * wave, 2 * wave + 1 of the column tile
            f32x4 da[2], db[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const int r = (2 * wave + f) * 16 + l15;
                da[f] = *reinterpret_cast<const f32x4*>(Ds + r * RLD + ko);
                db[f] = *reinterpret_cast<const f32x4*>(Bs + r * RLD + ko);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int f = 0; f < 2; ++f)
                    dacc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[f][j], db[f][j], dacc[f], 0, 0, 0);
            if (MAIN) {
                f32x4 af[RF], bfr[RF];
#pragma unroll
                for (int i = 0; i < RF; ++i)
                    af[i] = *reinterpret_cast<const f32x4*>(As + (wm + i * 16 + l15) * RLD + ko);
#pragma unroll
                for (int i = 0; i < RF; ++i)
                    bfr[i] = *reinterpret_cast<const f32x4*>(Bs + (wn + i * 16 + l15) * RLD + ko);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < RF; ++i)
#pragma unroll
                        for (int n = 0; n < RF; ++n)
                            acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][j], bfr[n][j], acc[i][n], 0, 0, 0);
            }
        }
    }
    // D layout: col = lane & 15, row = (lane >> 4) * 4 + reg: the fragment's diagonal sits where col == row
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (l15 == 4 * g + r) dl[(2 * wave + f) * 16 + l15] = dacc[f][r];
}

__global__ __launch_bounds__(256) void retrieval_ranks_kernel(const Operands P, int row0, int row_end, int splits,
                                                              int* __restrict__ rank_i2t, int* __restrict__ cnt_t2i) {
    __shared__ __attribute__((aligned(16))) float lds[3 * RT * RLD];
    __shared__ float drow_s[RT], dcol_s[RT];
    __shared__ int ccnt[RT], rcnt[RT];
    float* As = lds;
    float* Bs = lds + RT * RLD;
    float* Ds = lds + 2 * RT * RLD;

    const int panel = blockIdx.x / splits, split = blockIdx.x % splits;
    const int m0 = row0 + panel * RT;
    const int N = P.N;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * (RT / 2), wn = (wave & 1) * (RT / 2);
    const int l15 = lane & 15, g = lane >> 4;

    f32x4 acc[RF][RF];
    // d_i of the panel's rows: the diagonals of the (virtual) column tile at m0
    rt_tile<false>(P, m0, m0, As, Bs, Ds, drow_s, acc);
    if (t < RT) rcnt[t] = 0;
    __syncthreads();
    const int ntiles = (N + RT - 1) / RT;
    for (int ct = split; ct < ntiles; ct += splits) {
        const int n0 = ct * RT;
        rt_tile<true>(P, m0, n0, As, Bs, Ds, dcol_s, acc);
        if (t < RT) ccnt[t] = 0;
        __syncthreads();
        float dj[RF];
        bool dj_bad[RF];
        int cc[RF];
#pragma unroll
        for (int n = 0; n < RF; ++n) {
            dj[n] = dcol_s[wn + n * 16 + l15];
            dj_bad[n] = !rt_finite(dj[n]);
            cc[n] = 0;
        }
#pragma unroll
        for (int i = 0; i < RF; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ri = wm + i * 16 + g * 4 + r, gi = m0 + ri;
                const float di = drow_s[ri];
                const bool di_bad = !rt_finite(di);
                int rc = 0;
#pragma unroll
                for (int n = 0; n < RF; ++n) {
                    const int gj = n0 + wn + n * 16 + l15;
                    const float z = acc[i][n][r];
                    const bool live = gi < row_end && gj < N && gi != gj;
                    const bool above_i = di_bad || z > di || (z == di && gj < gi);
                    const bool above_j = dj_bad[n] || z > dj[n] || (z == dj[n] && gi < gj);
                    rc += (live && above_i) ? 1 : 0;
                    cc[n] += (live && above_j) ? 1 : 0;
                }
                // row count: over the 16 columns of a fragment (lanes l15); the two waves that share the row meet in LDS
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) rc += __shfl_xor(rc, o, 64);
                if (l15 == 0 && rc != 0) atomicAdd(&rcnt[ri], rc);
            }
#pragma unroll
        for (int n = 0; n < RF; ++n) {
            int c = cc[n];
            c += __shfl_xor(c, 16, 64);
            c += __shfl_xor(c, 32, 64);
            if (g == 0 && c != 0) atomicAdd(&ccnt[wn + n * 16 + l15], c);
        }
        __syncthreads();
        if (t < RT && n0 + t < N && ccnt[t] != 0) atomicAdd(&cnt_t2i[n0 + t], ccnt[t]);
    }
    __syncthreads();
    if (t < RT && m0 + t < row_end && rcnt[t] != 0) atomicAdd(&rank_i2t[m0 + t - row0], rcnt[t]);
}

}  // namespace

extern "C" int sc_retrieval_ranks(const float* image_feat, long long ld_image, const float* text_feat, long long ld_text,
                                  int N, int D, int row0, int M, int* rank_i2t, int* cnt_t2i, void* stream) {
    SC_CHECK(N >= 1 && D >= 1, "sc_retrieval_ranks: bad shape N=%d D=%d", N, D);
    SC_CHECK(row0 >= 0 && M >= 0 && (long long)row0 + M <= N, "sc_retrieval_ranks: row block [%d, %d + %d) outside [0, %d)",
             row0, row0, M, N);
    SC_CHECK(ld_image >= D && ld_text >= D, "sc_retrieval_ranks: row strides %lld / %lld shorter than D=%d", ld_image,
             ld_text, D);
    SC_CHECK(image_feat != nullptr && text_feat != nullptr && cnt_t2i != nullptr && (rank_i2t != nullptr || M == 0),
             "sc_retrieval_ranks: null argument");
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    Operands P;
    P.img = image_feat; P.ld_img = ld_image;
    P.txt = text_feat; P.ld_txt = ld_text;
    // 16-byte global loads need an aligned base and a row stride that keeps every row aligned
    P.img_al = (reinterpret_cast<uintptr_t>(image_feat) & 15) == 0 && (ld_image & 3) == 0;
    P.txt_al = (reinterpret_cast<uintptr_t>(text_feat) & 15) == 0 && (ld_text & 3) == 0;
    P.N = N; P.D = D;
    const int panels = (M + RT - 1) / RT, ntiles = (N + RT - 1) / RT;
    // few panels: split each panel's walk over the column tiles so that about 1024 workgroups share the chip
    int splits = (1024 + panels - 1) / panels;
    if (splits > ntiles) splits = ntiles;
    if (splits < 1) splits = 1;
    SC_CHECK((long long)panels * splits < (1ll << 30), "sc_retrieval_ranks: too many workgroups");
    if (hipMemsetAsync(rank_i2t, 0, (size_t)M * sizeof(int), st) != hipSuccess) {
        sc_set_error("sc_retrieval_ranks: clearing rank_i2t failed");
        return -2;
    }
    retrieval_ranks_kernel<<<(unsigned)(panels * splits), 256, 0, st>>>(P, row0, row0 + M, splits, rank_i2t, cnt_t2i);
    SC_LAUNCH_CHECK();
    return 0;
}
