// Token mean pooling of an average-pooled tower (pool_type 'avg'; VisionTransformer._global_pool,
// src/open_clip/transformer.py:773-781: x[:, 1:].mean(dim=1)).
//   sc_token_pool_fwd : mean[b, c] = (1 / n) * sum_{t >= t0} x[b, t, c], n = L - t0, fp32 accumulation in a fixed order
//   sc_token_pool_bwd : dx[b, t, c] = t < t0 ? 0 : d_mean[b, c] / n, EVERY element written (fp32 and / or its bf16 rounding)
// Both are pure streams over contiguous [B, L, d] rows.  A sample's rows are one contiguous run of L * d elements, so the
// threads of a workgroup are laid over it as P token phases x G 16-byte column slots (thread = phase * G + slot): phase p
// walks tokens t0 + p, t0 + p + P, ... and consecutive threads touch consecutive 16 bytes across the row boundary -- every
// lane is busy at any width, where one wave per row would idle 5 lanes in 8 at d = 192.  No atomics: bit-reproducible.
#include "sc_common.h"
#include "sc_kernels.h"

namespace {

constexpr int POOL_U = 8;           // row loads in flight per lane (guideline: several 16-byte loads per lane)

// V columns per lane: 8 bf16 (16 bytes), 4 fp32 (16 bytes), or 4 bf16 (8 bytes) when d % 8 == 4
template <int V, bool XB> struct PoolVec;
template <> struct PoolVec<8, true> {
    typedef bf16x8 raw;
    static SC_DEVICE void acc(float* a, raw v) {
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] += (float)v[c];
    }
};
template <> struct PoolVec<4, true> {
    typedef bf16x4 raw;
    static SC_DEVICE void acc(float* a, raw v) {
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] += (float)v[c];
    }
};
template <> struct PoolVec<4, false> {
    typedef f32x4 raw;
    static SC_DEVICE void acc(float* a, raw v) {
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] += v[c];
    }
};

// slots per slab / phases of a T-thread workgroup over rows of nvec column slots (host and device agree through this)
struct PoolGeom {
    int nslab, G, P;
};
__host__ __device__ inline PoolGeom pool_geom(int nvec, int T) {
    PoolGeom g;
    g.nslab = (nvec + T - 1) / T;
    g.G = (nvec + g.nslab - 1) / g.nslab;
    g.P = T / g.G;
    return g;
}

// one workgroup per (sample, column slab).  Thread (p, e): two accumulator sets over its tokens (even / odd loads of a group
// of POOL_U), then the P phases are combined through LDS in ascending p by the phase-0 threads.  The order depends only on
// (L, t0, d): a fixed summation order.
template <int T, int V, bool XB>
__global__ __launch_bounds__(T) void token_pool_fwd_kernel(const void* __restrict__ xin, float* __restrict__ mean_f32,
                                                           bf16* __restrict__ mean_bf16, int L, int t0, int d) {
    typedef PoolVec<V, XB> PV;
    typedef typename PV::raw raw;
    __shared__ __attribute__((aligned(16))) float sm[T * V];
    const int nvec = d / V;
    const PoolGeom g = pool_geom(nvec, T);
    const int b = blockIdx.x / g.nslab, slab = blockIdx.x - b * g.nslab;
    const int tid = threadIdx.x;
    const int p = tid / g.G, el = tid - p * g.G;
    const int e = slab * g.G + el;
    const bool active = p < g.P && e < nvec;
    float a0[V], a1[V];
#pragma unroll
    for (int c = 0; c < V; ++c) a0[c] = a1[c] = 0.f;
    if (active) {
        const raw* row = reinterpret_cast<const raw*>(xin) + (long long)b * L * nvec + e;
        const long long step = (long long)g.P * nvec;
        int t = t0 + p;
        for (; t + (POOL_U - 1) * g.P < L; t += POOL_U * g.P) {
            raw v[POOL_U];
#pragma unroll
            for (int u = 0; u < POOL_U; ++u) v[u] = row[(long long)t * nvec + u * step];
#pragma unroll
            for (int u = 0; u < POOL_U; u += 2) {
                PV::acc(a0, v[u]);
                PV::acc(a1, v[u + 1]);
            }
        }
        for (int u = 0; t < L; t += g.P, ++u) {
            const raw v = row[(long long)t * nvec];
            if (u & 1) PV::acc(a1, v); else PV::acc(a0, v);
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) a0[c] += a1[c];
    if (g.P > 1) {
        if (active) {
#pragma unroll
            for (int c = 0; c < V; ++c) sm[(p * g.G + el) * V + c] = a0[c];
        }
        __syncthreads();
        if (active && p == 0) {
            for (int q = 1; q < g.P; ++q) {
#pragma unroll
                for (int c = 0; c < V; ++c) a0[c] += sm[(q * g.G + el) * V + c];
            }
        }
    }
    if (active && p == 0) {
        const float n = (float)(L - t0);
        const long long o = (long long)b * d + (long long)e * V;
#pragma unroll
        for (int c = 0; c < V; ++c) a0[c] = a0[c] / n;
        if (mean_f32 != nullptr) {
#pragma unroll
            for (int c = 0; c < V; c += 4)
                *reinterpret_cast<f32x4*>(mean_f32 + o + c) = (f32x4){a0[c], a0[c + 1], a0[c + 2], a0[c + 3]};
        }
        if (mean_bf16 != nullptr) {
#pragma unroll
            for (int c = 0; c < V; c += 4)
                *reinterpret_cast<u32x2*>(mean_bf16 + o + c) = sc_pack4(a0[c], a0[c + 1], a0[c + 2], a0[c + 3]);
        }
    }
}

// work item = (sample, chunk of tokens); the grid loops over the items.  Thread (p, e) forms its columns of d_mean / n once per
// item and stores them to tokens c0 + p, c0 + p + P, ... of the chunk (zeros below t0) with 16-byte stores.  At V = 8 a thread
// owns bf16 slot e (columns 8e .. 8e + 7) and the fp32 slots e and e + G (columns 4e .. and 4(e + G) ..), so that the lanes of a
// wave write one contiguous run per store instruction in both outputs (a thread storing its own 32 bytes of fp32 in two halves
// left every instruction with half-filled lines); the value of a column is the same fp32 division wherever it is formed.
template <int V, bool DB>
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(const void* __restrict__ dmean, float* __restrict__ dx_f32,
                                                             bf16* __restrict__ dx_bf16, int B, int L, int t0, int d, int chunk,
                                                             int nchunk) {
    constexpr int NF = V / 4;                     // fp32 slots of four columns per thread
    const int nvec = d / V;
    const PoolGeom g = pool_geom(nvec, 256);      // V = 8: nvec <= 256, one slab, G = nvec
    const int tid = threadIdx.x;
    const int p = tid / g.G, el = tid - p * g.G;
    if (p >= g.P) return;
    const float n = (float)(L - t0);
    const long long items = (long long)B * nchunk * g.nslab;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int slab = (int)(it % g.nslab);
        const long long r = it / g.nslab;
        const int ck = (int)(r % nchunk), b = (int)(r / nchunk);
        const int e = slab * g.G + el;
        if (e >= nvec) continue;
        auto quad = [&](int col) {                // d_mean[b, col .. col + 3] / n
            f32x4 q;
            if (DB) {
                const bf16x4 h = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(dmean) + (long long)b * d + col);
                q = (f32x4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            } else {
                q = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(dmean) + (long long)b * d + col);
            }
            return (f32x4){q[0] / n, q[1] / n, q[2] / n, q[3] / n};
        };
        int colf[NF];
        f32x4 vf[NF], vb[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            colf[k] = (e + k * g.G) * 4;
            vf[k] = quad(colf[k]);
            vb[k] = quad(e * V + k * 4);
        }
        const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int c0 = ck * chunk;
        const int c1 = c0 + chunk < L ? c0 + chunk : L;
        for (int t = c0 + p; t < c1; t += g.P) {
            const bool z = t < t0;
            const long long o = ((long long)b * L + t) * d;
            if (dx_f32 != nullptr) {
#pragma unroll
                for (int k = 0; k < NF; ++k) *reinterpret_cast<f32x4*>(dx_f32 + o + colf[k]) = z ? zero : vf[k];
            }
            if (dx_bf16 != nullptr) {
                if (V == 8) {
                    const u32x2 lo = sc_pack4(vb[0][0], vb[0][1], vb[0][2], vb[0][3]);
                    const u32x2 hi = sc_pack4(vb[NF - 1][0], vb[NF - 1][1], vb[NF - 1][2], vb[NF - 1][3]);
                    u32x4 w = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                    if (z) w = (u32x4){0u, 0u, 0u, 0u};
                    *reinterpret_cast<u32x4*>(dx_bf16 + o + e * V) = w;
                } else {
                    u32x2 w = sc_pack4(vb[0][0], vb[0][1], vb[0][2], vb[0][3]);
                    if (z) w = (u32x2){0u, 0u};
                    *reinterpret_cast<u32x2*>(dx_bf16 + o + e * V) = w;
                }
            }
        }
    }
}

// 16 waves per workgroup split a sample's tokens: a row is at most 512 slots wide, so even one sample keeps 16 waves x POOL_U
// loads in flight, and a batch of 256 (one workgroup per CU) fills the machine
constexpr int POOL_T = 1024;

template <int V, bool XB>
void pool_fwd_pick(const void* x, int B, int L, int t0, int d, float* mf, void* mb, hipStream_t st) {
    const PoolGeom g = pool_geom(d / V, POOL_T);
    token_pool_fwd_kernel<POOL_T, V, XB><<<B * g.nslab, POOL_T, 0, st>>>(x, mf, (bf16*)mb, L, t0, d);
}

template <int V, bool DB>
void pool_bwd_launch(const void* dm, int B, int L, int t0, int d, float* df, void* db, hipStream_t st) {
    const PoolGeom g = pool_geom(d / V, 256);
    // token chunks: about 2048 work items at least, a chunk no shorter than one sweep of the phases
    int nchunk = (int)((2048 + (long long)B * g.nslab - 1) / ((long long)B * g.nslab));
    const int maxchunk = (L + g.P - 1) / g.P;
    if (nchunk > maxchunk) nchunk = maxchunk;
    if (nchunk < 1) nchunk = 1;
    const int chunk = (L + nchunk - 1) / nchunk;
    nchunk = (L + chunk - 1) / chunk;
    const long long items = (long long)B * nchunk * g.nslab;
    const int grid = (int)(items < 2048 ? items : 2048);
    token_pool_bwd_kernel<V, DB><<<grid, 256, 0, st>>>(dm, df, (bf16*)db, B, L, t0, d, chunk, nchunk);
}

bool pool_aligned(const void* p, int bytes) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

}  // namespace

extern "C" int sc_token_pool_fwd(const void* x, int x_is_bf16, int B, int L, int t0, int d, float* mean_f32, void* mean_bf16,
                                 void* stream) {
    SC_CHECK(B > 0 && L > 0 && t0 >= 0 && t0 < L && d > 0 && (d % 4) == 0 && d <= 2048,
             "sc_token_pool_fwd: bad shape B=%d L=%d t0=%d d=%d", B, L, t0, d);
    SC_CHECK(x != nullptr && (mean_f32 != nullptr || mean_bf16 != nullptr), "sc_token_pool_fwd: null input or no output");
    SC_CHECK(pool_aligned(x, 16) && pool_aligned(mean_f32, 16) && pool_aligned(mean_bf16, 16),
             "sc_token_pool_fwd: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (x_is_bf16) {
        if ((d % 8) == 0) pool_fwd_pick<8, true>(x, B, L, t0, d, mean_f32, mean_bf16, st);
        else pool_fwd_pick<4, true>(x, B, L, t0, d, mean_f32, mean_bf16, st);
    } else {
        pool_fwd_pick<4, false>(x, B, L, t0, d, mean_f32, mean_bf16, st);
    }
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_token_pool_bwd(const void* d_mean, int d_is_bf16, int B, int L, int t0, int d, float* dx_f32, void* dx_bf16,
                                 void* stream) {
    SC_CHECK(B > 0 && L > 0 && t0 >= 0 && t0 < L && d > 0 && (d % 4) == 0 && d <= 2048,
             "sc_token_pool_bwd: bad shape B=%d L=%d t0=%d d=%d", B, L, t0, d);
    SC_CHECK(d_mean != nullptr && (dx_f32 != nullptr || dx_bf16 != nullptr), "sc_token_pool_bwd: null input or no output");
    SC_CHECK(pool_aligned(d_mean, 16) && pool_aligned(dx_f32, 16) && pool_aligned(dx_bf16, 16),
             "sc_token_pool_bwd: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const bool v8 = (d % 8) == 0;
    if (d_is_bf16) {
        if (v8) pool_bwd_launch<8, true>(d_mean, B, L, t0, d, dx_f32, dx_bf16, st);
        else pool_bwd_launch<4, true>(d_mean, B, L, t0, d, dx_f32, dx_bf16, st);
    } else {
        if (v8) pool_bwd_launch<8, false>(d_mean, B, L, t0, d, dx_f32, dx_bf16, st);
        else pool_bwd_launch<4, false>(d_mean, B, L, t0, d, dx_f32, dx_bf16, st);
    }
    SC_LAUNCH_CHECK();
    return 0;
}
