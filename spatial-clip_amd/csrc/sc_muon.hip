// Muon (torch.optim.Muon of torch 2.10) for chosen matrices of the flat buffers, AdamW for every other slot.
//   muon_momentum_kernel  B, bf16(U) into a compact bf16 buffer, sum of squares of bf16(U) per 64-float slot
//   muon_scale_kernel     per tensor: the norm from its slots' sums in fp64 (fixed order), X = bf16(U / max(norm, eps))
//   muon_axpby_kernel     C = bf16(beta Cin + alpha acc): the epilogue of a Newton-Schulz product whose fp32 accumulators
//                         sc_gemm_bf16 (SC_EPI_F32) left behind
//   muon_apply_kernel     p = p (1 - lr wd) - lr ratio O on Muon slots, adamw_groups_kernel's update on the others
// The products of the Newton-Schulz iterations run matrix by matrix through sc_gemm_bf16 (optim.FusedMuon._newton_schulz).
#include "sc_common.h"
#include "sc_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- streaming
// torch's lerp as its vectorised CPU kernel rounds it (ATen LerpKernel.cpp, lerp_vec: fmadd(coeff, end - start, base) with
// coeff = w, base = start for |w| < 0.5 and coeff = w - 1, base = end otherwise, so that both ends are exact).  The fused forms
// are written out: bf16(U) feeds an iteration that amplifies a rank-deficient update's rounding noise to full size, and an
// fp32 last-bit difference in U flips bf16 roundings that the result then shows.
SC_DEVICE float muon_lerp(float start, float end, float w) {
    return w < 0.5f ? fmaf(w, end - start, start) : fmaf(w - 1.0f, end - start, end);
}

// float4 i belongs to slot i >> 4: the 16 lanes [16 k, 16 k + 16) of a wave hold one slot, and n is a multiple of 64, so a
// slot's lanes enter and leave the loop together (lamb_moments_kernel).
__global__ __launch_bounds__(256) void muon_momentum_kernel(const float* __restrict__ g, float* __restrict__ m, long long n,
                                                            const int* __restrict__ slot_tensor, const int* __restrict__ info,
                                                            int n_tensors, long long slot0, float mu, float one_minus_mu,
                                                            int nesterov, float gscale, const float* __restrict__ normclip,
                                                            bf16* __restrict__ ubuf, float* __restrict__ slot_sums) {
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        const long long sl = i >> 4;
        const int t = slot_tensor[sl];
        if (t < 0 || t >= n_tensors) continue;
        const long long first = info[4 * t], end = info[4 * t + 1], xs = info[4 * t + 2];
        const long long gslot = slot0 + sl;
        if (gslot < first || gslot >= end) continue;        // a table that disagrees with itself: nothing is written
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        bf16x4 ub;
        float q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ge = gg[c] * gs;
            mm[c] = muon_lerp(mm[c], ge, one_minus_mu);
            const float u = nesterov ? muon_lerp(ge, mm[c], mu) : mm[c];
            ub[c] = (bf16)u;
            const float ur = (float)ub[c];
            q[c] = ur * ur;
        }
        float su = (q[0] + q[1]) + (q[2] + q[3]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) su += __shfl_xor(su, o, 64);
        reinterpret_cast<f32x4*>(m)[i] = mm;
        *reinterpret_cast<bf16x4*>(ubuf + ((xs + (gslot - first)) << 6) + ((i & 15) << 2)) = ub;
        if ((threadIdx.x & 15) == 0) slot_sums[sl] = su;
    }
}

// grid (MUON_SCALE_CHUNKS, n_tensors), 256 threads.  Every block of a tensor sums ALL of the tensor's slots in the same order
// (thread k: slots first + k, first + k + 256, ...; wave butterfly; the four waves in order), so they agree on the norm to the
// bit, then scales its share of the slots.  The redundant reads are 4 bytes per 64 elements and block, out of L2.
constexpr int MUON_SCALE_CHUNKS = 16;
__global__ __launch_bounds__(256) void muon_scale_kernel(const float* __restrict__ slot_sums, long long n_slots,
                                                         const int* __restrict__ info, float eps,
                                                         const bf16* __restrict__ ubuf, bf16* __restrict__ xbuf,
                                                         float* __restrict__ norms) {
    __shared__ double sm[4];
    const int t = blockIdx.y;
    const long long first = info[4 * t], end = info[4 * t + 1], xs = info[4 * t + 2];
    if (!(first >= 0 && first <= end && end <= n_slots && xs >= 0)) return;      // uniform over the block
    double s = 0.0;
    for (long long k = first + threadIdx.x; k < end; k += 256) s += (double)slot_sums[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    const double tot = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    const float norm = (float)sqrt(tot);
    if (blockIdx.x == 0 && threadIdx.x == 0) norms[t] = norm;
    const float den = fmaxf(norm, eps);
    const long long n8 = (end - first) << 3;        // 8 vectors of 8 bf16 per slot
    const bf16x8* src = reinterpret_cast<const bf16x8*>(ubuf + (xs << 6));
    bf16x8* dst = reinterpret_cast<bf16x8*>(xbuf + (xs << 6));
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)MUON_SCALE_CHUNKS * 256) {
        const bf16x8 u = src[i];
        bf16x8 x;
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (bf16)((float)u[k] / den);
        dst[i] = x;
    }
}

// Muon slots: decoupled decay and the orthogonalised update.  Every other covered slot: the update of adamw_groups_kernel
// (sc_optim.hip) with the same bits.  Copying that kernel's source is not enough: inside this kernel -ffp-contract=fast
// contracted m = b1 m + (1 - b1) ge the other way round (fma(1 - b1, ge, b1 m) for its fma(b1, m, (1 - b1) ge)) and p came out one
// ulp off.  So the three contractions the compiler makes there are written out as fmaf here, with every product that stays a
// product in its own expression; tests/test_gpu_muon.py holds the bits against sc_adamw_step_groups.
__global__ __launch_bounds__(256) void muon_apply_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, long long n,
                                                         const unsigned char* __restrict__ chunk_group,
                                                         const int* __restrict__ slot_tensor, const int* __restrict__ info,
                                                         const float* __restrict__ ratio, int n_tensors, long long slot0,
                                                         const bf16* __restrict__ obuf, const float* __restrict__ hyper,
                                                         int n_groups, float b1, float b2, float eps, float gscale,
                                                         const float* __restrict__ normclip, bf16* __restrict__ pbf) {
    __shared__ float2 group_scalars[256];       // {decay, step} of each group
    __shared__ float group_lr[256];
    const float bc1 = hyper[0], bc2_sqrt = hyper[1];
    if ((int)threadIdx.x < n_groups) {
        const float lr = hyper[2 + 2 * threadIdx.x], wd = hyper[3 + 2 * threadIdx.x];
        const float decay = 1.0f - lr * wd;
        const float step = lr / bc1;
        group_scalars[threadIdx.x] = make_float2(decay, step);
        group_lr[threadIdx.x] = lr;
    }
    __syncthreads();
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        const long long sl = i >> 4;
        const int t = slot_tensor[sl];
        const int grp = chunk_group[sl];
        if (t == -1) {
            const float2 ds = group_scalars[grp];
            const float decay = ds.x, step = ds.y;
            f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
            const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
            f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float ge = gg[c] * gs;
                mm[c] = fmaf(b1, mm[c], (1.0f - b1) * ge);
                vv[c] = fmaf(b2, vv[c], ((1.0f - b2) * ge) * ge);
                const float denom = sqrtf(vv[c]) / bc2_sqrt + eps;
                pp[c] = fmaf(decay, pp[c], -(step * (mm[c] / denom)));
            }
            reinterpret_cast<f32x4*>(p)[i] = pp;
            if (pbf) {
                bf16x4 o;
                o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
                reinterpret_cast<bf16x4*>(pbf)[i] = o;
            }
            reinterpret_cast<f32x4*>(m)[i] = mm;
            reinterpret_cast<f32x4*>(v)[i] = vv;
        } else if (t >= 0 && t < n_tensors) {
            const long long first = info[4 * t], end = info[4 * t + 1], xs = info[4 * t + 2];
            const long long gslot = slot0 + sl;
            if (gslot < first || gslot >= end) continue;
            const float decay = group_scalars[grp].x;
            const float step = group_lr[grp] * ratio[t];
            const bf16x4 ob = *reinterpret_cast<const bf16x4*>(obuf + ((xs + (gslot - first)) << 6) + ((i & 15) << 2));
            f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) pp[c] = fmaf(-step, (float)ob[c], pp[c] * decay);
            reinterpret_cast<f32x4*>(p)[i] = pp;
            if (pbf) {
                bf16x4 o;
                o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
                reinterpret_cast<bf16x4*>(pbf)[i] = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- epilogue
// out = bf16(beta * cin + alpha * acc): the epilogue of a Newton-Schulz product whose fp32 accumulators a GEMM of sc_gemm.hip
// (SC_EPI_F32) left in acc -- ONE rounding per product.  8 elements per thread and trip.
__global__ __launch_bounds__(256) void muon_axpby_kernel(const float* __restrict__ acc, const bf16* __restrict__ cin,
                                                         bf16* __restrict__ out, long long n8, float alpha, float beta) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 a0 = reinterpret_cast<const f32x4*>(acc)[2 * i], a1 = reinterpret_cast<const f32x4*>(acc)[2 * i + 1];
        const bf16x8 ci = reinterpret_cast<const bf16x8*>(cin)[i];
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = (bf16)fmaf(beta, (float)ci[k], alpha * a0[k]);
            o[4 + k] = (bf16)fmaf(beta, (float)ci[4 + k], alpha * a1[k]);
        }
        reinterpret_cast<bf16x8*>(out)[i] = o;
    }
}

inline bool muon_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}
inline int muon_blocks(long long n) {
    long long nb = (n / 4 + 255) / 256;
    return (int)(nb > 4096 ? 4096 : nb);
}

}  // namespace

extern "C" int sc_muon_momentum(const float* grads, float* exp_avg, long long n, const int* slot_tensor, const int* tensor_info,
                                int n_tensors, long long slot0, float momentum, float one_minus_momentum, int nesterov,
                                float grad_scale, const float* norm_clip, void* ubuf, float* slot_sums, void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_muon_momentum: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_tensors >= 1 && n_tensors <= (1 << 20), "sc_muon_momentum: n_tensors = %d (1 .. 2^20)", n_tensors);
    SC_CHECK(slot0 >= 0, "sc_muon_momentum: slot0 = %lld (>= 0)", slot0);
    SC_CHECK(momentum >= 0.0f && momentum <= 1.0f, "sc_muon_momentum: momentum = %g (0 .. 1)", (double)momentum);
    SC_CHECK(fabsf(one_minus_momentum - (1.0f - momentum)) <= 1e-6f, "sc_muon_momentum: one_minus_momentum = %g is not 1 - %g",
             (double)one_minus_momentum, (double)momentum);
    SC_CHECK(grads && exp_avg, "sc_muon_momentum: grads and exp_avg are required");
    SC_CHECK(slot_tensor != nullptr && tensor_info != nullptr && ubuf != nullptr && slot_sums != nullptr,
             "sc_muon_momentum: slot_tensor, tensor_info, ubuf and slot_sums are required");
    SC_CHECK(muon_aligned16(grads, exp_avg, ubuf, nullptr), "sc_muon_momentum: the buffers must be 16-byte aligned");
    muon_momentum_kernel<<<muon_blocks(n), 256, 0, (hipStream_t)stream>>>(grads, exp_avg, n, slot_tensor, tensor_info, n_tensors,
                                                                         slot0, momentum, one_minus_momentum, nesterov ? 1 : 0, grad_scale,
                                                                         norm_clip,
                                                                         (bf16*)ubuf, slot_sums);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_muon_scale(const float* slot_sums, long long n_slots, const int* tensor_info, int n_tensors, float eps,
                             const void* ubuf, void* xbuf, float* norms, void* stream) {
    SC_CHECK(n_slots > 0 && n_slots <= 0x7fffffffLL, "sc_muon_scale: n_slots = %lld (1 .. 2^31 - 1)", n_slots);
    SC_CHECK(n_tensors >= 1 && n_tensors <= 65535, "sc_muon_scale: n_tensors = %d (1 .. 65535)", n_tensors);
    SC_CHECK(eps > 0.0f, "sc_muon_scale: eps = %g (> 0)", (double)eps);
    SC_CHECK(slot_sums != nullptr && tensor_info != nullptr && ubuf != nullptr && xbuf != nullptr && norms != nullptr,
             "sc_muon_scale: slot_sums, tensor_info, ubuf, xbuf and norms are required");
    SC_CHECK(ubuf != xbuf, "sc_muon_scale: xbuf must not be ubuf");
    SC_CHECK(muon_aligned16(ubuf, xbuf, nullptr, nullptr), "sc_muon_scale: the bf16 buffers must be 16-byte aligned");
    muon_scale_kernel<<<dim3(MUON_SCALE_CHUNKS, n_tensors), 256, 0, (hipStream_t)stream>>>(slot_sums, n_slots, tensor_info, eps,
                                                                                         (const bf16*)ubuf, (bf16*)xbuf, norms);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_muon_axpby(const float* acc, const void* cin, void* out, long long n, float alpha, float beta, void* stream) {
    SC_CHECK(n > 0 && (n % 8) == 0, "sc_muon_axpby: n = %lld must be a positive multiple of 8", n);
    SC_CHECK(acc != nullptr && cin != nullptr && out != nullptr, "sc_muon_axpby: acc, cin and out are required");
    SC_CHECK(muon_aligned16(acc, cin, out, nullptr), "sc_muon_axpby: the buffers must be 16-byte aligned");
    long long nb = (n / 8 + 255) / 256;
    if (nb > 4096) nb = 4096;
    muon_axpby_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(acc, (const bf16*)cin, (bf16*)out, n / 8, alpha, beta);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_muon_apply(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                             const unsigned char* chunk_group, const int* slot_tensor, const int* tensor_info, const float* ratio,
                             int n_tensors, long long slot0, const void* obuf, const float* group_hyper, int n_groups, float beta1,
                             float beta2, float eps, float grad_scale, const float* norm_clip, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_muon_apply: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_muon_apply: n_groups = %d (1 .. 256)", n_groups);
    SC_CHECK(n_tensors >= 0 && n_tensors <= (1 << 20), "sc_muon_apply: n_tensors = %d (0 .. 2^20)", n_tensors);
    SC_CHECK(slot0 >= 0, "sc_muon_apply: slot0 = %lld (>= 0)", slot0);
    SC_CHECK(params && grads && exp_avg && exp_avg_sq, "sc_muon_apply: params, grads and both moments are required");
    SC_CHECK(chunk_group != nullptr && slot_tensor != nullptr && group_hyper != nullptr,
             "sc_muon_apply: chunk_group, slot_tensor and group_hyper are required");
    SC_CHECK(n_tensors == 0 || (tensor_info != nullptr && ratio != nullptr && obuf != nullptr),
             "sc_muon_apply: tensor_info, ratio and obuf are required with n_tensors = %d", n_tensors);
    SC_CHECK(muon_aligned16(params, grads, exp_avg, exp_avg_sq) && (((uintptr_t)params_bf16) & 7) == 0 && (((uintptr_t)obuf) & 7) == 0,
             "sc_muon_apply: the buffers must be 16-byte aligned, the bf16 buffers 8-byte aligned");
    muon_apply_kernel<<<muon_blocks(n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, chunk_group, slot_tensor,
                                                                      tensor_info, ratio, n_tensors, slot0, (const bf16*)obuf,
                                                                      group_hyper, n_groups, beta1, beta2, eps, grad_scale,
                                                                      norm_clip, (bf16*)params_bf16);
    SC_LAUNCH_CHECK();
    return 0;
}
