// Optimiser step on flat fp32 buffers: global grad-norm (for clip_grad_norm_ 1.0), fused AdamW with the clip
// coefficient and the 1/world_size gradient averaging applied on the fly, no host synchronisation.
//   reference: torch.optim.AdamW(lr, betas=(0.9,0.98), eps=1e-6, weight_decay=0.1) over ALL parameters
//   (src/models/spatial_clip_module.py:138-158, configs/optimizer/adamw.yaml) + Lightning gradient_clip_val 1.0
//   (configs/trainer/default.yaml:19 == torch.nn.utils.clip_grad_norm_).
#include "sc_common.h"
#include "sc_kernels.h"

namespace {

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long long n,
                                                            double* __restrict__ partial) {
    __shared__ double sm[4];
    double acc = 0.0;
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double a4[4] = {0.0, 0.0, 0.0, 0.0};                 // four loads in flight per thread, four independent fp64 chains
    for (; i + 3 * stride < n4; i += 4 * stride) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i + u * stride];
            a4[u] += (double)(v[0] * v[0] + v[1] * v[1]) + (double)(v[2] * v[2] + v[3] * v[3]);
        }
    }
    for (; i < n4; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        acc += (double)(v[0] * v[0] + v[1] * v[1]) + (double)(v[2] * v[2] + v[3] * v[3]);
    }
    acc += (a4[0] + a4[1]) + (a4[2] + a4[3]);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = n4 << 2; i < n; ++i) acc += (double)x[i] * x[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// out[0] = sqrt(sum)*gscale (the norm of the averaged gradient), out[1] = clip coefficient
__global__ void sumsq_final_kernel(const double* __restrict__ partial, int nblk, float gscale, float max_norm,
                                   float* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s) * gscale;
        out[0] = norm;
        out[1] = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
    }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long long n,
                                                    float lr, float b1, float b2, float eps, float wd, float bc1,
                                                    float bc2_sqrt, float gscale, const float* __restrict__ normclip,
                                                    bf16* __restrict__ pbf, const float* __restrict__ hyper = nullptr) {
    if (hyper != nullptr) {     // step-dependent scalars from device memory: a captured hipGraph replays this launch every step
        lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2];
    }
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    const float decay = 1.0f - lr * wd;
    const float step = lr / bc1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ge = gg[c] * gs;
            pp[c] *= decay;
            mm[c] = b1 * mm[c] + (1.0f - b1) * ge;
            vv[c] = b2 * vv[c] + (1.0f - b2) * ge * ge;
            const float denom = sqrtf(vv[c]) / bc2_sqrt + eps;
            pp[c] -= step * (mm[c] / denom);
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if (pbf) {      // bf16 mirror of the master buffer: the forward GEMM operands are views of it
            bf16x4 o;
            o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
            reinterpret_cast<bf16x4*>(pbf)[i] = o;
        }
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
}

// ---- parameter groups (per-group lr / weight decay, torch.optim's list-of-dicts form): the same streaming update, ONE
// launch per range, with the two scalars that depend on the group looked up per 64-float slot.  The flat buffers are laid
// out in 64-float slots and no two parameters share one (params.py ALIGN), so float4 i belongs to slot i >> 4: sixteen
// consecutive lanes read the same table byte (one byte per 768 bytes of traffic) and the same LDS pair (a broadcast read).
//   hyper (DEVICE) = {1 - b1^t, sqrt(1 - b2^t)}, then {lr_g, wd_g} per group
// decay and step are formed per group at block start with adamw_kernel's expressions, and the loop body is adamw_kernel's,
// expression for expression: under -ffp-contract=fast the same source shape gets the same contractions, so a slot of group
// g comes out with the bits of adamw_kernel run on it with (lr_g, wd_g).  The table entries are validated where the table
// is built (optim.FusedAdamW); any byte indexes inside the 256 LDS pairs.
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long long n,
                                                           const unsigned char* __restrict__ chunk_group,
                                                           const float* __restrict__ hyper, int n_groups, float b1, float b2,
                                                           float eps, float gscale, const float* __restrict__ normclip,
                                                           bf16* __restrict__ pbf) {
    __shared__ float2 group_scalars[256];       // {decay, step} of each group
    const float bc1 = hyper[0], bc2_sqrt = hyper[1];
    if ((int)threadIdx.x < n_groups) {
        const float lr = hyper[2 + 2 * threadIdx.x], wd = hyper[3 + 2 * threadIdx.x];
        const float decay = 1.0f - lr * wd;
        const float step = lr / bc1;
        group_scalars[threadIdx.x] = make_float2(decay, step);
    }
    __syncthreads();
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        const float2 ds = group_scalars[chunk_group[i >> 4]];
        const float decay = ds.x, step = ds.y;
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ge = gg[c] * gs;
            pp[c] *= decay;
            mm[c] = b1 * mm[c] + (1.0f - b1) * ge;
            vv[c] = b2 * vv[c] + (1.0f - b2) * ge * ge;
            const float denom = sqrtf(vv[c]) / bc2_sqrt + eps;
            pp[c] -= step * (mm[c] / denom);
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if (pbf) {
            bf16x4 o;
            o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
            reinterpret_cast<bf16x4*>(pbf)[i] = o;
        }
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
}

// ---- Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", Algorithm 1; lion_pytorch.Lion, timm.optim.Lion):
// one moment, the update is the SIGN of an interpolation between moment and gradient:
//   c = b1 * m + (1 - b1) * ge;   p = p * (1 - lr * wd) - lr * sign(c);   m = b2 * m + (1 - b2) * ge
// with ge = g * grad_scale * clip as in adamw_kernel, decoupled weight decay applied first, no bias correction, no eps.
// sign(0) = 0: the zero padding of every parameter's last slot (p = g = m = 0) has c = 0 and must stay at zero.
// 22 bytes per parameter: 12 read (p, g, m), 10 written (p, m, bf16 mirror) against adamw_kernel's 30.
// ONE body for the three launch forms (host scalars, lr from device memory, per-slot groups): under -ffp-contract=fast the
// same source shape gets the same contractions, so the forms agree bit for bit (see adamw_groups_kernel above).
SC_DEVICE void lion_update(f32x4& pp, const f32x4& gg, f32x4& mm, float decay, float lr, float b1, float b2, float gs) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float ge = gg[c] * gs;
        const float cc = b1 * mm[c] + (1.0f - b1) * ge;
        const float upd = cc > 0.0f ? lr : (cc < 0.0f ? -lr : 0.0f);      // lr * sign(cc); 0 for cc = +-0 (and NaN)
        pp[c] *= decay;
        pp[c] -= upd;
        mm[c] = b2 * mm[c] + (1.0f - b2) * ge;
    }
}

// GROUPS = false: lr / wd are the arguments, or lr = lr_dev[0] when lr_dev is given (a captured hipGraph replays the launch).
// GROUPS = true: hyper (DEVICE) = {lr_g, wd_g} per group, chunk_group names the group of each 64-float slot (float4 i belongs
// to slot i >> 4); {decay, lr} of every group are formed at block start with the expression of the un-grouped form.
template <bool GROUPS>
__global__ __launch_bounds__(256) void lion_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   long long n, float lr, float wd, float b1, float b2, float gscale,
                                                   const float* __restrict__ normclip, bf16* __restrict__ pbf,
                                                   const float* __restrict__ lr_dev,
                                                   const unsigned char* __restrict__ chunk_group,
                                                   const float* __restrict__ hyper, int n_groups) {
    __shared__ float2 group_scalars[GROUPS ? 256 : 1];      // {decay, lr} of each group
    float decay = 0.f;
    if (GROUPS) {
        if ((int)threadIdx.x < n_groups) {
            const float lr_g = hyper[2 * threadIdx.x], wd_g = hyper[2 * threadIdx.x + 1];
            group_scalars[threadIdx.x] = make_float2(1.0f - lr_g * wd_g, lr_g);
        }
        __syncthreads();
    } else {
        if (lr_dev != nullptr) lr = lr_dev[0];
        decay = 1.0f - lr * wd;
    }
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        if (GROUPS) {
            const float2 ds = group_scalars[chunk_group[i >> 4]];
            decay = ds.x;
            lr = ds.y;
        }
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        lion_update(pp, gg, mm, decay, lr, b1, b2, gs);
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if (pbf) {      // bf16 mirror of the master buffer, as adamw_kernel writes it
            bf16x4 o;
            o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
            reinterpret_cast<bf16x4*>(pbf)[i] = o;
        }
        reinterpret_cast<f32x4*>(m)[i] = mm;
    }
}

// ---- LAMB (You et al. 2020; timm.optim.Lamb with its defaults, open_clip's `--opt timm/lamb`): Adam's moments, then a
// layer-wise trust ratio.  Per tensor T with {lr_T, wd_T}, for ge = g * grad_scale * clip:
//   m = b1 m + (1 - b1) ge;   v = b2 v + (1 - b2) ge^2
//   u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd_T p
//   r = ||p|| / ||u|| over T where both norms are positive, else 1 (and 1 where wd_T == 0 unless always_adapt);  p -= lr_T r u
// The update of an element depends on two norms over its whole tensor, and the flat buffers are cut into pieces that ignore
// tensor boundaries (buckets, trainable ranges, grid-stride trips).  So the reduction is segmented by the 64-float SLOT, the
// unit no cut divides: lamb_moments_kernel leaves {sum p^2, sum u^2} of every slot in a slot-indexed buffer, lamb_trust_kernel
// sums each tensor's slots, lamb_apply_kernel forms u again from (p, m, v) and applies the step.  A slot's pair depends on its
// 64 values alone, in a fixed order; a tensor's sums on its slots alone, in a fixed order; there are no atomics.  The bits are
// therefore the same however the buffer is cut and in whatever order the pieces are launched.
//   hyper (DEVICE) = {1 - b1^t, sqrt(1 - b2^t)}, then {lr_T, wd_T} per tensor (sc_lamb_hyper_host)
//   slot_tensor[slot] = the tensor of a slot, negative where the slot belongs to none (padding behind the last parameter, a
//   locked parameter): such a slot is neither read nor written.  32 bits wide: ViT-H + text has more than 256 tensors.
// u is formed by ONE function with explicit fmaf / division / sqrtf and no contractible product-sum, so that both kernels
// form the same bits from the same (p, m, v) whatever surrounds the call.  Slot padding (p = g = m = v = 0) gives u = 0.
SC_DEVICE float lamb_u(float p, float m, float v, float wd, float bc1, float bc2_sqrt, float eps) {
    return fmaf(wd, p, (m / bc1) / (sqrtf(v) / bc2_sqrt + eps));
}

// 42 bytes per parameter over the two streaming kernels: 16 read + 8 written here, 12 read + 6 written in lamb_apply_kernel.
// float4 i belongs to slot i >> 4, so the 16 lanes [16 k, 16 k + 16) of a wave hold one slot (the block starts on a multiple
// of 256 float4); n is a multiple of 64, so a slot's lanes enter and leave the loop together.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long long n,
                                                           const int* __restrict__ slot_tensor, const float* __restrict__ hyper,
                                                           int n_tensors, float b1, float b2, float eps, float gscale,
                                                           const float* __restrict__ normclip, float2* __restrict__ slot_sums) {
    const float bc1 = hyper[0], bc2_sqrt = hyper[1];
    const float gs = gscale * (normclip ? normclip[1] : 1.0f);
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        const int t = slot_tensor[i >> 4];
        if (t < 0 || t >= n_tensors) continue;
        const float wd = hyper[3 + 2 * t];
        const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        float pq[4], uq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ge = gg[c] * gs;
            mm[c] = b1 * mm[c] + (1.0f - b1) * ge;
            vv[c] = b2 * vv[c] + (1.0f - b2) * ge * ge;
            const float u = lamb_u(pp[c], mm[c], vv[c], wd, bc1, bc2_sqrt, eps);
            pq[c] = pp[c] * pp[c];
            uq[c] = u * u;
        }
        float sp = (pq[0] + pq[1]) + (pq[2] + pq[3]);
        float su = (uq[0] + uq[1]) + (uq[2] + uq[3]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {       // butterfly over the slot's 16 lanes: every lane ends with the same bits
            sp += __shfl_xor(sp, o, 64);
            su += __shfl_xor(su, o, 64);
        }
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if ((threadIdx.x & 15) == 0) slot_sums[i >> 4] = make_float2(sp, su);
    }
}

// One block of 1024 threads per tensor: its slots' pairs summed in fp64.  Thread k takes slots first + k, first + k + 1024, ...
// in turn, four at a time into four chains (four loads in flight: the largest tensor of configs[1] has 160 000 slots and its
// block is what the launch waits for), the rest into the first chain; then the chains, the wave butterfly and the sixteen
// waves in order.  tensor_slots = {first slot, one past the last} per tensor; a pair outside [0, n_slots] is not followed
// (r = 1).
__global__ __launch_bounds__(1024) void lamb_trust_kernel(const float2* __restrict__ slot_sums, long long n_slots,
                                                          const int* __restrict__ tensor_slots, const float* __restrict__ hyper,
                                                          int always_adapt, int trust_clip, float* __restrict__ trust) {
    __shared__ double sm[2][16];
    const int t = blockIdx.x;
    const long long first = tensor_slots[2 * t], end = tensor_slots[2 * t + 1];
    const bool ok = first >= 0 && first <= end && end <= n_slots;
    double p4[4] = {0.0, 0.0, 0.0, 0.0}, u4[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) {
        long long s = first + threadIdx.x;
        for (; s + 3 * 1024 < end; s += 4 * 1024) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 q = slot_sums[s + k * 1024];
                p4[k] += (double)q.x;
                u4[k] += (double)q.y;
            }
        }
        for (; s < end; s += 1024) {
            const float2 q = slot_sums[s];
            p4[0] += (double)q.x;
            u4[0] += (double)q.y;
        }
    }
    double sp = (p4[0] + p4[1]) + (p4[2] + p4[3]);
    double su = (u4[0] + u4[1]) + (u4[2] + u4[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sp += __shfl_xor(sp, o, 64);
        su += __shfl_xor(su, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[0][threadIdx.x >> 6] = sp;
        sm[1][threadIdx.x >> 6] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tp = 0.0, tu = 0.0;
        for (int w = 0; w < 16; ++w) {
            tp += sm[0][w];
            tu += sm[1][w];
        }
        const double pn = sqrt(tp), un = sqrt(tu);
        const float wd = hyper[3 + 2 * t];
        float r = 1.0f;
        if (ok && (always_adapt || wd != 0.0f) && pn > 0.0 && un > 0.0) r = (float)(pn / un);
        if (trust_clip) r = fminf(r, 1.0f);
        trust[t] = r;
    }
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                         const float* __restrict__ v, long long n,
                                                         const int* __restrict__ slot_tensor, const float* __restrict__ hyper,
                                                         const float* __restrict__ trust, int n_tensors, float eps,
                                                         bf16* __restrict__ pbf) {
    const float bc1 = hyper[0], bc2_sqrt = hyper[1];
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        const int t = slot_tensor[i >> 4];
        if (t < 0 || t >= n_tensors) continue;
        const float lr = hyper[2 + 2 * t], wd = hyper[3 + 2 * t];
        const float step = lr * trust[t];
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 mm = reinterpret_cast<const f32x4*>(m)[i];
        const f32x4 vv = reinterpret_cast<const f32x4*>(v)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float u = lamb_u(pp[c], mm[c], vv[c], wd, bc1, bc2_sqrt, eps);
            pp[c] -= step * u;
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if (pbf) {      // bf16 mirror of the master buffer, as adamw_kernel writes it
            bf16x4 o;
            o[0] = (bf16)pp[0]; o[1] = (bf16)pp[1]; o[2] = (bf16)pp[2]; o[3] = (bf16)pp[3];
            reinterpret_cast<bf16x4*>(pbf)[i] = o;
        }
    }
}

// ---- gradient accumulation (Trainer accumulate_grad_batches): every backward OVERWRITES the flat gradient buffer, so the
// sum over the micro-batches of a group is a running fp32 buffer beside it, folded once per micro-batch by this kernel:
//   mode 0 (first)  acc   = scale * grads
//   mode 1 (add)    acc   = acc + scale * grads
//   mode 2 (last)   grads = acc + scale * grads   (acc == nullptr: grads = scale * grads), acc untouched
// 12 bytes per parameter (two reads, one write), nothing else: a streaming kernel.  The product and the sum are two
// separately rounded fp32 operations, which makes the result bit-for-bit torch's `acc + scale * g` on a CPU.  This library
// is built with -ffp-contract=fast, under which the backend fuses a multiply into a dependent add whatever the source says
// (`#pragma clang fp contract(off)` is not enough), so the rounded product passes through an empty asm statement: no
// instruction, but a value the add cannot be fused across.
SC_DEVICE float accum_mul(float s, float g) {
    float p = s * g;
    asm("" : "+v"(p));
    return p;
}
SC_DEVICE float accum_mul_add(float a, float s, float g) { return a + accum_mul(s, g); }

template <int MODE>
SC_DEVICE float accum_one(float a, float s, float g, bool has_acc) {
    if (MODE == 0) return accum_mul(s, g);
    if (MODE == 2 && !has_acc) return accum_mul(s, g);
    return accum_mul_add(a, s, g);
}

// VEC: both pointers 16-byte aligned (every ParamStore range): 16-byte loads and stores, four vectors of each operand in
// flight per thread, grid-stride.  Otherwise (any 4-byte aligned pair, misaligned alike or differently): one float per
// lane and trip.  With `partial` (mode 2 only) the same pass leaves the block's fp64 sum of squares of the NEW gradient in
// partial[blockIdx.x], formed in the fixed order of sumsq_partial_kernel (thread chain, wave butterfly, four waves): no
// atomics, the same bits from run to run.  The launch then has exactly 1024 blocks, one producer per slot.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ grads, long long n,
                                                              float scale, double* __restrict__ partial) {
    const bool has_acc = acc != nullptr;
    float* dst = MODE == 2 ? grads : acc;       // one of the operands: every element is read before the same thread writes it
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double sq = 0.0;
    if (VEC) {
        const long long n4 = n >> 2;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (; i + 3 * stride < n4; i += 4 * stride) {
            f32x4 g[4], a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                g[u] = reinterpret_cast<const f32x4*>(grads)[i + u * stride];
                if (MODE != 0 && has_acc) a[u] = reinterpret_cast<const f32x4*>(acc)[i + u * stride];
                else a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                f32x4 r;
#pragma unroll
                for (int c = 0; c < 4; ++c) r[c] = accum_one<MODE>(a[u][c], scale, g[u][c], has_acc);
                reinterpret_cast<f32x4*>(dst)[i + u * stride] = r;
                if (MODE == 2 && partial) s4[u] += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
            }
        }
        for (; i < n4; i += stride) {
            const f32x4 g = reinterpret_cast<const f32x4*>(grads)[i];
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            if (MODE != 0 && has_acc) a = reinterpret_cast<const f32x4*>(acc)[i];
            f32x4 r;
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = accum_one<MODE>(a[c], scale, g[c], has_acc);
            reinterpret_cast<f32x4*>(dst)[i] = r;
            if (MODE == 2 && partial) sq += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
        }
        sq += (s4[0] + s4[1]) + (s4[2] + s4[3]);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (long long j = n4 << 2; j < n; ++j) {
                const float r = accum_one<MODE>((MODE != 0 && has_acc) ? acc[j] : 0.f, scale, grads[j], has_acc);
                dst[j] = r;
                if (MODE == 2 && partial) sq += (double)r * r;
            }
    } else {
        for (; i < n; i += stride) {
            const float r = accum_one<MODE>((MODE != 0 && has_acc) ? acc[i] : 0.f, scale, grads[i], has_acc);
            dst[i] = r;
            if (MODE == 2 && partial) sq += (double)r * r;
        }
    }
    if (MODE == 2 && partial) {
        __shared__ double sm[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) partial[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
    }
}

template <int MODE>
void launch_grad_accumulate(float* acc, float* grads, long long n, float scale, double* partial, hipStream_t st) {
    const bool vec = ((((uintptr_t)acc) | ((uintptr_t)grads)) & 15) == 0;
    const long long work = vec ? (n + 3) / 4 : n;
    long long nb = (work + 255) / 256;
    if (nb > 1024 || partial != nullptr) nb = 1024;       // the cap of sumsq_partial_kernel; with partials exactly its grid
    if (vec)
        grad_accumulate_kernel<MODE, true><<<(int)nb, 256, 0, st>>>(acc, grads, n, scale, partial);
    else
        grad_accumulate_kernel<MODE, false><<<(int)nb, 256, 0, st>>>(acc, grads, n, scale, partial);
}

}  // namespace

extern "C" int sc_grad_accumulate(float* acc, float* grads, long long n, float scale, int mode, double* partial1024,
                                  void* stream) {
    SC_CHECK(mode >= 0 && mode <= 2, "sc_grad_accumulate: mode %d (0 = first, 1 = add, 2 = last)", mode);
    SC_CHECK(grads != nullptr, "sc_grad_accumulate: grads is required");
    SC_CHECK(n >= 0, "sc_grad_accumulate: n = %lld", n);
    SC_CHECK(acc != nullptr || mode == 2, "sc_grad_accumulate: mode %d writes acc, which is NULL", mode);
    SC_CHECK(partial1024 == nullptr || mode == 2, "sc_grad_accumulate: the sums of squares are those of the summed gradient (mode 2)");
    SC_CHECK(((((uintptr_t)acc) | ((uintptr_t)grads)) & 3) == 0, "sc_grad_accumulate: pointers must be 4-byte aligned");
    SC_CHECK(acc != grads, "sc_grad_accumulate: acc and grads must not overlap");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0) launch_grad_accumulate<0>(acc, grads, n, scale, nullptr, st);
    else if (mode == 1) launch_grad_accumulate<1>(acc, grads, n, scale, nullptr, st);
    else launch_grad_accumulate<2>(acc, grads, n, scale, partial1024, st);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_grad_norm(const float* grads, long long n, float grad_scale, float max_norm, double* ws,
                            float* norm_clip_out, void* stream) {
    SC_CHECK(n > 0 && ws && norm_clip_out, "sc_grad_norm: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = 1024;
    sumsq_partial_kernel<<<nblk, 256, 0, st>>>(grads, n, ws);
    SC_LAUNCH_CHECK();
    sumsq_final_kernel<<<1, 64, 0, st>>>(ws, nblk, grad_scale, max_norm, norm_clip_out);
    SC_LAUNCH_CHECK();
    return 0;
}

// The two halves of sc_grad_norm as separate entry points, for the sharded optimiser (comm.ShardedGradExchange): every rank
// sums the squares of ITS shard of the reduced gradient into 1024 fp64 partials per contiguous piece, the partial arrays are
// all-reduced (SUM, fp64: a few KiB), and every rank finishes with the same global norm / clip coefficient.
extern "C" int sc_grad_sumsq_partial(const float* grads, long long n, double* partial1024, void* stream) {
    SC_CHECK(n > 0 && partial1024, "sc_grad_sumsq_partial: bad args");
    sumsq_partial_kernel<<<1024, 256, 0, (hipStream_t)stream>>>(grads, n, partial1024);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_grad_norm_final(const double* partial, int n_partial, float grad_scale, float max_norm, float* norm_clip_out,
                                  void* stream) {
    SC_CHECK(n_partial > 0 && partial && norm_clip_out, "sc_grad_norm_final: bad args");
    sumsq_final_kernel<<<1, 64, 0, (hipStream_t)stream>>>(partial, n_partial, grad_scale, max_norm, norm_clip_out);
    SC_LAUNCH_CHECK();
    return 0;
}

// host-side: the two bias-correction scalars exactly as sc_adamw_step forms them (one definition for the eager and the
// graph-replayed update: bit-identical weights)
static inline void adamw_bias_corrections(float beta1, float beta2, int step, float* bc1, float* bc2s) {
    *bc1 = 1.0f - powf(beta1, (float)step);
    *bc2s = sqrtf(1.0f - powf(beta2, (float)step));
}

extern "C" int sc_adamw_hyper_host(float lr, float beta1, float beta2, int step, float* out3_host) {
    SC_CHECK(out3_host != nullptr && step >= 1, "sc_adamw_hyper_host: host output triple required, step >= 1");
    out3_host[0] = lr;
    adamw_bias_corrections(beta1, beta2, step, out3_host + 1, out3_host + 2);
    return 0;
}

extern "C" int sc_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             const float* norm_clip, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 4) == 0 && step >= 1, "sc_adamw_step: n must be a positive multiple of 4, step >= 1");
    float bc1, bc2s;
    adamw_bias_corrections(beta1, beta2, step, &bc1, &bc2s);
    long long nb = (n / 4 + 255) / 256;
    if (nb > 4096) nb = 4096;
    adamw_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                                                           weight_decay, bc1, bc2s, grad_scale, norm_clip,
                                                           (bf16*)params_bf16);
    SC_LAUNCH_CHECK();
    return 0;
}

// The same update with its step-dependent scalars read from DEVICE memory: hyper[3] = {lr, 1 - beta1^step,
// sqrt(1 - beta2^step)} (what sc_adamw_step derives from its host arguments).  A training step captured into a hipGraph
// (spatial_clip_amd/graph.py) replays identical launches; the host refreshes the three floats before each replay.
extern "C" int sc_adamw_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                                 const float* hyper, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 const float* norm_clip, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 4) == 0 && hyper != nullptr, "sc_adamw_step_dev: n must be a positive multiple of 4, hyper required");
    long long nb = (n / 4 + 255) / 256;
    if (nb > 4096) nb = 4096;
    adamw_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2, eps,
                                                           weight_decay, 1.f, 1.f, grad_scale, norm_clip, (bf16*)params_bf16,
                                                           hyper);
    SC_LAUNCH_CHECK();
    return 0;
}

// Parameter groups: host-side scalars of one step, {1 - beta1^step, sqrt(1 - beta2^step)} (the bits sc_adamw_step forms) and
// then {lr_g, wd_g} per group, for the small pinned -> device copy in front of sc_adamw_step_groups.
extern "C" int sc_adamw_groups_hyper_host(const float* lr, const float* wd, int n_groups, float beta1, float beta2, int step,
                                          float* out_host) {
    SC_CHECK(lr != nullptr && wd != nullptr && out_host != nullptr, "sc_adamw_groups_hyper_host: lr, wd and the host output are required");
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_adamw_groups_hyper_host: n_groups = %d (1 .. 256)", n_groups);
    SC_CHECK(step >= 1, "sc_adamw_groups_hyper_host: step = %d (>= 1)", step);
    adamw_bias_corrections(beta1, beta2, step, out_host, out_host + 1);
    for (int k = 0; k < n_groups; ++k) {
        out_host[2 + 2 * k] = lr[k];
        out_host[3 + 2 * k] = wd[k];
    }
    return 0;
}

// AdamW over one range of the flat buffers with per-group lr / weight decay: chunk_group[n / 64] (DEVICE bytes) names the
// group of each 64-float slot of THIS range, group_hyper (DEVICE, 2 + 2 * n_groups floats) comes from
// sc_adamw_groups_hyper_host.  One launch form for the eager and the graph-captured step.
extern "C" int sc_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                                    const unsigned char* chunk_group, const float* group_hyper, int n_groups, float beta1,
                                    float beta2, float eps, float grad_scale, const float* norm_clip, void* params_bf16,
                                    void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_adamw_step_groups: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_adamw_step_groups: n_groups = %d (1 .. 256)", n_groups);
    SC_CHECK(chunk_group != nullptr && group_hyper != nullptr, "sc_adamw_step_groups: chunk_group and group_hyper are required");
    SC_CHECK(params && grads && exp_avg && exp_avg_sq, "sc_adamw_step_groups: params, grads and both moments are required");
    long long nb = (n / 4 + 255) / 256;
    if (nb > 4096) nb = 4096;
    adamw_groups_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, chunk_group, group_hyper,
                                                                  n_groups, beta1, beta2, eps, grad_scale, norm_clip,
                                                                  (bf16*)params_bf16);
    SC_LAUNCH_CHECK();
    return 0;
}

// ---- Lion: the three launch forms of lion_kernel, in the shape of the AdamW entry points (one moment, no eps, no step
// number: there is no bias correction).  n: a positive multiple of 4 (64 for the grouped form); params, grads and exp_avg are
// required, norm_clip and params_bf16 may be NULL.  A refusal launches nothing.
static inline int lion_blocks(long long n) {
    long long nb = (n / 4 + 255) / 256;
    return (int)(nb > 4096 ? 4096 : nb);
}

extern "C" int sc_lion_step(float* params, const float* grads, float* exp_avg, long long n, float lr, float beta1, float beta2,
                            float weight_decay, float grad_scale, const float* norm_clip, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 4) == 0, "sc_lion_step: n = %lld must be a positive multiple of 4", n);
    SC_CHECK(params && grads && exp_avg, "sc_lion_step: params, grads and exp_avg are required");
    lion_kernel<false><<<lion_blocks(n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, n, lr, weight_decay, beta1, beta2,
                                                                       grad_scale, norm_clip, (bf16*)params_bf16, nullptr,
                                                                       nullptr, nullptr, 0);
    SC_LAUNCH_CHECK();
    return 0;
}

// lr from ONE device float: the launch is identical from step to step (graph.GraphedTrainStep); same bits as sc_lion_step.
extern "C" int sc_lion_step_dev(float* params, const float* grads, float* exp_avg, long long n, const float* lr_dev, float beta1,
                                float beta2, float weight_decay, float grad_scale, const float* norm_clip, void* params_bf16,
                                void* stream) {
    SC_CHECK(n > 0 && (n % 4) == 0, "sc_lion_step_dev: n = %lld must be a positive multiple of 4", n);
    SC_CHECK(params && grads && exp_avg, "sc_lion_step_dev: params, grads and exp_avg are required");
    SC_CHECK(lr_dev != nullptr, "sc_lion_step_dev: lr_dev is required");
    lion_kernel<false><<<lion_blocks(n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, n, 0.f, weight_decay, beta1, beta2,
                                                                       grad_scale, norm_clip, (bf16*)params_bf16, lr_dev,
                                                                       nullptr, nullptr, 0);
    SC_LAUNCH_CHECK();
    return 0;
}

// Parameter groups: host-side {lr_g, wd_g} per group (2 * n_groups floats) for the small pinned -> device copy in front of
// sc_lion_step_groups.
extern "C" int sc_lion_groups_hyper_host(const float* lr, const float* wd, int n_groups, float* out_host) {
    SC_CHECK(lr != nullptr && wd != nullptr && out_host != nullptr, "sc_lion_groups_hyper_host: lr, wd and the host output are required");
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_lion_groups_hyper_host: n_groups = %d (1 .. 256)", n_groups);
    for (int k = 0; k < n_groups; ++k) {
        out_host[2 * k] = lr[k];
        out_host[2 * k + 1] = wd[k];
    }
    return 0;
}

extern "C" int sc_lion_step_groups(float* params, const float* grads, float* exp_avg, long long n,
                                   const unsigned char* chunk_group, const float* group_hyper, int n_groups, float beta1,
                                   float beta2, float grad_scale, const float* norm_clip, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_lion_step_groups: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_lion_step_groups: n_groups = %d (1 .. 256)", n_groups);
    SC_CHECK(chunk_group != nullptr && group_hyper != nullptr, "sc_lion_step_groups: chunk_group and group_hyper are required");
    SC_CHECK(params && grads && exp_avg, "sc_lion_step_groups: params, grads and exp_avg are required");
    lion_kernel<true><<<lion_blocks(n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, n, 0.f, 0.f, beta1, beta2, grad_scale,
                                                                      norm_clip, (bf16*)params_bf16, nullptr, chunk_group,
                                                                      group_hyper, n_groups);
    SC_LAUNCH_CHECK();
    return 0;
}

// ---- LAMB: the three kernels of one step and the host function that fills their scalar table.  One form for the eager
// and the graph-captured step, for one group and for many: the table carries every tensor's {lr, wd}.  A refusal launches
// nothing.
static inline bool lamb_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

extern "C" int sc_lamb_hyper_host(const float* lr, const float* wd, int n_groups, const int* tensor_group, int n_tensors,
                                  float beta1, float beta2, int step, float* out_host) {
    SC_CHECK(lr != nullptr && wd != nullptr && tensor_group != nullptr && out_host != nullptr,
             "sc_lamb_hyper_host: lr, wd, tensor_group and the host output are required");
    SC_CHECK(n_groups >= 1 && n_groups <= 256, "sc_lamb_hyper_host: n_groups = %d (1 .. 256)", n_groups);
    SC_CHECK(n_tensors >= 1 && n_tensors <= (1 << 20), "sc_lamb_hyper_host: n_tensors = %d (1 .. 2^20)", n_tensors);
    SC_CHECK(step >= 1, "sc_lamb_hyper_host: step = %d (>= 1)", step);
    for (int k = 0; k < n_tensors; ++k)
        SC_CHECK(tensor_group[k] >= 0 && tensor_group[k] < n_groups, "sc_lamb_hyper_host: tensor %d names group %d of %d", k,
                 tensor_group[k], n_groups);
    adamw_bias_corrections(beta1, beta2, step, out_host, out_host + 1);
    for (int k = 0; k < n_tensors; ++k) {
        out_host[2 + 2 * k] = lr[tensor_group[k]];
        out_host[3 + 2 * k] = wd[tensor_group[k]];
    }
    return 0;
}

extern "C" int sc_lamb_moments(const float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                               const int* slot_tensor, const float* hyper, int n_tensors, float beta1, float beta2, float eps,
                               float grad_scale, const float* norm_clip, float* slot_sums, void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_lamb_moments: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_tensors >= 1 && n_tensors <= (1 << 20), "sc_lamb_moments: n_tensors = %d (1 .. 2^20)", n_tensors);
    SC_CHECK(params && grads && exp_avg && exp_avg_sq, "sc_lamb_moments: params, grads and both moments are required");
    SC_CHECK(slot_tensor != nullptr && hyper != nullptr && slot_sums != nullptr,
             "sc_lamb_moments: slot_tensor, hyper and slot_sums are required");
    SC_CHECK(lamb_aligned16(params, grads, exp_avg, exp_avg_sq) && (((uintptr_t)slot_sums) & 7) == 0,
             "sc_lamb_moments: the buffers must be 16-byte aligned, slot_sums 8-byte aligned");
    lamb_moments_kernel<<<lion_blocks(n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, slot_tensor, hyper,
                                                                        n_tensors, beta1, beta2, eps, grad_scale, norm_clip,
                                                                        (float2*)slot_sums);
    SC_LAUNCH_CHECK();
    return 0;
}

// slot_sums: n_slots {sum p^2, sum u^2} pairs; tensor_slots (DEVICE): {first slot, one past the last} per tensor, inside
// [0, n_slots]; trust: n_tensors floats.
extern "C" int sc_lamb_trust(const float* slot_sums, long long n_slots, const int* tensor_slots, const float* hyper, int n_tensors,
                             int always_adapt, int trust_clip, float* trust, void* stream) {
    SC_CHECK(n_slots > 0 && n_slots <= 0x7fffffffLL, "sc_lamb_trust: n_slots = %lld (1 .. 2^31 - 1)", n_slots);
    SC_CHECK(n_tensors >= 1 && n_tensors <= (1 << 20), "sc_lamb_trust: n_tensors = %d (1 .. 2^20)", n_tensors);
    SC_CHECK(slot_sums != nullptr && tensor_slots != nullptr && hyper != nullptr && trust != nullptr,
             "sc_lamb_trust: slot_sums, tensor_slots, hyper and trust are required");
    SC_CHECK((((uintptr_t)slot_sums) & 7) == 0, "sc_lamb_trust: slot_sums must be 8-byte aligned");
    lamb_trust_kernel<<<n_tensors, 1024, 0, (hipStream_t)stream>>>((const float2*)slot_sums, n_slots, tensor_slots, hyper,
                                                                 always_adapt, trust_clip, trust);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_lamb_apply(float* params, const float* exp_avg, const float* exp_avg_sq, long long n, const int* slot_tensor,
                             const float* hyper, const float* trust, int n_tensors, float eps, void* params_bf16, void* stream) {
    SC_CHECK(n > 0 && (n % 64) == 0, "sc_lamb_apply: n = %lld must be a positive multiple of 64 (whole slots)", n);
    SC_CHECK(n_tensors >= 1 && n_tensors <= (1 << 20), "sc_lamb_apply: n_tensors = %d (1 .. 2^20)", n_tensors);
    SC_CHECK(params && exp_avg && exp_avg_sq, "sc_lamb_apply: params and both moments are required");
    SC_CHECK(slot_tensor != nullptr && hyper != nullptr && trust != nullptr, "sc_lamb_apply: slot_tensor, hyper and trust are required");
    SC_CHECK(lamb_aligned16(params, exp_avg, exp_avg_sq, nullptr) && (((uintptr_t)params_bf16) & 7) == 0,
             "sc_lamb_apply: the buffers must be 16-byte aligned, the bf16 mirror 8-byte aligned");
    lamb_apply_kernel<<<lion_blocks(n), 256, 0, (hipStream_t)stream>>>(params, exp_avg, exp_avg_sq, n, slot_tensor, hyper, trust,
                                                                      n_tensors, eps, (bf16*)params_bf16);
    SC_LAUNCH_CHECK();
    return 0;
}

// ---- weight averaging (an EMA / equal average of the master weights beside them) and the in-place exchange for validation.
//   reference: lightning.pytorch.callbacks.EMAWeightAveraging / WeightAveraging over torch.optim.swa_utils.AveragedModel
//   (get_ema_avg_fn(decay): decay * avg + (1 - decay) * p; the default rule: avg + (p - avg) / (n_averaged + 1)).
namespace {

constexpr int WAVG_THREADS = 256;
// One 16-byte vector of each operand per thread and trip; the rest of a long buffer is grid-strided.  Measured on the flat
// buffer of ViT-B-16-gene (96.7 M floats, cold): caps of 2048 / 4096 / 8192 / 16384 blocks gave 0.221 / 0.214 / 0.210 / 0.212 ms,
// no cap 0.198 ms, two measurements of one build differed by 0.013 ms; four vectors in flight per thread were slower (0.268
// against 0.239 ms at 4096 blocks in one run; profiles/weight_average_variants.txt).  The cap keeps the grid-stride loop within
// reach of a test.
constexpr int WAVG_MAX_BLOCKS = 16384;

struct wavg_ctl { int op; float a; float b; };

SC_DEVICE float wavg_barrier(float x) {     // keeps -ffp-contract=fast from fusing the operation in front with the one behind
    asm("" : "+v"(x));
    return x;
}

// every operation rounded to fp32 on its own: the bits a CPU gives for the same expression, evaluated operator by operator
template <int OP>
SC_DEVICE float wavg_one(float avg, float p, float a, float b) {
    if (OP == SC_WAVG_COPY) return p;
    if (OP == SC_WAVG_EMA) return wavg_barrier(a * avg) + wavg_barrier(b * p);
    const float d = wavg_barrier(p - avg);
    return avg + wavg_barrier(d / a);       // IEEE division (hipcc's default for fp32), not a reciprocal
}

// VEC: both pointers 16-byte aligned: 16-byte loads and stores, grid-stride; the n & 3 floats behind the last whole vector
// go to thread 0.  Otherwise one float per lane and trip.
// Every element is read before the same thread writes it; no two threads touch the same element: no atomics.
template <bool VEC, int OP>
SC_DEVICE void wavg_body(float* __restrict__ avg, const float* __restrict__ params, long long n, float a, float b) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const long long n4 = n >> 2;
        for (; i < n4; i += stride) {
            const f32x4 p = reinterpret_cast<const f32x4*>(params)[i];
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (OP != SC_WAVG_COPY) v = reinterpret_cast<const f32x4*>(avg)[i];
            f32x4 r;
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = wavg_one<OP>(v[c], p[c], a, b);
            reinterpret_cast<f32x4*>(avg)[i] = r;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (long long j = n4 << 2; j < n; ++j) avg[j] = wavg_one<OP>(OP != SC_WAVG_COPY ? avg[j] : 0.f, params[j], a, b);
    } else {
        for (; i < n; i += stride) avg[i] = wavg_one<OP>(OP != SC_WAVG_COPY ? avg[i] : 0.f, params[i], a, b);
    }
}

// DEV: {op, a, b} come from device memory (a captured hipGraph replays this launch; the host rewrites the block in front of
// each replay); op == skip -- or anything that is no op -- returns before any access to avg or params.
template <bool VEC, bool DEV>
__global__ __launch_bounds__(WAVG_THREADS) void weight_average_kernel(float* __restrict__ avg, const float* __restrict__ params,
                                                                       long long n, wavg_ctl host, const int* __restrict__ ctl) {
    int op = host.op;
    float a = host.a, b = host.b;
    if (DEV) {
        op = ctl[0];
        if (op == SC_WAVG_SKIP) return;
        a = __int_as_float(ctl[1]);
        b = __int_as_float(ctl[2]);
    }
    if (op == SC_WAVG_COPY) wavg_body<VEC, SC_WAVG_COPY>(avg, params, n, a, b);
    else if (op == SC_WAVG_EMA) wavg_body<VEC, SC_WAVG_EMA>(avg, params, n, a, b);
    else if (op == SC_WAVG_MEAN) wavg_body<VEC, SC_WAVG_MEAN>(avg, params, n, a, b);
}

template <bool VEC>
__global__ __launch_bounds__(WAVG_THREADS) void swap_f32_kernel(float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const long long n4 = n >> 2;
        for (; i < n4; i += stride) {
            const f32x4 p = reinterpret_cast<const f32x4*>(x)[i];
            const f32x4 v = reinterpret_cast<const f32x4*>(y)[i];
            reinterpret_cast<f32x4*>(x)[i] = v;
            reinterpret_cast<f32x4*>(y)[i] = p;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (long long j = n4 << 2; j < n; ++j) {
                const float p = x[j], v = y[j];
                x[j] = v;
                y[j] = p;
            }
    } else {
        for (; i < n; i += stride) {
            const float p = x[i], v = y[i];
            x[i] = v;
            y[i] = p;
        }
    }
}

int wavg_blocks(long long n, bool vec) {
    const long long work = vec ? (n + 3) / 4 : n;
    const long long nb = (work + WAVG_THREADS - 1) / WAVG_THREADS;
    return (int)(nb > WAVG_MAX_BLOCKS ? WAVG_MAX_BLOCKS : nb);
}

bool wavg_overlap(const float* x, const float* y, long long n) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y, bytes = (uintptr_t)n * 4;
    return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" long long sc_weight_average_pass_floats(void) {
    return (long long)WAVG_MAX_BLOCKS * WAVG_THREADS * 4;
}

extern "C" int sc_weight_average(float* avg, const float* params, long long n, int op, float a, float b, void* stream) {
    SC_CHECK(op >= SC_WAVG_SKIP && op <= SC_WAVG_MEAN, "sc_weight_average: op %d (0 = skip, 1 = copy, 2 = ema, 3 = mean)", op);
    SC_CHECK(avg != nullptr && params != nullptr, "sc_weight_average: avg and params are required");
    SC_CHECK(n >= 0, "sc_weight_average: n = %lld", n);
    SC_CHECK(((((uintptr_t)avg) | ((uintptr_t)params)) & 3) == 0, "sc_weight_average: pointers must be 4-byte aligned");
    SC_CHECK(n == 0 || !wavg_overlap(avg, params, n), "sc_weight_average: avg and params must not overlap");
    if (n == 0 || op == SC_WAVG_SKIP) return 0;
    const bool vec = ((((uintptr_t)avg) | ((uintptr_t)params)) & 15) == 0;
    const wavg_ctl c{op, a, b};
    if (vec)
        weight_average_kernel<true, false><<<wavg_blocks(n, true), WAVG_THREADS, 0, (hipStream_t)stream>>>(avg, params, n, c, nullptr);
    else
        weight_average_kernel<false, false><<<wavg_blocks(n, false), WAVG_THREADS, 0, (hipStream_t)stream>>>(avg, params, n, c, nullptr);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_weight_average_dev(float* avg, const float* params, long long n, const int* ctl, void* stream) {
    SC_CHECK(avg != nullptr && params != nullptr, "sc_weight_average_dev: avg and params are required");
    SC_CHECK(ctl != nullptr && (((uintptr_t)ctl) & 3) == 0, "sc_weight_average_dev: ctl (4-byte aligned device {op, a, b}) is required");
    SC_CHECK(n >= 0, "sc_weight_average_dev: n = %lld", n);
    SC_CHECK(((((uintptr_t)avg) | ((uintptr_t)params)) & 3) == 0, "sc_weight_average_dev: pointers must be 4-byte aligned");
    SC_CHECK(n == 0 || !wavg_overlap(avg, params, n), "sc_weight_average_dev: avg and params must not overlap");
    if (n == 0) return 0;
    const bool vec = ((((uintptr_t)avg) | ((uintptr_t)params)) & 15) == 0;
    const wavg_ctl c{SC_WAVG_SKIP, 0.f, 0.f};
    if (vec)
        weight_average_kernel<true, true><<<wavg_blocks(n, true), WAVG_THREADS, 0, (hipStream_t)stream>>>(avg, params, n, c, ctl);
    else
        weight_average_kernel<false, true><<<wavg_blocks(n, false), WAVG_THREADS, 0, (hipStream_t)stream>>>(avg, params, n, c, ctl);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_swap_f32(float* a, float* b, long long n, void* stream) {
    SC_CHECK(a != nullptr && b != nullptr, "sc_swap_f32: a and b are required");
    SC_CHECK(n >= 0, "sc_swap_f32: n = %lld", n);
    SC_CHECK(((((uintptr_t)a) | ((uintptr_t)b)) & 3) == 0, "sc_swap_f32: pointers must be 4-byte aligned");
    SC_CHECK(n == 0 || !wavg_overlap(a, b, n), "sc_swap_f32: a and b must not overlap");
    if (n == 0) return 0;
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
    if (vec)
        swap_f32_kernel<true><<<wavg_blocks(n, true), WAVG_THREADS, 0, (hipStream_t)stream>>>(a, b, n);
    else
        swap_f32_kernel<false><<<wavg_blocks(n, false), WAVG_THREADS, 0, (hipStream_t)stream>>>(a, b, n);
    SC_LAUNCH_CHECK();
    return 0;
}
