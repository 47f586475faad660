// Device side of the input pipeline: the two data-dependent steps the reference runs on CPU
// dataloader workers, moved next to the consumer so that a ~10 k pairs/s/GPU trainer is not fed at PIL speed.
//   sc_knn_alpha      spatial neighbours of every tile of one slide from its (x, y) centroid and their loss weights
//                     (docs/spatial_clip_data_pipeline.html "Step 1": KNN inside the same tissue sample,
//                     weight = 1 / (distance + 1e-6), alpha = weight / sum(weights); the Gaussian variant of
//                     notebooks/d1_dataset_construct_cw.ipynb is selectable)
//   sc_augment_tiles  RandomResizedCrop(scale, ratio) -> bicubic resize -> horizontal flip -> ColorJitter(brightness,
//                     contrast, saturation in a per-sample order) -> Normalize(mean, std) on decoded uint8 tiles
//                     (configs/model/spatial_clip.yaml:12-17 aug_cfg; src/open_clip/constants.py:1-2 mean / std)
//   sc_augment_tiles_ex  the rest of AugmentationCfg as timm's create_transform orders it (src/open_clip/transform.py:58-66,
//                     161-190): vertical flip, hue inside the jitter sequence, color_jitter_prob, RandomGrayscale,
//                     RandomErasing; one kernel body, two instantiations
// Random draws stay on the host (one small parameter row per sample), so a run is reproducible from its seed and the
// kernels are pure functions of their inputs.  Both are HBM-bound byte movers: coalesced reads of the source rows,
// one pass for the statistics the contrast step needs, one pass that writes the normalised fp32 NCHW tile.
#include <mutex>
#include <string.h>

#include "sc_common.h"
#include "sc_kernels.h"
#include "sc_color_core.h"

namespace {

// One wave per query tile.  K rounds; round r finds the candidate with the smallest (distance^2, index) key that is
// larger than the key selected in round r-1 -- no per-lane candidate lists, ties broken by index (deterministic).
__global__ __launch_bounds__(256) void knn_alpha_kernel(const float* __restrict__ xy, int N, int K, int mode, float sigma,
                                                        int* __restrict__ nbr, float* __restrict__ alpha) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= N) return;
    const float qx = xy[2 * wave], qy = xy[2 * wave + 1];
    float last_d = -1.f;
    int last_i = -1;
    float wsum = 0.f;
    for (int r = 0; r < K; ++r) {
        float best_d = 3.0e38f;
        int best_i = 0x7fffffff;
        for (int j = lane; j < N; j += 64) {
            if (j == wave) continue;
            const float dx = xy[2 * j] - qx, dy = xy[2 * j + 1] - qy;
            const float d = dx * dx + dy * dy;
            const bool after = d > last_d || (d == last_d && j > last_i);
            if (after && (d < best_d || (d == best_d && j < best_i))) { best_d = d; best_i = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(best_d, o, 64);
            const int oi = __shfl_xor(best_i, o, 64);
            if (od < best_d || (od == best_d && oi < best_i)) { best_d = od; best_i = oi; }
        }
        const bool found = best_i != 0x7fffffff;
        float w = 0.f;
        if (found) {
            const float dist = sqrtf(best_d);
            w = mode == 0 ? 1.0f / (dist + 1e-6f) : __expf(-best_d / (2.f * sigma * sigma));
            last_d = best_d;
            last_i = best_i;
        }
        wsum += w;
        if (lane == 0) {
            nbr[(long long)wave * K + r] = found ? best_i : -1;
            alpha[(long long)wave * K + r] = w;
        }
        if (!found) {                       // fewer than K other tiles: pad the rest
            for (int rr = r + 1; rr < K && lane == 0; ++rr) { nbr[(long long)wave * K + rr] = -1; alpha[(long long)wave * K + rr] = 0.f; }
            break;
        }
    }
    if (lane == 0 && wsum > 0.f) {
        const float inv = 1.0f / wsum;
        for (int r = 0; r < K; ++r) alpha[(long long)wave * K + r] *= inv;
    }
}

// One parameter row per sample: the 12 floats of sc_augment_tiles, or the SC_AUG_ROW floats of sc_augment_tiles_ex
// (include/spatial_clip_hip.h documents both; columns 9.. of a 12-float row read as 0)
constexpr int kAugRow = SC_AUG_ROW;
enum { kOpBrightness = 0, kOpContrast = 1, kOpSaturation = 2, kOpHue = 3 };
struct Jitter {
    float b, c, s;          // brightness / contrast / saturation factors (1 = identity)
    int shift;              // hue: what adjust_hue adds to the H channel, 0..255
    int seq, n;             // the ops in the order they run, two bits each from bit 0, and how many
};

// ---- What the reference's train transform does to a tile (src/open_clip/transform.py:186-204 with `use_timm: true`,
// configs/model/spatial_clip.yaml:12-17): timm's create_transform on a PIL image = RandomResizedCropAndInterpolation
// (torchvision F.resized_crop: img.crop(box).resize(size, BICUBIC)) -> RandomHorizontalFlip -> ColorJitter (PIL
// ImageEnhance.Brightness / Contrast / Color in a random order) -> ToTensor -> Normalize.  Everything up to ToTensor is
// 8-bit PIL arithmetic, restated here operation for operation so that the device result equals PIL's byte for byte:
//   * Image.resize = two separable passes (horizontal, then vertical) with an 8-bit intermediate image; per output pixel the
//     cubic-convolution filter (a = -0.5) with its support stretched by max(scale, 1) (that stretch IS the antialiasing),
//     taps clipped to the cropped image and renormalised; coefficients rounded to 22-bit fixed point, accumulator started
//     at 1 << 21, result >> 22 clipped to [0, 255] (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
//     ImagingResampleHorizontal_8bpc / Vertical_8bpc);
//   * ImageEnhance.X(img).enhance(f) = Image.blend(degenerate, img, f): out = (uint8)(d + f * (v - d)) in float32 with
//     truncation (clipped when f is outside [0, 1]; libImaging/Blend.c); degenerate = black (Brightness), the rounded mean
//     of the L image (Contrast), the L image (Color); L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Convert.c).
constexpr int kResampleBits = 32 - 8 - 2;           // PRECISION_BITS of Resample.c

SC_DEVICE double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// coefficients of output position `xx` for an axis of `in_size` source pixels resized to `out_size` (precompute_coeffs)
SC_DEVICE void pil_coeffs(int in_size, int out_size, int xx, int T, int* kk, int& xmin_out, int& cnt_out) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > T) xmax = T;                          // cannot happen: T is sized from the worst scale by the launcher
    double w[64];
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        w[x] = pil_bicubic((x + xmin - center + 0.5) * ss);
        ww += w[x];
    }
    for (int x = 0; x < xmax; ++x) {
        double k = ww != 0.0 ? w[x] / ww : w[x];
        kk[x] = k < 0 ? (int)(-0.5 + k * (1 << kResampleBits)) : (int)(0.5 + k * (1 << kResampleBits));
    }
    xmin_out = xmin;
    cnt_out = xmax;
}
SC_DEVICE int clip8(int ss) {
    ss >>= kResampleBits;
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}
using sc_color::pil_blend;
using sc_color::pil_luma;
template <bool EX>
SC_DEVICE void apply_op(int op, const Jitter& J, int mean_l, int (&v)[3]) {
    if (op == kOpBrightness) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(0, v[c], J.b);
    } else if (op == kOpContrast) {      // degenerate = mean L of the whole image at that point
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(mean_l, v[c], J.c);
    } else if (!EX || op == kOpSaturation) {
        const int g = pil_luma(v[0], v[1], v[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(g, v[c], J.s);
    } else {
        sc_color::pil_hue(J.shift, v[0], v[1], v[2]);
    }
}
// the first `n` ops of the sequence (n <= J.n)
template <bool EX>
SC_DEVICE void apply_seq(const Jitter& J, int n, int mean_l, int (&v)[3]) {
    if (EX) {
        for (int k = 0; k < n; ++k) apply_op<EX>((J.seq >> (2 * k)) & 3, J, mean_l, v);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n) apply_op<EX>((J.seq >> (2 * k)) & 3, J, mean_l, v);
    }
}
__constant__ int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// One workgroup per sample.  LDS: coefficient tables of both axes (int32 [S][T] + xmin / count per output position) and the
// 8-bit intermediate image of the horizontal pass for one channel ([crop_h][S]).  The resized 8-bit image is parked in the
// output tensor (as floats 0..255, flips applied on the way in) between the passes; the last pass overwrites it in place.
// EX = false reads 12-float rows (crop, three factors, order code, horizontal flip); EX = true reads the extended row:
// vertical flip, a jitter sequence of 0..4 ops with hue, the jitter switch, grayscale and erase boxes as well.
template <bool EX>
__global__ __launch_bounds__(1024) void augment_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                       const float* __restrict__ params, int stride, float* __restrict__ out,
                                                       int S, int T, float m0, float m1, float m2, float s0, float s1, float s2) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ long long red[16];
    const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    const float* p = params + (long long)b * stride;
    // integer crop box inside the tile (RandomResizedCrop draws integers; clamp defensively)
    int cw = min(max((int)p[2], 1), W), ch = min(max((int)p[3], 1), H);
    int x0 = min(max((int)p[0], 0), W - cw), y0 = min(max((int)p[1], 0), H - ch);
    int* kx = reinterpret_cast<int*>(lds);               // [S][T]
    int* ky = kx + S * T;                                // [S][T]
    int* xmin_x = ky + S * T;                            // [S] each
    int* cnt_x = xmin_x + S;
    int* ymin_y = cnt_x + S;
    int* cnt_y = ymin_y + S;
    unsigned char* tmp = reinterpret_cast<unsigned char*>(cnt_y + S);      // [ch][S]
    for (int i = t; i < 2 * S; i += nt) {
        if (i < S) pil_coeffs(cw, S, i, T, kx + i * T, xmin_x[i], cnt_x[i]);
        else pil_coeffs(ch, S, i - S, T, ky + (i - S) * T, ymin_y[i - S], cnt_y[i - S]);
    }
    __syncthreads();
    const unsigned char* img = src + (long long)b * H * W * 3;
    float* o = out + (long long)b * 3 * S * S;
    const bool flip = p[8] > 0.5f;
    const bool vflip = EX && p[9] > 0.5f;
    for (int c = 0; c < 3; ++c) {
        for (int i = t; i < ch * S; i += nt) {           // horizontal pass over the rows of the crop
            const int y = i / S, ox = i - y * S;
            const unsigned char* row = img + ((long long)(y0 + y) * W + x0 + xmin_x[ox]) * 3 + c;
            const int* k = kx + ox * T;
            int ss = 1 << (kResampleBits - 1);
            for (int x = 0; x < cnt_x[ox]; ++x) ss += (int)row[x * 3] * k[x];
            tmp[i] = (unsigned char)clip8(ss);
        }
        __syncthreads();
        for (int i = t; i < S * S; i += nt) {            // vertical pass
            const int oy = i / S, ox = i - oy * S;
            const int* k = ky + oy * T;
            const unsigned char* col = tmp + ymin_y[oy] * S + ox;
            int ss = 1 << (kResampleBits - 1);
            for (int y = 0; y < cnt_y[oy]; ++y) ss += (int)col[y * S] * k[y];
            o[c * S * S + (vflip ? S - 1 - oy : oy) * S + (flip ? S - 1 - ox : ox)] = (float)clip8(ss);
        }
        __syncthreads();
    }
    Jitter J;
    J.b = p[4]; J.c = p[5]; J.s = p[6];
    J.shift = 0;
    J.n = 3;
    if (!EX || (int)p[13] == 0) {                        // the 12-float rule: all three ops in the order of the code 0..5
        const int* perm = kPerm[min(max((int)p[7], 0), 5)];
        J.seq = perm[0] | (perm[1] << 2) | (perm[2] << 4);
    } else {
        J.n = min(max((int)p[13], 0), 4);
        J.seq = 0;
        for (int k = 0; k < J.n; ++k) J.seq |= ((int)p[14 + k] & 3) << (2 * k);
    }
    bool gray = false;
    int nbox = 0;
    int box[4][4];                                       // top, left, height, width
    if (EX) {
        J.shift = (int)((double)p[10] * 255.0) & 255;    // np.int32(hue_factor * 255).astype(np.uint8)
        if (p[12] > 0.5f) J.n = 0;                       // RandomApply left the jitter out
        gray = p[11] > 0.5f;
        nbox = min(max((int)p[18], 0), 4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) box[k][q] = k < nbox ? (int)p[20 + 4 * k + q] : 0;
    }
    int contrast_pos = -1;
    for (int k = J.n - 1; k >= 0; --k)
        if (((J.seq >> (2 * k)) & 3) == kOpContrast) contrast_pos = k;
    // mean of the L image as the contrast step meets it: int(ImageStat.Stat(L).mean[0] + 0.5)
    int mean_l = 0;
    if (!EX || contrast_pos >= 0) {
        long long part = 0;
        for (int i = t; i < S * S; i += nt) {
            int v[3] = {(int)o[i], (int)o[S * S + i], (int)o[2 * S * S + i]};
            apply_seq<EX>(J, contrast_pos, 0, v);
            part += pil_luma(v[0], v[1], v[2]);
        }
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        if ((t & 63) == 0) red[t >> 6] = part;
        __syncthreads();
        long long tot = 0;
        for (int w = 0; w < (nt >> 6); ++w) tot += red[w];
        mean_l = (int)((double)tot / (double)(S * S) + 0.5);
    }
    for (int i = t; i < S * S; i += nt) {
        int v[3] = {(int)o[i], (int)o[S * S + i], (int)o[2 * S * S + i]};
        apply_seq<EX>(J, J.n, mean_l, v);
        if (EX && gray) v[0] = v[1] = v[2] = pil_luma(v[0], v[1], v[2]);      // RandomGrayscale: convert("L") in three channels
        // ToTensor (uint8 / 255) then Normalize ((x - mean) / std), float32 like torchvision
        float r0 = ((float)v[0] / 255.0f - m0) / s0;
        float r1 = ((float)v[1] / 255.0f - m1) / s1;
        float r2 = ((float)v[2] / 255.0f - m2) / s2;
        if (EX && nbox > 0) {                            // RandomErasing (mode "const") on the normalised tensor
            const int y = i / S, x = i - y * S;
            bool hit = false;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                hit |= k < nbox && y >= box[k][0] && y < box[k][0] + box[k][2] && x >= box[k][1] && x < box[k][1] + box[k][3];
            if (hit) r0 = r1 = r2 = 0.0f;
        }
        o[i] = r0;
        o[S * S + i] = r1;
        o[2 * S * S + i] = r2;
    }
}

}  // namespace

extern "C" int sc_knn_alpha(const float* xy, int N, int K, int mode, float sigma, int* nbr_index, float* alpha,
                            void* stream) {
    SC_CHECK(N >= 1 && K >= 1 && K <= 64, "sc_knn_alpha: bad shape N=%d K=%d", N, K);
    SC_CHECK(mode == 0 || (mode == 1 && sigma > 0.f), "sc_knn_alpha: mode 0 (inverse distance) or 1 (gaussian, sigma > 0)");
    const int blocks = (N + 3) / 4;          // 4 waves (= 4 query tiles) per workgroup
    knn_alpha_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(xy, N, K, mode, sigma, nbr_index, alpha);
    SC_LAUNCH_CHECK();
    return 0;
}

namespace {

// shape checks, filter taps and LDS bytes shared by both augmentation entries; 0 or an error code
int augment_plan(const char* who, int B, int H, int W, int S, const float* mean3, const float* std3, int& T, size_t& lds) {
    SC_CHECK(B >= 1 && H >= 1 && W >= 1 && S >= 1, "%s: bad shape B=%d H=%d W=%d S=%d", who, B, H, W, S);
    SC_CHECK(mean3 && std3 && std3[0] > 0 && std3[1] > 0 && std3[2] > 0, "%s: mean / std (host pointers to 3 floats) required",
             who);
    // taps per output position: support 2 * max(scale, 1) either side of the centre, worst case = the whole tile
    const double fs = fmax(1.0, fmax((double)W, (double)H) / (double)S);
    T = (int)(4.0 * fs + 0.5) + 2;
    SC_CHECK(T <= 64, "%s: downsampling %dx%d tiles to %d needs %d filter taps (> 64)", who, W, H, S, T);
    lds = (size_t)(2 * S * T + 4 * S) * sizeof(int) + (size_t)H * S;
    SC_CHECK(lds <= 160 * 1024 - 256, "%s: %d x %d tiles at output size %d need %zu bytes of LDS", who, H, W, S, lds);
    return 0;
}

template <bool EX>
void augment_launch(const void* src, int B, int H, int W, const float* params_dev, int stride, float* out, int S, int T,
                    size_t lds, const float* mean3, const float* std3, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&augment_kernel<EX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024 - 256);
        attr_done = true;
    }
    augment_kernel<EX><<<B, 1024, lds, stream>>>((const unsigned char*)src, H, W, params_dev, stride, out, S, T, mean3[0],
                                                 mean3[1], mean3[2], std3[0], std3[1], std3[2]);
}

bool is_int_in(float v, int lo, int hi) { return v >= (float)lo && v <= (float)hi && v == (float)(int)v; }

// One extended row: 0, or an error code with sc_last_error set.  `uses_ex` reports whether the row asks for anything the
// 12-float kernel cannot do.
int augment_check_row(const float* p, int b, int S, bool& uses_ex) {
    SC_CHECK(is_int_in(p[13], 0, 4), "sc_augment_tiles_ex: row %d: %g jitter ops (0 = the 12-float rule, else 1..4)", b, p[13]);
    const int n = (int)p[13];
    int seen = 0;
    bool hue = false;
    for (int k = 0; k < n; ++k) {
        SC_CHECK(is_int_in(p[14 + k], 0, 3), "sc_augment_tiles_ex: row %d: op code %g at position %d is out of range 0..3", b,
                 p[14 + k], k);
        const int op = (int)p[14 + k];
        SC_CHECK(!(seen >> op & 1), "sc_augment_tiles_ex: row %d: op %d appears twice in the jitter sequence", b, op);
        seen |= 1 << op;
        hue |= op == kOpHue;
    }
    SC_CHECK(p[10] >= -0.5f && p[10] <= 0.5f, "sc_augment_tiles_ex: row %d: hue factor %g outside [-0.5, 0.5]", b, p[10]);
    SC_CHECK(is_int_in(p[18], 0, 4), "sc_augment_tiles_ex: row %d: %g erase boxes (at most 4)", b, p[18]);
    const int nbox = (int)p[18];
    for (int k = 0; k < nbox; ++k) {
        const float* q = p + 20 + 4 * k;
        SC_CHECK(is_int_in(q[0], 0, S - 1) && is_int_in(q[1], 0, S - 1) && is_int_in(q[2], 1, S) && is_int_in(q[3], 1, S) &&
                     (int)q[0] + (int)q[2] <= S && (int)q[1] + (int)q[3] <= S,
                 "sc_augment_tiles_ex: row %d: erase box %d (top %g, left %g, height %g, width %g) is not inside the %d x %d output",
                 b, k, q[0], q[1], q[2], q[3], S, S);
    }
    uses_ex = n != 0 || p[9] > 0.5f || p[11] > 0.5f || p[12] > 0.5f || nbox > 0;
    return 0;
}

// Parameter rows of sc_augment_tiles_ex travel host -> pinned slot -> device slot on the caller's stream.  A slot is taken
// again only after the kernel that last read it has finished (its event), so the call never waits for the stream it feeds.
struct ParamSlot {
    float* host = nullptr;
    float* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool busy = false;
};
constexpr int kParamSlots = 4;
ParamSlot g_slots[kParamSlots];
int g_next_slot = 0;
std::mutex g_slot_mu;

}  // namespace

extern "C" int sc_augment_tiles(const void* src_u8_hwc, int B, int H, int W, const float* params12, float* out_nchw,
                                int S, const float* mean3_host, const float* std3_host, void* stream) {
    int T;
    size_t lds;
    if (int rc = augment_plan("sc_augment_tiles", B, H, W, S, mean3_host, std3_host, T, lds)) return rc;
    augment_launch<false>(src_u8_hwc, B, H, W, params12, 12, out_nchw, S, T, lds, mean3_host, std3_host, (hipStream_t)stream);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_augment_tiles_ex(const void* src_u8_hwc, int B, int H, int W, const float* params_host, int param_stride,
                                   float* out_nchw, int S, const float* mean3_host, const float* std3_host, void* stream) {
    int T;
    size_t lds;
    if (int rc = augment_plan("sc_augment_tiles_ex", B, H, W, S, mean3_host, std3_host, T, lds)) return rc;
    SC_CHECK(params_host && param_stride >= kAugRow, "sc_augment_tiles_ex: params (HOST pointer) with a row stride >= %d floats",
             kAugRow);
    bool any_ex = false;
    for (int b = 0; b < B; ++b) {
        bool uses_ex = false;
        if (int rc = augment_check_row(params_host + (long long)b * param_stride, b, S, uses_ex)) return rc;
        any_ex |= uses_ex;
    }
    std::lock_guard<std::mutex> lock(g_slot_mu);
    ParamSlot& slot = g_slots[g_next_slot];
    g_next_slot = (g_next_slot + 1) % kParamSlots;
    if (slot.busy) {
        SC_CHECK(hipEventSynchronize(slot.done) == hipSuccess, "sc_augment_tiles_ex: waiting for a parameter slot failed");
        slot.busy = false;
    }
    const size_t bytes = (size_t)B * kAugRow * sizeof(float);
    if (slot.cap < bytes) {
        if (slot.host) (void)hipHostFree(slot.host);
        if (slot.dev) (void)hipFree(slot.dev);
        slot.host = slot.dev = nullptr;
        slot.cap = 0;
        const size_t cap = bytes + bytes / 4;
        SC_CHECK(hipHostMalloc(reinterpret_cast<void**>(&slot.host), cap, hipHostMallocDefault) == hipSuccess &&
                     hipMalloc(reinterpret_cast<void**>(&slot.dev), cap) == hipSuccess,
                 "sc_augment_tiles_ex: no memory for %zu bytes of parameter rows", cap);
        slot.cap = cap;
    }
    if (!slot.done)
        SC_CHECK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming) == hipSuccess,
                 "sc_augment_tiles_ex: hipEventCreate failed");
    for (int b = 0; b < B; ++b)
        memcpy(slot.host + (size_t)b * kAugRow, params_host + (long long)b * param_stride, kAugRow * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    SC_CHECK(hipMemcpyAsync(slot.dev, slot.host, bytes, hipMemcpyHostToDevice, st) == hipSuccess,
             "sc_augment_tiles_ex: copying the parameter rows failed");
    // rows that use nothing beyond the 12-float set run the 12-float kernel (same bytes, no extended-row reads)
    if (any_ex) augment_launch<true>(src_u8_hwc, B, H, W, slot.dev, kAugRow, out_nchw, S, T, lds, mean3_host, std3_host, st);
    else augment_launch<false>(src_u8_hwc, B, H, W, slot.dev, kAugRow, out_nchw, S, T, lds, mean3_host, std3_host, st);
    SC_LAUNCH_CHECK();
    slot.busy = hipEventRecord(slot.done, st) == hipSuccess;
    if (!slot.busy) (void)hipStreamSynchronize(st);
    return 0;
}
