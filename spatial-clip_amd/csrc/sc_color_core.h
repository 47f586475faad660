// 8-bit colour arithmetic of the device augmentation (sc_data.hip), written once for both sides: the HIP kernel and a plain
// g++ build (tests/test_cpu_color_core.py) include this file, so the conversions are checked against PIL over every
// input on the build machine before they run on a GPU.  No HIP types.
//
// Everything here restates Pillow operation for operation (the reference's train transform is timm / torchvision calling
// PIL on 8-bit tiles, src/open_clip/transform.py:58-66,161-190):
//   pil_luma     libImaging/Convert.c rgb2l:     L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   pil_blend    libImaging/Blend.c:             (uint8)(d + alpha * (v - d)) in float32, truncated (ImageEnhance.*)
//   pil_rgb2hsv  libImaging/Convert.c rgb2hsv_row: float32 with the double steps C's promotion rules give
//   pil_hsv2rgb  libImaging/Convert.c hsv2rgb
//   pil_hue      torchvision _functional_pil.adjust_hue: RGB -> HSV, h += shift (uint8, wraps), HSV -> RGB
// The library is built with -ffp-contract=fast, and a fused multiply-add rounds once where PIL rounds twice: the HSV code
// keeps every product apart from the sum that follows it (fmul / dmul below).
#pragma once
#include <math.h>

#ifndef SC_HD
#ifdef __HIPCC__
#define SC_HD __host__ __device__ __forceinline__
#else
#define SC_HD inline
#endif
#endif

namespace sc_color {

// A product that must be rounded on its own goes through fmul / dmul: on the device the result passes an empty asm
// statement, which the compiler cannot look through, so it cannot fuse the product into the sum that follows (only a
// product can be fused; sums, differences and quotients need nothing).
#ifdef __HIP_DEVICE_COMPILE__
SC_HD float fmul(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
SC_HD double dmul(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
#else
SC_HD float fmul(float a, float b) { return a * b; }
SC_HD double dmul(double a, double b) { return a * b; }
#endif

SC_HD int pil_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate d, image v, alpha) on one 8-bit value (float32 arithmetic, truncation)
SC_HD int pil_blend(int d, int v, float alpha) {
#ifdef __HIP_DEVICE_COMPILE__
    const float t = __fadd_rn((float)d, __fmul_rn(alpha, (float)(v - d)));
#else
    const float t = (float)d + alpha * (float)(v - d);
#endif
    if (alpha >= 0.f && alpha <= 1.0f) return (int)t & 255;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

SC_HD int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// image.convert("HSV") on one pixel
SC_HD void pil_rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    V = maxc;
    if (minc == maxc) {
        H = 0;
        S = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr;
    const float gc = (float)(maxc - g) / cr;
    const float bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;          // in [5/6, 11/6]: fmod(x, 1.0) = x - floor(x), exactly
    h = (float)(x - floor(x));
    H = clip255((int)dmul((double)h, 255.0));
    S = clip255((int)dmul((double)s, 255.0));
}

SC_HD int pil_round8(float v) { return clip255((int)roundf(v)); }       // C round: halves away from zero

// Image.merge("HSV", ...).convert("RGB") on one pixel
SC_HD void pil_hsv2rgb(int H, int S, int V, int& r, int& g, int& b) {
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double x = dmul((double)(float)H, 6.0) / 255.0;
    const int i = (int)floor(x);                               // 0..6
    const float f = (float)(x - (double)(float)i);
    const float fs = (float)((double)S / 255.0);
    const double v = (double)V;
    const int p = pil_round8((float)dmul(v, 1.0 - (double)fs));
    const int q = pil_round8((float)dmul(v, 1.0 - dmul((double)fs, (double)f)));
    const int t = pil_round8((float)dmul(v, 1.0 - dmul((double)fs, 1.0 - (double)f)));
    switch (i % 6) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

// torchvision adjust_hue(img, hue_factor) with shift = (uint8)(int32)(hue_factor * 255): the round trip runs even for
// shift 0 and is not the identity
SC_HD void pil_hue(int shift, int& r, int& g, int& b) {
    int H, S, V;
    pil_rgb2hsv(r, g, b, H, S, V);
    pil_hsv2rgb((H + shift) & 255, S, V, r, g, b);
}

}  // namespace sc_color
