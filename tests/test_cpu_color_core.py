"""csrc/sc_color_core.h (the 8-bit colour arithmetic of the device augmentation: HSV conversions, luma, blend) compiled by
g++ for the CPU and compared with PIL itself over EVERY input: 2^24 RGB triples through ``convert("HSV")``, 2^24 HSV
triples through ``convert("RGB")``, zero mismatches.  The kernel includes the same header, so what runs on the GPU is
this arithmetic (the device build swaps the plain products and sums for round-to-nearest intrinsics, nothing else)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageEnhance

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spatial-clip_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

_WRAPPER = r"""
#include "sc_color_core.h"
extern "C" {
void rgb2hsv_all(const unsigned char* in, unsigned char* out, long long n) {
    for (long long i = 0; i < n; ++i) {
        int h, s, v;
        sc_color::pil_rgb2hsv(in[3 * i], in[3 * i + 1], in[3 * i + 2], h, s, v);
        out[3 * i] = (unsigned char)h; out[3 * i + 1] = (unsigned char)s; out[3 * i + 2] = (unsigned char)v;
    }
}
void hsv2rgb_all(const unsigned char* in, unsigned char* out, long long n) {
    for (long long i = 0; i < n; ++i) {
        int r, g, b;
        sc_color::pil_hsv2rgb(in[3 * i], in[3 * i + 1], in[3 * i + 2], r, g, b);
        out[3 * i] = (unsigned char)r; out[3 * i + 1] = (unsigned char)g; out[3 * i + 2] = (unsigned char)b;
    }
}
void hue_all(const unsigned char* in, unsigned char* out, long long n, int shift) {
    for (long long i = 0; i < n; ++i) {
        int r = in[3 * i], g = in[3 * i + 1], b = in[3 * i + 2];
        sc_color::pil_hue(shift, r, g, b);
        out[3 * i] = (unsigned char)r; out[3 * i + 1] = (unsigned char)g; out[3 * i + 2] = (unsigned char)b;
    }
}
void luma_all(const unsigned char* in, unsigned char* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = (unsigned char)sc_color::pil_luma(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
}
void blend_all(const unsigned char* d, const unsigned char* v, unsigned char* out, long long n, float alpha) {
    for (long long i = 0; i < n; ++i) out[i] = (unsigned char)sc_color::pil_blend(d[i], v[i], alpha);
}
}
"""

# every conversion of every input once, under the sanitizers; prints two checksums the test compares with the plain build
_MAIN = r"""
#include <stdio.h>
#include "sc_color_core.h"
int main() {
    unsigned long long a = 0, b = 0;
    for (int r = 0; r < 256; ++r)
        for (int g = 0; g < 256; ++g)
            for (int c = 0; c < 256; ++c) {
                int x, y, z;
                sc_color::pil_rgb2hsv(r, g, c, x, y, z);
                a += (unsigned long long)(x * 65536 + y * 256 + z) * (unsigned)(r + 3 * g + 7 * c + 1);
                sc_color::pil_hsv2rgb(r, g, c, x, y, z);
                b += (unsigned long long)(x * 65536 + y * 256 + z) * (unsigned)(r + 3 * g + 7 * c + 1);
            }
    int r = 200, g = 10, c = 90;
    for (int shift = 0; shift < 256; ++shift) sc_color::pil_hue(shift, r, g, c);
    const float alphas[4] = {-0.5f, 0.0f, 0.7f, 1.9f};
    int acc = 0;
    for (int k = 0; k < 4; ++k)
        for (int d = 0; d < 256; ++d)
            for (int v = 0; v < 256; ++v) acc += sc_color::pil_blend(d, v, alphas[k]);
    printf("%llu %llu %d\n", a, b, acc + r + g + c);
    return 0;
}
"""


def _all_triples() -> np.ndarray:
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.ascontiguousarray(np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler on this machine")
    d = tmp_path_factory.mktemp("color_core")
    src, so = str(d / "color_core_host.cpp"), str(d / "libcolor_core_host.so")
    with open(src, "w") as f:
        f.write(_WRAPPER)
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)

    def call(name, inp, *extra):
        out = np.empty_like(inp) if name != "luma_all" else np.empty(len(inp), dtype=np.uint8)
        getattr(lib, name)(inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                           ctypes.c_longlong(len(inp)), *extra)
        return out
    call.lib, call.dir = lib, d
    return call


@pytest.fixture(scope="module")
def triples():
    return _all_triples()


def _pil_convert(triples: np.ndarray, src_mode: str, dst_mode: str) -> np.ndarray:
    im = Image.frombuffer(src_mode, (4096, 4096), triples.tobytes(), "raw", src_mode, 0, 1)
    return np.asarray(im.convert(dst_mode), dtype=np.uint8).reshape(-1, 3)


def test_rgb_to_hsv_equals_pil_on_all_inputs(core, triples):
    got = core("rgb2hsv_all", triples)
    want = _pil_convert(triples, "RGB", "HSV")
    assert int((got != want).any(axis=1).sum()) == 0


def test_hsv_to_rgb_equals_pil_on_all_inputs(core, triples):
    got = core("hsv2rgb_all", triples)
    want = _pil_convert(triples, "HSV", "RGB")
    assert int((got != want).any(axis=1).sum()) == 0


@pytest.mark.parametrize("factor", [0.0, 1 / 255, 0.5 - 1e-9, -0.5, 0.1234, -0.3])
def test_hue_op_equals_the_pil_round_trip(core, factor):
    """torchvision's adjust_hue spelled with PIL calls, on a 64^3 sub-lattice of the colour cube (every fourth level plus
    255): the shift is truncated toward zero and wraps in uint8; shift 0 still goes through HSV and is not the identity."""
    lv = np.r_[np.arange(0, 256, 4), 255].astype(np.uint8)
    px = np.ascontiguousarray(np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(-1, 3))
    shift = int(np.int32(factor * 255).astype(np.uint8))
    im = Image.fromarray(px.reshape(1, -1, 3))
    h, s, v = im.convert("HSV").split()
    h = Image.fromarray(np.array(h, dtype=np.uint8) + np.int32(factor * 255).astype(np.uint8))
    want = np.asarray(Image.merge("HSV", (h, s, v)).convert("RGB")).reshape(-1, 3)
    got = core("hue_all", px, ctypes.c_int(shift))
    assert np.array_equal(got, want)
    if factor == 0.0:
        assert (want != px).any()


def test_luma_and_blend_equal_pil(core):
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, size=(1 << 16, 3), dtype=np.uint8)
    im = Image.fromarray(px.reshape(256, 256, 3))
    assert np.array_equal(core("luma_all", px), np.asarray(im.convert("L")).reshape(-1))
    for alpha in (0.0, 0.37, 1.0, 1.4, -0.2):
        want = np.asarray(ImageEnhance.Brightness(im).enhance(alpha)).reshape(-1)
        v = np.ascontiguousarray(px.reshape(-1))
        got = np.empty_like(v)
        core.lib.blend_all(np.zeros_like(v).ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
                           got.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(len(v)), ctypes.c_float(alpha))
        assert np.array_equal(got, want), alpha


def test_color_core_is_clean_under_address_and_undefined_sanitizers(core, triples):
    """A stand-alone program (its own ``main``) over the header, built with -fsanitize=address,undefined and run as a child
    process: every conversion of every input.  Its checksums equal those of the plain build checked against PIL above."""
    src, exe = str(core.dir / "color_core_san.cpp"), str(core.dir / "color_core_san")
    with open(src, "w") as f:
        f.write(_MAIN)
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime: " + r.stderr[-200:])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    a, b, _ = (int(t) for t in run.stdout.split())
    w = (triples.astype(np.uint64) * np.array([1, 3, 7], dtype=np.uint64)).sum(axis=1) + np.uint64(1)
    pack = np.array([65536, 256, 1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        assert a == int((((core("rgb2hsv_all", triples).astype(np.uint64) * pack).sum(axis=1)) * w).sum())
        assert b == int((((core("hsv2rgb_all", triples).astype(np.uint64) * pack).sum(axis=1)) * w).sum())
