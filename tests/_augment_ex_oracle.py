"""TEST INFRASTRUCTURE -- numpy restatement of the whole extended train transform (``sc_augment_tiles_ex``): PIL's resize /
blend / luma from oracle/augment_oracle.py, plus vertical flip, the hue op (PIL's RGB -> HSV -> RGB round trip, the mixed
float32 / float64 arithmetic of libImaging/Convert.c), the jitter switch, grayscale and erase boxes.  Pinned byte for
byte by tests/golden/augment_ex_pil.npz, which PIL itself produced (tests/golden/make_golden_augment_ex.py).  Row layout:
include/spatial_clip_hip.h."""
import numpy as np

from oracle import augment_oracle as A

f32, f64 = np.float32, np.float64


def rgb_to_hsv(v: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [..., 3]: ``Image.convert("HSV")``."""
    r, g, b = (v[..., k].astype(np.int64) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                              (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32))).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip(np.nan_to_num(h.astype(f64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip(np.nan_to_num(s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    flat = maxc == minc
    return np.stack([np.where(flat, 0, H), np.where(flat, 0, S), maxc], axis=-1).astype(np.uint8)


def _round8(x32: np.ndarray) -> np.ndarray:          # C round() on a non-negative float32, clipped to a byte
    return np.clip(np.floor(x32.astype(f64) + 0.5).astype(np.int64), 0, 255)


def hsv_to_rgb(v: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [..., 3]: ``Image.merge("HSV", ...).convert("RGB")``."""
    H, S, V = (v[..., k].astype(np.int64) for k in range(3))
    x = H.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(x).astype(np.int64)
    f = (x - i.astype(f32).astype(f64)).astype(f32)
    fs = (S.astype(f64) / 255.0).astype(f32)
    Vd = V.astype(f64)
    p = _round8((Vd * (1.0 - fs.astype(f64))).astype(f32))
    q = _round8((Vd * (1.0 - fs.astype(f64) * f.astype(f64))).astype(f32))
    t = _round8((Vd * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))).astype(f32))
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    sel = i % 6
    out = np.stack([np.choose(sel, [tr[c] for tr in table]) for c in range(3)], axis=-1)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.uint8)


def hue_shift(factor) -> int:
    """What torchvision's adjust_hue adds to H: np.int32(hue_factor * 255).astype(np.uint8), the factor being the row's
    float32 value."""
    return int(np.int32(float(f32(factor)) * 255.0)) & 255


def hue(v: np.ndarray, factor) -> np.ndarray:
    hsv = rgb_to_hsv(v)
    hsv[..., 0] = hsv[..., 0] + np.uint8(hue_shift(factor))           # uint8: wraps
    return hsv_to_rgb(hsv)


def jitter_sequence(p: np.ndarray):
    if p[12] > 0.5:
        return []
    n = int(p[13])
    return list(A.PERMS[int(p[7])]) if n == 0 else [int(c) for c in p[14:14 + n]]


def augment_ex_u8(tile: np.ndarray, p: np.ndarray, S: int) -> np.ndarray:
    """One sample: uint8 [H, W, 3] + its extended row -> the 8-bit image in front of ToTensor, uint8 [S, S, 3]."""
    x0, y0, cw, ch = (int(c) for c in p[:4])
    v = A.resize_bicubic_u8(tile[y0:y0 + ch, x0:x0 + cw], S)
    if p[8] > 0.5:
        v = v[:, ::-1]
    if p[9] > 0.5:
        v = v[::-1]
    for op in jitter_sequence(p):
        if op == 0:
            v = A.blend(np.zeros_like(v), v, p[4])
        elif op == 1:
            m = int(float(A.luma(v).sum()) / (S * S) + 0.5)
            v = A.blend(np.full_like(v, m), v, p[5])
        elif op == 2:
            v = A.blend(np.repeat(A.luma(v)[..., None], 3, axis=-1).astype(np.uint8), v, p[6])
        else:
            v = hue(v, p[10])
    if p[11] > 0.5:
        v = np.repeat(A.luma(v)[..., None], 3, axis=-1).astype(np.uint8)
    return np.ascontiguousarray(v)


def boxes(p: np.ndarray):
    return [tuple(int(c) for c in p[20 + 4 * k:24 + 4 * k]) for k in range(int(p[18]))]


def augment_ex(tile: np.ndarray, p: np.ndarray, S: int, mean, std) -> np.ndarray:
    """-> the normalised fp32 [3, S, S] tensor with the erase boxes zeroed."""
    x = A.to_tensor_normalize(augment_ex_u8(tile, p, S), mean, std)
    for top, left, h, w in boxes(p):
        x[:, top:top + h, left:left + w] = 0.0
    return x
