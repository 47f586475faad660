#!/usr/bin/env python3
"""Fixture for the extended device augmentation (sc_augment_tiles_ex): the reference's train transform with every field of
open_clip's AugmentationCfg, applied by PIL itself.

The transform is timm's ``create_transform`` (src/open_clip/transform.py:58-66,161-190).  timm / torchvision are not
installed in the build container, but on PIL tiles they do nothing except call PIL -- the calls are spelled out here, in
timm's order (``transforms_imagenet_train``):
  RandomResizedCropAndInterpolation -> img.crop(box).resize(size, BICUBIC)
  RandomHorizontalFlip / RandomVerticalFlip -> img.transpose(FLIP_LEFT_RIGHT) / img.transpose(FLIP_TOP_BOTTOM)
  RandomApply([ColorJitter], p=color_jitter_prob): the ops with a non-zero range, in a random order:
      brightness / contrast / saturation -> ImageEnhance.Brightness / Contrast / Color (img).enhance(factor)
      hue -> torchvision _functional_pil.adjust_hue: h, s, v = img.convert("HSV").split();
             h += np.int32(hue_factor * 255).astype(np.uint8) in uint8; Image.merge("HSV", (h, s, v)).convert("RGB")
  RandomGrayscale -> torchvision rgb_to_grayscale(img, 3): img.convert("L") stacked three times
  ToTensor -> float32 / 255;  Normalize -> (x - mean) / std
  RandomErasing(mode="const") -> boxes of 0.0 in the normalised tensor
The random draws are inputs of the kernel, so the fixture fixes them (row layout: include/spatial_clip_hip.h).
Run in the build container:  python tests/golden/make_golden_augment_ex.py   (writes tests/golden/augment_ex_pil.npz)"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

MEAN = np.array((0.48145466, 0.4578275, 0.40821073), dtype=np.float32)     # src/open_clip/constants.py:1-2
STD = np.array((0.26862954, 0.26130258, 0.27577711), dtype=np.float32)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
ROW = 36


def adjust_hue(im: Image.Image, hue_factor: float) -> Image.Image:
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h = np_h + np.int32(hue_factor * 255).astype(np.uint8)
    h = Image.fromarray(np_h, "L")
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def pil_pipeline(tile: np.ndarray, p: np.ndarray, S: int) -> np.ndarray:
    x0, y0, cw, ch = (int(v) for v in p[:4])
    im = Image.fromarray(tile).crop((x0, y0, x0 + cw, y0 + ch)).resize((S, S), Image.BICUBIC)
    if p[8] > 0.5:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if p[9] > 0.5:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    n = int(p[13])
    seq = [] if p[12] > 0.5 else (list(PERMS[int(p[7])]) if n == 0 else [int(c) for c in p[14:14 + n]])
    for op in seq:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(float(p[4]))
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(float(p[5]))
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(float(p[6]))
        else:
            im = adjust_hue(im, float(p[10]))
    if p[11] > 0.5:
        g = np.array(im.convert("L"), dtype=np.uint8)
        im = Image.fromarray(np.dstack([g, g, g]), "RGB")
    x = np.asarray(im, dtype=np.uint8).astype(np.float32) / np.float32(255.0)
    x = np.ascontiguousarray(((x - MEAN) / STD).transpose(2, 0, 1))
    for k in range(int(p[18])):
        top, left, h, w = (int(v) for v in p[20 + 4 * k:24 + 4 * k])
        x[:, top:top + h, left:left + w] = 0.0
    return x


def rows(rng, B, H, W):
    P = np.zeros((B, ROW), dtype=np.float32)
    for b in range(B):
        cw, ch = int(rng.integers(max(2, W // 3), W + 1)), int(rng.integers(max(2, H // 3), H + 1))
        P[b, 0:4] = (rng.integers(0, W - cw + 1), rng.integers(0, H - ch + 1), cw, ch)
        P[b, 4:7] = rng.uniform(0.6, 1.4, size=3).astype(np.float32)
    return P


def set_seq(p, seq):
    p[13] = len(seq)
    p[14:14 + len(seq)] = seq


def set_boxes(p, bx):
    p[18] = len(bx)
    for k, box in enumerate(bx):
        p[20 + 4 * k:24 + 4 * k] = box


def smooth_src(rng, B, H, W):          # low-frequency content (like stained tissue)
    base = rng.uniform(0, 255, size=(B, H // 4 + 2, W // 4 + 2, 3)).astype(np.float32)
    return np.stack([np.asarray(Image.fromarray(b.astype(np.uint8)).resize((W, H), Image.BILINEAR)) for b in base])


def primaries_tile():
    """16 x 16: a grey ramp (max == min), black, white, the six saturated primaries / secondaries (S = 255, H at every sixth
    of the circle, where the shifted H wraps) and a few dark / pale colours."""
    t = np.zeros((16, 16, 3), dtype=np.uint8)
    t[0:4] = (np.arange(16) * 17)[None, :, None]
    t[4:6, :8], t[4:6, 8:] = 0, 255
    cols = [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255), (255, 128, 0), (1, 0, 0)]
    for k, c in enumerate(cols):
        t[6:11, 2 * k:2 * k + 2] = c
    pale = [(254, 255, 255), (200, 199, 199), (3, 2, 1), (128, 0, 255), (255, 0, 128), (0, 128, 255), (17, 34, 51), (90, 90, 91)]
    for k, c in enumerate(pale):
        t[11:16, 2 * k:2 * k + 2] = c
    return t


HUE_BYTES = {0: 0.0, 1: 1.2 / 255, 127: 0.4999, 129: -0.5}      # shift byte -> a factor that truncates to it


def main():
    rng = np.random.default_rng(20261018)
    orders = list(itertools.permutations(range(4)))             # all 24 orders of the four ops
    z = {}

    # up (40 x 52 -> 64, smooth) and down (96 x 80 -> 32, noise): the 24 orders, random hue factors, flips, erase boxes
    for name, (B, H, W, S, smooth), my in (("up", (12, 40, 52, 64, True), orders[:12]),
                                           ("down", (12, 96, 80, 32, False), orders[12:])):
        src = smooth_src(rng, B, H, W) if smooth else rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
        P = rows(rng, B, H, W)
        for b in range(B):
            set_seq(P[b], my[b])
            P[b, 10] = np.float32(rng.uniform(-0.5, 0.5))
            P[b, 8], P[b, 9] = float(b % 2), float((b // 2) % 2)            # none, h, v, both flips
        set_boxes(P[1], [(0, 0, S // 3, S // 2)])                                         # one box in the corner
        set_boxes(P[2], [(S - 5, S - 9, 5, 9), (3, 4, 10, 6), (8, 6, 9, 12), (0, S - 2, S - 1, 2)])  # four: borders, overlap
        set_boxes(P[3], [(S // 2, 0, 1, S - 1)])                                          # one row high
        z[f"{name}_src"], z[f"{name}_params"], z[f"{name}_S"] = src.astype(np.uint8), P, np.int64(S)

    # same (48 x 48 -> 48, smooth): short sequences, the hue bytes, the switches
    B, H, W, S = 12, 48, 48, 48
    src, P = smooth_src(rng, B, H, W), rows(rng, B, H, W)
    set_seq(P[0], [3]); P[0, 10] = HUE_BYTES[0]                  # hue alone, shift 0: the round trip is not the identity
    set_seq(P[1], [3]); P[1, 10] = HUE_BYTES[1]
    set_seq(P[2], [1, 3]); P[2, 10] = HUE_BYTES[127]             # contrast then hue
    set_seq(P[3], [3, 1]); P[3, 10] = HUE_BYTES[129]             # hue then contrast
    set_seq(P[4], [2, 3, 0]); P[4, 10] = 0.1234                  # three ops
    set_seq(P[5], [1]); P[5, 9] = 1.0                            # one op, vertical flip alone
    P[6, 7] = 4                                                  # the 12-float rule (order code) with a vertical flip
    P[6, 9] = 1.0
    set_seq(P[7], [0, 3, 1, 2]); P[7, 10] = 0.3; P[7, 12] = 1.0  # jitter switched off: the sequence is ignored
    P[8, 12] = 1.0; P[8, 11] = 1.0                               # grayscale without jitter
    set_seq(P[9], [3, 2]); P[9, 10] = -0.2; P[9, 11] = 1.0       # grayscale after jitter
    P[10, 7] = 2; P[10, 8] = 1.0                                 # a 12-float row, zero-extended
    set_seq(P[11], [0, 1, 2, 3]); P[11, 10] = 0.05; P[11, 8] = P[11, 9] = 1.0
    set_boxes(P[11], [(10, 10, 20, 20), (20, 20, 27, 27)])       # overlapping, up to the last row / column
    z["same_src"], z["same_params"], z["same_S"] = src.astype(np.uint8), P, np.int64(S)

    # prim (16 x 16 -> 16): grey ramp, black, white, saturated primaries; full tile, so the pixels reach the ops unchanged
    B, S = 8, 16
    src = np.stack([primaries_tile()] * B)
    P = np.zeros((B, ROW), dtype=np.float32)
    P[:, 2:4], P[:, 4:7] = 16, 1.0
    for b, byte in enumerate((0, 1, 127, 129)):
        set_seq(P[b], [3]); P[b, 10] = HUE_BYTES[byte]
    set_seq(P[4], [3]); P[4, 10] = np.float32(rng.uniform(-0.5, 0.5))
    set_seq(P[5], [2, 3, 1, 0]); P[5, 4:7] = (1.3, 0.7, 1.4); P[5, 10] = 0.45
    set_seq(P[6], [3, 0]); P[6, 4] = 0.5; P[6, 10] = -0.25; P[6, 11] = 1.0
    P[7, 12] = 1.0; set_boxes(P[7], [(0, 0, 15, 15)])
    z["prim_src"], z["prim_params"], z["prim_S"] = src.astype(np.uint8), P, np.int64(S)

    for name in ("up", "down", "same", "prim"):
        src, P, S = z[f"{name}_src"], z[f"{name}_params"], int(z[f"{name}_S"])
        z[f"{name}_out"] = np.stack([pil_pipeline(src[b], P[b], S) for b in range(len(src))])
    for byte, f in HUE_BYTES.items():
        assert int(np.int32(float(np.float32(f)) * 255).astype(np.uint8)) == byte, (byte, f)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_ex_pil.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), {k: v.shape for k, v in z.items()})


if __name__ == "__main__":
    main()
