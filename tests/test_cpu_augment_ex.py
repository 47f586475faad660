"""CPU checks of the extended device augmentation (sc_augment_tiles_ex): the numpy restatement of the whole transform
against the fixture PIL itself wrote, what the fixture covers, the parameter draws (``shards.draw_aug_params_ex``) and the
settings the data module refuses.  The kernel is checked in tests/test_gpu_augment_ex.py."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import _lib, hydra_lite, ops, shards
from tests import _augment_ex_oracle as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("up", "down", "same", "prim")
LEGACY_CFG = {"scale": [0.9, 1.0], "ratio": [0.75, 1.333], "color_jitter": 0.2, "use_timm": True}
FULL_CFG = {"scale": [0.5, 1.0], "ratio": [0.75, 1.333], "color_jitter": [0.3, 0.2, 0.4, 0.05], "color_jitter_prob": 0.8,
            "gray_scale_prob": 0.2, "re_prob": 0.5, "re_count": 3, "use_timm": True, "vflip": 0.5}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "augment_ex_pil.npz"))


def test_oracle_equals_pil_fixture_bitwise(fixture):
    for name in CASES:
        src, P, want, S = (fixture[f"{name}_{k}"] for k in ("src", "params", "out", "S"))
        for b in range(len(src)):
            got = X.augment_ex(src[b], P[b], int(S), shards.OPENAI_MEAN, shards.OPENAI_STD)
            assert got.dtype == np.float32 and np.array_equal(got, want[b]), (name, b, float(np.abs(got - want[b]).max()))


def test_fixture_covers_what_it_promises(fixture):
    P = np.concatenate([fixture[f"{n}_params"] for n in CASES])
    assert P.shape[1] == ops.AUG_ROW == shards.AUG_ROW
    seqs = [tuple(int(c) for c in p[14:14 + int(p[13])]) for p in P if p[12] < 0.5]
    assert set(itertools.permutations(range(4))) <= set(seqs)                  # all 24 orders of the four ops
    assert {1, 2, 3} <= {len(s) for s in seqs} and () in seqs                  # short sequences, the 12-float rule
    shifts = {X.hue_shift(p[10]) for p in P if 3 in p[14:14 + int(p[13])]}
    assert {0, 1, 127, 129} <= shifts and len(shifts) > 6
    assert any(s.index(3) < s.index(1) for s in seqs if 1 in s and 3 in s)      # hue before contrast ...
    assert any(s.index(3) > s.index(1) for s in seqs if 1 in s and 3 in s)      # ... and after
    assert (P[:, 12] > 0.5).any()                                              # jitter switched off
    assert ((P[:, 11] > 0.5) & (P[:, 12] > 0.5)).any() and ((P[:, 11] > 0.5) & (P[:, 12] < 0.5)).any()
    assert {(0, 0), (0, 1), (1, 0), (1, 1)} <= {(int(p[8]), int(p[9])) for p in P}
    assert {0, 1, 4} <= {int(p[18]) for p in P}
    # shift 0 still changes pixels (the HSV round trip is lossy)
    src, p, S = fixture["prim_src"][0], fixture["prim_params"][0].copy(), int(fixture["prim_S"])
    with_hue = X.augment_ex_u8(src, p, S)
    p[12] = 1.0
    assert (with_hue != X.augment_ex_u8(src, p, S)).any()
    for name in CASES:                                                         # every box is inside its output
        S = int(fixture[f"{name}_S"])
        for p in fixture[f"{name}_params"]:
            for top, left, h, w in X.boxes(p):
                assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= S and left + w <= S


def test_header_declares_the_new_entry_with_types_the_binding_knows():
    restype, argtypes = _lib.parse_header()["sc_augment_tiles_ex"]
    assert len(argtypes) == 11 and "sc_augment_tiles" in _lib.parse_header()
    assert "#define SC_AUG_ROW %d" % ops.AUG_ROW in open(_lib.HEADER_PATH).read()


@pytest.mark.parametrize("cfg", [LEGACY_CFG, {"scale": [0.3, 1.0], "color_jitter": 0.4, "hflip": 0.3},
                                 {"scale": [0.9, 1.0]}, {"color_jitter": 0.0, "use_timm": False}])
def test_legacy_config_draws_equal_draw_aug_params_bit_for_bit(cfg):
    """Same generator state -> the same twelve columns, the same number of draws consumed, nothing in the new columns."""
    r0, r1 = np.random.default_rng(11), np.random.default_rng(11)
    old = shards.draw_aug_params(64, 224, 200, cfg, r0)
    new = shards.draw_aug_params_ex(64, 224, 200, cfg, r1, out_size=224)
    assert new.shape == (64, shards.AUG_ROW) and new.dtype == torch.float32 and not new.is_cuda
    assert np.array_equal(old.numpy().view(np.uint32), new[:, :12].numpy().view(np.uint32))
    assert not new[:, 12:].any()
    assert r0.bit_generator.state == r1.bit_generator.state


def test_a_feature_that_is_off_draws_nothing():
    base = shards.draw_aug_params_ex(32, 64, 64, LEGACY_CFG, np.random.default_rng(5), out_size=32)
    off = dict(LEGACY_CFG, vflip=0.0, gray_scale_prob=0.0, re_prob=0.0, re_count=2, color_jitter_prob=None)
    assert torch.equal(base, shards.draw_aug_params_ex(32, 64, 64, off, np.random.default_rng(5), out_size=32))


def test_new_draws_ranges_and_frequencies():
    B, H, W, S = 2000, 64, 80, 48
    P = shards.draw_aug_params_ex(B, H, W, FULL_CFG, np.random.default_rng(7), out_size=S).numpy()
    tol = 4 * 0.5 / math.sqrt(B)                          # four standard deviations of a frequency over B samples
    assert abs(P[:, 8].mean() - 0.5) < tol and abs(P[:, 9].mean() - 0.5) < tol
    assert set(np.unique(P[:, [8, 9, 11, 12]])) <= {0.0, 1.0}
    assert abs(P[:, 12].mean() - 0.2) < tol and abs(P[:, 11].mean() - 0.2) < tol
    on = P[P[:, 12] < 0.5]
    assert (on[:, 13] == 4).all()
    assert all(sorted(r[14:18].tolist()) == [0, 1, 2, 3] for r in on)
    first = np.bincount(on[:, 14].astype(int), minlength=4) / len(on)
    assert np.abs(first - 0.25).max() < tol                # every op leads equally often
    assert len({tuple(r[14:18]) for r in on}) == 24
    for col, j in ((4, 0.3), (5, 0.2), (6, 0.4)):
        assert on[:, col].min() >= np.float32(1 - j) and on[:, col].max() <= np.float32(1 + j)
        assert abs(on[:, col].mean() - 1.0) < 4 * (2 * j / math.sqrt(12)) / math.sqrt(len(on))
    assert np.abs(on[:, 10]).max() <= np.float32(0.05) and on[:, 10].min() < -0.04 and on[:, 10].max() > 0.04
    off = P[P[:, 12] > 0.5]                                 # a skipped jitter leaves identity factors and no sequence
    assert (off[:, 4:7] == 1).all() and not off[:, [7, 10, 13, 14, 15, 16, 17]].any()
    erased = P[:, 18] > 0
    assert abs(erased.mean() - 0.5) < tol and set(np.unique(P[:, 18])) <= {0.0, 1.0, 2.0, 3.0}
    assert (P[erased, 18] == 3).mean() > 0.95              # ten attempts per box almost never all fail
    lo, hi = 0.02 * S * S / 3, S * S / 3 / 3                # timm: area fraction U(0.02, 1/3) of the image / count
    for p in P[erased]:
        for top, left, h, w in X.boxes(p):
            assert 0 <= top and 0 <= left and 1 <= h < S and 1 <= w < S and top + h <= S and left + w <= S
            # h = round(sqrt(area * ar)), w = round(sqrt(area / ar)): each side is at most 0.5 off its real value
            assert (h - 0.5) * (w - 0.5) <= hi and (h + 0.5) * (w + 0.5) >= lo
            assert 0.3 * 0.3 <= ((h + 0.5) / (w - 0.5)) * ((h + 0.5) / (w - 0.5)) or h <= 2 or w <= 2
    assert not P[~erased, 18:].any()


def test_color_jitter_forms():
    rng = np.random.default_rng(3)
    P3 = shards.draw_aug_params_ex(200, 32, 32, {"color_jitter": [0.4, 0.0, 0.2]}, rng, out_size=32).numpy()
    assert (P3[:, 13] == 2).all() and all(sorted(r[14:16].tolist()) == [0, 2] for r in P3)      # a zero range is absent
    assert (P3[:, 5] == 1).all() and not P3[:, 10].any() and P3[:, 4].std() > 0.1
    P4 = shards.draw_aug_params_ex(200, 32, 32, {"color_jitter": [0, 0, 0, 0.5]}, rng, out_size=32).numpy()
    assert (P4[:, 13] == 1).all() and (P4[:, 14] == 3).all() and np.abs(P4[:, 10]).max() <= 0.5
    assert {X.hue_shift(v) for v in P4[:, 10]} - set(range(0, 128)) - set(range(129, 256)) == set()
    Ps = shards.draw_aug_params_ex(50, 32, 32, {"color_jitter": 0.3}, rng, out_size=32).numpy()
    assert not Ps[:, 13].any() and set(np.unique(Ps[:, 7])) <= set(range(6))                     # scalar: no hue (timm)
    P0 = shards.draw_aug_params_ex(20, 32, 32, {"color_jitter": [0, 0, 0]}, rng, out_size=32).numpy()
    assert (P0[:, 12] == 1).all()


def test_evaluation_rows_stay_the_identity():
    for cfg in (FULL_CFG, LEGACY_CFG, None):
        r = np.random.default_rng(1)
        state = r.bit_generator.state
        P = shards.draw_aug_params_ex(5, 24, 30, cfg, r, train=False, out_size=24)
        want = np.zeros((5, shards.AUG_ROW), dtype=np.float32)
        want[:, 2], want[:, 3], want[:, 4:7] = 30, 24, 1.0
        assert np.array_equal(P.numpy(), want) and r.bit_generator.state == state
        assert np.array_equal(P[:, :12].numpy(), shards.draw_aug_params(5, 24, 30, cfg, r, train=False).numpy())


@pytest.mark.parametrize("bad,match", [
    ({"color_jitter": [0.2, 0.2, 0.2, 0.6]}, "hue"), ({"color_jitter": [0.2, 0.2, 0.2, -0.1]}, "hue"),
    ({"color_jitter": [0.2, 0.2]}, "color_jitter"), ({"color_jitter": [0.2, -0.2, 0.2]}, "negative"),
    ({"color_jitter_prob": 1.5}, "color_jitter_prob"), ({"gray_scale_prob": -0.1}, "gray_scale_prob"),
    ({"grayscale_prob": 2}, "grayscale_prob"), ({"re_prob": 1.01}, "re_prob"), ({"vflip": 7}, "vflip"),
    ({"hflip": -1}, "hflip"), ({"re_count": 0}, "re_count"), ({"re_count": 5}, "re_count"),
    ({"re_mode": "pixel"}, "re_mode"), ({"auto_augment": "rand-m9-mstd0.5"}, "not available on the device"),
    ({"gaussian_blur_prob": 0.1}, "not available on the device"),
    ({"gray_scale_prob": 0.1, "grayscale_prob": 0.2}, "synonyms")])
def test_the_data_module_refuses_what_the_device_path_cannot_do(bad, match):
    with pytest.raises(ValueError, match=match):
        shards.ShardedSpatialDataModule(data_dir="/nonexistent", aug_cfg=dict(LEGACY_CFG, **bad))


def test_the_data_module_accepts_every_supported_key():
    ok = dict(FULL_CFG, grayscale_prob=0.2, re_mode="const", auto_augment=None, gaussian_blur_prob=None, hflip=0.5,
              _target_="open_clip.AugmentationCfg")
    shards.ShardedSpatialDataModule(data_dir="/nonexistent", aug_cfg=ok)
    assert shards.parse_aug_cfg({"grayscale_prob": 0.3})["gray"] == shards.parse_aug_cfg({"gray_scale_prob": 0.3})["gray"] == 0.3
    shards.ShardedSpatialDataModule(data_dir="/nonexistent", aug_cfg=None)


def test_he_aug_experiment_reaches_the_data_module(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    cfg = hydra_lite.compose("train.yaml", ["experiment=vitb16_gene_b256_he_aug"])
    aug = cfg.model.net.aug_cfg
    assert len(aug.color_jitter) == 4 and 0 < aug.color_jitter[3] <= 0.1 and aug.vflip == 0.5 and aug.re_prob > 0
    dm = hydra_lite.instantiate(cfg.data)
    assert isinstance(dm, shards.ShardedSpatialDataModule)
    c = shards.parse_aug_cfg(dm.aug_cfg)
    assert c["jitter"] == tuple(aug.color_jitter) and c["vflip"] == 0.5 and c["re_prob"] == aug.re_prob and not c["legacy_jitter"]


def test_the_entry_checks_rows_before_it_touches_the_device():
    """The rows are host memory and the checks run first, so a refused row is refused on a machine without a GPU too."""
    import ctypes
    l = _lib.lib()
    m3, s3 = (ctypes.c_float * 3)(*shards.OPENAI_MEAN), (ctypes.c_float * 3)(*shards.OPENAI_STD)

    def call(P, stride=ops.AUG_ROW):
        rc = l.sc_augment_tiles_ex(None, len(P), 24, 24, P.data_ptr(), stride, None, 32, ctypes.cast(m3, ctypes.c_void_p),
                                   ctypes.cast(s3, ctypes.c_void_p), None)
        return rc, l.sc_last_error().decode()

    def row():
        return shards.draw_aug_params_ex(3, 24, 24, None, np.random.default_rng(0), train=False)
    P = row()
    rc, msg = call(P, 12)
    assert rc < 0 and "stride" in msg
    P = row(); P[1, 18] = 5
    rc, msg = call(P)
    assert rc < 0 and "row 1" in msg and "boxes" in msg
    P = row(); P[2, 18] = 1; P[2, 20:24] = torch.tensor([0.0, 20.0, 4.0, 13.0])
    rc, msg = call(P)
    assert rc < 0 and "row 2" in msg and "not inside" in msg
    P = row(); P[0, 13] = 2; P[0, 14:16] = torch.tensor([0.0, 4.0])
    rc, msg = call(P)
    assert rc < 0 and "row 0" in msg and "op code" in msg
