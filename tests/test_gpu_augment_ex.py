"""sc_augment_tiles_ex on the device: bit-exact against the fixture PIL itself wrote (tests/golden/augment_ex_pil.npz) and
against the numpy restatement on drawn rows, the 12-float rows through the new entry, the rows it refuses, and one pass
of the shards loader with the H&E experiment's aug_cfg."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mods():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops, shards
    return ops, shards


def test_augment_tiles_ex_equals_pil_fixture_bitwise():
    ops, shards = _mods()
    z = np.load(os.path.join(GOLDEN, "augment_ex_pil.npz"))
    for name in ("up", "down", "same", "prim"):
        src, P, want, S = z[name + "_src"], z[name + "_params"], z[name + "_out"], int(z[name + "_S"])
        out = ops.augment_tiles_ex(torch.from_numpy(src).cuda(), torch.from_numpy(P), S, shards.OPENAI_MEAN,
                                   shards.OPENAI_STD).cpu().numpy()
        bad = [b for b in range(len(src)) if not np.array_equal(out[b].view(np.uint32), want[b].view(np.uint32))]
        assert not bad, (name, bad, float(np.abs(out - want).max()))


def test_drawn_rows_with_everything_on_equal_the_numpy_restatement():
    ops, shards = _mods()
    from tests import _augment_ex_oracle as X
    B, H, W, S = 12, 40, 52, 32
    cfg = {"scale": [0.4, 1.0], "ratio": [0.75, 1.333], "color_jitter": [0.4, 0.4, 0.4, 0.5], "color_jitter_prob": 0.9,
           "gray_scale_prob": 0.25, "re_prob": 0.9, "re_count": 4, "use_timm": True, "vflip": 0.5}
    P = shards.draw_aug_params_ex(B, H, W, cfg, np.random.default_rng(21), out_size=S)
    assert (P[:, 18] > 0).any() and (P[:, 13] == 4).any() and P[:, 9].any() and P[:, 11].any()
    src = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    out = ops.augment_tiles_ex(src.cuda(), P, S, shards.OPENAI_MEAN, shards.OPENAI_STD).cpu().numpy()
    for b in range(B):
        want = X.augment_ex(src[b].numpy(), P[b].numpy(), S, shards.OPENAI_MEAN, shards.OPENAI_STD)
        assert np.array_equal(out[b].view(np.uint32), want.view(np.uint32)), (b, float(np.abs(out[b] - want).max()))
        for top, left, h, w in X.boxes(P[b].numpy()):
            assert not out[b][:, top:top + h, left:left + w].any()


def test_twelve_float_rows_through_the_new_entry_equal_sc_augment_tiles():
    ops, shards = _mods()
    z = np.load(os.path.join(GOLDEN, "augment_pil.npz"))
    for name in ("up", "down", "same"):
        src, P12, want, S = z[name + "_src"], z[name + "_params"], z[name + "_out"], int(z[name + "_S"])
        P = np.zeros((len(P12), ops.AUG_ROW + 3), dtype=np.float32)          # a wider stride than the row is fine
        P[:, :12] = P12
        dsrc = torch.from_numpy(src).cuda()
        old = ops.augment_tiles(dsrc, torch.from_numpy(P12).cuda(), S, shards.OPENAI_MEAN, shards.OPENAI_STD)
        new = ops.augment_tiles_ex(dsrc, torch.from_numpy(P), S, shards.OPENAI_MEAN, shards.OPENAI_STD)
        assert torch.equal(old.view(torch.int32), new.view(torch.int32))
        assert np.array_equal(new.cpu().numpy(), want)
        # the same rows next to one row that uses a new feature run the extended kernel: still the same bytes
        P[-1, 9] = 1.0
        mixed = ops.augment_tiles_ex(dsrc, torch.from_numpy(P), S, shards.OPENAI_MEAN, shards.OPENAI_STD)
        assert torch.equal(mixed[:-1].view(torch.int32), old[:-1].view(torch.int32))
        assert torch.equal(mixed[-1].view(torch.int32), old[-1].flip(1).view(torch.int32))


def _set(col, val):
    def f(p):
        p[col] = val
    return f


def _box(k, n, box):
    def f(p):
        p[18] = n
        p[20 + 4 * k:24 + 4 * k] = torch.tensor(box, dtype=torch.float32)
    return f


_REJECTED = {
    "five boxes": _set(18, 5.0), "a negative box count": _set(18, -1.0),
    "a box past the right edge": _box(0, 1, (0, 20, 4, 13)), "a box past the bottom": _box(1, 2, (30, 0, 3, 4)),
    "a box at a negative row": _box(0, 1, (-1, 0, 4, 4)), "an empty box": _box(0, 1, (3, 3, 0, 4)),
    "op code 4": lambda p: p.__setitem__(slice(13, 16), torch.tensor((2.0, 0.0, 4.0))),
    "op code -1": lambda p: p.__setitem__(slice(13, 15), torch.tensor((1.0, -1.0))),
    "five ops": _set(13, 5.0), "an op used twice": lambda p: p.__setitem__(slice(13, 16), torch.tensor((2.0, 1.0, 1.0))),
    "a hue factor beyond 0.5": _set(10, 0.75)}


@pytest.mark.parametrize("why", list(_REJECTED))
def test_rejected_rows_return_an_error_and_leave_the_output_untouched(why):
    ops, shards = _mods()
    from spatial_clip_amd import _lib
    B, S = 3, 32
    src = torch.randint(0, 256, (B, 24, 24, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    P = shards.draw_aug_params_ex(B, 24, 24, None, np.random.default_rng(0), train=False)
    for k in range(4):
        P[1, 20 + 4 * k:24 + 4 * k] = torch.tensor([1.0, 1.0, 2.0, 2.0])      # valid boxes behind the count
    _REJECTED[why](P[1])
    out = torch.full((B, 3, S, S), -7.0, device="cuda")
    with pytest.raises(_lib.SpatialClipHipError, match="row 1"):
        ops.augment_tiles_ex(src, P, S, shards.OPENAI_MEAN, shards.OPENAI_STD, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), why
    with pytest.raises(_lib.SpatialClipHipError, match="stride"):            # a 12-float stride is not an extended row
        m3, s3 = (ctypes.c_float * 3)(*shards.OPENAI_MEAN), (ctypes.c_float * 3)(*shards.OPENAI_STD)
        _lib.check(_lib.lib().sc_augment_tiles_ex(src.data_ptr(), B, 24, 24, P.data_ptr(), 12, out.data_ptr(), S,
                                                  ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), None),
                   "sc_augment_tiles_ex")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_shards_loader_with_the_he_experiment_aug_cfg(tmp_path, monkeypatch):
    ops, shards = _mods()
    from spatial_clip_amd import data, hydra_lite
    from tests import _augment_ex_oracle as X
    from tests.test_cpu_pipeline import _make_shards
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    aug = dict(hydra_lite.compose("train.yaml", ["experiment=vitb16_gene_b256_he_aug"]).model.net.aug_cfg)
    aug["re_prob"], aug["re_count"] = 0.6, 2                   # more boxes than the experiment's 0.25 x 1 in 72 tiles
    root = _make_shards(str(tmp_path / "processed"), slides=2, tiles=36, px=32)
    genes = [f"GENE{i}" for i in range(36)] + ["ACTB", "B2M", "FTL", "MALAT1"]
    dm = data.SpatialClipDataModule(data_dir=root, k_neighbors=4, batch_size=12, dataset_format="shards_v1",
                                    splits={"train": ["SAMPLE_A", "SAMPLE_B"], "val": ["SAMPLE_B"]}, image_size=32,
                                    gene_vocab=genes, aug_cfg=aug, centers_per_batch=3, max_neighbors_per_center=3)
    dm.preprocess_fn, dm.tokenizer = (lambda x: x), (lambda x: x)
    dm.setup("fit")
    batches = list(dm.train_dataloader())
    assert len(batches) == 72 // 12
    rng = np.random.default_rng([dm.seed, 0, 0, 0])           # the loader's generator: (seed, epoch, rank, train)
    boxes = 0
    for b in batches:
        img = b["images"]
        assert tuple(img.shape) == (12, 3, 32, 32) and img.is_cuda and img.dtype == torch.float32
        assert tuple(b["texts"].shape) == (12, len(genes)) and b["neighbor_tile_ids"].shape == (12, 4)
        assert torch.equal(b["image_tile_ids"], b["text_tile_ids"]) and len(b["raw_text"]) == 12
        assert bool(torch.isfinite(img).all())
        P = shards.draw_aug_params_ex(12, 32, 32, aug, rng, True, 32).numpy()
        zero = (img == 0).all(dim=1).cpu().numpy()
        assert np.array_equal(zero, (img == 0).any(dim=1).cpu().numpy())         # a box clears all three channels
        for k in range(12):
            want = np.zeros((32, 32), dtype=bool)
            for top, left, h, w in X.boxes(P[k]):
                want[top:top + h, left:left + w] = True
                boxes += 1
            assert np.array_equal(zero[k], want), k           # exactly 0.0 inside the boxes, nowhere else
    assert boxes > 10
    val = list(dm.val_dataloader())                           # evaluation: the tile as it is, normalised
    assert len(val) == 3 and not bool((val[0]["images"] == 0).any())
