"""Host side of the distillation loss (DistillClipLoss with a frozen teacher): the float64 oracle against the reference's
goldens, configuration, signatures, the header entry points, the gfx950 compile and the construction-time checks.  No GPU."""
import dataclasses
import glob
import inspect
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _distill_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("closs", "dloss", "gimg_c", "gtxt_c", "gscale_c", "gimg_d", "gtxt_d", "gscale_d")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, hydra_lite, losses, model_configs as mc, module
    return _lib, hydra_lite, losses, mc, module


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))


def w1_files(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "distill_w1_*.npz")))


def test_oracle_agrees_with_every_one_rank_golden(golden_dir):
    """Pins the closed forms (d D / d x = p_s - p_t included) before any kernel: 1e-12 relative, per array."""
    seen = set()
    for path in w1_files(golden_dir):
        z = np.load(path, allow_pickle=False)
        scales = json.loads(str(z["scales"]))
        for B, D, Dt, tag in json.loads(str(z["cases"])):
            s, st = scales[tag]
            f = [torch.from_numpy(z[f"B{B}_D{D}_{k}"]) for k in ("img", "txt", "timg", "ttxt")]
            assert f[0].shape == (B, D) and f[2].shape == (B, Dt)
            got = DO.distill_single(f[0], f[1], s, f[2], f[3], st)
            for k in KEYS:
                assert _rel(got[k], z[f"B{B}_D{D}_{tag}_{k}"]) <= 1e-12, (B, D, tag, k)
            assert np.isfinite(float(got["dloss"])) and float(got["dloss"]) >= 0.0
            seen.add((B, D, Dt, tag))
    want = {(B, D, Dt, tag) for B in (7, 12, 64, 300) for D, Dt in ((16, 16), (64, 48))
            for tag in ("s14_t14", "s100_t100", "s10_t100", "s100_t1")}
    assert seen == want


@pytest.mark.parametrize("layout", ["local", "global"])
def test_oracle_agrees_with_the_two_rank_golden(golden_dir, layout):
    z = np.load(os.path.join(golden_dir, "distill_w2.npz"), allow_pickle=False)
    f = [torch.from_numpy(z[k]) for k in ("img", "txt", "timg", "ttxt")]
    world = int(z["world"])
    got = DO.distill_ranks(f[0], f[1], float(z["scale"]), f[2], f[3], float(z["dist_scale"]), world, layout == "local")
    for r in range(world):
        for k in KEYS:
            assert _rel(got[r][k], z[f"r{r}_{layout}_{k}"]) <= 1e-12, (r, k)


def test_golden_files_are_small_fixtures(golden_dir):
    files = w1_files(golden_dir) + [os.path.join(golden_dir, "distill_w2.npz")]
    assert len(files) == 12
    for path in files:
        assert os.path.getsize(path) < (1 << 20), path
        assert not any("logit" in k for k in np.load(path).files), path       # features, never logits


def test_distill_experiment_composes_to_the_loss_and_a_teacher_block():
    _lib, H, losses, mc, module = _pkg()
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_distill_vitl14"])
    assert cfg["loss"]["_target_"] == "open_clip.loss.DistillClipLoss"
    assert H.TARGET_MAP["open_clip.loss.DistillClipLoss"] == "spatial_clip_amd.losses.DistillClipLoss"
    assert H.TARGET_MAP["open_clip.DistillClipLoss"] == "spatial_clip_amd.losses.DistillClipLoss"
    loss = H.instantiate(cfg["loss"])
    assert isinstance(loss, losses.DistillClipLoss) and isinstance(loss, losses.ClipLoss)
    assert loss.local_loss and loss.gather_with_grad
    model = cfg["model"]
    assert model["net"]["model_name"] == "ViT-B-16-gene" and cfg["data"]["batch_size"] == 256
    teacher = model["dist_net"]
    assert teacher["_target_"] == model["net"]["_target_"] and teacher["model_name"] == "ViT-L-14-gene"
    assert teacher["pretrained"] == "???" and teacher["n_genes"] == cfg["data"]["n_genes"]
    # the teacher / student pair of the experiment passes the input check; loss=distill alone carries no teacher block
    module.check_teacher_config(mc.get_model_config("ViT-B-16-gene", teacher["n_genes"]),
                                mc.get_model_config("ViT-L-14-gene", teacher["n_genes"]))
    assert "dist_net" not in H.compose("train.yaml", ["experiment=smoke_shards", "loss=distill"])["model"]


def test_distill_loss_signatures_match_the_reference():
    _lib, H, losses, mc, module = _pkg()
    ctor = list(inspect.signature(losses.DistillClipLoss.__init__).parameters)
    assert ctor == ["self", "local_loss", "gather_with_grad", "cache_labels", "rank", "world_size", "use_horovod"]
    fwd = inspect.signature(losses.DistillClipLoss.forward).parameters
    assert list(fwd) == ["self", "image_features", "text_features", "logit_scale", "dist_image_features",
                         "dist_text_features", "dist_logit_scale", "output_dict"]
    assert fwd["output_dict"].default is False and "logit_bias" not in fwd
    l = losses.DistillClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=3, world_size=8)
    assert l.rank == 0 and l.world_size == 1 and l.mode == "clip"       # read live from the (absent) process group
    assert module.loss_wants_teacher(l) and not module.loss_wants_teacher(losses.ClipLoss())
    assert not module.loss_wants_teacher(losses.SigLipLoss())


def test_header_declares_the_distill_entry_points():
    _lib, H, losses, mc, module = _pkg()
    decl = _lib.parse_header()
    for name, nargs in (("sc_distill_loss", 13), ("sc_axpby_scalars", 7), ("sc_distill_resident_max_g", 0)):
        assert name in decl and len(decl[name][1]) == nargs, name
    src = open(_lib.HEADER_PATH).read()
    assert "#define SC_DISTILL_RESIDENT_MAX_G 2048" in src


def test_library_validates_distill_arguments_without_a_gpu():
    _lib, H, losses, mc, module = _pkg()
    l = _lib.lib()
    assert l.sc_abi_version() == 1
    assert l.sc_distill_resident_max_g() == 2048
    for args, msg in (((None, None, 0, 8, 0, None, None, None, None, None, None, None, None), b"bad shape"),
                      ((None, None, 8, 4, 0, None, None, None, None, None, None, None, None), b"bad shape"),
                      ((None, None, 8, 16, 9, None, None, None, None, None, None, None, None), b"bad shape"),
                      ((None, None, 8, 16, 8, None, None, None, None, None, None, None, None), b"null argument")):
        assert l.sc_distill_loss(*args) < 0 and msg in l.sc_last_error(), args
    assert l.sc_axpby_scalars(None, None, None, None, None, 4, None) < 0 and b"sc_axpby_scalars" in l.sc_last_error()


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_distill_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "spatial-clip_amd", "csrc", "sc_loss.hip")
    out = str(tmp_path / "sc_loss.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "--cuda-device-only",
                        "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    for name in ("distill_rows_kernelILb1E", "distill_rows_kernelILb0E", "distill_finalize_kernel", "axpby_scalars_kernel"):
        assert name in asm, name
    # both row paths (register-resident and re-reading) must not spill: the kernel descriptor's private segment is 0 bytes
    for path in ("ILb1E", "ILb0E"):
        meta = asm[asm.index(f".amdhsa_kernel _ZN12_GLOBAL__N_119distill_rows_kernel{path}"):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert ".amdhsa_private_segment_fixed_size 0" in meta, path


def test_teacher_binding_is_checked_at_construction():
    _lib, H, losses, mc, module = _pkg()
    with pytest.raises(ValueError, match="needs a teacher"):
        module.check_teacher_binding(losses.DistillClipLoss(), False)
    for plain in (losses.ClipLoss(), losses.SigLipLoss(), losses.SpatialLoss()):
        with pytest.raises(ValueError, match="takes no dist_image_features"):
            module.check_teacher_binding(plain, True)
        module.check_teacher_binding(plain, False)
    module.check_teacher_binding(losses.DistillClipLoss(), True)
    # the module constructor runs the check before it touches either net
    with pytest.raises(ValueError, match="needs a teacher"):
        module.SpatialClipLitModule(None, losses.DistillClipLoss(), None, None)
    with pytest.raises(ValueError, match="takes no dist_image_features"):
        module.SpatialClipLitModule(None, losses.ClipLoss(), None, None, dist_net=object())
    assert "dist_net" in inspect.signature(module.SpatialClipLitModule.__init__).parameters


def test_teacher_inputs_must_match_the_students():
    _lib, H, losses, mc, module = _pkg()
    student = mc.get_model_config("ViT-B-16-gene", 2000)
    module.check_teacher_config(student, mc.get_model_config("ViT-L-14-gene", 2000))      # other width, patch, embed dim: fine
    with pytest.raises(ValueError, match="n_genes"):
        module.check_teacher_config(student, mc.get_model_config("ViT-L-14-gene", 3000))
    with pytest.raises(ValueError, match="image_size"):
        module.check_teacher_config(student, mc.get_model_config("ViT-L-14-336-gene", 2000))
    text_student = mc.get_model_config("ViT-B-16")
    module.check_teacher_config(text_student, mc.get_model_config("ViT-L-14"))
    with pytest.raises(ValueError, match="gene / text"):
        module.check_teacher_config(student, text_student)
    t = mc.get_model_config("ViT-L-14")
    with pytest.raises(ValueError, match="context_length"):
        module.check_teacher_config(text_student, dataclasses.replace(t, text=dataclasses.replace(t.text, context_length=64)))
    with pytest.raises(ValueError, match="vocab_size"):
        module.check_teacher_config(text_student, dataclasses.replace(t, text=dataclasses.replace(t.text, vocab_size=32000)))
