"""Host side of the sigmoid (SigLIP) loss and the learnable logit bias: configuration, parameter layout, the header entry
point and its gfx950 compile.  No GPU needed."""
import dataclasses
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, hydra_lite, losses, model_configs as mc, params
    return _lib, hydra_lite, losses, mc, params


def test_siglip_experiment_composes_to_the_sigmoid_loss_and_a_bias_net():
    _lib, H, losses, mc, params = _pkg()
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_siglip"])
    assert cfg["loss"]["_target_"] == "open_clip.loss.SigLipLoss" and cfg["loss"]["dist_impl"] == "bidir"
    assert H.TARGET_MAP["open_clip.loss.SigLipLoss"] == "spatial_clip_amd.losses.SigLipLoss"
    assert H.TARGET_MAP["open_clip.SigLipLoss"] == "spatial_clip_amd.losses.SigLipLoss"
    loss = H.instantiate(cfg["loss"])
    assert isinstance(loss, losses.SigLipLoss) and loss.dist_impl == "bidir"
    net = cfg["model"]["net"]
    assert net["model_name"] == "ViT-B-16-gene" and cfg["data"]["batch_size"] == 256
    assert float(net["init_logit_bias"]) == -10.0 and abs(float(net["init_logit_scale"]) - 2.302585092994046) < 1e-12
    # loss=siglip on the default net: no bias key at all (bias None, as the reference allows)
    plain = H.compose("train.yaml", ["experiment=smoke_shards", "loss=siglip"])
    assert "init_logit_bias" not in plain["model"]["net"]


def test_siglip_loss_constructor():
    _lib, H, losses, mc, params = _pkg()
    for impl in ("bidir", "shift", "reduce", "gather"):
        assert losses.SigLipLoss(dist_impl=impl).dist_impl == impl
    assert losses.SigLipLoss().dist_impl == "bidir"
    with pytest.raises(AssertionError):
        losses.SigLipLoss(dist_impl="ring")
    l = losses.SigLipLoss(cache_labels=True, rank=3, world_size=8)
    assert l.rank == 0 and l.world_size == 1           # read live from the (absent) process group
    assert tuple(l.skip_gather) == ("image",)


def test_logit_bias_param_only_when_configured():
    _lib, H, losses, mc, params = _pkg()
    for name in ("ViT-B-16-gene", "ViT-B-16"):
        cfg = mc.get_model_config(name)
        assert cfg.init_logit_bias is None
        base = params.build_specs(cfg)
        assert "logit_bias" not in [s.name for s in base]
        biased = params.build_specs(dataclasses.replace(cfg, init_logit_bias=-10.0))
        assert [s.name for s in biased] == [s.name for s in base] + ["logit_bias"]
        for a, b in zip(base, biased):          # the existing flat layout is untouched
            assert (a.name, a.shape, a.offset, a.init) == (b.name, b.shape, b.offset, b.init)
        lb = biased[-1]
        assert lb.shape == () and lb.init == "const:-10.0" and lb.offset >= base[-1].offset + 1


def test_header_declares_the_siglip_entry_point():
    _lib, H, losses, mc, params = _pkg()
    decl = _lib.parse_header()
    assert "sc_siglip_loss" in decl
    restype, args = decl["sc_siglip_loss"]
    assert len(args) == 12


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_siglip_kernel_compiles_for_gfx950(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "spatial-clip_amd", "csrc", "sc_loss.hip")
    out = str(tmp_path / "sc_loss.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "--cuda-device-only",
                        "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    assert "siglip_rows_kernel" in asm and "siglip_finalize_kernel" in asm
