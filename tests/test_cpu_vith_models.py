"""ViT-H towers (width 1280 = 16 heads of 80): the ViT-H-14 / ViT-H-14-quickgelu / ViT-H-16 names, their parameter
layouts against the reference's state_dicts, the names that stay unknown, and the construction-time check of the head dims
and lengths the attention kernels take."""
import json
import os

import pytest

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import model_configs as mc
from spatial_clip_amd import params


def _specs(cfg):
    return {s.name: list(s.shape) for s in params.build_specs(cfg)}


def _manifest(golden_dir, which="state_dict_manifest_vith.json"):
    return json.load(open(os.path.join(golden_dir, which)))


@pytest.mark.parametrize("name,patch,tokens", [("ViT-H-14", 14, 257), ("ViT-H-14-quickgelu", 14, 257), ("ViT-H-16", 16, 197)])
def test_vith_names_resolve(name, patch, tokens):
    cfg = mc.get_model_config(name)
    v, t = cfg.vision, cfg.text
    assert cfg.embed_dim == 1024
    assert (v.image_size, v.patch_size, v.width, v.layers, v.head_width, v.heads, v.tokens, v.mlp_ratio) == \
        (224, patch, 1280, 32, 80, 16, tokens, 4.0)
    assert (t.context_length, t.vocab_size, t.width, t.heads, t.layers) == (77, 49408, 1024, 16, 24)
    assert cfg.gene is None and cfg.quick_gelu == name.endswith("-quickgelu")
    mc.check_attention_support(cfg)
    assert name in mc.list_models()
    for suffix, kind in (("-gene", "mlp"), ("-genetr", "transformer")):
        g = mc.get_model_config(name + suffix)
        assert g.text is None and g.gene is not None and g.gene.kind == kind
        assert g.vision == v and g.embed_dim == 1024 and g.quick_gelu == cfg.quick_gelu
        assert name + suffix in mc.list_models()
        mc.check_attention_support(g)


@pytest.mark.parametrize("label,name", [("ViT-H-14", "ViT-H-14"), ("ViT-H-14", "ViT-H-14-quickgelu"),
                                        ("ViT-H-16", "ViT-H-16")])
def test_vith_layout_matches_reference_manifest(golden_dir, label, name):
    ref = _manifest(golden_dir)[label]
    specs = _specs(mc.get_model_config(name))
    assert set(specs) == set(ref), set(specs) ^ set(ref)
    for k, shp in ref.items():
        assert specs[k] == shp, k
    assert specs["visual.transformer.resblocks.31.attn.in_proj_weight"] == [3840, 1280]
    assert specs["transformer.resblocks.23.attn.in_proj_weight"] == [3072, 1024]


# every name registered before the ViT-H entries, with the fields of its config restated:
# (embed, vision layers, width, patch, image, text width, text heads, quick_gelu)
_BEFORE = {
    "ViT-B-16": (512, 12, 768, 16, 224, 512, 8, False), "ViT-B-32": (512, 12, 768, 32, 224, 512, 8, False),
    "ViT-L-14": (768, 24, 1024, 14, 224, 768, 12, False), "ViT-L-14-336": (768, 24, 1024, 14, 336, 768, 12, False),
    "ViT-L-14-280": (768, 24, 1024, 14, 280, 768, 12, False), "ViT-S-16": (384, 12, 384, 16, 224, 384, 6, False),
    "ViT-S-32": (384, 12, 384, 32, 224, 384, 6, False), "ViT-Ti-16": (512, 12, 192, 16, 224, 256, 4, False),
    "ViT-B-16-quickgelu": (512, 12, 768, 16, 224, 512, 8, True), "ViT-B-32-quickgelu": (512, 12, 768, 32, 224, 512, 8, True),
    "ViT-L-14-quickgelu": (768, 24, 1024, 14, 224, 768, 12, True),
    "ViT-L-14-336-quickgelu": (768, 24, 1024, 14, 336, 768, 12, True),
}


@pytest.mark.parametrize("name", sorted(_BEFORE))
def test_previously_registered_names_unchanged(golden_dir, name):
    embed, layers, width, patch, image, t_width, t_heads, quick = _BEFORE[name]
    want = mc.ModelCfg(embed_dim=embed, vision=mc.VisionCfg(image, patch, width, layers, 64, 4.0),
                       text=mc.TextCfg(77, 49408, t_width, t_heads, 12, 4.0), gene=None, quick_gelu=quick)
    cfg = mc.get_model_config(name)
    assert cfg == want
    mc.check_attention_support(cfg)
    for suffix, kind in (("-gene", "mlp"), ("-genetr", "transformer")):
        g = mc.get_model_config(name + suffix)
        assert g == mc.ModelCfg(embed_dim=embed, vision=want.vision, text=None, gene=mc.GeneCfg(20000, 512, kind=kind),
                                quick_gelu=quick)
        mc.check_attention_support(g)
    # specs: against the reference manifests where they hold the name, and always the vision tower's head-independent
    # layout (the q/k/v projection is one [3 width, width] matrix whatever the head dim)
    specs = _specs(cfg)
    for which in ("state_dict_manifest.json", "state_dict_manifest_hires.json"):
        ref = _manifest(golden_dir, which).get(name[:-len("-quickgelu")] if quick else name)
        if ref is not None and "visual.conv1.weight" in ref and "token_embedding.weight" in ref:
            assert set(specs) == set(ref) and all(specs[k] == list(shp) for k, shp in ref.items()), which
    assert specs["visual.transformer.resblocks.0.attn.in_proj_weight"] == [3 * width, width]
    assert specs["visual.positional_embedding"] == [(image // patch) ** 2 + 1, width]
    assert len(specs) == len(_specs(want))


def test_registry_holds_exactly_the_old_names_and_vith():
    names = set(mc.list_models())
    base = set(_BEFORE) | {"ViT-H-14", "ViT-H-14-quickgelu", "ViT-H-16"}
    assert names == base | {n + "-gene" for n in base} | {n + "-genetr" for n in base}


@pytest.mark.parametrize("name", ["ViT-g-14", "ViT-bigG-14", "ViT-H-14-378", "ViT-H-14-378-quickgelu", "ViT-H-16-quickgelu",
                                  "ViT-g-14-gene", "ViT-bigG-14-genetr"])
def test_names_without_a_kernel_still_raise(name):
    with pytest.raises(RuntimeError, match="not found"):
        mc.get_model_config(name)


def test_attention_support_check_names_the_limits():
    # ViT-H-14 at 378 px: 730 tokens at head dim 80
    cfg = mc.get_model_config("ViT-H-14-gene", image_size=378)
    assert cfg.vision.tokens == 730
    with pytest.raises(ValueError, match=r"head dim 80 at 730 tokens.*32 / 64 / 80 up to 320 tokens"):
        mc.check_attention_support(cfg)
    # the largest ViT-H-14 input that fits: 17 x 17 patches + 1 = 290 tokens; 18 x 18 + 1 = 325 does not
    mc.check_attention_support(mc.get_model_config("ViT-H-14-gene", image_size=238))
    with pytest.raises(ValueError, match="320"):
        mc.check_attention_support(mc.get_model_config("ViT-H-14-gene", image_size=252))
    # head dims of ViT-g-14 (88) and ViT-bigG-14 (104), and others without a kernel
    for hw, width in ((88, 1408), (104, 1664), (48, 768), (96, 768), (128, 1024)):
        bad = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(224, 14, width, 2, hw), text=None, gene=mc.GeneCfg(64, 32))
        with pytest.raises(ValueError, match=rf"head dim {hw}\b.*32 / 64 / 80"):
            mc.check_attention_support(bad)
    # head dim 64 keeps every length (non-causal); head dim 32 stops at 320 tokens
    mc.check_attention_support(mc.get_model_config("ViT-L-14-336-gene"))
    mc.check_attention_support(mc.get_model_config("ViT-B-16-gene", image_size=512))
    with pytest.raises(ValueError, match="head dim 32 at 577 tokens"):
        mc.check_attention_support(mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(384, 16, 256, 2, 32), text=None,
                                               gene=mc.GeneCfg(64, 32)))
    # a width that is not a whole number of heads
    with pytest.raises(ValueError, match="multiple of the head dim"):
        mc.check_attention_support(mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(224, 16, 200, 2, 80), text=None,
                                               gene=mc.GeneCfg(64, 32)))
    # the text tower is causal: a long context has no kernel even at head dim 64
    long_text = mc.get_model_config("ViT-B-16")
    long_text.text.context_length = 400
    with pytest.raises(ValueError, match=r"text tower.*400 tokens \(causal\)"):
        mc.check_attention_support(long_text)
