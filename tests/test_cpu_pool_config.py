"""Configuration surface of the average-pooled towers (vision pool_type / no_ln_pre / final_ln_after_pool, text pool_type /
no_causal_mask, the vision_cfg / text_cfg override mappings): field defaults leave every registered config as it was, the
reference's CLIPA configs applied as overrides give the reference's state_dict layout, keys of features this build lacks
are refused by name -- and the oracle composition the GPU tests compare against (tests/_pool_oracle.py) reproduces the
reference's own fixtures on the CPU."""
import json
import os
from dataclasses import fields

import numpy as np
import pytest
import torch

import spatial_clip_amd  # noqa: F401
from oracle import spatial_clip_oracle as O
from spatial_clip_amd import hydra_lite
from spatial_clip_amd import model_configs as mc
from spatial_clip_amd import params
from tests import _pool_oracle as PO


def _manifest(golden_dir):
    return json.load(open(os.path.join(golden_dir, "state_dict_manifest_clipa.json")))


def _clipa(golden_dir, label, base):
    cfgs = _manifest(golden_dir)["cfg"][label]
    cfg = mc.with_vision_overrides(mc.get_model_config(base), cfgs["vision_cfg"])
    return mc.with_text_overrides(cfg, cfgs["text_cfg"]), cfgs


def test_new_fields_have_neutral_defaults_and_leave_positional_construction_alone():
    # the vision fields are keyword-only (patch_dropout stays the last positional argument AND the last field, which
    # tests/test_cpu_patch_dropout.py pins); the text fields are appended
    vis = {f.name: f for f in fields(mc.VisionCfg)}
    assert all(vis[k].kw_only for k in ("pool_type", "no_ln_pre", "final_ln_after_pool"))
    assert [f.name for f in fields(mc.VisionCfg) if not f.kw_only][-2:] == ["mlp_ratio", "patch_dropout"]
    with pytest.raises(TypeError):
        mc.VisionCfg(32, 8, 64, 2, 32, 2.0, 0.5, "avg")
    assert [f.name for f in fields(mc.TextCfg)][6:] == ["pool_type", "no_causal_mask"]
    v, t = mc.VisionCfg(), mc.TextCfg()
    assert (v.pool_type, v.no_ln_pre, v.final_ln_after_pool) == ("tok", False, False)
    assert (t.pool_type, t.no_causal_mask) == ("argmax", False)
    # positional construction as the existing tests do it still means what it meant
    assert mc.VisionCfg(32, 8, 64, 2, 32, 2.0, 0.5).patch_dropout == 0.5


def test_registered_configs_and_names_are_unchanged():
    names = mc.list_models()
    assert len(names) == len(set(names)) == 45 and not any("CLIPA" in n for n in names)
    for name in names:
        cfg = mc.get_model_config(name)
        v = cfg.vision
        assert (v.pool_type, v.no_ln_pre, v.final_ln_after_pool, v.patch_dropout) == ("tok", False, False, 0.0), name
        assert v == mc.VisionCfg(v.image_size, v.patch_size, v.width, v.layers, v.head_width, v.mlp_ratio), name
        if cfg.text is not None:
            t = cfg.text
            assert t == mc.TextCfg(t.context_length, t.vocab_size, t.width, t.heads, t.layers, t.mlp_ratio), name
        specs = [s.name for s in params.build_specs(cfg)]
        assert "visual.ln_pre.weight" in specs and "visual.ln_pre.bias" in specs, name
    # empty override mappings change nothing
    base = mc.get_model_config("ViT-B-16")
    assert mc.with_text_overrides(mc.with_vision_overrides(base, {}), {}) == base


@pytest.mark.parametrize("label,base", [("ViT-L-14-CLIPA", "ViT-L-14"), ("ViT-H-14-CLIPA", "ViT-H-14")])
def test_clipa_overrides_give_the_reference_layout(golden_dir, label, base):
    cfg, cfgs = _clipa(golden_dir, label, base)
    assert cfg.embed_dim == cfgs["embed_dim"]
    v, t = cfg.vision, cfg.text
    assert (v.pool_type, v.no_ln_pre, v.final_ln_after_pool) == ("avg", True, True)
    assert (t.pool_type, t.no_causal_mask, t.context_length, t.vocab_size) == ("last", True, 32, 32000)
    ref = _manifest(golden_dir)["state_dict"][label]
    specs = {s.name: list(s.shape) for s in params.build_specs(cfg)}
    assert set(specs) == set(ref), set(specs) ^ set(ref)
    for k, shp in ref.items():
        assert specs[k] == list(shp), k
    assert not any(k.startswith("visual.ln_pre.") for k in specs)
    # the flat layout follows from the specs: offsets ascending, 64-float aligned, nothing reserved for the absent LayerNorm
    offs = [s.offset for s in params.build_specs(cfg)]
    assert offs == sorted(offs) and all(o % params.ALIGN == 0 for o in offs)
    with_ln = params.build_specs(mc.with_text_overrides(mc.get_model_config(base), cfgs["text_cfg"]))
    assert len(with_ln) == len(specs) + 2
    # 32 tokens, non-causal text tower; 257 vision tokens
    mc.check_attention_support(cfg)
    assert v.tokens == 257


def test_attention_support_uses_the_real_causal_flag(golden_dir):
    cfg, cfgs = _clipa(golden_dir, "ViT-H-14-CLIPA", "ViT-H-14")
    # ViT-H-14 + CLIPA overrides at 336 px: head dim 80 at 577 tokens has no kernel
    hi = mc.with_vision_overrides(cfg, {"image_size": 336})
    assert hi.vision.tokens == 577
    with pytest.raises(ValueError, match=r"vision tower.*head dim 80 at 577 tokens"):
        mc.check_attention_support(hi)
    # a long NON-causal text tower at head dim 64 has a kernel, the causal one has not
    long_text = mc.with_text_overrides(mc.get_model_config("ViT-B-16"), {"context_length": 400, "no_causal_mask": True})
    mc.check_attention_support(long_text)
    with pytest.raises(ValueError, match=r"text tower.*400 tokens \(causal\)"):
        mc.check_attention_support(mc.with_text_overrides(long_text, {"no_causal_mask": False}))


_REFUSED_VISION = [("ls_init_value", 1e-5), ("attentional_pool", True), ("attn_pooler_queries", 64), ("attn_pooler_heads", 4),
                   ("pos_embed_type", "sin_cos_2d"), ("output_tokens", True), ("timm_model_name", "vit_base_patch16_224"),
                   ("timm_pool", "token"), ("timm_drop_path", 0.1), ("pool_type", "none"), ("qk_norm", True),
                   ("not_a_key", 1)]
_REFUSED_TEXT = [("ls_init_value", 1e-5), ("hf_model_name", "roberta-base"), ("embed_cls", True), ("output_tokens", True),
                 ("pos_embed_type", "sin_cos_2d"), ("attentional_pool", True), ("pool_type", "none"), ("pool_type", "eos"),
                 ("proj_bias", True), ("not_a_key", 1)]


@pytest.mark.parametrize("key,value", _REFUSED_VISION)
def test_refused_vision_keys_raise_naming_the_key(key, value):
    with pytest.raises(ValueError, match=key):
        mc.with_vision_overrides(mc.get_model_config("ViT-B-16-gene"), {"width": 768, key: value})


@pytest.mark.parametrize("key,value", _REFUSED_TEXT)
def test_refused_text_keys_raise_naming_the_key(key, value):
    with pytest.raises(ValueError, match=key):
        mc.with_text_overrides(mc.get_model_config("ViT-B-16"), {"width": 512, key: value})


def test_unsupported_keys_pass_with_open_clips_default_value():
    base = mc.get_model_config("ViT-B-16")
    v = mc.with_vision_overrides(base, {"ls_init_value": None, "attentional_pool": False, "attn_pooler_queries": 256,
                                        "attn_pooler_heads": 8, "pos_embed_type": "learnable", "output_tokens": False,
                                        "timm_model_name": None, "timm_pool": "avg", "timm_proj": "linear",
                                        "timm_model_pretrained": False, "timm_proj_bias": False, "timm_drop": 0.0,
                                        "timm_drop_path": None, "pool_type": "tok", "mlp_ratio": 4})
    assert v == base and isinstance(v.vision.mlp_ratio, float)
    t = mc.with_text_overrides(base, {"ls_init_value": None, "hf_model_name": None, "embed_cls": False, "output_tokens": False,
                                      "hf_tokenizer_name": "bert-base-uncased", "tokenizer_kwargs": {"strip_sep_token": True}})
    assert t == base
    # every accepted key lands in its field
    got = mc.with_vision_overrides(base, {"image_size": 64, "patch_size": 8, "width": 128, "layers": 3, "head_width": 32,
                                          "mlp_ratio": 2.0, "patch_dropout": 0.25, "pool_type": "avg", "no_ln_pre": True,
                                          "final_ln_after_pool": True}).vision
    assert got == mc.VisionCfg(64, 8, 128, 3, 32, 2.0, 0.25, pool_type="avg", no_ln_pre=True, final_ln_after_pool=True)
    assert got != mc.VisionCfg(64, 8, 128, 3, 32, 2.0, 0.25)
    got = mc.with_text_overrides(base, {"context_length": 16, "vocab_size": 97, "width": 64, "heads": 2, "layers": 1,
                                        "mlp_ratio": 2.0, "pool_type": "first", "no_causal_mask": True}).text
    assert got == mc.TextCfg(16, 97, 64, 2, 1, 2.0, "first", True)
    with pytest.raises(ValueError, match="image_size"):
        mc.with_vision_overrides(base, {"image_size": 100})          # not a multiple of the patch size


@pytest.mark.parametrize("name", ["ViT-B-16-gene", "ViT-L-14-genetr"])
def test_text_cfg_on_a_gene_model_raises(name):
    with pytest.raises(ValueError, match="text_cfg"):
        mc.with_text_overrides(mc.get_model_config(name), {"pool_type": "last"})
    # the gene transformer keeps ln_pre and the class token whatever the vision tower does
    cfg = mc.with_vision_overrides(mc.get_model_config(name), {"no_ln_pre": True, "pool_type": "avg"})
    specs = [s.name for s in params.build_specs(cfg)]
    assert "visual.ln_pre.weight" not in specs
    assert ("gene.ln_pre.weight" in specs) == name.endswith("-genetr")


def test_experiment_config_carries_the_overrides_as_plain_mappings():
    cfg = hydra_lite.compose("train", ["experiment=vitl14_clipa_gene_b128"])
    net = cfg.model.net
    assert net.model_name == "ViT-L-14-gene" and cfg.data.batch_size == 128
    assert dict(net.vision_cfg) == {"no_ln_pre": True, "pool_type": "avg", "final_ln_after_pool": True}
    got = mc.with_vision_overrides(mc.get_model_config(net.model_name), net.vision_cfg)
    assert (got.vision.pool_type, got.vision.no_ln_pre, got.vision.final_ln_after_pool) == ("avg", True, True)
    assert got.vision.width == 1024 and got.gene is not None


# ------------------------------------------------------------------------- the oracle composition against the reference
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _tiny_ocfg():
    return O.ModelCfg(embed_dim=32, vision=O.VisionCfg(32, 8, 64, 2, 32, 2.0), text=O.TextCfg(16, 97, 64, 2, 1, 4.0), gene=None)


def test_pool_oracle_matches_the_reference_fixtures(golden_dir):
    z, zg, za = (_load(golden_dir, n) for n in ("clipa_tiny.npz", "clipa_tiny_grads.npz", "clipa_tiny_avg.npz"))
    ocfg = _tiny_ocfg()
    p = {k[2:]: v.clone().requires_grad_(True) for k, v in z.items() if k.startswith("w.")}
    assert not any("ln_pre" in k for k in p)
    fi = PO.encode_image(z["images"], p, ocfg, pool_type="avg", no_ln_pre=True, final_ln_after_pool=True)
    ft = PO.encode_text(z["tokens"], p, ocfg, pool_type="last", no_causal_mask=True)
    assert float((fi.detach() - z["image_features"]).abs().max()) < 1e-5
    assert float((ft.detach() - z["text_features"]).abs().max()) < 1e-5
    ((fi * z["target_image"]).sum() + (ft * z["target_text"]).sum()).backward()
    for k, g in zg.items():
        got = p[k[2:]].grad if p[k[2:]].grad is not None else torch.zeros_like(p[k[2:]])
        assert float((got - g).abs().max()) <= 1e-4 * float(g.abs().max()) + 1e-7, k
    # the second tower: pool avg alone (ln_pre kept, ln_post on every token before the pool)
    p2 = {k[2:]: v.clone().requires_grad_(True) for k, v in za.items() if k.startswith("w.")}
    f2 = PO.encode_image(z["images"], p2, ocfg, pool_type="avg")
    assert float((f2.detach() - za["features"]).abs().max()) < 1e-5
    (f2 * z["target_image"]).sum().backward()
    for k, g in za.items():
        if k.startswith("g."):
            assert float((p2[k[2:]].grad - g).abs().max()) <= 1e-4 * float(g.abs().max()) + 1e-7, k
    # with no flag set the composition IS the oracle's own tower
    p3 = {k: v.detach() for k, v in p2.items()}
    assert torch.equal(PO.encode_image(z["images"], p3, ocfg), O.encode_image(z["images"], p3, ocfg))
