#!/usr/bin/env python3
"""Fixtures of the average-pooled (CLIPA) towers from the REFERENCE's own modules (imported, never copied; recipe and caveats:
make_golden.py).  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clipa.py

Output
  clipa_tiny.npz                   the reference's tiny CLIP (embed 32; vision 32 px / patch 8 / width 64 / 2 layers / head
                                   width 32 / mlp_ratio 2 with no_ln_pre, pool_type avg, final_ln_after_pool; text L 16 / vocab
                                   97 / width 64 / 2 heads / 1 layer with pool_type last, no_causal_mask), B = 6, fp32, CPU:
                                   images, token ids, "w.<name>" weights, normalised features of both towers, the targets of
                                   the scalar loss sum(image_features * target_image) + sum(text_features * target_text).
                                   To stay under the 1 MiB limit of a committed file the rest lives beside it in
  clipa_tiny_grads.npz             "g.<name>" = the gradient of every parameter of that model, and
  clipa_tiny_avg.npz               a SECOND vision tower with pool_type avg only (ln_pre kept, ln_post on every token
                                   before the pool): "w.<name>", "features", "g.<name>" for the same images and target_image.
  state_dict_manifest_clipa.json   {"state_dict": {name: {key: shape}}, "cfg": {name: {"embed_dim", "vision_cfg", "text_cfg"}}}
                                   of open_clip.factory.create_model(name, pretrained=None) / get_model_config(name) for
                                   ViT-L-14-CLIPA and ViT-H-14-CLIPA (the scheme of state_dict_manifest.json plus the config
                                   dicts the reference read)."""
import importlib
import json
import os
import sys

sys.dont_write_bytecode = True
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npz  # noqa: E402
from make_golden_hires import _stub  # noqa: E402

NAMES = ("ViT-L-14-CLIPA", "ViT-H-14-CLIPA")
VISION = {"image_size": 32, "layers": 2, "width": 64, "patch_size": 8, "head_width": 32, "mlp_ratio": 2.0}
TEXT = {"context_length": 16, "vocab_size": 97, "width": 64, "heads": 2, "layers": 1}
CFG_CLIPA = {"embed_dim": 32,
             "vision_cfg": dict(VISION, no_ln_pre=True, pool_type="avg", final_ln_after_pool=True),
             "text_cfg": dict(TEXT, pool_type="last", no_causal_mask=True)}
CFG_AVG = {"embed_dim": 32, "vision_cfg": dict(VISION, pool_type="avg"), "text_cfg": dict(TEXT)}
B = 6


def _tiny(model, cfg, seed):
    torch.manual_seed(seed)
    clip = model.CLIP(**cfg)
    for n, p_ in clip.named_parameters():      # make biases / LN affine non-trivial
        if p_.ndim == 1 and "logit" not in n:
            p_.data.add_(0.05 * torch.randn_like(p_))
    clip.train()
    return clip


def tiny(model):
    g = torch.Generator().manual_seed(32)
    images = torch.randn(B, 3, 32, 32, generator=g)
    tokens = torch.randint(1, TEXT["vocab_size"], (B, TEXT["context_length"]), generator=g)
    t_img = torch.randn(B, 32, generator=g)
    t_txt = torch.randn(B, 32, generator=g)
    clip = _tiny(model, CFG_CLIPA, 31)
    assert not any("ln_pre" in k for k in clip.state_dict()), "no_ln_pre left ln_pre keys"
    fi = F.normalize(clip.encode_image(images), dim=-1)
    ft = F.normalize(clip.encode_text(tokens), dim=-1)
    loss = (fi * t_img).sum() + (ft * t_txt).sum()
    loss.backward()
    arrs = {"images": images, "tokens": tokens, "target_image": t_img, "target_text": t_txt, "image_features": fi,
            "text_features": ft, "loss": loss}
    for k, v in clip.state_dict().items():
        arrs["w." + k] = v
    npz("clipa_tiny.npz", **arrs)
    npz("clipa_tiny_grads.npz", **{"g." + k: (p_.grad if p_.grad is not None else torch.zeros_like(p_))
                                   for k, p_ in clip.named_parameters()})
    clip2 = _tiny(model, CFG_AVG, 33)
    f2 = F.normalize(clip2.encode_image(images), dim=-1)
    (f2 * t_img).sum().backward()
    arrs = {"features": f2}
    for k, v in clip2.visual.state_dict().items():
        arrs["w.visual." + k] = v
    for k, p_ in clip2.visual.named_parameters():
        arrs["g.visual." + k] = p_.grad if p_.grad is not None else torch.zeros_like(p_)
    npz("clipa_tiny_avg.npz", **arrs)


def manifest():
    for name in ("torchvision.transforms", "torchvision.transforms.functional"):
        _stub(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    for name in ("omegaconf", "ftfy", "regex", "huggingface_hub", "safetensors", "safetensors.torch", "timm"):
        try:
            importlib.import_module(name)
        except ImportError:
            _stub(name)
    factory = importlib.import_module("open_clip.factory")
    out = {"state_dict": {}, "cfg": {}}
    for name in NAMES:
        cfg = factory.get_model_config(name)
        out["cfg"][name] = {k: cfg[k] for k in ("embed_dim", "vision_cfg", "text_cfg")}
        torch.manual_seed(0)
        m = factory.create_model(name, pretrained=None)
        out["state_dict"][name] = {k: list(v.shape) for k, v in m.state_dict().items()}
        print(name, len(out["state_dict"][name]), "keys,", sum(p.numel() for p in m.parameters()) // 10**6, "M parameters",
              flush=True)
        del m
    json.dump(out, open(os.path.join(HERE, "state_dict_manifest_clipa.json"), "w"), indent=0)
    print("wrote state_dict_manifest_clipa.json")


def main():
    torch.set_num_threads(8)
    model, _, _ = import_reference()
    tiny(model)
    if "--tiny-only" not in sys.argv:
        manifest()


if __name__ == "__main__":
    main()
