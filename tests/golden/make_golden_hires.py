#!/usr/bin/env python3
"""State_dict manifest of the vision towers above 320 tokens, from the REFERENCE's own factory.

Run in the build container only (imports the reference, never copies it; the output holds names and shapes only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hires.py

Output
  state_dict_manifest_hires.json  {label: {state_dict key: shape}} of open_clip.factory.create_model(name,
                                  pretrained=None) for ViT-L-14-336 (577 tokens) and ViT-L-14-280 (401), and for
                                  ViT-B-16 with force_image_size=384 (577); the scheme of state_dict_manifest.json."""
import importlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

CASES = (("ViT-L-14-336", "ViT-L-14-336", None), ("ViT-L-14-280", "ViT-L-14-280", None),
         ("ViT-B-16@384", "ViT-B-16", 384))


class _Placeholder(type):
    def __getattr__(cls, attr):          # class attributes used as defaults at import time (InterpolationMode.BICUBIC)
        return attr


def _stub(name):
    """A module whose every attribute is a placeholder class: the factory imports image transforms and tokenizers that
    building a model never calls (torchvision, ftfy, ... are not needed to construct the towers)."""
    mod = types.ModuleType(name)
    mod.__path__ = []
    mod.__getattr__ = lambda attr: _Placeholder(attr, (), {})
    sys.modules[name] = mod
    return mod


def main():
    import_reference()
    for name in ("torchvision.transforms", "torchvision.transforms.functional"):
        _stub(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    for name in ("omegaconf", "ftfy", "regex", "huggingface_hub", "safetensors", "safetensors.torch", "timm"):
        try:
            importlib.import_module(name)
        except ImportError:
            _stub(name)
    factory = importlib.import_module("open_clip.factory")
    manifest = {}
    for label, name, size in CASES:
        torch.manual_seed(0)
        m = factory.create_model(name, pretrained=None, force_image_size=size)
        manifest[label] = {k: list(v.shape) for k, v in m.state_dict().items()}
        print(label, "visual.positional_embedding", manifest[label]["visual.positional_embedding"], flush=True)
        del m
    json.dump(manifest, open(os.path.join(HERE, "state_dict_manifest_hires.json"), "w"), indent=0)
    print("wrote state_dict_manifest_hires.json")


if __name__ == "__main__":
    main()
