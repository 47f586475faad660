#!/usr/bin/env python3
"""ViT-H fixtures (head dim 80) from the REFERENCE's own modules.

Run in the build container only (imports the reference, never copies it; the outputs are names, shapes, inputs and
expected outputs only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vith.py

Output
  state_dict_manifest_vith.json  {name: {state_dict key: shape}} of open_clip.factory.create_model(name, pretrained=None)
                                 for ViT-H-14 and ViT-H-16 (one model at a time: ViT-H-14 is about 1 B parameters); the
                                 scheme of state_dict_manifest.json.
  blk_dh80.npz                   one ResidualAttentionBlock(160, 2, mlp_ratio=1.0) -- two heads of 80 -- at L = 257,
  blk_dh80_causal.npz            non-causal, and at L = 77 with the causal mask, written the way make_golden.py writes
                                 blk_d128.npz: fp32 x, y, gy, gx, "p.<name>" parameters and "g.<name>" their gradients.
                                 To stay under the 1 MiB limit of a committed file the six weight MATRICES and their
                                 gradients live beside them in
  blk_dh80_weights.npz           "p.<name>" of every 2-D parameter, and
  blk_dh80_wgrads.npz            "g.<name>" of the non-causal run,
  blk_dh80_causal_wgrads.npz     "g.<name>" of the causal run (same block, same weights).
                                 mlp_ratio = 1.0 (MLP width 160) keeps the matrices at 6 * 160^2 * 4 B = 600 KiB per file;
                                 attention, the part under test, does not depend on it.  Batch 1 at 257 tokens (643 KiB of
                                 activations), batch 3 at 77."""
import importlib
import json
import os
import sys

sys.dont_write_bytecode = True
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npz  # noqa: E402
from make_golden_hires import _stub  # noqa: E402

NAMES = ("ViT-H-14", "ViT-H-16")


def blocks():
    tf = sys.modules["open_clip.transformer"]
    torch.manual_seed(1)
    blk = tf.ResidualAttentionBlock(160, 2, mlp_ratio=1.0)
    for n, p_ in blk.named_parameters():   # make biases / LN affine non-trivial
        if p_.ndim == 1:
            p_.data.add_(0.1 * torch.randn_like(p_))
    npz("blk_dh80_weights.npz", **{"p." + n: p_ for n, p_ in blk.named_parameters() if p_.ndim == 2})
    for tag, B, L, causal in (("blk_dh80", 1, 257, False), ("blk_dh80_causal", 3, 77, True)):
        blk.zero_grad(set_to_none=True)
        x = torch.randn(B, L, 160, requires_grad=True)
        mask = torch.full((L, L), float("-inf")).triu_(1) if causal else None
        y = blk(x, attn_mask=mask)
        gy = torch.randn_like(y)
        y.backward(gy)
        arrs = {"x": x, "y": y, "gy": gy, "gx": x.grad, "heads": 2, "causal": int(causal)}
        big = {}
        for n, p_ in blk.named_parameters():
            if p_.ndim == 2:
                big["g." + n] = p_.grad
            else:
                arrs["p." + n] = p_
                arrs["g." + n] = p_.grad
        npz(f"{tag}.npz", **arrs)
        npz(f"{tag}_wgrads.npz", **big)


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
    out = {}
    for name in NAMES:
        torch.manual_seed(0)
        m = factory.create_model(name, pretrained=None)
        out[name] = {k: list(v.shape) for k, v in m.state_dict().items()}
        print(name, len(out[name]), "keys,", sum(p.numel() for p in m.parameters()) // 10**6, "M parameters", flush=True)
        del m
    json.dump(out, open(os.path.join(HERE, "state_dict_manifest_vith.json"), "w"), indent=0)
    print("wrote state_dict_manifest_vith.json")


def main():
    torch.set_num_threads(8)
    import_reference()
    blocks()
    manifest()


if __name__ == "__main__":
    main()
