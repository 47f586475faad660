"""fp32 oracle of the towers with the reference's other head shapes, composed of the oracle's public functions only
(O.patchify, O.linear, O.layer_norm, O.resblock): the vision tower with ``pool_type`` tok / avg, ``no_ln_pre`` and
``final_ln_after_pool`` (VisionTransformer.forward, src/open_clip/transformer.py:783-823), optionally on the kept patches
of a FLIP patch-dropout forward, and the text tower with ``pool_type`` argmax / last / first and ``no_causal_mask``
(text_global_pool, transformer.py:921-940).  tests/test_cpu_pool_config.py holds it against the reference's own fixtures."""
import torch
import torch.nn.functional as F

from oracle import spatial_clip_oracle as O


def vit_embed(images, p, v, no_ln_pre=False):
    """O.vit_embed with an optional ln_pre: patch GEMM, class token, positions."""
    w = p["visual.conv1.weight"].reshape(v.width, -1)
    x = O.linear(O.patchify(images, v.patch_size), w)
    cls = p["visual.class_embedding"].view(1, 1, -1).expand(x.shape[0], -1, -1)
    x = torch.cat([cls, x], dim=1) + p["visual.positional_embedding"]
    return x if no_ln_pre else O.layer_norm(x, p["visual.ln_pre.weight"], p["visual.ln_pre.bias"])


def encode_image(images, p, cfg, pool_type="tok", no_ln_pre=False, final_ln_after_pool=False, keep=None, normalize=True):
    """``keep``: integer [B, K] patch indices (0-based, class token excluded) of a dropping forward, or None.  The stem runs on
    all tokens and the kept ones are gathered behind it: LayerNorm is per token, so this equals the reference's drop in front
    of ln_pre."""
    v = cfg.vision
    x = vit_embed(images, p, v, no_ln_pre)
    if keep is not None:
        B = x.shape[0]
        idx = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.as_tensor(keep).long() + 1], dim=1)
        x = x[torch.arange(B)[:, None], idx]
    for i in range(v.layers):
        x = O.resblock(x, p, f"visual.transformer.resblocks.{i}.", v.heads, causal=False, quick=cfg.quick_gelu)
    ln = lambda t: O.layer_norm(t, p["visual.ln_post.weight"], p["visual.ln_post.bias"])
    pool = (lambda t: t[:, 1:].mean(dim=1)) if pool_type == "avg" else (lambda t: t[:, 0])
    pooled = ln(pool(x)) if final_ln_after_pool else pool(ln(x))
    f = pooled @ p["visual.proj"]
    return F.normalize(f, dim=-1) if normalize else f


def encode_text(text, p, cfg, pool_type="argmax", no_causal_mask=False, normalize=True):
    t = cfg.text
    x = p["token_embedding.weight"][text] + p["positional_embedding"]
    for i in range(t.layers):
        x = O.resblock(x, p, f"transformer.resblocks.{i}.", t.heads, causal=not no_causal_mask, quick=cfg.quick_gelu)
    x = O.layer_norm(x, p["ln_final.weight"], p["ln_final.bias"])
    if pool_type == "argmax":
        x = x[torch.arange(x.shape[0]), text.argmax(dim=-1)]
    else:
        x = x[:, -1] if pool_type == "last" else x[:, 0]
    f = x @ p["text_projection"]
    return F.normalize(f, dim=-1) if normalize else f


def net_forward(images, texts, p, cfg, keep=None, **vision_flags):
    """O.net_forward of a ``*-gene`` model (gene-MLP second tower) with the image tower built with ``vision_flags``."""
    return {"image_features": encode_image(images, p, cfg, keep=keep, **vision_flags),
            "text_features": O.encode_gene(texts, p, cfg, normalize=True),
            "logit_scale": p["logit_scale"].exp(), "logit_bias": None}
