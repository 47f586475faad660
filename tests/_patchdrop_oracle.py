"""fp32 oracle of the vision tower with FLIP patch dropout, composed of the oracle's public functions only: the stem on ALL
tokens (O.vit_embed: LayerNorm is per token, so dropping after ln_pre equals the reference's drop before it), a gather of
the class token and the kept patches in ascending order, the residual blocks, ln_post on the class token, the projection."""
import torch
import torch.nn.functional as F

from oracle import spatial_clip_oracle as O


def encode_image_keep(images, p, cfg, keep, normalize=True):
    """``keep``: integer [B, K] patch indices (0-based, class token excluded)."""
    v = cfg.vision
    x = O.vit_embed(images, p, v)
    B = x.shape[0]
    idx = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.as_tensor(keep).long() + 1], dim=1)
    x = x[torch.arange(B)[:, None], idx]
    for i in range(v.layers):
        x = O.resblock(x, p, f"visual.transformer.resblocks.{i}.", v.heads, quick=cfg.quick_gelu)
    pooled = O.layer_norm(x[:, 0], p["visual.ln_post.weight"], p["visual.ln_post.bias"])
    f = pooled @ p["visual.proj"]
    return F.normalize(f, dim=-1) if normalize else f


def net_forward_keep(images, texts, p, cfg, keep):
    """O.net_forward of a ``*-gene`` model with the image tower dropping patches."""
    return {"image_features": encode_image_keep(images, p, cfg, keep),
            "text_features": O.encode_gene(texts, p, cfg, normalize=True),
            "logit_scale": p["logit_scale"].exp(), "logit_bias": None}
