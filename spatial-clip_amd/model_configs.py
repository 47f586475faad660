"""Model registry.  The reference resolves ``model_name`` through src/open_clip/model_configs/*.json
(src/open_clip/factory.py:392-502); the same names resolve here to the same architectures (values restated from
those JSON files).  ``<name>-gene`` swaps the reference's CLIP text tower for the gene-expression MLP named by
BASELINE.json (no reference counterpart: SURVEY.md section 8a row G); ``ViT-Ti-16-gene`` is the small config of
BASELINE.json configs[0]."""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Dict, Optional


@dataclass
class VisionCfg:
    image_size: int = 224
    patch_size: int = 16
    width: int = 768
    layers: int = 12
    head_width: int = 64
    mlp_ratio: float = 4.0
    # open_clip vision_cfg.pool_type / no_ln_pre / final_ln_after_pool (src/open_clip/transformer.py:594-603,652,773-823; every
    # CLIPA config sets avg / true / true): "tok" pools the class token, "avg" the mean of the patch tokens; no_ln_pre drops the
    # LayerNorm in front of the blocks (and its two parameters); final_ln_after_pool applies ln_post to the pooled row instead of
    # to every token before the pool.  Keyword-only: positional construction stops at patch_dropout, which stays the last field.
    pool_type: str = field(default="tok", kw_only=True)
    no_ln_pre: bool = field(default=False, kw_only=True)
    final_ln_after_pool: bool = field(default=False, kw_only=True)
    # FLIP patch dropout (open_clip vision_cfg.patch_dropout): fraction of the patch tokens a TRAINING forward drops, 0 = off
    patch_dropout: float = 0.0

    @property
    def heads(self) -> int:
        return self.width // self.head_width          # src/open_clip/model.py:170

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def tokens(self) -> int:
        return self.grid * self.grid + 1


@dataclass
class TextCfg:
    context_length: int = 77
    vocab_size: int = 49408
    width: int = 512
    heads: int = 8
    layers: int = 12
    mlp_ratio: float = 4.0
    # open_clip text_cfg.pool_type (text_global_pool, src/open_clip/transformer.py:921-940): the pooled row is the one at
    # text.argmax(-1) (the EOT token, CLIP's default), the last or the first token; no_causal_mask: full attention (CLIPA)
    pool_type: str = "argmax"
    no_causal_mask: bool = False


@dataclass
class GeneCfg:
    """Gene-expression tower (no reference symbol: SURVEY.md 8a row G).  ``kind="mlp"``: n_genes -> hidden -(GELU)->
    embed_dim (BASELINE configs[0]-[3]).  ``kind="transformer"`` (configs[4]): the expression vector is cut into
    ceil(n_genes / patch) contiguous patches of ``patch`` genes (zero padded), each embedded by one bias-free linear
    map -- a 1-D ViT patch embedding -- then class token + learned positions, ln_pre, ``layers`` pre-LN residual
    attention blocks (the reference's ResidualAttentionBlock), ln_post on the class token, projection to embed_dim."""
    n_genes: int = 20000
    hidden: int = 512
    kind: str = "mlp"
    patch: int = 256
    width: int = 512
    layers: int = 6
    head_width: int = 64
    mlp_ratio: float = 4.0

    @property
    def tokens(self) -> int:
        return (self.n_genes + self.patch - 1) // self.patch + 1

    @property
    def heads(self) -> int:
        return self.width // self.head_width


@dataclass
class ModelCfg:
    embed_dim: int = 512
    vision: VisionCfg = field(default_factory=VisionCfg)
    text: Optional[TextCfg] = None
    gene: Optional[GeneCfg] = None
    init_logit_scale: float = math.log(1 / 0.07)     # src/open_clip/model.py:273
    # `quick_gelu: true` of the *-quickgelu model configs: act_layer = QuickGELU in BOTH reference towers
    # (src/open_clip/model.py:142-145,228; the OpenAI-pretrained weights were trained with it).  The gene towers are this
    # build's own definition and keep the exact-erf GELU.
    quick_gelu: bool = False
    # SigLIP's learnable logit bias (src/open_clip/model.py:299-302; the training entry sets -10 with --siglip,
    # main.py:225-227).  None (the default): no bias parameter at all -- parameters, flat layout and state_dict keys as before.
    init_logit_bias: Optional[float] = None


def _clip(embed, v_layers, v_width, patch, t_width, t_heads, t_layers=12, image=224, head_width=64) -> ModelCfg:
    return ModelCfg(embed_dim=embed, vision=VisionCfg(image, patch, v_width, v_layers, head_width),
                    text=TextCfg(77, 49408, t_width, t_heads, t_layers))


_REGISTRY: Dict[str, ModelCfg] = {
    "ViT-B-16": _clip(512, 12, 768, 16, 512, 8),
    "ViT-B-32": _clip(512, 12, 768, 32, 512, 8),
    "ViT-L-14": _clip(768, 24, 1024, 14, 768, 12),
    # src/open_clip/model_configs/ViT-L-14-336.json, ViT-L-14-280.json: ViT-L/14 at 336 px (577 tokens; OpenAI's 336-px
    # weights) and 280 px (401 tokens); above 320 tokens attention takes the long-sequence kernels
    "ViT-L-14-336": _clip(768, 24, 1024, 14, 768, 12, image=336),
    "ViT-L-14-280": _clip(768, 24, 1024, 14, 768, 12, image=280),
    "ViT-S-16": _clip(384, 12, 384, 16, 384, 6),
    "ViT-S-32": _clip(384, 12, 384, 32, 384, 6),
    "ViT-Ti-16": _clip(512, 12, 192, 16, 256, 4),
    # src/open_clip/model_configs/ViT-H-14.json, ViT-H-16.json: width 1280 = 16 heads of 80 (sc_attention_stream.hip), 32
    # layers, 257 / 197 tokens; text tower 1024 wide, 16 heads of 64, 24 layers
    "ViT-H-14": _clip(1024, 32, 1280, 14, 1024, 16, t_layers=24, head_width=80),
    "ViT-H-16": _clip(1024, 32, 1280, 16, 1024, 16, t_layers=24, head_width=80),
}
# src/open_clip/model_configs/ViT-B-16-quickgelu.json, ViT-B-32-quickgelu.json, ViT-L-14-quickgelu.json,
# ViT-L-14-336-quickgelu.json, ViT-H-14-quickgelu.json: the same architectures with `"quick_gelu": true`
for _base in ("ViT-B-16", "ViT-B-32", "ViT-L-14", "ViT-L-14-336", "ViT-H-14"):
    _REGISTRY[_base + "-quickgelu"] = replace(_REGISTRY[_base], quick_gelu=True)


def get_model_config(model_name: str, n_genes: Optional[int] = None, gene_hidden: Optional[int] = None,
                     image_size: Optional[int] = None) -> ModelCfg:
    """``ViT-B-16`` -> reference architecture (vision + CLIP text tower); ``ViT-B-16-gene`` -> gene-MLP tower;
    ``ViT-L-14-genetr`` -> 6-layer gene transformer tower (BASELINE configs[4]).  ``image_size`` overrides the vision
    tower's input size (the reference's ``create_model(force_image_size=...)``, src/open_clip/factory.py:438-439); it must
    be a multiple of the patch size.  None keeps the config's own size."""
    name = model_name
    gene = False
    kind = "mlp"
    if name.endswith("-genetr"):
        name, gene, kind = name[:-7], True, "transformer"
    elif name.endswith("-gene"):
        name, gene = name[:-5], True
    if name not in _REGISTRY:
        # same failure mode as open_clip.factory.create_model (factory.py:399-402)
        raise RuntimeError(f"Model config for {model_name} not found. Available: {sorted(list_models())}")
    cfg = _REGISTRY[name]
    cfg = ModelCfg(cfg.embed_dim, replace(cfg.vision), replace(cfg.text) if cfg.text else None, None,
                   cfg.init_logit_scale, cfg.quick_gelu)
    if image_size is not None:
        cfg = with_image_size(cfg, image_size)
    if gene:
        cfg.text = None
        cfg.gene = GeneCfg(n_genes or 20000, gene_hidden or 512, kind=kind)
    return cfg


def with_image_size(cfg: ModelCfg, image_size: int) -> ModelCfg:
    """A copy of ``cfg`` whose vision tower takes ``image_size`` px (a positive multiple of the patch size, else
    ValueError): (image_size / patch)^2 + 1 tokens, the positions resized on checkpoint load."""
    size = int(image_size)
    if size != image_size or size <= 0 or size % cfg.vision.patch_size:
        raise ValueError(f"image_size {image_size} is not a positive multiple of the patch size {cfg.vision.patch_size}")
    return replace(cfg, vision=replace(cfg.vision, image_size=size))


# what the attention kernels take (csrc/sc_attention*.hip): head dims 32 / 64 / 80 up to 320 tokens, causal or not; above
# that only head dim 64, non-causal
ATTN_HEAD_DIMS = (32, 64, 80)
ATTN_MAX_TOKENS = 320


def check_attention_support(cfg: ModelCfg) -> None:
    """ValueError, naming the supported head dims and lengths, if a tower of ``cfg`` has a (head dim, token count) that no
    attention kernel takes -- raised when the net is constructed, not at its first forward."""
    towers = [("vision", cfg.vision.width, cfg.vision.head_width, cfg.vision.tokens, False)]
    if cfg.text is not None:
        towers.append(("text", cfg.text.width, cfg.text.width // max(cfg.text.heads, 1), cfg.text.context_length,
                       not cfg.text.no_causal_mask))
    if cfg.gene is not None and cfg.gene.kind == "transformer":
        towers.append(("gene", cfg.gene.width, cfg.gene.head_width, cfg.gene.tokens, False))
    for tower, width, dh, tokens, causal in towers:
        if dh <= 0 or width % dh:
            raise ValueError(f"{tower} tower: width {width} is not a multiple of the head dim {dh}")
        ok = (dh in ATTN_HEAD_DIMS and tokens <= ATTN_MAX_TOKENS) or (dh == 64 and not causal)
        if not ok:
            raise ValueError(
                f"{tower} tower: no attention kernel for head dim {dh} at {tokens} tokens"
                f"{' (causal)' if causal else ''}; supported: head dims {' / '.join(map(str, ATTN_HEAD_DIMS))} up to "
                f"{ATTN_MAX_TOKENS} tokens, and head dim 64 (non-causal) at any length")


# open_clip's CLIPVisionCfg / CLIPTextCfg keys (src/open_clip/model.py:28-103) that SpatialClipNet(vision_cfg= / text_cfg=) takes
VISION_OVERRIDE_KEYS = ("image_size", "patch_size", "width", "layers", "head_width", "mlp_ratio", "patch_dropout", "pool_type",
                        "no_ln_pre", "final_ln_after_pool")
TEXT_OVERRIDE_KEYS = ("context_length", "vocab_size", "width", "heads", "layers", "mlp_ratio", "pool_type", "no_causal_mask")
TEXT_IGNORED_KEYS = ("hf_tokenizer_name", "tokenizer_kwargs")
VISION_POOL_TYPES = ("tok", "avg")
TEXT_POOL_TYPES = ("argmax", "last", "first")
# keys of features this build does not have: accepted only with open_clip's default value
_VISION_UNSUPPORTED = {"ls_init_value": None, "attentional_pool": False, "attn_pooler_queries": 256, "attn_pooler_heads": 8,
                       "pos_embed_type": "learnable", "output_tokens": False, "timm_model_name": None,
                       "timm_model_pretrained": False, "timm_pool": "avg", "timm_proj": "linear", "timm_proj_bias": False,
                       "timm_drop": 0.0, "timm_drop_path": None}
_TEXT_UNSUPPORTED = {"ls_init_value": None, "hf_model_name": None, "embed_cls": False, "output_tokens": False,
                     "pos_embed_type": "learnable", "attentional_pool": False, "attn_pooler_queries": 256,
                     "attn_pooler_heads": 8}


def _check_override_keys(tower: str, over, known, ignored, unsupported) -> Dict[str, object]:
    if not hasattr(over, "items"):
        raise TypeError(f"{tower}_cfg must be a mapping of open_clip {tower}_cfg keys, got {type(over)}")
    out = {}
    for k, v in over.items():
        k = str(k)
        if k in known:
            out[k] = v
        elif k in ignored:
            continue
        elif k in unsupported or k.startswith(("timm_", "attn_pooler_")):
            default = unsupported.get(k)
            same = v == default and type(v) is type(default) if isinstance(default, bool) else v == default
            if not same:
                raise ValueError(f"{tower}_cfg key {k!r} = {v!r}: not supported by this build (only open_clip's default "
                                 f"{default!r} is accepted)")
        else:
            raise ValueError(f"{tower}_cfg key {k!r} is not known; accepted: {', '.join(known + ignored)}")
    return out


def _typed(tower: str, key: str, value, like):
    """The override ``value`` in the type of the field's default ``like`` (a YAML 4 for mlp_ratio becomes 4.0)."""
    try:
        if isinstance(like, bool):
            if not isinstance(value, (bool, int)) or value not in (0, 1, True, False):
                raise TypeError
            return bool(value)
        if isinstance(like, int):
            if int(value) != value:
                raise TypeError
            return int(value)
        if isinstance(like, float):
            return float(value)
        return str(value)
    except (TypeError, ValueError):
        raise ValueError(f"{tower}_cfg key {key!r}: {value!r} is not a valid {type(like).__name__}") from None


def with_vision_overrides(cfg: ModelCfg, over) -> ModelCfg:
    """A copy of ``cfg`` with the open_clip ``vision_cfg`` mapping ``over`` applied on top of its vision tower.  ValueError,
    naming the key, for a key of a feature this build lacks (unless it carries open_clip's default) or an unknown key."""
    vals = _check_override_keys("vision", over, VISION_OVERRIDE_KEYS, (), _VISION_UNSUPPORTED)
    base = VisionCfg()
    vals = {k: _typed("vision", k, v, getattr(base, k)) for k, v in vals.items()}
    if vals.get("pool_type", "tok") not in VISION_POOL_TYPES:
        raise ValueError(f"vision_cfg key 'pool_type' = {vals['pool_type']!r}: this build pools {' / '.join(VISION_POOL_TYPES)}")
    vision = replace(cfg.vision, **vals)
    if vision.image_size <= 0 or vision.patch_size <= 0 or vision.image_size % vision.patch_size:
        raise ValueError(f"vision_cfg: image_size {vision.image_size} is not a positive multiple of patch_size {vision.patch_size}")
    return replace(cfg, vision=vision)


def with_text_overrides(cfg: ModelCfg, over) -> ModelCfg:
    """The same for the reference's text tower (``text_cfg``); ValueError on a config without one (``-gene`` / ``-genetr``)."""
    if cfg.text is None:
        raise ValueError("text_cfg: this model has no text tower (a -gene / -genetr model fills the text slot with a gene tower)")
    vals = _check_override_keys("text", over, TEXT_OVERRIDE_KEYS, TEXT_IGNORED_KEYS, _TEXT_UNSUPPORTED)
    base = TextCfg()
    vals = {k: _typed("text", k, v, getattr(base, k)) for k, v in vals.items()}
    if vals.get("pool_type", "argmax") not in TEXT_POOL_TYPES:
        raise ValueError(f"text_cfg key 'pool_type' = {vals['pool_type']!r}: this build pools {' / '.join(TEXT_POOL_TYPES)}")
    return replace(cfg, text=replace(cfg.text, **vals))


def list_models():
    return list(_REGISTRY) + [n + "-gene" for n in _REGISTRY] + [n + "-genetr" for n in _REGISTRY]
