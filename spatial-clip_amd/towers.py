"""Encoder towers as explicit forward / backward kernel sequences over pre-allocated HBM buffers.

No autograd graph, no tracing compiler: every step is a C-ABI kernel launch on the current HIP stream, the
activations needed by backward live in buffers sized once per batch shape (288 GB of HBM3E make activation
recomputation unnecessary at these sizes), parameter gradients are written straight into the flat fp32 gradient
buffer of :class:`ParamStore`.

Reference semantics: VisionTransformer.forward (src/open_clip/transformer.py:783-823,907-918),
ResidualAttentionBlock.forward (:289-300), CLIP.encode_image (src/open_clip/model.py:326-328).
Residual stream fp32, GEMM operands bf16 with fp32 accumulation, LayerNorm / softmax / normalisation in fp32 --
the reference's ``precision: bf16-mixed`` autocast policy."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional

import torch

from . import ops
from .model_configs import ModelCfg
from .lock import TowerLock
from .params import ParamStore
from .stack import BF16, F32, TransformerStack, _Bufs, _res_stream_bf16, _splitk_for  # noqa: F401  (re-exported)


def _head_fwd(t, x: torch.Tensor, ldx: Optional[int] = None) -> torch.Tensor:
    """Head of a tower: pooled rows ``x`` [B, d] (row stride ``ldx``) -> final LayerNorm -> projection -> L2 normalise.
    ``pooled``, ``f_raw`` and the statistics stay in the tower's buffers for ``_head_bwd``; the features are ``t.f``."""
    s, bf, B, d, D = t.s, t.bufs, t.B, t.d, t.D
    ln_w, ln_b, proj = t.param_names_head()
    pooled = bf.get("pooled", (B, d), BF16)
    ops.layernorm_fwd(x, s.p(ln_w), s.p(ln_b), pooled, bf.get("m_post", (B,), F32), bf.get("r_post", (B,), F32), B, d, ldx=ldx)
    return _proj_fwd(t, pooled)


def _proj_fwd(t, pooled: torch.Tensor) -> torch.Tensor:
    """Tail of ``_head_fwd``: the normalised pooled rows ``pooled`` (bf16 [B, d], the tower's "pooled" buffer) -> projection ->
    L2 normalise."""
    s, bf, B, d, D = t.s, t.bufs, t.B, t.d, t.D
    proj = t.param_names_head()[2]
    f_raw = bf.get("f_raw", (B, D), F32)
    ops.gemm(ops.NT, ops.EPI_F32, pooled, s.copies[proj].wf, f_raw, M=B, N=D, K=d)
    t.f = torch.empty((B, D), dtype=F32, device=pooled.device)
    ops.l2norm_fwd(f_raw, t.f, None, bf.get("inv", (B,), F32), B, D)
    return t.f


def _head_bwd(t, d_f: torch.Tensor, dgrad: bool = True) -> Optional[torch.Tensor]:
    """Backward of ``_head_fwd`` down to the final LayerNorm's output: writes the projection's gradient, returns d(pooled).
    ``dgrad=False`` (a locked tower whose projection alone is trainable): the weight gradient only, returns None."""
    s, bf, B, d, D = t.s, t.bufs, t.B, t.d, t.D
    proj = t.param_names_head()[2]
    d_raw = bf.get("d_raw", (B, D), BF16)
    ops.l2norm_bwd(d_f.contiguous().float(), t.f, bf.get("inv", (B,), F32), d_raw, B, D)
    d_pooled = None
    if dgrad:
        d_pooled = bf.get("d_pooled", (B, d), BF16)
        ops.gemm(ops.NT, ops.EPI_BF16, d_raw, s.copies[proj].wb, d_pooled, M=B, N=d, K=D)
    ops.gemm(ops.TN, ops.EPI_F32, bf.get("pooled", (B, d), BF16), d_raw, s.g(proj), M=d, N=D, K=B)
    return d_pooled


def _set_lock(t, unlocked: Optional[int]) -> None:
    """Give tower ``t`` (with a ``stack`` of ``layers`` blocks) the lock ``unlocked`` (None: not locked)."""
    t.lock = TowerLock(t.stack.layers, unlocked)
    t.stack.floor = t.lock.floor


class PatchTransformerTower:
    """Patch embedding (one bias-free linear map per patch) + class token + learned positions + ln_pre + N residual
    attention blocks + ln_post on the class token (pool 'tok') + output projection + L2 normalise.  The image tower
    (VisionTransformer, src/open_clip/transformer.py:583-918) and the gene transformer (configs[4]; 1-D patches of the
    expression vector) are both instances: they differ in how the [B * patches, patch_dim] operand is formed
    (``_patchify``) and in the parameter-name prefix.

    The image tower also takes the reference's other head shapes (vision_cfg.pool_type / no_ln_pre / final_ln_after_pool,
    transformer.py:594-603,652,773-823); the gene transformer keeps ln_pre and 'tok':
      * ``no_ln_pre``: the stem adds class token and positions and applies no LayerNorm (no ln_pre parameters exist);
      * ``pool_type == "avg"``: the last block runs at full width and the pooled row is the mean of the PATCH tokens
        (ops.token_pool_fwd, t0 = 1; after patch dropout: of the kept ones) -- with ``final_ln_after_pool`` (CLIPA) ln_post is
        applied to that mean, without it to every token before the mean;
      * ``pool_type == "tok"`` with ``final_ln_after_pool`` is today's path: LayerNorm is per row."""

    prefix = "visual."
    quick_gelu = False          # set by the subclass before super().__init__: only the reference's towers take the config flag
    pool_type = "tok"           # likewise: vision_cfg.pool_type / no_ln_pre / final_ln_after_pool
    no_ln_pre = False
    final_ln_after_pool = False

    def __init__(self, cfg: ModelCfg, store: ParamStore, width: int, heads: int, layers: int, mlp_ratio: float,
                 tokens: int, patch_dim: int):
        self.cfg, self.s = cfg, store
        self.d, self.D, self.L = width, cfg.embed_dim, tokens
        self.n_layers = layers
        self.kp = patch_dim
        self.kp_pad = store.copies[self.prefix + "conv1.weight"].k_pad
        self.stack = TransformerStack(store, self.prefix + "transformer.resblocks.", width, heads, layers,
                                      int(width * mlp_ratio), causal=False, cls_only_last=self.pool_type == "tok", res16_ok=True,
                                      quick_gelu=self.quick_gelu)
        self.bufs = _Bufs(store.device)
        # state of the last forward, read by its backward: the token count of THAT pass (K + 1 when patches were dropped) and
        # its (keep [B, K], slot [B, n]) pair, (None, None) for a full-length pass (set by _patchify: VisionTower)
        self.L_run = tokens
        self._keep = (None, None)
        self._pad_zeroed: Dict[str, torch.Tensor] = {}      # patch buffer name -> the tensor whose K padding is zeroed
        self.lock = TowerLock(layers)       # LiT: nothing locked (SpatialClipNet.lock_image_tower -> set_lock)

    def set_lock(self, unlocked: Optional[int]) -> None:
        _set_lock(self, unlocked)

    def _n(self, leaf: str) -> str:
        return self.prefix + leaf

    def _name_pass_bufs(self) -> None:
        """The activations of a dropping pass live under buffer names of their own."""
        self.bufs.suffix = self.stack.bufs.suffix = "" if self._keep[0] is None else ".keep"

    def param_names_head(self) -> List[str]:
        return [self._n("ln_post.weight"), self._n("ln_post.bias"), self._n("proj")]

    def param_names_stem(self) -> List[str]:
        names = [self._n("conv1.weight"), self._n("class_embedding"), self._n("positional_embedding")]
        return names if self.no_ln_pre else names + [self._n("ln_pre.weight"), self._n("ln_pre.bias")]

    def _patchify(self, x: torch.Tensor) -> torch.Tensor:
        """-> bf16 [B * (L - 1), kp_pad] patch rows (sets self.B)."""
        raise NotImplementedError

    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        s, d = self.s, self.d
        s.wait_names(self.param_names_stem())
        self._keep = (None, None)
        self._name_pass_bufs()
        patches = self._patchify(inp)
        B, keep = self.B, self._keep[0]
        L = self.L_run = self.L if keep is None else keep.shape[1] + 1
        M, Mp = B * L, B * (L - 1)
        bf = self.bufs
        patch_out = bf.get("patch_out", (Mp, d), F32)
        ops.gemm(ops.NT, ops.EPI_F32, patches, s.copies[self._n("conv1.weight")].wf, patch_out, M=Mp, N=d, K=self.kp_pad)
        # the stream's first tensor in the stream's own precision: with the bf16 stream ln_pre writes bf16 (as the reference's does
        # under bf16-mixed) instead of an fp32 copy that a cast pass then halves (310 MB of traffic per step at ViT-B/16)
        r16 = self.stack.res16_ok and _res_stream_bf16(self.stack.res_stream) and os.environ.get("SC_STEM_BF16", "1") != "0"
        x0 = bf.get("x0.16", (M, d), BF16) if r16 else bf.get("x0", (M, d), F32)
        if self.no_ln_pre:          # the row kernels' "no LN" body: no gamma, no statistics
            ops.embed_ln_fwd(patch_out, s.p(self._n("class_embedding")), s.p(self._n("positional_embedding")), None, None, x0,
                             None, None, B, L, d, keep=keep)
        else:
            ops.embed_ln_fwd(patch_out, s.p(self._n("class_embedding")), s.p(self._n("positional_embedding")),
                             s.p(self._n("ln_pre.weight")), s.p(self._n("ln_pre.bias")), x0,
                             bf.get("m_pre", (M,), F32), bf.get("r_pre", (M,), F32), B, L, d, keep=keep)
        xf = self.stack.forward(x0, B, L)
        self.xf = xf
        s.wait_names(self.param_names_head())
        if self.pool_type == "avg":
            return self._head_fwd_avg(xf, B, L)
        self.x_ld = d if self.stack.cls_only_last else L * d          # xf is compact [B, d] in CLS-only mode
        return _head_fwd(self, xf, ldx=self.x_ld)

    def _head_fwd_avg(self, xf: torch.Tensor, B: int, L: int) -> torch.Tensor:
        """Head of an average-pooled tower over the full-width output ``xf`` [B * L, d] of the last block."""
        s, d, bf = self.s, self.d, self.bufs
        if self.final_ln_after_pool:
            # CLIPA order (transformer.py:816-818): mean of the patch tokens, then ln_post on the B mean rows
            mean = bf.get("pool_mean", (B, d), F32)
            ops.token_pool_fwd(xf, B, L, 1, d, mean_f32=mean)
            return _head_fwd(self, mean, ldx=d)
        # transformer.py:820-821: ln_post on every token, then the mean of the patch tokens' rows
        ln_w, ln_b, _ = self.param_names_head()
        M = B * L
        y = bf.get("ln_post_all", (M, d), BF16)
        ops.layernorm_fwd(xf, s.p(ln_w), s.p(ln_b), y, bf.get("m_post_all", (M,), F32), bf.get("r_post_all", (M,), F32), M, d)
        pooled = bf.get("pooled", (B, d), BF16)
        ops.token_pool_fwd(y, B, L, 1, d, mean_bf16=pooled)
        return _proj_fwd(self, pooled)

    def raw_features(self) -> torch.Tensor:
        """Projected features of the last forward before F.normalize (encode_image(normalize=False))."""
        return self.bufs.get("f_raw", (self.B, self.D), F32)

    def backward(self, d_f: torch.Tensor, on_bucket: Optional[Callable[[List[str]], None]] = None) -> None:
        s, d, B = self.s, self.d, self.B
        # the token count and the buffers of the forward this backward belongs to (K + 1 tokens after a dropping forward)
        L = self.L_run
        keep, slot = self._keep
        self._name_pass_bufs()
        M, Mp = B * L, B * (L - 1)
        bf = self.bufs
        if self.lock.head_only:         # locked up to the projection: the backward is that one weight gradient
            _head_bwd(self, d_f, dgrad=False)
            if on_bucket is not None:
                on_bucket(self.param_names_head()[2:])
            return
        d_pooled = _head_bwd(self, d_f)
        head_bwd = self._head_bwd_avg if self.pool_type == "avg" else self._head_bwd_tok
        dres, dres_bf = head_bwd(d_pooled, B, L)
        if on_bucket is not None:
            on_bucket(self.param_names_head())
        cb = (lambda i: on_bucket(self.stack.layer_param_names(i))) if on_bucket is not None else None
        dres = self.stack.backward(dres, dres_bf, last_bias_colsum_done=True, on_layer_done=cb)
        if not self.lock.stem:          # locked stem: nothing below the floor block has a gradient
            return
        # stem: ln_pre / positional / class embedding / patch embedding (no gradient flows to the input)
        dpatch = bf.get("dpatch", (Mp, d), BF16)
        if self.no_ln_pre:
            ops.embed_ln_bwd(dres, bf.get("patch_out", (Mp, d), F32), s.p(self._n("class_embedding")),
                             s.p(self._n("positional_embedding")), None, None, None, dpatch, None, None,
                             s.g(self._n("positional_embedding")), s.g(self._n("class_embedding")), B, L, d, keep=keep, slot=slot)
        else:
            ops.embed_ln_bwd(dres, bf.get("patch_out", (Mp, d), F32), s.p(self._n("class_embedding")),
                             s.p(self._n("positional_embedding")), bf.get("m_pre", (M,), F32), bf.get("r_pre", (M,), F32),
                             s.p(self._n("ln_pre.weight")), dpatch, s.g(self._n("ln_pre.weight")), s.g(self._n("ln_pre.bias")),
                             s.g(self._n("positional_embedding")), s.g(self._n("class_embedding")), B, L, d, keep=keep, slot=slot)
        gw = s.g(self._n("conv1.weight")).view(d, self.kp)
        ops.gemm(ops.TN, ops.EPI_F32, dpatch, bf.get("patches", (Mp, self.kp_pad), BF16), gw, M=d, N=self.kp, K=Mp,
                 splitk=_splitk_for(d, self.kp, Mp))
        if on_bucket is not None:
            on_bucket(self.param_names_stem())

    def _head_bwd_tok(self, d_pooled: torch.Tensor, B: int, L: int):
        """ln_post backward on the class-token rows (pool 'tok'): the residual gradient of the last block's output, the ln_post
        gradients and the last block's c_proj.bias gradient.  Returns (dres, dres_bf)."""
        s, d, bf = self.s, self.d, self.bufs
        M = B * L
        last = self.n_layers - 1
        if self.stack.cls_only_last:
            # class-token-only last block: its fp32 residual gradient lives in the class-token rows of the FULL buffer
            # (row stride L * d) from the start, so nothing has to be zeroed or copied when the full-width blocks take over
            dres = self.stack.bufs.get("dres_full", (M, d), F32)
            dres_bf = bf.get("dres_c_bf", (B, d), BF16)
            ld = d
        else:
            dres = bf.get("dres", (M, d), F32)
            dres_bf = bf.get("dres_bf", (M, d), BF16)
            dres.zero_()
            dres_bf.zero_()
            ld = L * d
        ops.layernorm_bwd(d_pooled, self.xf, bf.get("m_post", (B,), F32), bf.get("r_post", (B,), F32),
                          s.p(self._n("ln_post.weight")), dres, dres_bf, s.g(self._n("ln_post.weight")),
                          s.g(self._n("ln_post.bias")), s.g(self._n(f"transformer.resblocks.{last}.mlp.c_proj.bias")),
                          B, d, accumulate=False, ldx=self.x_ld, lddres=L * d, lddbf=ld)
        return dres, dres_bf

    def _head_bwd_avg(self, d_pooled: torch.Tensor, B: int, L: int):
        """Mirror of ``_head_fwd_avg`` from d(pooled) [B, d] (bf16) down to the stack: writes EVERY element of the residual
        gradient of the last block's output (fp32 ``dres`` and bf16 ``dres_bf``, no memset), the ln_post gradients and the last
        block's c_proj.bias gradient.  Returns (dres, dres_bf)."""
        s, d, bf = self.s, self.d, self.bufs
        M = B * L
        dres = bf.get("dres", (M, d), F32)
        dres_bf = bf.get("dres_bf", (M, d), BF16)
        ln_w, ln_b, _ = self.param_names_head()
        bias_g = s.g(self._n(f"transformer.resblocks.{self.n_layers - 1}.mlp.c_proj.bias"))
        if self.final_ln_after_pool:
            # LayerNorm backward on the B mean rows; its column sum IS the c_proj.bias gradient: each of the n pooled rows of a
            # sample receives d_mean / n
            d_mean = bf.get("d_pool_mean", (B, d), F32)
            ops.layernorm_bwd(d_pooled, bf.get("pool_mean", (B, d), F32), bf.get("m_post", (B,), F32),
                              bf.get("r_post", (B,), F32), s.p(ln_w), d_mean, None, s.g(ln_w), s.g(ln_b), bias_g, B, d,
                              accumulate=False)
            ops.token_pool_bwd(d_mean, B, L, 1, d, dx_f32=dres, dx_bf16=dres_bf)
        else:
            dy = bf.get("d_ln_post_all", (M, d), BF16)
            ops.token_pool_bwd(d_pooled, B, L, 1, d, dx_bf16=dy)
            ops.layernorm_bwd(dy, self.xf, bf.get("m_post_all", (M,), F32), bf.get("r_post_all", (M,), F32), s.p(ln_w), dres,
                              dres_bf, s.g(ln_w), s.g(ln_b), bias_g, M, d, accumulate=False)
        return dres, dres_bf


class VisionTower(PatchTransformerTower):
    """VisionTransformer (pool 'tok' or 'avg', learnable pos-embed, ln_pre unless no_ln_pre, ln_post before or after the pool,
    output projection) + L2 normalise."""

    prefix = "visual."

    def __init__(self, cfg: ModelCfg, store: ParamStore):
        v = cfg.vision
        self.v = v
        self.quick_gelu = bool(getattr(cfg, "quick_gelu", False))
        self.pool_type = str(getattr(v, "pool_type", "tok"))
        if self.pool_type not in ("tok", "avg"):
            raise ValueError(f"vision pool_type {self.pool_type!r}: 'tok' or 'avg'")
        self.no_ln_pre = bool(getattr(v, "no_ln_pre", False))
        self.final_ln_after_pool = bool(getattr(v, "final_ln_after_pool", False))
        super().__init__(cfg, store, v.width, v.heads, v.layers, v.mlp_ratio, v.tokens, 3 * v.patch_size * v.patch_size)
        # FLIP patch dropout (vision_cfg.patch_dropout; PatchDropout, src/open_clip/transformer.py:48-89): a forward that will be
        # differentiated, on a net in training mode, keeps K of the n patch tokens.  SpatialClipNet.forward arms ``drop`` for that
        # one forward -- {"seed", "draw", "rank", "keep" (explicit indices or None)} -- every other forward finds it None and
        # runs all tokens (validation, the zero-shot bank, encode_image, anything after net.eval()).
        self.patch_dropout = float(getattr(v, "patch_dropout", 0.0) or 0.0)
        self.drop: Optional[Dict[str, object]] = None
        self.keep_idx: Optional[torch.Tensor] = None      # int32 [B, K] of the last dropping forward (ascending patch indices)

    def _select(self, B: int, drop: Dict[str, object]):
        """(keep [B, K], slot [B, n]) of a dropping forward: drawn on the device (sc_patch_keep), or the explicit indices of
        SpatialClipNet.set_patch_keep."""
        from . import patch_dropout as pd
        n = self.L - 1
        K = pd.num_keep(n, self.patch_dropout)
        bf = self.bufs
        keep, slot = bf.get("keep.idx", (B, K), torch.int32), bf.get("keep.slot", (B, n), torch.int32)
        given = drop.get("keep")
        if given is not None:
            idx = pd.validate_keep(given, B, n, K)
            keep.copy_(torch.from_numpy(idx))
            slot.copy_(torch.from_numpy(pd.slots_from_keep(idx, n)))
        else:
            ops.patch_keep(drop["seed"], drop["draw"], drop["rank"] * B, B, n, K, keep=keep, slot=slot)
        self.keep_idx = keep
        return keep, slot

    def _patchify(self, images: torch.Tensor) -> torch.Tensor:
        v = self.v
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != v.image_size or images.shape[3] != v.image_size:
            raise ValueError(f"images must be [B,3,{v.image_size},{v.image_size}], got {tuple(images.shape)}")
        images = images.contiguous().float()
        self.B = B = images.shape[0]
        drop, self.drop = self.drop, None               # armed for ONE forward
        if drop is not None and self.patch_dropout > 0.0:
            self._keep = self._select(B, drop)
            self._name_pass_bufs()
        keep = self._keep[0]
        name = "patches" + self.bufs.suffix
        patches = self.bufs.get("patches", (B * (self.L - 1 if keep is None else keep.shape[1]), self.kp_pad), BF16)
        if self.kp_pad != self.kp and self._pad_zeroed.get(name) is not patches:
            patches.zero_()            # the K padding must be finite zeros; im2col only writes the real columns
            self._pad_zeroed[name] = patches
        ops.im2col(images, patches, v.patch_size, keep=keep)
        return patches


class GeneTransformerTower(PatchTransformerTower):
    """BASELINE configs[4]'s gene transformer (no reference symbol; model_configs.GeneCfg kind="transformer"): fills the
    ``texts`` slot of the batch with a float [B, n_genes] matrix like the gene-MLP tower."""

    prefix = "gene."

    def __init__(self, cfg: ModelCfg, store: ParamStore):
        g = cfg.gene
        self.g = g
        if g.patch % 64:
            raise ValueError(f"gene patch size {g.patch} must be a multiple of 64")
        super().__init__(cfg, store, g.width, g.heads, g.layers, g.mlp_ratio, g.tokens, g.patch)

    def param_names(self) -> List[str]:
        return [n for n in self.s.by_name if n.startswith("gene.")]

    def _patchify(self, x: torch.Tensor) -> torch.Tensor:
        g = self.g
        if x.dim() != 2 or x.shape[1] != g.n_genes:
            raise ValueError(f"gene matrix must be [B,{g.n_genes}], got {tuple(x.shape)}")
        x = x.contiguous().float()
        self.B = B = x.shape[0]
        T = self.L - 1
        patches = self.bufs.get("patches", (B * T, g.patch), BF16)
        # one cast pass: row b of the padded [B, T * patch] matrix IS rows b*T .. b*T+T-1 of the patch operand
        ops.cast_pad_bf16(x, patches.view(B, T * g.patch), B, g.n_genes, T * g.patch)
        return patches


class GeneTower:
    """Row G of SURVEY.md section 8a (no reference symbol): gene-expression MLP  n_genes -> hidden -(GELU)-> embed_dim,
    L2-normalised; fills the ``texts`` slot of the batch with a float [B, n_genes] matrix."""

    def __init__(self, cfg: ModelCfg, store: ParamStore):
        g = cfg.gene
        self.cfg, self.g, self.s = cfg, g, store
        self.D = cfg.embed_dim
        self.kpad = store.copies["gene.fc1.weight"].k_pad
        self.bufs = _Bufs(store.device)

    def param_names(self) -> List[str]:
        return ["gene.fc1.weight", "gene.fc1.bias", "gene.fc2.weight", "gene.fc2.bias"]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s, g, D = self.s, self.g, self.D
        if x.dim() != 2 or x.shape[1] != g.n_genes:
            raise ValueError(f"gene matrix must be [B,{g.n_genes}], got {tuple(x.shape)}")
        x = x.contiguous().float()
        B = x.shape[0]
        self.B = B
        bf = self.bufs
        s.wait_names(self.param_names())
        xg = bf.get("xg", (B, self.kpad), BF16)
        ops.cast_pad_bf16(x, xg, B, g.n_genes, self.kpad)
        u1 = bf.get("u1", (B, g.hidden), BF16)
        h1 = bf.get("h1", (B, g.hidden), BF16)
        # M = batch is small and K = n_genes is huge: split K over the chip (fp32 slabs), then bias + GELU
        ktiles = self.kpad // 64
        tiles = ((B + 127) // 128) * ((g.hidden + 127) // 128)
        splitk = max(1, min(ktiles // 2, 256 // max(tiles, 1), 64))
        if splitk > 1:
            pre = bf.get("pre1", (B, g.hidden), F32)
            ops.gemm(ops.NT, ops.EPI_F32, xg, s.copies["gene.fc1.weight"].wf, pre, M=B, N=g.hidden, K=self.kpad,
                     splitk=splitk)
            ops.bias_gelu_pair(pre, s.p("gene.fc1.bias"), u1, h1, B, g.hidden)
        else:
            ops.gemm(ops.NT, ops.EPI_GELU_PAIR, xg, s.copies["gene.fc1.weight"].wf, u1, M=B, N=g.hidden, K=self.kpad,
                     bias=s.p("gene.fc1.bias"), out2=h1)
        f_raw = bf.get("f_raw", (B, D), F32)
        ops.gemm(ops.NT, ops.EPI_F32_BIAS_RES, h1, s.copies["gene.fc2.weight"].wf, f_raw, M=B, N=D, K=g.hidden,
                 bias=s.p("gene.fc2.bias"))
        f = torch.empty((B, D), dtype=F32, device=x.device)
        ops.l2norm_fwd(f_raw, f, None, bf.get("inv", (B,), F32), B, D)
        self.f = f
        return f

    def raw_features(self) -> torch.Tensor:
        return self.bufs.get("f_raw", (self.B, self.D), F32)

    def backward(self, d_f: torch.Tensor, on_bucket: Optional[Callable[[List[str]], None]] = None) -> None:
        s, g, D, B = self.s, self.g, self.D, self.B
        bf = self.bufs
        d_raw = bf.get("d_raw", (B, D), BF16)
        ops.l2norm_bwd(d_f.contiguous().float(), self.f, bf.get("inv", (B,), F32), d_raw, B, D)
        h1, u1 = bf.get("h1", (B, g.hidden), BF16), bf.get("u1", (B, g.hidden), BF16)
        ops.gemm(ops.TN, ops.EPI_F32, d_raw, h1, s.g("gene.fc2.weight"), M=D, N=g.hidden, K=B)
        ops.colsum_bf16(d_raw, B, D, s.g("gene.fc2.bias"))
        dU = bf.get("dU", (B, g.hidden), BF16)
        ops.gemm(ops.NT, ops.EPI_BF16_DGELU, d_raw, s.copies["gene.fc2.weight"].wb, dU, M=B, N=g.hidden, K=D, aux=u1)
        ops.gemm(ops.TN, ops.EPI_F32, dU, bf.get("xg", (B, self.kpad), BF16), s.g("gene.fc1.weight"),
                 M=g.hidden, N=g.n_genes, K=B)
        ops.colsum_bf16(dU, B, g.hidden, s.g("gene.fc1.bias"))
        if on_bucket is not None:
            on_bucket(self.param_names())


class TextTower:
    """The reference's second tower: CLIP text transformer on BPE token ids (CLIP.encode_text,
    src/open_clip/model.py:330-345): embedding gather + positional embedding, causal pre-LN blocks, ln_final, EOT
    (argmax id) pooling, text_projection, L2 normalise.  ln_final is per token, so only the pooled rows are
    normalised (the reference normalises all 77 and then picks one)."""

    def __init__(self, cfg: ModelCfg, store: ParamStore):
        t = cfg.text
        self.cfg, self.t, self.s = cfg, t, store
        self.d, self.D, self.L, self.V = t.width, cfg.embed_dim, t.context_length, t.vocab_size
        self.stack = TransformerStack(store, "transformer.resblocks.", t.width, t.heads, t.layers,
                                      int(t.width * t.mlp_ratio), causal=not getattr(t, "no_causal_mask", False),
                                      quick_gelu=bool(getattr(cfg, "quick_gelu", False)))
        self.bufs = _Bufs(store.device)
        # text_cfg.pool_type (text_global_pool, src/open_clip/transformer.py:921-940): the pooled row is the one at text.argmax(-1)
        # (EOT), the last or the first token; for the two fixed ones the index buffer is filled once per buffer, not per step
        self.pool_type = str(getattr(t, "pool_type", "argmax"))
        if self.pool_type not in ("argmax", "last", "first"):
            raise ValueError(f"text pool_type {self.pool_type!r}: 'argmax', 'last' or 'first'")
        self._eot_filled: Optional[torch.Tensor] = None
        self.lock = TowerLock(t.layers)     # LiT: nothing locked (SpatialClipNet.lock_text_tower -> set_lock)

    def set_lock(self, unlocked: Optional[int]) -> None:
        _set_lock(self, unlocked)

    def param_names_head(self) -> List[str]:
        return ["ln_final.weight", "ln_final.bias", "text_projection"]

    def param_names_stem(self) -> List[str]:
        return ["token_embedding.weight", "positional_embedding"]

    def forward(self, text: torch.Tensor) -> torch.Tensor:
        s, d, L = self.s, self.d, self.L
        if text.dim() != 2 or text.shape[1] != L or text.dtype != torch.int64:
            raise ValueError(f"texts must be int64 [B,{L}] token ids, got {tuple(text.shape)} {text.dtype}")
        text = text.contiguous()
        B = text.shape[0]
        M = B * L
        self.B, self.text = B, text
        bf = self.bufs
        x0 = bf.get("x0", (M, d), F32)
        s.wait_names(self.param_names_stem())
        ops.token_embed_fwd(text, s.p("token_embedding.weight"), s.p("positional_embedding"), x0, B, L, d, self.V)
        xf = self.stack.forward(x0, B, L)
        s.wait_names(self.param_names_head())
        eot = bf.get("eot", (B,), torch.int32)
        if self.pool_type == "argmax":
            ops.argmax_rows(text, eot, B, L)
        elif self._eot_filled is not eot:
            eot.fill_(L - 1 if self.pool_type == "last" else 0)
            self._eot_filled = eot
        xe = bf.get("x_eot", (B, d), F32)
        ops.gather_rows(xf, eot, L, xe, B, d)
        return _head_fwd(self, xe)

    def raw_features(self) -> torch.Tensor:
        return self.bufs.get("f_raw", (self.B, self.D), F32)

    def backward(self, d_f: torch.Tensor, on_bucket: Optional[Callable[[List[str]], None]] = None) -> None:
        s, d, L, B = self.s, self.d, self.L, self.B
        M = B * L
        bf = self.bufs
        if self.lock.head_only:         # locked up to text_projection: the backward is that one weight gradient
            _head_bwd(self, d_f, dgrad=False)
            if on_bucket is not None:
                on_bucket(self.param_names_head()[2:])
            return
        d_pooled = _head_bwd(self, d_f)
        dxe = bf.get("dx_eot", (B, d), F32)
        last = self.t.layers - 1
        ops.layernorm_bwd(d_pooled, bf.get("x_eot", (B, d), F32), bf.get("m_post", (B,), F32),
                          bf.get("r_post", (B,), F32), s.p("ln_final.weight"), dxe, None, s.g("ln_final.weight"),
                          s.g("ln_final.bias"), s.g(f"transformer.resblocks.{last}.mlp.c_proj.bias"), B, d,
                          accumulate=False)
        dres = bf.get("dres", (M, d), F32)
        dres_bf = bf.get("dres_bf", (M, d), BF16)
        dres.zero_()
        dres_bf.zero_()
        ops.scatter_rows(dxe, bf.get("eot", (B,), torch.int32), L, dres, dres_bf, B, d)
        if on_bucket is not None:
            on_bucket(self.param_names_head())
        cb = (lambda i: on_bucket(self.stack.layer_param_names(i))) if on_bucket is not None else None
        self.stack.backward(dres, dres_bf, last_bias_colsum_done=True, on_layer_done=cb)
        if not self.lock.stem:          # locked embeddings: nothing below the floor block has a gradient
            return
        # scatter-add of the embedding gather: bit-reproducible by default (SC_EMBED_BWD_ATOMIC=1: the float-atomic kernel, A/B)
        ops.token_embed_bwd(self.text, dres, s.g("token_embedding.weight"), s.g("positional_embedding"), B, L, d, self.V,
                            eot=bf.get("eot", (B,), torch.int32) if self.stack.causal else None, deterministic=os.environ.get("SC_EMBED_BWD_ATOMIC", "0") != "1")
        if on_bucket is not None:
            on_bucket(self.param_names_stem())
