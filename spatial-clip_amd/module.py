"""SpatialClipLitModule: the reference's task module (``src/models/spatial_clip_module.py:17-158``) without Lightning.

Same constructor kwargs, same hook names and return contracts: ``forward``, ``model_step`` (signature-filtered
loss kwargs, ``:44,55-61``), ``training_step(batch, batch_idx) -> loss``, ``validation_step``, ``test_step``,
``configure_optimizers() -> {"optimizer", "lr_scheduler": {...}}``.  ``self.log`` / ``self.log_dict`` collect into
``self.logged`` (device scalars, no host sync) for the trainer's logger."""
from __future__ import annotations

import functools
import inspect
import operator
import os
from collections.abc import Mapping
from typing import Any, Callable, Dict, Optional

import torch

from . import comm, ops
from .metrics import ContrastiveMetrics, RetrievalMetrics, ZeroShotGeneExpressionMetric, check_retrieval_ks
from .net import SpatialClipNet


class _HParams(dict):
    __getattr__ = dict.get


class StepOutput(dict):
    """``model_step`` result with the reference's keys (``loss``, ``logits``, ``image_features``;
    spatial_clip_module.py:66-70).  ``logits`` -- the local [B,B] ``image_features @ text_features.T * logit_scale``
    the reference computes for its metrics -- is materialised on first access: R@k already rides on the loss
    kernels' similarity matrix here, so the training step itself never needs it."""

    _LAZY = "logits"

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        dict.__setitem__(self, self._LAZY, None)

    def _materialise(self):
        v = dict.__getitem__(self, self._LAZY)
        if v is None:
            v = SpatialClipLitModule.local_logits(self)
            dict.__setitem__(self, self._LAZY, v)
        return v

    def __getitem__(self, k):
        return self._materialise() if k == self._LAZY else dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


TEACHER_KWARGS = ("dist_image_features", "dist_text_features", "dist_logit_scale")


def loss_wants_teacher(loss_fn) -> bool:
    """Does the loss's ``forward`` name ``dist_image_features`` (open_clip's DistillClipLoss does)?"""
    return TEACHER_KWARGS[0] in inspect.signature(loss_fn.forward).parameters


def check_teacher_binding(loss_fn, has_teacher: bool) -> None:
    """A loss that takes teacher features needs ``dist_net``; a ``dist_net`` needs a loss that takes them.  ValueError."""
    wants = loss_wants_teacher(loss_fn)
    if wants and not has_teacher:
        raise ValueError(f"{type(loss_fn).__name__}.forward takes dist_image_features: the module needs a teacher "
                         "(dist_net=..., config key model.dist_net)")
    if has_teacher and not wants:
        raise ValueError(f"dist_net was given, but {type(loss_fn).__name__}.forward takes no dist_image_features: "
                         "use loss=distill (DistillClipLoss) or drop model.dist_net")


def check_teacher_config(student, teacher) -> None:
    """The teacher sees the student's batch as it is (open_clip's training loop assumes identical transforms and tokenizer,
    open_clip_train/main.py; here it is checked): same image size, same gene count / same text context length and
    vocabulary.  ``student`` / ``teacher``: model_configs.ModelCfg.  ValueError naming the field that differs."""
    def diff(what, a, b):
        if a != b:
            raise ValueError(f"distillation teacher: {what} differs from the student's ({b} vs {a}); the teacher is fed the "
                             "student's batch, so both must read the same inputs")
    diff("vision tower presence", student.vision is None, teacher.vision is None)
    if student.vision is not None:
        diff("image_size", student.vision.image_size, teacher.vision.image_size)
    diff("second tower kind (gene / text)", student.gene is None, teacher.gene is None)
    if student.gene is not None:
        diff("n_genes", student.gene.n_genes, teacher.gene.n_genes)
    else:
        diff("text context_length", student.text.context_length, teacher.text.context_length)
        diff("text vocab_size", student.text.vocab_size, teacher.text.vocab_size)


def check_full_retrieval_cfg(cfg) -> Optional[tuple]:
    """``full_retrieval`` of the module -> the ks of its RetrievalMetrics, or None when the feature is off."""
    if cfg is None or cfg is False:
        return None
    if cfg is True:
        return RetrievalMetrics("").ks
    if isinstance(cfg, Mapping):
        unknown = sorted(set(cfg) - {"ks"})
        if unknown:
            raise ValueError(f"full_retrieval: unknown key(s) {unknown}; the mapping form is {{'ks': [...]}}")
        return check_retrieval_ks(cfg["ks"]) if cfg.get("ks") is not None else RetrievalMetrics("").ks
    raise ValueError(f"full_retrieval must be None, a bool or a mapping {{'ks': [...]}}, got {type(cfg).__name__}: {cfg!r}")


class SpatialClipLitModule(torch.nn.Module):
    def __init__(self, net: SpatialClipNet, loss_fn: torch.nn.Module, optimizer_cfg: Callable, scheduler_cfg: Callable,
                 train_metrics: Optional[ContrastiveMetrics] = None, val_metrics: Optional[ContrastiveMetrics] = None,
                 test_metrics: Optional[ContrastiveMetrics] = None, global_hvg_path: Optional[str] = None,
                 dist_net: Optional[SpatialClipNet] = None, param_groups: Any = None, full_retrieval: Any = None):
        super().__init__()
        # full-set retrieval metrics of validation / test (config key model.full_retrieval; open_clip's get_clip_metrics):
        # None / False -- off, nothing is allocated or launched; True or {"ks": [...]} -- one RetrievalMetrics per prefix
        ks = check_full_retrieval_cfg(full_retrieval)
        self.val_retrieval = RetrievalMetrics("val/", ks) if ks else None
        self.test_retrieval = RetrievalMetrics("test/", ks) if ks else None
        # optimiser parameter groups (config key model.param_groups): None -- the reference's un-grouped
        # optimizer_cfg(params=self.parameters()); a mapping {"no_decay": "open_clip" | None, "lr_scale": {prefix: factor}};
        # or a callable (net) -> list of group dicts.  Checked here, so that a bad key fails before anything trains.
        from . import optim
        self.param_groups = optim.check_param_groups_cfg(param_groups)
        # distillation teacher (open_clip --distill-model / --distill-pretrained): frozen, evaluated under no_grad on the
        # student's batch.  Kept OUT of the module tree (a tuple is not a submodule): parameters(), state_dict(), checkpoints,
        # the optimiser and the DDP gradient exchange see the student alone, and module.train() cannot take it out of eval().
        check_teacher_binding(loss_fn, dist_net is not None)
        if dist_net is not None:
            check_teacher_config(net.cfg, dist_net.cfg)
            dist_net.eval()
        self._teacher = (dist_net,)
        self._loss_terms: Dict[str, torch.Tensor] = {}
        self.hparams = _HParams(optimizer_cfg=optimizer_cfg, scheduler_cfg=scheduler_cfg,
                                global_hvg_path=global_hvg_path)      # save_hyperparameters(ignore=[net, loss_fn])
        self.net = net
        self.loss_fn = loss_fn
        self.train_metrics = train_metrics or ContrastiveMetrics("train/")
        self.val_metrics = val_metrics or ContrastiveMetrics("val/")
        self.test_metrics = test_metrics or ContrastiveMetrics("test/")
        self.global_hvg_path = global_hvg_path
        # validation-only zero-shot path (spatial_clip_module.py:36-41)
        self.zero_shot_metric = ZeroShotGeneExpressionMetric(global_hvg_path=global_hvg_path) if global_hvg_path else None
        self.gene_bank_embeddings = None
        self.trainer = None
        self._feature_gather = None
        self.logged: Dict[str, Any] = {}
        self.synced = set()                    # names logged with sync_dist=True
        # spatial_clip_module.py:44 -- cache the kwarg names the loss accepts, once
        self._loss_fn_arg_names = set(inspect.signature(self.loss_fn.forward).parameters.keys())

    @property
    def device(self) -> torch.device:
        return self.net.device_

    @property
    def dist_net(self) -> Optional[SpatialClipNet]:
        """The frozen distillation teacher, or None."""
        return self._teacher[0]

    def teacher_features(self, batch: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        """``dist_image_features`` / ``dist_text_features`` / ``dist_logit_scale`` of the batch (open_clip_train/train.py:
        134-137): the teacher's evaluation forward -- all tokens, no patch dropout, nothing kept for a backward."""
        teacher = self.dist_net
        with torch.no_grad():
            out = teacher(batch["images"], batch["texts"])
        return {k: out[k[len("dist_"):]].detach() for k in TEACHER_KWARGS}

    def log(self, name: str, value, sync_dist: bool = False, **kw) -> None:
        """Collects into ``self.logged`` (device scalars, no host sync).  ``sync_dist=True`` (the reference sets it on
        every loss it logs, spatial_clip_module.py:105,107,113,121) marks the name in ``self.synced``: the trainer
        averages those values over the ranks when it turns them into host numbers (``comm.all_reduce_mean_scalars``,
        one collective per record)."""
        self.logged[name] = value.detach() if isinstance(value, torch.Tensor) else value
        if sync_dist:
            self.synced.add(name)

    def log_dict(self, metrics, **kw) -> None:
        self.logged["__metrics__" + metrics.prefix] = metrics

    def forward(self, images: torch.Tensor, texts: torch.Tensor) -> Dict[str, torch.Tensor]:
        return self.net(images, texts)

    def model_step(self, batch: Dict[str, Any], metrics: Optional[ContrastiveMetrics] = None) -> Dict[str, torch.Tensor]:
        # W > 1: let the net launch the feature all-gathers from inside its forward (text side under the vision tower,
        # image side under the first similarity GEMM); the loss picks the gathered tensors up by identity
        fg = None
        if comm.is_dist() and hasattr(self.loss_fn, "prefetched") and os.environ.get("SC_GATHER_OVERLAP", "1") != "0":
            fg = self._feature_gather
            if fg is None:
                fg = self._feature_gather = comm.FeatureGather(self.device)
            want_ids = "image_tile_ids" in self._loss_fn_arg_names
            fg.skip = frozenset(getattr(self.loss_fn, "skip_gather", ()))
            fg.begin(batch.get("image_tile_ids") if want_ids else None, batch.get("text_tile_ids") if want_ids else None)
        self.net.feature_gather = fg
        if hasattr(self.loss_fn, "prefetched"):
            self.loss_fn.prefetched = fg
        # the teacher goes first: its forward is over before the student's writes the activations the backward will read
        teacher_out = self.teacher_features(batch) if self.dist_net is not None else {}
        features = self.forward(batch["images"], batch["texts"])
        self.net.feature_gather = None
        available_data = {**features, **batch, **teacher_out}
        loss_input = {k: v for k, v in available_data.items() if k in self._loss_fn_arg_names}
        fused_hits = metrics is not None and hasattr(self.loss_fn, "recall_hits")
        if fused_hits:
            metrics._ensure(self.device)
            self.loss_fn.recall_hits = metrics.hits      # R@k hit counting rides on the loss kernels' z matrix
        loss_dict = self.loss_fn(**loss_input)
        if fused_hits:
            metrics.add_hits(features["image_features"].shape[0])
            self.loss_fn.recall_hits = None
        terms = {}
        if isinstance(loss_dict, torch.Tensor):         # SigLipLoss: bare 0-d
            loss = loss_dict
        elif isinstance(loss_dict, tuple):              # DistillClipLoss: (contrastive_loss, distill_loss)
            terms = dict(zip(("contrastive_loss", "distill_loss"), loss_dict))
        elif len(loss_dict) > 1:
            terms = dict(loss_dict)
        else:
            loss = loss_dict["contrastive_loss"]
        if terms:       # open_clip_train/train.py: total_loss = sum(losses.values()) -- a device add, no host sync
            loss = functools.reduce(operator.add, terms.values())
        self._loss_terms = terms
        return StepOutput({"loss": loss, "image_features": features["image_features"],
                           "text_features": features["text_features"], "logit_scale": features["logit_scale"]})

    def _log_terms(self, prefix: str, **kw) -> None:
        """``<prefix>contrastive_loss`` / ``<prefix>distill_loss`` beside ``<prefix>loss`` (their sum) for a multi-term loss."""
        for name, value in self._loss_terms.items():
            self.log(prefix + name, value, **kw)

    @staticmethod
    def local_logits(output: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``image_features @ text_features.T * logit_scale`` (spatial_clip_module.py:68), on demand."""
        f_i = dict.__getitem__(output, "image_features").detach().contiguous()
        f_t = dict.__getitem__(output, "text_features").detach().contiguous()
        B, D = f_i.shape
        z = torch.empty((B, B), dtype=torch.float32, device=f_i.device)
        ops.sgemm(f_i, D, 1, f_t, D, 1, z, B, B, B, D)
        return z * dict.__getitem__(output, "logit_scale").detach()

    def root_gradient(self, loss: torch.Tensor) -> torch.Tensor:
        """The 1.0 that ``loss.backward()`` would materialise with an ATen fill on every step, kept resident instead:
        ``loss.backward(module.root_gradient(loss))`` leaves no ATen kernel in the training step."""
        g = getattr(self, "_root_grad", None)
        if g is None or g.device != loss.device or g.dtype != loss.dtype:
            g = self._root_grad = torch.ones((), dtype=loss.dtype, device=loss.device)
        return g

    def training_step(self, batch: Dict[str, Any], batch_idx: int) -> torch.Tensor:
        output = self.model_step(batch, self.train_metrics)
        self.log("train/loss", output["loss"], on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        self._log_terms("train/", on_step=True, on_epoch=True, sync_dist=True)
        self.log_dict(self.train_metrics, on_step=False, on_epoch=True, sync_dist=True)
        return output["loss"]

    # ------------------------------------------------------------------ cached-feature gradient accumulation (accum_freq)
    def check_cached_accumulation(self, accum_freq: int) -> None:
        """What the cached-feature form cannot run with; ValueError naming the offending values."""
        from . import losses
        if self.dist_net is not None or isinstance(self.loss_fn, losses.DistillClipLoss):
            raise ValueError(f"accum_freq={accum_freq} with {type(self.loss_fn).__name__} / dist_net: distillation has no "
                             "cached-feature form here (the teacher's features would need a cache of their own); use accum_freq=1")
        if not isinstance(self.loss_fn, (losses.ClipLoss, losses.SpatialLoss, losses.SigLipLoss)):
            raise ValueError(f"accum_freq={accum_freq} with {type(self.loss_fn).__name__}: the group loss is evaluated by the "
                             "fused head; ClipLoss, SpatialLoss and SigLipLoss are supported")
        if getattr(self.net, "precision", "bf16") == "fp8":
            raise ValueError(f"accum_freq={accum_freq} with precision='fp8': the caching pass would advance the delayed scaling")
        if comm.is_dist():
            raise ValueError(f"accum_freq={accum_freq} under a process group of {comm.world()[1]} ranks: the group cache is "
                             "single-process")

    def group_accumulator(self, accum_freq: int):
        """The ``optim.GradAccumulator`` (scale 1: the group loss is already a mean over all N * B pairs) the group step folds with."""
        from . import optim
        acc = getattr(self, "_group_accum", None)
        if acc is None or acc.every != accum_freq or acc.store is not self.net.store:
            acc = self._group_accum = optim.GradAccumulator(self.net.store, accum_freq, scale=1.0)
        return acc

    def _group_cache(self, N: int, B: int, D: int, K: Optional[int]) -> Dict[str, Optional[torch.Tensor]]:
        """The caches of one group shape, allocated once: features [N*B, D] of both towers and, for SpatialLoss (K is not None),
        the tile ids [N*B] and the neighbour ids / alphas [N*B, K]."""
        key = (N, B, D, K)
        c = getattr(self, "_group_caches", None)
        if c is None or c["key"] != key:
            G, dev = N * B, self.device
            c = {"key": key, "image": torch.empty((G, D), dtype=torch.float32, device=dev),
                 "text": torch.empty((G, D), dtype=torch.float32, device=dev), "ids_i": None, "ids_t": None, "nb": None, "al": None}
            if K is not None:
                c.update(ids_i=torch.empty(G, dtype=torch.int64, device=dev), ids_t=torch.empty(G, dtype=torch.int64, device=dev),
                         nb=torch.empty((G, K), dtype=torch.int64, device=dev),
                         al=torch.empty((G, K), dtype=torch.float32, device=dev))
            self._group_caches = c
        return c

    def cached_group_step(self, batches, partial: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimiser step's gradient from N micro-batches of B pairs as ONE batch of G = N * B (open_clip's ``--accum-freq``,
        open_clip_train/train.py:113-192).  Phase 1: ``net.cache_features`` on every micro-batch (training
        semantics, not differentiated), its features and SpatialLoss inputs copied into row block j of the group cache
        (``sc_group_cache_put``).  The loss: the fused head once on the cache, as a single-process batch of G -- a neighbour id
        found in another micro-batch's rows gets its weight.  Phase 2: each micro-batch forward again with the same patch
        dropout draw, its backward seeded with rows [jB, (j+1)B) of the head's feature gradients (views); the first one also
        takes d logit_scale / d logit_bias (ONCE per group: the exact gradient, where open_clip's loop applies it N times); each
        gradient is folded at scale 1 (``group_accumulator``).  On return ``store.grad`` holds the gradient of the group loss,
        ready for ``optimizer.step``; ``partial`` (``accumulator.sumsq_partial()``) collects the clip's sums of squares in the
        last fold.  Returns the group loss (0-d, device); ``train/loss`` logs it and the train metrics see the G x G block once."""
        from . import contrastive, losses, streams
        batches = list(batches)                 # the group keeps its N input batches until phase 2 has used them
        N = len(batches)
        if N < 1:
            raise ValueError("cached_group_step: an empty group")
        self.check_cached_accumulation(N)
        net, loss_fn = self.net, self.loss_fn
        spatial = isinstance(loss_fn, losses.SpatialLoss)
        siglip = isinstance(loss_fn, losses.SigLipLoss)
        accum = self.group_accumulator(N)
        self.net.feature_gather = None
        with streams.chain_stream():
            # ---- phase 1: features of every micro-batch, training semantics, nothing kept for a backward
            draw0 = net.patch_dropout_draw
            cache = None
            for j, b in enumerate(batches):
                img, txt = net.cache_features(b["images"], b["texts"], draw=draw0 + j)
                B, D = img.shape
                if cache is None:
                    K = int(b["neighbor_tile_ids"].shape[1]) if spatial else None
                    cache = self._group_cache(N, B, D, K)
                    B0 = B
                elif B != B0:
                    raise ValueError(f"cached_group_step: micro-batch {j} has {B} pairs, the group's first one {B0}: every "
                                     "micro-batch of a group must have the same size")
                if spatial:
                    ops.group_cache_put(img, txt, cache["image"], cache["text"], j, N,
                                        image_tile_ids=b["image_tile_ids"].contiguous(), text_tile_ids=b["text_tile_ids"].contiguous(),
                                        neighbor_tile_ids=b["neighbor_tile_ids"].contiguous(),
                                        neighbor_alphas=b["neighbor_alphas"].contiguous().float(),
                                        image_id_cache=cache["ids_i"], text_id_cache=cache["ids_t"],
                                        neighbor_id_cache=cache["nb"], neighbor_alpha_cache=cache["al"])
                else:
                    ops.group_cache_put(img, txt, cache["image"], cache["text"], j, N)
            # ---- the loss of the whole group, once, and its gradients with respect to the cached features
            has_bias = net.has_logit_bias
            net.store.wait_names(["logit_scale", "logit_bias"] if has_bias else ["logit_scale"])
            scale = torch.empty(1, dtype=torch.float32, device=self.device)
            ops.exp_scalar(net.store.p("logit_scale").view(1), scale)
            bias = net.store.p("logit_bias").detach() if has_bias else None
            metrics = self.train_metrics
            metrics._ensure(self.device)
            if siglip:
                res = contrastive.siglip_forward_backward(cache["image"], cache["text"], scale, bias, recall_hits=metrics.hits,
                                                          join_local=True)
            else:
                res = contrastive.contrastive_forward_backward(
                    cache["image"], cache["text"], scale, mode=loss_fn.mode, image_tile_ids=cache["ids_i"],
                    text_tile_ids=cache["ids_t"], neighbor_tile_ids=cache["nb"], neighbor_alphas=cache["al"],
                    cap_logit_scale=loss_fn.cap_logit_scale, temp_reg_weight=loss_fn.temp_reg_weight,
                    neighbor_alpha_scale=loss_fn.neighbor_alpha_scale, logit_bias=bias, recall_hits=metrics.hits,
                    want_recall=False, join_local=True)
            metrics.add_hits(N * B0)
            loss_fn.last = res
            loss = res["loss"]
            # ---- phase 2: each micro-batch again, differentiated, seeded with its rows of the group's feature gradients
            # (logit_scale / logit_bias: the group's gradient on the first micro-batch, a resident 0 on the others -- written by
            # the same in-tree launches, where ``None`` would zero them with an ATen fill)
            zero = getattr(self, "_zero1", None)
            if zero is None or zero.device != self.device:
                zero = self._zero1 = torch.zeros(1, dtype=torch.float32, device=self.device)
            replay = net.patch_dropout > 0.0 and net.training
            for j, b in enumerate(batches):
                if replay:
                    net.patch_dropout_draw = draw0 + j      # the draw of its caching pass: the same kept patches
                with torch.enable_grad():
                    net(b["images"], b["texts"])            # a training forward: the towers hold what this backward reads
                rows = slice(j * B0, (j + 1) * B0)
                net.store.wait_all()        # as _NetFn.backward: an update running behind the forward reads the gradients
                net._backward(res["d_image"][rows], res["d_text"][rows], res["d_scale"] if j == 0 else zero,
                              (res["d_bias"] if j == 0 else zero) if has_bias else None)
                last = j == N - 1
                accum.fold(j == 0, last, partial=partial if last else None)
        self._loss_terms = {}
        self.log("train/loss", loss, on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        self.log_dict(self.train_metrics, on_step=False, on_epoch=True, sync_dist=True)
        return loss

    def on_validation_start(self) -> None:
        """Build the gene bank once: text-tower embeddings of every gene name in ``global_hvg_path``
        (spatial_clip_module.py:73-103).  ``net.tokenizer`` must turn a list of gene names into token ids; the
        built-in one does not tokenise strings (BPE is CPU-side data preparation), so a data module that wants this
        metric installs its tokenizer on the net, as the reference's data module does."""
        if not self.zero_shot_metric or self.gene_bank_embeddings is not None:
            return
        path = self.global_hvg_path
        if not path or not os.path.exists(path):
            print(f"Warning: Global HVG path {path} not found.")
            return
        with open(path, "r") as f:
            gene_list = [line.strip() for line in f if line.strip()]
        if not gene_list:
            return
        embs = []
        with torch.no_grad():
            for i in range(0, len(gene_list), 256):
                tokens = self.net.tokenizer(gene_list[i:i + 256])
                tokens = tokens.to(self.device) if isinstance(tokens, torch.Tensor) else torch.as_tensor(tokens).to(self.device)
                embs.append(self.net.model.encode_text(tokens, normalize=True).float())
        self.gene_bank_embeddings = torch.cat(embs, dim=0).contiguous()

    def _zero_shot_update(self, batch: Dict[str, Any], output: Dict[str, torch.Tensor], name: str) -> None:
        if self.zero_shot_metric and self.gene_bank_embeddings is not None and "raw_text" in batch:
            f_i = output["image_features"].detach().float().contiguous()
            bank = self.gene_bank_embeddings
            B, D = f_i.shape
            n = bank.shape[0]
            logits = torch.empty((B, n), dtype=torch.float32, device=f_i.device)     # image_features @ bank.T
            ops.sgemm(f_i, D, 1, bank, D, 1, logits, n, B, n, D)
            self.zero_shot_metric.update(logits, batch["raw_text"])
            self.log(name, self.zero_shot_metric, on_step=False, on_epoch=True, sync_dist=True)

    def validation_step(self, batch: Dict[str, Any], batch_idx: int) -> None:
        with torch.no_grad():
            output = self.model_step(batch, self.val_metrics)
        self.log("val/loss", output["loss"], on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)
        self._log_terms("val/", on_step=False, on_epoch=True, sync_dist=True)
        self.log_dict(self.val_metrics, on_step=False, on_epoch=True, sync_dist=True)
        if self.val_retrieval is not None:
            self.val_retrieval.update(output["image_features"], output["text_features"])
        self._zero_shot_update(batch, output, "val/zero_shot_pcc")

    def test_step(self, batch: Dict[str, Any], batch_idx: int) -> None:
        with torch.no_grad():
            output = self.model_step(batch, self.test_metrics)
        self.log("test/loss", output["loss"], on_step=False, on_epoch=True, sync_dist=True)
        self._log_terms("test/", on_step=False, on_epoch=True, sync_dist=True)
        self.log_dict(self.test_metrics, on_step=False, on_epoch=True, sync_dist=True)
        if self.test_retrieval is not None:
            self.test_retrieval.update(output["image_features"], output["text_features"])
        self._zero_shot_update(batch, output, "test/zero_shot_pcc")

    def optimizer_param_groups(self):
        """The group dicts ``param_groups`` asks for.  The base learning rate and weight decay are the ones ``optimizer_cfg``
        will build the optimiser with: its bound keywords (a ``functools.partial``, as Hydra's ``_partial_`` gives), else the
        defaults of its signature."""
        from . import optim
        if callable(self.param_groups):
            return list(self.param_groups(self.net))
        cfg = self.hparams.optimizer_cfg

        def bound(key):
            keywords = getattr(cfg, "keywords", None) or {}
            if key in keywords:
                return keywords[key]
            par = inspect.signature(getattr(cfg, "func", cfg)).parameters.get(key)
            if par is None or par.default is inspect.Parameter.empty:
                raise ValueError(f"param_groups: optimizer_cfg neither binds {key!r} nor has a default for it, and the groups "
                                 "are scaled from it")
            return par.default
        return optim.build_param_groups(self.net, self.param_groups, lr=float(bound("lr")),
                                        weight_decay=float(bound("weight_decay")))

    def configure_optimizers(self) -> Dict[str, Any]:
        if self.param_groups is None:
            optimizer = self.hparams.optimizer_cfg(params=self.parameters())
        else:
            optimizer = self.hparams.optimizer_cfg(params=self.optimizer_param_groups())
        if self.trainer is None:
            return {"optimizer": optimizer}
        if self.trainer.max_steps == -1:
            total_steps = self.trainer.estimated_stepping_batches if self.trainer.max_epochs is not None else 1_000_000
        else:
            total_steps = self.trainer.max_steps
        if total_steps == float("inf") or total_steps == -1:
            total_steps = 1_000_000
        scheduler = self.hparams.scheduler_cfg(optimizer=optimizer, num_training_steps=int(total_steps))
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "monitor": self.hparams.get("optimized_metric", "val/loss"),
                                 "interval": "step", "frequency": 1}}
