"""Optimiser and LR schedule with the reference's config surface.

``FusedAdamW(params, lr, betas, eps, weight_decay)`` takes the kwargs of ``torch.optim.AdamW``
(configs/optimizer/adamw.yaml) and applies one fused kernel over the flat fp32 buffers of the ParamStore: global
grad-norm clip (Lightning ``gradient_clip_val``), DDP's 1/world_size mean, decoupled weight decay on ALL
parameters (the reference passes ``self.parameters()`` un-grouped, src/models/spatial_clip_module.py:139) and the
bf16 compute-copy refresh.  ``params`` may also be torch's other form, a list of ``{"params": [...], "lr": ...,
"weight_decay": ...}`` dicts (``open_clip_param_groups``, ``scaled_lr_groups``): with two or more groups every step form
launches ``ops.adamw_step_groups``, one streaming launch per range with a per-slot group table.
``FusedLion(params, lr, betas, weight_decay)`` takes the kwargs of ``lion_pytorch.Lion`` / ``timm.optim.Lion`` and runs the
same step forms with one moment (``ops.lion_step*``); ``FusedLamb`` takes the kwargs of ``timm.optim.Lamb``
and runs them with per-tensor trust ratios (``ops.lamb_*``, section 4m); ``FusedMuon`` takes the kwargs of ``torch.optim.Muon``,
orthogonalises the block Linears' updates by Newton-Schulz GEMMs and runs AdamW on the rest (``ops.muon_*``, section 4p); all four are
``_FlatOptimizer`` with their own launches.
``WeightAverager`` keeps an averaged copy of the weights (Lightning's ``EMAWeightAveraging`` / ``WeightAveraging``) in a flat
buffer of its own, updated behind every piece of those step forms (``ops.weight_average*``, section 4n).
``get_cosine_schedule_with_warmup`` reproduces transformers' LambdaLR schedule
(configs/scheduler/cosine.yaml): the first optimiser step runs with lr = 0."""
from __future__ import annotations

import math
import os
from typing import Any, Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import torch

from . import ops


class _FlatOptimizer:
    """Everything the fused optimisers share: parameter groups and their slot table, trainable ranges and the compact moment
    layout under a lock, the clip, every step form (one launch per range, bucket by bucket behind the next forward, the
    graph-captured form, the sharded form) and the checkpoint layout.  A subclass names itself (``NAME``), lists its state
    tensors (``STATE``: attributes of that name, one flat fp32 buffer each) and supplies the launches: ``_update`` (a piece
    with host scalars), ``_update_dev`` (the same with its step-dependent scalars in device memory), ``_update_groups`` (the
    grouped form), ``_refresh_scalar_hyper`` / ``_fill_group_hyper`` (the device scalars of the step about to run)."""
    NAME = ""
    STATE: Tuple[str, ...] = ()
    KIND: Optional[str] = None      # the "optimizer" entry of state_dict(); None: the key is not written (AdamW files)
    SHARDABLE = True                # comm.ShardedGradExchange is supported

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float, betas, eps: Optional[float], weight_decay: float):
        params = list(params)
        self.chunk_group: Optional[torch.Tensor] = None     # two or more groups: uint8 group of every 64-float slot (device)
        self.group_hyper: Optional[torch.Tensor] = None     # ... and their device scalars (refresh_hyper / _refresh_group_hyper)
        self._group_hyper_behind: Optional[torch.Tensor] = None     # the same for the form that launches on the communication stream
        self._group_stage: list = []                         # pinned staging ring of the same: [host tensor, event of its copy]
        self._group_stage_next = 0
        if params and all(isinstance(g, Mapping) for g in params):
            self._init_groups(params, lr, tuple(betas), eps, weight_decay)
        else:
            if any(isinstance(g, Mapping) for g in params):
                raise ValueError(f"{self.NAME}: params mixes parameters and group dicts; pass either an iterable of parameters or "
                                 "an iterable of {'params': [...], ...} dicts")
            stores = {id(getattr(p, "_sc_store", None)): getattr(p, "_sc_store", None) for p in params}
            if len(stores) != 1 or None in stores.values():
                raise ValueError(f"{self.NAME} needs the parameters of exactly one SpatialClipNet (flat ParamStore)")
            self.store = next(iter(stores.values()))
            if len(params) != len(self.store.specs):
                raise ValueError(f"{self.NAME} updates the whole flat buffer: pass all parameters (reference passes "
                                 "self.parameters() un-grouped)")
            self.param_groups = [{"params": params, "lr": lr, "initial_lr": lr, "betas": tuple(betas),
                                  **({} if eps is None else {"eps": eps}), "weight_decay": weight_decay}]
        # Locked towers (SpatialClipNet.lock_image_tower / lock_text_tower): Lightning still passes every parameter; the ones
        # with requires_grad=False get what torch.optim.AdamW gives a parameter without .grad -- no update, no weight decay, no
        # moments.  Every step form runs over the trainable ranges of the flat buffers (one range, the whole buffer, without a
        # lock) and the moments are laid out compactly: range k starts at ``self._moff[k]``.
        self.ranges: List[Tuple[int, int]] = list(self.store.trainable_ranges())
        self._moff: List[int] = []
        n = 0
        for lo, hi in self.ranges:
            self._moff.append(n)
            n += hi - lo
        self.store.optimizer_built = True       # the lock methods refuse from here on
        dev = self.store.device
        self._alloc_state(n)
        self.norm_clip = torch.zeros(2, dtype=torch.float32, device=dev)
        self._range_partials: Optional[torch.Tensor] = None     # locked: 1024 fp64 sums of squares per trainable range
        self.step_count = 0
        self.exchange = None        # comm.ShardedGradExchange when this rank owns 1/W of every gradient bucket
        self._behind = None         # bucket plan of the replicated optimiser's overlapped form (_step_behind_forward)
        # graph-captured steps (graph.GraphedTrainStep): the step-dependent scalars live in device memory
        self.hyper = None           # fp32, what _refresh_scalar_hyper writes (AdamW: {lr, 1 - beta1^step, sqrt(1 - beta2^step)})
        self._hyper_host = None     # pinned staging of the same
        self.averager: Optional["WeightAverager"] = None    # WeightAverager.attach: an averaged copy of the weights

    def _alloc_state(self, n: int) -> None:
        for name in self.STATE:
            setattr(self, name, torch.zeros(n, dtype=torch.float32, device=self.store.device))

    def _state(self) -> List[torch.Tensor]:
        return [getattr(self, name) for name in self.STATE]

    # ---- the launches a subclass supplies
    def _update(self, lo: int, hi: int, moments, grad_scale: float, clip) -> None:
        """flat[lo:hi] with the scalars of ``param_groups[0]`` as host arguments; ``moments``: the state slices of the piece."""
        raise NotImplementedError

    def _update_dev(self, lo: int, hi: int, moments, grad_scale: float, clip) -> None:
        """The same with the step-dependent scalars read from ``self.hyper`` (``_refresh_scalar_hyper``)."""
        raise NotImplementedError

    def _update_groups(self, lo: int, hi: int, moments, grad_scale: float, clip, table: torch.Tensor) -> None:
        """The grouped form: one launch, slot table ``self.chunk_group[lo // 64:]``, device scalars ``table``."""
        raise NotImplementedError

    def _refresh_scalar_hyper(self) -> None:
        """One group: the step-dependent scalars of the step about to run into ``self.hyper`` (an async copy)."""
        raise NotImplementedError

    def _group_hyper_floats(self, n_groups: int) -> int:
        raise NotImplementedError

    def _fill_group_hyper(self, host: torch.Tensor) -> None:
        """Two or more groups: the same for every group into the pinned HOST tensor ``host``."""
        raise NotImplementedError

    def _uses_table(self) -> bool:
        """The launches read a device table of scalars (``group_hyper``): with two or more groups."""
        return self.chunk_group is not None

    def _clip_threshold(self, max_norm: Optional[float]) -> Optional[float]:
        """The threshold ``_clip`` clips at, from the ``max_norm`` a step form was called with."""
        return max_norm

    def _before_pieces(self, grad_scale: float, clip, table: Optional[torch.Tensor]) -> None:
        """Launches of a step that must cover EVERY trainable range before the first ``_update_piece`` (LAMB: the moments and
        the per-tensor trust ratios), on the stream of the pieces; ``table`` as in ``_update_piece``."""

    # ---- parameter groups
    GROUP_KEYS = ("params", "lr", "weight_decay", "betas", "eps", "initial_lr", "param_names")
    MAX_GROUPS = 256        # the slot table holds one byte per slot, the kernel 256 {decay, step} pairs in LDS

    def _init_groups(self, groups: Sequence[Mapping], lr: float, betas, eps: float, weight_decay: float) -> None:
        """``params`` as a list of group dicts: validate, lay ``param_groups`` out and -- with two or more groups -- build the
        slot table.  Every failure is a ValueError that names the parameter or key."""
        if len(groups) > self.MAX_GROUPS:
            raise ValueError(f"{self.NAME}: {len(groups)} parameter groups; at most {self.MAX_GROUPS} are supported (one byte per "
                             "64-float slot names the group)")
        out, store, seen = [], None, {}
        for gi, g in enumerate(groups):
            unknown = [k for k in g if k not in self.GROUP_KEYS]
            if unknown:
                raise ValueError(f"{self.NAME}: parameter group {gi} has unknown key(s) {unknown}; accepted: "
                                 f"{list(self.GROUP_KEYS)}")
            if "params" not in g:
                raise ValueError(f"{self.NAME}: parameter group {gi} has no 'params'")
            if "betas" in g and tuple(float(b) for b in g["betas"]) != tuple(float(b) for b in betas):
                raise ValueError(f"{self.NAME}: parameter group {gi} sets betas={tuple(g['betas'])}; per-group betas are not "
                                 f"supported (the optimiser's are {tuple(betas)})")
            if "eps" in g and float(g["eps"]) != float(eps):
                raise ValueError(f"{self.NAME}: parameter group {gi} sets eps={g['eps']}; per-group eps is not supported (the "
                                 f"optimiser's is {eps})")
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            names = []
            for p in ps:
                st = getattr(p, "_sc_store", None)
                if st is None:
                    raise ValueError(f"{self.NAME}: parameter group {gi} holds a tensor of shape {tuple(getattr(p, 'shape', ()))} "
                                     "that is no parameter of a SpatialClipNet (flat ParamStore)")
                if store is None:
                    store = st
                    by_id = {id(q): n for n, q in st.params.items()}
                elif st is not store:
                    raise ValueError(f"{self.NAME}: parameter group {gi} holds parameters of another SpatialClipNet; all groups "
                                     "must share one flat ParamStore")
                name = by_id[id(p)]
                if name in seen:
                    raise ValueError(f"{self.NAME}: parameter {name} is listed twice (groups {seen[name]} and {gi})")
                seen[name] = gi
                names.append(name)
            g_lr = float(g.get("lr", lr))
            out.append({"params": ps, "lr": g_lr, "initial_lr": float(g.get("initial_lr", g_lr)), "betas": tuple(betas),
                        **({} if eps is None else {"eps": eps}), "weight_decay": float(g.get("weight_decay", weight_decay)),
                        "param_names": names})
        if store is None:
            raise ValueError(f"{self.NAME}: the parameter groups hold no parameters")
        missing = [n for n, p in store.params.items() if p.requires_grad and n not in seen]
        if missing:
            raise ValueError(f"{self.NAME}: {len(missing)} trainable parameter(s) are in no group (first: {missing[0]}); every "
                             "parameter with requires_grad=True must be in exactly one group")
        self.store = store
        self.param_groups = out
        if len(out) > 1:
            self.chunk_group = slot_table(store, [g["param_names"] for g in out]).to(store.device)
            self._alloc_group_hyper(len(out))

    def _alloc_group_hyper(self, n_groups: int) -> None:
        """The device scalar tables of ``n_groups`` groups and their pinned staging ring: allocated where the optimiser is
        built, on the stream it is built on, not inside a step."""
        dev = self.store.device
        n = self._group_hyper_floats(n_groups)
        cuda = torch.device(dev).type == "cuda"
        self.group_hyper = torch.zeros(n, dtype=torch.float32, device=dev)
        self._group_hyper_behind = torch.zeros(n, dtype=torch.float32, device=dev)
        for _ in range(4):
            host = torch.zeros(n, dtype=torch.float32)
            self._group_stage.append([host.pin_memory() if cuda else host, None])

    def _refresh_group_hyper(self, behind: bool = False) -> torch.Tensor:
        """Two or more groups: {1 - beta1^step, sqrt(1 - beta2^step)} and every group's {lr, weight_decay} for the step about
        to run (``step_count`` already advanced) into device memory: one small async copy on the CURRENT stream, in front of
        the launches that read it on that stream; returns the device table.  The forms that launch on the stream of the step
        (one launch per range, graph-captured) share ``self.group_hyper``.  ``behind``: the form that launches on the
        communication stream calls this with that stream current and has a table of its own, written and read on that stream
        alone -- so the copy waits for nothing but the previous update and lands while the backward still runs, off the
        path to the first bucket.  The pinned staging is a ring of four, each with the event of its last copy, so that a host
        running ahead of the device never rewrites floats a pending copy still has to read."""
        dev = self.store.device
        cuda = torch.device(dev).type == "cuda"
        slot = self._group_stage[self._group_stage_next]
        self._group_stage_next = (self._group_stage_next + 1) % len(self._group_stage)
        if slot[1] is not None:
            slot[1].synchronize()
        self._fill_group_hyper(slot[0])
        table = self._group_hyper_behind if behind else self.group_hyper
        table.copy_(slot[0], non_blocking=True)
        if cuda:
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(dev))
        return table

    def _update_piece(self, k: int, lo: int, hi: int, grad_scale: float, clip, table: Optional[torch.Tensor] = None,
                      dev: bool = False) -> None:
        """The update of flat[lo:hi], a piece of trainable range ``k`` (lo a multiple of 64): one launch, in the grouped form
        with two or more groups, else with host scalars or (``dev``) device scalars."""
        moments = self._moments(k, lo, hi)
        if self._uses_table():
            self._update_groups(lo, hi, moments, grad_scale, clip, self.group_hyper if table is None else table)
        elif dev:
            self._update_dev(lo, hi, moments, grad_scale, clip)
        else:
            self._update(lo, hi, moments, grad_scale, clip)

    def attach_exchange(self, exchange) -> None:
        """Data-parallel runs: hand the optimiser the gradient exchange of the process group.  With a
        ``comm.ShardedGradExchange`` the optimiser state shrinks to this rank's 1/W of every bucket (Adam moments: 8 bytes
        per parameter / W) and ``step`` becomes reduce-scattered gradients -> grad-norm (one tiny all-reduce) -> AdamW on the
        shard -> all-gather of the updated masters behind the next forward.  Anything else (None, the all-reduce reducer)
        keeps the replicated optimiser.  Call before ``load_state_dict``."""
        from . import comm
        if not isinstance(exchange, comm.ShardedGradExchange):
            self.exchange = None
            return
        if not self.SHARDABLE:
            raise ValueError(f"{self.NAME}: the sharded gradient exchange (SC_GRAD_EXCHANGE=sharded) is not supported; use the "
                             "all-reduce exchange")
        if len(self.param_groups) > 1:
            raise ValueError(f"{self.NAME}: {len(self.param_groups)} parameter groups with the sharded gradient exchange "
                             "(SC_GRAD_EXCHANGE=sharded) are not supported; use the all-reduce exchange")
        if self.store.locked:
            raise ValueError(f"{self.NAME}: a locked tower with the sharded gradient exchange (SC_GRAD_EXCHANGE=sharded) is not "
                             "supported; use the all-reduce exchange")
        self.exchange = exchange
        self._alloc_state(exchange.shard_floats())
        dev = self.store.device
        self._partials = torch.zeros(1024 * len(exchange.buckets), dtype=torch.float64, device=dev)

    def _clip(self, grad_scale: float, max_norm: Optional[float], sumsq_partial: Optional[torch.Tensor]):
        """The clip coefficient of the replicated forms (None: no clipping).  ``sumsq_partial``: 1024 fp64 partial sums of squares
        of the gradient, left by the pass that formed it (``GradAccumulator.fold`` of a group's last micro-batch): the norm is
        finished from them and the gradient is not read a second time."""
        max_norm = self._clip_threshold(max_norm)
        if max_norm is None or max_norm <= 0:
            return None
        st = self.store
        if sumsq_partial is not None:
            ops.grad_norm_final(sumsq_partial, sumsq_partial.numel(), grad_scale, max_norm, self.norm_clip)
        elif self.ranges == [(0, st.total)]:
            ops.grad_norm(st.grad, st.total, grad_scale, max_norm, self.norm_clip)
        else:       # trainable gradients only, as clip_grad_norm_ sees them: the locked ranges are not read
            if self._range_partials is None:
                self._range_partials = torch.zeros(1024 * len(self.ranges), dtype=torch.float64, device=st.grad.device)
            for k, (lo, hi) in enumerate(self.ranges):
                ops.grad_sumsq_partial(st.grad[lo:hi], hi - lo, self._range_partials[1024 * k:1024 * (k + 1)])
            ops.grad_norm_final(self._range_partials, self._range_partials.numel(), grad_scale, max_norm, self.norm_clip)
        return self.norm_clip

    def _moments(self, k: int, lo: int, hi: int):
        """Moment slices of flat[lo:hi], a piece of trainable range ``k``."""
        a = self._moff[k] + lo - self.ranges[k][0]
        return tuple(t[a:a + hi - lo] for t in self._state())

    def _step_sharded(self, grad_scale: float, max_norm: Optional[float]) -> torch.Tensor:
        st, ex = self.store, self.exchange
        st.wait_all()               # a step without a forward in between (tests): the previous gathers must have landed
        clip = None
        if max_norm is not None and max_norm > 0:
            for k in range(len(ex.buckets)):
                a, b = ex.piece(k)
                ops.grad_sumsq_partial(st.grad[a:b], b - a, self._partials[1024 * k:1024 * (k + 1)])
            ex.all_reduce_partials(self._partials)
            ops.grad_norm_final(self._partials, self._partials.numel(), grad_scale, max_norm, self.norm_clip)
            clip = self.norm_clip
        off = {}
        pos = 0
        for k in range(len(ex.buckets)):
            a, b = ex.piece(k)
            off[k] = pos
            pos += b - a
        for k in ex.order:          # in the order the next forward consumes the buckets
            a, b = ex.piece(k)
            self._update(a, b, tuple(t[off[k]:off[k] + (b - a)] for t in self._state()), grad_scale, clip)
            ex.gather_bucket(k)
        return self.norm_clip

    # ---- replicated optimiser, update hidden behind the next forward (round 5)
    def _behind_plan(self, bucket_floats: int = 16 * 1024 * 1024):
        """Static buckets of the flat buffers in the order the forward consumes them (the second tower runs first and sits at
        the END of the buffers), each with the derived weight copies that are complete once it is."""
        if self._behind is None:
            st = self.store
            size = max(64, (int(bucket_floats) + 63) // 64 * 64)
            buckets, owner = [], []          # owner: the trainable range a bucket is a piece of
            for r, (rlo, rhi) in enumerate(self.ranges):
                edges = list(range(rlo, rhi, size)) + [rhi]
                if len(edges) > 2 and edges[-1] - edges[-2] < size // 2:
                    edges.pop(-2)
                buckets += [(edges[k], edges[k + 1]) for k in range(len(edges) - 1)]
                owner += [r] * (len(edges) - 1)
            first_second = min((sp.offset for sp in st.specs if not sp.name.startswith("visual.")), default=0)
            k0 = next((k for k, (lo, hi) in enumerate(buckets) if hi > first_second), 0)
            order = list(range(k0, len(buckets))) + list(range(0, k0))
            pos = {k: i for i, k in enumerate(order)}
            copies = [[] for _ in buckets]
            for c in st.trainable_copies():      # a locked weight's copies were built once and never change
                sp = st.by_name[c.name]
                touched = [k for k, (lo, hi) in enumerate(buckets) if lo < sp.offset + sp.numel and sp.offset < hi]
                copies[max(touched, key=lambda k: pos[k])].append(c)
            self._behind = (buckets, order, copies, [st._transpose_plan(cs) for cs in copies], owner)
        return self._behind

    def _step_behind_forward(self, grad_scale: float, max_norm: Optional[float],
                             sumsq_partial: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The replicated update (one process, or the all-reduce route) bucket by bucket on the communication stream, in the order
        the next forward consumes the buckets: the forward waits per bucket at the first use of its parameters
        (``ParamStore.wait_names``, the mechanism of the sharded optimiser), so all but the first bucket of the HBM-bound update
        (AdamW: 30 bytes per parameter, Lion: 22) runs under the matrix-bound start of the next step.  Same kernels on the same values: weights
        bit-identical to the one-launch form (``SC_ADAMW_BEHIND=0``)."""
        from . import streams
        st = self.store
        st.wait_all()               # a step without a forward in between: the previous update must be complete
        wa = self.averager
        if wa is not None:
            wa.begin_step(self.step_count - 1)
        clip = self._clip(grad_scale, max_norm, sumsq_partial)
        buckets, order, copies, plans, owner = self._behind_plan(int(os.environ.get("SC_ADAMW_BUCKET", 16 * 1024 * 1024)))
        cur = torch.cuda.current_stream(st.device)
        side = streams.comm_stream(st.device)       # (a low-priority stream of its own measured the same on ViT-B/16, worse on ViT-L/14)
        table = None
        if self._uses_table():
            with torch.cuda.stream(side):   # in front of the wait for the backward: behind the last update in stream order only
                table = self._refresh_group_hyper(behind=True)
        ready = torch.cuda.Event()
        ready.record(cur)
        side.wait_event(ready)
        with torch.cuda.stream(side):
            self._before_pieces(grad_scale, clip, table)
            for k in order:
                lo, hi = buckets[k]
                self._update_piece(owner[k], lo, hi, grad_scale, clip, table)
                if wa is not None:          # on this stream, in front of the bucket's event: store.wait_all() covers it
                    wa.after_piece(lo, hi)
                st.refresh_range(lo, hi, copies[k], plans[k], fresh=(lo, hi))
                done = torch.cuda.Event()
                done.record(side)
                st.add_pending(lo, hi, done)
        return self.norm_clip

    # ---- graph-captured steps: identical launches every step, step-dependent scalars refreshed from the host
    def refresh_hyper(self) -> None:
        """Write {lr, 1 - beta1^step, sqrt(1 - beta2^step)} for the step about to run (``step_count`` already advanced) into
        the device triple ``self.hyper``: one 12-byte async H2D copy on the current stream, enqueued in front of the graph
        replay that reads it.  With two or more parameter groups: the group table ``self.group_hyper`` instead."""
        if self.averager is not None:
            self.averager.refresh_ctl(self.step_count - 1)
        if self._uses_table():
            self._refresh_group_hyper()
            return
        self._refresh_scalar_hyper()

    def step_captured(self, grad_scale: float = 1.0, max_norm: Optional[float] = None,
                      sumsq_partial: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The replicated one-launch update in the form a hipGraph can replay: clip coefficient and the step-dependent
        scalars from device memory (``refresh_hyper``), no host-side step counter.  Single process only."""
        if self.exchange is not None:
            raise RuntimeError("step_captured: the sharded optimiser issues collectives; graph capture is single-process")
        st = self.store
        st.wait_all()
        clip = self._clip(grad_scale, max_norm, sumsq_partial)
        self._before_pieces(grad_scale, clip, None)
        for k, (lo, hi) in enumerate(self.ranges):
            self._update_piece(k, lo, hi, grad_scale, clip, dev=True)
            if self.averager is not None:
                self.averager.after_piece_captured(lo, hi)
        st.refresh_compute_copies(mirror_is_fresh=True)
        return self.norm_clip

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Gradients are overwritten by every backward; nothing to clear."""

    def step(self, grad_scale: float = 1.0, max_norm: Optional[float] = None,
             sumsq_partial: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``sumsq_partial``: see ``_clip`` (accumulated steps of one process).  The replicated forms take it; the sharded
        optimiser forms its norm from per-shard partials and refuses it."""
        st = self.store
        if self.exchange is not None and sumsq_partial is not None:
            raise ValueError(f"{self.NAME}.step: sumsq_partial= is for the replicated optimiser; the sharded exchange "
                             "(SC_GRAD_EXCHANGE=sharded) computes its own per-shard partials")
        self.step_count += 1
        if self.exchange is not None:
            return self._step_sharded(grad_scale, max_norm)
        # Default: behind the forward for models up to 200 M parameters.  Measured (same box, interleaved): ViT-B/16 + gene-MLP
        # (97 M) -0.12 ms per step; ViT-L/14 + gene transformer (428 M) +0.3 ms whatever the bucket size or stream priority -- its
        # longer update and its forward contend for HBM longer than the overlap returns.  SC_ADAMW_BEHIND=1 / 0 forces either form.
        behind = os.environ.get("SC_ADAMW_BEHIND", "auto")
        if st.master.is_cuda and (behind == "1" or (behind not in ("0", "1") and st.total <= 200_000_000)):
            return self._step_behind_forward(grad_scale, max_norm, sumsq_partial)
        wa = self.averager
        if wa is not None:
            wa.begin_step(self.step_count - 1)
        clip = self._clip(grad_scale, max_norm, sumsq_partial)
        if self._uses_table():
            self._refresh_group_hyper()
        self._before_pieces(grad_scale, clip, None)
        for k, (lo, hi) in enumerate(self.ranges):
            self._update_piece(k, lo, hi, grad_scale, clip)
            if wa is not None:
                wa.after_piece(lo, hi)
        st.refresh_compute_copies(mirror_is_fresh=True)
        return self.norm_clip

    def state_dict(self):
        """Full flat-layout moments whatever the exchange (a checkpoint written by W ranks resumes on any W').  With the
        sharded exchange this is a COLLECTIVE: every rank must call it (the trainer does, before rank 0 writes the file)."""
        self.store.wait_all()           # an update may still be running behind the forward (communication stream)
        if self.exchange is not None:
            full = [self.exchange.gather_moments(t) for t in self._state()]
        elif self.ranges == [(0, self.store.total)]:
            full = [t.clone() for t in self._state()]
        else:       # the full flat layout, zeros in the locked ranges: the file resumes with or without the lock
            full = [self._expand(t) for t in self._state()]
        return {**({} if self.KIND is None else {"optimizer": self.KIND}), "step": self.step_count, **dict(zip(self.STATE, full)),
                "param_groups": [{k: v_ for k, v_ in g.items() if k != "params"} for g in self.param_groups]}

    def _check_kind(self, sd) -> None:
        """A checkpoint of another optimiser kind ("adamw", "lion", "lamb", "muon") is refused.  The kind is the "optimizer" entry; an
        AdamW file carries none (it was written before that entry existed, and still is) and is known by its second moment."""
        mine = self.KIND or "adamw"
        has_sq = "exp_avg_sq" in sd
        theirs = sd.get("optimizer", "adamw" if has_sq else "lion")
        if theirs != mine or has_sq != ("exp_avg_sq" in self.STATE):
            other = theirs if theirs != mine else ("adamw" if has_sq else "lion")
            kinds = ("AdamW and Lion" if {mine, other} == {"adamw", "lion"} else
                     "AdamW, Lion, LAMB and Muon" if "muon" in (mine, other) else "AdamW, Lion and LAMB")
            raise ValueError(f"{self.NAME}.load_state_dict: the state dict (keys {sorted(k for k in sd if k != 'param_groups')}) is "
                             f"that of an {other!r} optimiser; this one is {mine!r} and keeps {list(self.STATE)}.  {kinds} "
                             "states do not convert into each other")

    def load_state_dict(self, sd) -> None:
        self._check_kind(sd)
        self.store.wait_all()
        self.step_count = int(sd["step"])
        n = self.store.total
        full = [sd[name] for name in self.STATE]
        for i, m in enumerate(full):
            if m.numel() != n:      # a file written with another padding (other world size): the real parameters come first
                keep = min(m.numel(), n)
                m2 = torch.zeros(n, dtype=m.dtype, device=m.device)
                m2[:keep] = m[:keep]
                full[i] = m2
        if self.exchange is not None:
            for m, mine in zip(full, self._state()):
                self.exchange.scatter_moments(m.to(mine.device), mine)
        else:       # the trainable slices of the full layout
            for k, (lo, hi) in enumerate(self.ranges):
                for m, dm in zip(full, self._moments(k, lo, hi)):
                    dm.copy_(m[lo:hi])

    def _expand(self, compact: torch.Tensor) -> torch.Tensor:
        full = torch.zeros(self.store.total, dtype=compact.dtype, device=compact.device)
        for k, (lo, hi) in enumerate(self.ranges):
            full[lo:hi] = compact[self._moff[k]:self._moff[k] + hi - lo]
        return full


class FusedAdamW(_FlatOptimizer):
    NAME = "FusedAdamW"
    STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        super().__init__(params, lr, betas, eps, weight_decay)

    def _update(self, lo, hi, moments, grad_scale, clip) -> None:
        st, g = self.store, self.param_groups[0]
        m, v = moments
        ops.adamw_step(st.master[lo:hi], st.grad[lo:hi], m, v, hi - lo, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                       g["weight_decay"], self.step_count, grad_scale, clip, st.master_bf16[lo:hi])

    def _update_dev(self, lo, hi, moments, grad_scale, clip) -> None:
        st, g = self.store, self.param_groups[0]
        m, v = moments
        ops.adamw_step_dev(st.master[lo:hi], st.grad[lo:hi], m, v, hi - lo, self.hyper, g["betas"][0], g["betas"][1], g["eps"],
                           g["weight_decay"], grad_scale, clip, st.master_bf16[lo:hi])

    def _update_groups(self, lo, hi, moments, grad_scale, clip, table) -> None:
        st, g = self.store, self.param_groups[0]
        m, v = moments
        ops.adamw_step_groups(st.master[lo:hi], st.grad[lo:hi], m, v, hi - lo, self.chunk_group[lo // 64:], table,
                              len(self.param_groups), g["betas"][0], g["betas"][1], g["eps"], grad_scale, clip,
                              st.master_bf16[lo:hi])

    def _refresh_scalar_hyper(self) -> None:
        g = self.param_groups[0]
        if self.hyper is None:
            self.hyper = torch.zeros(3, dtype=torch.float32, device=self.store.device)
            self._hyper_host = torch.zeros(3, dtype=torch.float32).pin_memory()
        # formed by the library itself, with the expressions of sc_adamw_step: same bits as the eager launch
        from . import _lib
        _lib.check(_lib.lib().sc_adamw_hyper_host(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), int(self.step_count),
                                                  self._hyper_host.data_ptr()), "sc_adamw_hyper_host")
        self.hyper.copy_(self._hyper_host, non_blocking=True)

    def _group_hyper_floats(self, n_groups: int) -> int:
        return 2 + 2 * n_groups

    def _fill_group_hyper(self, host: torch.Tensor) -> None:
        g0 = self.param_groups[0]
        ops.adamw_groups_hyper_host([g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups],
                                    g0["betas"][0], g0["betas"][1], self.step_count, host)


class FusedLion(_FlatOptimizer):
    """Lion (Chen et al. 2023, Algorithm 1) with the keywords of ``lion_pytorch.Lion`` / ``timm.optim.Lion``: one moment
    (4 bytes of state per parameter), ``p = p (1 - lr wd) - lr sign(b1 m + (1 - b1) g)``, ``m = b2 m + (1 - b2) g``, no bias
    correction, no eps.  Parameter groups, locked towers, accumulation, the overlapped and the graph-captured step are
    ``FusedAdamW``'s, on the same code; the sharded gradient exchange is refused.  The options of the two public classes that
    change the update are accepted at their off value only."""
    NAME = "FusedLion"
    STATE = ("exp_avg",)
    KIND = "lion"
    SHARDABLE = False
    GROUP_KEYS = tuple(k for k in _FlatOptimizer.GROUP_KEYS if k != "eps")
    OFF_ONLY = {"use_triton": (False,), "decoupled_weight_decay": (False,), "caution": (False,), "maximize": (False,),
                "foreach": (None, False)}

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-4, betas=(0.9, 0.99), weight_decay: float = 0.0,
                 **options):
        for key, value in options.items():
            if key not in self.OFF_ONLY:
                raise ValueError(f"FusedLion: unknown keyword {key!r}; accepted: lr, betas, weight_decay and (off only) "
                                 f"{list(self.OFF_ONLY)}")
            if not any(value is off for off in self.OFF_ONLY[key]):
                raise ValueError(f"FusedLion: {key}={value!r} is not supported; only {key}={self.OFF_ONLY[key][0]!r} (the plain "
                                 "update of Algorithm 1 with decoupled weight decay) is")
        super().__init__(params, lr, betas, None, weight_decay)

    def _update(self, lo, hi, moments, grad_scale, clip) -> None:
        st, g = self.store, self.param_groups[0]
        ops.lion_step(st.master[lo:hi], st.grad[lo:hi], moments[0], hi - lo, g["lr"], g["betas"][0], g["betas"][1],
                      g["weight_decay"], grad_scale, clip, st.master_bf16[lo:hi])

    def _update_dev(self, lo, hi, moments, grad_scale, clip) -> None:
        st, g = self.store, self.param_groups[0]
        ops.lion_step_dev(st.master[lo:hi], st.grad[lo:hi], moments[0], hi - lo, self.hyper, g["betas"][0], g["betas"][1],
                          g["weight_decay"], grad_scale, clip, st.master_bf16[lo:hi])

    def _update_groups(self, lo, hi, moments, grad_scale, clip, table) -> None:
        st, g = self.store, self.param_groups[0]
        ops.lion_step_groups(st.master[lo:hi], st.grad[lo:hi], moments[0], hi - lo, self.chunk_group[lo // 64:], table,
                             len(self.param_groups), g["betas"][0], g["betas"][1], grad_scale, clip, st.master_bf16[lo:hi])

    def _refresh_scalar_hyper(self) -> None:
        if self.hyper is None:
            self.hyper = torch.zeros(1, dtype=torch.float32, device=self.store.device)
            self._hyper_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._hyper_host[0] = float(self.param_groups[0]["lr"])       # rounded to fp32 as the host-scalar launch rounds it
        self.hyper.copy_(self._hyper_host, non_blocking=True)

    def _group_hyper_floats(self, n_groups: int) -> int:
        return 2 * n_groups

    def _fill_group_hyper(self, host: torch.Tensor) -> None:
        ops.lion_groups_hyper_host([g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups], host)


class FusedLamb(_FlatOptimizer):
    """LAMB (You et al. 2020) with the keywords and defaults of ``timm.optim.Lamb``: Adam's moments, then per tensor -- one
    parameter of the store -- the trust ratio ``r = ||p|| / ||u||`` of ``u = m_hat / (sqrt(v_hat) + eps) + wd p`` and
    ``p -= lr r u``.  A tensor of a group without weight decay gets ``r = 1`` unless ``always_adapt``; ``trust_clip`` caps r at 1.
    timm's built-in clip (``max_grad_norm``) and the Trainer's ``gradient_clip_val`` compose to ONE clip at the smaller
    threshold, which is what runs (``_clip_threshold``).  A step is ``ops.lamb_moments`` over every trainable range,
    ``ops.lamb_trust`` once, ``ops.lamb_apply`` over the pieces of the step form; one group or many are the
    same launches, the device table carries every tensor's {lr, wd}.  Parameter groups, locked towers, accumulation, the
    overlapped and the graph-captured step are ``FusedAdamW``'s, on the same code; the sharded gradient exchange is refused."""
    NAME = "FusedLamb"
    STATE = ("exp_avg", "exp_avg_sq")
    KIND = "lamb"
    SHARDABLE = False
    ON_ONLY = ("bias_correction", "grad_averaging")
    OFF_ONLY = {"caution": (False,), "decoupled_decay": (False,), "maximize": (False,), "foreach": (None, False)}

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, max_grad_norm: Optional[float] = 1.0, trust_clip: bool = False,
                 always_adapt: bool = False, **options):
        for key, value in options.items():
            if key in self.ON_ONLY:
                if value is not True:
                    raise ValueError(f"FusedLamb: {key}={value!r} is not supported; only {key}=True (timm's default) is")
            elif key not in self.OFF_ONLY:
                raise ValueError(f"FusedLamb: unknown keyword {key!r}; accepted: lr, betas, eps, weight_decay, max_grad_norm, "
                                 f"trust_clip, always_adapt, (on only) {list(self.ON_ONLY)} and (off only) {list(self.OFF_ONLY)}")
            elif not any(value is off for off in self.OFF_ONLY[key]):
                raise ValueError(f"FusedLamb: {key}={value!r} is not supported; only {key}={self.OFF_ONLY[key][0]!r} (the plain "
                                 "update of timm.optim.Lamb) is")
        for key, value in (("trust_clip", trust_clip), ("always_adapt", always_adapt)):
            if not isinstance(value, bool):
                raise ValueError(f"FusedLamb: {key}={value!r}: True or False is expected")
        if max_grad_norm is not None and (isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float))
                                          or not math.isfinite(max_grad_norm) or max_grad_norm <= 0):
            raise ValueError(f"FusedLamb: max_grad_norm={max_grad_norm!r}: a positive float, or None for no built-in clip, is "
                             "expected")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.trust_clip, self.always_adapt = trust_clip, always_adapt
        super().__init__(params, lr, betas, eps, weight_decay)
        # the tensor tables, over the trainable parameters only: a locked parameter's slots belong to no tensor
        st = self.store
        names = st.trainable_names()
        group_of = {n: gi for gi, g in enumerate(self.param_groups) for n in g.get("param_names", ())}
        slot_tensor = torch.full((st.total // 64,), -1, dtype=torch.int32)
        tensor_slots = torch.zeros((len(names), 2), dtype=torch.int32)
        for ti, n in enumerate(names):
            sp = st.by_name[n]
            lo = sp.offset // 64
            hi = lo + (max(sp.numel, 1) + 63) // 64
            slot_tensor[lo:hi] = ti
            tensor_slots[ti, 0], tensor_slots[ti, 1] = lo, hi
        self.tensor_names = names
        self.tensor_group = torch.tensor([group_of.get(n, 0) for n in names], dtype=torch.int32)       # host: _fill_group_hyper
        dev = st.device
        self.slot_tensor, self.tensor_slots = slot_tensor.to(dev), tensor_slots.to(dev)
        self.slot_sums = torch.zeros(2 * (st.total // 64), dtype=torch.float32, device=dev)     # {sum p^2, sum u^2} per slot
        self.trust = torch.ones(len(names), dtype=torch.float32, device=dev)                    # r of the last step, per tensor
        if self.group_hyper is None:        # one group: the same table and staging ring as with many (_init_groups)
            self._alloc_group_hyper(1)

    def _uses_table(self) -> bool:
        return True

    def _clip_threshold(self, max_norm):
        given = [float(x) for x in (max_norm, self.max_grad_norm) if x is not None and x > 0]
        return min(given) if given else None

    def _group_hyper_floats(self, n_groups: int) -> int:
        return 2 + 2 * len(self.store.trainable_names())

    def _fill_group_hyper(self, host: torch.Tensor) -> None:
        g0 = self.param_groups[0]
        ops.lamb_hyper_host([g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups],
                            self.tensor_group, g0["betas"][0], g0["betas"][1], self.step_count, host)

    def _before_pieces(self, grad_scale, clip, table) -> None:
        st, g = self.store, self.param_groups[0]
        table = self.group_hyper if table is None else table
        n_tensors = len(self.tensor_names)
        for k, (lo, hi) in enumerate(self.ranges):
            m, v = self._moments(k, lo, hi)
            ops.lamb_moments(st.master[lo:hi], st.grad[lo:hi], m, v, hi - lo, self.slot_tensor[lo // 64:], table, n_tensors,
                             g["betas"][0], g["betas"][1], g["eps"], grad_scale, clip, self.slot_sums[2 * (lo // 64):])
        ops.lamb_trust(self.slot_sums, st.total // 64, self.tensor_slots, table, n_tensors, self.always_adapt, self.trust_clip,
                       self.trust)

    def _update_groups(self, lo, hi, moments, grad_scale, clip, table) -> None:
        st = self.store
        m, v = moments
        ops.lamb_apply(st.master[lo:hi], m, v, hi - lo, self.slot_tensor[lo // 64:], table, self.trust, len(self.tensor_names),
                       self.param_groups[0]["eps"], st.master_bf16[lo:hi])


MUON_LEAVES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")
MUON_ADJUST_LR = (None, "original", "match_rms_adamw")


def is_muon_name(name: str) -> bool:
    """The default rule: the four Linear weights of a transformer block of any tower -- a state-dict name that ends in one of
    ``MUON_LEAVES`` directly under a ``resblocks.<i>.``."""
    for leaf in MUON_LEAVES:
        if name.endswith("." + leaf):
            parts = name[:-len(leaf) - 1].split(".")
            return len(parts) >= 2 and parts[-2] == "resblocks" and parts[-1].isdigit()
    return False


def muon_shape_ok(shape) -> bool:
    """What the Newton-Schulz GEMMs take: a 2-D tensor, both dimensions positive multiples of 8."""
    return len(shape) == 2 and all(int(s) > 0 and int(s) % 8 == 0 for s in shape)


def muon_adjust_ratio(adjust_lr_fn: Optional[str], shape) -> float:
    """``lr_adj / lr`` of ``torch.optim._muon._adjust_lr`` for a parameter of ``shape``."""
    r, c = int(shape[0]), int(shape[1])
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(r, c))
    return math.sqrt(max(1, r / c))


def muon_param_groups(named_parameters, lr: Optional[float] = None, weight_decay: Optional[float] = None,
                      adamw_lr: Optional[float] = None, adamw_weight_decay: Optional[float] = None) -> List[Dict[str, Any]]:
    """The default split of ``FusedMuon``: the block Linears (``is_muon_name``, shapes the kernel takes) in a group with
    ``use_muon=True``, every other tensor -- embeddings, ``visual.proj`` / ``text_projection``, the gene-MLP, LayerNorm, biases,
    ``logit_scale`` / ``logit_bias`` -- in one with ``use_muon=False``.  ``named_parameters``: ``(name, tensor)`` pairs, names
    looked up in the ParamStore; a parameter with ``requires_grad=False`` is left out.  ``lr`` / ``weight_decay`` (and the
    ``adamw_*`` pair for the second group) are written into the groups when given; an empty group is dropped."""
    muon: Dict[str, Any] = {"params": [], "param_names": [], "use_muon": True}
    rest: Dict[str, Any] = {"params": [], "param_names": [], "use_muon": False}
    for key, value, g in (("lr", lr, muon), ("weight_decay", weight_decay, muon), ("lr", adamw_lr, rest),
                          ("weight_decay", adamw_weight_decay, rest)):
        if value is not None:
            g[key] = float(value)
    for name, p in named_parameters:
        if isinstance(p, torch.nn.Parameter) and not p.requires_grad:
            continue
        name = _reference_name(name, p)
        g = muon if is_muon_name(name) and muon_shape_ok(tuple(p.shape)) else rest
        g["params"].append(p)
        g["param_names"].append(name)
    return [g for g in (muon, rest) if g["params"]]


def muon_newton_schulz(x0: torch.Tensor, x1: torch.Tensor, lo: int, r: int, c: int, gbuf: torch.Tensor, pbuf: torch.Tensor,
                       acc: torch.Tensor, ns_steps: int, coefficients) -> torch.Tensor:
    """``ns_steps`` Newton-Schulz iterations on the matrix [r, c] at element ``lo`` of the compact bf16 buffers: X from ``x0`` to
    ``x1`` and back, never in place; returns the buffer that holds the result (``x1`` for an odd ``ns_steps``).  Three products
    per iteration through ``ops.gemm``; none needs a transpose, because G and P are symmetric: for r <= c ``G = X X^T`` (NT),
    ``G G`` (NT) and ``P X`` as the TN product with At = P; for r > c, where torch works on X^T, ``G = X_s^T X_s`` is the TN
    product of the stored matrix with itself and ``X_s P`` the NT product with B = P.  The two products with an epilogue leave
    fp32 accumulators (``EPI_F32``) in ``acc`` (r * c floats) that ``ops.muon_axpby`` combines with ``beta Cin`` and rounds once.
    ``gbuf`` / ``pbuf``: ``min(r, c)^2`` bf16 each."""
    m = min(r, c)
    a, b, cc = coefficients
    g, p = gbuf[:m * m].view(m, m), pbuf[:m * m].view(m, m)
    acc_mm, acc_x = acc[:m * m].view(m, m), acc[:r * c].view(r, c)
    bufs = (x0, x1)
    for it in range(ns_steps):
        x = bufs[it & 1][lo:lo + r * c].view(r, c)
        y = bufs[1 - (it & 1)][lo:lo + r * c].view(r, c)
        if r > c:
            ops.gemm(ops.TN, ops.EPI_BF16, x, x, g, M=c, N=c, K=r)
        else:
            ops.gemm(ops.NT, ops.EPI_BF16, x, x, g, M=r, N=r, K=c)
        ops.gemm(ops.NT, ops.EPI_F32, g, g, acc_mm, M=m, N=m, K=m)
        ops.muon_axpby(acc_mm, g, p, m * m, cc, b)
        if r > c:
            ops.gemm(ops.NT, ops.EPI_F32, x, p, acc_x, M=r, N=c, K=c)
        else:
            ops.gemm(ops.TN, ops.EPI_F32, p, x, acc_x, M=r, N=c, K=r)
        ops.muon_axpby(acc_x, x, y, r * c, 1.0, a)
    return x1 if ns_steps & 1 else x0


class FusedMuon(_FlatOptimizer):
    """Muon for the hidden matrices, AdamW for everything else, in one object.  The first nine arguments are the keywords and
    defaults of ``torch.optim.Muon`` (torch 2.10; its code, ``torch/optim/_muon.py``, is the reference): per Muon tensor a
    momentum buffer (``exp_avg``), ``ns_steps`` Newton-Schulz iterations on the bf16 update in the MFMA GEMMs of ``ops.gemm``
    (matrix by matrix; fp32 accumulators, one rounding per product) and ``p = p (1 - lr wd) - lr_adj O``.  The ``adamw_*`` arguments belong to the other
    part (``None``: the Muon value), which is ``FusedAdamW``'s grouped update bit for bit.  ``params``: a plain parameter list,
    split by the default rule (``muon_param_groups``), or group dicts; a dict may carry ``use_muon: bool``, one without it is split
    by the default rule.  ``use_muon=True`` is accepted for 2-D tensors whose two dimensions are multiples of 8.  A step is
    ``ops.muon_momentum`` over every trainable range, ``ops.muon_scale``, ``_newton_schulz`` per matrix (``_before_pieces``),
    then ``ops.muon_apply`` over the pieces of the step form.  Parameter groups, locked towers,
    accumulation, weight averaging, the overlapped and the graph-captured step are ``FusedAdamW``'s, on the same code; the
    sharded gradient exchange is refused."""
    NAME = "FusedMuon"
    STATE = ("exp_avg", "exp_avg_sq")
    KIND = "muon"
    SHARDABLE = False
    OFF_ONLY = {"maximize": (False,), "foreach": (None, False)}
    MUON_GROUP_KEYS = ("momentum", "nesterov", "ns_steps", "ns_coefficients", "adjust_lr_fn")

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, weight_decay: float = 0.1, momentum: float = 0.95,
                 nesterov: bool = True, ns_coefficients=(3.4445, -4.7750, 2.0315), eps: float = 1e-7, ns_steps: int = 5,
                 adjust_lr_fn: Optional[str] = None, adamw_lr: Optional[float] = None, adamw_betas=(0.9, 0.999),
                 adamw_eps: float = 1e-8, adamw_weight_decay: Optional[float] = None, **options):
        for key, value in options.items():
            if key not in self.OFF_ONLY:
                raise ValueError(f"FusedMuon: unknown keyword {key!r}; accepted: lr, weight_decay, momentum, nesterov, "
                                 "ns_coefficients, eps, ns_steps, adjust_lr_fn, adamw_lr, adamw_betas, adamw_eps, "
                                 f"adamw_weight_decay and (off only) {list(self.OFF_ONLY)}")
            if not any(value is off for off in self.OFF_ONLY[key]):
                raise ValueError(f"FusedMuon: {key}={value!r} is not supported; only {key}={self.OFF_ONLY[key][0]!r} is")
        if isinstance(ns_steps, bool) or not isinstance(ns_steps, int) or not 1 <= ns_steps <= 99:
            raise ValueError(f"FusedMuon: ns_steps={ns_steps!r}: an integer from 1 to 99 is expected")
        if adjust_lr_fn not in MUON_ADJUST_LR:
            raise ValueError(f"FusedMuon: adjust_lr_fn={adjust_lr_fn!r}: one of {list(MUON_ADJUST_LR)} is expected")
        if not isinstance(nesterov, bool):
            raise ValueError(f"FusedMuon: nesterov={nesterov!r}: True or False is expected")
        if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum <= 1.0:
            raise ValueError(f"FusedMuon: momentum={momentum!r}: a float from 0 to 1 is expected")
        try:
            coeffs = tuple(float(x) for x in ns_coefficients)
        except TypeError:
            coeffs = ()
        if len(coeffs) != 3 or not all(math.isfinite(x) for x in coeffs):
            raise ValueError(f"FusedMuon: ns_coefficients={ns_coefficients!r}: three finite floats are expected")
        if not (isinstance(eps, (int, float)) and eps > 0):
            raise ValueError(f"FusedMuon: eps={eps!r}: a positive float is expected")
        self.momentum, self.nesterov, self.ns_coefficients = float(momentum), nesterov, coeffs
        self.muon_eps, self.ns_steps, self.adjust_lr_fn = float(eps), ns_steps, adjust_lr_fn
        own = {"momentum": self.momentum, "nesterov": nesterov, "ns_steps": ns_steps, "ns_coefficients": coeffs,
               "adjust_lr_fn": adjust_lr_fn}
        rest_lr = lr if adamw_lr is None else adamw_lr
        rest_wd = weight_decay if adamw_weight_decay is None else adamw_weight_decay
        params = list(params)
        if any(isinstance(g, Mapping) for g in params) and not all(isinstance(g, Mapping) for g in params):
            raise ValueError("FusedMuon: params mixes parameters and group dicts; pass either an iterable of parameters or an "
                             "iterable of {'params': [...], ...} dicts")
        if not params or not isinstance(params[0], Mapping):
            stores = {id(getattr(p, "_sc_store", None)): getattr(p, "_sc_store", None) for p in params}
            if len(stores) != 1 or None in stores.values():
                raise ValueError("FusedMuon needs the parameters of exactly one SpatialClipNet (flat ParamStore)")
            if len(params) != len(next(iter(stores.values())).specs):
                raise ValueError("FusedMuon updates the whole flat buffer: pass all parameters (reference passes "
                                 "self.parameters() un-grouped)")
            params = [{"params": params}]
        groups, kinds = [], []
        for gi, g in enumerate(params):
            for key in self.MUON_GROUP_KEYS:
                if key in g:
                    value = tuple(float(x) for x in g[key]) if key == "ns_coefficients" else g[key]
                    if value != own[key]:
                        raise ValueError(f"FusedMuon: parameter group {gi} sets {key}={g[key]!r}; per-group {key} is not "
                                         f"supported (the optimiser's is {own[key]!r})")
            if "params" not in g:
                raise ValueError(f"FusedMuon: parameter group {gi} has no 'params'")
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            names = []
            for p in ps:
                st = getattr(p, "_sc_store", None)
                if st is None:
                    raise ValueError(f"FusedMuon: parameter group {gi} holds a tensor of shape {tuple(getattr(p, 'shape', ()))} "
                                     "that is no parameter of a SpatialClipNet (flat ParamStore)")
                names.append(_reference_name("", p))
            use = g.get("use_muon")
            if use is not None and not isinstance(use, bool):
                raise ValueError(f"FusedMuon: parameter group {gi} sets use_muon={use!r}: True or False is expected")
            if use is True:
                for n, p in zip(names, ps):
                    if not muon_shape_ok(tuple(p.shape)):
                        raise ValueError(f"FusedMuon: parameter group {gi} sets use_muon=True for {n} of shape {tuple(p.shape)}; "
                                         "Muon takes 2-D tensors whose two dimensions are multiples of 8")
            pick = [use if use is not None else (is_muon_name(n) and muon_shape_ok(tuple(p.shape))) for n, p in zip(names, ps)]
            base = {k: v for k, v in g.items() if k not in ("params", "param_names", "use_muon") + self.MUON_GROUP_KEYS}
            for kind in (True, False):
                part = [(n, p) for n, p, k in zip(names, ps, pick) if k is kind]
                if not part and (ps or kind):       # an input group without parameters goes through once, to the base's refusal
                    continue
                new = dict(base)
                new["params"], new["param_names"] = [p for _, p in part], [n for n, _ in part]
                new.setdefault("lr", lr if kind else rest_lr)
                new.setdefault("weight_decay", weight_decay if kind else rest_wd)
                groups.append(new)
                kinds.append(kind)
        super().__init__(groups, lr, adamw_betas, adamw_eps, weight_decay)
        for g, kind in zip(self.param_groups, kinds):
            g["use_muon"] = kind
        self._build_tables()

    def _build_tables(self) -> None:
        """The per-slot and per-tensor tables and the scratch buffers, over the trainable Muon tensors only: a locked matrix is
        no tensor, gets no momentum and no Newton-Schulz iteration."""
        st = self.store
        dev = st.device
        n_slots = st.total // 64
        if self.chunk_group is None:        # one group: the same tables and staging ring as with many (_init_groups)
            self.chunk_group = slot_table(st, [self.param_groups[0]["param_names"]]).to(dev)
            self._alloc_group_hyper(1)
        trainable = set(st.trainable_names())
        names = sorted((n for g in self.param_groups if g["use_muon"] for n in g["param_names"] if n in trainable),
                       key=lambda n: st.by_name[n].offset)
        self.muon_names = names
        slot_tensor = torch.full((n_slots,), -1, dtype=torch.int32)     # -1: an AdamW slot
        info = torch.zeros((max(len(names), 1), 4), dtype=torch.int32)
        ratio = torch.ones(max(len(names), 1), dtype=torch.float32)
        shapes: List[Tuple[int, int]] = []
        x_slot = 0
        for ti, n in enumerate(names):
            sp = st.by_name[n]
            lo, k = sp.offset // 64, sp.numel // 64
            slot_tensor[lo:lo + k] = ti
            info[ti, 0], info[ti, 1], info[ti, 2] = lo, lo + k, x_slot
            ratio[ti] = muon_adjust_ratio(self.adjust_lr_fn, sp.shape)
            shapes.append((int(sp.shape[0]), int(sp.shape[1])))
            x_slot += k
        self.compact_slots = x_slot
        self.muon_shapes = shapes                    # [r, c] of every Muon tensor, in buffer order
        self.slot_tensor_host, self.tensor_info_host = slot_tensor, info
        self.slot_tensor, self.tensor_info, self.ratio = slot_tensor.to(dev), info.to(dev), ratio.to(dev)
        bf = torch.bfloat16
        self.x0 = torch.zeros(max(64 * x_slot, 64), dtype=bf, device=dev)      # X ping
        self.x1 = torch.zeros(max(64 * x_slot, 64), dtype=bf, device=dev)      # bf16(U), then X pong
        mm = max([min(r, c) ** 2 for r, c in shapes] + [64])
        self.gbuf = torch.zeros(mm, dtype=bf, device=dev)                      # G and P of the matrix in flight
        self.pbuf = torch.zeros(mm, dtype=bf, device=dev)
        self.acc = torch.zeros(max([r * c for r, c in shapes] + [64]), dtype=torch.float32, device=dev)     # fp32 accumulators of a product
        self.slot_sums = torch.zeros(n_slots, dtype=torch.float32, device=dev)
        self.norms = torch.zeros(max(len(names), 1), dtype=torch.float32, device=dev)      # ||bf16(U)|| of the last step

    def _uses_table(self) -> bool:
        return True

    def _group_hyper_floats(self, n_groups: int) -> int:
        return 2 + 2 * n_groups

    def _fill_group_hyper(self, host: torch.Tensor) -> None:
        g0 = self.param_groups[0]
        ops.adamw_groups_hyper_host([g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups],
                                    g0["betas"][0], g0["betas"][1], self.step_count, host)

    def _obuf(self) -> torch.Tensor:
        return self.x1 if self.ns_steps & 1 else self.x0

    def _before_pieces(self, grad_scale, clip, table) -> None:
        n_mu = len(self.muon_names)
        if n_mu == 0:
            return
        st = self.store
        for k, (lo, hi) in enumerate(self.ranges):
            m, _ = self._moments(k, lo, hi)
            ops.muon_momentum(st.grad[lo:hi], m, hi - lo, self.slot_tensor[lo // 64:], self.tensor_info, n_mu, lo // 64,
                              self.momentum, self.nesterov, grad_scale, clip, self.x1, self.slot_sums[lo // 64:],
                              self.compact_slots)
        ops.muon_scale(self.slot_sums, st.total // 64, self.tensor_info, n_mu, self.muon_eps, self.x1, self.x0, self.norms,
                       self.compact_slots)
        for ti in range(n_mu):
            self._newton_schulz(ti)

    def _newton_schulz(self, ti: int) -> None:
        r, c = self.muon_shapes[ti]
        muon_newton_schulz(self.x0, self.x1, int(self.tensor_info_host[ti, 2]) * 64, r, c, self.gbuf, self.pbuf, self.acc,
                           self.ns_steps, self.ns_coefficients)

    def _update_groups(self, lo, hi, moments, grad_scale, clip, table) -> None:
        st, g = self.store, self.param_groups[0]
        m, v = moments
        ops.muon_apply(st.master[lo:hi], st.grad[lo:hi], m, v, hi - lo, self.chunk_group[lo // 64:], self.slot_tensor[lo // 64:],
                       self.tensor_info, self.ratio, len(self.muon_names), lo // 64, self._obuf(), table, len(self.param_groups),
                       g["betas"][0], g["betas"][1], g["eps"], grad_scale, clip, st.master_bf16[lo:hi], self.compact_slots)


def slot_table(store, group_names: Sequence[Sequence[str]]) -> torch.Tensor:
    """uint8 [store.total // 64] on the host: the group of every 64-float slot of the flat buffers.  A parameter starts on a
    slot boundary and shares no slot with another (params.ALIGN), so each of its slots -- the zero padding of its last one
    included -- carries its group; slots of no listed parameter (the padding behind the last parameter, locked parameters
    left out of every group) read 0: their gradients are zero or no launch covers them."""
    from .params import ALIGN
    if ALIGN != 64:
        raise ValueError(f"slot_table: the grouped AdamW kernel maps float4 i to slot i >> 4; params.ALIGN is {ALIGN}, not 64")
    if len(group_names) > FusedAdamW.MAX_GROUPS:
        raise ValueError(f"slot_table: {len(group_names)} groups; at most {FusedAdamW.MAX_GROUPS}")
    table = torch.zeros(store.total // ALIGN, dtype=torch.uint8)
    for gi, names in enumerate(group_names):
        for name in names:
            sp = store.by_name[name]
            lo = sp.offset // ALIGN
            table[lo:lo + (max(sp.numel, 1) + ALIGN - 1) // ALIGN] = gi
    return table


def _reference_name(name: str, p) -> str:
    """The state-dict name of ``p``: the ParamStore's, if ``p`` is one of a store's parameters (``net.named_parameters()``
    spells ``visual.proj`` as ``visual__proj``); otherwise the name given."""
    st = getattr(p, "_sc_store", None)
    if st is not None:
        for n, q in st.params.items():
            if q is p:
                return n
    return name


NO_DECAY_MARKERS = ("bn", "ln", "bias", "logit_scale")


def open_clip_param_groups(named_parameters, weight_decay: Optional[float] = None) -> List[Dict[str, Any]]:
    """The two groups open_clip trains with: gains, biases and scalars -- every tensor with fewer than two dimensions, and every
    tensor whose state-dict name contains ``bn``, ``ln``, ``bias`` or ``logit_scale`` -- get ``weight_decay = 0`` (first group);
    everything else gets ``weight_decay`` (second group; ``None`` leaves it to the optimiser's default).  ``named_parameters``:
    ``(name, tensor)`` pairs, e.g. ``net.named_parameters()``; names are looked up in the ParamStore.  An ``nn.Parameter`` with
    ``requires_grad=False`` (a locked tower) is left out, as open_clip leaves it out.  An empty group is dropped."""
    no_decay: Dict[str, list] = {"params": [], "weight_decay": 0.0, "param_names": []}
    decay: Dict[str, Any] = {"params": [], "param_names": []}
    if weight_decay is not None:
        decay["weight_decay"] = float(weight_decay)
    for name, p in named_parameters:
        if isinstance(p, torch.nn.Parameter) and not p.requires_grad:
            continue
        name = _reference_name(name, p)
        g = no_decay if p.ndim < 2 or any(mark in name for mark in NO_DECAY_MARKERS) else decay
        g["params"].append(p)
        g["param_names"].append(name)
    return [g for g in (no_decay, decay) if g["params"]]


def scaled_lr_groups(groups: Sequence[Mapping], lr: float, lr_scale: Mapping[str, float]) -> List[Dict[str, Any]]:
    """Split every group by the longest prefix in ``lr_scale`` that its parameters' state-dict names start with: the
    parameters under prefix ``q`` move to a group of their own with ``lr = base * lr_scale[q]`` (``base``: the group's own
    ``lr``, else ``lr``); the others stay as they were.  ``{"visual.": 0.1}`` trains the image tower at a tenth of ``lr``.
    The order of the groups and of the parameters inside them is kept; empty groups are dropped."""
    scales = check_lr_scale(lr_scale)
    prefixes = sorted(scales, key=len, reverse=True)
    out: List[Dict[str, Any]] = []
    for g in groups:
        ps = g["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        given = list(g.get("param_names", ()))
        if given and len(given) != len(ps):
            raise ValueError(f"scaled_lr_groups: a group lists {len(ps)} parameters and {len(given)} param_names")
        names = [_reference_name(given[i] if given else "", p) for i, p in enumerate(ps)]
        parts: Dict[Optional[str], Tuple[list, list]] = {}
        for name, p in zip(names, ps):
            key = next((q for q in prefixes if name.startswith(q)), None)
            part = parts.setdefault(key, ([], []))
            part[0].append(p)
            part[1].append(name)
        for key in [None] + [q for q in scales if q in parts]:
            if key not in parts:
                continue
            new = {k: v for k, v in g.items() if k not in ("params", "param_names", "initial_lr")}
            new["params"], new["param_names"] = parts[key]
            if key is not None:
                new["lr"] = float(g.get("lr", lr)) * scales[key]
            out.append(new)
    return out


def check_lr_scale(lr_scale) -> Dict[str, float]:
    """``{name prefix: positive factor}`` or ValueError naming the offending entry."""
    if not isinstance(lr_scale, Mapping):
        raise ValueError(f"lr_scale={lr_scale!r}: a mapping {{name prefix: factor}} is expected")
    out = {}
    for prefix, factor in lr_scale.items():
        ok = isinstance(factor, (int, float)) and not isinstance(factor, bool) and math.isfinite(factor) and factor > 0
        if not isinstance(prefix, str) or not prefix or not ok:
            raise ValueError(f"lr_scale[{prefix!r}]={factor!r}: a non-empty name prefix and a positive, finite factor are "
                             "expected")
        out[prefix] = float(factor)
    return out


PARAM_GROUPS_KEYS = ("no_decay", "lr_scale")


def check_param_groups_cfg(cfg):
    """``SpatialClipLitModule(param_groups=...)`` / the config key ``model.param_groups``: None, a callable ``(net) -> list of
    group dicts``, or a mapping ``{"no_decay": "open_clip" | None, "lr_scale": {prefix: factor}}``.  Returns it (a mapping as a
    plain dict); ValueError names an unknown key, another ``no_decay`` rule or a bad scale."""
    if cfg is None or callable(cfg):
        return cfg
    if not isinstance(cfg, Mapping):
        raise ValueError(f"param_groups={cfg!r}: None, a callable (net) -> groups, or a mapping with the keys "
                         f"{list(PARAM_GROUPS_KEYS)} is expected")
    unknown = [k for k in cfg if k not in PARAM_GROUPS_KEYS]
    if unknown:
        raise ValueError(f"param_groups: unknown key(s) {unknown}; accepted: {list(PARAM_GROUPS_KEYS)}")
    no_decay = cfg.get("no_decay")
    if no_decay not in (None, "open_clip"):
        raise ValueError(f"param_groups.no_decay={no_decay!r}: 'open_clip' (gains, biases and scalars without weight decay) or "
                         "null")
    scales = cfg.get("lr_scale")
    return {"no_decay": no_decay, "lr_scale": check_lr_scale(scales) if scales is not None else None}


def build_param_groups(net, cfg, lr: float, weight_decay: Optional[float] = None) -> List[Dict[str, Any]]:
    """The group dicts of ``check_param_groups_cfg``'s mapping for ``net``, over its trainable parameters."""
    store = net.store
    named = [(n, p) for n, p in store.params.items() if p.requires_grad]
    if cfg.get("no_decay") == "open_clip":
        groups = open_clip_param_groups(named, weight_decay)
    else:
        groups = [{"params": [p for _, p in named], "param_names": [n for n, _ in named]}]
    if cfg.get("lr_scale"):
        groups = scaled_lr_groups(groups, lr, cfg["lr_scale"])
    return groups


WEIGHT_AVERAGING_KINDS = ("ema", "mean")
WEIGHT_AVERAGING_KEYS = ("decay", "update_every_n_steps", "update_starting_at_step", "update_starting_at_epoch", "device", "kind")


def validate_weight_averaging(decay=0.999, update_every_n_steps=1, update_starting_at_step=None, update_starting_at_epoch=None,
                              device=None, kind="ema") -> Dict[str, Any]:
    """The arguments of ``lightning.pytorch.callbacks.EMAWeightAveraging`` as this build takes them, plus ``kind`` ("ema", or
    "mean": ``AveragedModel``'s default equal average).  Returns the arguments of ``WeightAverager``; ValueError names the
    argument that is refused."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if kind not in WEIGHT_AVERAGING_KINDS:
        raise ValueError(f"weight_averaging: kind={kind!r}: one of {list(WEIGHT_AVERAGING_KINDS)} is expected")
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
        raise ValueError(f"weight_averaging: decay={decay!r}: a number in [0, 1] is expected")
    if not is_int(update_every_n_steps) or update_every_n_steps < 1:
        raise ValueError(f"weight_averaging: update_every_n_steps={update_every_n_steps!r}: an integer >= 1 is expected")
    if update_starting_at_step is not None and (not is_int(update_starting_at_step) or update_starting_at_step < 0):
        raise ValueError(f"weight_averaging: update_starting_at_step={update_starting_at_step!r}: None or an integer >= 0 is "
                         "expected")
    if update_starting_at_epoch is not None:
        raise ValueError(f"weight_averaging: update_starting_at_epoch={update_starting_at_epoch!r} is not supported (updates "
                         "are scheduled by optimiser step: update_starting_at_step); only None is accepted")
    if device is not None:
        raise ValueError(f"weight_averaging: device={device!r} is not supported (the average lives beside the master weights, "
                         "on their device); only None is accepted")
    return {"decay": float(decay), "update_every_n_steps": int(update_every_n_steps),
            "update_starting_at_step": update_starting_at_step, "kind": kind}


def check_weight_averaging_cfg(cfg) -> Optional[Dict[str, Any]]:
    """``Trainer(callbacks={"weight_averaging": {...}})``: None (absent) or a mapping of ``validate_weight_averaging``'s
    arguments."""
    if cfg is None:
        return None
    if not isinstance(cfg, Mapping):
        raise ValueError(f"callbacks.weight_averaging={cfg!r}: a mapping with the keys {list(WEIGHT_AVERAGING_KEYS)} is expected")
    unknown = [k for k in cfg if k not in WEIGHT_AVERAGING_KEYS]
    if unknown:
        raise ValueError(f"callbacks.weight_averaging: unknown key(s) {unknown}; accepted: {list(WEIGHT_AVERAGING_KEYS)}")
    return validate_weight_averaging(**dict(cfg))


class WeightAverager:
    """An averaged copy of the weights (``lightning.pytorch.callbacks.EMAWeightAveraging`` / ``WeightAveraging`` over
    ``torch.optim.swa_utils.AveragedModel``) for a net that has no ``nn.Module`` to copy: ``avg`` is a flat fp32 buffer in the
    layout of ``store.master`` (4 more bytes per parameter) and one streaming kernel (``ops.weight_average``, 12 bytes per
    parameter) updates it right behind the optimiser's update of every range or bucket, on the optimiser's stream.

    After optimiser step ``s`` (0-based) an update happens iff ``s >= (update_starting_at_step or 0)`` and
    ``s % update_every_n_steps == 0``; the first one copies the weights, every later one is ``decay * avg + (1 - decay) * p``
    (``kind="ema"``) or ``avg + (p - avg) / (n_averaged + 1)`` (``kind="mean"``), with torch's CPU bits.  The trainable ranges are
    averaged; locked ranges of ``avg`` are a copy of the masters made once.  The graph-captured step launches the form that
    reads {op, a, b} from the device block ``ctl``, which ``refresh_ctl`` rewrites in front of every replay."""

    def __init__(self, store, decay: float = 0.999, update_every_n_steps: int = 1, update_starting_at_step: Optional[int] = None,
                 kind: str = "ema", update_starting_at_epoch=None, device=None):
        args = validate_weight_averaging(decay, update_every_n_steps, update_starting_at_step, update_starting_at_epoch, device,
                                         kind)
        if getattr(store, "fp8", False):
            raise ValueError("weight_averaging with precision='fp8' is not supported: the delayed e4m3 activation scales "
                             "belong to the training weights, not to their average; use precision='bf16-mixed'")
        self.store = store
        self.decay, self.every, self.kind = args["decay"], args["update_every_n_steps"], args["kind"]
        self.update_starting_at_step = args["update_starting_at_step"]
        self.n_averaged = 0
        self.latest_update_step = -1            # the optimiser step (0-based) of the last update; -1: none yet
        self._decided: Optional[Tuple[int, int, float, float]] = None      # (step, op, a, b) of the step last decided
        store.wait_all()
        self.avg = store.master.clone()
        self.ranges: List[Tuple[int, int]] = list(store.trainable_ranges())
        self.ctl: Optional[torch.Tensor] = None        # device {int32 op, fp32 a, fp32 b, pad}: what the captured launches read
        self._ctl_stage: list = []                      # pinned staging ring of the same: [host tensor, event of its copy]
        self._ctl_next = 0

    # ---- the schedule
    def should_update(self, step: int) -> bool:
        return step >= (self.update_starting_at_step or 0) and step % self.every == 0

    def _decide(self, step: int) -> Tuple[int, float, float]:
        """(op, a, b) of the update behind optimiser step ``step`` (0-based); counts it.  Asked again for the same step (the
        capture of a graph refreshes the block of the step that then replays) it answers the same and counts nothing."""
        step = int(step)
        if self._decided is not None and self._decided[0] == step:
            return self._decided[1:]
        if not self.should_update(step):
            out = (ops.WAVG_SKIP, 0.0, 0.0)
        else:
            if self.n_averaged == 0:
                out = (ops.WAVG_COPY, 0.0, 0.0)
            elif self.kind == "ema":
                out = (ops.WAVG_EMA, self.decay, 1.0 - self.decay)      # 1 - decay in double; rounded to fp32 once, at the launch
            else:
                out = (ops.WAVG_MEAN, float(self.n_averaged + 1), 0.0)
            self.n_averaged += 1
            self.latest_update_step = step
        self._decided = (step,) + out
        return out

    def attach(self, optimizer) -> "WeightAverager":
        """Make ``optimizer`` (a ``_FlatOptimizer`` over the same store) call this averager behind every piece of its update.
        Call after ``optimizer.attach_exchange`` and before a checkpoint is loaded."""
        if getattr(optimizer, "store", None) is not self.store:
            raise ValueError("WeightAverager.attach: the optimiser updates another ParamStore")
        if getattr(optimizer, "exchange", None) is not None:
            raise ValueError("weight_averaging with the sharded gradient exchange (SC_GRAD_EXCHANGE=sharded) is not supported: "
                             "a rank updates 1/W of every bucket and gathers the rest behind the next forward; use the "
                             "all-reduce exchange")
        self.ranges = list(optimizer.ranges)
        optimizer.averager = self
        return self

    # ---- the launches, called by the optimiser
    def begin_step(self, step: int) -> None:
        """The eager step forms: decide the update of optimiser step ``step`` before its pieces run."""
        self._decide(step)

    def after_piece(self, lo: int, hi: int) -> None:
        """Behind the optimiser's update of flat[lo:hi] (a trainable range or a bucket of one), on the current stream."""
        op, a, b = self._decided[1:]
        if op != ops.WAVG_SKIP:
            ops.weight_average(self.avg[lo:hi], self.store.master[lo:hi], hi - lo, op, a, b)

    def after_piece_captured(self, lo: int, hi: int) -> None:
        """The same inside a graph capture: {op, a, b} are read from ``ctl`` by every replay."""
        ops.weight_average_dev(self.avg[lo:hi], self.store.master[lo:hi], hi - lo, self._ctl())

    def _ctl(self) -> torch.Tensor:
        if self.ctl is None:
            dev = self.store.device
            cuda = torch.device(dev).type == "cuda"
            self.ctl = torch.zeros(4, dtype=torch.int32, device=dev)
            for _ in range(4):
                host = torch.zeros(4, dtype=torch.int32)
                self._ctl_stage.append([host.pin_memory() if cuda else host, None])
        return self.ctl

    def refresh_ctl(self, step: int) -> None:
        """Write {op, a, b} of optimiser step ``step`` into ``ctl``: one 16-byte async copy on the current stream, in front of
        the replay that reads it.  The pinned staging is a ring of four, each with the event of its last copy (as the
        optimiser's group table, ``_refresh_group_hyper``): a host running ahead of the device never rewrites a block that a
        pending copy still has to read."""
        import struct
        op, a, b = self._decide(step)
        ctl = self._ctl()
        slot = self._ctl_stage[self._ctl_next]
        self._ctl_next = (self._ctl_next + 1) % len(self._ctl_stage)
        if slot[1] is not None:
            slot[1].synchronize()
        bits = struct.unpack("<2i", struct.pack("<2f", a, b))      # rounded to fp32 as the host-scalar launch rounds them
        slot[0][0], slot[0][1], slot[0][2] = int(op), bits[0], bits[1]
        ctl.copy_(slot[0], non_blocking=True)
        if ctl.is_cuda:
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(ctl.device))

    # ---- validation and the end of training
    def swap(self) -> None:
        """Exchange masters and average in place and refresh every compute copy."""
        st = self.store
        st.wait_all()
        ops.swap_f32(st.master, self.avg, st.total)
        self._refresh_copies()

    def _refresh_copies(self) -> None:
        if self.store.master.is_cuda:       # (a host-side store -- tests of the layout -- has no compute copies to refresh)
            self.store.refresh_compute_copies()

    def applied(self):
        """Context manager: the net computes with the averaged weights inside (masters and average exchanged in place, compute
        copies refreshed) and with the training weights, bit for bit, afterwards."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            self.swap()
            try:
                yield self
            finally:
                self.swap()
        return ctx()

    def copy_to_model(self) -> None:
        """The end of training (Lightning's ``on_train_end``): the model holds the average.  The training weights stay in
        checkpoints written before (``current_model_state``)."""
        st = self.store
        st.wait_all()
        st.master.copy_(self.avg)
        self._refresh_copies()

    def reset_from_model(self) -> None:
        """Start over from the model's weights (a checkpoint without an average was loaded): ``n_averaged = 0``."""
        self.store.wait_all()
        self.avg.copy_(self.store.master)
        self.n_averaged, self.latest_update_step, self._decided = 0, -1, None

    # ---- checkpoints
    def _named(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {s.name: flat[s.offset:s.offset + s.numel].view(s.shape).detach().clone() for s in self.store.specs}

    def averaged_state_dict(self) -> Dict[str, torch.Tensor]:
        """The average under the names of ``net.state_dict()``; the model's weights while nothing has been averaged."""
        self.store.wait_all()
        return self._named(self.avg if self.n_averaged > 0 else self.store.master)

    def state_dict(self) -> Dict[str, Any]:
        """The ``"weight_averaging"`` entry of a checkpoint, whose ``"state_dict"`` carries ``averaged_state_dict()``."""
        self.store.wait_all()
        return {"current_model_state": self._named(self.store.master), "n_averaged": int(self.n_averaged),
                "latest_update_step": int(self.latest_update_step), "kind": self.kind, "decay": float(self.decay)}

    def load_state_dict(self, sd: Mapping, averaged: Optional[Mapping] = None) -> None:
        """``sd``: a checkpoint's ``"weight_averaging"`` entry; ``averaged``: its ``"state_dict"`` (None: the masters hold it, as
        after ``net.load_checkpoint_state_dict``).  The average takes ``averaged``, the masters ``current_model_state``."""
        missing = [k for k in ("current_model_state", "n_averaged", "latest_update_step", "kind", "decay") if k not in sd]
        if missing:
            raise ValueError(f"WeightAverager.load_state_dict: the entry lacks {missing}")
        if sd["kind"] != self.kind:
            raise ValueError(f"WeightAverager.load_state_dict: the file's average is of kind {sd['kind']!r}, this averager's "
                             f"kind={self.kind!r}")
        st = self.store
        st.wait_all()
        if averaged is None:
            self.avg.copy_(st.master)
        else:
            for s in st.specs:
                self.avg[s.offset:s.offset + s.numel].view(s.shape).copy_(averaged[s.name].to(self.avg.device, torch.float32))
        current = sd["current_model_state"]
        lacking = [s.name for s in st.specs if s.name not in current]
        if lacking:
            raise ValueError(f"WeightAverager.load_state_dict: current_model_state lacks {lacking[:5]} ({len(lacking)} in all)")
        with torch.no_grad():
            for s in st.specs:
                st.master[s.offset:s.offset + s.numel].view(s.shape).copy_(current[s.name].to(st.master.device, torch.float32))
        self._refresh_copies()
        self.n_averaged, self.latest_update_step = int(sd["n_averaged"]), int(sd["latest_update_step"])
        self._decided = None


class GradAccumulator:
    """The running gradient sum of ``Trainer(accumulate_grad_batches=every)``.  Every backward overwrites the flat gradient
    buffer of the ``ParamStore``, so the sum of a group's micro-batches lives in a second flat fp32 buffer ``acc`` beside it and
    one streaming kernel (``ops.grad_accumulate``, 12 bytes per parameter) folds each micro-batch in with weight ``1/every``:
    the first of a group starts the sum, the last leaves ``sum + its own share`` in ``store.grad`` -- where the reducer, the
    clip and AdamW expect the gradient -- and does not write ``acc``.  ``acc`` is allocated on first use and only when
    ``every > 1``; no producer kernel learns an accumulate mode.  ``scale`` replaces the weight ``1/every``: the cached-feature
    form (``Trainer(accum_freq=N)``) folds at 1."""

    def __init__(self, store, every: int, scale: Optional[float] = None):
        every = validate_accumulate_grad_batches(every)
        self.store, self.every = store, every
        # ``scale=1.0``: the cached-feature form (Trainer accum_freq): each micro-batch's gradient is already its share of the
        # group loss, a mean over all N * B pairs
        self.scale = 1.0 / every if scale is None else float(scale)
        self.acc: Optional[torch.Tensor] = None
        self.partial: Optional[torch.Tensor] = None     # 1024 fp64 sums of squares of the summed gradient (sumsq_partial())
        self._folded: List[Tuple[int, int]] = []        # ranges folded since the last hook() (sorted, disjoint)

    def _acc(self) -> torch.Tensor:
        if self.acc is None:
            self.acc = torch.zeros(self.store.total, dtype=torch.float32, device=self.store.grad.device)
        return self.acc

    def _ranges(self) -> List[Tuple[int, int]]:
        """The trainable ranges of the flat buffer (locked towers: nothing else is ever folded; the locked part of
        ``store.grad`` holds zeros that no backward writes)."""
        f = getattr(self.store, "trainable_ranges", None)
        return list(f()) if f is not None else [(0, self.store.total)]

    def sumsq_partial(self) -> torch.Tensor:
        """The fp64 buffer (1024 slots per trainable range: 1024 without a lock) to pass as ``fold(..., partial=)`` and then
        as ``FusedAdamW.step(sumsq_partial=)``."""
        n = 1024 * len(self._ranges())
        if self.partial is None or self.partial.numel() != n:
            self.partial = torch.zeros(n, dtype=torch.float64, device=self.store.grad.device)
        return self.partial

    def fold(self, first: bool, last: bool, lo: int = 0, hi: Optional[int] = None, partial: Optional[torch.Tensor] = None) -> None:
        """Fold ``store.grad[lo:hi]`` of the micro-batch that has just run its backward, on the current stream.  ``first`` /
        ``last``: its place in the group (both: a group of one, the gradient is only scaled).  ``partial``: whole-buffer folds of
        a last micro-batch may leave the sums of squares for the clip in it."""
        hi = self.store.total if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo <= hi <= self.store.total:
            raise ValueError(f"GradAccumulator.fold: range [{lo}, {hi}) outside the flat buffer of {self.store.total} floats")
        if partial is not None and (not last or lo != 0 or hi != self.store.total):
            raise ValueError("GradAccumulator.fold: partial= needs the whole buffer of a group's last micro-batch")
        if hi == lo:
            return
        ranges = self._ranges()
        if ranges != [(0, self.store.total)]:      # locked towers: the pieces of [lo, hi) that hold trainable gradients
            from .lock import intersect
            if partial is not None and partial.numel() != 1024 * len(ranges):
                raise ValueError("GradAccumulator.fold: partial= must come from sumsq_partial() (1024 slots per trainable range)")
            for k, (a, b) in enumerate(ranges):
                for x, y in intersect([(a, b)], lo, hi):
                    self._fold_piece(first, last, x, y, None if partial is None else partial[1024 * k:1024 * (k + 1)])
            return
        self._fold_piece(first, last, lo, hi, partial)

    def _fold_piece(self, first: bool, last: bool, lo: int, hi: int, partial: Optional[torch.Tensor]) -> None:
        g = self.store.grad
        if last:
            acc = None if first else self._acc()[lo:hi]
            ops.grad_accumulate(acc, g[lo:hi], hi - lo, self.scale, 2, partial)
        else:
            ops.grad_accumulate(self._acc()[lo:hi], g[lo:hi], hi - lo, self.scale, 0 if first else 1)

    def _fold_new(self, first: bool, last: bool, lo: int, hi: int) -> None:
        """Fold what of [lo, hi) this micro-batch has not folded yet (announced ranges may touch or overlap)."""
        pos, out = lo, []
        for a, b in self._folded:
            if b <= pos or a >= hi:
                continue
            if a > pos:
                out.append((pos, a))
            pos = max(pos, b)
        if pos < hi:
            out.append((pos, hi))
        for a, b in out:
            self.fold(first, last, a, b)
        merged: List[Tuple[int, int]] = []
        for a, b in sorted(self._folded + out):
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        self._folded = merged

    def hook(self, first: bool, last: bool, inner: Optional[Callable[[int, int], None]] = None) -> Callable[[int, int], None]:
        """The ``net.grad_bucket_hook`` of ONE micro-batch: folds each announced range as soon as backward has completed it (on
        the stream that announces it) and, on a group's last micro-batch only, hands the range on to ``inner``
        (``reducer.bucket_ready``): the other micro-batches issue no gradient collective (Lightning's ``no_sync``).  Follow the
        backward with ``fold_rest`` -- before ``reducer.finish()`` -- for what no call announced."""
        self._folded = []

        def on_range(lo: int, hi: int) -> None:
            self._fold_new(first, last, int(lo), int(hi))
            if last and inner is not None:
                inner(lo, hi)
        return on_range

    def fold_rest(self, first: bool, last: bool) -> None:
        """Fold every range of the buffer that the hook of this micro-batch was not called for (``reducer.finish()`` reduces
        that complement in one go: it has to hold the sum by then)."""
        self._fold_new(first, last, 0, self.store.total)


def validate_accumulate_grad_batches(value) -> int:
    """``accumulate_grad_batches`` as this build takes it: an integer >= 1 (1: no accumulation).  Lightning also accepts a
    ``{epoch: N}`` dict through its GradientAccumulationScheduler callback; that form is refused, like every other value."""
    ok = isinstance(value, int) and not isinstance(value, bool) and value >= 1
    if not ok:
        raise ValueError(f"accumulate_grad_batches={value!r}: an integer >= 1 is accepted (1 = an optimiser step after every "
                         "batch); a per-epoch dict schedule (GradientAccumulationScheduler), 0, negative or fractional "
                         "values are not")
    return int(value)


def cosine_warmup_lambda(step: int, num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.5) -> float:
    if step < num_warmup_steps:
        return float(step) / float(max(1, num_warmup_steps))
    progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))


class LambdaLR:
    """torch.optim.lr_scheduler.LambdaLR semantics: lr = initial_lr * f(number of scheduler steps so far)."""

    def __init__(self, optimizer, lr_lambda):
        self.optimizer, self.lr_lambda = optimizer, lr_lambda
        self.last_epoch = 0
        self._apply()

    def _apply(self) -> None:
        for g in self.optimizer.param_groups:
            g["lr"] = g["initial_lr"] * self.lr_lambda(self.last_epoch)

    def step(self) -> None:
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]


def get_cosine_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int,
                                    num_cycles: float = 0.5, last_epoch: int = -1) -> LambdaLR:
    return LambdaLR(optimizer, lambda s: cosine_warmup_lambda(s, num_warmup_steps, num_training_steps, num_cycles))
