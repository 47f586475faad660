"""The transformer stack of a tower (``TransformerStack``) and the parts it is built from, one concern each: ``SideScheduler``
(which stream a launch goes to, the event edges between the two), ``OverlapTrial`` (SC_OVERLAP=auto), ``Fp8Scales`` (the delayed-
scaling table and its slot layout), ``StackPass`` (what a forward hands to its backward), ``GradRing`` (the rotating residual-
gradient buffers), ``wgrad_plan`` / ``launch_wgrads`` (how weight gradients are launched).  Importing it needs no device."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch

from . import ops
from .params import ParamStore

BF16 = torch.bfloat16
F32 = torch.float32


def _splitk_for(m_out: int, n_out: int, k: int) -> int:
    """Split-K factor for a weight-gradient GEMM: ~one 256x256 workgroup per CU (256 CUs)."""
    tiles = ((m_out + 255) // 256) * ((n_out + 255) // 256)
    ktiles = (k + 63) // 64
    want = max(1, min((256 + tiles // 2) // max(tiles, 1), ktiles // 4))
    return max(1, min(want, 32))


def _splitk_for_group(shapes, k: int, one_round: bool = False) -> int:
    """Common split-K factor of a grouped weight-gradient launch: the smallest one that fills >= 95 % of whole rounds of
    256 workgroups (256 CUs, one 256x256 tile each); ``one_round``: the largest one that stays within ONE round (the
    weight gradients run beside the data-gradient chain: a launch of several rounds holds the chain's kernels back)."""
    tiles = sum(((m + 255) // 256) * ((n + 255) // 256) for m, n in shapes)
    ktiles = (k + 63) // 64
    best = 1
    for s in range(1, max(1, min(32, ktiles // 4)) + 1):
        wg = tiles * s
        if wg <= 256:
            best = s
        if not one_round and wg / (-(-wg // 256) * 256) >= 0.95:
            return s
    return best


MAX_SIDE_KTILES = 200       # longest K chain (64-token tiles) a grouped weight-gradient workgroup may own


def wgrad_plan(mode: str, branch: str, shapes, k: int):
    """How the weight gradients ``shapes`` = [(m, n), ...] of one branch, summed over ``k`` tokens, are launched:
    ("group", split-K) = one grouped launch, or ("each", [split-K per problem]) = one launch per Linear.  ``mode`` is
    SC_WGRAD_GROUP, read at every backward: auto (default), 0 (one launch per Linear, rounds 1-3), 1 (attention branch
    grouped), 2 / 3 (both branches grouped, whole rounds / one round), 4 (all four of a block in one launch: ``branch`` =
    "block") -- A/B switch.  ``auto`` groups a branch's pair when the grouped launch fits ONE round of workgroups with K chains
    of at most MAX_SIDE_KTILES tiles: the weight gradients run beside the data-gradient chain, and long-lived or multi-round
    side launches hold the chain's kernels back.  Same-box A/B (profiles/r04_wgrad_group_ab.txt): ViT-B/16 -0.06 ... -0.16 ms
    per step with the attention branch grouped (113-tile chains); the MLP pair at one round (263-tile chains) -0.04 more on one
    box; ViT-L/14 (257- / 514-tile chains) +2.4 ms bf16, +3.9 ms e4m3 with both grouped, +1.3 ms e4m3 with the attention branch
    alone -- hence the cap.  ``branch`` = "cls": the class-token block's K = batch launches, never grouped, never split."""
    if branch == "block":
        return "group", _splitk_for_group(shapes, k)
    if branch == "cls":
        return "each", [1] * len(shapes)
    if mode == "auto":
        s = _splitk_for_group(shapes, k, one_round=True)
        group = ((k + 63) // 64 + s - 1) // s <= MAX_SIDE_KTILES
    else:
        group = mode in ("2", "3") or (mode == "1" and branch == "attn")
    if group:
        return "group", _splitk_for_group(shapes, k, one_round=mode != "2")
    return "each", [_splitk_for(m, n, k) for m, n in shapes]


def launch_wgrads(probs, K: int, branch: str, mode: str, fp8=None) -> None:
    """The weight-gradient launches of ``probs`` = [(dy, x, dw, dbias or None, m, n), ...] (dw[m, n] = dy^T . x over K tokens,
    dbias = column sums of dy): the e4m3 kernel per problem when ``fp8`` = [(dy8, dy_scale_inv, x8, x_scale_inv), ...] gives
    per-tensor e4m3 operands, else what ``wgrad_plan`` says."""
    if fp8 is not None:
        for (_, _, dw, db, m, n), (dy8, dys, x8, xs) in zip(probs, fp8):
            ops.gemm_wgrad_fp8(dy8, dys, x8, xs, dw, db, M=m, N=n, K=K, splitk=_splitk_for(m, n, K))
        return
    kind, sk = wgrad_plan(mode, branch, [(p[4], p[5]) for p in probs], K)
    if kind == "group":
        ops.gemm_wgrad_group(probs, K=K, splitk=sk)
        return
    for (dy, x, dw, db, m, n), s in zip(probs, sk):
        if db is None:
            ops.gemm(ops.TN, ops.EPI_F32, dy, x, dw, M=m, N=n, K=K, splitk=s)
        else:
            ops.gemm_wgrad_bias(dy, x, dw, db, M=m, N=n, K=K, splitk=s)


def _res_stream_bf16(configured: str = "bf16") -> bool:
    """Read at every forward: the residual stream of the patch towers in bf16 (default: the reference's precision under its
    bf16 autocast) or fp32 -- SpatialClipNet(residual_stream=...), overridden by SC_RES_STREAM=bf16|fp32 for A/B."""
    return os.environ.get("SC_RES_STREAM", configured) == "bf16"


def _res_grad_bf16() -> bool:
    """Read at every backward: SC_RES_GRAD=fp32 restores the fp32 residual-gradient buffer (A/B, tests)."""
    return os.environ.get("SC_RES_GRAD", "bf16") != "fp32"


class _Bufs:
    """Named device buffers, (re)allocated when the requested shape changes.  ``suffix`` is appended to every name asked for
    while it is set: a pass of another token count (the FLIP patch-dropout training forward / backward beside full-length
    evaluation) gets buffers of its own instead of reallocating the other pass's at every switch; ``shared=True`` opts a
    buffer out (its shape does not depend on the token count)."""

    def __init__(self, device):
        self.device = device
        self.suffix = ""
        self._b: Dict[str, torch.Tensor] = {}

    def get(self, name: str, shape, dtype, shared: bool = False) -> torch.Tensor:
        if self.suffix and not shared:
            name = name + self.suffix
        t = self._b.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._b[name] = t
        return t

    def bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._b.values())


class SideScheduler:
    """Where the launches of one backward call go.  The data-gradient chain stays on ``main``; work that only feeds the
    optimiser (weight gradients, bias column sums, the LayerNorm column reductions, the bucket callbacks) goes through
    ``run``: on ``side`` behind everything enqueued on main so far (one fresh event per run), or in place when ``overlap`` is
    off.  Buffers a side launch reads are remembered with that run's "done" event; the chain calls ``before_write`` on a
    buffer before it reuses it."""

    def __init__(self, overlap: bool, main, side, ln_ws=None):
        self.overlap, self.main, self.side = overlap, main, side
        self._last_read = {}                     # buffer address -> event recorded on the side stream
        self._ln_ws, self._ln_pos = ln_ws, 0     # four rotating LayerNorm-backward workspaces (overlap only)

    def run(self, fn, reads=()) -> None:
        if not self.overlap:
            fn()
            return
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            fn()
            done = torch.cuda.Event()
            done.record(self.side)
        for t in reads:
            self._last_read[t.data_ptr()] = done

    def before_write(self, t: torch.Tensor) -> None:
        ev = self._last_read.pop(t.data_ptr(), None)
        if ev is not None:
            self.main.wait_event(ev)

    def ln_workspace(self) -> torch.Tensor:
        ws = self._ln_ws[self._ln_pos % 4]
        self._ln_pos += 1
        self.before_write(ws)
        return ws

    def join(self) -> None:
        if self.overlap:
            ev = torch.cuda.Event()
            ev.record(self.side)
            self.main.wait_event(ev)


class OverlapTrial:
    """SC_OVERLAP=auto for one batch shape of one stack: the stack's own backward is timed on both schedules (``warm`` untimed
    calls, then ``per`` timed calls each, alternating) and the faster one is kept."""
    __slots__ = ("calls", "ms", "pending", "choice", "ms_best")

    def __init__(self):
        self.calls = 0
        self.ms = {True: [], False: []}           # side stream on / off -> backward times of the finished trials
        self.pending: List[tuple] = []            # (side stream?, start event, end event) of trials still in flight
        self.choice: Optional[bool] = None
        self.ms_best: Optional[Dict[str, float]] = None

    def _collect(self, wait: bool) -> None:
        for rec in list(self.pending):
            if wait:
                rec[2].synchronize()
            if wait or rec[2].query():
                self.ms[rec[0]].append(rec[1].elapsed_time(rec[2]))
                self.pending.remove(rec)

    def next(self, main, warm: int, per: int, margin: float):
        """(use the side stream?, trial record or None) for the backward call about to run."""
        if self.choice is not None:
            return self.choice, None
        self._collect(wait=False)                 # trials whose end event has passed (normally a whole step ago)
        c = self.calls
        self.calls += 1
        if c < warm:
            return True, None
        if c >= warm + 2 * per:
            self._collect(wait=True)              # decision time: wait for the last trial if it is still in flight
            on, off = self.ms[True], self.ms[False]
            # The side stream is the schedule of rounds 1-3 and the safe one for the big models; leave it only when one stream is
            # faster by a clear margin (the two are within 1 % on ViT-B/16 and the trial timings carry that much noise: without
            # a margin the choice, and with it the step time, varies from run to run -- advisor, round 4).  All ranks take rank
            # 0's decision: the trials of a rank include its collective waits, and ranks on different schedules would only
            # wait for each other.
            choice = True
            if on and off:
                choice = not (min(off) < min(on) * (1.0 - margin))
                self.ms_best = {"side_stream": round(min(on), 3), "one_stream": round(min(off), 3)}
            from . import comm
            self.choice = comm.broadcast_flag(choice)
            return self.choice, None
        use = ((c - warm) % 2) == 0               # on, off, on, off, ...
        rec = (use, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        rec[1].record(main)
        self.pending.append(rec)
        return use, rec


class Fp8Scales:
    """fp8 delayed scaling: per-tensor scales taken from the maxima of the previous ``HISTORY`` steps, four tensors per block.
    A slot is ``(scale[k:k+1], scale_inv[k:k+1], amax[k])``; for ``L`` blocks, ``h(i)`` = GELU output of block i (k = 2 i; A of
    the c_proj forward), ``dU(i)`` = its gradient (2 i + 1; A of the c_fc data gradient), and for the e4m3 MLP weight
    gradients ``a2(i)`` = ln_2 output (2 L + 2 i) and ``g(i)`` = the residual gradient that enters block i's MLP branch
    (2 L + 2 i + 1).  Not ``ready`` until one backward has run.  Off the fp8 path the table has no slots."""
    HISTORY = 4                 # steps of per-tensor maxima the delayed scales are taken over

    def __init__(self, layers: int, device):
        n, self.layers = 4 * layers, layers
        self.scale = torch.zeros(n, dtype=F32, device=device)
        self.scale_inv = torch.ones(n, dtype=F32, device=device)
        self.amax = torch.zeros((n, 64), dtype=F32, device=device)
        self.hist = torch.zeros((self.HISTORY, n), dtype=F32, device=device)
        self.ready, self.step = False, 0

    def _slot(self, k: int):
        return self.scale[k:k + 1], self.scale_inv[k:k + 1], self.amax[k]

    def h(self, i: int):
        return self._slot(2 * i)

    def dU(self, i: int):
        return self._slot(2 * i + 1)

    def a2(self, i: int):
        return self._slot(2 * self.layers + 2 * i)

    def g(self, i: int):
        return self._slot(2 * self.layers + 2 * i + 1)

    def reset(self) -> None:
        """Forget the history (the next step runs the h / dU consumers in bf16 and records fresh maxima): the fp8 path is a
        function of (weights, batch, scales of the previous steps).  Called whenever the weights are replaced."""
        self.ready, self.step = False, 0
        self.scale.zero_()
        self.scale_inv.fill_(1.0)
        self.amax.zero_()
        self.hist.zero_()

    def state(self) -> Dict[str, object]:
        """Host tensors, checkpointed beside the weights: a resumed run continues with the scales it stopped with."""
        return {"scale": self.scale.cpu(), "scale_inv": self.scale_inv.cpu(), "hist": self.hist.cpu(),
                "ready": bool(self.ready), "step": int(self.step)}

    def load(self, st) -> None:
        self.reset()
        if not isinstance(st, dict):
            return
        want = {"scale": self.scale, "scale_inv": self.scale_inv, "hist": self.hist}
        for k, dst in want.items():          # a malformed / foreign checkpoint entry resets the history instead of raising
            t = st.get(k)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(dst.shape):
                return
        for k, dst in want.items():
            dst.copy_(st[k])
        self.ready, self.step = bool(st.get("ready", False)), int(st.get("step", 0))

    def update(self) -> None:
        """Next step's scales from the maxima of the last HISTORY steps (enqueued on the current stream)."""
        ops.fp8_scale_update(self.amax, self.scale, self.scale_inv, margin_bits=1, hist=self.hist, slot=self.step % self.HISTORY)
        self.step += 1
        self.ready = True


@dataclass
class StackPass:
    """What one forward of the stack leaves for its backward."""
    B: int
    L: int
    M: int
    r16: bool                           # residual stream in bf16
    w8: bool                            # the per-tensor e4m3 copies for the MLP weight gradients were written
    u_holds_grad: bool = True           # the u buffers hold gelu'(u) (default) or u itself (recomputation mode)
    q_cls_only: bool = False            # the last block projected q for the class tokens only
    x_in: List[Optional[torch.Tensor]] = field(default_factory=list)      # input of every block
    g_t8_ok: bool = False               # class-token block's backward: it left the e4m3 copy of its residual gradient ...
    g_q8: Optional[tuple] = None        # ... and the row-scaled one


class GradRing:
    """The residual gradient between the blocks: three rotating bf16 buffers (a side launch may still read the one the chain
    left two hops ago) and, for the e4m3 MLP weight gradients, a per-tensor e4m3 copy in the same slot."""

    def __init__(self, bf16, t8=None):
        self._bf16, self._t8, self._pos = bf16, t8, 0

    @property
    def current(self):
        return self._bf16[self._pos], (self._t8[self._pos] if self._t8 is not None else None)

    def advance(self):
        self._pos = (self._pos + 1) % 3
        return self.current


@dataclass
class _Bwd:
    """One backward call: the pass it belongs to, its schedule, the buffers every block shares and the two facts that travel
    from block to block."""
    p: StackPass
    sched: SideScheduler
    dres: torch.Tensor
    qg: Optional[tuple]                 # fp8: (e4m3 bytes, row scale_inv) scratch of the residual gradient LayerNorm backward forms
    g16: bool                           # residual gradient between the blocks in bf16
    w8: bool                            # e4m3 MLP weight gradients: per-tensor copies travel beside the ring
    wg_mode: str
    dA: torch.Tensor
    dO: torch.Tensor
    delta: torch.Tensor
    ring: Optional[GradRing] = None
    g_has_q8: bool = False              # is the e4m3 copy of the current residual gradient in qg?
    g0_t8_ok: bool = False              # does the ring's e4m3 slot hold the copy of its current bf16 slot?


class TransformerStack:
    """N pre-LN residual attention blocks (ResidualAttentionBlock, transformer.py:238-300)."""

    OVERLAP_TRIAL_CALLS = (2, 4)                  # untimed warm-up calls, timed calls per schedule
    OVERLAP_MARGIN = 0.01                         # one stream must beat the side stream by this fraction to be chosen

    def __init__(self, store: ParamStore, prefix: str, width: int, heads: int, layers: int, mlp: int, causal: bool,
                 cls_only_last: bool = False, res16_ok: bool = False, quick_gelu: bool = False):
        # cls_only_last: only token 0 of the last block's output is consumed downstream (ViT pool 'tok'), so that
        # block computes K/V for all tokens but attention output, out_proj and the MLP for the CLS rows only -- the
        # values the reference would compute for the other 196 rows are dead.
        self.cls_only_last = cls_only_last and os.environ.get("SC_CLS_ONLY", "1") != "0"
        self.s, self.prefix = store, prefix
        self.d, self.H, self.layers, self.mlp, self.causal = width, heads, layers, mlp, causal
        self.dh = width // heads
        self.bufs = _Bufs(store.device)
        # act_layer = QuickGELU for towers built from a `quick_gelu: true` config (OpenAI-pretrained weights,
        # src/open_clip/model.py:142-145,228): the three GELU epilogues with x * sigmoid(1.702 x) and its derivative
        self.quick_gelu = bool(quick_gelu)
        self.epi_pair, self.epi_grad_pair, self.epi_dgelu = ops.act_epilogues(self.quick_gelu)
        self.fp8 = bool(getattr(store, "fp8", False))
        # residual stream in bf16 (what the reference's autocast keeps; SC_RES_STREAM, read at every forward) for the towers
        # whose stem / head kernels take it (the patch towers); off: fp32 stream
        self.res16_ok = res16_ok
        self.res_stream = "bf16"
        # activation recomputation (set_grad_checkpointing): the LayerNorm outputs and the GELU output of a block are not
        # kept for the backward (12 of the 36 d bytes a token saves per block); the backward rebuilds them, bit-identically,
        # from the saved residual stream / pre-activation right before the weight-gradient GEMMs that read them
        self.recompute = False
        # fp8 delayed scaling (h = GELU output -> c_proj forward, dU -> c_fc data gradient; Fp8Scales).  SC_FP8_DELAYED=0: A/B
        # switch that keeps the h / dU consumers in bf16
        self.scales = Fp8Scales(layers if self.fp8 else 0, store.device)
        self._dq_on = os.environ.get("SC_FP8_DELAYED", "1") != "0"
        # a forward whose backward will run (grad mode on: set by SpatialClipNet.forward) records maxima and may consume the
        # delayed scales; evaluation forwards (validation, test, zero-shot bank) do neither: they run the h consumer in bf16, so
        # a fresh eval process and an in-fit validation of the same weights give the same numbers (advisor, round 3)
        self.fp8_train_pass = False     # set per call by SpatialClipNet.forward; encode_image / encode_text never train
        # e4m3 weight gradients of the MLP pair (round 4, sc_gemm_wgrad_fp8): their operands need ONE scale per tensor -- h and
        # dU have such copies already; the LayerNorm kernels add per-tensor copies of a2 = ln_2(x) and of the residual gradient
        # g0 that enters the block's MLP branch.  SC_FP8_WGRAD=0: A/B.
        self._w8_on = os.environ.get("SC_FP8_WGRAD", "1") != "0"
        self.fwd: Optional[StackPass] = None        # the last forward, read by its backward
        self.no_side_stream = False     # set by SpatialClipNet: this stack runs beside the other tower on a stream of its own
        self._side: Optional[torch.cuda.Stream] = None      # ONE weight-gradient side stream per stack, created on first use
        self._trials: Dict[tuple, OverlapTrial] = {}        # SC_OVERLAP=auto: (B, L) -> trial
        self._zero_bias_set = False
        # locked tower (lock.TowerLock): index of the first trainable block.  The blocks below it run their forward as ever but
        # keep nothing per block (their buffers rotate between two sets) and the backward stops after block ``floor``
        self.floor = 0

    def _tag(self, i: int) -> str:
        """Buffer-name tag of block ``i``: its index, or one of two rotating sets for a locked block."""
        return f"lk{i & 1}" if i < self.floor else str(i)

    @property
    def r16(self) -> bool:
        """Did the last forward run the residual stream in bf16?"""
        return self.fwd is not None and self.fwd.r16

    @property
    def x_in(self) -> List[Optional[torch.Tensor]]:
        """The block inputs of the last forward."""
        return self.fwd.x_in

    def set_grad_checkpointing(self, enable: bool = True) -> None:
        self.recompute = bool(enable)

    def overlap_choice(self, B: int, L: int) -> Optional[bool]:
        """The schedule SC_OVERLAP=auto settled on for this batch shape: True = side stream, False = one stream, None = still
        measuring (or pinned by SC_OVERLAP=0 / 1)."""
        t = self._trials.get((B, L))
        return None if t is None else t.choice

    def overlap_timing(self, B: int, L: int) -> Optional[Dict[str, float]]:
        """The best backward time (ms) SC_OVERLAP=auto measured on each schedule for this batch shape, or None."""
        t = self._trials.get((B, L))
        return None if t is None else t.ms_best

    def overlap_settled(self) -> bool:
        """Has SC_OVERLAP=auto chosen for every batch shape this stack has run (and for at least one)?"""
        return bool(self._trials) and all(t.choice is not None for t in self._trials.values())

    def _act(self, kind: str, i: int, shape) -> torch.Tensor:
        """Buffer of a block's recomputable activation (a1 / a2 / h): one per block, or two rotating ones in
        recomputation mode (the CLS-only last block keeps its own: it runs first in the backward, nothing to rebuild)."""
        if i < self.floor:
            return self.bufs.get(f"{kind}.lk{i & 1}", shape, BF16)
        if self.recompute and not (self.cls_only_last and i == self.layers - 1):
            return self.bufs.get(f"{kind}.rc{i & 1}", shape, BF16)
        return self.bufs.get(f"{kind}.{i}", shape, BF16)

    def _linear_fwd(self, epi: int, x: torch.Tensor, name: str, out: torch.Tensor, *, M: int, N: int, K: int, q8=None,
                    **kw):
        """One forward Linear of a full-width block: the bf16 MFMA GEMM, or -- fp8 path, when the producer of ``x`` has
        also emitted its e4m3 copy ``q8 = (bytes, scale_inv)`` and the weight has an e4m3 copy -- the fp8 MFMA GEMM."""
        cp = self.s.copies[name]
        if q8 is None or cp.w8 is None:
            return ops.gemm(ops.NT, epi, x, cp.wf, out, M=M, N=N, K=K, **kw)
        return ops.gemm_fp8(epi, q8[0], q8[1], cp.w8, cp.w8s, out, M=M, N=N, K=K, **kw)

    def _zero_bias(self, n: int) -> torch.Tensor:
        z = self.bufs.get("zero.bias", (n,), F32, shared=True)
        if not self._zero_bias_set:
            z.zero_()
            self._zero_bias_set = True
        return z

    def _q_dead_ok(self, qa, i: int) -> bool:
        """May the last block skip the q projection of the rows whose attention output nobody reads?  bf16 operands only (the
        e4m3 GEMMs take whole-matrix scales), unpadded K; ``SC_CLS_Q=0`` restores the full projection."""
        cp = self.s.copies[self._n(i, "attn.in_proj_weight")]
        return (qa is None or cp.w8 is None) and cp.wf.shape[1] == self.d and self.d % 64 == 0 and \
            os.environ.get("SC_CLS_Q", "1") != "0"

    def _q8(self, tag: str, M: int, K: int):
        """(e4m3 bytes [M, K], scale_inv [M]) scratch for a fused quantiser output, or None off the fp8 path."""
        if not self.fp8:
            return None
        return self.bufs.get(f"q8.{tag}", (M, K), torch.uint8), self.bufs.get(f"q8s.{tag}", (M,), F32)

    def _n(self, i: int, leaf: str) -> str:
        return f"{self.prefix}{i}.{leaf}"

    def _stats(self, k: int, i: int, rows: int):
        """(mean, rstd) buffers of LayerNorm ``k`` (1 or 2) of block ``i``."""
        t = self._tag(i)
        return self.bufs.get(f"m{k}.{t}", (rows,), F32), self.bufs.get(f"r{k}.{t}", (rows,), F32)

    def layer_param_names(self, i: int) -> List[str]:
        leaves = ["ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                  "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                  "mlp.c_proj.weight", "mlp.c_proj.bias"]
        return [self._n(i, l) for l in leaves]

    # -------------------------------------------------------------------------------- forward
    def forward(self, x0: torch.Tensor, B: int, L: int) -> torch.Tensor:
        s, d, mlp, bf = self.s, self.d, self.mlp, self.bufs
        M = B * L
        r16 = self.res16_ok and _res_stream_bf16(self.res_stream)
        x = x0
        if r16 and x0.dtype != BF16:                  # a stem that writes fp32 (the text tower's embedding): one cast pass per step
            x = ops.cast_pad_bf16(x0, bf.get("x0.16", (M, d), BF16), M, d, d)
        # e4m3 MLP weight gradients: only for a pass that will be differentiated, on the bf16 stream (the per-tensor LayerNorm
        # copies exist for bf16 rows), token count a multiple of the 128-token K tile.  With activation recomputation the e4m3
        # copies of h and a2 are KEPT per block (1 + 0.25 bytes per MLP element instead of the 2 + 0.5 of the bf16 tensors that
        # recomputation drops), and the backward then has nothing to rebuild for the MLP branch
        w8 = bool(self.fp8 and self._dq_on and self._w8_on and self.fp8_train_pass and r16
                  and M % 128 == 0 and d % 16 == 0 and mlp % 16 == 0 and d >= 256 and mlp >= 256)
        # the MLP's backward needs gelu'(u), not u: the default path stores that factor (the forward epilogue holds the erf
        # pieces anyway) and the c_proj data gradient becomes one multiply; recomputation mode keeps u, from which it rebuilds
        # h = gelu(u)
        p = self.fwd = StackPass(B, L, M, r16, w8, u_holds_grad=not self.recompute, x_in=[None] * self.layers)
        if self.floor >= 2:
            self._reserve_locked_sets(p)
        for i in range(self.layers):
            s.wait_names(self.layer_param_names(i))      # sharded optimiser: this block's refreshed weights have landed (no-op otherwise)
            p.x_in[i] = x
            x = self._block_fwd(i, x, p)
        return x

    def _reserve_locked_sets(self, p: StackPass) -> None:
        """Both rotating buffer sets of a locked prefix, whole, whatever the blocks will touch (a class-token-only last block
        leaves the MLP part of its set unused): the activation memory of the prefix is the same at every depth."""
        bf, d, mlp, M = self.bufs, self.d, self.mlp, p.M
        XD = BF16 if p.r16 else F32
        for t in ("lk0", "lk1"):
            for kind, shape, dt in (("a1", (M, d), BF16), ("a2", (M, d), BF16), ("h", (M, mlp), BF16), ("qkv", (M, 3 * d), BF16),
                                    ("o", (M, d), BF16), ("u", (M, mlp), BF16), ("xmid", (M, d), XD), ("xout", (M, d), XD),
                                    ("lse", (p.B, self.H, p.L), F32), ("m1", (M,), F32), ("r1", (M,), F32), ("m2", (M,), F32),
                                    ("r2", (M,), F32)):
                bf.get(f"{kind}.{t}", shape, dt)

    def _block_fwd(self, i: int, x: torch.Tensor, p: StackPass) -> torch.Tensor:
        s, d, mlp, bf, B, L, M = self.s, self.d, self.mlp, self.bufs, p.B, p.L, p.M
        XD = BF16 if p.r16 else F32                   # dtype of the residual stream between the blocks
        epi_res = ops.EPI_BF16_BIAS_RES if p.r16 else ops.EPI_F32_BIAS_RES
        a1 = self._act("a1", i, (M, d))
        qa = self._q8("a", M, d)            # fp8: LayerNorm also emits the e4m3 copy + row scales (rotating scratch)
        ops.layernorm_fwd(x, s.p(self._n(i, "ln_1.weight")), s.p(self._n(i, "ln_1.bias")), a1, *self._stats(1, i, M), M, d,
                          q8=qa and qa[0], q8_scale_inv=qa and qa[1])
        tg = self._tag(i)
        qkv = bf.get(f"qkv.{tg}", (M, 3 * d), BF16)
        last_cls = self.cls_only_last and i == self.layers - 1
        p.q_cls_only = last_cls and self._q_dead_ok(qa, i)
        if p.q_cls_only:
            # last block, only the class token is consumed: K and V of every token, but Q of the class tokens alone -- the
            # other rows' q (a third of this GEMM, of its data gradient and of its weight gradient) is never read
            wq = s.copies[self._n(i, "attn.in_proj_weight")].wf
            bq = s.p(self._n(i, "attn.in_proj_bias"))
            ops.gemm(ops.NT, ops.EPI_BF16_BIAS, a1, wq[d:], qkv[:, d:], M=M, N=2 * d, K=d, bias=bq[d:])
            ops.gemm(ops.NT, ops.EPI_BF16_BIAS, a1.view(B, L * d)[:, :d], wq[:d], qkv.view(B, L * 3 * d)[:, :d],
                     M=B, N=d, K=d, bias=bq[:d])
        else:
            self._linear_fwd(ops.EPI_BF16_BIAS, a1, self._n(i, "attn.in_proj_weight"), qkv,
                             M=M, N=3 * d, K=d, bias=s.p(self._n(i, "attn.in_proj_bias")), q8=qa)
        o = bf.get(f"o.{tg}", (M, d), BF16)
        lse = bf.get(f"lse.{tg}", (B, self.H, L), F32)
        if last_cls:
            return self._forward_last_cls(i, x, qkv, o, lse, p)
        ops.attn_fwd(qkv, B, L, self.H, self.dh, self.causal, out=o, lse=lse)
        xmid = bf.get(f"xmid.{tg}", (M, d), XD)
        self._linear_fwd(epi_res, o, self._n(i, "attn.out_proj.weight"), xmid,
                         M=M, N=d, K=d, bias=s.p(self._n(i, "attn.out_proj.bias")), res=x)
        a2 = self._act("a2", i, (M, d))
        t8a = None
        if p.w8:        # per-tensor e4m3 copy of a2, kept per block: X operand of the e4m3 c_fc weight gradient
            sc, _, amax = self.scales.a2(i)
            t8a = (bf.get(f"t8.a2.{i}", (M, d), torch.uint8), sc, amax)
        ops.layernorm_fwd(xmid, s.p(self._n(i, "ln_2.weight")), s.p(self._n(i, "ln_2.bias")), a2, *self._stats(2, i, M), M, d,
                          q8=qa and qa[0], q8_scale_inv=qa and qa[1], t8=t8a)
        u = bf.get(f"u.{tg}", (M, mlp), BF16)
        h = self._act("h", i, (M, mlp))
        hq = None
        if self.fp8 and self._dq_on and self.fp8_train_pass:      # the GELU epilogue also emits e4m3(h) with last step's scale + records max|h|
            h8 = bf.get(f"q8.h.{i}" if p.w8 else "q8.h", (M, mlp), torch.uint8)     # kept per block when the weight gradient reads it
            h_scale, h_scale_inv, h_amax = self.scales.h(i)
            hq = dict(q8_out=h8, q8_scale=h_scale, q8_amax=h_amax)
        self._linear_fwd(self.epi_grad_pair if p.u_holds_grad else self.epi_pair, a2, self._n(i, "mlp.c_fc.weight"), u,
                         M=M, N=mlp, K=d, bias=s.p(self._n(i, "mlp.c_fc.bias")), out2=h, q8=qa, **(hq or {}))
        xo = bf.get(f"xout.{tg}", (M, d), XD)
        cpj = s.copies[self._n(i, "mlp.c_proj.weight")]
        if hq is not None and self.scales.ready and cpj.w8 is not None:
            ops.gemm_fp8(epi_res, h8, h_scale_inv, cpj.w8, cpj.w8s, xo, M=M, N=d,
                         K=mlp, bias=s.p(self._n(i, "mlp.c_proj.bias")), res=xmid, a_scale_scalar=True)
        else:
            self._linear_fwd(epi_res, h, self._n(i, "mlp.c_proj.weight"), xo,
                             M=M, N=d, K=mlp, bias=s.p(self._n(i, "mlp.c_proj.bias")), res=xmid)
        return xo

    def _forward_last_cls(self, i: int, x: torch.Tensor, qkv: torch.Tensor, o: torch.Tensor, lse: torch.Tensor, p: StackPass):
        """Last block, CLS rows only (compact [B, d] tensors; the CLS rows of full tensors are strided views)."""
        s, d, mlp, bf, B, L = self.s, self.d, self.mlp, self.bufs, p.B, p.L
        ops.attn_fwd(qkv, B, L, self.H, self.dh, self.causal, out=o, lse=lse, q_rows=1)
        o_c = o.view(B, L * d)[:, :d]
        x_c = x.view(B, L * d)[:, :d]
        XD = BF16 if p.r16 else F32
        epi_res = ops.EPI_BF16_BIAS_RES if p.r16 else ops.EPI_F32_BIAS_RES
        xmid = bf.get("c.xmid", (B, d), XD)
        ops.gemm(ops.NT, epi_res, o_c, s.copies[self._n(i, "attn.out_proj.weight")].wf, xmid,
                 M=B, N=d, K=d, bias=s.p(self._n(i, "attn.out_proj.bias")), res=x_c)
        a2 = bf.get("c.a2", (B, d), BF16)
        ops.layernorm_fwd(xmid, s.p(self._n(i, "ln_2.weight")), s.p(self._n(i, "ln_2.bias")), a2,
                          bf.get("c.m2", (B,), F32), bf.get("c.r2", (B,), F32), B, d)
        u, h = bf.get("c.u", (B, mlp), BF16), bf.get("c.h", (B, mlp), BF16)
        ops.gemm(ops.NT, self.epi_grad_pair, a2, s.copies[self._n(i, "mlp.c_fc.weight")].wf, u, M=B, N=mlp, K=d,
                 bias=s.p(self._n(i, "mlp.c_fc.bias")), out2=h)           # "u" holds gelu'(u): this block is never recomputed
        xo = bf.get("c.xout", (B, d), XD)
        ops.gemm(ops.NT, epi_res, h, s.copies[self._n(i, "mlp.c_proj.weight")].wf, xo, M=B, N=d, K=mlp,
                 bias=s.p(self._n(i, "mlp.c_proj.bias")), res=xmid)
        return xo

    # -------------------------------------------------------------------------------- backward
    def _backward_last_cls(self, c: _Bwd, dres_c_bf: torch.Tensor) -> torch.Tensor:
        """Backward of the CLS-only last block.  In: dL/d(x_out[CLS]) in the class-token rows of the FULL fp32 buffer
        ``c.dres`` [M, d] (the other rows hold nothing yet) + its compact bf16 copy.  Out: the same fp32 buffer and a full
        bf16 buffer (returned) holding dL/d(block input) for every row."""
        s, d, mlp, bf, p, dres = self.s, self.d, self.mlp, self.bufs, c.p, c.dres
        B, L, M = p.B, p.L, p.M
        i = self.layers - 1
        g = lambda leaf: s.g(self._n(i, leaf))
        cp = lambda leaf: s.copies[self._n(i, leaf)]
        a1, qkv, o = bf.get(f"a1.{i}", (M, d), BF16), bf.get(f"qkv.{i}", (M, 3 * d), BF16), bf.get(f"o.{i}", (M, d), BF16)
        lse = bf.get(f"lse.{i}", (B, self.H, L), F32)
        a2, u, h, xmid = bf.get("c.a2", (B, d), BF16), bf.get("c.u", (B, mlp), BF16), bf.get("c.h", (B, mlp), BF16), \
            bf.get("c.xmid", (B, d), BF16 if p.r16 else F32)
        dU = bf.get("c.dU", (B, mlp), BF16)
        dA_c = bf.get("c.dA", (B, d), BF16)
        ops.gemm(ops.NT, ops.EPI_BF16_MUL_AUX, dres_c_bf, cp("mlp.c_proj.weight").wb, dU, M=B, N=mlp, K=d, aux=u)
        mlp_probs = [(dres_c_bf, h, g("mlp.c_proj.weight"), None, d, mlp), (dU, a2, g("mlp.c_fc.weight"), g("mlp.c_fc.bias"), mlp, d)]
        c.sched.run(lambda: launch_wgrads(mlp_probs, B, "cls", c.wg_mode))
        ops.gemm(ops.NT, ops.EPI_BF16, dU, cp("mlp.c_fc.weight").wb, dA_c, M=B, N=d, K=mlp)
        g1_c = bf.get("c.dres_bf1", (B, d), BF16)
        ops.layernorm_bwd(dA_c, xmid, bf.get("c.m2", (B,), F32), bf.get("c.r2", (B,), F32),
                          s.p(self._n(i, "ln_2.weight")), dres, g1_c, g("ln_2.weight"), g("ln_2.bias"),
                          g("attn.out_proj.bias"), B, d, accumulate=True, lddres=L * d)      # in place on the class-token rows
        # attention branch: only the CLS rows of dO exist (written through a strided view); sc_attn_bwd with q_rows = 1
        # reads nothing else of dO / o and writes ALL of dqkv (zeros for the dq rows nobody consumed): no memsets
        ops.gemm(ops.NT, ops.EPI_BF16, g1_c, cp("attn.out_proj.weight").wb, c.dO.view(B, L * d)[:, :d], M=B, N=d, K=d)
        dqkv = bf.get(f"dqkv.{i & 1}", (M, 3 * d), BF16)
        ops.attn_bwd(qkv, o, c.dO, lse, B, L, self.H, self.dh, self.causal, dqkv=dqkv, delta=c.delta, q_rows=1)
        dq_c, a1_c = dqkv.view(B, L * 3 * d)[:, :d], a1.view(B, L * d)[:, :d]
        gw, gb = g("attn.in_proj_weight"), g("attn.in_proj_bias")

        def w_attn():
            launch_wgrads([(g1_c, o.view(B, L * d)[:, :d], g("attn.out_proj.weight"), None, d, d)], B, "cls", c.wg_mode)
            if p.q_cls_only:    # dq is zero off the class-token rows: W_q's gradient from those B rows, W_k / W_v's from all
                launch_wgrads([(dqkv[:, d:], a1, gw[d:], gb[d:], 2 * d, d)], M, "attn", "0")
                launch_wgrads([(dq_c, a1_c, gw[:d], gb[:d], d, d)], B, "cls", c.wg_mode)
            else:
                launch_wgrads([(dqkv, a1, gw, gb, 3 * d, d)], M, "attn", "0")
        c.sched.run(w_attn, (dqkv,))
        wb = cp("attn.in_proj_weight").wb
        if p.q_cls_only:    # data gradient: the k | v columns for every row, then the q columns added on the class-token rows
            ops.gemm(ops.NT, ops.EPI_BF16, dqkv[:, d:], wb[:, d:], c.dA, M=M, N=d, K=2 * d)
            dA_c = c.dA.view(B, L * d)[:, :d]
            ops.gemm(ops.NT, ops.EPI_BF16_BIAS_RES, dq_c, wb[:, :d], dA_c, M=B, N=d, K=d, bias=self._zero_bias(d), res=dA_c)
        else:
            ops.gemm(ops.NT, ops.EPI_BF16, dqkv, wb, c.dA, M=M, N=d, K=3 * d)
        dres_bf = bf.get("dres_bf.0", (M, d), BF16)
        prev_bias = s.g(self._n(i - 1, "mlp.c_proj.bias")) if i > self.floor else None    # block i - 1 locked: no gradient of its bias
        qg = p.g_q8 = self._q8("g", M, d)
        t8g = None
        if p.w8 and i > 0 and qg is not None and _res_grad_bf16():     # per-tensor e4m3 copy: dY of block i - 1's c_proj weight gradient
            sc, _, amax = self.scales.g(i - 1)
            t8g = (bf.get("t8.g.0", (M, d), torch.uint8), sc, amax)
        ops.layernorm_bwd(c.dA, p.x_in[i], *self._stats(1, i, M),
                          s.p(self._n(i, "ln_1.weight")), dres, dres_bf, g("ln_1.weight"), g("ln_1.bias"),
                          prev_bias, M, d, accumulate=-L,       # only the class-token rows carry a residual gradient
                          q8=qg and qg[0], q8_scale_inv=qg and qg[1],
                          g16=_res_grad_bf16(), write_f32=(i == 0), t8=t8g)  # bf16 stream: fp32 only in front of the stem
        p.g_t8_ok = t8g is not None
        return dres_bf

    def _schedule(self, p: StackPass, main):
        """(use the side stream?, trial record or None) for this backward call.  Whether the side stream pays depends on the
        shapes: round 2 measured 37.8 vs 38.4 ms/step with it on ViT-B/16 (B = 256); with round 4's kernels the same model is
        0.4-0.5 ms FASTER on one stream, while the configs[4] model gains 2.1-2.4 ms (bf16) / 4 ms (e4m3) from the side stream
        (profiles/r04_side_stream_auto.txt).  Both schedules give the same bits (tests/test_gpu_model.py), so the default,
        SC_OVERLAP=auto, times this stack's own backward in both (OverlapTrial) and keeps the faster one; SC_OVERLAP=1 / 0 pin
        it, and a stack that runs beside the other tower on a stream of its own (net.py) never opens a side stream."""
        ov_env = "0" if self.no_side_stream else os.environ.get("SC_OVERLAP", "auto")
        trial = None
        if ov_env in ("0", "1"):
            overlap = ov_env == "1"
        else:
            overlap, trial = self._trials.setdefault((p.B, p.L), OverlapTrial()).next(
                main, *self.OVERLAP_TRIAL_CALLS, self.OVERLAP_MARGIN)
        if overlap and self._side is None:
            # lowest priority the runtime offers: the side stream's workgroups should only take what the chain leaves
            self._side = torch.cuda.Stream(priority=int(os.environ.get("SC_SIDE_PRIO", "1")))
        return overlap, trial

    def backward(self, dres: torch.Tensor, dres_bf: torch.Tensor, last_bias_colsum_done: bool,
                 on_layer_done: Optional[Callable[[int], None]] = None) -> None:
        """``dres`` (fp32) / ``dres_bf`` (bf16 copy) hold dL/d(output of the last block) on entry; ``dres`` holds
        dL/d(input of block 0) on exit.  ``last_bias_colsum_done``: the caller already wrote the last block's
        c_proj.bias gradient (column sum of dres).  The data-gradient chain (dgrad GEMMs, attention backward, LayerNorm
        backward) is the critical path on the caller's stream; what only feeds the optimiser goes through the SideScheduler and
        fills the tail rounds / memory-bound phases of the chain.  Buffers a side kernel reads (bf16 residual gradient, dU,
        dqkv) rotate."""
        p, bf, d = self.fwd, self.bufs, self.d
        B, L, M = p.B, p.L, p.M
        main = torch.cuda.current_stream()
        overlap, trial = self._schedule(p, main)
        # LayerNorm backward: the token pass stays on the chain; the column reductions (dgamma, dbeta, the bias gradient
        # of the Linear in front) feed only the optimiser, so with the side stream on they leave their partial sums in
        # one of four rotating workspaces and are finished on the side stream
        ln_ws_n = ops.layernorm_bwd_ws_floats(M, d)
        sched = SideScheduler(overlap, main, self._side if overlap else main,
                              [bf.get(f"ln_ws.{k}", (ln_ws_n,), F32) for k in range(4)] if overlap else None)
        # The residual gradient between the blocks travels in bf16 (three rotating buffers), which is the precision the
        # reference's autocast carries it in; the fp32 buffer is written by the stack's last hop only (the stem reads it).
        # SC_RES_GRAD=fp32 keeps the fp32 read-modify-write of rounds 1-2 (16 instead of 10 bytes per element).  The text
        # tower has an fp32 stream AND an fp32 residual gradient, as the reference's.
        g16 = _res_grad_bf16() and self.res16_ok
        # fp8 path: LayerNorm backward also emits the e4m3 copy (+ row scales) of the residual gradient it has just formed -- the
        # A operand of the next data-gradient GEMM.  Producer and consumer are both on the chain, back to back: ONE scratch.
        qg = self._q8("g", M, d)
        c = _Bwd(p, sched, dres, qg, g16, bool(p.w8 and g16 and qg is not None), os.environ.get("SC_WGRAD_GROUP", "auto"),
                 bf.get("dA", (M, d), BF16), bf.get("dO", (M, d), BF16), bf.get("delta", (B, self.H, L), F32))
        top = self.layers
        if self.cls_only_last:
            dres_bf = self._backward_last_cls(c, dres_bf)
            top -= 1
            c.g_has_q8 = qg is not None
            c.g0_t8_ok = c.w8 and p.g_t8_ok
            if on_layer_done is not None:
                sched.run(lambda: on_layer_done(top))
        c.ring = GradRing([dres_bf, bf.get("dres_bf.1", (M, d), BF16), bf.get("dres_bf.2", (M, d), BF16)],
                          [bf.get(f"t8.g.{k}", (M, d), torch.uint8) for k in range(3)] if c.w8 else None)
        for i in reversed(range(self.floor, top)):     # a locked tower's backward stops after its first trainable block
            if i == self.layers - 1 and not last_bias_colsum_done:
                ops.colsum_bf16(c.ring.current[0], M, d, self.s.g(self._n(i, "mlp.c_proj.bias")))
            mlp_wgrads = self._mlp_bwd(i, c)
            self._attn_bwd(i, c, *mlp_wgrads)
            if on_layer_done is not None:
                sched.run(lambda: on_layer_done(i))      # the bucket all-reduce follows the side stream
        # Join the side stream BEFORE the scale update: the side stream's e4m3 weight-gradient GEMMs read the inverse scales
        # through device pointers when they RUN (sc_gemm8p.hip), and the low-priority side stream can lag the chain by
        # several blocks -- an update enqueued on the chain first could replace a scale that operands quantised with the old
        # one are still waiting to be multiplied by (advisor, round 4).
        sched.join()
        if self.fp8 and self._dq_on:
            self.scales.update()
        if trial is not None:                     # end of a timed trial call (the side stream's work is joined above)
            trial[2].record(main)
        return dres

    def _ln_bwd(self, c: _Bwd, dy, x, stats, gamma, g_in, g_bf, dgamma, dbeta, colsum, last=False, t8=None) -> None:
        """LayerNorm backward of a full-width block; with the side stream on, its column reductions are finished there."""
        M, d = c.p.M, self.d
        kw = dict(q8=c.qg[0], q8_scale_inv=c.qg[1]) if c.qg is not None else {}
        if c.g16:
            kw.update(g16=True, g_in=g_in, write_f32=last)
        if t8 is not None:
            kw.update(t8=t8)
        if not c.sched.overlap:
            ops.layernorm_bwd(dy, x, *stats, gamma, c.dres, g_bf, dgamma, dbeta, colsum, M, d, accumulate=True, **kw)
            return
        ws = c.sched.ln_workspace()
        ops.layernorm_bwd(dy, x, *stats, gamma, c.dres, g_bf, dgamma, dbeta, colsum, M, d, accumulate=True,
                          ws=ws, defer_reduce=True, **kw)
        c.sched.run(lambda: ops.layernorm_bwd_reduce(ws, dgamma, dbeta, colsum, M, d), (ws,))

    def _dgrad(self, c: _Bwd, epi, g_bf, name, out, *, N, K, have_q8, q8kw=None, **kw) -> None:
        """Data-gradient GEMM out[M, N] = g[M, K] . W (NT against the transposed weight copy): e4m3 operands when the
        residual gradient's e4m3 copy is live in ``c.qg`` and the weight has one, bf16 otherwise."""
        w = self.s.copies[name]
        if have_q8 and c.qg is not None and w.wb8 is not None:
            ops.gemm_fp8(epi, c.qg[0], c.qg[1], w.wb8, w.wb8s, out, M=c.p.M, N=N, K=K, **kw, **(q8kw or {}))
        else:
            ops.gemm(ops.NT, epi, g_bf, w.wb, out, M=c.p.M, N=N, K=K, **kw)

    def _mlp_bwd(self, i: int, c: _Bwd):
        """MLP branch of block i: x_out = xmid + c_proj(gelu(c_fc(ln_2(xmid)))).  Returns (its weight-gradient problems, the
        buffers they read) for SC_WGRAD_GROUP=4, which launches them with the attention branch's."""
        s, d, mlp, bf, p, sched = self.s, self.d, self.mlp, self.bufs, c.p, c.sched
        M = p.M
        g = lambda leaf: s.g(self._n(i, leaf))
        a2, u, h = self._act("a2", i, (M, d)), bf.get(f"u.{i}", (M, mlp), BF16), self._act("h", i, (M, mlp))
        xmid = bf.get(f"xmid.{i}", (M, d), BF16 if p.r16 else F32)
        dU = bf.get(f"dU.{i & 1}", (M, mlp), BF16)
        g0, g0_8 = c.ring.current
        sched.before_write(dU)
        dq = dU8 = None
        if self.fp8 and self._dq_on:      # GELU' epilogue: e4m3(dU) with last step's scale + max|dU| for the next one
            dU8 = bf.get(f"q8.dU.{i & 1}" if c.w8 else "q8.dU", (M, mlp), torch.uint8)     # rotates with dU when the side stream reads it
            sched.before_write(dU8)
            dU_scale, dU_scale_inv, dU_amax = self.scales.dU(i)
            dq = dict(q8_out=dU8, q8_scale=dU_scale, q8_amax=dU_amax)
        dU_has_q8 = dq is not None and c.g_has_q8 and self.scales.ready
        # aux = the stored factor gelu'(u) (default) or u itself (recomputation mode): same bits either way
        self._dgrad(c, ops.EPI_BF16_MUL_AUX if p.u_holds_grad else self.epi_dgelu, g0, self._n(i, "mlp.c_proj.weight"), dU,
                    N=mlp, K=d, have_q8=c.g_has_q8, aux=u, q8kw=dq)
        probs = [(g0, h, g("mlp.c_proj.weight"), None, d, mlp), (dU, a2, g("mlp.c_fc.weight"), g("mlp.c_fc.bias"), mlp, d)]
        # e4m3 weight gradients of the MLP pair: every operand has a per-tensor copy made with scales that were ready when the
        # forward ran (h8 / a2 by the forward, dU8 / g0 by this backward); the first step after a reset stays in bf16
        w8_now = bool(c.w8 and dU_has_q8 and c.g0_t8_ok)
        fp8 = None
        if w8_now:
            fp8 = [(g0_8, self.scales.g(i)[1], bf.get(f"q8.h.{i}", (M, mlp), torch.uint8), self.scales.h(i)[1]),
                   (dU8, dU_scale_inv, bf.get(f"t8.a2.{i}", (M, d), torch.uint8), self.scales.a2(i)[1])]
        rebuild = self.recompute and not w8_now     # h = gelu(u) and a2 = ln_2(xmid) for the two (bf16) weight gradients
        if rebuild:
            sched.before_write(h)
            ops.gelu_bf16(u, h, quick=self.quick_gelu)
            sched.before_write(a2)
            ops.layernorm_fwd(xmid, s.p(self._n(i, "ln_2.weight")), s.p(self._n(i, "ln_2.bias")), a2, *self._stats(2, i, M), M, d)
        if c.wg_mode != "4":
            reads = (g0, dU) + ((h, a2) if rebuild else ()) + ((g0_8, dU8) if w8_now else ())
            sched.run(lambda: launch_wgrads(probs, M, "mlp", c.wg_mode, fp8), reads)
        cfc = s.copies[self._n(i, "mlp.c_fc.weight")]
        if dU_has_q8 and cfc.wb8 is not None:
            ops.gemm_fp8(ops.EPI_BF16, dU8, dU_scale_inv, cfc.wb8, cfc.wb8s, c.dA, M=M, N=d, K=mlp, a_scale_scalar=True)
        else:
            ops.gemm(ops.NT, ops.EPI_BF16, dU, cfc.wb, c.dA, M=M, N=d, K=mlp)
        # LN2 backward accumulates into the residual gradient; its column sum is out_proj.bias' gradient
        g1, _ = c.ring.advance()
        sched.before_write(g1)
        self._ln_bwd(c, c.dA, xmid, self._stats(2, i, M), s.p(self._n(i, "ln_2.weight")), g0, g1,
                     g("ln_2.weight"), g("ln_2.bias"), g("attn.out_proj.bias"))
        return probs, ((g0, dU, h, a2) if self.recompute else (g0, dU))

    def _attn_bwd(self, i: int, c: _Bwd, mlp_probs, mlp_reads) -> None:
        """Attention branch of block i: xmid = x_in + out_proj(attn(in_proj(ln_1(x_in))))."""
        s, d, bf, p, sched = self.s, self.d, self.bufs, c.p, c.sched
        B, L, M = p.B, p.L, p.M
        g = lambda leaf: s.g(self._n(i, leaf))
        a1, qkv, o = self._act("a1", i, (M, d)), bf.get(f"qkv.{i}", (M, 3 * d), BF16), bf.get(f"o.{i}", (M, d), BF16)
        lse = bf.get(f"lse.{i}", (B, self.H, L), F32)
        dqkv = bf.get(f"dqkv.{i & 1}", (M, 3 * d), BF16)
        g1, _ = c.ring.current
        self._dgrad(c, ops.EPI_BF16, g1, self._n(i, "attn.out_proj.weight"), c.dO, N=d, K=d, have_q8=True)
        sched.before_write(dqkv)
        ops.attn_bwd(qkv, o, c.dO, lse, B, L, self.H, self.dh, self.causal, dqkv=dqkv, delta=c.delta)
        probs = [(g1, o, g("attn.out_proj.weight"), None, d, d), (dqkv, a1, g("attn.in_proj_weight"), g("attn.in_proj_bias"), 3 * d, d)]
        if self.recompute:          # rebuild a1 = ln_1(x_in) for the in_proj weight gradient
            sched.before_write(a1)
            ops.layernorm_fwd(p.x_in[i], s.p(self._n(i, "ln_1.weight")), s.p(self._n(i, "ln_1.bias")), a1, *self._stats(1, i, M), M, d)
        reads = (g1, dqkv, a1) if self.recompute else (g1, dqkv)
        if c.wg_mode == "4":        # all four weight gradients of the block in one launch
            sched.run(lambda: launch_wgrads(mlp_probs + probs, M, "block", "4"), reads + mlp_reads)
        else:                       # grouped, out_proj (9 tiles) no longer needs split-K 28 to fill the chip
            sched.run(lambda: launch_wgrads(probs, M, "attn", c.wg_mode), reads)
        ops.gemm(ops.NT, ops.EPI_BF16, dqkv, s.copies[self._n(i, "attn.in_proj_weight")].wb, c.dA, M=M, N=d, K=3 * d)
        # LN1 backward; its column sum is the previous block's c_proj.bias gradient
        prev_bias = s.g(self._n(i - 1, "mlp.c_proj.bias")) if i > self.floor else None    # block i - 1 locked: no gradient of its bias
        g2, g2_8 = c.ring.advance()
        sched.before_write(g2)
        t8n = None
        if c.w8 and i > 0:          # g2 is block i - 1's g0: its per-tensor e4m3 copy, in the ring slot beside it
            sched.before_write(g2_8)
            sc, _, amax = self.scales.g(i - 1)
            t8n = (g2_8, sc, amax)
        self._ln_bwd(c, c.dA, p.x_in[i], self._stats(1, i, M), s.p(self._n(i, "ln_1.weight")), g1, g2,
                     g("ln_1.weight"), g("ln_1.bias"), prev_bias, last=(i == 0), t8=t8n)
        c.g_has_q8 = c.qg is not None
        c.g0_t8_ok = t8n is not None
