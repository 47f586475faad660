#!/usr/bin/env python3
"""Muon beside AdamW on configs[1] (ViT-B-16-gene, 20000 genes): the whole step, then the kernels of the update.

1. ``--parent-root DIR``: ``bench.py`` (FusedAdamW, no kernel of it changes) in child processes under this tree and under a
   checkout of the parent commit with its own library in DIR, taking turns, ``--pairs`` pairs.
2. The whole step.  configs[1] (batch 256, ClipLoss, clip 1.0, eager, the update behind the next forward) under ``FusedAdamW``
   (configs/optimizer/adamw.yaml) and under ``FusedMuon`` with open_clip's no-decay groups
   (experiment=vitb16_gene_b256_muon): two nets built once, taking turns, ``--rounds`` rounds of ``--steps`` steps.
3. The kernels of the Muon update on the model's flat buffer with the optimiser's own tables: ``sc_muon_momentum``,
   ``sc_muon_scale``, ``sc_muon_apply`` beside ``sc_adamw_step_groups``, and ``_before_pieces`` as a whole; the Newton-Schulz
   phase is what ``_before_pieces`` takes beyond the first two, reported with its launch count and as TFLOP/s against
   ``ns_steps * sum (4 m^2 n + 2 m^3)`` (1.52 TFLOP for this model; at the NT rate README.md states that is 1.7 ms), in
   total and for the matrices of each shape alone.

Writes profiles/muon_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.

    python tools/bench_muon.py [--launches 20] [--rounds 5] [--steps 20] [--warmup 15] [--parent-root DIR]"""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAMW = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)       # configs/optimizer/adamw.yaml
MUON = dict(lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True, ns_steps=5, adjust_lr_fn="match_rms_adamw",
            adamw_betas=(0.9, 0.98), adamw_eps=1e-6)                         # configs/optimizer/muon.yaml
NT_RATE = 0.89e15           # FLOP/s: the NT GEMM rate README.md states for this chip (873 - 905 TFLOP/s)
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def block(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def ns_flops(shapes, steps):
    """ns_steps * sum over the matrices of (4 m^2 n + 2 m^3), m / n the smaller / larger dimension."""
    return steps * sum(4 * min(r, c) ** 2 * max(r, c) + 2 * min(r, c) ** 3 for r, c in shapes)


class Variant:
    """One configs[1] module with its optimiser; ``run`` is the eager training step of GraphedTrainStep.eager."""

    def __init__(self, name, optimizer_cfg, warmup, param_groups=None):
        from spatial_clip_amd import data, losses, module, net, optim
        self.name = name
        self.net = n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
        self.m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), optimizer_cfg,
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000), param_groups=param_groups)

        class _T:
            max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
        self.m.trainer = _T()
        oc = self.m.configure_optimizers()
        self.opt, self.sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        rates = data.make_gene_rates(20000)
        self.batches = [{k: v.cuda() for k, v in data.synthetic_batch(256, 224, 20000, K=8, step=s, gene_rates=rates).items()}
                        for s in range(2)]
        self.i, self.ms = 0, []
        self.run(warmup)
        torch.cuda.synchronize()

    def run(self, steps):
        from spatial_clip_amd import streams
        for _ in range(steps):
            with streams.chain_stream():
                loss = self.m.training_step(self.batches[self.i % 2], self.i)
                loss.backward(self.m.root_gradient(loss))
                self.opt.step(grad_scale=1.0, max_norm=1.0)
                self.sched.step()
            self.i += 1

    def timed(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(steps)
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(round(e0.elapsed_time(e1) / steps, 3))


def update_kernels(args, v):
    """The streaming kernels of the Muon step and the whole ``_before_pieces`` on the optimiser's own buffers and tables."""
    from spatial_clip_amd import ops
    opt, st = v.opt, v.opt.store
    n = st.total
    n_mu = len(opt.muon_names)
    m, vv = opt._moments(0, 0, n)
    g = opt.param_groups[0]
    clip = opt.norm_clip

    def momentum():
        ops.muon_momentum(st.grad, m, n, opt.slot_tensor, opt.tensor_info, n_mu, 0, opt.momentum, opt.nesterov, 1.0, clip, opt.x1,
                          opt.slot_sums, opt.compact_slots)

    def scale():
        ops.muon_scale(opt.slot_sums, n // 64, opt.tensor_info, n_mu, opt.muon_eps, opt.x1, opt.x0, opt.norms, opt.compact_slots)

    def apply():
        ops.muon_apply(st.master, st.grad, m, vv, n, opt.chunk_group, opt.slot_tensor, opt.tensor_info, opt.ratio, n_mu, 0, opt._obuf(),
                       opt.group_hyper, len(opt.param_groups), g["betas"][0], g["betas"][1], g["eps"], 1.0, clip, st.master_bf16,
                       opt.compact_slots)

    def adamw():
        ops.adamw_step_groups(st.master, st.grad, m, vv, n, opt.chunk_group, opt.group_hyper, len(opt.param_groups), g["betas"][0],
                              g["betas"][1], g["eps"], 1.0, clip, st.master_bf16)

    def before_pieces():
        opt._before_pieces(1.0, clip, None)

    st.wait_all()
    opt._refresh_group_hyper()          # the table of the forms that launch on the stream of the step
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("sc_muon_momentum", momentum), ("sc_muon_scale", scale), ("sc_muon_apply", apply),
                     ("sc_adamw_step_groups", adamw), ("before_pieces (momentum + scale + Newton-Schulz)", before_pieces)):
        block(fn, args.launches)
        res[name] = round(statistics.median(block(fn, args.launches) for _ in range(3)), 4)
    per_shape = {}
    for shape in sorted(set(opt.muon_shapes)):          # the Newton-Schulz iterations of one shape's matrices alone
        members = [ti for ti, sh in enumerate(opt.muon_shapes) if sh == shape]

        def ns(members=members):
            for ti in members:
                opt._newton_schulz(ti)
        block(ns, args.launches)
        ms = statistics.median(block(ns, args.launches) for _ in range(3))
        fl_s = ns_flops([shape] * len(members), opt.ns_steps)
        per_shape[f"{shape[0]}x{shape[1]}"] = {"matrices": len(members), "launches": 5 * opt.ns_steps * len(members), "ms": round(ms, 4),
                                               "GFLOP": round(fl_s / 1e9, 2), "TFLOPs": round(fl_s / ms / 1e9, 1),
                                               "floor_ms_at_the_NT_rate_of_README": round(fl_s / NT_RATE * 1e3, 4)}
    emit({"newton_schulz_per_shape": per_shape, "route": "matrix by matrix: 3 sc_gemm_bf16 + 2 sc_muon_axpby per iteration"})
    scratch = sum(t.numel() * t.element_size() for t in (opt.x0, opt.x1, opt.gbuf, opt.pbuf, opt.acc, opt.slot_sums))
    ns_ms = res["before_pieces (momentum + scale + Newton-Schulz)"] - res["sc_muon_momentum"] - res["sc_muon_scale"]
    fl = ns_flops(opt.muon_shapes, opt.ns_steps)
    emit({"update_kernels_ms": res, "model": "ViT-B-16-gene", "flat_floats": n, "muon_tensors": n_mu,
          "muon_floats": 64 * opt.compact_slots, "shapes": {f"{r}x{c}": opt.muon_shapes.count((r, c)) for r, c in sorted(set(opt.muon_shapes))},
          "newton_schulz_ms": round(ns_ms, 3), "newton_schulz_launches_per_step": 5 * opt.ns_steps * n_mu,
          "newton_schulz_TFLOP": round(fl / 1e12, 3), "newton_schulz_TFLOPs": round(fl / ns_ms / 1e9, 1),
          "floor_ms_at_the_NT_rate_of_README": round(fl / NT_RATE * 1e3, 3), "scratch_bytes": scratch,
          "launches_per_block": args.launches})


def whole_step(args):
    from spatial_clip_amd import optim
    os.environ["SC_ADAMW_BEHIND"] = "1"
    variants = [Variant("FusedAdamW", functools.partial(optim.FusedAdamW, **ADAMW), args.warmup),
                Variant("FusedMuon", functools.partial(optim.FusedMuon, **MUON), args.warmup, {"no_decay": "open_clip"})]
    for _ in range(args.rounds):
        for v in variants:
            v.timed(args.steps)
    base = statistics.median(variants[0].ms)
    for v in variants:
        state = sum(t.numel() * t.element_size() for t in v.opt._state())
        emit({"step": v.name, "model": "ViT-B-16-gene", "batch": 256, "form": "eager, update behind the forward",
              "groups": len(v.opt.param_groups), "ms_per_round": v.ms, "ms_median": statistics.median(v.ms),
              "spread_ms": round(max(v.ms) - min(v.ms), 3), "share_of_adamw": round(statistics.median(v.ms) / base, 4),
              "optimizer_state_bytes": state, "state_bytes_per_param": round(state / v.opt.store.total, 3)})
    emit({"step": "summary", "muon_minus_adamw_ms": round(statistics.median(variants[1].ms) - base, 3)})
    update_kernels(args, variants[1])


def parent_ab(args):
    """bench.py in fresh child processes, this tree and the parent's checkout taking turns."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "40", "--warmup", "10", "--no-cpu-baseline", "--no-kernel-events",
           "--no-loss-delta", "--no-comm-probe"]
    env = dict(os.environ, SC_OVERLAP="1", SC_GRAPH="off")
    env.pop("SC_HIP_LIB", None)
    ms = {"this": [], "parent": []}
    for k in range(args.pairs):
        for who in (("this", "parent") if k % 2 == 0 else ("parent", "this")):
            r = subprocess.run(cmd, cwd=ROOT if who == "this" else args.parent_root, env=env, capture_output=True, text=True, timeout=600)
            line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{") and "ms_per_step" in ln), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"bench.py failed under {who}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            ms[who].append(json.loads(line)["ms_per_step"])
            print(who, ms[who][-1], flush=True)
    emit({"bench.py": "FusedAdamW, configs[1], schedule pinned (SC_OVERLAP=1, graph off), 40 steps after 10, fresh processes taking turns",
          "this_ms_per_step": ms["this"], "parent_ms_per_step": ms["parent"], "this_median": statistics.median(ms["this"]),
          "parent_median": statistics.median(ms["parent"])})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "muon_bench.txt"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 per block")
    sys.path.insert(0, ROOT)
    import spatial_clip_amd  # noqa: F401,E402
    if not torch.cuda.is_available():
        sys.exit("bench_muon.py measures on the GPU; none is available")
    emit({"tool": "tools/bench_muon.py", "device": torch.cuda.get_device_name(0),
          "timing": "device events, warmed, the two sides taking turns in one process; bench.py in fresh processes"})
    if args.parent_root:
        parent_ab(args)
    whole_step(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
