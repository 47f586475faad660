#!/usr/bin/env python3
"""The grouped AdamW launch beside the un-grouped one, on the flat buffers of BASELINE configs[1] (ViT-B-16-gene, 20000 genes).

1. Kernels.  ``sc_adamw_step`` (A) and ``sc_adamw_step_groups`` with open_clip's two groups (B) over the whole flat buffer,
   both with the bf16 mirror and a clip coefficient, on buffers of their own (the same values for both).  Both are warmed; then
   blocks of ``--launches`` launches each are timed with device events in the order A, A, B, ``--rounds`` times, in one
   process.  Reported: the median block of A and of B (ms per launch), the A/A spread -- the range (max - min) of all A
   blocks, i.e. what two measurements of the SAME kernel differ by in this run -- and the achieved bytes/s of both medians
   against the HBM peak of the MI355X (8.0 TB/s specified; a float4 copy reaches 6.29 TB/s).  Bytes per launch: 30 per float
   (p, g, m, v read; p, m, v and the bf16 mirror written), plus one table byte per 64 floats for B.
   ``accepted``: median(B) <= median(A) * (1 + table byte share) + A/A spread.
2. The whole step.  configs[1] (batch 256, ClipLoss, clip 1.0, eager, the update bucket by bucket behind the next forward) with
   ``param_groups=None`` -- twice, two nets: what two builds of the SAME step differ by -- and with
   ``{"no_decay": "open_clip"}``: three nets built once, taking turns, ``--rounds`` rounds of ``--steps`` steps.

Writes profiles/adamw_groups_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.

    python tools/bench_adamw_groups.py [--launches 20] [--rounds 7] [--steps 20] [--warmup 15] [--no-step]"""
import argparse
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12           # bytes/s, MI355X specification
HBM_COPY = 6.29e12          # bytes/s, what a float4 copy reaches
B1, B2, EPS, LR, WD = 0.9, 0.98, 1e-6, 1e-3, 0.1
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


def kernels(args):
    from spatial_clip_amd import model_configs as mc, ops, optim, params
    dev = torch.device("cuda", 0)
    store = params.ParamStore(mc.get_model_config("ViT-B-16-gene", n_genes=20000), dev, init=False)
    for p in store.params.values():
        p._sc_store = store
    n = store.total
    groups = optim.open_clip_param_groups(store.params.items(), WD)
    table = optim.slot_table(store, [g["param_names"] for g in groups]).to(dev)
    no_decay_floats = int((table == 0).sum()) * 64
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen) * 0.02
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    mirror = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    nc = torch.zeros(2, device=dev)
    ops.grad_norm(g, n, 1.0, 1.0, nc)
    host = torch.zeros(2 + 2 * len(groups))
    ops.adamw_groups_hyper_host([LR] * len(groups), [gr.get("weight_decay", WD) for gr in groups], B1, B2, 10, host)
    hyper = host.to(dev)

    def a():
        ops.adamw_step(p, g, m, v, n, LR, B1, B2, EPS, WD, 10, 1.0, nc, mirror)

    def b():
        ops.adamw_step_groups(p, g, m, v, n, table, hyper, len(groups), B1, B2, EPS, 1.0, nc, mirror)

    for fn in (a, b):
        block(fn, args.launches)
    blocks_a, blocks_b = [], []
    for _ in range(args.rounds):
        blocks_a.append(block(a, args.launches))
        blocks_a.append(block(a, args.launches))
        blocks_b.append(block(b, args.launches))
    med_a, med_b = statistics.median(blocks_a), statistics.median(blocks_b)
    spread = max(blocks_a) - min(blocks_a)
    bytes_a, bytes_b = 30 * n, 30 * n + n // 64
    share = (n // 64) / bytes_a
    emit({"kernels": "sc_adamw_step (A) vs sc_adamw_step_groups (B)", "flat_floats": n, "groups": len(groups),
          "no_decay_floats": no_decay_floats, "launches_per_block": args.launches, "rounds": args.rounds, "order": "A A B",
          "A_ms_blocks": [round(x, 4) for x in blocks_a], "B_ms_blocks": [round(x, 4) for x in blocks_b],
          "A_ms_median": round(med_a, 4), "B_ms_median": round(med_b, 4), "AA_spread_ms": round(spread, 4),
          "B_minus_A_ms": round(med_b - med_a, 4), "table_byte_share": round(share, 6),
          "A_TBps": round(bytes_a / med_a / 1e9, 3), "B_TBps": round(bytes_b / med_b / 1e9, 3),
          "A_share_of_hbm_peak": round(bytes_a / (med_a * 1e-3) / HBM_PEAK, 3),
          "B_share_of_hbm_peak": round(bytes_b / (med_b * 1e-3) / HBM_PEAK, 3),
          "B_share_of_float4_copy": round(bytes_b / (med_b * 1e-3) / HBM_COPY, 3),
          "accepted": bool(med_b <= med_a * (1 + share) + spread)})


class Variant:
    """One configs[1] module with its optimiser; ``step`` is the eager training step of GraphedTrainStep.eager."""

    def __init__(self, name, param_groups, warmup):
        from spatial_clip_amd import data, losses, module, net, optim
        self.name = name
        self.net = n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
        self.m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
            functools.partial(optim.FusedAdamW, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD),
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


def whole_step(args):
    os.environ["SC_ADAMW_BEHIND"] = "1"
    variants = [Variant("param_groups=None", None, args.warmup), Variant("param_groups=None (second net)", None, args.warmup),
                Variant("no_decay=open_clip", {"no_decay": "open_clip"}, args.warmup)]
    for _ in range(args.rounds):
        for v in variants:
            v.timed(args.steps)
    base = statistics.median(variants[0].ms)
    for v in variants:
        emit({"step": v.name, "model": "ViT-B-16-gene", "batch": 256, "form": "eager, update behind the forward",
              "groups": len(v.opt.param_groups), "ms_per_round": v.ms, "ms_median": statistics.median(v.ms),
              "spread_ms": round(max(v.ms) - min(v.ms), 3), "share_of_ungrouped": round(statistics.median(v.ms) / base, 4)})
    meds = [statistics.median(v.ms) for v in variants]
    emit({"step": "summary", "AA_ms": round(abs(meds[1] - meds[0]), 3),
          "grouped_minus_ungrouped_ms": round(meds[2] - min(meds[0], meds[1]), 3),
          "grouped_minus_slower_ungrouped_ms": round(meds[2] - max(meds[0], meds[1]), 3)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_groups_bench.txt"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 per block")
    sys.path.insert(0, ROOT)
    import spatial_clip_amd  # noqa: F401,E402
    if not torch.cuda.is_available():
        sys.exit("bench_adamw_groups.py measures on the GPU; none is available")
    emit({"tool": "tools/bench_adamw_groups.py", "device": torch.cuda.get_device_name(0),
          "timing": "device events, warmed, the variants taking turns in one process"})
    kernels(args)
    if not args.no_step:
        torch.cuda.empty_cache()
        whole_step(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
