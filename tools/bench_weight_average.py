#!/usr/bin/env python3
"""What an averaged copy of the weights costs: the update kernel alone, then the whole configs[1] step with averaging off, every
step and every tenth step.

1. The kernel.  ``sc_weight_average`` (EMA, decay 0.999) and ``sc_swap_f32`` over the whole flat buffer of ``ViT-B-16-gene``
   (20000 genes).  Cold buffers: ``--pairs`` pairs of (average, weights) take turns, so that a launch finds nothing of its
   operands in the 256 MiB Infinity Cache (one pair is 2 x 387 MB).  Blocks of ``--launches`` launches, device events,
   ``--rounds`` rounds; reported: the median block (ms per launch) and bytes/s at 12 bytes per parameter (average and weights
   read, average written; the swap: 16) against the HBM peak of the MI355X.
2. The whole step.  configs[1] (ViT-B-16-gene, batch 256, ClipLoss, clip 1.0, FusedAdamW, eager, the update bucket by bucket
   behind the next forward) with ``WeightAverager`` absent, with ``update_every_n_steps=1`` and with 10: three nets built once,
   taking turns, ``--rounds`` rounds of ``--steps`` steps (a multiple of 10, so every round of the third variant holds the same
   number of updates).  ``exposed_ms`` of a variant is its median step minus the median step without averaging: what of the
   update the forward it runs behind does not hide.

Writes profiles/weight_average_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.

    python tools/bench_weight_average.py [--launches 20] [--rounds 7] [--steps 20] [--warmup 15] [--pairs 3] [--no-step]"""
import argparse
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12           # bytes/s, MI355X specification
ADAMW = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)       # configs/optimizer/adamw.yaml
AVG_BYTES, SWAP_BYTES = 12, 16
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def block(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernels(args):
    from spatial_clip_amd import model_configs as mc, ops, params
    dev = torch.device("cuda", 0)
    n = params.ParamStore(mc.get_model_config("ViT-B-16-gene", n_genes=20000), torch.device("cpu"), init=False).total
    gen = torch.Generator(device=dev).manual_seed(0)
    pairs = [(torch.randn(n, device=dev, generator=gen) * 0.02, torch.randn(n, device=dev, generator=gen) * 0.02)
             for _ in range(args.pairs)]

    def ema(k):
        avg, p = pairs[k % len(pairs)]
        ops.weight_average(avg, p, n, ops.WAVG_EMA, 0.999, 1.0 - 0.999)

    def swap(k):
        avg, p = pairs[k % len(pairs)]
        ops.swap_f32(avg, p, n)

    for name, fn, nbytes in (("sc_weight_average (ema)", ema, AVG_BYTES), ("sc_swap_f32", swap, SWAP_BYTES)):
        block(fn, args.launches)
        blocks = [block(fn, args.launches) for _ in range(args.rounds)]
        med = statistics.median(blocks)
        emit({"kernel": name, "model": "ViT-B-16-gene", "flat_floats": n, "buffers": f"cold: {len(pairs)} pairs taking turns",
              "launches_per_block": args.launches, "rounds": args.rounds, "ms_blocks": [round(x, 4) for x in blocks],
              "ms_median": round(med, 4), "spread_ms": round(max(blocks) - min(blocks), 4), "bytes_per_param": nbytes,
              "GBps": round(nbytes * n / med / 1e6, 1), "share_of_hbm_peak": round(nbytes * n / (med * 1e-3) / HBM_PEAK, 3)})
    del pairs
    torch.cuda.empty_cache()


class Variant:
    """One configs[1] module under FusedAdamW, with or without an averager; ``run`` is the eager training step."""

    def __init__(self, name, every, warmup):
        from spatial_clip_amd import data, losses, module, net, optim
        self.name, self.every = name, every
        self.net = n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
        self.m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), functools.partial(optim.FusedAdamW, **ADAMW),
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000))

        class _T:
            max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
        self.m.trainer = _T()
        oc = self.m.configure_optimizers()
        self.opt, self.sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        self.wa = None if every is None else optim.WeightAverager(n.store, decay=0.999, update_every_n_steps=every).attach(self.opt)
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


def whole_step(args, kernel_ms):
    os.environ["SC_ADAMW_BEHIND"] = "1"
    warmup = (args.warmup + 9) // 10 * 10       # whole tens: the every-10 variant is at the same phase in every round
    variants = [Variant("averaging off", None, warmup), Variant("update_every_n_steps=1", 1, warmup),
                Variant("update_every_n_steps=10", 10, warmup)]
    for _ in range(args.rounds):
        for v in variants:
            v.timed(args.steps)
    base = statistics.median(variants[0].ms)
    for v in variants:
        med = statistics.median(v.ms)
        rec = {"step": v.name, "model": "ViT-B-16-gene", "batch": 256, "form": "eager, update behind the forward",
               "steps_per_round": args.steps, "ms_per_round": v.ms, "ms_median": med, "spread_ms": round(max(v.ms) - min(v.ms), 3),
               "exposed_ms": round(med - base, 3)}
        if v.wa is not None:
            rec["n_averaged"] = v.wa.n_averaged
            rec["average_bytes"] = v.wa.avg.numel() * 4
            if kernel_ms:
                rec["kernel_alone_ms_per_step"] = round(kernel_ms / v.every, 4)
        emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_average_bench.txt"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 per block")
    if args.steps % 10:
        ap.error("--steps: a multiple of 10")
    sys.path.insert(0, ROOT)
    import spatial_clip_amd  # noqa: F401,E402
    if not torch.cuda.is_available():
        sys.exit("bench_weight_average.py measures on the GPU; none is available")
    emit({"tool": "tools/bench_weight_average.py", "device": torch.cuda.get_device_name(0),
          "timing": "device events, warmed, the variants taking turns in one process"})
    kernels(args)
    kernel_ms = next((json.loads(l)["ms_median"] for l in LINES if '"sc_weight_average (ema)"' in l), None)
    if not args.no_step:
        whole_step(args, kernel_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
