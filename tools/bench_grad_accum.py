#!/usr/bin/env python3
"""Cost of gradient accumulation on BASELINE configs[1] (ViT-B-16-gene, ClipLoss, one process, eager step, clip 1.0): one
optimiser step from a group of N micro-batches (``optim.GradAccumulator``: a fold per micro-batch, clip and AdamW once) at
(B = 64, N = 4) and (B = 128, N = 2), against N plain optimiser steps at the same B -- the N = 1 path, which gradient
accumulation leaves untouched, on the same build.

The expectation comes from bytes: a fold moves 12 bytes per parameter per micro-batch, every non-final micro-batch skips AdamW's
30, so a group of N should cost no more than N plain steps.  Accepted when

    median t(group of N)  <=  median N * t(plain step)  +  spread of the plain legs (max - min over this session's repeats)

and when it does not hold the numbers stay as measured and the line says which term is over: the fold time (HIP events around
the fold launches of a group) against the clip + AdamW launches skipped by the non-final micro-batches (HIP events around the
plain ``opt.step``: the sum-of-squares read, its final and AdamW; N - 1 of them).  The group's last step also skips the
sum-of-squares read (``sumsq_partial``); that saving is not in the term.

One fresh child process per batch size, each under its own ``timeout``, chained with ``&&``: a child that faults or hangs ends
the run and nothing else is started on the device.  Inside a child the two legs are interleaved and repeated.

    python tools/bench_grad_accum.py [--reps 6] [--groups 5] [--warmup 16] [--out profiles/grad_accum_bench.txt]"""
import argparse
import functools
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((64, 4), (128, 2))


def child(batch: int, every: int, reps: int, groups: int, warmup: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, module, net, optim, streams
    n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000))

    class _T:
        max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
    m.trainer = _T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    acc = optim.GradAccumulator(n.store, every)
    rates = data.make_gene_rates(20000)
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(batch, 224, 20000, K=8, step=s, gene_rates=rates).items()}
               for s in range(every)]

    def plain(i):                       # what Trainer.fit runs per batch at accumulate_grad_batches = 1
        with streams.chain_stream():
            loss = m.training_step(batches[i % every], i)
            loss.backward(m.root_gradient(loss))
            opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()

    def group(i):                       # what it runs per group of `every` batches
        for k in range(every):
            first, last = k == 0, k == every - 1
            with streams.chain_stream():
                loss = m.training_step(batches[k], i)
                loss.backward(m.root_gradient(loss))
                partial = acc.sumsq_partial() if last else None
                acc.fold(first, last, partial=partial)
                if last:
                    opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
        sched.step()

    def timed(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(count):
            fn(i)
        n.store.wait_all()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for i in range(warmup):             # past the side-stream schedule trials of the stack
        plain(i)
    group(0)
    plain_ms, group_ms = [], []
    for r in range(reps):               # interleaved legs; both in "ms per optimiser-step-of-a-group" (= N plain steps)
        plain_ms.append(timed(plain, groups * every) / groups)
        group_ms.append(timed(group, groups) / groups)
    # the two terms of the expectation, each alone on the device
    fold_ms = []
    for r in range(5):
        def folds(_):
            for k in range(every):
                acc.fold(k == 0, k == every - 1, partial=acc.sumsq_partial() if k == every - 1 else None)
        fold_ms.append(timed(folds, 1))
    step_ms = [timed(lambda _: opt.step(grad_scale=1.0, max_norm=1.0), 1) for r in range(5)]      # clip (full read) + AdamW
    spread = max(plain_ms) - min(plain_ms)
    med_plain, med_group = statistics.median(plain_ms), statistics.median(group_ms)
    fold, saved = statistics.median(fold_ms), statistics.median(step_ms) * (every - 1)
    holds = med_group <= med_plain + spread
    rec = {"model": "ViT-B-16-gene", "batch": batch, "accumulate_grad_batches": every, "params": n.store.total,
           "reps": reps, "groups_per_leg": groups, "warmup": warmup,
           "plain_ms_per_N_steps": [round(x, 3) for x in plain_ms], "group_ms": [round(x, 3) for x in group_ms],
           "median_plain_ms": round(med_plain, 3), "median_group_ms": round(med_group, 3), "plain_spread_ms": round(spread, 3),
           "folds_per_group_ms": round(fold, 3), "clip_adamw_skipped_per_group_ms": round(saved, 3),
           "fold_GBps": round(12e-6 * n.store.total * every / max(fold, 1e-9) - 4e-6 * n.store.total / max(fold, 1e-9), 1),
           "expectation_holds": bool(holds)}
    if not holds:
        rec["over"] = ("the folds cost more than the clip + AdamW launches the non-final micro-batches skip" if fold > saved else
                       "neither term explains it: folds are cheaper than the clip + AdamW launches skipped; the rest of the group is slower")
    print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--groups", type=int, default=5, help="groups (and groups x N plain steps) per timed leg")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_bench.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        b, e = (int(x) for x in args.child.split(","))
        child(b, e, args.reps, args.groups, args.warmup)
        return
    me = os.path.abspath(__file__)
    cmds = [f"timeout -k 10 {args.timeout} {shlex.quote(sys.executable)} {shlex.quote(me)} --child {b},{e} --reps {args.reps} "
            f"--groups {args.groups} --warmup {args.warmup}" for b, e in CASES]
    r = subprocess.run(" && ".join(cmds), shell=True, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    with open(args.out, "w") as f:
        f.write("# tools/bench_grad_accum.py: one optimiser step from a group of N micro-batches against N plain steps at the same\n"
                "# batch size (same build, same process, legs interleaved); ms per group, HIP events; as measured, nothing tuned\n")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                f.write(l + "\n")
        if r.returncode != 0:
            f.write(f"# stopped: a child ended with status {r.returncode}; nothing was started after it\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
