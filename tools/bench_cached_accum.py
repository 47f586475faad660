#!/usr/bin/env python3
"""Cost of cached-feature gradient accumulation (Trainer accum_freq) on BASELINE configs[1]
(ViT-B-16-gene, ClipLoss, one process, eager step, clip 1.0) at (B = 64, N = 4) and (B = 128, N = 2).

Legs, interleaved in one process and repeated; ms per optimiser step, HIP events:

    cached    one cached group: N caching forwards, the head at G = N * B, N x (forward + backward + fold), clip + AdamW
    plain_N   N plain optimiser steps at B      (the parent's code path: the baseline)
    plain_G   one plain optimiser step at N * B (what the cached group computes, with the activations of N * B pairs)
    fwdbwd    forward + loss + backward at B, no optimiser
    fwd       the caching forward at B alone
    head      the contrastive head alone at G
    folds     the N folds of a group alone
    step      clip + AdamW alone

The expectation, stated before anything was measured:

    cached  ~=  N * (fwdbwd + fwd) + head + folds + step

(``fwdbwd`` contains the head at B, which the cached group does not run: the sum overstates by N small heads.)  The file
reports measured / expected per case and the peak device memory of the three routes (``max_memory_allocated`` around one
step of each, taken in a fresh process in the order cached, plain_N, plain_G, before any larger buffer exists).  There is no
pass threshold.

One fresh child process per case, each under its own ``timeout``, chained with ``&&``: a child that faults or hangs ends the
run and nothing else is started on the device.

    python tools/bench_cached_accum.py [--reps 6] [--groups 3] [--warmup 12] [--out profiles/cached_accum_bench.txt]"""
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


def child(batch: int, freq: int, reps: int, groups: int, warmup: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import contrastive, data, losses, module, net, optim, streams
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
    acc = m.group_accumulator(freq)
    rates = data.make_gene_rates(20000)
    G = batch * freq
    micro = [{k: v.cuda() for k, v in data.synthetic_batch(batch, 224, 20000, K=8, step=s, gene_rates=rates).items()}
             for s in range(freq)]
    big = {k: torch.cat([b[k] for b in micro]) for k in micro[0]}

    def plain_step(b, i):
        with streams.chain_stream():
            loss = m.training_step(b, i)
            loss.backward(m.root_gradient(loss))
            opt.step(grad_scale=1.0, max_norm=1.0)
        sched.step()

    def cached(i):
        partial = acc.sumsq_partial()
        m.cached_group_step(micro, partial=partial)
        with streams.chain_stream():
            opt.step(grad_scale=1.0, max_norm=1.0, sumsq_partial=partial)
        sched.step()

    def plain_n(i):
        for k in range(freq):
            plain_step(micro[k], i)

    def plain_g(i):
        plain_step(big, i)

    def fwdbwd(i):
        with streams.chain_stream():
            loss = m.training_step(micro[i % freq], i)
            loss.backward(m.root_gradient(loss))

    def fwd(i):
        with streams.chain_stream():
            n.cache_features(micro[i % freq]["images"], micro[i % freq]["texts"])

    gen = torch.Generator(device="cuda").manual_seed(1)
    D = n.cfg.embed_dim
    f_i = torch.nn.functional.normalize(torch.randn(G, D, device="cuda", generator=gen), dim=-1)
    f_t = torch.nn.functional.normalize(torch.randn(G, D, device="cuda", generator=gen), dim=-1)
    scale = torch.full((1,), 14.285, device="cuda")

    def head(i):
        with streams.chain_stream():
            contrastive.contrastive_forward_backward(f_i, f_t, scale, mode="clip", want_recall=False, join_local=True)

    def folds(i):
        with streams.chain_stream():
            for k in range(freq):
                acc.fold(k == 0, k == freq - 1, partial=acc.sumsq_partial() if k == freq - 1 else None)

    def step(i):
        with streams.chain_stream():
            opt.step(grad_scale=1.0, max_norm=1.0)

    def peak(fn):
        n.store.wait_all()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn(0)
        n.store.wait_all()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() / 2 ** 20

    # peak memory first, smallest route first: no buffer of a larger batch exists yet
    peaks = {"cached": peak(cached), "plain_N": peak(plain_n), "plain_G": peak(plain_g)}

    def timed(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(count):
            fn(i)
        n.store.wait_all()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    for i in range(warmup):             # past the side-stream schedule trials of the stack, at both batch sizes
        plain_step(micro[i % freq], i)
    for i in range(4):
        plain_g(i)
        cached(i)
    legs = {"cached": (cached, groups), "plain_N": (plain_n, groups), "plain_G": (plain_g, groups), "fwdbwd": (fwdbwd, groups * freq),
            "fwd": (fwd, groups * freq), "head": (head, groups * 4), "folds": (folds, groups), "step": (step, groups)}
    ms = {k: [] for k in legs}
    for r in range(reps):               # interleaved
        for k, (fn, count) in legs.items():
            fn(0)                       # the leg's buffer shapes are current before it is timed
            ms[k].append(timed(fn, count))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    expected = freq * (med["fwdbwd"] + med["fwd"]) + med["head"] + med["folds"] + med["step"]
    rec = {"model": "ViT-B-16-gene", "batch": batch, "accum_freq": freq, "G": G, "params": n.store.total, "reps": reps,
           "groups_per_leg": groups, "warmup": warmup,
           "median_ms": {k: round(v, 3) for k, v in med.items()}, "spread_ms": {k: round(v, 3) for k, v in spread.items()},
           "expected_cached_ms": round(expected, 3), "measured_over_expected": round(med["cached"] / expected, 4),
           "cached_over_plain_N": round(med["cached"] / med["plain_N"], 4), "cached_over_plain_G": round(med["cached"] / med["plain_G"], 4),
           "pairs_per_s": {k: round(G / med[k] * 1e3, 1) for k in ("cached", "plain_N", "plain_G")},
           "peak_MiB": {k: round(v, 1) for k, v in peaks.items()}}
    print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--groups", type=int, default=3, help="optimiser steps per timed leg")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cached_accum_bench.txt"))
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
        f.write("# tools/bench_cached_accum.py: one cached group of N micro-batches of B (accum_freq = N) against N plain steps at B and\n"
                "# one plain step at N * B (same build, same process, legs interleaved); ms per optimiser step, HIP events.\n"
                "# expectation: cached ~= N * (fwdbwd + fwd) + head + folds + step; as measured, nothing tuned, no pass threshold\n")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                f.write(l + "\n")
        if r.returncode != 0:
            f.write(f"# stopped: a child ended with status {r.returncode}; nothing was started after it\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
