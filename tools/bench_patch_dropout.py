#!/usr/bin/env python3
"""Step time of BASELINE configs[1] (ViT-B-16-gene, local batch 256, one process, ClipLoss, eager step) with FLIP patch dropout
at p in {0, 0.5, 0.75}: 197, 99 and 50 tokens in the vision tower's training forward and backward.

Every measurement is a fresh child process (its own allocator, schedule trials and code-object loads), each under its own
``timeout``, chained with ``&&``: a child that faults or hangs ends the run and nothing else is started on the device.  The
children's JSON lines go to stdout and to profiles/patch_dropout_bench.txt.  Nothing is asserted: the expectation -- the
vision tower is > 99 % of the step's FLOPs and its GEMMs scale with the token count, attention faster than that, the stem,
the head, the second tower, the loss and the optimiser not at all, so roughly tokens-proportional -- is an expectation.

    python tools/bench_patch_dropout.py [--steps 20] [--warmup 15] [--fractions 0,0.5,0.75] [--out profiles/patch_dropout_bench.txt]"""
import argparse
import functools
import json
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(p: float, steps: int, warmup: int, batch: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, module, net, optim, patch_dropout, streams
    n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0, force_patch_dropout=p if p > 0 else None)
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
        functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000))

    class _T:
        max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
    m.trainer = _T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    rates = data.make_gene_rates(20000)
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(batch, 224, 20000, K=8, step=s, gene_rates=rates).items()}
               for s in range(2)]

    def step(i):
        with streams.chain_stream():
            loss = m.training_step(batches[i % 2], i)
            loss.backward(m.root_gradient(loss))
            opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
        return loss
    for i in range(warmup):          # past the side-stream schedule trials of the stack (towers.TransformerStack.OVERLAP_TRIAL_CALLS)
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        loss = step(warmup + i)
    e1.record()
    torch.cuda.synchronize()
    n_patch = n.cfg.vision.tokens - 1
    tokens = patch_dropout.num_keep(n_patch, p) + 1 if p > 0 else n_patch + 1
    print(json.dumps({"model": "ViT-B-16-gene", "batch": batch, "patch_dropout": p, "train_tokens": tokens,
                      "step_ms": round(e0.elapsed_time(e1) / steps, 3), "steps": steps, "warmup": warmup,
                      "loss": round(float(loss.detach()), 5), "side_stream": n.side_stream_choice().get("vision"),
                      "draws": n.patch_dropout_draw}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--fractions", default="0,0.5,0.75")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout_bench.txt"))
    ap.add_argument("--child", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.steps, args.warmup, args.batch)
        return
    me = os.path.abspath(__file__)
    cmds = [f"timeout -k 10 {args.timeout} {shlex.quote(sys.executable)} {shlex.quote(me)} --child {float(p)} --steps {args.steps} "
            f"--warmup {args.warmup} --batch {args.batch}" for p in args.fractions.split(",")]
    r = subprocess.run(" && ".join(cmds), shell=True, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    sys.stdout.write(r.stdout)
    base = None
    with open(args.out, "w") as f:
        f.write("# tools/bench_patch_dropout.py: eager training step, one fresh process per line; step_ms as measured, nothing asserted\n")
        for l in lines:
            rec = json.loads(l)
            base = rec if base is None and rec["patch_dropout"] == 0 else base
            if base is not None:
                rec["step_vs_p0"] = round(rec["step_ms"] / base["step_ms"], 3)
                rec["tokens_vs_p0"] = round(rec["train_tokens"] / base["train_tokens"], 3)
            f.write(json.dumps(rec) + "\n")
        if r.returncode != 0:
            f.write(f"# stopped: a child ended with status {r.returncode}; nothing was started after it\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
