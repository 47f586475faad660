#!/usr/bin/env python3
"""Token mean pooling (sc_token_pool_fwd / sc_token_pool_bwd) beside what it stands next to, and the step of an average-pooled
tower beside the class-token tower.

Kernels, bf16 rows, at ViT-B/16 (B 256, L 197, d 768) and ViT-L/14 (B 256, L 257, d 1024):
  * forward: ``token_pool_fwd`` beside ``layernorm_fwd`` over the same rows (reads the same bytes and writes them again: twice
    the traffic).  THE BAR: the pooling forward must not take longer than that LayerNorm.
  * backward: ``token_pool_bwd`` (fp32 + bf16 residual gradient, every element written) beside the two ``zero_()`` calls on the
    same buffers that the non-class-token path issued in its place.
Method: one process; every kernel works on a ring of operand sets larger than the last-level caches together (cold operands);
HIP events around ``--calls`` back-to-back launches; the kernels of a pair alternate over ``--rounds`` rounds; median and
minimum per call, and the bytes the algorithm needs over the median.

Step: ``ViT-L-14-gene`` against the same model with the CLIPA vision overrides (no_ln_pre, pool_type avg,
final_ln_after_pool) at one batch size, eager step, one fresh process each.  Recorded, not judged: the average-pooled tower
loses the class-token-only last block by construction.

Every child runs under its own ``timeout``, chained with ``&&``: a child that faults or hangs ends the run.

    python tools/bench_pool.py [--batch 128] [--steps 10] [--warmup 15] [--out profiles/token_pool_bench.txt]"""
import argparse
import functools
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("ViT-B/16", 256, 197, 768), ("ViT-L/14", 256, 257, 1024))
CLIPA = {"no_ln_pre": True, "pool_type": "avg", "final_ln_after_pool": True}


def kernels(rounds: int, calls: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    dev = "cuda"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls          # us per call

    for name, B, L, d in SHAPES:
        M = B * L
        ring = max(3, -(-(768 << 20) // (M * d * 2)))          # >= 768 MB of bf16 rows in the ring
        xs = [torch.randn(M, d, device=dev).to(torch.bfloat16) for _ in range(ring)]
        gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
        y = [torch.empty(M, d, dtype=torch.bfloat16, device=dev) for _ in range(ring)]
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        pooled = torch.empty(B, d, device=dev)
        dm = torch.randn(B, d, device=dev)
        bring = max(3, -(-(768 << 20) // (M * d * 6)))
        df = [torch.empty(M, d, device=dev) for _ in range(bring)]
        db = [torch.empty(M, d, dtype=torch.bfloat16, device=dev) for _ in range(bring)]
        pairs = {
            "token_pool_fwd": (lambda i: ops.token_pool_fwd(xs[i % ring], B, L, 1, d, mean_f32=pooled), M * d * 2 + B * d * 4),
            "layernorm_fwd": (lambda i: ops.layernorm_fwd(xs[i % ring], gamma, beta, y[i % ring], mean, rstd, M, d), M * d * 4),
            "token_pool_bwd": (lambda i: ops.token_pool_bwd(dm, B, L, 1, d, dx_f32=df[i % bring], dx_bf16=db[i % bring]), M * d * 6),
            "two_zero_": (lambda i: (df[i % bring].zero_(), db[i % bring].zero_()), M * d * 6),
        }
        for fn, _ in pairs.values():          # warm up: code objects, allocator
            timed(fn)
        us = {k: [] for k in pairs}
        for _ in range(rounds):               # the kernels alternate round by round
            for k, (fn, _) in pairs.items():
                us[k].append(timed(fn))
        for k, (_, nbytes) in pairs.items():
            med = statistics.median(us[k])
            print(json.dumps({"kernel": k, "shape": name, "B": B, "L": L, "d": d, "rows": "bf16", "us_median": round(med, 2),
                              "us_min": round(min(us[k]), 2), "bytes": nbytes, "TB_per_s": round(nbytes / med * 1e-6, 3),
                              "rounds": rounds, "calls_per_round": calls}), flush=True)
        del xs, y, df, db
        torch.cuda.empty_cache()


def step_child(clipa: bool, steps: int, warmup: int, batch: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, module, net, optim, streams
    n = net.SpatialClipNet("ViT-L-14-gene", None, n_genes=20000, seed=0, vision_cfg=CLIPA if clipa else None)
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
    for i in range(warmup):          # past the side-stream schedule trials of the stack
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        loss = step(warmup + i)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"model": "ViT-L-14-gene", "vision_cfg": CLIPA if clipa else {}, "batch": batch,
                      "cls_only_last": n.vision.stack.cls_only_last, "step_ms": round(e0.elapsed_time(e1) / steps, 3),
                      "steps": steps, "warmup": warmup, "loss": round(float(loss.detach()), 5),
                      "side_stream": n.side_stream_choice().get("vision")}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_pool_bench.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "kernels":
        kernels(args.rounds, args.calls)
        return
    if args.child in ("tok", "clipa"):
        step_child(args.child == "clipa", args.steps, args.warmup, args.batch)
        return
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))}"
    tail = f"--rounds {args.rounds} --calls {args.calls} --steps {args.steps} --warmup {args.warmup} --batch {args.batch}"
    cmds = [f"timeout -k 10 {args.timeout} {me} --child {c} {tail}" for c in ("kernels", "tok", "clipa")]
    r = subprocess.run(" && ".join(cmds), shell=True, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    with open(args.out, "w") as f:
        f.write("# tools/bench_pool.py on one MI355X: cold operands (ring > last-level caches), HIP events, interleaved rounds in one\n"
                "# process for the kernels; one fresh process per training-step line.  Measured on one box, one run.\n")
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
        by = {(rec.get("kernel"), rec.get("shape")): rec for rec in recs if "kernel" in rec}
        for name, *_ in SHAPES:
            a, b = by.get(("token_pool_fwd", name)), by.get(("layernorm_fwd", name))
            if a and b:
                ok = a["us_median"] <= b["us_median"]
                f.write(f"# {name}: token_pool_fwd {a['us_median']} us vs layernorm_fwd {b['us_median']} us on the same rows: "
                        f"the bar (pool <= LayerNorm) is {'MET' if ok else 'MISSED'}\n")
            a, b = by.get(("token_pool_bwd", name)), by.get(("two_zero_", name))
            if a and b:
                f.write(f"# {name}: token_pool_bwd {a['us_median']} us vs the two zero_() it replaces {b['us_median']} us\n")
        st = [rec for rec in recs if "step_ms" in rec]
        if len(st) == 2:
            f.write(f"# step: class-token tower {st[0]['step_ms']} ms, CLIPA (average-pooled, full-width last block) "
                    f"{st[1]['step_ms']} ms = x{st[1]['step_ms'] / st[0]['step_ms']:.3f} (recorded, not judged)\n")
        if r.returncode != 0:
            f.write(f"# stopped: a child ended with status {r.returncode}; nothing was started after it\n")
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
