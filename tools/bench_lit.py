#!/usr/bin/env python3
"""Timing of the training step with a locked image tower (LiT) beside the unlocked step: BASELINE configs[1] (ViT-B-16-gene,
batch 256, ClipLoss, FusedAdamW, clip 1.0) unlocked and with ``lock_image_tower(unlocked_groups)`` for 0, 2 and 7.

  * every variant is built once and the variants take turns (``--rounds`` rounds of ``--steps`` steps each, device events,
    warmed): drift of the box shows as a difference between the rounds of one variant, not between the variants;
  * per variant: ms per step of every round, the best round's share of the unlocked step, peak device memory the variant added
    (torch's allocator, from building the net to the end of its warm-up) and the trainable floats;
  * for ``unlocked_groups=0``: an ``encode_image`` forward and the step of the second tower alone (the same module step with
    the vision forward replaced by its last features), whose sum is what the locked step should cost.

``--only unlocked`` times the unlocked step alone and ``--root DIR`` imports the package from another checkout: the parent
commit's unlocked step on the same box is the yardstick for "no regression".

Writes profiles/lit_bench.txt (one JSON line per measurement; ``--append`` adds to it).  Recorded numbers, not assertions.

    python tools/bench_lit.py [--steps 20] [--warmup 15] [--rounds 3] [--only unlocked] [--root DIR] [--tag NAME]"""
import argparse
import functools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


class Variant:
    def __init__(self, name, unlocked, warmup):
        from spatial_clip_amd import data, losses, module, net, optim
        self.name = name
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        kw = {} if unlocked is None else dict(lock_image=True, lock_image_unlocked_groups=unlocked)
        self.net = n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0, **kw)
        self.m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
            functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000))

        class _T:
            max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
        self.m.trainer = _T()
        oc = self.m.configure_optimizers()
        self.opt, self.sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        rates = data.make_gene_rates(20000)
        self.batches = [{k: v.cuda() for k, v in data.synthetic_batch(256, 224, 20000, K=8, step=s, gene_rates=rates).items()}
                        for s in range(2)]
        self.i = 0
        self.run(warmup)
        torch.cuda.synchronize()
        self.peak_mib = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        st = n.store
        self.trainable = st.trainable_floats() if hasattr(st, "trainable_floats") else st.total
        self.total = st.total
        self.ms = []

    def step(self):
        from spatial_clip_amd import streams
        with streams.chain_stream():
            loss = self.m.training_step(self.batches[self.i % 2], self.i)
            loss.backward(self.m.root_gradient(loss))
            self.opt.step(grad_scale=1.0, max_norm=1.0)
            self.sched.step()
        self.i += 1
        return loss

    def run(self, steps):
        for _ in range(steps):
            loss = self.step()
        return loss

    def timed(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(steps)
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(round(e0.elapsed_time(e1) / steps, 3))


def timeit(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def parts_of_the_locked_step(v, steps):
    """encode_image alone, and the locked step with the vision forward replaced by the features it left last."""
    images = v.batches[0]["images"]
    fwd_ms = timeit(lambda: v.net.model.encode_image(images, normalize=True), steps)
    v.step()                                    # a training forward again: tower.f and the buffers of a training pass
    tower, real = v.net.vision, v.net.vision.forward
    tower.forward = lambda _images: tower.f
    try:
        second_ms = timeit(v.step, steps)
    finally:
        tower.forward = real
    return round(fwd_ms, 3), round(second_ms, 3)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="'unlocked': the unlocked step alone")
    ap.add_argument("--root", default=ROOT, help="checkout to import the package from")
    ap.add_argument("--tag", default="working tree")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lit_bench.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import spatial_clip_amd  # noqa: F401,E402
    emit({"tool": "tools/bench_lit.py", "tree": args.tag, "device": torch.cuda.get_device_name(0), "steps": args.steps,
          "warmup": args.warmup, "rounds": args.rounds, "model": "ViT-B-16-gene", "batch": 256,
          "timing": "device events, warmed, the variants taking turns in one process"})
    todo = [("unlocked", None)] if args.only == "unlocked" else [("unlocked", None), ("unlocked_groups=0", 0),
                                                                 ("unlocked_groups=2", 2), ("unlocked_groups=7", 7)]
    variants = [Variant(name, g, args.warmup) for name, g in todo]
    for _ in range(args.rounds):
        for v in variants:
            v.timed(args.steps)
    base = min(variants[0].ms)
    for v in variants:
        emit({"step": v.name, "tree": args.tag, "ms_per_round": v.ms, "ms": min(v.ms), "spread_ms": round(max(v.ms) - min(v.ms), 3),
              "share_of_unlocked": round(min(v.ms) / base, 3), "peak_mib": v.peak_mib, "trainable_floats": v.trainable,
              "flat_floats": v.total})
    for v in variants:
        if v.name == "unlocked_groups=0":
            fwd_ms, second_ms = parts_of_the_locked_step(v, args.steps)
            emit({"parts_of": v.name, "encode_image_ms": fwd_ms, "second_tower_step_ms": second_ms,
                  "sum_ms": round(fwd_ms + second_ms, 3), "locked_step_ms": min(v.ms),
                  "gap_ms": round(min(v.ms) - fwd_ms - second_ms, 3)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(LINES) + "\n")
