#!/usr/bin/env python3
"""Timing of the distillation head beside the clip head, and of the training step with and without a frozen teacher.

  * the head alone at (B, G, D, D_t) = (256, 256, 512, 768) and (256, 2048, 512, 768): ClipLoss head and distill head
    alternating in one process, warmed, device-event timings; plus the distill head's rows pass (sc_distill_loss) alone;
  * the ViT-B-16-gene step at batch 256 with ClipLoss and with DistillClipLoss + a ViT-L-14-gene teacher (alternating), beside
    the teacher's no_grad forward timed on its own.

Writes profiles/distill_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.  Run on the GPU box:

    python tools/bench_distill.py [--steps 20] [--warmup 5] [--no-step] [--out profiles/distill_bench.txt]"""
import argparse
import functools
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spatial_clip_amd  # noqa: F401,E402
from spatial_clip_amd import contrastive as C, ops  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def timeit(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def heads(B, G, D, Dt):
    W = G // B
    r = W // 2
    g = torch.Generator(device="cuda").manual_seed(0)
    unit = functools.partial(torch.nn.functional.normalize, dim=-1)
    img = unit(torch.randn(G, D, device="cuda", generator=g))
    txt = unit(img + 0.7 * torch.randn(G, D, device="cuda", generator=g))
    timg = unit(torch.randn(G, Dt, device="cuda", generator=g))
    ttxt = unit(timg + 0.4 * torch.randn(G, Dt, device="cuda", generator=g))
    sl = slice(r * B, (r + 1) * B)
    fi, ft, ti, tt = (x[sl].contiguous() for x in (img, txt, timg, ttxt))
    s, st = torch.tensor(14.3, device="cuda"), torch.tensor(50.0, device="cuda")
    if W == 1:
        clip = lambda: C.contrastive_forward_backward(fi, ft, s, mode="clip", join_local=True, want_recall=False)
        dist = lambda: C.distill_forward_backward(fi, ft, s, ti, tt, st, join_local=True)
    else:
        clip = lambda: C.contrastive_forward_backward(fi, ft, s, mode="clip", all_image=img, all_text=txt, rank=r,
                                                      want_recall=False)
        dist = lambda: C.distill_forward_backward(fi, ft, s, ti, tt, st, all_image=img, all_text=txt, dist_all_image=timg,
                                                  dist_all_text=ttxt, rank=r)
    ms = {"clip": [], "distill": []}
    for _ in range(2):                      # alternating: drift shows as a difference between the pairs
        ms["clip"].append(timeit(clip))
        ms["distill"].append(timeit(dist))
    z_s, z_t = torch.randn(2, B, G, device="cuda") * 0.2, torch.randn(2, B, G, device="cuda") * 0.2
    w_s, w_t = torch.empty_like(z_s), torch.empty_like(z_t)
    rowpart, lo, gs = torch.empty(2 * B, 4, device="cuda"), torch.empty(4, device="cuda"), torch.empty(2, device="cuda")

    def rows():          # the pass overwrites its inputs: restore them (two D2D copies, timed separately below)
        w_s.copy_(z_s); w_t.copy_(z_t)
        ops.distill_loss(w_s, w_t, B, G, r * B, s.view(1), st.view(1), rowpart, lo, gs[:1], gs[1:])

    def copies():
        w_s.copy_(z_s); w_t.copy_(z_t)
    ms_rows = timeit(rows) - timeit(copies)
    emit({"head": [B, G, D, Dt], "clip_head_ms": [round(x, 4) for x in ms["clip"]],
          "distill_head_ms": [round(x, 4) for x in ms["distill"]],
          "ratio": round(min(ms["distill"]) / min(ms["clip"]), 3), "distill_rows_pass_us": round(ms_rows * 1e3, 1),
          "rows_path": "resident" if G <= ops.distill_resident_max_g() else "reread"})


def step_time(kind, steps, warmup, teacher):
    from spatial_clip_amd import data, losses, module, net, optim, streams
    n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
    if kind == "distill":
        loss_fn = losses.DistillClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    else:
        loss_fn = losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000),
        dist_net=teacher if kind == "distill" else None)

    class _T:
        max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
    m.trainer = _T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    rates = data.make_gene_rates(20000)
    batches = [{k: v.cuda() for k, v in data.synthetic_batch(256, 224, 20000, K=8, step=s, gene_rates=rates).items()}
               for s in range(2)]

    def step(i):
        with streams.chain_stream():
            loss = m.training_step(batches[i % 2], i)
            loss.backward(m.root_gradient(loss))
            opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
        return loss
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        loss = step(i)
    e1.record()
    torch.cuda.synchronize()
    rec = {"step": kind, "student": "ViT-B-16-gene", "batch": 256, "ms": round(e0.elapsed_time(e1) / steps, 3),
           "loss": round(float(loss.detach()), 5)}
    if kind == "distill":
        rec.update(teacher="ViT-L-14-gene", contrastive_loss=round(float(m.logged["train/contrastive_loss"]), 5),
                   distill_loss=round(float(m.logged["train/distill_loss"]), 5))

        def fwd():
            with torch.no_grad():
                teacher(batches[0]["images"], batches[0]["texts"])
        rec["teacher_forward_ms"] = round(timeit(fwd, n=steps, warm=2), 3)
    emit(rec)
    del m, n, opt
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.txt"))
    args = ap.parse_args()
    emit({"tool": "tools/bench_distill.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
          "warmup": args.warmup, "timing": "device events, warmed, clip and distill alternating in one process"})
    for shape in ((256, 256, 512, 768), (256, 2048, 512, 768)):
        heads(*shape)
    if not args.no_step:
        from spatial_clip_amd import net
        teacher = net.SpatialClipNet("ViT-L-14-gene", None, n_genes=20000, seed=1)
        for kind in ("clip", "distill", "clip", "distill"):
            step_time(kind, args.steps, args.warmup, teacher)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
