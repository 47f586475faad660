#!/usr/bin/env python3
"""Timing of the sigmoid (SigLIP) head beside the clip head (tools/bench_head.py) at the per-rank sizes of BASELINE configs
[2]/[3] (B=256, G in {256, 2048}, D=512) and [4] (B=1024, G=8192, D=768), with the per-launch times (similarity GEMM,
loss pass, gradient GEMMs) that explain the ratio; then the configs[1] training step (ViT-B/16 + gene-MLP, local batch 256,
one process) with ClipLoss and with SigLipLoss, timed by the same eager loop.  Run on the GPU box:

    python tools/bench_siglip.py [--steps 20] [--warmup 5] [--no-step]"""
import argparse
import functools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import contrastive as C, ops


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def heads(B, G, D):
    W = G // B
    r = W // 2
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.nn.functional.normalize(torch.randn(G, D, device="cuda", generator=g), dim=-1)
    txt = torch.nn.functional.normalize(img + 0.7 * torch.randn(G, D, device="cuda", generator=g), dim=-1)
    sl = slice(r * B, (r + 1) * B)
    fi, ft = img[sl].contiguous(), txt[sl].contiguous()
    s, b = torch.tensor(10.0, device="cuda"), torch.tensor(-10.0, device="cuda")
    if W == 1:
        clip = lambda: C.contrastive_forward_backward(fi, ft, s, mode="clip", join_local=True, want_recall=False)
        sig = lambda: C.siglip_forward_backward(fi, ft, s, b, join_local=True)
    else:
        clip = lambda: C.contrastive_forward_backward(fi, ft, s, mode="clip", all_image=img, all_text=txt, rank=r,
                                                      want_recall=False)
        sig = lambda: C.siglip_forward_backward(fi, ft, s, b, all_text=txt, rank=r)
    ms_c, ms_s = timeit(clip), timeit(sig)
    # per launch of the sigmoid head
    z = torch.empty(B, G, device="cuda")
    ms_sim = timeit(lambda: ops.sgemm_grouped([(fi, D, 1, txt, D, 1, z, G, B, G, D)]))
    rowpart, lo, gr = torch.empty(B, 3, device="cuda"), torch.empty(1, device="cuda"), torch.empty(2, device="cuda")
    zz = z.clone()
    ms_loss = timeit(lambda: ops.siglip_loss(zz, B, G, r * B, s.view(1), b.view(1), rowpart, lo, gr[:1], gr[1:]))
    d1, da = torch.empty(B, D, device="cuda"), torch.empty(G, D, device="cuda")
    ms_grad = timeit(lambda: ops.sgemm_grouped([(z, G, 1, txt, 1, D, d1, D, B, D, G), (z, 1, G, fi, 1, D, da, D, G, D, B)]))
    out = {"B": B, "G": G, "D": D, "clip_head_ms": round(ms_c, 4), "siglip_head_ms": round(ms_s, 4),
           "ratio": round(ms_s / ms_c, 3), "siglip_sim_gemm_us": round(ms_sim * 1e3, 1),
           "siglip_loss_pass_us": round(ms_loss * 1e3, 1), "siglip_grad_gemms_us": round(ms_grad * 1e3, 1)}
    print(json.dumps(out), flush=True)
    return out


def step_time(loss_kind, steps, warmup):
    from spatial_clip_amd import data, losses, module, net, optim, streams
    bias = -10.0 if loss_kind == "siglip" else None
    scale = 2.302585092994046 if loss_kind == "siglip" else None
    n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0, init_logit_scale=scale, init_logit_bias=bias)
    loss_fn = losses.SigLipLoss() if loss_kind == "siglip" else losses.ClipLoss(local_loss=True, gather_with_grad=True,
                                                                                 cache_labels=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000))

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
    ms = e0.elapsed_time(e1) / steps
    out = {"step": loss_kind, "ms": round(ms, 3), "loss": round(float(loss.detach()), 5)}
    if bias is not None:
        out["logit_bias"] = round(float(n.store.p("logit_bias")), 5)
    print(json.dumps(out), flush=True)
    del m, n, opt
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    for B, G, D in ((256, 256, 512), (256, 2048, 512), (1024, 8192, 768)):
        heads(B, G, D)
    if not args.no_step:
        for kind in ("clip", "siglip", "clip", "siglip"):       # interleaved: drift shows as a difference between the pairs
            step_time(kind, args.steps, args.warmup)
