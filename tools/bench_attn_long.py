#!/usr/bin/env python3
"""Attention forward / backward alone above 320 tokens (sc_attention_stream.hip): B=64, H=16, dh=64 at
L in {321, 401, 577, 785, 1025} on Gaussian inputs, with F.scaled_dot_product_attention on the same tensors beside it.
TFLOP/s counts 4*B*H*L^2*dh (forward) and 10*B*H*L^2*dh (backward).  Then, at L = 197 and 257, the long kernels forced by
SC_ATTN_LONG=1 against the in-tree kernels of that length, interleaved.

    python tools/bench_attn_long.py [--lengths 577,1025] [--batch 64] [--heads 16] [--iters 20] [--json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_clip_amd  # noqa: E402,F401
from spatial_clip_amd import ops  # noqa: E402

DH = 64


def timeit(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def tensors(B, L, H):
    d = H * DH
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = torch.randn(B * L, 3 * d, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B * L, d, device="cuda", generator=g).bfloat16()
    out = torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, L, device="cuda")
    return qkv, dout, out, lse, torch.empty_like(qkv), torch.empty(B, H, L, device="cuda")


def ours(B, L, H, iters):
    qkv, dout, out, lse, dqkv, delta = tensors(B, L, H)
    f = timeit(lambda: ops.attn_fwd(qkv, B, L, H, DH, out=out, lse=lse), iters)
    b = timeit(lambda: ops.attn_bwd(qkv, out, dout, lse, B, L, H, DH, dqkv=dqkv, delta=delta), iters)
    return f, b


def sdpa(B, L, H, iters):
    qkv, dout, *_ = tensors(B, L, H)
    d = H * DH
    q, k, v = (t.view(B, L, H, DH).transpose(1, 2).detach().requires_grad_(True) for t in qkv.view(B, L, 3 * d).split(d, -1))
    go = dout.view(B, L, H, DH).transpose(1, 2)
    with torch.no_grad():
        f = timeit(lambda: F.scaled_dot_product_attention(q, k, v), iters)
    o = F.scaled_dot_product_attention(q, k, v)
    b = timeit(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True), iters)
    return f, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="321,401,577,785,1025")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--no-forced", action="store_true")
    ap.add_argument("--json", action="store_true", help="one JSON line per measurement besides the table")
    a = ap.parse_args()
    B, H = a.batch, a.heads
    os.environ.pop("SC_ATTN_LONG", None)
    print(f"B={B} H={H} dh={DH}; us per launch over {a.iters} launches; TFLOP/s = 4 (fwd) / 10 (bwd) * B*H*L^2*dh / t")
    print(f"{'L':>5} | {'fwd us':>8} {'TF/s':>6} | {'bwd us':>8} {'TF/s':>6} | {'sdpa fwd':>8} {'TF/s':>6} | {'sdpa bwd':>8} {'TF/s':>6}")
    for L in (int(x) for x in a.lengths.split(",")):
        fl = B * H * L * L * DH
        f, b = ours(B, L, H, a.iters)
        sf, sb = sdpa(B, L, H, a.iters) if not a.no_sdpa else (float("nan"), float("nan"))
        tf = lambda n, t: n * fl / t / 1e6  # noqa: E731
        print(f"{L:5d} | {f:8.1f} {tf(4, f):6.0f} | {b:8.1f} {tf(10, b):6.0f} | {sf:8.1f} {tf(4, sf):6.0f} | "
              f"{sb:8.1f} {tf(10, sb):6.0f}", flush=True)
        if a.json:
            print(json.dumps({"L": L, "B": B, "H": H, "fwd_us": f, "bwd_us": b, "fwd_tflops": tf(4, f),
                              "bwd_tflops": tf(10, b), "sdpa_fwd_us": sf, "sdpa_bwd_us": sb}), flush=True)
    if a.no_forced:
        return
    print("forced SC_ATTN_LONG=1 against the in-tree kernels, interleaved (us)")
    for L in (197, 257):
        for rep in range(2):
            for sw, tag in (("0", "in-tree"), ("1", "long (forced)")):
                os.environ["SC_ATTN_LONG"] = sw
                f, b = ours(B, L, H, a.iters)
                print(f"L={L} rep {rep} {tag:14s} fwd {f:8.1f} bwd {b:8.1f}", flush=True)
        os.environ.pop("SC_ATTN_LONG", None)


if __name__ == "__main__":
    main()
