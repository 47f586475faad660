#!/usr/bin/env python3
"""Attention forward / backward alone at head dim 80 (sc_attention_stream.hip; ViT-H): B=64, H=16 at L in {77 causal, 197,
257} on Gaussian inputs, with F.scaled_dot_product_attention on the same tensors beside it and the in-tree dh = 64
kernels at H = 20 (the same B * L * width, hence the same FLOP count) beside that.  TFLOP/s counts 4*B*H*L^2*dh
(forward) and 10*B*H*L^2*dh (backward), causal or not.  The SDPA backend that the default call takes is named by timing
each backend alone (forward) and picking the one whose time the default call matches.

    python tools/bench_attn_d80.py [--cases 77c,197,257] [--batch 64] [--heads 16] [--iters 20] [--json]
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

DH = 80


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


def tensors(B, L, H, dh):
    d = H * dh
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = torch.randn(B * L, 3 * d, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B * L, d, device="cuda", generator=g).bfloat16()
    out = torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, L, device="cuda")
    return qkv, dout, out, lse, torch.empty_like(qkv), torch.empty(B, H, L, device="cuda")


def ours(B, L, H, dh, causal, iters):
    qkv, dout, out, lse, dqkv, delta = tensors(B, L, H, dh)
    f = timeit(lambda: ops.attn_fwd(qkv, B, L, H, dh, causal=causal, out=out, lse=lse), iters)
    b = timeit(lambda: ops.attn_bwd(qkv, out, dout, lse, B, L, H, dh, causal=causal, dqkv=dqkv, delta=delta), iters)
    return f, b


def sdpa(B, L, H, dh, causal, iters):
    qkv, dout, *_ = tensors(B, L, H, dh)
    d = H * dh
    q, k, v = (t.view(B, L, H, dh).transpose(1, 2).detach().requires_grad_(True) for t in qkv.view(B, L, 3 * d).split(d, -1))
    go = dout.view(B, L, H, dh).transpose(1, 2)
    with torch.no_grad():
        f = timeit(lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal), iters)
    o = F.scaled_dot_product_attention(q, k, v, is_causal=causal)
    b = timeit(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True), iters)
    per = {}
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        for be in (SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION, SDPBackend.MATH):
            try:
                with torch.no_grad(), sdpa_kernel([be]):
                    per[be.name] = timeit(lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal), iters)
            except RuntimeError:
                per[be.name] = None                   # this backend does not take the shape
    except ImportError:
        pass
    usable = {n: t for n, t in per.items() if t is not None}
    backend = min(usable, key=lambda n: abs(usable[n] - f)) if usable else "unknown"
    return f, b, backend, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="77c,197,257", help="lengths; a trailing c = causal")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--json", action="store_true", help="one JSON line per measurement besides the table")
    a = ap.parse_args()
    B, H = a.batch, a.heads
    H64 = H * DH // 64
    assert H64 * 64 == H * DH, "heads * 80 must be a multiple of 64 for the equal-width dh = 64 run"
    print(f"B={B} H={H} dh={DH} (dh = 64 beside it at H={H64}); us per launch over {a.iters} launches; "
          f"TFLOP/s = 4 (fwd) / 10 (bwd) * B*H*L^2*dh / t")
    print(f"{'L':>6} | {'fwd us':>8} {'TF/s':>6} | {'bwd us':>8} {'TF/s':>6} | {'sdpa fwd':>8} {'TF/s':>6} | {'sdpa bwd':>8} "
          f"{'TF/s':>6} | {'d64 fwd':>8} {'d64 bwd':>8} | sdpa backend")
    for case in a.cases.split(","):
        causal = case.endswith("c")
        L = int(case.rstrip("c"))
        fl = B * H * L * L * DH
        f, b = ours(B, L, H, DH, causal, a.iters)
        f64, b64 = ours(B, L, H64, 64, causal, a.iters)
        sf, sb, backend, per = (sdpa(B, L, H, DH, causal, a.iters) if not a.no_sdpa
                                else (float("nan"), float("nan"), "-", {}))
        tf = lambda n, t: n * fl / t / 1e6  # noqa: E731
        print(f"{case:>6} | {f:8.1f} {tf(4, f):6.0f} | {b:8.1f} {tf(10, b):6.0f} | {sf:8.1f} {tf(4, sf):6.0f} | "
              f"{sb:8.1f} {tf(10, sb):6.0f} | {f64:8.1f} {b64:8.1f} | {backend} {per}", flush=True)
        if a.json:
            print(json.dumps({"L": L, "causal": causal, "B": B, "H": H, "dh": DH, "fwd_us": f, "bwd_us": b,
                              "fwd_tflops": tf(4, f), "bwd_tflops": tf(10, b), "sdpa_fwd_us": sf, "sdpa_bwd_us": sb,
                              "sdpa_backend": backend, "sdpa_fwd_us_by_backend": per, "d64_heads": H64,
                              "d64_fwd_us": f64, "d64_bwd_us": b64, "fwd_ratio_to_d64": f / f64,
                              "bwd_ratio_to_d64": b / b64}), flush=True)


if __name__ == "__main__":
    main()
