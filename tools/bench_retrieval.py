#!/usr/bin/env python3
"""Full-set retrieval ranks: the fused kernel (``sc_retrieval_ranks``, no N x N matrix) beside the straightforward route on
the same GPU, at N = 4096, 32768, 131072 pairs of D = 512 unit features.

F  fused      one ``ops.retrieval_ranks`` launch over all N rows: both rank vectors, nothing but 2 N ints written.
Y  yardstick  row chunks of ``ops.sgemm`` (the same f32-MFMA tile body) into a [chunk, N] fp32 buffer, then a counting pass
              over the buffer with torch (``z > d`` summed along the rows and along the columns).  Its diagonals are a plain
              row-wise dot product and it ignores ties, so it does LESS than the fused kernel; its ranks are compared with
              the fused ones and the number of rows that differ is reported (near-ties), not asserted.
C  host       at N = 4096 only: the reference's route (open_clip_train/train.py get_clip_metrics) restated -- the N x N
              logits copied to the host and a full descending argsort per direction -- timed with the host clock.

Operands are cold: before every timed launch a 1 GiB buffer is overwritten, which evicts the features from the L2s and the
256 MB last-level cache.  F and Y take turns (F Y F Y ...) in one process after one warm-up launch each; every launch is
timed on its own with device events and a synchronise.  Reported per N: the median and range of each, the achieved FLOP/s of
F for the 2 N^2 D operations of the similarity matrix (the kernel's 1/8 extra diagonal-fragment MFMAs are not counted as
useful work) against the 155 TFLOP/s measured f32-MFMA rate of the MI355X, and the peak device memory each route allocates
beyond the features (2 N D 4 bytes), from the caching allocator's peak counter.

Writes profiles/retrieval_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.

    python tools/bench_retrieval.py [--sizes 4096 32768 131072] [--dim 512] [--chunk 4096] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MFMA_RATE = 155e12          # FLOP/s, measured v_mfma_f32_16x16x4_f32 rate of the MI355X
REPS = {4096: 9, 32768: 5, 131072: 3}
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def features(N, D, dev):
    g = torch.Generator(device=dev).manual_seed(1000 + N + D)
    fi = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=-1)
    ft = torch.nn.functional.normalize(fi + 3.0 * torch.randn(N, D, device=dev, generator=g), dim=-1)
    return fi.contiguous(), ft.contiguous()


def timed(fn, flush):
    flush.add_(1.0)                                     # cold operands: 1 GiB written through the caches
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    del out
    return extra


def size(N, D, chunk, flush):
    from spatial_clip_amd import ops
    dev = torch.device("cuda", 0)
    fi, ft = features(N, D, dev)
    chunk = min(chunk, N)

    def fused():
        return ops.retrieval_ranks(fi, ft)

    def yardstick():
        z = torch.empty((chunk, N), dtype=torch.float32, device=dev)
        d = (fi * ft).sum(-1)
        r_i = torch.empty(N, dtype=torch.int64, device=dev)
        r_t = torch.zeros(N, dtype=torch.int64, device=dev)
        for r0 in range(0, N, chunk):
            m = min(chunk, N - r0)
            ops.sgemm(fi[r0:r0 + m], D, 1, ft, D, 1, z, N, m, N, D)
            zz = z[:m]
            own = (zz.diagonal(offset=r0) > d[r0:r0 + m]).long()     # z_ii against the separately formed d_i: no competitor
            r_i[r0:r0 + m] = (zz > d[r0:r0 + m, None]).sum(1) - own
            r_t += (zz > d[None, :]).sum(0)
            r_t[r0:r0 + m] -= own
        return r_i, r_t

    extra_f, extra_y = peak_extra(fused), peak_extra(yardstick)
    fused(), yardstick()                                # warm-up of both routes at this shape
    ms_f, ms_y = [], []
    for _ in range(REPS.get(N, 3)):
        t, out_f = timed(fused, flush)
        ms_f.append(t)
        t, out_y = timed(yardstick, flush)
        ms_y.append(t)
    differ = [int((a.long() != b).sum()) for a, b in zip(out_f, out_y)]
    med_f, med_y = statistics.median(ms_f), statistics.median(ms_y)
    flops = 2.0 * N * N * D
    rec = {"N": N, "D": D, "launches_each": len(ms_f), "order": "F Y", "operands": "cold (1 GiB written before every launch)",
           "F_ms": [round(x, 3) for x in ms_f], "Y_ms": [round(x, 3) for x in ms_y],
           "F_ms_median": round(med_f, 3), "Y_ms_median": round(med_y, 3),
           "F_spread_ms": round(max(ms_f) - min(ms_f), 3), "Y_spread_ms": round(max(ms_y) - min(ms_y), 3),
           "F_over_Y": round(med_f / med_y, 4), "Y_chunk_rows": chunk,
           "F_TFLOPs": round(flops / (med_f * 1e-3) / 1e12, 2), "F_share_of_155TF_f32_mfma": round(flops / (med_f * 1e-3) / F32_MFMA_RATE, 4),
           "floor_ms_at_155TF": round(flops / F32_MFMA_RATE * 1e3, 3),
           "feature_bytes": 2 * N * D * 4, "F_extra_bytes_peak": extra_f, "F_extra_bytes_expected_2N_ints": 2 * N * 4,
           "Y_extra_bytes_peak": extra_y, "full_matrix_bytes_never_allocated": 4 * N * N,
           "rows_where_Y_differs_from_F": {"image_to_text": differ[0], "text_to_image": differ[1]}}
    if N <= 4096:
        scale = 100.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logits = (scale * fi @ ft.t()).cpu()
        host = []
        for lg in (logits, logits.t()):
            order = lg.argsort(dim=1, descending=True)
            host.append(order.argsort(dim=1).diagonal().clone())          # position of column i in row i's order
        rec["C_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["C_host_matrix_bytes"] = 4 * N * N
        rec["rows_where_C_differs_from_F"] = {"image_to_text": int((host[0] != out_f[0].cpu().long()).sum()),
                                              "text_to_image": int((host[1] != out_f[1].cpu().long()).sum())}
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 32768, 131072])
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=4096, help="rows per sgemm chunk of the yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import spatial_clip_amd  # noqa: F401,E402
    if not torch.cuda.is_available():
        sys.exit("bench_retrieval.py measures on the GPU; none is available")
    emit({"tool": "tools/bench_retrieval.py", "device": torch.cuda.get_device_name(0),
          "timing": "device events around single launches, cold operands, the two routes taking turns in one process"})
    flush = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    for N in args.sizes:
        size(N, args.dim, args.chunk, flush)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
