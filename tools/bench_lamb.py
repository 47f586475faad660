#!/usr/bin/env python3
"""The LAMB update beside the AdamW update: the kernels on the flat buffer of configs[1], then the whole configs[1] step.

1. Kernels.  One LAMB update -- ``sc_lamb_moments`` over the buffer, ``sc_lamb_trust``, ``sc_lamb_apply`` over the buffer (L),
   with the tensor tables of the model's own ParamStore -- and ``sc_adamw_step`` (A) over the whole flat buffer of
   ``ViT-B-16-gene`` (20000 genes) and of ``ViT-L-14-genetr``, each with the bf16 mirror and a clip coefficient, on buffers of
   their own (the same values).  Both are warmed; then blocks of ``--launches`` updates are timed with device events in the
   order A, L, A, L ..., ``--rounds`` rounds, in one process; the three LAMB kernels are also timed one by one.  Reported per
   size: the median block of each (ms per update), the range of the A blocks (what two measurements of the same kernel differ
   by in this run), the achieved bytes/s at 42 bytes per parameter for L (moments: p, g, m, v read, m, v written; apply: p, m,
   v read, p and the bf16 mirror written) and 30 for A against the HBM peak of the MI355X, and the measured L / A ratio beside
   the 42 / 30 the byte counts predict.  The byte count is arithmetic; the ratio is the measurement.
2. The whole step.  configs[1] (ViT-B-16-gene, batch 256, ClipLoss, clip 1.0, eager, the update behind the next forward) under
   ``FusedAdamW`` (configs/optimizer/adamw.yaml) and under ``FusedLamb`` with open_clip's no-decay groups
   (experiment=vitb16_gene_b256_lamb): two nets built once, taking turns, ``--rounds`` rounds of ``--steps`` steps.

Writes profiles/lamb_bench.txt (one JSON line per measurement).  Recorded numbers, not assertions.

    python tools/bench_lamb.py [--launches 20] [--rounds 7] [--steps 20] [--warmup 15] [--no-step]"""
import argparse
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12           # bytes/s, MI355X specification
ADAMW = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)       # configs/optimizer/adamw.yaml
LAMB = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)      # configs/optimizer/lamb.yaml
LAMB_BYTES, ADAMW_BYTES = 42, 30
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def block(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def host_store(model):
    from spatial_clip_amd import model_configs as mc, params
    kw = {"n_genes": 20000} if model.endswith("-gene") else {}
    return params.ParamStore(mc.get_model_config(model, **kw), torch.device("cpu"), init=False)


def kernels(args, model):
    from spatial_clip_amd import ops
    dev = torch.device("cuda", 0)
    st = host_store(model)
    n, n_t = st.total, len(st.specs)
    slot_tensor = torch.full((n // 64,), -1, dtype=torch.int32)
    tensor_slots = torch.zeros((n_t, 2), dtype=torch.int32)
    for ti, sp in enumerate(st.specs):
        lo = sp.offset // 64
        hi = lo + (max(sp.numel, 1) + 63) // 64
        slot_tensor[lo:hi] = ti
        tensor_slots[ti, 0], tensor_slots[ti, 1] = lo, hi
    largest = max(sp.numel for sp in st.specs)
    slot_tensor, tensor_slots = slot_tensor.to(dev), tensor_slots.to(dev)
    host = torch.zeros(2 + 2 * n_t, dtype=torch.float32)
    ops.lamb_hyper_host([LAMB["lr"]], [LAMB["weight_decay"]], torch.zeros(n_t, dtype=torch.int32), *LAMB["betas"], 10, host)
    hyper = host.to(dev)
    sums = torch.zeros(2 * (n // 64), device=dev)
    trust = torch.ones(n_t, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    pa = torch.randn(n, device=dev, generator=gen) * 0.02
    pl = pa.clone()
    ma, va, ml, vl = (torch.zeros(n, device=dev) for _ in range(4))
    mirror_a, mirror_l = (torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(2))
    nc = torch.zeros(2, device=dev)
    ops.grad_norm(g, n, 1.0, 1.0, nc)

    def a():
        ops.adamw_step(pa, g, ma, va, n, ADAMW["lr"], *ADAMW["betas"], ADAMW["eps"], ADAMW["weight_decay"], 10, 1.0, nc, mirror_a)

    def moments():
        ops.lamb_moments(pl, g, ml, vl, n, slot_tensor, hyper, n_t, *LAMB["betas"], LAMB["eps"], 1.0, nc, sums)

    def ratios():
        ops.lamb_trust(sums, n // 64, tensor_slots, hyper, n_t, False, False, trust)

    def apply():
        ops.lamb_apply(pl, ml, vl, n, slot_tensor, hyper, trust, n_t, LAMB["eps"], mirror_l)

    def l():
        moments()
        ratios()
        apply()

    for fn in (a, l):
        block(fn, args.launches)
    blocks_a, blocks_l = [], []
    for _ in range(args.rounds):
        blocks_a.append(block(a, args.launches))
        blocks_l.append(block(l, args.launches))
    parts = {name: statistics.median(block(fn, args.launches) for _ in range(3))
             for name, fn in (("moments", moments), ("trust", ratios), ("apply", apply))}
    med_a, med_l = statistics.median(blocks_a), statistics.median(blocks_l)
    emit({"kernels": "sc_adamw_step (A) vs sc_lamb_moments + sc_lamb_trust + sc_lamb_apply (L)", "model": model, "flat_floats": n,
          "tensors": n_t, "largest_tensor_floats": largest, "launches_per_block": args.launches, "rounds": args.rounds, "order": "A L",
          "A_ms_blocks": [round(x, 4) for x in blocks_a], "L_ms_blocks": [round(x, 4) for x in blocks_l],
          "A_ms_median": round(med_a, 4), "L_ms_median": round(med_l, 4), "AA_spread_ms": round(max(blocks_a) - min(blocks_a), 4),
          "LL_spread_ms": round(max(blocks_l) - min(blocks_l), 4),
          "L_ms_by_kernel": {k: round(v, 4) for k, v in parts.items()},
          "A_bytes_per_param": ADAMW_BYTES, "L_bytes_per_param": LAMB_BYTES,
          "A_TBps": round(ADAMW_BYTES * n / med_a / 1e9, 3), "L_TBps": round(LAMB_BYTES * n / med_l / 1e9, 3),
          "A_share_of_hbm_peak": round(ADAMW_BYTES * n / (med_a * 1e-3) / HBM_PEAK, 3),
          "L_share_of_hbm_peak": round(LAMB_BYTES * n / (med_l * 1e-3) / HBM_PEAK, 3),
          "L_over_A_measured": round(med_l / med_a, 4), "L_over_A_by_bytes": round(LAMB_BYTES / ADAMW_BYTES, 4)})
    del g, pa, pl, ma, va, ml, vl, mirror_a, mirror_l, sums
    torch.cuda.empty_cache()


class Variant:
    """One configs[1] module with its optimiser; ``run`` is the eager training step of GraphedTrainStep.eager."""

    def __init__(self, name, optimizer_cfg, warmup, param_groups=None):
        from spatial_clip_amd import data, losses, module, net, optim
        self.name = name
        self.net = n = net.SpatialClipNet("ViT-B-16-gene", None, n_genes=20000, seed=0)
        self.m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), optimizer_cfg,
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2000), param_groups=param_groups)

        class _T:
            max_steps, max_epochs, estimated_stepping_batches = 1_000_000, None, 1_000_000
        self.m.trainer = _T()
        oc = self.m.configure_optimizers()
        self.opt, self.sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        rates = data.make_gene_rates(20000)
        self.batches = [{k: v.cuda() for k, v in data.synthetic_batch(256, 224, 20000, K=8, step=s, gene_rates=rates).items()}
                        for s in range(2)]
        self.i, self.ms = 0, []
        self.run(warmup)
        torch.cuda.synchronize()

    def run(self, steps):
        from spatial_clip_amd import streams
        for _ in range(steps):
            with streams.chain_stream():
                loss = self.m.training_step(self.batches[self.i % 2], self.i)
                loss.backward(self.m.root_gradient(loss))
                self.opt.step(grad_scale=1.0, max_norm=1.0)
                self.sched.step()
            self.i += 1

    def timed(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(steps)
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(round(e0.elapsed_time(e1) / steps, 3))


def whole_step(args):
    from spatial_clip_amd import optim
    os.environ["SC_ADAMW_BEHIND"] = "1"
    variants = [Variant("FusedAdamW", functools.partial(optim.FusedAdamW, **ADAMW), args.warmup),
                Variant("FusedLamb", functools.partial(optim.FusedLamb, **LAMB), args.warmup, {"no_decay": "open_clip"})]
    for _ in range(args.rounds):
        for v in variants:
            v.timed(args.steps)
    base = statistics.median(variants[0].ms)
    for v in variants:
        state = sum(t.numel() * t.element_size() for t in v.opt._state())
        emit({"step": v.name, "model": "ViT-B-16-gene", "batch": 256, "form": "eager, update behind the forward",
              "groups": len(v.opt.param_groups), "ms_per_round": v.ms, "ms_median": statistics.median(v.ms),
              "spread_ms": round(max(v.ms) - min(v.ms), 3), "share_of_adamw": round(statistics.median(v.ms) / base, 4),
              "optimizer_state_bytes": state, "state_bytes_per_param": round(state / v.opt.store.total, 3)})
    emit({"step": "summary", "lamb_minus_adamw_ms": round(statistics.median(variants[1].ms) - base, 3)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_bench.txt"))
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 per block")
    sys.path.insert(0, ROOT)
    import spatial_clip_amd  # noqa: F401,E402
    if not torch.cuda.is_available():
        sys.exit("bench_lamb.py measures on the GPU; none is available")
    emit({"tool": "tools/bench_lamb.py", "device": torch.cuda.get_device_name(0),
          "timing": "device events, warmed, the two optimisers taking turns in one process"})
    for model in ("ViT-B-16-gene", "ViT-L-14-genetr"):
        kernels(args, model)
    if not args.no_step:
        whole_step(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
