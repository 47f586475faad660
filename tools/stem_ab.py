#!/usr/bin/env python3
"""Stem kernels (csrc/sc_embed.hip) of the working tree against a library built from another revision: bits and time.

    python tools/build_from_rev.py parent HEAD~ sc_embed.hip        # -> spatial-clip_amd/lib/libspatialclip_hip_parent.so
    python tools/stem_ab.py [--parent <that library>] [--rounds 5] [--out profiles/stem_merge_ab.txt]

Every entry point of the file that launches a changed kernel runs on seeded inputs at the shapes users run (ViT-B/16 at batch
256, ViT-L/14 and ViT-H/14 at batch 128; ViT-B/16 with patch dropout 0.5 and 0.75; the text tower's embedding backward at batch
256), first once for a SHA-256 of every output buffer (round 1 only), then 20 warm-up and 1000 timed calls between two device
events.  A round is one fresh child process per library (SC_HIP_LIB selects it), parent first, each under its own ``timeout``,
all chained with ``&&``: one process on the device at a time, and a child that faults or hangs ends the run.

The two lists of hashes must be equal.  The atomic sc_token_embed_bwd is not reproducible even within one build: each child
compares its dtable with the deterministic kernel's by allclose, and the deterministic one is hashed.
Bar per case: this tree's median <= the parent's median * (1 + the parent's spread), spread = (max - min) / median
over its rounds.  A time is per CALL of the entry point (sc_embed_ln_bwd is three launches), host enqueue included."""
import argparse
import hashlib
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "spatial-clip_amd", "lib", "libspatialclip_hip_parent.so")
# name, B, tokens of the pass, width, patch size, image size
FULL = [("ViT-B/16 B=256", 256, 197, 768, 16, 224), ("ViT-L/14 B=128", 128, 257, 1024, 14, 224),
        ("ViT-H/14 B=128", 128, 257, 1280, 14, 224)]
DROP = [("ViT-B/16 B=256 p=0.5", 256, 99, 768, 16, 224), ("ViT-B/16 B=256 p=0.75", 256, 50, 768, 16, 224),
        ("ViT-L/14 B=128 p=0.5", 128, 129, 1024, 14, 224)]
WARMUP, TIMED = 20, 1000


def child(hashing: bool) -> None:
    sys.path.insert(0, ROOT)
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, ops, patch_dropout as pd

    def sha(t):
        if not hashing:
            return "-"
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    def clock(case, what, f):
        for _ in range(WARMUP):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(TIMED):
            f()
        e1.record()
        torch.cuda.synchronize()
        print(f"time|{case}|{what}|{e0.elapsed_time(e1) / TIMED * 1e3:.2f}", flush=True)

    def dev(*shape, g, dtype=torch.float32):
        return torch.randn(*shape, generator=g).to(dtype).cuda()

    for keep_pass, cases in ((False, FULL), (True, DROP)):
        for name, B, L, d, P, S in cases:
            g = torch.Generator().manual_seed(1000 * L + d)
            n = (S // P) ** 2
            K = L - 1
            kp = 3 * P * P
            kpad = (kp + 63) // 64 * 64
            keep = slot = None
            if keep_pass:
                kh = pd.keep_indices_host(7, 3, 0, B, n, K)
                keep = torch.from_numpy(kh).cuda()
                slot = torch.from_numpy(pd.slots_from_keep(kh, n)).cuda()
            img = dev(B, 3, S, S, g=g)
            patches = torch.zeros(B * K, kpad, dtype=torch.bfloat16, device="cuda")
            patch_out, cls, pos = dev(B * K, d, g=g), dev(d, g=g), dev(n + 1 if keep_pass else L, d, g=g)
            gamma, beta, dy = 1.0 + 0.1 * dev(d, g=g), dev(d, g=g), dev(B * L, d, g=g)
            x, x16 = torch.empty(B * L, d, device="cuda"), torch.empty(B * L, d, dtype=torch.bfloat16, device="cuda")
            mean, rstd = torch.empty(B * L, device="cuda"), torch.empty(B * L, device="cuda")
            mean16, rstd16 = torch.empty_like(mean), torch.empty_like(rstd)
            dres, dpatch = dy.clone(), torch.empty(B * K, d, dtype=torch.bfloat16, device="cuda")
            dg, db, dcls = (torch.empty(d, device="cuda") for _ in range(3))
            dpos = torch.empty_like(pos)
            calls = [
                ("im2col", lambda: ops.im2col(img, patches, P, keep=keep), {"patches": patches}),
                ("embed_ln_fwd", lambda: ops.embed_ln_fwd(patch_out, cls, pos, gamma, beta, x, mean, rstd, B, L, d, keep=keep),
                 {"x": x, "mean": mean, "rstd": rstd}),
                ("embed_ln_fwd_x16", lambda: ops.embed_ln_fwd(patch_out, cls, pos, gamma, beta, x16, mean16, rstd16, B, L, d,
                                                              keep=keep), {"x": x16, "mean": mean16, "rstd": rstd16}),
                # in place on dres: the timed calls go on from the last result (same data in both libraries)
                ("embed_ln_bwd", lambda: ops.embed_ln_bwd(dres, patch_out, cls, pos, mean, rstd, gamma, dpatch, dg, db, dpos, dcls,
                                                          B, L, d, keep=keep, slot=slot),
                 {"dres": dres, "dpatch": dpatch, "dgamma": dg, "dbeta": db, "dpos": dpos, "dcls": dcls}),
            ]
            for what, f, outs in calls:
                what += "_keep" if keep_pass else ""
                f()
                for k, t in outs.items():
                    print(f"hash|{name}|{what}|{k}|{sha(t)}", flush=True)
                clock(name, what, f)

    name, B, L, d, V = "text B=256", 256, 77, 512, 49408
    g = torch.Generator().manual_seed(77)
    tokens = data.synthetic_captions(B, L, V, seed=3).cuda()
    dres = dev(B * L, d, g=g)
    dt_det, dt_atomic = torch.empty(V, d, device="cuda"), torch.empty(V, d, device="cuda")
    dp_det, dp_atomic = torch.empty(L, d, device="cuda"), torch.empty(L, d, device="cuda")
    det = lambda: ops.token_embed_bwd(tokens, dres, dt_det, dp_det, B, L, d, V)
    atomic = lambda: ops.token_embed_bwd(tokens, dres, dt_atomic, dp_atomic, B, L, d, V, deterministic=False)
    det()
    atomic()
    print(f"hash|{name}|token_embed_bwd_det|dtable|{sha(dt_det)}")
    print(f"hash|{name}|token_embed_bwd_det|dpos|{sha(dp_det)}")
    print(f"hash|{name}|token_embed_bwd|dpos|{sha(dp_atomic)}")
    ok = torch.allclose(dt_atomic, dt_det, rtol=1e-5, atol=1e-5)
    print(f"close|{name}|token_embed_bwd|dtable against the deterministic kernel's, allclose(rtol=1e-5, atol=1e-5)|{ok}|"
          f"max abs difference {float((dt_atomic - dt_det).abs().max()):.3g}", flush=True)
    clock(name, "token_embed_bwd_det", det)
    clock(name, "token_embed_bwd", atomic)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=PARENT, help="library built by tools/build_from_rev.py")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_merge_ab.txt"))
    ap.add_argument("--child", choices=["hash", "time"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child == "hash")
        return 0
    me = shlex.quote(os.path.abspath(__file__))
    run = f"timeout -k 10 {args.timeout} {shlex.quote(sys.executable)} {me} --child "
    steps = []
    for r in range(args.rounds):
        mode = "hash" if r == 0 else "time"
        steps += [f"echo 'run|{r + 1}|parent' && SC_HIP_LIB={shlex.quote(args.parent)} {run}{mode}",
                  f"echo 'run|{r + 1}|this' && {run}{mode}"]
    env = {k: v for k, v in os.environ.items() if k != "SC_HIP_LIB"}
    p = subprocess.run(" && ".join(steps), shell=True, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
    hashes, times, close, who = {}, {}, [], None
    for line in p.stdout.splitlines():
        f = line.split("|")
        if f[0] == "run":
            who = (int(f[1]), f[2])
        elif f[0] == "hash":
            hashes.setdefault(who, []).append(tuple(f[1:]))
        elif f[0] == "time":
            times.setdefault((f[1], f[2]), {}).setdefault(who[1], []).append(float(f[3]))
        elif f[0] == "close":
            close.append((who, f[1:]))
    out = ["Stem kernels (sc_embed.hip): the working tree against the parent commit's sc_embed.o in an otherwise identical library,",
           "one MI355X.  Commands:",
           "    python tools/build_from_rev.py parent HEAD~ sc_embed.hip",
           f"    python tools/stem_ab.py --rounds {args.rounds}",
           f"{args.rounds} rounds, each one fresh process per library, parent first; per case {WARMUP} warm-up and {TIMED} timed calls "
           "between two device events.", ""]
    ok = p.returncode == 0
    if not ok:
        out.append(f"STOPPED: a child ended with status {p.returncode}; nothing was started after it")
    ref = hashes.get((1, "parent"), [])
    hashes = {who: hs for who, hs in hashes.items() if who[0] == 1}
    same = ok and bool(ref) and len(hashes) == 2 and all(h == ref for h in hashes.values())
    out.append(f"== bits: SHA-256 of every output buffer in round 1, {len(ref)} buffers: "
               + ("ALL EQUAL in the two libraries" if same else "DIFFERENT"))
    for h in ref:
        out.append("    " + " | ".join(h[:3]) + " " + h[3][:16])
    if not same:
        for who, hs in hashes.items():
            for a, b in zip(ref, hs):
                if a != b:
                    out.append(f"    differs in {who[1]}: {' | '.join(b[:3])} {b[3][:16]} (parent {a[3][:16]})")
    for who, f in close:
        out.append(f"    round {who[0]} {who[1]}: {f[1]} {f[2]}: {f[3]}, {f[4]}")
    out += ["", "== time: us per call, every round, then median / ratio / parent spread / bar"]
    over = []
    for (case, what), t in times.items():
        a, b = t.get("parent", []), t.get("this", [])
        out.append(f"{case:24s} {what:24s} parent " + " ".join(f"{v:8.2f}" for v in a) + "   this " + " ".join(f"{v:8.2f}" for v in b))
        if len(a) == args.rounds and len(b) == args.rounds:
            ma, mb = statistics.median(a), statistics.median(b)
            spread = (max(a) - min(a)) / ma
            within = mb <= ma * (1 + spread)
            if not within:
                over.append((case, what))
            out.append(f"{'':49s} median parent {ma:8.2f} this {mb:8.2f} ratio {mb / ma:.4f}  parent spread {spread:.4f}  "
                       f"bar {1 + spread:.4f}  {'WITHIN' if within else 'OVER'} the bar")
    out += ["", "over the bar: " + (", ".join(f"{c} {w}" for c, w in over) if over else "none")]
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
