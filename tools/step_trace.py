#!/usr/bin/env python3
"""Host-order launch trace of a few tiny training steps, for comparing two revisions of the Python that sequences the kernels.

Every public function of ``spatial_clip_amd.ops`` and ``torch.cuda.Event.record`` / ``Stream.wait_event`` / ``Stream.wait_stream``
are wrapped; each call becomes one line: the op name, the role of the stream it was enqueued on (chain, side, tower, comm, default,
other), every scalar argument, and for every tensor argument a storage id (numbered by first appearance in the trace), byte offset,
shape, strides and dtype; event calls carry an event id numbered the same way.  After the steps come sha256 of every loss, of
every gradient and of every weight.  Two revisions that enqueue the same launches, on the same streams, with the same arguments and
the same event edges, write byte-identical files.

    python tools/step_trace.py --out DIR [--cells a,b,...]     every cell in a fresh child process (needs the GPU)
    python tools/step_trace.py --compare DIR_A DIR_B           per cell: line counts and identical / DIFFERENT (no GPU)

``SC_OVERLAP`` is pinned in every cell: ``auto`` times the backward and is covered by tests/test_gpu_model.py."""
import argparse
import functools
import hashlib
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(kind="gene", vision=(48, 16, 128, 3, 64), B=64, steps=2)
FP8 = dict(kind="gene", vision=(32, 8, 256, 3, 64), B=128, steps=3, precision="fp8", n_genes=200)
RC = dict(kind="genetr", vision=(48, 16, 128, 4, 64), B=24, steps=2)
TEXT = dict(kind="text", steps=2)


def _cell(spec, env=None, **kw):
    return dict(spec, env=dict({"SC_OVERLAP": "1"}, **(env or {})), **kw)


CELLS = {
    "base_ov0": _cell(BASE, {"SC_OVERLAP": "0"}),
    "base_ov1": _cell(BASE),                                   # = SC_WGRAD_GROUP auto
    **{f"wgrad_group_{m}": _cell(BASE, {"SC_WGRAD_GROUP": m}) for m in "01234"},
    "res_stream_fp32": _cell(BASE, {"SC_RES_STREAM": "fp32"}),
    "res_grad_fp32": _cell(BASE, {"SC_RES_GRAD": "fp32"}),
    "cls_only_0": _cell(BASE, {"SC_CLS_ONLY": "0"}),
    "cls_q_0": _cell(BASE, {"SC_CLS_Q": "0"}),
    "quick_gelu": _cell(BASE, quick_gelu=True),
    **{f"recompute_{'on' if rc else 'off'}_ov{ov}": _cell(RC, {"SC_OVERLAP": ov}, recompute=rc)
       for rc in (False, True) for ov in "01"},
    "text_sequential": _cell(TEXT, {"SC_TOWER_OVERLAP": "0"}),
    "text_side_by_side": _cell(TEXT, {"SC_TOWER_OVERLAP": "1"}),
    "fp8_wgrad_1": _cell(FP8, {"SC_FP8_WGRAD": "1"}),
    "fp8_wgrad_0": _cell(FP8, {"SC_FP8_WGRAD": "0"}),
    "fp8_delayed_0": _cell(FP8, {"SC_FP8_DELAYED": "0"}),
    "fp8_recompute": _cell(FP8, recompute=True),
    "patch_dropout": _cell(BASE, patch_dropout=0.5),
    "bucket_callback": _cell(BASE, bucket=True, steps=1),
}


# ------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    def __init__(self, torch, streams):
        self.torch, self.streams = torch, streams
        self.lines, self.storages, self.events, self.others = [], {}, 0, {}
        self.net = None

    def role(self, stream=None):
        torch, st = self.torch, self.streams
        s = torch.cuda.current_stream() if stream is None else stream
        h = s.cuda_stream
        for name, table in (("chain", st._chain), ("tower", st._tower), ("comm", st._comm)):
            if any(x.cuda_stream == h for x in table.values()):
                return name
        for tower in ((self.net.vision, self.net.second) if self.net is not None else ()):
            side = getattr(getattr(tower, "stack", None), "_side", None)
            if side is not None and side.cuda_stream == h:
                return "side"
        if h == torch.cuda.default_stream().cuda_stream:
            return "default"
        return "other%d" % self.others.setdefault(h, len(self.others))

    def event_id(self, ev):
        if not hasattr(ev, "_trace_id"):
            ev._trace_id = self.events
            self.events += 1
        return "E%d" % ev._trace_id

    def fmt(self, v):
        torch = self.torch
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                return "host%s%s" % (tuple(v.shape), str(v.dtype)[6:])
            base = v.untyped_storage().data_ptr()
            sid = self.storages.setdefault(base, len(self.storages))
            return "T%d+%d%s%s%s" % (sid, v.data_ptr() - base, list(v.shape), list(v.stride()), str(v.dtype)[6:])
        if isinstance(v, torch.cuda.Event):
            return self.event_id(v)
        if isinstance(v, torch.cuda.Stream):
            return "stream:" + self.role(v)
        if isinstance(v, (list, tuple)):
            return "[" + ",".join(self.fmt(x) for x in v) + "]"
        if isinstance(v, dict):
            return "{" + ",".join("%s=%s" % (k, self.fmt(x)) for k, x in sorted(v.items())) + "}"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        return "<%s>" % type(v).__name__

    def emit(self, name, role, args):
        self.lines.append("%s @%s %s" % (name, role, " ".join("%s=%s" % (k, self.fmt(v)) for k, v in args)))

    def wrap_op(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def traced(*a, **k):
            try:
                bound = sig.bind(*a, **k)
                bound.apply_defaults()          # the effective arguments: a default spelled out is the same call
                args = list(bound.arguments.items())
            except TypeError:
                args = [("arg%d" % i, v) for i, v in enumerate(a)] + sorted(k.items())
            self.emit(name, self.role(), args)
            return fn(*a, **k)
        return traced

    def install(self, ops):
        torch = self.torch
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and not name.startswith("_") and fn.__module__ == ops.__name__:
                setattr(ops, name, self.wrap_op(name, fn))
        rec, wev, wst = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def record(ev, stream=None):
            self.emit("event.record", self.role(stream), [("event", ev)])
            return rec(ev) if stream is None else rec(ev, stream)

        def wait_event(stream, ev):
            self.emit("stream.wait_event", self.role(stream), [("event", ev)])
            return wev(stream, ev)

        def wait_stream(stream, other):
            self.emit("stream.wait_stream", self.role(stream), [("other", other)])
            return wst(stream, other)
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = record, wait_event, wait_stream

    def sha(self, tag, t):
        self.torch.cuda.synchronize()
        self.lines.append("sha256 %s %s" % (tag, hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(
            self.torch.uint8).numpy().tobytes()).hexdigest()))


# ------------------------------------------------------------------------------------------------ one cell (child process)
def _model(cell):
    import numpy as np
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, model_configs as mc, net
    kw = dict(precision=cell.get("precision", "bf16"))
    if cell.get("patch_dropout"):
        kw["force_patch_dropout"] = cell["patch_dropout"]
    if cell["kind"] == "text":
        import json
        z = np.load(os.path.join(ROOT, "tests", "golden", "train3_tiny_text.npz"), allow_pickle=False)
        c = json.loads(str(z["cfg"]))
        v, t = c["vision_cfg"], c["text_cfg"]
        cfg = mc.ModelCfg(embed_dim=c["embed_dim"],
                          vision=mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64)),
                          text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, **kw)
        n.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0.")})
        g = lambda k: torch.from_numpy(z[k]).cuda()
        batch = {"images": g("images"), "texts": g("texts"), "image_tile_ids": g("ids"), "text_tile_ids": g("ids"),
                 "neighbor_tile_ids": g("nb"), "neighbor_alphas": g("alpha")}
        return n, (lambda step: batch)
    image, patch, width, layers, head = cell["vision"]
    n_genes = cell.get("n_genes", 100)
    gene = mc.GeneCfg(300, 0, "transformer", 64, 64, 4, 32) if cell["kind"] == "genetr" else mc.GeneCfg(n_genes, 64)
    cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(image, patch, width, layers, head), text=None, gene=gene,
                      quick_gelu=bool(cell.get("quick_gelu", False)))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3, **kw)
    gen = torch.Generator().manual_seed(11)          # non-trivial biases / LayerNorm affine parameters
    sd = n.state_dict()
    n.load_state_dict({k: (v.cpu() + 0.05 * torch.randn(v.shape, generator=gen) if v.ndim == 1 else v) for k, v in sd.items()})

    def batch(step):
        return {k: v.cuda() for k, v in data.synthetic_batch(cell["B"], image, cfg.gene.n_genes, K=4, step=step).items()}
    return n, batch


def run_cell(name, out_dir):
    cell = CELLS[name]
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import losses, module, ops, optim, streams
    n, batch_of = _model(cell)
    if cell.get("recompute"):
        n.model.set_grad_checkpointing(True)
    n.train()
    loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                 neighbor_alpha_scale=0.5, float32_logits=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=1))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = 10, None, 10
    m.trainer = T()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    batches = [batch_of(s) for s in range(cell["steps"])]
    torch.cuda.synchronize()
    r = Recorder(torch, streams)
    r.net = n
    r.install(ops)
    for step, b in enumerate(batches):
        r.lines.append("# step %d" % step)
        with streams.chain_stream():
            if cell.get("bucket"):
                # the towers' backward called directly with a recording callback: its order and its stream are in the trace
                out = n(b["images"], b["texts"])
                on_bucket = lambda names: r.emit("on_bucket", r.role(), [("names", ",".join(names))])
                gen = torch.Generator().manual_seed(5)
                d = [torch.randn(f.shape, generator=gen).cuda() for f in (out["text_features"], out["image_features"])]
                n.second.backward(d[0], on_bucket=on_bucket)
                n.vision.backward(d[1], on_bucket=on_bucket)
                loss = out["logit_scale"]
            else:
                loss = m.training_step(b, step)
                loss.backward()
        r.sha("loss.%d" % step, loss)
        if not cell.get("bucket"):
            with streams.chain_stream():
                opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
    n.store.wait_all()
    for k in n.state_dict():
        r.sha("grad." + k, n.store.g(k))
    for k, v in n.state_dict().items():
        r.sha("weight." + k, v)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".trace"), "w") as f:
        f.write("\n".join(r.lines) + "\n")
    print("[step_trace] %s: %d lines" % (name, len(r.lines)), flush=True)


# ------------------------------------------------------------------------------------------------ driver / comparison
def run_all(out_dir, names):
    for name in names:
        env = dict(os.environ, **CELLS[name]["env"])
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", name, "--out", out_dir], env=env, timeout=180)
        if p.returncode != 0:       # a fault ends the run: nothing more is started on the device
            print("[step_trace] %s: exit %d -- stopping" % (name, p.returncode), flush=True)
            return p.returncode
    return 0


def compare(a, b):
    bad = 0
    print("%-22s %8s %8s  %s" % ("cell", "lines A", "lines B", "verdict"))
    for name in CELLS:
        pa, pb = (os.path.join(d, name + ".trace") for d in (a, b))
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("%-22s %8s %8s  MISSING" % (name, "-", "-"))
            bad += 1
            continue
        ta, tb = open(pa, "rb").read(), open(pb, "rb").read()
        same = ta == tb
        bad += not same
        print("%-22s %8d %8d  %s" % (name, ta.count(b"\n"), tb.count(b"\n"), "identical" if same else "DIFFERENT"))
        if not same:
            la, lb = ta.decode().split("\n"), tb.decode().split("\n")
            k = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("    first difference at line %d:\n    A: %s\n    B: %s" % (k + 1, la[k][:400] if k < len(la) else "<end>",
                                                                           lb[k][:400] if k < len(lb) else "<end>"))
    print("%d cells, %d differ" % (len(CELLS), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory the .trace files go to")
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--cell")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out DIR is required")
    sys.path.insert(0, ROOT)
    if a.cell:
        run_cell(a.cell, a.out)
        return
    sys.exit(run_all(a.out, a.cells.split(",")))


if __name__ == "__main__":
    main()
