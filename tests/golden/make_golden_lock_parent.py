#!/usr/bin/env python3
"""Three training steps of a net WITHOUT a lock on a fixed seed and batch -> tests/golden/lock_parent_bits.json.

Run on an MI355X from a checkout of the commit IN FRONT OF the locked-tower feature (built with its own kernels); the file in
the tree was recorded that way.  An unlocked net uses nothing the feature adds, so a later checkout must reproduce the same bits
and the same sequence of kernel-library calls -- which tests/test_gpu_lock_towers.py::test_unlocked_net_gives_the_parents_bits_
and_launches holds: tiny tower (32 px, patch 8, width 64, 2 layers, head 32, embed 32) + gene-MLP(100 -> 64), seed 3, perturbed
1-D parameters, synthetic batches of 12, ClipLoss, FusedAdamW (lr 1e-3, betas (0.9, 0.98), eps 1e-6, weight decay 0.1), clip
1.0, warm-up 2 of 10, weight gradients on the side stream; once per optimiser step form (behind the forward / one launch).

Recorded: SHA-256 of the flat fp32 master buffer and of both moment buffers after the three steps, the three losses and clip
norms as float hex, and the names of the library entry points the THIRD step called, in call order.

    python tests/golden/make_golden_lock_parent.py [ROOT_OF_THE_CHECKOUT_TO_RECORD]"""
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def perturb(netobj, seed=11):
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = netobj.state_dict()
    for k, v in sd.items():
        if v.ndim == 1:
            sd[k] = v.cpu() + 0.05 * torch.randn(v.shape, generator=g)
    netobj.load_state_dict(sd)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class CallLog:
    """Names of the kernel-library entry points (``sc_*``) called while ``on``, in call order."""

    def __init__(self):
        from spatial_clip_amd import _lib
        self.names, self.on = [], False
        self._lib, self._orig = _lib.lib(), {}
        for name in _lib.parse_header():
            fn = getattr(self._lib, name, None)
            if fn is not None:
                self._orig[name] = fn
                setattr(self._lib, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*a):
            if self.on:
                self.names.append(name)
            return fn(*a)
        return call

    def restore(self):
        for name, fn in self._orig.items():
            setattr(self._lib, name, fn)


def three_steps(behind: str, log: CallLog):
    """-> {"master", "exp_avg", "exp_avg_sq" (SHA-256), "losses", "norms" (float hex), "calls" (third step)}."""
    import torch
    from spatial_clip_amd import data, losses, model_configs as mc, module, net, optim
    old = {k: os.environ.get(k) for k in ("SC_ADAMW_BEHIND", "SC_OVERLAP")}
    os.environ.update({"SC_ADAMW_BEHIND": behind, "SC_OVERLAP": "1"})
    try:
        cfg = mc.ModelCfg(embed_dim=32, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(100, 64))
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
        perturb(n)
        m = module.SpatialClipLitModule(
            n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True),
            functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2))

        class T:
            max_steps, max_epochs, estimated_stepping_batches = 10, None, 10
        m.trainer = T()
        oc = m.configure_optimizers()
        opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        ls, norms = [], []
        log.names = []
        for step in range(3):
            batch = {k: v.cuda() for k, v in data.synthetic_batch(12, 32, 100, K=4, step=step).items()}
            torch.cuda.synchronize()
            log.on = step == 2
            loss = m.training_step(batch, step)
            loss.backward()
            nc = opt.step(grad_scale=1.0, max_norm=1.0)
            log.on = False
            sched.step()
            ls.append(float(loss.detach()).hex())
            norms.append(float(nc[0]).hex())
        n.store.wait_all()
        torch.cuda.synchronize()
        return {"master": _sha(n.store.master), "exp_avg": _sha(opt.exp_avg), "exp_avg_sq": _sha(opt.exp_avg_sq),
                "losses": ls, "norms": norms, "calls": list(log.names)}
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "lock_parent_bits.json")
    sys.path.insert(0, root)
    import spatial_clip_amd  # noqa: F401
    log = CallLog()
    out = {f"behind={b}": three_steps(b, log) for b in ("1", "0")}
    log.restore()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path, "from", os.path.dirname(spatial_clip_amd.__file__),
          {k: (v["master"][:12], len(v["calls"])) for k, v in out.items()})


if __name__ == "__main__":
    main()
