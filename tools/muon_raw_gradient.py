#!/usr/bin/env python3
"""The Newton-Schulz result on RAW gradients: one FusedMuon step of the tiny two-tower net of tests/test_gpu_muon.py from zero
moments (U is the rank-deficient gradient of a 12-sample batch), per Muon tensor the deviation from the float64 iteration of
the kernels, of torch.optim.Muon on the CPU and of the CPU emulation of the kernels' arithmetic (tests/_muoncases.ns_emulated),
all on bit-identical inputs, and the distance between the kernels and that emulation.  With and without a locked image tower.

Writes profiles/muon_raw_gradient.txt (one JSON line per tensor).  Recorded numbers, not assertions.

    python tools/muon_raw_gradient.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _muoncases as C            # noqa: E402
from tests import test_gpu_muon as T         # noqa: E402

if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("muon_raw_gradient.py measures on the GPU; none is available")
    os.environ["SC_OVERLAP"], os.environ["SC_ADAMW_BEHIND"] = "1", "0"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "muon_raw_gradient.txt")
    lines = [json.dumps({"tool": "tools/muon_raw_gradient.py", "device": torch.cuda.get_device_name(0),
                         "dev": "||O - O_64||_F / ||O_64||_F, O recovered from the weights"})]
    for lock in (True, False):
        n = T._net(lock_image=lock)
        st = n.store
        m, opt, sched = T._module(n, {"no_decay": "open_clip"}, warmup=1)
        sched.step()
        T._backward(m, T._batch(0))
        before = T._state(opt)
        opt.step(grad_scale=1.0, max_norm=1.0)
        got = T._state(opt)
        g, c = st.grad.detach().cpu(), float(opt.norm_clip[1])
        ge32 = C.effective(g, c, torch.float32, 1.0)
        group_of = {nm: gi for gi, grp in enumerate(opt.param_groups) for nm in grp["param_names"]}
        for name in opt.muon_names:
            sp = st.by_name[name]
            r, cc = sp.shape
            s = slice(sp.offset, sp.offset + sp.numel)
            grp = opt.param_groups[group_of[name]]
            p0, b0 = before[0][s].reshape(r, cc), before[1][s].reshape(r, cc)
            _, u32 = C.update_of(b0, ge32[s].reshape(r, cc), opt.momentum, opt.nesterov, torch.float32)
            p_t, _ = C.torch_step(p0, b0, ge32[s].reshape(r, cc), grp["lr"], grp["weight_decay"], opt.momentum, opt.nesterov, None)
            lr_adj = C._f32(grp["lr"]) * C.adjust_ratio(None, r, cc)
            ok = C.recover_o(p0, got[0][s].reshape(r, cc), grp["lr"], grp["weight_decay"], lr_adj)
            ot = C.recover_o(p0, p_t, grp["lr"], grp["weight_decay"], lr_adj)
            o64, oe = C.ns64(u32), C.ns_emulated(u32).double()
            sv = torch.linalg.svdvals(u32.double())
            dk, dt, de = C.deviation(ok, o64), C.deviation(ot, o64), C.deviation(oe, o64)
            lines.append(json.dumps({"locked_image_tower": lock, "tensor": name, "shape": [r, cc],
                                     "smallest_over_largest_singular_value_of_U": float(sv.min() / sv.max()),
                                     "dev_kernels": round(dk, 4), "dev_torch": round(dt, 4), "dev_emulation": round(de, 4),
                                     "kernels_over_torch": round(dk / dt, 3), "kernels_vs_emulation": round(C.deviation(ok, oe), 5)}))
            print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
