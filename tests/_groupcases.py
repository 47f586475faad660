"""Inputs and float64 / fp32 references of the grouped AdamW kernel tests (tests/test_gpu_adamw_groups.py) and of their CPU-side
check (tests/test_cpu_param_groups.py).  CPU only: importing this module needs neither a GPU nor the HIP library.

Gradients, steps and the un-grouped hyper-parameters are those of tests/test_gpu_optim_kernels.py (``_adam_grad`` with its
exact-zero elements; four steps, the last at step 1000 with a warm-up learning rate).  A case is a flat buffer of 64-float
slots with a group per slot and (lr factor, weight decay) per group; the reference is ``torch.optim.AdamW(foreach=False)``
built with REAL parameter groups, one tensor per group holding exactly that group's slots."""
import torch

from tests.test_gpu_optim_kernels import ADAM_STEPS, ADAM_WRAP_N, B1, B2, EPS, GS, WD, _adam_grad, _f32

SLOT = 64


class Case:
    def __init__(self, name, n, slot_group, scalars):
        """``scalars``: per group (lr as a multiple of the step's base lr, weight decay)."""
        assert n % SLOT == 0 and len(slot_group) == n // SLOT and max(slot_group) < len(scalars)
        self.name, self.n, self.scalars = name, n, scalars
        self.slot_group = torch.tensor(slot_group, dtype=torch.uint8)
        self.n_groups = len(scalars)
        self.slots_of = [torch.nonzero(self.slot_group == g).flatten() for g in range(self.n_groups)]

    def group_hyper(self, base_lr):
        """[(lr_g, wd_g)] at the fp32 values the kernel receives."""
        return [(_f32(_f32(base_lr) * f), _f32(wd)) for f, wd in self.scalars]

    def gather(self, flat, g):
        """A contiguous copy of exactly the slots of group ``g``."""
        return flat.view(-1, SLOT)[self.slots_of[g].to(flat.device)].reshape(-1)


def _wide_case():
    """Past the grid cap (the grid-stride loop wraps), 256 groups, the group changing at every slot; per-group scalars from a
    seeded generator: lr between a quarter and four times the base, weight decay between 0 and 0.2."""
    n = ADAM_WRAP_N + 192
    gen = torch.Generator().manual_seed(256)
    f = 0.25 * 16.0 ** torch.rand(256, generator=gen)
    wd = 0.2 * torch.rand(256, generator=gen)
    return Case("wrap-256-groups", n, [s % 256 for s in range(n // SLOT)], [(float(a), float(b)) for a, b in zip(f, wd)])


CASES = {
    "one-slot-one-group": lambda: Case("one-slot-one-group", 64, [0], [(1.0, WD)]),
    # group 2 has lr = 0: its parameters and their mirror keep their bits while its moments advance
    "five-slots-three-groups": lambda: Case("five-slots-three-groups", 320, [0, 1, 0, 1, 2], [(1.0, WD), (4.0, 0.0), (0.0, WD)]),
    "wrap-256-groups": _wide_case,
}
FROZEN_GROUP = {"five-slots-three-groups": 2}


def start(n):
    """p, m, v at step 0."""
    return torch.randn(n, generator=torch.Generator().manual_seed(n)), torch.zeros(n), torch.zeros(n)


def torch_grouped(case, p, m, v, grad, step, base_lr, dtype):
    """One ``torch.optim.AdamW(foreach=False)`` step in ``dtype`` over real parameter groups from the given flat state;
    returns per group (p, m, v), each the group's slots in slot order."""
    hyper = case.group_hyper(base_lr)
    tensors, groups = [], []
    for g, (lr, wd) in enumerate(hyper):
        t = case.gather(p, g).to(dtype).clone()
        t.grad = case.gather(grad, g).to(dtype)
        tensors.append(t)
        groups.append({"params": [t], "lr": lr, "weight_decay": wd})
    opt = torch.optim.AdamW(groups, betas=(_f32(B1), _f32(B2)), eps=_f32(EPS), foreach=False)
    for g, t in enumerate(tensors):
        opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": case.gather(m, g).to(dtype).clone(),
                        "exp_avg_sq": case.gather(v, g).to(dtype).clone()}
    opt.step()
    return [(t.detach(), opt.state[t]["exp_avg"], opt.state[t]["exp_avg_sq"]) for t in tensors]


def scatter(case, flat, g, values):
    flat.view(-1, SLOT)[case.slots_of[g]] = values.view(-1, SLOT).to(flat.dtype)


__all__ = ["ADAM_STEPS", "B1", "B2", "EPS", "GS", "WD", "CASES", "Case", "FROZEN_GROUP", "SLOT", "_adam_grad", "_f32", "start",
           "torch_grouped", "scatter"]
