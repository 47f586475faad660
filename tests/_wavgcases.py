"""The oracle and the inputs of the weight-averaging tests (tests/test_cpu_weight_average.py, tests/test_gpu_weight_average.py).
CPU only: importing this module needs neither a GPU nor the HIP library.

The oracle is torch on the CPU: ``torch.optim.swa_utils.AveragedModel`` over a module with ONE flat parameter, with
``get_ema_avg_fn(decay)`` (``kind="ema"``: ``decay * avg + (1 - decay) * p``, 1 - decay formed in double and rounded to fp32
by the multiplication, product and sum rounded separately) or with its default rule (``kind="mean"``:
``avg + (p - avg) / (n_averaged + 1)``, IEEE division).  It is fed with snapshots of the weights taken after every optimiser
step; the update schedule applied to it is ``updates`` below, written from the specification and not from the code under test:
after optimiser step ``s`` (0-based) an update happens iff ``s >= (start or 0)`` and ``s % every == 0``.

Bit comparisons (``same_bits``) treat every NaN as equal to every NaN: which NaN an invalid operation (0 * inf, inf - inf) or
an operation on a NaN returns is left open by IEEE 754, and an x86 CPU and the GPU choose differently (sign and payload).
Everything else, signed zeros, denormals and infinities included, must agree bit for bit."""
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_avg_fn

DECAYS = (0.0, 0.5, 0.999, 0.9999, 1.0)
SMALL_SIZES = (1, 3, 4, 60, 64, 68, 1028)
SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, float("inf"), -float("inf"), float("nan"), 3e38, -3e38, 1.17549435e-38)


class _Flat(torch.nn.Module):
    def __init__(self, flat: torch.Tensor):
        super().__init__()
        self.w = torch.nn.Parameter(flat.detach().clone().float())


def _averaged(model: _Flat, kind: str, decay: float) -> AveragedModel:
    if kind == "ema":
        return AveragedModel(model, avg_fn=get_ema_avg_fn(decay))
    assert kind == "mean", kind
    return AveragedModel(model)


def updates(step: int, every: int, start) -> bool:
    return step >= (start or 0) and step % every == 0


def oracle_update(avg: torch.Tensor, p: torch.Tensor, kind: str, decay: float, n_averaged: int) -> torch.Tensor:
    """ONE ``AveragedModel.update_parameters`` from the state (avg, n_averaged) with the weights ``p``; n_averaged == 0 copies."""
    model = _Flat(avg)
    am = _averaged(model, kind, decay)          # deep copy: the average starts as ``avg``
    am.n_averaged.fill_(int(n_averaged))
    with torch.no_grad():
        model.w.copy_(p.detach().cpu().float())
    am.update_parameters(model)
    return am.module.w.detach().clone()


def oracle_run(snapshots, kind: str, decay: float, every: int, start, initial: torch.Tensor, trainable=None):
    """The average after feeding ``snapshots[s]`` (flat fp32 weights after optimiser step s) through the schedule.  ``initial``:
    the weights the averager was built on; elements outside the boolean mask ``trainable`` keep them.  Returns (avg,
    n_averaged)."""
    model = _Flat(initial.cpu())
    am = _averaged(model, kind, decay)
    for s, snap in enumerate(snapshots):
        if updates(s, every, start):
            with torch.no_grad():
                model.w.copy_(snap.detach().cpu().float())
            am.update_parameters(model)
    avg = am.module.w.detach().clone()
    if trainable is not None:
        keep = ~trainable.cpu()
        avg[keep] = initial.cpu().float()[keep]
    return avg, int(am.n_averaged)


def values(n: int, seed: int):
    """(avg, p): n random floats each with the special values scattered over both -- at the same index in one half of the
    cases (inf with inf, 0 with -0) and at neighbouring indices in the other."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    avg, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
    k = len(SPECIALS)
    for i, v in enumerate(SPECIALS):
        for t, j in ((avg, 5 * i), (p, 5 * i + (i % 2)), (avg, 5 * (i + k) + 2), (p, 5 * ((i + 3) % k + k) + 2)):
            if j < n:
                t[j] = v
    if n <= 4:      # too short for the scatter: one special pair per seed
        avg[0], p[n - 1] = SPECIALS[seed % k], SPECIALS[(seed + 5) % k]
    return avg, p


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    return (bits(got) == bits(want)) | (torch.isnan(got) & torch.isnan(want))


def assert_same_bits(got, want, what: str) -> None:
    ok = same_bits(got, want)
    if not bool(ok.all()):
        bad = (~ok).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {ok.numel()} elements differ, first at {i}: got "
                             f"{float(got.flatten()[i])!r} ({int(bits(got).flatten()[i]):#x}), oracle "
                             f"{float(want.flatten()[i])!r} ({int(bits(want).flatten()[i]):#x})")


# the written-out schedule table of the CPU test: (every, start) -> the steps of 0..7 behind which an update happens
SCHEDULE_TABLE = {
    (1, None): [0, 1, 2, 3, 4, 5, 6, 7], (1, 0): [0, 1, 2, 3, 4, 5, 6, 7], (1, 1): [1, 2, 3, 4, 5, 6, 7], (1, 5): [5, 6, 7],
    (2, None): [0, 2, 4, 6], (2, 0): [0, 2, 4, 6], (2, 1): [2, 4, 6], (2, 5): [6],
    (3, None): [0, 3, 6], (3, 0): [0, 3, 6], (3, 1): [3, 6], (3, 5): [6],
}
