"""Gradient accumulation (Trainer accumulate_grad_batches) without a GPU: the stepping rule and what is sized from it, the
refusals, the host expressions of ``ops.grad_accumulate`` against hand values, and two gloo ranks driving
``GradAccumulator.hook`` in front of the bucketed all-reduce."""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import ops, optim, trainer as T


def _steps(n, every):
    return [i for i, s in enumerate(T.accum_steps_after(n, every)) if s]


def test_accum_steps_after_rule():
    assert _steps(5, 2) == [1, 3, 4]            # a short last group still steps
    assert _steps(4, 4) == [3]
    assert _steps(3, 4) == [2]                  # fewer batches than one group
    assert _steps(7, 1) == list(range(7))
    assert T.accum_steps_after(0, 3) == []


class _FiveBatches:
    """The least of a data module that ``Trainer.fit`` touches before its first batch."""
    preprocess_fn = tokenizer = None

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [None] * 5


def test_estimated_stepping_batches_and_resume_arithmetic():
    tr = T.Trainer(max_epochs=3, accumulate_grad_batches=2)
    assert tr.accumulate_grad_batches == 2
    assert T.steps_per_epoch(5, 2) == 3 and T.steps_per_epoch(5, 2) * 3 == 9

    class _Stop(Exception):
        pass

    class _Model:
        net = SimpleNamespace(preprocess_train=None, tokenizer=None, precision="bf16")

        def configure_optimizers(self):     # fit() has sized the schedule by the time it asks for the optimiser
            raise _Stop

    with pytest.raises(_Stop):
        tr.fit(_Model(), _FiveBatches())
    assert tr.estimated_stepping_batches == 9
    # global_step 4 of that run: epoch 0 took 3 steps (batches 0-1, 2-3, 4), so it is 1 step = 2 batches into epoch 1
    assert T.resume_position(4, 5, 2) == (1, 2)
    assert T.resume_position(3, 5, 2) == (1, 0) and T.resume_position(2, 5, 2) == (0, 4)
    assert T.resume_position(7, 5, 1) == (1, 2)             # N = 1: today's arithmetic (global_step // n_train, remainder)


@pytest.mark.parametrize("bad", [0, -1, 2.5, 1.0, "2", None, True, {0: 2, 4: 4}])
def test_refused_values_name_the_argument(bad):
    with pytest.raises(ValueError, match="accumulate_grad_batches") as e:
        T.Trainer(accumulate_grad_batches=bad)
    assert "integer >= 1" in str(e.value)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        optim.GradAccumulator(SimpleNamespace(total=4, grad=torch.zeros(4)), bad)


def test_sharded_exchange_is_refused_with_accumulation(monkeypatch):
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    with pytest.raises(ValueError, match="SC_GRAD_EXCHANGE") as e:
        T.Trainer(accumulate_grad_batches=2)
    assert "accumulate_grad_batches" in str(e.value)
    assert T.Trainer(accumulate_grad_batches=1).accumulate_grad_batches == 1      # N = 1 keeps every route
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "allreduce")
    assert T.Trainer(accumulate_grad_batches=2).accumulate_grad_batches == 2


def test_default_is_one_and_changes_nothing():
    a, b = T.Trainer(), T.Trainer(accumulate_grad_batches=1)
    assert a.accumulate_grad_batches == 1 and a.accumulator is None
    assert vars(a) == vars(b)


def test_hydra_key_reaches_the_trainer(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    from spatial_clip_amd import hydra_lite as H
    tr = H.instantiate(H.compose("train.yaml", ["experiment=smoke_shards", "+trainer.accumulate_grad_batches=4"]).trainer)
    assert tr.accumulate_grad_batches == 4
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b64_accum4"])
    assert cfg.trainer.accumulate_grad_batches == 4 and cfg.data.batch_size == 64
    assert cfg.model.net.model_name == "ViT-B-16-gene"
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        H.instantiate(H.compose("train.yaml", ["experiment=smoke_shards", "+trainer.accumulate_grad_batches=0"]).trainer)


# ---------------------------------------------------------------------------------------------- host expressions
THIRD = 1.0 / 3.0      # ops passes it on as fp32: 0x3eaaaaab


def test_host_expressions_round_twice():
    """acc = 637, g = 850, scale = fl32(1/3): the product rounds to 283.33334, the sum to 920.33337; one fused rounding of
    637 + 850 * fl32(1/3) gives 920.3333 (one ulp less)."""
    two_roundings, fused = 920.3333740234375, 920.33331298828125
    s32 = torch.tensor(THIRD, dtype=torch.float32)
    exact = s32.double() * 850.0 + 637.0            # exact in fp64: 24-bit x 10-bit product, small sum
    assert float(exact.float()) == fused and fused != two_roundings
    prod = float(torch.tensor(850.0) * s32)
    acc, g = torch.tensor([637.0, 1.0, -2.0]), torch.tensor([850.0, 3.0, 8.0])
    # mode 1: acc += scale * g
    a, gg = acc.clone(), g.clone()
    ops.grad_accumulate(a, gg, 3, THIRD, 1)
    assert a.tolist() == [two_roundings, 2.0, float(torch.tensor(-2.0) + torch.tensor(8.0) * s32)] and torch.equal(gg, g)
    # mode 0: acc = scale * g, whatever acc held
    a = torch.full((3,), float("nan"))
    ops.grad_accumulate(a, gg, 3, THIRD, 0)
    assert a.tolist() == [prod, 1.0, float(torch.tensor(8.0) * s32)] and torch.equal(gg, g)
    # mode 2: grads = acc + scale * g, acc untouched
    a, gg = acc.clone(), g.clone()
    ops.grad_accumulate(a, gg, 3, THIRD, 2)
    assert gg.tolist()[:2] == [two_roundings, 2.0] and torch.equal(a, acc)
    # mode 2 without acc (a group of one): grads = scale * g
    gg = g.clone()
    ops.grad_accumulate(None, gg, 3, THIRD, 2)
    assert gg.tolist()[:2] == [prod, 1.0]
    # n limits the range; the sums of squares of the new gradient ride along in mode 2
    a, gg, part = acc.clone(), g.clone(), torch.full((1024,), float("nan"), dtype=torch.float64)
    ops.grad_accumulate(a, gg, 2, 0.5, 2, part)
    assert gg.tolist() == [637.0 + 425.0, 2.5, 8.0]
    assert float(part.sum()) == (637.0 + 425.0) ** 2 + 2.5 ** 2


def test_host_wrapper_validates():
    a, g = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError, match="mode"):
        ops.grad_accumulate(a, g, 4, 0.5, 3)
    with pytest.raises(ValueError, match="acc"):
        ops.grad_accumulate(None, g, 4, 0.5, 0)
    with pytest.raises(ValueError, match="mode 2"):
        ops.grad_accumulate(a, g, 4, 0.5, 1, torch.zeros(1024, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.grad_accumulate(a.double(), g, 4, 0.5, 1)
    with pytest.raises(ValueError):
        ops.grad_accumulate(a, g, 5, 0.5, 1)


def test_accumulator_allocates_only_when_it_accumulates():
    store = SimpleNamespace(total=8, grad=torch.arange(8, dtype=torch.float32))
    one = optim.GradAccumulator(store, 1)
    one.fold(True, True)
    assert one.acc is None and torch.equal(store.grad, torch.arange(8, dtype=torch.float32))
    two = optim.GradAccumulator(store, 2)
    assert two.acc is None
    two.fold(True, True)                        # a group of one at N = 2: scaled, still no buffer
    assert two.acc is None and torch.equal(store.grad, torch.arange(8, dtype=torch.float32) * 0.5)
    two.fold(True, False)
    assert two.acc is not None and two.acc.numel() == 8
    # ranges that touch or overlap are folded once
    store.grad.copy_(torch.ones(8))
    cb = two.hook(False, True)
    cb(4, 8); cb(2, 6); cb(2, 4)
    two.fold_rest(False, True)
    assert torch.equal(store.grad, torch.arange(8, dtype=torch.float32) * 0.25 + 0.5)


# ---------------------------------------------------------------------------------------------- two gloo ranks
def _fill(rank: int, micro: int) -> torch.Tensor:
    return ((torch.arange(1000) * (rank + 2) + 7 * micro) % 64 - 20).float() * 2      # small even integers: halves are exact


def _worker(rank, world, port, ret):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, optim
    flat = torch.zeros(1000, dtype=torch.float32)
    red = comm.GradBucketReducer(flat, bucket_floats=256)
    acc = optim.GradAccumulator(SimpleNamespace(total=1000, grad=flat), 2)
    out = {}
    for micro in range(2):
        first, last = micro == 0, micro == 1
        flat.copy_(_fill(rank, micro))
        cb = acc.hook(first, last, red.bucket_ready)
        for lo, hi in ((900, 1000), (700, 900), (300, 700)):        # (0, 300) is never announced
            cb(lo, hi)
        acc.fold_rest(first, last)
        if last:
            red.finish()
        else:
            out["launched_after_0"] = list(red.launched) + list(red.works)
            out["flat_after_0"] = flat.clone().numpy()
            out["acc_after_0"] = acc.acc.clone().numpy()
    out["flat"] = flat.numpy()
    out["acc"] = acc.acc.numpy()
    ret[rank] = out
    dist.destroy_process_group()


def test_two_gloo_ranks_reduce_only_the_groups_sum():
    world = 2
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, 29671, ret), nprocs=world, join=True)
        res = dict(ret)
    want = sum(0.5 * _fill(r, 0) + 0.5 * _fill(r, 1) for r in range(world))
    assert float(want[:300].abs().sum()) > 0
    for r in range(world):
        assert res[r]["launched_after_0"] == []                                     # no collective on a non-final micro-batch
        assert torch.equal(torch.from_numpy(res[r]["flat_after_0"]), _fill(r, 0))     # its gradient is left as backward wrote it
        assert torch.equal(torch.from_numpy(res[r]["acc_after_0"]), 0.5 * _fill(r, 0))    # the hole (0, 300) included
        assert torch.equal(torch.from_numpy(res[r]["flat"]), want)                  # every range folded AND reduced
        assert torch.equal(torch.from_numpy(res[r]["acc"]), 0.5 * _fill(r, 0))      # the last fold does not write acc
