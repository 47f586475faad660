"""Cached-feature gradient accumulation (Trainer accum_freq; open_clip's --accum-freq) without a GPU: the epoch arithmetic
(open_clip's: n // N optimiser steps, the tail that fills no group dropped), what is sized from it, and every refusal that
``Trainer.__init__`` / the first lines of ``fit`` can raise on a host."""
from types import SimpleNamespace

import pytest
import torch

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd import optim, trainer as T


def test_steps_per_epoch_is_floor_division():
    assert [T.group_steps_per_epoch(n, 2) for n in range(6)] == [0, 0, 1, 1, 2, 2]
    assert T.group_steps_per_epoch(5, 1) == 5 and T.group_steps_per_epoch(12, 4) == 3 and T.group_steps_per_epoch(3, 4) == 0
    # Lightning's rule for accumulate_grad_batches steps on the short tail instead
    assert T.steps_per_epoch(5, 2) == 3 and T.group_steps_per_epoch(5, 2) == 2


def test_which_batches_close_a_group_and_the_dropped_tail():
    closes = lambda n, N: [i for i, c in enumerate(T.group_closes_after(n, N)) if c]
    assert closes(5, 2) == [1, 3] and T.group_dropped_tail(5, 2) == 1
    assert closes(4, 4) == [3] and T.group_dropped_tail(4, 4) == 0
    assert closes(3, 4) == [] and T.group_dropped_tail(3, 4) == 3         # fewer batches than one group: nothing ever steps
    assert closes(7, 3) == [2, 5] and T.group_dropped_tail(7, 3) == 1
    assert closes(4, 1) == [0, 1, 2, 3] and T.group_dropped_tail(4, 1) == 0
    assert T.group_closes_after(0, 3) == []
    for n in range(0, 14):
        for N in range(1, 6):
            c = T.group_closes_after(n, N)
            assert len(c) == n and sum(c) == T.group_steps_per_epoch(n, N)
            assert not any(c[n - T.group_dropped_tail(n, N):])                 # no batch of the tail closes anything


def test_resume_position_counts_whole_groups():
    # 5 batches, N = 2: 2 steps per epoch (batches 0-1, 2-3; batch 4 dropped)
    assert T.group_resume_position(0, 5, 2) == (0, 0)
    assert T.group_resume_position(1, 5, 2) == (0, 2)
    assert T.group_resume_position(2, 5, 2) == (1, 0)       # the epoch-end checkpoint: the dropped tail is not revisited
    assert T.group_resume_position(3, 5, 2) == (1, 2)
    assert T.group_resume_position(7, 12, 4) == (2, 4)
    assert T.group_resume_position(7, 5, 1) == T.resume_position(7, 5, 1) == (1, 2)
    for step in range(0, 20):
        epoch, skip = T.group_resume_position(step, 7, 3)
        assert skip % 3 == 0 and skip < 6 and epoch * 2 + skip // 3 == step     # never inside a group


def test_estimated_stepping_batches():
    assert T.group_estimated_stepping_batches(5, 2, 3) == 6
    assert T.group_estimated_stepping_batches(5, 2, 3, max_steps=4) == 4
    assert T.group_estimated_stepping_batches(12, 4, 1) == 3


class _FiveBatches:
    """The least of a data module that ``Trainer.fit`` touches before its first batch."""
    preprocess_fn = tokenizer = None

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [None] * 5


class _Stop(Exception):
    pass


class _Model:
    net = SimpleNamespace(preprocess_train=None, tokenizer=None, precision="bf16")

    def check_cached_accumulation(self, n):
        pass

    def configure_optimizers(self):     # fit() has sized the schedule by the time it asks for the optimiser
        raise _Stop


def test_fit_sizes_the_schedule_in_optimiser_steps():
    tr = T.Trainer(max_epochs=3, accum_freq=2)
    assert tr.accum_freq == 2 and tr.accumulate_grad_batches == 1
    with pytest.raises(_Stop):
        tr.fit(_Model(), _FiveBatches())
    assert tr.estimated_stepping_batches == 6
    tr = T.Trainer(max_epochs=3, accum_freq=2, max_steps=5)
    with pytest.raises(_Stop):
        tr.fit(_Model(), _FiveBatches())
    assert tr.estimated_stepping_batches == 5


def test_fewer_batches_than_one_group_is_refused_by_fit():
    tr = T.Trainer(max_epochs=1, accum_freq=6)
    with pytest.raises(ValueError, match="accum_freq=6") as e:
        tr.fit(_Model(), _FiveBatches())
    assert "5 training batches" in str(e.value)
    tr = T.Trainer(max_epochs=1, accum_freq=4, limit_train_batches=3)
    with pytest.raises(ValueError, match="accum_freq=4"):
        tr.fit(_Model(), _FiveBatches())


@pytest.mark.parametrize("bad", [0, -1, 2.5, 1.0, "2", None, True, {0: 2}])
def test_refused_values_name_the_argument(bad):
    with pytest.raises(ValueError, match="accum_freq") as e:
        T.Trainer(accum_freq=bad)
    assert "integer >= 1" in str(e.value) and repr(bad) in str(e.value)


def test_the_two_forms_do_not_nest():
    with pytest.raises(ValueError, match="accum_freq=2") as e:
        T.Trainer(accum_freq=2, accumulate_grad_batches=3)
    assert "accumulate_grad_batches=3" in str(e.value)
    assert T.Trainer(accum_freq=1, accumulate_grad_batches=3).accumulate_grad_batches == 3
    assert T.Trainer(accum_freq=3, accumulate_grad_batches=1).accum_freq == 3


def test_fp8_is_refused():
    with pytest.raises(ValueError, match="accum_freq=2") as e:
        T.Trainer(accum_freq=2, precision="fp8-mixed")
    assert "fp8" in str(e.value)
    assert T.Trainer(accum_freq=1, precision="fp8-mixed").precision == "fp8"


def test_sharded_exchange_is_refused(monkeypatch):
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    with pytest.raises(ValueError, match="SC_GRAD_EXCHANGE") as e:
        T.Trainer(accum_freq=2)
    assert "accum_freq=2" in str(e.value)
    assert T.Trainer(accum_freq=1).accum_freq == 1
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "allreduce")
    assert T.Trainer(accum_freq=2).accum_freq == 2


def test_a_process_group_is_refused_before_it_is_joined(monkeypatch):
    with pytest.raises(ValueError, match="accum_freq=2") as e:
        T.Trainer(accum_freq=2, devices=2, strategy="ddp")          # asked for by the config
    assert "2 ranks" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "4")                           # described by the launcher
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match="accum_freq=3") as e:
        T.Trainer(accum_freq=3)
    assert "4 ranks" in str(e.value)


def test_distillation_is_refused():
    """``module.check_cached_accumulation`` (called by fit and by the group step) on a module-shaped object: host only."""
    from spatial_clip_amd import losses, module
    host = SimpleNamespace(dist_net=None, loss_fn=losses.DistillClipLoss(), net=SimpleNamespace(precision="bf16"))
    with pytest.raises(ValueError, match="accum_freq=2") as e:
        module.SpatialClipLitModule.check_cached_accumulation(host, 2)
    assert "DistillClipLoss" in str(e.value)
    host = SimpleNamespace(dist_net=object(), loss_fn=losses.ClipLoss(), net=SimpleNamespace(precision="bf16"))
    with pytest.raises(ValueError, match="dist_net"):
        module.SpatialClipLitModule.check_cached_accumulation(host, 2)
    host = SimpleNamespace(dist_net=None, loss_fn=losses.ClipLoss(), net=SimpleNamespace(precision="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        module.SpatialClipLitModule.check_cached_accumulation(host, 4)
    for ok in (losses.ClipLoss(), losses.SpatialLoss(), losses.SigLipLoss()):
        module.SpatialClipLitModule.check_cached_accumulation(
            SimpleNamespace(dist_net=None, loss_fn=ok, net=SimpleNamespace(precision="bf16")), 2)


def test_default_is_one_and_changes_nothing():
    a, b = T.Trainer(), T.Trainer(accum_freq=1)
    assert a.accum_freq == 1 and a.accumulator is None
    assert vars(a) == vars(b)


def test_accumulator_at_scale_one():
    store = SimpleNamespace(total=4, grad=torch.tensor([1.0, 2.0, 3.0, 4.0]))
    acc = optim.GradAccumulator(store, 3, scale=1.0)
    assert acc.scale == 1.0 and optim.GradAccumulator(store, 3).scale == 1.0 / 3
    acc.fold(True, False)
    store.grad.copy_(torch.tensor([10.0, 20.0, 30.0, 40.0]))
    acc.fold(False, False)
    store.grad.copy_(torch.tensor([100.0, 200.0, 300.0, 400.0]))
    acc.fold(False, True)
    assert store.grad.tolist() == [111.0, 222.0, 333.0, 444.0]          # the plain sum: the group loss is already a mean


def test_hydra_key_reaches_the_trainer(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    from spatial_clip_amd import hydra_lite as H
    tr = H.instantiate(H.compose("train.yaml", ["experiment=smoke_shards", "+trainer.accum_freq=4"]).trainer)
    assert tr.accum_freq == 4
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b64_cached4"])
    assert cfg.trainer.accum_freq == 4 and cfg.data.batch_size == 64
    assert cfg.model.net.model_name == "ViT-B-16-gene"
    assert H.instantiate(cfg.trainer).accum_freq == 4
    with pytest.raises(ValueError, match="accum_freq"):
        H.instantiate(H.compose("train.yaml", ["experiment=smoke_shards", "+trainer.accum_freq=0"]).trainer)
