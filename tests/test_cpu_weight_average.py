"""Weight averaging without a device: the update schedule against a written-out table, the host expressions of
``ops.weight_average`` against ``torch.optim.swa_utils.AveragedModel`` (the oracle of the GPU test), every refusal, the Trainer
and Hydra surface, the checkpoint layout and the three resume cases on a host-side ParamStore, and the entry points of the
library."""
import pytest
import torch

from tests import _wavgcases as W


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, lock, model_configs as mc, ops, optim, params
    return comm, lock, mc, ops, optim, params


def _tiny_cfg():
    comm, lock, mc, ops, optim, params = _pkg()
    return mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))


def _store(seed=0, lock_image=False):
    """A ParamStore laid out on the host with random weights; no kernel runs (init=False)."""
    comm, lock, mc, ops, optim, params = _pkg()
    cfg = _tiny_cfg()
    st = params.ParamStore(cfg, torch.device("cpu"), init=False)
    for p in st.params.values():
        p._sc_store = st
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for sp in st.specs:
            st.master[sp.offset:sp.offset + sp.numel].copy_(torch.randn(sp.numel, generator=g))
    if lock_image:
        locked, free = lock.split_groups(lock.vision_groups(cfg.vision.layers), 0)
        st.unlock(free)
        st.lock(locked)
    return st


def _mask(st):
    m = torch.zeros(st.total, dtype=torch.bool)
    for lo, hi in st.trainable_ranges():
        m[lo:hi] = True
    return m


def _drive(st, opt, wa, steps, seed=1):
    """What an optimiser does as far as the averager sees it: change the trainable weights, call it behind every range."""
    g = torch.Generator().manual_seed(seed)
    snaps = []
    real = torch.zeros(st.total)            # the padding behind a parameter holds zeros and stays zero
    for sp in st.specs:
        real[sp.offset:sp.offset + sp.numel] = 1.0
    for _ in range(steps):
        opt.step_count += 1
        wa.begin_step(opt.step_count - 1)
        for lo, hi in opt.ranges:
            with torch.no_grad():
                st.master[lo:hi].add_(0.1 * torch.randn(hi - lo, generator=g) * real[lo:hi])
            wa.after_piece(lo, hi)
        snaps.append(st.master.detach().clone())
    return snaps


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("every,start", sorted(W.SCHEDULE_TABLE, key=str))
def test_update_schedule_matches_the_table(every, start):
    comm, lock, mc, ops, optim, params = _pkg()
    st = _store()
    wa = optim.WeightAverager(st, decay=0.9, update_every_n_steps=every, update_starting_at_step=start)
    assert [s for s in range(8) if wa.should_update(s)] == W.SCHEDULE_TABLE[(every, start)]
    assert [s for s in range(8) if W.updates(s, every, start)] == W.SCHEDULE_TABLE[(every, start)]      # the oracle's own
    opt = optim.FusedAdamW(list(st.params.values()))
    wa.attach(opt)
    p0 = st.master.detach().clone()
    seen = []
    for s in range(8):
        before = wa.n_averaged
        _drive(st, opt, wa, 1, seed=s)
        if wa.n_averaged != before:
            seen.append(s)
            assert wa.latest_update_step == s
    assert seen == W.SCHEDULE_TABLE[(every, start)] and wa.n_averaged == len(seen)
    assert not torch.equal(st.master, p0)


@pytest.mark.parametrize("kind", ["ema", "mean"])
@pytest.mark.parametrize("lock_image", [False, True], ids=["free", "locked-image-tower"])
def test_host_path_equals_the_oracle_over_the_snapshots(kind, lock_image):
    """The host expressions (what a host-side store evaluates) against AveragedModel fed with the snapshots: first update
    copies, later ones average; locked ranges keep the weights the averager was built on and are never touched."""
    comm, lock, mc, ops, optim, params = _pkg()
    st = _store(seed=2, lock_image=lock_image)
    opt = optim.FusedLion(list(st.params.values()))
    wa = optim.WeightAverager(st, decay=0.9, update_every_n_steps=2, update_starting_at_step=1, kind=kind).attach(opt)
    initial = st.master.detach().clone()
    mask = _mask(st)
    assert bool(mask.all()) != lock_image and wa.ranges == list(st.trainable_ranges())
    snaps = _drive(st, opt, wa, 7)
    want, n = W.oracle_run(snaps, kind, 0.9, 2, 1, initial, mask)
    assert wa.n_averaged == n == 3 and wa.latest_update_step == 6
    W.assert_same_bits(wa.avg, want, f"{kind} average over 7 steps")
    assert torch.equal(wa.avg[~mask], initial[~mask]) and torch.equal(st.master[~mask], initial[~mask])


@pytest.mark.parametrize("n", [1, 3, 64, 1028])
def test_host_expressions_on_special_values(n):
    comm, lock, mc, ops, optim, params = _pkg()
    for seed, decay in enumerate(W.DECAYS):
        avg, p = W.values(n, seed)
        got = avg.clone()
        ops.weight_average(got, p, n, ops.WAVG_EMA, decay, 1.0 - decay)
        W.assert_same_bits(got, W.oracle_update(avg, p, "ema", decay, 3), f"ema decay {decay} n {n}")
    for k in (1, 2, 7, 1000):
        avg, p = W.values(n, k)
        got = avg.clone()
        ops.weight_average(got, p, n, ops.WAVG_MEAN, float(k + 1))
        W.assert_same_bits(got, W.oracle_update(avg, p, "mean", 0.0, k), f"mean n_averaged {k} n {n}")
    avg, p = W.values(n, 9)
    got = avg.clone()
    ops.weight_average(got, p, n, ops.WAVG_COPY)
    W.assert_same_bits(got, W.oracle_update(avg, p, "ema", 0.5, 0), "copy")
    assert torch.equal(W.bits(got), W.bits(p))
    got = avg.clone()
    ops.weight_average(got, p, n, ops.WAVG_SKIP)
    assert torch.equal(W.bits(got), W.bits(avg))
    a, b = avg.clone(), p.clone()
    ops.swap_f32(a, b, n)
    assert torch.equal(W.bits(a), W.bits(p)) and torch.equal(W.bits(b), W.bits(avg))


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_names_its_argument(monkeypatch):
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd.trainer import Trainer
    st = _store()
    bad = [({"decay": -0.1}, "decay"), ({"decay": 1.5}, "decay"), ({"decay": "x"}, "decay"),
           ({"update_every_n_steps": 0}, "update_every_n_steps"), ({"update_every_n_steps": 1.5}, "update_every_n_steps"),
           ({"update_starting_at_epoch": 0}, "update_starting_at_epoch"), ({"device": "cpu"}, "device"),
           ({"kind": "swa"}, "kind"), ({"update_starting_at_step": -1}, "update_starting_at_step")]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            optim.WeightAverager(st, **kw)
        with pytest.raises(ValueError, match=name):
            Trainer(callbacks={"weight_averaging": kw})
    for ok in ({"decay": 0}, {"decay": 1}, {"decay": 1.0, "update_every_n_steps": 3, "update_starting_at_step": 0},
               {"update_starting_at_epoch": None, "device": None, "kind": "mean"}):
        optim.WeightAverager(st, **ok)
    with pytest.raises(ValueError, match="decya"):
        Trainer(callbacks={"weight_averaging": {"decya": 0.9}})
    with pytest.raises(ValueError, match="weight_averaging"):
        Trainer(callbacks={"weight_averaging": 0.999})
    # fp8: the delayed activation scales belong to the training weights
    with pytest.raises(ValueError, match="(?s)weight_averaging.*fp8"):
        Trainer(precision="fp8-mixed", callbacks={"weight_averaging": {}})
    st8 = _store()
    st8.fp8 = True
    with pytest.raises(ValueError, match="(?s)weight_averaging.*fp8"):
        optim.WeightAverager(st8)
    # the sharded exchange: by the switch at construction, and by what the optimiser holds at attach
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    assert comm.grad_exchange_mode() == "sharded"
    with pytest.raises(ValueError, match="(?s)weight_averaging.*SC_GRAD_EXCHANGE=sharded"):
        Trainer(callbacks={"weight_averaging": {}})
    monkeypatch.delenv("SC_GRAD_EXCHANGE")
    opt = optim.FusedAdamW(list(st.params.values()))
    opt.exchange = object()
    with pytest.raises(ValueError, match="(?s)weight_averaging.*sharded"):
        optim.WeightAverager(st).attach(opt)
    assert opt.averager is None
    other = optim.FusedAdamW(list(_store().params.values()))
    with pytest.raises(ValueError, match="another ParamStore"):
        optim.WeightAverager(st).attach(other)


# ------------------------------------------------------------------------------------------------ Trainer and Hydra
def test_trainer_reads_the_callback_and_builds_nothing_without_it():
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd.trainer import Trainer
    tr = Trainer(callbacks={"weight_averaging": {"decay": 0.99, "update_every_n_steps": 10}})
    assert tr.weight_averaging == {"decay": 0.99, "update_every_n_steps": 10, "update_starting_at_step": None, "kind": "ema"}
    assert tr.weight_averager is None           # built by fit(), behind the optimiser
    tr = Trainer(callbacks={"weight_averaging": {}})
    assert tr.weight_averaging == {"decay": 0.999, "update_every_n_steps": 1, "update_starting_at_step": None, "kind": "ema"}
    for cbs in (None, {}, {"model_checkpoint": {"dirpath": "/tmp/x"}}):
        tr = Trainer(callbacks=cbs)
        assert tr.weight_averaging is None and tr.weight_averager is None
    opt = optim.FusedAdamW(list(_store().params.values()))
    assert opt.averager is None


def test_hydra_composes_the_callback_group_and_the_experiment(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    from spatial_clip_amd.trainer import Trainer
    base = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    default = H.compose("train.yaml", ["callbacks=default"])
    want = {"kind": "ema", "decay": 0.999, "update_every_n_steps": 1, "update_starting_at_step": None}
    for over in (["callbacks=ema"], ["experiment=vitb16_gene_b256_ema"]):
        cfg = H.compose("train.yaml", over)
        assert cfg["_choices_"]["callbacks"] == "ema"
        cbs = dict(cfg["callbacks"])
        assert dict(cbs["weight_averaging"]) == want
        assert {k: dict(v) for k, v in cbs.items() if k != "weight_averaging"} == {k: dict(v) for k, v in default["callbacks"].items()}
        assert optim.check_weight_averaging_cfg(cbs["weight_averaging"]) == \
            {"decay": 0.999, "update_every_n_steps": 1, "update_starting_at_step": None, "kind": "ema"}
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_ema"])
    assert cfg["model"]["net"] == base["model"]["net"] and cfg.data.batch_size == 256 and cfg["optimizer"] == base["optimizer"]
    assert cfg["loss"] == base["loss"] and cfg["trainer"] == base["trainer"]
    assert not base.get("callbacks") or "weight_averaging" not in base["callbacks"]
    cfg = H.compose("train.yaml", ["callbacks=ema", "callbacks.weight_averaging.kind=mean",
                                   "callbacks.weight_averaging.update_every_n_steps=10"])
    tr = Trainer(callbacks=dict(cfg["callbacks"]))
    assert tr.weight_averaging["kind"] == "mean" and tr.weight_averaging["update_every_n_steps"] == 10
    text = open(H.__file__.replace("hydra_lite.py", "configs/callbacks/ema.yaml")).read()
    assert "lightning.pytorch.callbacks.EMAWeightAveraging" in text


# ------------------------------------------------------------------------------------------------ checkpoints
class _Net:
    """What Trainer.save_checkpoint / load_checkpoint reach through ``model.net``, over a host-side store."""

    def __init__(self, st):
        self.store = st

    def state_dict(self):
        return self.store.state_dict()

    def _put(self, sd):
        with torch.no_grad():
            for sp in self.store.specs:
                self.store.master[sp.offset:sp.offset + sp.numel].view(sp.shape).copy_(sd[sp.name])

    def load_checkpoint_state_dict(self, ck, source=""):
        self._put(ck["state_dict"])

    def load_state_dict(self, sd):
        self._put(sd)


class _Model:
    device = torch.device("cpu")

    def __init__(self, st):
        self.net = _Net(st)


def _averaged_run(tmp_path, steps=5):
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd.trainer import Trainer
    st = _store(seed=3)
    opt = optim.FusedLion(list(st.params.values()))
    wa = optim.WeightAverager(st, decay=0.9).attach(opt)
    _drive(st, opt, wa, steps)
    path = str(tmp_path / "averaged.ckpt")
    Trainer.save_checkpoint(path, _Model(st), opt, None, steps)
    return st, opt, wa, path


def test_checkpoint_layout(tmp_path):
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd.trainer import Trainer
    st, opt, wa, path = _averaged_run(tmp_path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck) == ["state_dict", "global_step", "optimizer", "weight_averaging"]
    entry = ck["weight_averaging"]
    assert list(entry) == ["current_model_state", "n_averaged", "latest_update_step", "kind", "decay"]
    assert (entry["n_averaged"], entry["latest_update_step"], entry["kind"], entry["decay"]) == (5, 4, "ema", 0.9)
    names = [sp.name for sp in st.specs]
    assert list(ck["state_dict"]) == names == list(entry["current_model_state"])
    for sp in st.specs:
        s = slice(sp.offset, sp.offset + sp.numel)
        assert torch.equal(ck["state_dict"][sp.name].flatten(), wa.avg[s]), sp.name               # what was validated
        assert torch.equal(entry["current_model_state"][sp.name].flatten(), st.master[s]), sp.name
    assert not torch.equal(wa.avg, st.master)
    # while nothing has been averaged, state_dict carries the model's weights
    st0 = _store(seed=3)
    opt0 = optim.FusedLion(list(st0.params.values()))
    wa0 = optim.WeightAverager(st0, update_starting_at_step=100).attach(opt0)
    _drive(st0, opt0, wa0, 2)
    assert wa0.n_averaged == 0 and not torch.equal(wa0.avg, st0.master)
    p0 = str(tmp_path / "not_yet.ckpt")
    Trainer.save_checkpoint(p0, _Model(st0), opt0, None, 2)
    ck0 = torch.load(p0, map_location="cpu", weights_only=False)
    assert ck0["weight_averaging"]["n_averaged"] == 0 and ck0["weight_averaging"]["latest_update_step"] == -1
    for sp in st0.specs:
        assert torch.equal(ck0["state_dict"][sp.name].flatten(), st0.master[sp.offset:sp.offset + sp.numel])
    # without the callback the file has the keys it always had
    st1 = _store(seed=3)
    opt1 = optim.FusedLion(list(st1.params.values()))
    p1 = str(tmp_path / "plain.ckpt")
    Trainer.save_checkpoint(p1, _Model(st1), opt1, None, 0)
    assert list(torch.load(p1, map_location="cpu", weights_only=False)) == ["state_dict", "global_step", "optimizer"]


def test_the_three_resume_cases(tmp_path):
    comm, lock, mc, ops, optim, params = _pkg()
    from spatial_clip_amd.trainer import Trainer
    st, opt, wa, path = _averaged_run(tmp_path)
    # 1. averaging on, a file with the entry: masters <- current_model_state, average <- state_dict, counters restored
    st1 = _store(seed=8)
    opt1 = optim.FusedLion(list(st1.params.values()))
    wa1 = optim.WeightAverager(st1, decay=0.9).attach(opt1)
    assert Trainer.load_checkpoint(path, _Model(st1), opt1, None) == 5
    assert torch.equal(st1.master, st.master) and torch.equal(wa1.avg, wa.avg)
    assert (wa1.n_averaged, wa1.latest_update_step, opt1.step_count) == (5, 4, 5)
    more, more1 = _drive(st, opt, wa, 2, seed=77), _drive(st1, opt1, wa1, 2, seed=77)     # and it goes on as the first run does
    assert torch.equal(more[-1], more1[-1]) and torch.equal(wa1.avg, wa.avg) and wa1.n_averaged == wa.n_averaged == 7
    with pytest.raises(ValueError, match="kind"):
        wm = optim.WeightAverager(st1, kind="mean").attach(opt1)
        Trainer.load_checkpoint(path, _Model(st1), opt1, None)
    # 2. averaging on, a file without the entry: the average starts as a copy of the loaded weights
    st, opt, wa, path = _averaged_run(tmp_path)
    plain = str(tmp_path / "plain.ckpt")
    stp = _store(seed=4)
    Trainer.save_checkpoint(plain, _Model(stp), optim.FusedLion(list(stp.params.values())), None, 3)
    st2 = _store(seed=9)
    opt2 = optim.FusedLion(list(st2.params.values()))
    wa2 = optim.WeightAverager(st2).attach(opt2)
    wa2.n_averaged, wa2.latest_update_step = 4, 3
    Trainer.load_checkpoint(plain, _Model(st2), opt2, None)
    assert torch.equal(st2.master, stp.master) and torch.equal(wa2.avg, stp.master)
    assert (wa2.n_averaged, wa2.latest_update_step) == (0, -1)
    # 3. a file with the entry, fit without averaging: trains on from current_model_state; test / eval read state_dict
    st3 = _store(seed=10)
    opt3 = optim.FusedLion(list(st3.params.values()))
    Trainer.load_checkpoint(path, _Model(st3), opt3, None)
    assert opt3.averager is None and torch.equal(st3.master, st.master) and not torch.equal(st3.master, wa.avg)
    st4 = _store(seed=11)
    Trainer.load_checkpoint(path, _Model(st4))
    assert torch.equal(st4.master, wa.avg)


# ------------------------------------------------------------------------------------------------ the library
def test_the_entry_points_exist_in_the_library():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib
    declared = _lib.parse_header()
    for name in ("sc_weight_average", "sc_weight_average_dev", "sc_swap_f32"):
        assert name in declared, f"{name} is not declared in include/spatial_clip_hip.h"
        assert getattr(_lib.lib(), name) is not None
    assert len(declared["sc_weight_average"][1]) == 7 and len(declared["sc_weight_average_dev"][1]) == 5
    assert len(declared["sc_swap_f32"][1]) == 4
    assert _lib.lib().sc_weight_average_pass_floats() > 0 and _lib.lib().sc_abi_version() == 1
