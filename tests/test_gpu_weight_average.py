"""Weight averaging on the device (``optim.WeightAverager``; sc_weight_average, sc_weight_average_dev, sc_swap_f32).

The oracle is torch on the CPU, ``torch.optim.swa_utils.AveragedModel`` fed with snapshots of the weights
(tests/_wavgcases.py); every comparison is bit for bit (NaNs compare equal to NaNs, see there).  Kernels first -- every op at
sizes around the vector width, one past a full trip of the grid, misaligned pointers, special values, the device-control form
against the host form, the exchange -- then the averager through every form of the optimiser step on the tiny gene model of the
Lion and LAMB tests, a graph replay without a host sync, validation on the average, checkpoint and resume, the refusals."""
import functools

import pytest
import torch

from tests import _wavgcases as W

pytestmark = pytest.mark.gpu


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, ops
    return _lib, ops


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, optim, streams
    return data, graph, losses, mc, module, net, optim, streams


def _ctl(ops, op, a=0.0, b=0.0):
    import struct
    bits = struct.unpack("<2i", struct.pack("<2f", a, b))
    return torch.tensor([op, bits[0], bits[1], 0], dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=4)
def _values(n, seed):
    """tests/_wavgcases.values, never written; one draw serves every op at the size past a trip of the grid."""
    return W.values(n, seed if n <= 4096 else 0)


def _pairs(n, seed, offsets=(0, 0)):
    """(avg, p) on the host and device views of them that start ``offsets`` floats into 16-byte aligned buffers."""
    avg, p = _values(n, seed)
    bufs = [torch.zeros(n + 8, dtype=torch.float32).cuda() for _ in range(2)]
    views = [buf[o:o + n] for buf, o in zip(bufs, offsets)]
    views[0].copy_(avg)
    views[1].copy_(p)
    return avg, p, views[0], views[1], bufs


def _op_cases():
    _lib, ops = _ops()
    cases = [("copy", ops.WAVG_COPY, 0.0, 0.0, ("ema", 0.5, 0))]
    for d in W.DECAYS:
        cases.append((f"ema {d}", ops.WAVG_EMA, d, 1.0 - d, ("ema", d, 2)))
    for k in (1, 9):
        cases.append((f"mean {k}", ops.WAVG_MEAN, float(k + 1), 0.0, ("mean", 0.0, k)))
    return cases


# ================================================================================================ kernels
@pytest.mark.parametrize("n", list(W.SMALL_SIZES) + ["one-trip-of-the-grid+4"])
def test_kernel_equals_the_cpu_oracle_bit_for_bit(n):
    _lib, ops = _ops()
    if not isinstance(n, int):
        n = ops.weight_average_pass_floats() + 4
        assert n == 16384 * 256 * 4 + 4             # blocks x threads x floats per vector: the launch constants
    for seed, (name, op, a, b, oracle) in enumerate(_op_cases()):
        avg, p, da, dp, bufs = _pairs(n, seed)
        ops.weight_average(da, dp, n, op, a, b)
        W.assert_same_bits(da, W.oracle_update(avg, p, *oracle), f"n {n} {name}")
        assert torch.equal(W.bits(dp), W.bits(p)), "params were written"
        assert float(bufs[0][n:].abs().max()) == 0.0, "written past n"


@pytest.mark.parametrize("offsets", [(1, 1), (1, 0), (0, 3)], ids=["both+1", "avg+1", "params+3"])
def test_pointers_that_are_only_4_byte_aligned(offsets):
    _lib, ops = _ops()
    n = 1028
    for seed, (name, op, a, b, oracle) in enumerate(_op_cases()):
        avg, p, da, dp, bufs = _pairs(n, seed, offsets)
        assert (da.data_ptr() | dp.data_ptr()) % 16 != 0
        ops.weight_average(da, dp, n, op, a, b)
        W.assert_same_bits(da, W.oracle_update(avg, p, *oracle), f"offsets {offsets} {name}")
        dev = da.clone()
        da.copy_(avg)
        ops.weight_average_dev(da, dp, n, _ctl(ops, op, a, b))
        assert torch.equal(W.bits(da), W.bits(dev)), f"offsets {offsets} {name}: device form differs from the host form"
        assert float(bufs[0][:offsets[0]].abs().sum()) == 0.0 and float(bufs[0][offsets[0] + n:].abs().sum()) == 0.0


@pytest.mark.parametrize("n", list(W.SMALL_SIZES) + ["one-trip-of-the-grid+4"])
def test_device_form_has_the_bits_of_the_host_form(n):
    _lib, ops = _ops()
    if not isinstance(n, int):
        n = ops.weight_average_pass_floats() + 4
    for seed, (name, op, a, b, _) in enumerate(_op_cases()):
        avg, p, da, dp, _ = _pairs(n, seed)
        ops.weight_average(da, dp, n, op, a, b)
        host = da.clone()
        da.copy_(avg)
        ops.weight_average_dev(da, dp, n, _ctl(ops, op, a, b))
        assert torch.equal(W.bits(da), W.bits(host)), f"n {n} {name}"       # same code on the same GPU: NaN payloads included
    # skip: a poisoned average is untouched, by both forms
    poison = torch.full((n,), float("nan")).cuda()
    poison.view(torch.int32).fill_(0x7FC12345)
    want = W.bits(poison).clone()
    p = torch.randn(n).cuda()
    ops.weight_average_dev(poison, p, n, _ctl(ops, ops.WAVG_SKIP, 0.5, 0.5))
    ops.weight_average(poison, p, n, ops.WAVG_SKIP, 0.5, 0.5)
    assert torch.equal(W.bits(poison), want)


@pytest.mark.parametrize("n", list(W.SMALL_SIZES) + ["one-trip-of-the-grid+4"])
def test_swap_exchanges_exactly_and_twice_is_the_identity(n):
    _lib, ops = _ops()
    if not isinstance(n, int):
        n = ops.weight_average_pass_floats() + 4
    for offsets in ((0, 0), (1, 2)) if n == 1028 else ((0, 0),):
        a, b, da, db, bufs = _pairs(n, 3, offsets)
        ops.swap_f32(da, db, n)
        assert torch.equal(W.bits(da), W.bits(b)) and torch.equal(W.bits(db), W.bits(a))
        ops.swap_f32(da, db, n)
        assert torch.equal(W.bits(da), W.bits(a)) and torch.equal(W.bits(db), W.bits(b))
        for buf, o in zip(bufs, offsets):
            assert float(buf[:o].abs().sum()) == 0.0 and float(buf[o + n:].abs().sum()) == 0.0


def test_argument_refusals_set_the_error_and_write_nothing():
    _lib, ops = _ops()
    lib = _lib.lib()
    E = _lib.SpatialClipHipError
    n = 128
    buf = torch.randn(2 * n).cuda()
    before = buf.clone()
    a, b = buf[:n], buf[n:]
    st = torch.cuda.current_stream().cuda_stream
    ctl = _ctl(ops, ops.WAVG_EMA, 0.5, 0.5)
    with pytest.raises(E, match="sc_swap_f32:.*overlap"):
        ops.swap_f32(buf[:n], buf[4:n + 4], n)
    with pytest.raises(E, match="sc_swap_f32:.*overlap"):
        ops.swap_f32(a, a, n)
    with pytest.raises(E, match="sc_weight_average:.*overlap"):
        ops.weight_average(buf[:n], buf[n - 1:2 * n - 1], n, ops.WAVG_EMA, 0.5, 0.5)
    with pytest.raises(E, match="sc_weight_average_dev:.*overlap"):
        ops.weight_average_dev(a, a, n, ctl)
    assert lib.sc_weight_average(a.data_ptr(), b.data_ptr(), n, 4, 0.5, 0.5, st) != 0 and b"op 4" in lib.sc_last_error()
    assert lib.sc_weight_average(a.data_ptr(), b.data_ptr(), n, -1, 0.5, 0.5, st) != 0
    assert lib.sc_weight_average(None, b.data_ptr(), n, 2, 0.5, 0.5, st) != 0 and b"required" in lib.sc_last_error()
    assert lib.sc_weight_average(a.data_ptr(), b.data_ptr(), -1, 2, 0.5, 0.5, st) != 0
    assert lib.sc_weight_average(a.data_ptr() + 2, b.data_ptr(), 8, 2, 0.5, 0.5, st) != 0 and b"aligned" in lib.sc_last_error()
    assert lib.sc_weight_average_dev(a.data_ptr(), b.data_ptr(), n, None, st) != 0 and b"ctl" in lib.sc_last_error()
    assert lib.sc_weight_average_dev(a.data_ptr(), None, n, ctl.data_ptr(), st) != 0
    assert lib.sc_swap_f32(a.data_ptr(), None, n, st) != 0 and b"required" in lib.sc_last_error()
    assert lib.sc_swap_f32(a.data_ptr() + 1, b.data_ptr(), 8, st) != 0
    # n == 0 launches nothing, also on buffers that would overlap
    assert lib.sc_weight_average(a.data_ptr(), a.data_ptr(), 0, 2, 0.5, 0.5, st) == 0
    assert lib.sc_weight_average_dev(a.data_ptr(), b.data_ptr(), 0, ctl.data_ptr(), st) == 0
    assert lib.sc_swap_f32(a.data_ptr(), a.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(W.bits(buf), W.bits(before))
    with pytest.raises(ValueError, match="op"):
        ops.weight_average(a, b, n, 7)
    with pytest.raises(TypeError, match="float32"):
        ops.weight_average(a.double(), b, n, ops.WAVG_COPY)
    with pytest.raises(ValueError, match="ctl"):
        ops.weight_average_dev(a, b, n, ctl.float())


# ================================================================================================ through the optimiser
DECAY, EVERY, START, STEPS = 0.9, 2, 1, 5
OPTIMIZERS = {
    "adamw": lambda optim: functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
    "lion": lambda optim: functools.partial(optim.FusedLion, lr=1e-4, betas=(0.9, 0.99), weight_decay=1.0),
    "lamb": lambda optim: functools.partial(optim.FusedLamb, lr=1e-3, weight_decay=0.01),
}
FORMS = ("one_launch", "behind", "graph", "groups", "lock", "accum")


def _net(seed=3, lock_image=False):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    if lock_image:
        n.lock_image_tower(0)
    return n


def _two_groups(net_):
    """Two parameter groups with the optimiser's own lr and weight decay: the grouped launches, the ungrouped step's weights."""
    st = net_.store
    named = [(n, p) for n, p in st.params.items() if p.requires_grad]
    halves = [[(n, p) for n, p in named if n.startswith("visual.")], [(n, p) for n, p in named if not n.startswith("visual.")]]
    return [{"params": [p for _, p in h], "param_names": [n for n, _ in h]} for h in halves if h]


def _module(n, kind, param_groups=None, warmup=2, total=40):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), OPTIMIZERS[kind](optim),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=warmup), param_groups=param_groups)

    class T:
        max_steps, max_epochs, estimated_stepping_batches = total, None, total
    m.trainer = T()
    oc = m.configure_optimizers()
    return m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _batch(step, B=12):
    data, *_ = _pkg()
    return {k: v.cuda() for k, v in data.synthetic_batch(B, 32, 200, K=4, step=step).items()}


def _trainable_mask(store):
    mask = torch.zeros(store.total, dtype=torch.bool)
    for lo, hi in store.trainable_ranges():
        mask[lo:hi] = True
    return mask


def _run_form(form, kind, monkeypatch, avg_kind="ema"):
    """STEPS optimiser steps of one form with the averager attached; returns the snapshots of the weights after every step,
    the average, the averager, the initial weights and the trainable mask."""
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    monkeypatch.setenv("SC_ADAMW_BEHIND", "1" if form == "behind" else "0")
    n = _net(lock_image=form == "lock")
    m, opt, sched = _module(n, kind, _two_groups if form == "groups" else None)
    st = n.store
    if form == "groups":
        assert len(opt.param_groups) == 2
    wa = optim.WeightAverager(st, decay=DECAY, update_every_n_steps=EVERY, update_starting_at_step=START, kind=avg_kind).attach(opt)
    initial = st.master.detach().clone().cpu()
    gstep = graph.GraphedTrainStep(m, opt, max_norm=1.0)
    assert gstep.capturable() is None
    acc = optim.GradAccumulator(st, 2) if form == "accum" else None
    snaps = []
    for s in range(STEPS):
        if form == "accum":
            for j in (0, 1):
                with streams.chain_stream():
                    loss = m.training_step(_batch(2 * s + j), 0)
                    loss.backward(m.root_gradient(loss))
                    acc.fold(j == 0, j == 1)
                    if j == 1:
                        opt.step(grad_scale=1.0, max_norm=1.0)
        elif form == "graph":
            gstep(_batch(s))
        else:
            gstep.eager(_batch(s))
        sched.step()
        st.wait_all()
        snaps.append(st.master.detach().clone())
        torch.cuda.synchronize()        # (the unsynchronised replay has a test of its own below)
    if form == "graph":
        assert gstep.failed is None and gstep.replays == STEPS - 1, (gstep.failed, gstep.replays)
    assert opt.step_count == STEPS
    return [t.cpu() for t in snaps], wa.avg.detach().clone().cpu(), wa, initial, _trainable_mask(st)


@pytest.mark.parametrize("kind", list(OPTIMIZERS))
def test_every_step_form_averages_what_the_oracle_does(kind, monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BUCKET", "4096")
    runs = {form: _run_form(form, kind, monkeypatch) for form in FORMS}
    for form, (snaps, avg, wa, initial, mask) in runs.items():
        want, n_avg = W.oracle_run(snaps, "ema", DECAY, EVERY, START, initial, mask)
        assert wa.n_averaged == n_avg == 2 and wa.latest_update_step == 4, (form, wa.n_averaged)      # steps 2 (copy) and 4
        W.assert_same_bits(avg, want, f"{kind} {form}: average against the oracle over its own snapshots")
        assert not torch.equal(avg[mask], snaps[-1][mask]) and not torch.equal(avg[mask], initial[mask]), form
        if form == "lock":
            assert 0 < int(mask.sum()) < mask.numel()
            assert torch.equal(avg[~mask], initial[~mask]) and torch.equal(snaps[-1][~mask], initial[~mask])
    # within one optimiser the forms agree bit for bit wherever the weights do
    first = runs["one_launch"]
    for form in ("behind", "graph"):
        assert all(torch.equal(a, b) for a, b in zip(first[0], runs[form][0])), f"{kind} {form}: weights differ from one_launch"
        assert torch.equal(W.bits(first[1]), W.bits(runs[form][1])), f"{kind} {form}: average differs from one_launch"
    if all(torch.equal(a, b) for a, b in zip(first[0], runs["groups"][0])):
        assert torch.equal(W.bits(first[1]), W.bits(runs["groups"][1])), f"{kind} groups: average differs from one_launch"
    for form in ("accum", "lock"):      # other weights by construction
        assert not torch.equal(first[0][-1], runs[form][0][-1])


def test_mean_kind_through_the_graph(monkeypatch):
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_ADAMW_BUCKET", "4096")
    out = {}
    for form in ("behind", "graph"):
        snaps, avg, wa, initial, mask = _run_form(form, "lion", monkeypatch, avg_kind="mean")
        want, n_avg = W.oracle_run(snaps, "mean", DECAY, EVERY, START, initial, mask)
        assert wa.n_averaged == n_avg == 2
        W.assert_same_bits(avg, want, f"mean {form}")
        out[form] = avg
    assert torch.equal(W.bits(out["behind"]), W.bits(out["graph"]))


# ================================================================================================ Trainer
def _fit(kind="lamb", averaging=None, ckpt_path=None, steps_per_epoch=4, param_groups=None, **kw):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    n = _net()
    # a warm-up longer than any run here: the learning rate is step / warm-up, whatever number of steps the schedule is sized for
    m = module.SpatialClipLitModule(
        n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), OPTIMIZERS[kind](optim),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=100), param_groups=param_groups)
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=steps_per_epoch,
                                         val_steps=2)
    cbs = {} if averaging is None else {"weight_averaging": averaging}
    kw.setdefault("max_epochs", 1)
    tr = Trainer(gradient_clip_val=1.0, callbacks=cbs, **kw)
    tr.fit(m, dm, ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    return n, m, tr, dm


@pytest.mark.parametrize("kind,groups", [("lamb", None), ("adamw", {"no_decay": "open_clip"})], ids=["lamb", "adamw-two-groups"])
def test_graph_replay_without_a_host_sync(kind, groups, monkeypatch):
    """Eight steps, seven of them replays, and nothing makes the host wait for the device in between: the control block of step
    k + 1 is staged while the replay of step k may not have started.  The average has the bits of the eager run.  The two
    optimisers here refresh their step scalars through the device table, whose staging ring is protected against a host
    running ahead like the averager's control block; the one-group AdamW and Lion steps stage theirs in a single pinned slot
    and are compared with a host sync per step (test_every_step_form_averages_what_the_oracle_does)."""
    monkeypatch.setenv("SC_OVERLAP", "1")
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SC_GRAPH", mode)
        n, m, tr, _ = _fit(kind, {"decay": 0.9, "update_every_n_steps": 3, "update_starting_at_step": 1}, steps_per_epoch=8,
                           param_groups=groups, log_every_n_steps=1000, check_val_every_n_epoch=1000)
        assert tr.global_step == 8 and tr.val_runs == 0 and not [h for h in tr.history if "step" in h]
        if mode == "1":
            assert tr.graphed_step is not None and tr.graphed_step.failed is None and tr.graphed_step.replays == 7
        else:
            assert tr.graphed_step is None
        wa = tr.weight_averager
        assert wa.n_averaged == 2 and wa.latest_update_step == 6          # steps 3 and 6
        res[mode] = (wa.avg.clone(), n.store.master.clone(), tr.optimizer.exp_avg.clone())
    for a, b, what in zip(res["0"], res["1"], ("average", "model after fit", "exp_avg")):
        assert torch.equal(W.bits(a), W.bits(b)), f"{what}: the replayed run differs from the eager run"
    assert torch.equal(res["1"][0], res["1"][1])          # fit leaves the average in the model


def test_validation_runs_on_the_average(monkeypatch):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    avg_cfg = {"decay": 0.5}
    n, m, tr, dm = _fit("adamw", avg_cfg, val_check_interval=2, log_every_n_steps=1)
    wa = tr.weight_averager
    assert tr.val_runs == 2 and wa.n_averaged == 4 and tr.global_step == 4
    # the model after fit is the average, and so are its derived copies
    sd = n.state_dict()
    for sp in n.store.specs:
        assert torch.equal(sd[sp.name].flatten(), wa.avg[sp.offset:sp.offset + sp.numel]), sp.name
    mirror = n.store.master_bf16.clone()
    n.store.refresh_compute_copies()
    assert torch.equal(mirror.view(torch.int16), n.store.master_bf16.view(torch.int16))
    # the same run with validation off: the same weights, average and optimiser state, bit for bit
    n0, m0, tr0, _ = _fit("adamw", avg_cfg, check_val_every_n_epoch=1000, log_every_n_steps=1)
    assert tr0.val_runs == 0
    assert torch.equal(W.bits(n0.store.master), W.bits(n.store.master)), "validation changed the weights"
    assert torch.equal(W.bits(tr0.weight_averager.avg), W.bits(wa.avg))
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(W.bits(getattr(tr0.optimizer, name)), W.bits(getattr(tr.optimizer, name))), name
    assert [h["train/loss"] for h in tr0.history if "step" in h] == [h["train/loss"] for h in tr.history if "step" in h and
                                                                     "train/loss" in h]
    # without averaging the run's weights differ from the average (the swap is not a no-op) ...
    n1, m1, tr1, _ = _fit("adamw", None, val_check_interval=2, log_every_n_steps=1)
    assert tr1.weight_averager is None and tr1.optimizer.averager is None
    assert not torch.equal(n1.store.master, n.store.master)
    # ... and the last validation's metrics are those of a fresh net loaded with the average
    n2 = _net(seed=9)
    n2.load_state_dict({k: v.clone() for k, v in sd.items()})
    m2 = module.SpatialClipLitModule(n2, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    tr2 = Trainer(callbacks={})
    m2.trainer = tr2
    fresh = tr2._validate(m2, dm)
    last = tr.history[-1]
    assert "val/loss" in fresh and len(fresh) > 1
    assert {k: last[k] for k in fresh} == fresh, "the epoch-end validation did not run on the average"
    plain = {k: tr1.history[-1][k] for k in fresh}
    assert plain != fresh, "the averaged and the plain weights validate alike: the check above shows nothing"


def test_checkpoint_and_resume(monkeypatch, tmp_path):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_GRAPH", "0")
    cfg = {"decay": 0.8, "update_every_n_steps": 2}
    common = dict(steps_per_epoch=3, enable_checkpointing=True, log_every_n_steps=1)
    _, _, tr_a, _ = _fit("adamw", cfg, max_epochs=2, default_root_dir=str(tmp_path / "a"), **common)
    _, _, tr_b, _ = _fit("adamw", cfg, max_epochs=1, default_root_dir=str(tmp_path / "b"), **common)
    first = tr_b.checkpoint_callback.last_model_path
    ck = torch.load(first, map_location="cpu", weights_only=False)
    entry = ck["weight_averaging"]
    assert ck["global_step"] == 3 and (entry["n_averaged"], entry["latest_update_step"], entry["kind"], entry["decay"]) == \
        (2, 2, "ema", 0.8)
    assert list(ck["state_dict"]) == list(entry["current_model_state"])
    assert any(not torch.equal(ck["state_dict"][k], entry["current_model_state"][k]) for k in ck["state_dict"])
    n_c, _, tr_c, _ = _fit("adamw", cfg, ckpt_path=first, max_epochs=2, default_root_dir=str(tmp_path / "c"), **common)
    assert tr_c.global_step == tr_a.global_step == 6 and tr_c.weight_averager.n_averaged == 3
    want = torch.load(tr_a.checkpoint_callback.last_model_path, map_location="cpu", weights_only=False)
    got = torch.load(tr_c.checkpoint_callback.last_model_path, map_location="cpu", weights_only=False)
    for k in want["state_dict"]:
        assert torch.equal(W.bits(want["state_dict"][k]), W.bits(got["state_dict"][k])), f"average {k}"
        assert torch.equal(W.bits(want["weight_averaging"]["current_model_state"][k]),
                           W.bits(got["weight_averaging"]["current_model_state"][k])), f"training weights {k}"
    assert {k: v for k, v in want["weight_averaging"].items() if k != "current_model_state"} == \
        {k: v for k, v in got["weight_averaging"].items() if k != "current_model_state"}
    assert torch.equal(W.bits(want["optimizer"]["exp_avg"]), W.bits(got["optimizer"]["exp_avg"]))
    # evaluation of the file reads the average
    n_e = _net(seed=9)
    m_e = module.SpatialClipLitModule(n_e, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=3, val_steps=2)
    tr_e = Trainer()
    m_e.trainer = tr_e
    out = tr_e.test(m_e, dm, ckpt_path=tr_a.checkpoint_callback.last_model_path)
    sd = n_e.state_dict()
    for k in want["state_dict"]:
        assert torch.equal(sd[k].cpu(), want["state_dict"][k]), k
    assert out and "test/loss" in out[0]
    # a run that resumes the file without averaging trains on from the training weights
    n_p, _, tr_p, _ = _fit("adamw", None, ckpt_path=first, max_epochs=1, max_steps=3, default_root_dir=str(tmp_path / "p"),
                           steps_per_epoch=3, log_every_n_steps=1)
    assert tr_p.global_step == 3
    for sp in n_p.store.specs:
        assert torch.equal(n_p.store.master[sp.offset:sp.offset + sp.numel].cpu(),
                           entry["current_model_state"][sp.name].flatten()), sp.name


def test_refusals(monkeypatch):
    data, graph, losses, mc, module, net, optim, streams = _pkg()
    from spatial_clip_amd.trainer import Trainer
    with pytest.raises(ValueError, match="(?s)weight_averaging.*fp8"):
        Trainer(precision="fp8-mixed", callbacks={"weight_averaging": {"decay": 0.9}})
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    with pytest.raises(ValueError, match="(?s)weight_averaging.*sharded"):
        Trainer(callbacks={"weight_averaging": {"decay": 0.9}})
    monkeypatch.delenv("SC_GRAD_EXCHANGE")
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 128, 2, 64), text=None, gene=mc.GeneCfg(200, 64))
    n8 = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=1, precision="fp8")
    with pytest.raises(ValueError, match="(?s)weight_averaging.*fp8"):
        optim.WeightAverager(n8.store)
