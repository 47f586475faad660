"""LAMB without a device: the conditions the GPU kernel test (tests/test_gpu_lamb.py) rests on -- torch's fp32 evaluation of
the formula, with the norms summed in the kernels' order (fp32 per 64-float slot, float64 over the slots), meets that test's
element rule, its bf16 share cap and its trust-ratio bound on exactly its inputs -- the equivalence of timm's clip composed
with Lightning's and the one clip at the smaller threshold, then ``FusedLamb``'s constructor refusals, the Hydra surface
(``optimizer=lamb``, the experiment, the two ``_target_`` strings) and, on a host-side ParamStore, the tensor tables, the
state-dict keys, the three-way kind-mismatch matrix, the sharded-exchange refusal and the compact moments under a lock."""
import functools
import inspect

import pytest
import torch

from tests import _lambcases as C


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, lock, model_configs as mc, optim, params
    return comm, lock, mc, optim, params


def _tiny_cfg(text=False):
    comm, lock, mc, optim, params = _pkg()
    return mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=mc.TextCfg(16, 97, 64, 2, 2) if text else None,
                       gene=None if text else mc.GeneCfg(200, 64))


def _store(cfg=None):
    """A ParamStore laid out on the host; no kernel runs (init=False)."""
    comm, lock, mc, optim, params = _pkg()
    st = params.ParamStore(cfg or _tiny_cfg(), torch.device("cpu"), init=False)
    for p in st.params.values():
        p._sc_store = st
    return st


# ------------------------------------------------------------------------------------------------ the kernel test's reference
VARIANTS = {"plain": {}, "always_adapt": {"always_adapt": True}, "trust_clip": {"trust_clip": True}}
REFERENCE_RUNS = [("full", 1.0, "plain"), ("full", 0.5, "plain")] + [("small", 0.5, v) for v in VARIANTS]


@pytest.mark.parametrize("which,clip,variant", REFERENCE_RUNS, ids=[f"{w}-clip{c}-{v}" for w, c, v in REFERENCE_RUNS])
def test_fp32_in_the_kernels_summation_order_meets_the_rule_of_the_kernel_test(which, clip, variant):
    """On the inputs of tests/test_gpu_lamb.py (same buffers, gradients, learning rates; a clip coefficient of exactly 0.5 for
    the kernel's measured one near 0.5) the fp32 reference with per-slot partial sums, chained from its own state, is judged like
    the kernel: the bound is one the reference alone meets in another summation order."""
    tb, kw = C.table(which), VARIANTS[variant]
    state = C.start(which)
    for k, lr in enumerate(C.STEPS):
        g = C.grad(which, k)
        ge = (C.effective(g, clip, torch.float64), C.effective(g, clip, torch.float32))
        p32, m32, v32, r32 = C.step_ref(tb, *state, ge[1], lr, k + 1, torch.float32, slot_order=True, **kw)
        r64 = C.check_step(f"{which} clip={clip} {variant} step {k}", tb, (p32, m32, v32), state, ge, lr, k + 1,
                           mirror=p32.to(torch.bfloat16), got_r=r32, **kw)
        if which == "small":        # ... and tensor by tensor, each with the E32 of its own elements
            C.check_step(f"{which} clip={clip} {variant} step {k}", tb, (p32, m32, v32), state, ge, lr, k + 1, per_tensor=True, **kw)
        # what the table is for
        r = dict(zip(tb.names, r64.tolist()))
        assert r["still"] == 1.0 and (r["zero_p"] == 1.0) == (k == 0)       # p = 0 before the first step only
        assert (r["nodecay"] == 1.0) == (variant != "always_adapt")
        if variant == "trust_clip":
            assert r["big_r"] == 1.0 and max(r.values()) == 1.0
        else:
            assert r["big_r"] > 1.0 and 0.0 < min(r.values()) < 1.0
        for t in (p32, m32, v32):           # the slot padding stays an exact zero
            pad = ~tb.owned
            for lo, hi in tb.holes:
                pad[lo:hi] = False
            assert not bool(t[pad].view(torch.int32).any())
        state = (p32, m32, v32)


def test_the_large_tensor_spans_the_second_trip_of_the_capped_grid():
    tb = C.table("full")
    ti = tb.index("large")
    assert tb.offset[ti] < C.GRID_CAP_N < tb.offset[ti] + tb.numel[ti] and tb.n > C.GRID_CAP_N
    assert [tb.numel[tb.index(n)] for n in ("one", "slot", "two", "five")] == [1, 64, 65, 320]
    assert tb.tensor_slots[tb.index("two")].tolist()[1] - tb.tensor_slots[tb.index("two")].tolist()[0] == 2
    assert int((tb.slot_tensor < 0).sum()) == 1 and len(tb.holes) == 1


@pytest.mark.parametrize("clip_val,max_grad_norm,norm", [(1.0, 1.0, 3.0), (0.5, 1.0, 3.0), (2.0, 1.0, 3.0), (1.0, 2.0, 1.5),
                                                           (1.0, 1.0, 0.5), (None, 1.0, 3.0), (1.0, None, 3.0), (4.0, 2.0, 3.0)])
def test_two_clips_in_a_row_are_one_clip_at_the_smaller_threshold(clip_val, max_grad_norm, norm):
    """Lightning scales the gradient by min(1, c / ||g||) before the optimiser runs and timm.optim.Lamb then divides it by
    max(1, ||g'|| / max_grad_norm): on numbers, that is min(1, min(c, max_grad_norm) / ||g||).  (The 1e-6 both add to the norm
    is left out; it is below the rounding of these norms.)"""
    g = torch.randn(1000, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    g = g * (norm / float(g.norm()))
    a = g * min(1.0, clip_val / float(g.norm())) if clip_val is not None else g
    b = a / max(1.0, float(a.norm()) / max_grad_norm) if max_grad_norm is not None else a
    comm, lock, mc, optim, params = _pkg()
    opt = optim.FusedLamb(list(_store().params.values()), max_grad_norm=max_grad_norm)
    threshold = opt._clip_threshold(clip_val)
    assert threshold == min(x for x in (clip_val, max_grad_norm) if x is not None)
    one = g * min(1.0, threshold / float(g.norm()))
    assert float((one - b).abs().max()) <= 1e-15 * norm


def test_no_threshold_at_all_is_no_clip():
    comm, lock, mc, optim, params = _pkg()
    opt = optim.FusedLamb(list(_store().params.values()), max_grad_norm=None)
    assert opt._clip_threshold(None) is None and opt._clip(1.0, None, None) is None
    assert opt._clip_threshold(0.0) is None             # the Trainer's "no clipping"
    assert optim.FusedAdamW(list(_store().params.values()))._clip_threshold(0.7) == 0.7


# ------------------------------------------------------------------------------------------------ constructor
def test_defaults_are_timms():
    comm, lock, mc, optim, params = _pkg()
    par = inspect.signature(optim.FusedLamb.__init__).parameters
    assert (par["lr"].default, tuple(par["betas"].default), par["eps"].default, par["weight_decay"].default) == \
        (1e-3, (0.9, 0.999), 1e-6, 0.01)
    assert (par["max_grad_norm"].default, par["trust_clip"].default, par["always_adapt"].default) == (1.0, False, False)
    st = _store()
    opt = optim.FusedLamb(list(st.params.values()))
    g = opt.param_groups[0]
    assert (g["lr"], g["initial_lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, 1e-3, (0.9, 0.999), 1e-6, 0.01)
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.total and opt.max_grad_norm == 1.0


def test_constructor_refusals_name_the_key_or_parameter():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    ps = list(st.params.values())
    names = list(st.params)
    for key, ok in (("bias_correction", True), ("grad_averaging", True), ("caution", False), ("decoupled_decay", False),
                    ("maximize", False), ("foreach", None), ("foreach", False), ("max_grad_norm", None), ("max_grad_norm", 0.5),
                    ("trust_clip", True), ("always_adapt", True)):
        optim.FusedLamb(list(_store().params.values()), **{key: ok})
    for key in ("bias_correction", "grad_averaging"):
        with pytest.raises(ValueError, match=f"FusedLamb: {key}=False is not supported; only {key}=True"):
            optim.FusedLamb(ps, **{key: False})
    for key in ("caution", "decoupled_decay", "maximize", "foreach"):
        with pytest.raises(ValueError, match=f"FusedLamb: {key}=True is not supported; only {key}={'None' if key == 'foreach' else 'False'}"):
            optim.FusedLamb(ps, **{key: True})
    for key in ("amsgrad", "momentum", "use_triton"):
        with pytest.raises(ValueError, match=f"FusedLamb: unknown keyword '{key}'"):
            optim.FusedLamb(ps, **{key: 1e-6})
    for bad in (0.0, -1.0, float("inf"), True, "1"):
        with pytest.raises(ValueError, match="FusedLamb: max_grad_norm="):
            optim.FusedLamb(ps, max_grad_norm=bad)
    for key in ("trust_clip", "always_adapt"):
        with pytest.raises(ValueError, match=f"FusedLamb: {key}=1: True or False"):
            optim.FusedLamb(ps, **{key: 1})
    # the two forms of params, as FusedAdamW validates them
    with pytest.raises(ValueError, match="FusedLamb: params mixes parameters and group dicts"):
        optim.FusedLamb([ps[0], {"params": ps[1:]}])
    with pytest.raises(ValueError, match="FusedLamb updates the whole flat buffer"):
        optim.FusedLamb(ps[1:])
    with pytest.raises(ValueError, match=r"FusedLamb: parameter group 1 sets betas=\(0.9, 0.98\); per-group betas"):
        optim.FusedLamb([{"params": ps[:3]}, {"params": ps[3:], "betas": (0.9, 0.98)}])
    with pytest.raises(ValueError, match="FusedLamb: parameter group 0 sets eps=1e-08; per-group eps"):
        optim.FusedLamb([{"params": ps, "eps": 1e-8}])
    with pytest.raises(ValueError, match=r"FusedLamb: parameter group 0 has unknown key\(s\) \['trust_clip'\]"):
        optim.FusedLamb([{"params": ps, "trust_clip": True}])
    with pytest.raises(ValueError, match=f"FusedLamb: parameter {names[0]} is listed twice"):
        optim.FusedLamb([{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match=f"FusedLamb: 1 trainable parameter.*first: {names[-1]}"):
        optim.FusedLamb([{"params": ps[:-1]}])


def test_tensor_tables_cover_every_parameter_and_carry_its_group():
    comm, lock, mc, optim, params = _pkg()
    st = _store(_tiny_cfg(text=True))
    groups = optim.scaled_lr_groups(optim.open_clip_param_groups(st.params.items(), 0.05), 2e-3, {"visual.": 0.1})
    opt = optim.FusedLamb(groups, lr=2e-3, weight_decay=0.05)
    assert len(opt.param_groups) == 4 and opt.tensor_names == [sp.name for sp in st.specs]
    n_t = len(st.specs)
    assert opt.slot_tensor.dtype == torch.int32 and opt.slot_tensor.numel() == st.total // 64
    assert opt.group_hyper.numel() == 2 + 2 * n_t and opt.trust.numel() == n_t and opt.slot_sums.numel() == 2 * (st.total // 64)
    by_name = {n: gi for gi, g in enumerate(opt.param_groups) for n in g["param_names"]}
    for ti, sp in enumerate(st.specs):
        lo, hi = opt.tensor_slots[ti].tolist()
        assert lo == sp.offset // 64 and hi - lo == (max(sp.numel, 1) + 63) // 64
        assert bool((opt.slot_tensor[lo:hi] == ti).all()) and int(opt.tensor_group[ti]) == by_name[sp.name]
    one = st.by_name["logit_scale"]
    assert one.numel == 1 and opt.param_groups[by_name["logit_scale"]]["weight_decay"] == 0.0
    assert "in_proj_weight" in "".join(opt.tensor_names)          # the fused q/k/v matrix is ONE tensor
    covered = int((opt.slot_tensor >= 0).sum())
    assert covered == sum((max(sp.numel, 1) + 63) // 64 for sp in st.specs) <= st.total // 64
    # a plain parameter list: one group, the same tables
    plain = optim.FusedLamb(list(_store(_tiny_cfg(text=True)).params.values()))
    assert torch.equal(plain.slot_tensor, opt.slot_tensor) and not bool(plain.tensor_group.any())
    assert plain.group_hyper.numel() == opt.group_hyper.numel() and plain._uses_table()


# ------------------------------------------------------------------------------------------------ Hydra surface
def test_the_two_targets_map_to_fused_lamb():
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    for target in ("timm.optim.Lamb", "timm.optim.lamb.Lamb"):
        assert H._locate(target) is optim.FusedLamb
        part = H.instantiate({"_target_": target, "_partial_": True, "lr": 3e-3})
        assert isinstance(part, functools.partial) and part.func is optim.FusedLamb and part.keywords == {"lr": 3e-3}
    assert H._locate("torch.optim.AdamW") is optim.FusedAdamW and H._locate("timm.optim.Lion") is optim.FusedLion


def test_lamb_configs_compose_to_a_fused_lamb_partial(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    adamw = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    want = {"lr": 2.0e-3, "betas": [0.9, 0.999], "eps": 1.0e-6, "weight_decay": 0.01, "bias_correction": True,
            "grad_averaging": True, "max_grad_norm": 1.0, "trust_clip": False, "always_adapt": False}
    for over in (["optimizer=lamb"], ["experiment=vitb16_gene_b256_lamb"]):
        cfg = H.compose("train.yaml", over)
        assert cfg["_choices_"]["optimizer"] == "lamb" and cfg.optimizer["_target_"] == "timm.optim.Lamb"
        part = H.instantiate(cfg.optimizer)
        assert isinstance(part, functools.partial) and part.func is optim.FusedLamb and part.keywords == want
        opt = part(params=list(_store().params.values()))         # the keywords are all accepted
        assert isinstance(opt, optim.FusedLamb) and opt.param_groups[0]["lr"] == 2.0e-3
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lamb"])
    assert cfg["model"]["net"] == adamw["model"]["net"] and cfg.data.batch_size == 256
    assert dict(cfg["model"]["param_groups"]) == {"no_decay": "open_clip"}
    assert cfg["loss"] == adamw["loss"] and cfg["trainer"] == adamw["trainer"]


def test_param_groups_of_the_module_read_the_lamb_partial():
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import module

    class _Net:
        store = _store()
    for part, lr, wd in ((functools.partial(optim.FusedLamb, lr=2e-3, weight_decay=0.05), 2e-3, 0.05),
                         (functools.partial(optim.FusedLamb), 1e-3, 0.01)):
        m = module.SpatialClipLitModule.__new__(module.SpatialClipLitModule)
        torch.nn.Module.__init__(m)
        m.net, m.param_groups = _Net(), optim.check_param_groups_cfg({"no_decay": "open_clip"})
        m.hparams = type("H", (), {"optimizer_cfg": part})()
        opt = part(params=m.optimizer_param_groups())
        assert isinstance(opt, optim.FusedLamb)
        assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(lr, 0.0), (lr, wd)]


# ------------------------------------------------------------------------------------------------ state on a host-side store
def test_state_dict_keys_and_the_three_way_kind_matrix():
    comm, lock, mc, optim, params = _pkg()
    mk = lambda cls, **kw: cls(list(_store().params.values()), **kw)       # noqa: E731
    opts = {"adamw": mk(optim.FusedAdamW), "lion": mk(optim.FusedLion), "lamb": mk(optim.FusedLamb, lr=2e-3)}
    lamb = opts["lamb"]
    lamb.step_count, lamb.exp_avg[:], lamb.exp_avg_sq[:] = 7, 0.25, 0.5
    sds = {k: o.state_dict() for k, o in opts.items()}
    sd = sds["lamb"]
    assert list(sd) == ["optimizer", "step", "exp_avg", "exp_avg_sq", "param_groups"] and sd["optimizer"] == "lamb" and sd["step"] == 7
    assert sd["exp_avg"].numel() == sd["exp_avg_sq"].numel() == lamb.store.total and "params" not in sd["param_groups"][0]
    assert sd["param_groups"][0] == {"lr": 2e-3, "initial_lr": 2e-3, "betas": (0.9, 0.999), "eps": 1e-6, "weight_decay": 0.01}
    assert list(sds["adamw"]) == ["step", "exp_avg", "exp_avg_sq", "param_groups"]      # AdamW files are what they were
    assert list(sds["lion"]) == ["optimizer", "step", "exp_avg", "param_groups"]
    for mine, opt in opts.items():
        for theirs, file in sds.items():
            if mine == theirs:
                opt.load_state_dict(file)
                continue
            before = opt.step_count
            with pytest.raises(ValueError, match=f"(?s){opt.NAME}.*{theirs!r}.*{mine!r}"):
                opt.load_state_dict(file)
            assert opt.step_count == before         # a refused load changes nothing
    with pytest.raises(ValueError, match="(?s)FusedLamb.*'adamw'.*'lamb'"):     # an AdamW file that names its kind
        lamb.load_state_dict({**sds["adamw"], "optimizer": "adamw"})
    with pytest.raises(ValueError, match="(?s)FusedLamb.*'lion'.*'lamb'"):      # a LAMB file without its second moment
        lamb.load_state_dict({k: v for k, v in sd.items() if k != "exp_avg_sq"})
    # the messages of the two older kinds are what they were
    with pytest.raises(ValueError, match="AdamW and Lion states do not convert into each other"):
        opts["lion"].load_state_dict(sds["adamw"])
    with pytest.raises(ValueError, match="AdamW, Lion and LAMB states do not convert into each other"):
        opts["adamw"].load_state_dict(sd)
    fresh = mk(optim.FusedLamb)
    fresh.load_state_dict(sd)
    assert fresh.step_count == 7 and bool((fresh.exp_avg == 0.25).all()) and bool((fresh.exp_avg_sq == 0.5).all())


def test_sharded_exchange_is_refused():
    comm, lock, mc, optim, params = _pkg()
    opt = optim.FusedLamb(list(_store().params.values()))
    ex = comm.ShardedGradExchange.__new__(comm.ShardedGradExchange)
    with pytest.raises(ValueError, match="FusedLamb.*sharded"):
        opt.attach_exchange(ex)
    assert opt.exchange is None
    opt.attach_exchange(None)           # the all-reduce route needs nothing
    assert opt.exchange is None


def test_moments_and_tables_under_a_lock_and_resume_under_another_grouping():
    comm, lock, mc, optim, params = _pkg()
    cfg = _tiny_cfg()

    def locked_store():
        st = _store(cfg)
        locked, free = lock.split_groups(lock.vision_groups(cfg.vision.layers), 0)
        st.unlock(free)
        st.lock(locked)
        return st
    st = locked_store()
    opt = optim.FusedLamb(list(st.params.values()), weight_decay=0.05)
    # no moment float and no tensor for a locked parameter
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.trainable_floats() < st.total
    assert opt.ranges == list(st.trainable_ranges()) and opt.tensor_names == st.trainable_names()
    assert 0 < len(opt.tensor_names) < len(st.specs) and opt.group_hyper.numel() == 2 + 2 * len(opt.tensor_names)
    mask = torch.zeros(st.total, dtype=torch.bool)
    for lo, hi in opt.ranges:
        mask[lo:hi] = True
    owned = (opt.slot_tensor >= 0).repeat_interleave(64)
    assert not bool((owned & ~mask).any()), "a slot outside the trainable ranges names a tensor"
    for n in st.locked:
        sp = st.by_name[n]
        assert bool((opt.slot_tensor[sp.offset // 64:(sp.offset + max(sp.numel, 1) + 63) // 64] == -1).all())
    opt.exp_avg[:] = torch.arange(1, opt.exp_avg.numel() + 1, dtype=torch.float32)
    opt.exp_avg_sq[:] = 0.5 * opt.exp_avg
    opt.step_count = 3
    sd = opt.state_dict()
    assert list(sd) == ["optimizer", "step", "exp_avg", "exp_avg_sq", "param_groups"]
    for key in ("exp_avg", "exp_avg_sq"):
        assert sd[key].numel() == st.total and float(sd[key][~mask].abs().max()) == 0.0
        assert torch.equal(sd[key][mask], getattr(opt, key))
    # the file resumes without the lock (full layout), with it (compact again), and under another grouping
    free_opt = optim.FusedLamb(list(_store(cfg).params.values()))
    free_opt.load_state_dict(sd)
    assert torch.equal(free_opt.exp_avg, sd["exp_avg"]) and torch.equal(free_opt.exp_avg_sq, sd["exp_avg_sq"])
    st2 = locked_store()
    again = optim.FusedLamb(optim.open_clip_param_groups(st2.params.items(), 0.05))
    assert len(again.param_groups) == 2 and again.tensor_names == opt.tensor_names
    again.load_state_dict(sd)
    assert again.step_count == 3 and torch.equal(again.exp_avg, opt.exp_avg) and torch.equal(again.exp_avg_sq, opt.exp_avg_sq)
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(again.state_dict()[key], sd[key])
