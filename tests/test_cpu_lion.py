"""Lion without a device: the conditions the GPU kernel test (tests/test_gpu_lion.py) rests on -- torch's fp32 evaluation of the
formula meets that test's element rule on exactly its inputs, the tie band is empty at the small sizes and tiny at the large
one, fp32 and float64 agree in sign outside it -- then ``FusedLion``'s constructor refusals, the Hydra surface
(``optimizer=lion``, the two experiments, the three ``_target_`` strings) and, on a host-side ParamStore, the state-dict keys,
the two kind-mismatch errors, the sharded-exchange refusal and the compact moment buffer under a lock."""
import functools
import inspect

import pytest
import torch

from tests import _lioncases as L


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
@pytest.mark.parametrize("clip", [1.0, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", L.SIZES)
def test_torch_fp32_meets_the_rule_of_the_kernel_test(n, clip):
    """On the inputs of tests/test_gpu_lion.py (same buffers, gradients, learning rates; a clip coefficient of exactly 0.5 for
    the kernel's measured one near 0.5) the fp32 reference, chained from its own state, is judged like the kernel."""
    p, m = L.start(n)
    for k, lr in enumerate(L.STEPS):
        g = L.grad(n, k)
        p32, m32, _, _ = L.step_ref(p, m, L.effective(g, clip, torch.float32), lr, L.WD, torch.float32)
        fig = L.check_step(f"n={n} clip={clip} step {k}", p32, m32, p, m, g, clip, lr, L.WD)
        assert fig["flips"] == 0, "fp32 and float64 disagree in sign(c) outside the tie band"
        if n <= 320:
            assert fig["band"] == 0, "an element of a small case sits in the tie band: pick another seed"
        else:
            assert fig["band"] <= L.BAND_SHARE_CAP * n
        if n >= 5 * L.SLOT:
            for s in (L.ZERO_SLOT, L.NEG_ZERO_SLOT):       # the padding stays an exact +0 under weight decay
                assert torch.equal(p32[L.slot(s)].view(torch.int32), torch.zeros(L.SLOT, dtype=torch.int32))
                assert float(m32[L.slot(s)].abs().max()) == 0.0
            s = L.slot(L.MOMENT_ONLY_SLOT)
            moved = p32[s].double() - p[s].double() * (1.0 - L._f32(lr) * L._f32(L.WD))
            assert torch.equal(torch.sign(moved), -torch.sign(m[s]).double()), "g = 0: the step follows the sign of m"
        p, m = p32, m32


def test_sign_of_zero_is_zero_in_the_reference():
    z = torch.tensor([0.0, -0.0])
    p, m, c, mag = L.step_ref(torch.ones(2), z, z, 0.1, 0.5, torch.float32)
    assert p.tolist() == [L._f32(1.0 - L._f32(0.1) * 0.5)] * 2 and m.tolist() == [0.0, 0.0]
    assert not bool(L.near_tie(c.double(), mag.double()).any())


# ------------------------------------------------------------------------------------------------ constructor
def test_defaults_are_the_papers():
    comm, lock, mc, optim, params = _pkg()
    par = inspect.signature(optim.FusedLion.__init__).parameters
    assert (par["lr"].default, tuple(par["betas"].default), par["weight_decay"].default) == (1e-4, (0.9, 0.99), 0.0)
    st = _store()
    opt = optim.FusedLion(list(st.params.values()))
    assert opt.param_groups[0]["lr"] == opt.param_groups[0]["initial_lr"] == 1e-4
    assert opt.param_groups[0]["betas"] == (0.9, 0.99) and opt.param_groups[0]["weight_decay"] == 0.0
    assert "eps" not in opt.param_groups[0] and not hasattr(opt, "exp_avg_sq")
    assert opt.exp_avg.numel() == st.total and opt.exp_avg.dtype == torch.float32


def test_constructor_refusals_name_the_key_or_parameter():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    ps = list(st.params.values())
    names = list(st.params)
    # the options of lion_pytorch.Lion / timm.optim.Lion: at their off value only
    for key, off in (("use_triton", False), ("decoupled_weight_decay", False), ("caution", False), ("maximize", False),
                     ("foreach", None), ("foreach", False)):
        optim.FusedLion(list(_store().params.values()), **{key: off})
    for key in ("use_triton", "decoupled_weight_decay", "caution", "maximize", "foreach"):
        with pytest.raises(ValueError, match=f"FusedLion: {key}=True"):
            optim.FusedLion(ps, **{key: True})
    for key in ("eps", "amsgrad", "momentum"):
        with pytest.raises(ValueError, match=f"FusedLion: unknown keyword '{key}'"):
            optim.FusedLion(ps, **{key: 1e-6})
    # the two forms of params, as FusedAdamW validates them
    with pytest.raises(ValueError, match="FusedLion: params mixes parameters and group dicts"):
        optim.FusedLion([ps[0], {"params": ps[1:]}])
    with pytest.raises(ValueError, match="FusedLion updates the whole flat buffer"):
        optim.FusedLion(ps[1:])
    with pytest.raises(ValueError, match="FusedLion needs the parameters of exactly one SpatialClipNet"):
        optim.FusedLion(ps + list(_store().params.values()))
    with pytest.raises(ValueError, match=r"FusedLion: parameter group 1 sets betas=\(0.9, 0.98\); per-group betas"):
        optim.FusedLion([{"params": ps[:3]}, {"params": ps[3:], "betas": (0.9, 0.98)}])
    with pytest.raises(ValueError, match=r"FusedLion: parameter group 0 has unknown key\(s\) \['eps'\]"):
        optim.FusedLion([{"params": ps, "eps": 1e-6}])
    with pytest.raises(ValueError, match="FusedLion: parameter group 0 has no 'params'"):
        optim.FusedLion([{"lr": 1e-4}])
    with pytest.raises(ValueError, match=f"FusedLion: parameter {names[0]} is listed twice"):
        optim.FusedLion([{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match=f"FusedLion: 1 trainable parameter.*first: {names[-1]}"):
        optim.FusedLion([{"params": ps[:-1]}])
    with pytest.raises(ValueError, match="FusedLion: parameter group 0 holds a tensor of shape"):
        optim.FusedLion([{"params": [torch.zeros(3)]}])
    with pytest.raises(ValueError, match="FusedLion: 257 parameter groups; at most 256"):
        optim.FusedLion([{"params": []} for _ in range(257)])


def test_groups_carry_lr_and_weight_decay_and_a_slot_table():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    groups = optim.scaled_lr_groups(optim.open_clip_param_groups(st.params.items(), 1.0), 1e-4, {"visual.": 0.1})
    opt = optim.FusedLion(groups, lr=1e-4, weight_decay=1.0)
    assert len(opt.param_groups) == 4 and opt.chunk_group.numel() == st.total // 64
    assert opt.group_hyper.numel() == 2 * 4         # {lr, wd} per group: no bias corrections in front
    by_name = {n: g for g in opt.param_groups for n in g["param_names"]}
    assert (by_name["logit_scale"]["lr"], by_name["logit_scale"]["weight_decay"]) == (1e-4, 0.0)
    assert by_name["visual.proj"]["lr"] == pytest.approx(1e-5) and by_name["visual.proj"]["weight_decay"] == 1.0
    assert torch.equal(opt.chunk_group, optim.slot_table(st, [g["param_names"] for g in opt.param_groups]))
    assert all("eps" not in g and g["betas"] == (0.9, 0.99) for g in opt.param_groups)


# ------------------------------------------------------------------------------------------------ Hydra surface
def test_the_three_targets_map_to_fused_lion():
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    for target in ("lion_pytorch.Lion", "timm.optim.Lion", "timm.optim.lion.Lion"):
        assert H._locate(target) is optim.FusedLion
        part = H.instantiate({"_target_": target, "_partial_": True, "lr": 3e-5})
        assert isinstance(part, functools.partial) and part.func is optim.FusedLion and part.keywords == {"lr": 3e-5}
    assert H._locate("torch.optim.AdamW") is optim.FusedAdamW


def test_lion_configs_compose_to_a_fused_lion_partial(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    adamw = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    lit = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lit"])
    want = {"lr": 1.0e-4, "betas": [0.9, 0.99], "weight_decay": 1.0}
    for over in (["optimizer=lion"], ["experiment=vitb16_gene_b256_lion"], ["experiment=vitb16_gene_b256_lit_lion"]):
        cfg = H.compose("train.yaml", over)
        assert cfg["_choices_"]["optimizer"] == "lion" and cfg.optimizer["_target_"] == "lion_pytorch.Lion"
        part = H.instantiate(cfg.optimizer)
        assert isinstance(part, functools.partial) and part.func is optim.FusedLion and part.keywords == want
        # the paper's rule: lr 10x below AdamW's, weight decay 10x above, the product unchanged
        assert cfg.optimizer.lr * cfg.optimizer.weight_decay == pytest.approx(adamw.optimizer.lr * adamw.optimizer.weight_decay)
        assert cfg.optimizer.lr == pytest.approx(adamw.optimizer.lr / 10)
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lion"])
    assert cfg["model"]["net"] == adamw["model"]["net"] and cfg.data.batch_size == 256 and "param_groups" not in cfg["model"]
    assert cfg["loss"] == adamw["loss"] and cfg["trainer"] == adamw["trainer"]
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lit_lion"])
    assert cfg["model"]["net"] == lit["model"]["net"] and cfg["model"]["net"]["lock_image"] is True
    assert dict(cfg["model"]["param_groups"]) == {"no_decay": "open_clip"}


def test_param_groups_of_the_module_read_the_lion_partial():
    """``SpatialClipLitModule(param_groups=...)`` scales its groups from the partial's bound lr / weight decay, or from
    FusedLion's defaults where the partial binds none."""
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import module

    class _Net:
        store = _store()
    for part, lr, wd in ((functools.partial(optim.FusedLion, lr=2e-4, weight_decay=0.5), 2e-4, 0.5),
                         (functools.partial(optim.FusedLion), 1e-4, 0.0)):
        m = module.SpatialClipLitModule.__new__(module.SpatialClipLitModule)
        torch.nn.Module.__init__(m)
        m.net, m.param_groups = _Net(), optim.check_param_groups_cfg({"no_decay": "open_clip", "lr_scale": {"visual.": 0.5}})
        m.hparams = type("H", (), {"optimizer_cfg": part})()
        groups = m.optimizer_param_groups()
        opt = part(params=groups)
        assert isinstance(opt, optim.FusedLion) and len(opt.param_groups) == 4
        assert sorted({(g["lr"], g["weight_decay"]) for g in opt.param_groups}) == \
            sorted({(lr, 0.0), (lr * 0.5, 0.0), (lr, wd), (lr * 0.5, wd)})


# ------------------------------------------------------------------------------------------------ state on a host-side store
def test_state_dict_keys_and_kind_mismatch_errors():
    comm, lock, mc, optim, params = _pkg()
    lion = optim.FusedLion(list(_store().params.values()), lr=1e-4, weight_decay=1.0)
    adamw = optim.FusedAdamW(list(_store().params.values()))
    lion.step_count, lion.exp_avg[:] = 7, 0.25
    sd = lion.state_dict()
    assert list(sd) == ["optimizer", "step", "exp_avg", "param_groups"] and sd["optimizer"] == "lion" and sd["step"] == 7
    assert sd["exp_avg"].numel() == lion.store.total and "params" not in sd["param_groups"][0]
    assert sd["param_groups"][0] == {"lr": 1e-4, "initial_lr": 1e-4, "betas": (0.9, 0.99), "weight_decay": 1.0}
    asd = adamw.state_dict()
    assert list(asd) == ["step", "exp_avg", "exp_avg_sq", "param_groups"]        # AdamW files are what they were
    with pytest.raises(ValueError, match="(?s)FusedLion.*'adamw'.*'lion'"):
        lion.load_state_dict(asd)
    with pytest.raises(ValueError, match="(?s)FusedLion.*'adamw'.*'lion'"):
        lion.load_state_dict({**sd, "exp_avg_sq": sd["exp_avg"]})
    with pytest.raises(ValueError, match="(?s)FusedAdamW.*'lion'.*'adamw'"):
        adamw.load_state_dict(sd)
    assert lion.step_count == 7 and adamw.step_count == 0       # a refused load changes nothing
    adamw.load_state_dict({**asd, "step": 3})                   # no "optimizer" key: loads as before
    assert adamw.step_count == 3
    fresh = optim.FusedLion(list(_store().params.values()))
    fresh.load_state_dict(sd)
    assert fresh.step_count == 7 and bool((fresh.exp_avg == 0.25).all())
    # the trainer's resume test accepts the file
    assert "exp_avg" in sd


def test_sharded_exchange_is_refused():
    comm, lock, mc, optim, params = _pkg()
    opt = optim.FusedLion(list(_store().params.values()))
    ex = comm.ShardedGradExchange.__new__(comm.ShardedGradExchange)
    with pytest.raises(ValueError, match="FusedLion.*sharded"):
        opt.attach_exchange(ex)
    assert opt.exchange is None
    opt.attach_exchange(None)           # the all-reduce route needs nothing
    assert opt.exchange is None


def test_moments_are_compact_under_a_lock_and_the_file_is_full():
    comm, lock, mc, optim, params = _pkg()
    cfg = _tiny_cfg()
    st = _store(cfg)
    locked, free = lock.split_groups(lock.vision_groups(cfg.vision.layers), 0)
    st.unlock(free)
    st.lock(locked)
    opt = optim.FusedLion(list(st.params.values()), weight_decay=1.0)
    assert opt.exp_avg.numel() == st.trainable_floats() < st.total and opt.ranges == list(st.trainable_ranges())
    opt.exp_avg[:] = torch.arange(1, opt.exp_avg.numel() + 1, dtype=torch.float32)
    sd = opt.state_dict()
    assert sd["exp_avg"].numel() == st.total
    mask = torch.zeros(st.total, dtype=torch.bool)
    for lo, hi in opt.ranges:
        mask[lo:hi] = True
    assert float(sd["exp_avg"][~mask].abs().max()) == 0.0 and torch.equal(sd["exp_avg"][mask], opt.exp_avg)
    # the file resumes without the lock (full layout) and with it (compact again)
    free_opt = optim.FusedLion(list(_store(cfg).params.values()))
    free_opt.load_state_dict(sd)
    assert torch.equal(free_opt.exp_avg, sd["exp_avg"])
    st2 = _store(cfg)
    st2.unlock(free)
    st2.lock(locked)
    again = optim.FusedLion(list(st2.params.values()))
    again.load_state_dict(sd)
    assert torch.equal(again.exp_avg, opt.exp_avg)
