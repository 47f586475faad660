"""Muon without a device: the rule the GPU tests (tests/test_gpu_muon.py) hold the Newton-Schulz kernels to is shown to be
satisfiable -- a bf16 emulation of the kernels' arithmetic meets it on every matrix and input kind of tests/_muoncases.py, and a
single wrong element fails it -- then ``FusedMuon``'s defaults and constructor refusals, the default split, the Hydra surface
(``optimizer=muon``, the experiment, the ``_target_`` string, the module's ``param_groups``) and, on a host-side ParamStore, the
tensor tables (also under a lock), the state-dict keys, the kind matrix against the three older optimisers and the
sharded-exchange refusal."""
import functools
import inspect

import pytest
import torch

from tests import _muoncases as C


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, lock, model_configs as mc, optim, params
    return comm, lock, mc, optim, params


def _tiny_cfg(text=True):
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


BLOCK_LEAVES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


# ------------------------------------------------------------------------------------------------ the rule for O
@pytest.mark.parametrize("kind", C.KINDS)
def test_a_bf16_emulation_of_the_kernels_meets_the_rule_for_o(kind):
    """Ratios dev(emulation) / dev(torch) measured here, over the shapes of ``MATRICES`` (seed 0): gauss 0.94 - 1.12, half
    0.85 - 1.10, tiny 0.92 - 1.03; torch's own deviation 1.2e-2 - 2.0e-2.  The all-zero update gives exactly 0 on both."""
    for name, (r, c) in C.MATRICES:
        u = C.matrix_input(kind, r, c, seed=0)
        o64 = C.ns64(u)
        dk, dt = C.check_o(f"{kind} {name} [{r}, {c}]", C.ns_emulated(u).double(), C.torch_o(u), o64)
        if kind != "zero":
            assert 5e-3 < dt < 4e-2, "torch's own deviation left the range the rule was written for"
        else:
            assert dk == dt == 0.0


def test_one_wrong_element_of_a_64_by_64_result_fails_the_rule():
    u = C.matrix_input("gauss", 64, 64, seed=0)
    o64, o_t = C.ns64(u), C.torch_o(u)
    o = C.ns_emulated(u).double()
    C.check_o("intact", o, o_t, o64)
    o[17, 5] += 1.0         # an entry of an orthogonalised 64 x 64 matrix is about 1 / 8
    with pytest.raises(AssertionError, match="allowed 1.5 x"):
        C.check_o("one wrong element", o, o_t, o64)
    o = C.ns_emulated(u).double().T.contiguous()          # the transposed result
    with pytest.raises(AssertionError, match="allowed 1.5 x"):
        C.check_o("transposed", o, o_t, o64)


def test_the_float64_formula_orthogonalises_and_transposes_tall_matrices():
    u = C.matrix_input("gauss", 192, 64, seed=1)
    o = C.ns64(u)
    assert o.shape == (192, 64)
    s = torch.linalg.svdvals(o)
    assert 0.5 < float(s.min()) and float(s.max()) < 1.5          # S' ~ Uniform(0.5, 1.5) (torch/optim/_muon.py)
    assert torch.allclose(o, C.ns64(u.T.contiguous()).T, atol=1e-12)


def test_o_is_recovered_from_the_weights_far_below_the_rule():
    tb = C.table()
    p0 = C.start()[0][tb.elements(tb.index("odd"))].reshape(72, 200)
    u = C.matrix_input("gauss", 72, 200, seed=0)
    lr, wd = C.STEPS[2] * 0.5, 0.1
    p1, _ = C.torch_step(p0, torch.zeros(72, 200), u, lr, wd, 0.0, True, None)
    o_direct = C.torch_o(u)
    o_rec = C.recover_o(p0, p1, lr, wd, lr * C.adjust_ratio(None, 72, 200))
    assert C.deviation(o_rec, o_direct) < 1e-4


def test_the_table_holds_the_shapes_the_issue_names():
    tb = C.table()
    shapes = [s for _, s in C.MATRICES]
    for s in ((64, 64), (192, 64), (64, 128), (72, 200), (136, 136)):
        assert s in shapes
    assert len(tb.classes[(64, 128)]) == 3 and sum(len(v) == 1 for v in tb.classes.values()) >= 4
    offs = tb.class_offsets((64, 128)).tolist()
    assert offs[1] - offs[0] != offs[2] - offs[1], "the class of three sits at equal strides"
    assert sorted(tb.numel[i] for i in tb.adamw) == [1, 64, 65, 320] and len(tb.holes) == 1
    assert int((tb.slot_tensor == -2).sum()) == 1 and int((tb.slot_tensor >= 0).sum()) == tb.compact_slots
    assert all(min(s) >= 64 for s in shapes)


# ------------------------------------------------------------------------------------------------ constructor
def test_defaults_are_torchs():
    comm, lock, mc, optim, params = _pkg()
    mine = inspect.signature(optim.FusedMuon.__init__).parameters
    theirs = inspect.signature(torch.optim.Muon.__init__).parameters
    shared = [k for k in theirs if k not in ("self", "params")]
    assert shared == ["lr", "weight_decay", "momentum", "nesterov", "ns_coefficients", "eps", "ns_steps", "adjust_lr_fn"]
    assert list(mine)[2:2 + len(shared)] == shared
    for k in shared:
        a, b = mine[k].default, theirs[k].default
        assert (tuple(a) == tuple(b)) if k == "ns_coefficients" else (a == b), k
    adamw = inspect.signature(torch.optim.AdamW.__init__).parameters
    assert tuple(mine["adamw_betas"].default) == tuple(adamw["betas"].default) and mine["adamw_eps"].default == adamw["eps"].default
    assert mine["adamw_lr"].default is None and mine["adamw_weight_decay"].default is None
    st = _store()
    opt = optim.FusedMuon(list(st.params.values()))
    assert [g["use_muon"] for g in opt.param_groups] == [True, False]
    for g in opt.param_groups:          # None: the Muon value
        assert (g["lr"], g["initial_lr"], g["weight_decay"], g["betas"], g["eps"]) == (1e-3, 1e-3, 0.1, (0.9, 0.999), 1e-8)
    opt = optim.FusedMuon(list(_store().params.values()), lr=0.02, weight_decay=0.0, adamw_lr=3e-4, adamw_weight_decay=0.2)
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(0.02, 0.0), (3e-4, 0.2)]
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.total


def test_constructor_refusals_name_the_key_or_parameter():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    ps, names = list(st.params.values()), list(st.params)
    mk = lambda **kw: optim.FusedMuon(list(_store().params.values()), **kw)     # noqa: E731
    for kw in (dict(foreach=None), dict(foreach=False), dict(maximize=False), dict(ns_steps=1), dict(ns_steps=99),
               dict(adjust_lr_fn="original"), dict(adjust_lr_fn="match_rms_adamw"), dict(nesterov=False), dict(momentum=0.0)):
        mk(**kw)
    for key in ("foreach", "maximize"):
        with pytest.raises(ValueError, match=f"FusedMuon: {key}=True is not supported"):
            mk(**{key: True})
    for bad in (0, 100, -1, 2.5, True):
        with pytest.raises(ValueError, match="FusedMuon: ns_steps="):
            mk(ns_steps=bad)
    with pytest.raises(ValueError, match="FusedMuon: adjust_lr_fn='rms'"):
        mk(adjust_lr_fn="rms")
    with pytest.raises(ValueError, match="FusedMuon: unknown keyword 'betas'"):
        mk(betas=(0.9, 0.99))
    with pytest.raises(ValueError, match="FusedMuon: ns_coefficients="):
        mk(ns_coefficients=(1.0, 2.0))
    with pytest.raises(ValueError, match="FusedMuon: nesterov=1"):
        mk(nesterov=1)
    with pytest.raises(ValueError, match="FusedMuon: momentum=1.5"):
        mk(momentum=1.5)
    with pytest.raises(ValueError, match="FusedMuon: eps=0"):
        mk(eps=0)
    for key, value in (("momentum", 0.9), ("nesterov", False), ("ns_steps", 3), ("ns_coefficients", (1.0, 2.0, 3.0)),
                       ("adjust_lr_fn", "match_rms_adamw")):
        with pytest.raises(ValueError, match=f"FusedMuon: parameter group 0 sets {key}=.*per-group {key} is not supported"):
            optim.FusedMuon([{"params": ps, key: value}])
    optim.FusedMuon([{"params": list(_store().params.values()), "momentum": 0.95, "ns_steps": 5}])      # the optimiser's own values
    with pytest.raises(ValueError, match=r"FusedMuon: parameter group 1 sets betas=\(0.9, 0.98\); per-group betas"):
        optim.FusedMuon([{"params": ps[:3], "use_muon": False}, {"params": ps[3:], "use_muon": False, "betas": (0.9, 0.98)}])
    with pytest.raises(ValueError, match="FusedMuon: parameter group 0 sets eps=1e-06; per-group eps"):
        optim.FusedMuon([{"params": ps, "use_muon": False, "eps": 1e-6}])
    with pytest.raises(ValueError, match=r"FusedMuon: parameter group 0 has unknown key\(s\) \['trust_clip'\]"):
        optim.FusedMuon([{"params": ps, "trust_clip": True}])
    with pytest.raises(ValueError, match="FusedMuon: parameter group 0 sets use_muon=1"):
        optim.FusedMuon([{"params": ps, "use_muon": 1}])
    with pytest.raises(ValueError, match="FusedMuon: params mixes parameters and group dicts"):
        optim.FusedMuon([ps[0], {"params": ps[1:]}])
    with pytest.raises(ValueError, match="FusedMuon updates the whole flat buffer"):
        optim.FusedMuon(ps[1:])
    with pytest.raises(ValueError, match=f"FusedMuon: parameter {names[0]} is listed twice"):
        optim.FusedMuon([{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match=f"FusedMuon: 1 trainable parameter.*first: {names[-1]}"):
        optim.FusedMuon([{"params": ps[:-1]}])
    # use_muon=True on what the kernel does not take names the tensor
    with pytest.raises(ValueError, match=r"use_muon=True for logit_scale of shape \(\)|use_muon=True for logit_scale"):
        optim.FusedMuon([{"params": [st.params["logit_scale"]], "use_muon": True},
                         {"params": [p for n, p in st.params.items() if n != "logit_scale"]}])
    bias = "visual.transformer.resblocks.0.attn.in_proj_bias"
    with pytest.raises(ValueError, match=f"use_muon=True for {bias} of shape"):
        optim.FusedMuon([{"params": [st.params[bias]], "use_muon": True}, {"params": [p for n, p in st.params.items() if n != bias]}])
    # more than 256 groups after the split
    big = [{"params": []} for _ in range(300)]
    with pytest.raises(ValueError, match="FusedMuon: .* parameter groups; at most 256"):
        optim.FusedMuon(big + [{"params": ps}])


# ------------------------------------------------------------------------------------------------ the default split and the tables
def test_default_split_takes_the_block_linears_of_every_tower():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    groups = optim.muon_param_groups(st.params.items(), lr=0.02, adamw_lr=1e-3, adamw_weight_decay=0.0)
    assert [g["use_muon"] for g in groups] == [True, False]
    assert groups[0]["lr"] == 0.02 and "weight_decay" not in groups[0] and (groups[1]["lr"], groups[1]["weight_decay"]) == (1e-3, 0.0)
    want = [sp.name for sp in st.specs if ".resblocks." in sp.name and sp.name.endswith(BLOCK_LEAVES)]
    assert len(want) == 2 * 2 * 4 and sorted(groups[0]["param_names"]) == sorted(want)         # two towers, two blocks, four Linears
    rest = set(groups[1]["param_names"])
    assert len(rest) + len(want) == len(st.specs)
    for name in ("visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.proj", "text_projection",
                 "token_embedding.weight", "positional_embedding", "logit_scale", "visual.ln_post.weight",
                 "visual.transformer.resblocks.0.attn.in_proj_bias", "visual.transformer.resblocks.1.ln_1.weight"):
        assert name in rest, name
    assert optim.is_muon_name("transformer.resblocks.11.mlp.c_proj.weight") and optim.is_muon_name("gene.transformer.resblocks.0.attn.in_proj_weight")
    for name in ("visual.proj", "gene.fc1.weight", "resblocks.x.mlp.c_fc.weight", "visual.transformer.resblocks.0.mlp.c_fc.bias",
                 "mlp.c_fc.weight", "visual.transformer.resblocks.0.extra.mlp.c_fc.weight"):
        assert not optim.is_muon_name(name), name
    # the gene-MLP's Linears run AdamW: no resblocks above them
    st2 = _store(_tiny_cfg(text=False))
    g2 = optim.muon_param_groups(st2.params.items())
    assert len(g2[0]["param_names"]) == 2 * 4 and all(n.startswith("visual.transformer.resblocks.") for n in g2[0]["param_names"])
    assert any(n.startswith("gene.") for n in g2[1]["param_names"])
    assert optim.muon_shape_ok((64, 8)) and not optim.muon_shape_ok((64, 12)) and not optim.muon_shape_ok((64,)) and not optim.muon_shape_ok((8, 8, 8))
    assert optim.muon_adjust_ratio(None, (192, 64)) == 3 ** 0.5 and optim.muon_adjust_ratio("original", (64, 256)) == 1.0
    assert optim.muon_adjust_ratio("match_rms_adamw", (64, 256)) == 0.2 * 16.0


def _check_tables(opt, st, want_names):
    assert opt.muon_names == want_names
    n_slots = st.total // 64
    assert opt.slot_tensor.dtype == torch.int32 and opt.slot_tensor.numel() == n_slots and opt.chunk_group.numel() == n_slots
    assert opt.tensor_info.shape == (max(len(want_names), 1), 4) and opt.slot_sums.numel() == n_slots
    seen = torch.zeros(n_slots, dtype=torch.int32)
    x_slot = 0
    for ti, name in enumerate(want_names):
        sp = st.by_name[name]
        lo, hi, xs, _ = opt.tensor_info[ti].tolist()
        assert lo == sp.offset // 64 and (hi - lo) * 64 == sp.numel and xs == x_slot
        assert bool((opt.slot_tensor[lo:hi] == ti).all())
        seen[lo:hi] += 1
        x_slot += hi - lo
        assert abs(float(opt.ratio[ti]) - max(1.0, sp.shape[0] / sp.shape[1]) ** 0.5) < 1e-6
    assert opt.compact_slots == x_slot and opt.x0.numel() == opt.x1.numel() == max(64 * x_slot, 64)
    assert int(seen.max()) <= 1 and int(seen.sum()) == int((opt.slot_tensor >= 0).sum())        # every Muon slot once
    assert bool((opt.slot_tensor[seen == 0] == -1).all())
    assert opt.muon_shapes == [tuple(st.by_name[n].shape) for n in want_names]
    assert opt.gbuf.numel() == opt.pbuf.numel() >= max([min(s_) ** 2 for s_ in opt.muon_shapes] + [64])
    assert opt.acc.dtype == torch.float32 and opt.acc.numel() >= max([s_[0] * s_[1] for s_ in opt.muon_shapes] + [64])


def test_tensor_tables_cover_every_muon_tensor_once():
    comm, lock, mc, optim, params = _pkg()
    st = _store()
    opt = optim.FusedMuon(list(st.params.values()))
    want = [sp.name for sp in st.specs if ".resblocks." in sp.name and sp.name.endswith(BLOCK_LEAVES)]
    _check_tables(opt, st, want)
    assert sorted(set(opt.muon_shapes)) == [(64, 64), (64, 256), (192, 64), (256, 64)]
    assert opt._uses_table() and opt.group_hyper.numel() == 2 + 2 * 2
    by_group = {n: gi for gi, g in enumerate(opt.param_groups) for n in g["param_names"]}
    for sp in st.specs:
        lo = sp.offset // 64
        assert int(opt.chunk_group[lo]) == by_group[sp.name]
    # the module's no-decay groups carry no use_muon and are split by the default rule: three groups
    st2 = _store()
    opt2 = optim.FusedMuon(optim.open_clip_param_groups(st2.params.items(), 0.05), lr=0.02, adamw_lr=1e-3)
    assert [(g["use_muon"], g["lr"], g["weight_decay"]) for g in opt2.param_groups] == [(False, 1e-3, 0.0), (True, 0.02, 0.05),
                                                                                       (False, 1e-3, 0.05)]
    _check_tables(opt2, st2, want)
    # every group use_muon=False: no Muon tensor, one AdamW group
    st3 = _store()
    opt3 = optim.FusedMuon([{"params": list(st3.params.values()), "use_muon": False}])
    assert opt3.muon_names == [] and len(opt3.param_groups) == 1 and bool((opt3.slot_tensor == -1).all()) and opt3.chunk_group is not None
    # use_muon=True on a matrix outside the default rule
    st4 = _store()
    extra = "text_projection"
    opt4 = optim.FusedMuon([{"params": [st4.params[extra]], "use_muon": True},
                            {"params": [p for n, p in st4.params.items() if n != extra]}])
    assert extra in opt4.muon_names and len(opt4.muon_names) == len(want) + 1 and len(opt4.param_groups) == 3


def test_tables_under_a_lock_hold_no_locked_matrix():
    comm, lock, mc, optim, params = _pkg()
    cfg = _tiny_cfg()
    st = _store(cfg)
    locked, free = lock.split_groups(lock.vision_groups(cfg.vision.layers), 0)
    st.unlock(free)
    st.lock(locked)
    opt = optim.FusedMuon(list(st.params.values()))
    want = [n for n in st.trainable_names() if ".resblocks." in n and n.endswith(BLOCK_LEAVES)]
    assert len(want) == 2 * 4 and not any(n.startswith("visual.") for n in want)
    _check_tables(opt, st, want)
    assert sorted(set(opt.muon_shapes)) == [(64, 64), (64, 256), (192, 64), (256, 64)]
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == st.trainable_floats() < st.total
    for n in st.locked:
        sp = st.by_name[n]
        assert bool((opt.slot_tensor[sp.offset // 64:(sp.offset + max(sp.numel, 1) + 63) // 64] == -1).all())


# ------------------------------------------------------------------------------------------------ Hydra surface
def test_the_target_maps_to_fused_muon():
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    assert H._locate("torch.optim.Muon") is optim.FusedMuon
    part = H.instantiate({"_target_": "torch.optim.Muon", "_partial_": True, "lr": 3e-3})
    assert isinstance(part, functools.partial) and part.func is optim.FusedMuon and part.keywords == {"lr": 3e-3}
    assert H._locate("torch.optim.AdamW") is optim.FusedAdamW and H._locate("timm.optim.Lamb") is optim.FusedLamb


def test_muon_configs_compose_to_a_fused_muon_partial(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import hydra_lite as H
    adamw = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    want = {"lr": 1e-3, "weight_decay": 0.1, "momentum": 0.95, "nesterov": True, "ns_coefficients": [3.4445, -4.7750, 2.0315],
            "eps": 1e-7, "ns_steps": 5, "adjust_lr_fn": "match_rms_adamw", "adamw_lr": None, "adamw_betas": [0.9, 0.98],
            "adamw_eps": 1e-6, "adamw_weight_decay": None}
    for over in (["optimizer=muon"], ["experiment=vitb16_gene_b256_muon"]):
        cfg = H.compose("train.yaml", over)
        assert cfg["_choices_"]["optimizer"] == "muon" and cfg.optimizer["_target_"] == "torch.optim.Muon"
        part = H.instantiate(cfg.optimizer)
        assert isinstance(part, functools.partial) and part.func is optim.FusedMuon and part.keywords == want
        opt = part(params=list(_store().params.values()))         # the keywords are all accepted
        assert isinstance(opt, optim.FusedMuon) and opt.adjust_lr_fn == "match_rms_adamw" and opt.param_groups[1]["betas"] == (0.9, 0.98)
        assert abs(float(opt.ratio[0]) - 0.2 * 192 ** 0.5) < 1e-6
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_muon"])
    assert cfg["model"]["net"] == adamw["model"]["net"] and cfg.data.batch_size == 256
    assert dict(cfg["model"]["param_groups"]) == {"no_decay": "open_clip"}
    assert cfg["loss"] == adamw["loss"] and cfg["trainer"] == adamw["trainer"]


def test_param_groups_of_the_module_compose_with_the_split():
    comm, lock, mc, optim, params = _pkg()
    from spatial_clip_amd import module

    class _Net:
        store = _store()
    for part, lr, wd in ((functools.partial(optim.FusedMuon, lr=2e-2, weight_decay=0.05), 2e-2, 0.05),
                         (functools.partial(optim.FusedMuon), 1e-3, 0.1)):
        m = module.SpatialClipLitModule.__new__(module.SpatialClipLitModule)
        torch.nn.Module.__init__(m)
        m.net, m.param_groups = _Net(), optim.check_param_groups_cfg({"no_decay": "open_clip"})
        m.hparams = type("H", (), {"optimizer_cfg": part})()
        groups = m.optimizer_param_groups()
        assert not any("use_muon" in g for g in groups)
        opt = part(params=groups)
        assert isinstance(opt, optim.FusedMuon)
        assert [(g["use_muon"], g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(False, lr, 0.0), (True, lr, wd), (False, lr, wd)]
        assert len(opt.muon_names) == 16


# ------------------------------------------------------------------------------------------------ state on a host-side store
def test_state_dict_keys_and_the_kind_matrix():
    comm, lock, mc, optim, params = _pkg()
    mk = lambda cls, **kw: cls(list(_store().params.values()), **kw)       # noqa: E731
    opts = {"adamw": mk(optim.FusedAdamW), "lion": mk(optim.FusedLion), "lamb": mk(optim.FusedLamb), "muon": mk(optim.FusedMuon, lr=2e-2)}
    muon = opts["muon"]
    muon.step_count, muon.exp_avg[:], muon.exp_avg_sq[:] = 7, 0.25, 0.5
    sds = {k: o.state_dict() for k, o in opts.items()}
    sd = sds["muon"]
    assert list(sd) == ["optimizer", "step", "exp_avg", "exp_avg_sq", "param_groups"] and sd["optimizer"] == "muon" and sd["step"] == 7
    assert sd["exp_avg"].numel() == sd["exp_avg_sq"].numel() == muon.store.total and "params" not in sd["param_groups"][0]
    assert [g["use_muon"] for g in sd["param_groups"]] == [True, False] and sd["param_groups"][0]["lr"] == 2e-2
    for mine, opt in opts.items():
        for theirs, file in sds.items():
            if mine == theirs:
                opt.load_state_dict(file)
                continue
            before = opt.step_count
            with pytest.raises(ValueError, match=f"(?s){opt.NAME}.*{theirs!r}.*{mine!r}"):
                opt.load_state_dict(file)
            assert opt.step_count == before         # a refused load changes nothing
    with pytest.raises(ValueError, match="AdamW, Lion, LAMB and Muon states do not convert into each other"):
        opts["adamw"].load_state_dict(sd)
    with pytest.raises(ValueError, match="AdamW, Lion and LAMB states do not convert into each other"):      # as it was
        opts["adamw"].load_state_dict(sds["lamb"])
    fresh = mk(optim.FusedMuon)
    fresh.load_state_dict(sd)
    assert fresh.step_count == 7 and bool((fresh.exp_avg == 0.25).all()) and bool((fresh.exp_avg_sq == 0.5).all())


def test_sharded_exchange_is_refused():
    comm, lock, mc, optim, params = _pkg()
    assert optim.FusedMuon.SHARDABLE is False
    opt = optim.FusedMuon(list(_store().params.values()))
    ex = comm.ShardedGradExchange.__new__(comm.ShardedGradExchange)
    with pytest.raises(ValueError, match="FusedMuon.*sharded"):
        opt.attach_exchange(ex)
    assert opt.exchange is None
    opt.attach_exchange(None)
    assert opt.exchange is None
