"""Optimiser parameter groups without a device: the slot table, the two group builders (open_clip's no-decay rule against the
reference's own lists, tests/golden/param_groups_manifest.json; the learning-rate scaling by name prefix), every refusal of
``FusedAdamW`` and of the ``param_groups`` key, the checkpoint entries -- and the condition the GPU kernel test rests on:
torch's own fp32 grouped AdamW step meets the reference-relative rule on exactly that test's inputs."""
import functools
import json
import os

import pytest
import torch

from tests import _groupcases as C
from tests import _refbounds as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import model_configs as mc, optim, params
    return mc, optim, params


def _tiny_text_cfg():
    mc, optim, params = _pkg()
    with open(os.path.join(GOLDEN, "lock_groups_manifest.json")) as f:
        c = json.load(f)["cfg"]
    v, t = c["vision_cfg"], c["text_cfg"]
    return mc.ModelCfg(embed_dim=c["embed_dim"],
                       vision=mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64)),
                       text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)


def _store(cfg):
    """A ParamStore laid out on the host; no kernel runs (init=False)."""
    mc, optim, params = _pkg()
    st = params.ParamStore(cfg, torch.device("cpu"), init=False)
    for p in st.params.values():
        p._sc_store = st
    return st


def _adamw(groups, **kw):
    mc, optim, params = _pkg()
    return optim.FusedAdamW(groups, **{"lr": 1e-3, "betas": (0.9, 0.98), "eps": 1e-6, "weight_decay": 0.1, **kw})


# ------------------------------------------------------------------------------------------------ the slot table
@pytest.mark.parametrize("model", ["tiny-text", "ViT-B-16-gene"])
def test_slot_table_gives_every_slot_of_a_parameter_its_group(model):
    mc, optim, params = _pkg()
    cfg = _tiny_text_cfg() if model == "tiny-text" else mc.get_model_config("ViT-B-16-gene", n_genes=20000)
    st = _store(cfg)
    groups = optim.scaled_lr_groups(optim.open_clip_param_groups(st.params.items(), 0.1), 1e-3, {"visual.": 0.1})
    assert len(groups) == 4
    opt = _adamw(groups)
    table = opt.chunk_group
    assert table.dtype == torch.uint8 and table.numel() == st.total // 64 and st.total % 64 == 0
    want = [0] * (st.total // 64)                   # per-name loop; slots of no parameter read 0
    owned = [False] * (st.total // 64)
    for gi, g in enumerate(opt.param_groups):
        for p in g["params"]:
            name = next(n for n, q in st.params.items() if q is p)
            sp = st.by_name[name]
            assert sp.offset % 64 == 0
            for slot in range(sp.offset // 64, (sp.offset + max(sp.numel, 1) + 63) // 64):
                assert not owned[slot], f"{name} shares slot {slot} with another parameter"
                want[slot], owned[slot] = gi, True
    assert table.tolist() == want
    assert all(owned[:st.specs[-1].offset // 64 + 1]) and sorted(set(want)) == [0, 1, 2, 3]
    # what the groups say: vectors and scalars without decay; the image tower at a tenth of the learning rate
    by_name = {n: g for g in opt.param_groups for n in g["param_names"]}
    assert by_name["logit_scale"]["weight_decay"] == 0.0 and by_name["logit_scale"]["lr"] == 1e-3
    assert by_name["visual.ln_post.weight"]["weight_decay"] == 0.0 and by_name["visual.ln_post.weight"]["lr"] == pytest.approx(1e-4)
    assert by_name["visual.proj"]["weight_decay"] == 0.1 and by_name["visual.proj"]["lr"] == pytest.approx(1e-4)
    second = "text_projection" if model == "tiny-text" else "gene.fc2.weight"
    assert by_name[second]["weight_decay"] == 0.1 and by_name[second]["lr"] == 1e-3
    assert all(g["initial_lr"] == g["lr"] and g["betas"] == (0.9, 0.98) and g["eps"] == 1e-6 for g in opt.param_groups)


# ------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize("model", ["ViT-B-16", "ViT-B-32", "ViT-L-14"])
def test_open_clip_groups_reproduce_the_references_no_decay_list(model):
    mc, optim, params = _pkg()
    with open(os.path.join(GOLDEN, "state_dict_manifest.json")) as f:
        shapes = json.load(f)[model]
    with open(os.path.join(GOLDEN, "param_groups_manifest.json")) as f:
        man = json.load(f)[model]
    assert len(shapes) == man["parameters"]         # (a CLIP state dict of these models holds parameters only)
    named = [(n, torch.empty(s, device="meta")) for n, s in shapes.items()]
    groups = optim.open_clip_param_groups(named, 0.2)
    assert len(groups) == 2 and groups[0]["weight_decay"] == 0.0 and groups[1]["weight_decay"] == 0.2
    assert sorted(groups[0]["param_names"]) == sorted(man["no_decay"])
    assert sorted(groups[0]["param_names"] + groups[1]["param_names"]) == sorted(shapes)       # every name exactly once
    assert [tuple(p.shape) for p in groups[0]["params"]] == [tuple(shapes[n]) for n in groups[0]["param_names"]]
    assert "weight_decay" not in optim.open_clip_param_groups(named)[1]       # None: the optimiser's default applies


def test_open_clip_groups_take_the_stores_names_and_skip_locked_parameters():
    mc, optim, params = _pkg()
    st = _store(_tiny_text_cfg())
    mangled = [(n.replace(".", "__"), p) for n, p in st.params.items()]       # what net.named_parameters() yields
    groups = optim.open_clip_param_groups(mangled, 0.1)
    with open(os.path.join(GOLDEN, "train3_tiny_text_groups.npz"), "rb") as f:
        import numpy as np
        want = json.loads(str(np.load(f, allow_pickle=False)["no_decay"]))
    assert sorted(groups[0]["param_names"]) == sorted(want)
    assert sorted(groups[0]["param_names"] + groups[1]["param_names"]) == sorted(st.params)
    st.lock([n for n in st.params if n.startswith("visual.")])
    left = optim.open_clip_param_groups(mangled, 0.1)
    assert not any(n.startswith("visual.") for g in left for n in g["param_names"])
    assert sorted(n for g in left for n in g["param_names"]) == sorted(st.trainable_names())


def test_scaled_lr_groups_split_by_the_longest_prefix():
    mc, optim, params = _pkg()
    st = _store(_tiny_text_cfg())
    base = [{"params": list(st.params.values()), "weight_decay": 0.05}]
    scale = {"visual.": 0.1, "visual.transformer.resblocks.1.": 0.5, "logit_scale": 2.0, "nothing.": 3.0}
    out = optim.scaled_lr_groups(base, 1e-3, scale)
    lrs = [g.get("lr") for g in out]
    assert lrs == [None, pytest.approx(1e-4), pytest.approx(5e-4), pytest.approx(2e-3)]      # unmatched first, then in key order
    assert all(g["weight_decay"] == 0.05 for g in out)
    for g, lr in zip(out, lrs):
        for n in g["param_names"]:
            if n.startswith("visual.transformer.resblocks.1."):
                assert lr == pytest.approx(5e-4), n
            elif n.startswith("visual."):
                assert lr == pytest.approx(1e-4), n
            elif n == "logit_scale":
                assert lr == pytest.approx(2e-3)
            else:
                assert lr is None, n
    assert sorted(n for g in out for n in g["param_names"]) == sorted(st.params)
    # a group's own lr is the base of its scaled part
    own = optim.scaled_lr_groups([{"params": list(st.params.values()), "lr": 4e-3}], 1e-3, {"visual.": 0.25})
    assert [g["lr"] for g in own] == [4e-3, pytest.approx(1e-3)]
    for bad in ({"visual.": 0.0}, {"visual.": -1.0}, {"": 0.5}, {"visual.": "fast"}, {"visual.": float("nan")}):
        with pytest.raises(ValueError, match="lr_scale"):
            optim.scaled_lr_groups(base, 1e-3, bad)
    with pytest.raises(ValueError, match="lr_scale"):
        optim.scaled_lr_groups(base, 1e-3, [("visual.", 0.1)])


# ------------------------------------------------------------------------------------------------ FusedAdamW's refusals
def test_every_refusal_names_the_parameter_or_the_key():
    mc, optim, params = _pkg()
    st = _store(_tiny_text_cfg())
    ps = list(st.params.values())
    half = len(ps) // 2
    with pytest.raises(ValueError, match="listed twice") as e:
        _adamw([{"params": ps[:half + 1]}, {"params": ps[half:]}])
    assert st.specs[half].name in str(e.value)
    with pytest.raises(ValueError, match="in no group") as e:
        _adamw([{"params": ps[:half]}, {"params": ps[half + 1:]}])
    assert st.specs[half].name in str(e.value)
    other = _store(_tiny_text_cfg())
    with pytest.raises(ValueError, match="another SpatialClipNet"):
        _adamw([{"params": ps}, {"params": list(other.params.values())}])
    with pytest.raises(ValueError, match="no parameter of a SpatialClipNet"):
        _adamw([{"params": ps}, {"params": [torch.nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError, match="betas"):
        _adamw([{"params": ps[:half]}, {"params": ps[half:], "betas": (0.9, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        _adamw([{"params": ps[:half]}, {"params": ps[half:], "eps": 1e-8}])
    _adamw([{"params": ps[:half], "betas": [0.9, 0.98], "eps": 1e-6}, {"params": ps[half:]}])       # equal values are fine
    st = _store(_tiny_text_cfg())
    ps = list(st.params.values())
    with pytest.raises(ValueError, match="momentum"):
        _adamw([{"params": ps, "momentum": 0.9}])
    with pytest.raises(ValueError, match="no 'params'"):
        _adamw([{"lr": 1e-3}])
    with pytest.raises(ValueError, match="257 parameter groups"):
        _adamw([{"params": []} for _ in range(257)])
    with pytest.raises(ValueError, match="mixes"):
        _adamw([{"params": ps[:half]}] + ps[half:])
    # the un-grouped form keeps its own message
    with pytest.raises(ValueError, match="pass all parameters"):
        _adamw(ps[:half])


def test_locked_parameters_may_be_in_a_group_or_in_none():
    mc, optim, params = _pkg()
    for listed in (True, False):
        st = _store(_tiny_text_cfg())
        st.lock([n for n in st.params if n.startswith("visual.")])
        named = [(n, p) for n, p in st.params.items() if listed or p.requires_grad]
        no_decay = [p for n, p in named if p.ndim < 2]
        rest = [p for n, p in named if p.ndim >= 2]
        opt = _adamw([{"params": no_decay, "weight_decay": 0.0}, {"params": rest}])
        assert opt.exp_avg.numel() == st.trainable_floats() < st.total and opt.ranges == st.trainable_ranges()
        assert sum(len(g["params"]) for g in opt.param_groups) == (len(st.params) if listed else len(st.trainable_names()))
        slot = st.by_name["text_projection"].offset // 64
        assert int(opt.chunk_group[slot]) == 1 and int(opt.chunk_group[st.by_name["ln_final.bias"].offset // 64]) == 0


def test_one_group_is_the_ungrouped_optimiser_and_state_dicts_carry_the_names():
    mc, optim, params = _pkg()
    st = _store(_tiny_text_cfg())
    ps = list(st.params.values())
    one = _adamw([{"params": ps, "lr": 2e-3}])
    assert len(one.param_groups) == 1 and one.chunk_group is None and one.group_hyper is None
    assert one.param_groups[0]["lr"] == one.param_groups[0]["initial_lr"] == 2e-3 and one.param_groups[0]["weight_decay"] == 0.1
    sd = one.state_dict()
    assert sd["param_groups"][0]["param_names"] == [s.name for s in st.specs] and "params" not in sd["param_groups"][0]
    st2 = _store(_tiny_text_cfg())
    plain = _adamw(list(st2.params.values()))
    assert plain.chunk_group is None and list(plain.state_dict()["param_groups"][0]) == ["lr", "initial_lr", "betas", "eps", "weight_decay"]
    st3 = _store(_tiny_text_cfg())
    groups = optim.open_clip_param_groups(st3.params.items(), 0.1)
    two = _adamw(groups)
    sd = two.state_dict()
    assert len(sd["param_groups"]) == 2
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, 0.1]
    assert sorted(sd["param_groups"][0]["param_names"] + sd["param_groups"][1]["param_names"]) == sorted(st3.params)
    assert sd["exp_avg"].numel() == st3.total         # moments stay in the flat layout: the file resumes under any grouping
    two.param_groups[0]["lr"] = 123.0
    two.load_state_dict(sd)                            # stored hyper-parameters are ignored, as before
    assert two.param_groups[0]["lr"] == 123.0
    plain.load_state_dict(sd)
    # LambdaLR walks every group
    sched = optim.get_cosine_schedule_with_warmup(two, num_warmup_steps=2, num_training_steps=10)
    two.param_groups[0]["initial_lr"], two.param_groups[1]["initial_lr"] = 1e-3, 4e-3
    sched.step()
    assert sched.get_last_lr() == [pytest.approx(5e-4), pytest.approx(2e-3)]


def test_sharded_exchange_refuses_more_than_one_group():
    mc, optim, params = _pkg()
    from spatial_clip_amd import comm
    st = _store(_tiny_text_cfg())
    opt = _adamw(optim.open_clip_param_groups(st.params.items(), 0.1))
    ex = comm.ShardedGradExchange.__new__(comm.ShardedGradExchange)
    with pytest.raises(ValueError, match="parameter groups.*sharded"):
        opt.attach_exchange(ex)
    opt.attach_exchange(None)


def test_group_scalars_reach_the_staging_buffer():
    """The host half of a grouped step: {1 - b1^t, sqrt(1 - b2^t)} as the un-grouped captured step forms them, then every
    group's (lr, weight_decay) as the scheduler left them."""
    mc, optim, params = _pkg()
    from spatial_clip_amd import _lib
    st = _store(_tiny_text_cfg())
    opt = _adamw(optim.open_clip_param_groups(st.params.items(), 0.1))
    opt.param_groups[1]["lr"] = 7e-4
    opt.step_count = 5
    opt.refresh_hyper()
    three = torch.zeros(3)
    _lib.check(_lib.lib().sc_adamw_hyper_host(1e-3, 0.9, 0.98, 5, three.data_ptr()), "sc_adamw_hyper_host")
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert opt.hyper is None and opt.group_hyper.tolist() == [float(three[1]), float(three[2]), f32(1e-3), 0.0, f32(7e-4), f32(0.1)]


# ------------------------------------------------------------------------------------------------ the module's key
def test_param_groups_key_is_checked_when_the_module_is_built():
    mc, optim, params = _pkg()
    ok = optim.check_param_groups_cfg({"no_decay": "open_clip", "lr_scale": {"visual.": 0.1}})
    assert ok == {"no_decay": "open_clip", "lr_scale": {"visual.": 0.1}}
    assert optim.check_param_groups_cfg(None) is None and optim.check_param_groups_cfg({}) == {"no_decay": None, "lr_scale": None}
    fn = lambda net: []
    assert optim.check_param_groups_cfg(fn) is fn
    with pytest.raises(ValueError, match="nodecay"):
        optim.check_param_groups_cfg({"nodecay": "open_clip"})
    with pytest.raises(ValueError, match="timm"):
        optim.check_param_groups_cfg({"no_decay": "timm"})
    with pytest.raises(ValueError, match=r"lr_scale\['visual.'\]=0"):
        optim.check_param_groups_cfg({"lr_scale": {"visual.": 0}})
    with pytest.raises(ValueError, match=r"lr_scale\['gene.'\]=-0.5"):
        optim.check_param_groups_cfg({"lr_scale": {"visual.": 1.0, "gene.": -0.5}})
    with pytest.raises(ValueError, match="param_groups"):
        optim.check_param_groups_cfg("open_clip")


def test_module_builds_the_groups_from_its_key():
    """configure_optimizers without a device: a stand-in net that owns a host-side store."""
    mc, optim, params = _pkg()
    from spatial_clip_amd import module

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.store = _store(_tiny_text_cfg())
            self.cfg, self.device_ = self.store.cfg, torch.device("cpu")
            for n, p in self.store.params.items():
                self.register_parameter(n.replace(".", "__"), p)

    class Loss(torch.nn.Module):
        def forward(self, image_features, text_features, logit_scale):
            return {"contrastive_loss": None}

    cfg = functools.partial(optim.FusedAdamW, lr=2e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
    m = module.SpatialClipLitModule(Net(), Loss(), cfg, None, param_groups={"no_decay": "open_clip", "lr_scale": {"visual.": 0.1}})
    opt = m.configure_optimizers()["optimizer"]
    got = [(g["lr"], g["weight_decay"]) for g in opt.param_groups]
    assert got == [(2e-3, 0.0), (pytest.approx(2e-4), 0.0), (2e-3, 0.2), (pytest.approx(2e-4), 0.2)]
    first = opt.param_groups[0]["param_names"] + opt.param_groups[1]["param_names"]
    assert "logit_scale" in first and all(n in first for n in m.net.store.params if "ln_" in n or n.endswith("bias"))
    # a callable gets the net; None is the reference's un-grouped call
    m = module.SpatialClipLitModule(Net(), Loss(), cfg, None,
                                    param_groups=lambda net: [{"params": list(net.store.params.values()), "lr": 5e-3}])
    opt = m.configure_optimizers()["optimizer"]
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 5e-3 and opt.chunk_group is None
    m = module.SpatialClipLitModule(Net(), Loss(), cfg, None)
    opt = m.configure_optimizers()["optimizer"]
    assert len(opt.param_groups) == 1 and "param_names" not in opt.param_groups[0] and opt.param_groups[0]["lr"] == 2e-3
    with pytest.raises(ValueError, match="decay_rule"):
        module.SpatialClipLitModule(Net(), Loss(), cfg, None, param_groups={"decay_rule": "open_clip"})


def test_new_experiments_compose_and_carry_the_key(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import hydra_lite as H, module, optim
    base = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    assert "param_groups" not in base["model"]
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_nodecay"])
    assert dict(cfg["model"]["param_groups"]) == {"no_decay": "open_clip"}
    assert cfg["model"]["net"] == base["model"]["net"] and cfg.data.batch_size == 256
    lit = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lit_lr"])
    assert lit["model"]["net"]["lock_image"] is True and int(lit["model"]["net"]["lock_image_unlocked_groups"]) == 2
    assert optim.check_param_groups_cfg(H.instantiate(lit["model"]["param_groups"])) == \
        {"no_decay": "open_clip", "lr_scale": {"visual.": 0.1}}
    over = H.compose("train.yaml", ["experiment=vitb16_gene_b256", "model.param_groups={no_decay: open_clip}"])
    assert dict(over["model"]["param_groups"]) == {"no_decay": "open_clip"}
    assert H._locate(cfg["model"]["_target_"]) is module.SpatialClipLitModule
    with pytest.raises(ValueError, match="lr_scale"):
        optim.check_param_groups_cfg(H.instantiate(H.compose(
            "train.yaml", ["experiment=vitb16_gene_b256_lit_lr", "model.param_groups.lr_scale={visual.: 0}"])["model"]["param_groups"]))


# ------------------------------------------------------------------------------------------------ the kernel test's reference
@pytest.mark.parametrize("name", list(C.CASES))
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_torch_fp32_grouped_step_meets_the_rule_of_the_kernel_test(name, clip):
    """On the inputs of tests/test_gpu_adamw_groups.py (same buffers, gradients, steps, group scalars; a clip coefficient of
    the size that test produces), torch.optim.AdamW(foreach=False) with real parameter groups in fp32 lies within
    REF_FACTOR * E32 + ulp of the same optimiser in float64, per group and tensor: the rule the kernel is held to is one the
    reference arithmetic itself meets, with E32 > 0 wherever anything is rounded.  The state advances along the fp32 run."""
    case = C.CASES[name]()
    p, m, v = C.start(case.n)
    c = 0.5 if clip else 1.0
    frozen = C.FROZEN_GROUP.get(name)
    for step, lr in C.ADAM_STEPS:
        grad = C._adam_grad(case.n, step)
        ref64 = C.torch_grouped(case, p, m, v, grad.double() * C.GS * c, step, lr, torch.float64)
        ref32 = C.torch_grouped(case, p, m, v, grad * C.GS * C._f32(c), step, lr, torch.float32)
        nonzero = 0
        for g in range(case.n_groups):
            for what, r64, r32 in zip("pmv", ref64[g], ref32[g]):
                ref = R.Ref(r64, r32)
                assert ref.e32 == ref.e32 and ref.e32 < float("inf")
                ratio = R._ratio((r32.double() - ref.r64).abs(), ref.allowed_f32())
                assert ratio <= 1.0, f"step {step} group {g} {what}: torch's fp32 step at {ratio} of the allowance"
                nonzero += ref.e32 > 0
            if g == frozen:
                assert torch.equal(ref32[g][0], case.gather(p, g)) and torch.equal(ref64[g][0], case.gather(p, g).double())
                assert not torch.equal(ref32[g][1], case.gather(m, g))
        assert nonzero >= case.n_groups           # the moments, at least, are rounded in every group
        for g in range(case.n_groups):
            for flat, new in zip((p, m, v), ref32[g]):
                C.scatter(case, flat, g, new)
        assert bool((m[1::97] == 0).all()) and bool((v[1::97] == 0).all())
