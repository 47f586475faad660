"""Locked towers (LiT) without a device: which parameters ``lock_image_tower`` / ``lock_text_tower`` freeze (against the
reference's own lists, tests/golden/lock_groups_manifest.json), the trainable ranges of the flat buffers, the refusals, the
Hydra experiment, the optimiser's checkpoint layout and the gradient reducer's complement."""
import json
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _manifest():
    with open(os.path.join(GOLDEN, "lock_groups_manifest.json")) as f:
        return json.load(f)


def _tiny_cfg(man=None, gene=False):
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import model_configs as mc
    c = (man or _manifest())["cfg"]
    v, t = c["vision_cfg"], c["text_cfg"]
    vision = mc.VisionCfg(v["image_size"], v["patch_size"], v["width"], v["layers"], v.get("head_width", 64))
    if gene:
        return mc.ModelCfg(embed_dim=c["embed_dim"], vision=vision, text=None, gene=mc.GeneCfg(100, 64))
    return mc.ModelCfg(embed_dim=c["embed_dim"], vision=vision,
                       text=mc.TextCfg(t["context_length"], t["vocab_size"], t["width"], t["heads"], t["layers"]), gene=None)


def _store(cfg):
    """A ParamStore laid out on the host; no kernel runs (init=False)."""
    from spatial_clip_amd import params
    st = params.ParamStore(cfg, torch.device("cpu"), init=False)
    for p in st.params.values():
        p._sc_store = st
    return st


def _lock(st, cfg, image=None, text=None):
    """What SpatialClipNet.lock_image_tower / lock_text_tower do to the store."""
    from spatial_clip_amd import lock
    if image is not None:
        locked, free = lock.split_groups(lock.vision_groups(cfg.vision.layers), image)
        st.unlock(free)
        st.lock(locked)
    if text is not None:
        locked, free = lock.split_groups(lock.text_groups(cfg.text.layers), text)
        st.unlock(free)
        st.lock(locked)


def _check_ranges(st):
    from spatial_clip_amd.params import ALIGN
    ranges = st.trainable_ranges()
    assert ranges == sorted(ranges) and len(ranges) <= 3
    for (lo, hi), nxt in zip(ranges, ranges[1:] + [(st.total + 1, None)]):
        assert 0 <= lo < hi <= st.total and lo % ALIGN == 0 and hi % ALIGN == 0
        assert hi < nxt[0], "touching ranges must have been merged"
    inside = lambda s: any(lo <= s.offset and s.offset + max(s.numel, 1) <= hi for lo, hi in ranges)
    overlaps = lambda s: any(lo < s.offset + max(s.numel, 1) and s.offset < hi for lo, hi in ranges)
    for s in st.specs:
        if s.name in st.locked:
            assert not overlaps(s), s.name
        else:
            assert inside(s), s.name
    return ranges


@pytest.mark.parametrize("tower", ["image", "text"])
def test_trainable_names_and_ranges_equal_the_reference_for_every_group_count(tower):
    man = _manifest()
    cfg = _tiny_cfg(man)
    layers = cfg.vision.layers if tower == "image" else cfg.text.layers
    assert sorted(int(k) for k in man[tower]) == list(range(layers + 4))
    for count in range(layers + 4):
        st = _store(cfg)
        _lock(st, cfg, **{tower: count})
        want = sorted(man[tower][str(count)])       # (the reference lists its parameters in module order, the store in forward order)
        assert sorted(st.trainable_names()) == want, (tower, count)
        assert sorted(n for n, p in st.params.items() if p.requires_grad) == want
        assert st.trainable_names() == [s.name for s in st.specs if s.name in set(want)]
        assert all(st.params[n].grad is None for n in st.locked)
        assert "logit_scale" in want
        ranges = _check_ranges(st)
        assert sum(hi - lo for lo, hi in ranges) == st.trainable_floats()
        if count >= layers + 2:
            assert ranges == [(0, st.total)] and not st.locked
    # the layout facts: an image lock leaves a suffix of the vision range plus everything behind it -- one range; a text lock
    # leaves the vision range, a suffix of the text range and the scalars
    st = _store(cfg)
    _lock(st, cfg, image=2)
    (lo, hi), = st.trainable_ranges()
    assert lo == st.by_name["visual.transformer.resblocks.1.ln_1.weight"].offset and hi == st.total
    st = _store(cfg)
    _lock(st, cfg, text=0)
    assert st.trainable_ranges() == [(0, st.by_name["token_embedding.weight"].offset),
                                     (st.by_name["logit_scale"].offset, st.total)]
    st = _store(cfg)
    _lock(st, cfg, image=1, text=1)
    assert st.trainable_ranges() == [(st.by_name["visual.proj"].offset, st.by_name["token_embedding.weight"].offset),
                                     (st.by_name["text_projection"].offset, st.total)]


def test_relocking_with_another_count_replaces_the_lock_and_zeroes_the_locked_gradient():
    cfg = _tiny_cfg()
    man = _manifest()
    st = _store(cfg)
    st.grad.fill_(1.0)
    _lock(st, cfg, image=0)
    _lock(st, cfg, image=2)
    assert sorted(st.trainable_names()) == sorted(man["image"]["2"])
    assert st.params["visual.proj"].grad.data_ptr() == st.g("visual.proj").data_ptr()
    for s in st.specs:
        g = st.grad[s.offset:s.offset + s.numel]
        # the parts locked by EITHER call were zeroed once; what was never locked is untouched
        assert float(g.abs().max()) == (0.0 if s.name.startswith("visual.") else 1.0), s.name


def test_tower_lock_floor_positions():
    from spatial_clip_amd.lock import TowerLock
    for layers in (1, 2, 4):
        free = TowerLock(layers)
        assert (free.floor, free.stem, free.proj, free.head_only) == (0, True, True, False)
        none = TowerLock(layers, 0)
        assert not none.any_trainable and none.floor == layers and not none.stem
        head = TowerLock(layers, 1)
        assert head.head_only and head.floor == layers and not head.stem
        for g in range(2, layers + 2):
            lk = TowerLock(layers, g)
            assert lk.floor == layers + 1 - g and lk.proj and not lk.head_only and not lk.stem
        for g in (layers + 2, layers + 5):
            lk = TowerLock(layers, g)
            assert (lk.floor, lk.stem, lk.proj) == (0, True, True)


def test_refusals_before_anything_is_built(monkeypatch):
    """The ValueErrors of the constructor come before the device is looked at."""
    import spatial_clip_amd  # noqa: F401
    import inspect
    from spatial_clip_amd import net
    par = inspect.signature(net.SpatialClipNet.__init__).parameters
    assert [par[k].default for k in ("lock_image", "lock_image_unlocked_groups", "lock_text", "lock_text_unlocked_layers")] \
        == [False, 0, False, 0]
    assert inspect.signature(net.SpatialClipNet.lock_image_tower).parameters["freeze_bn_stats"].default is False
    assert inspect.signature(net.SpatialClipNet.lock_text_tower).parameters["freeze_layer_norm"].default is True
    monkeypatch.delenv("SC_GRAD_EXCHANGE", raising=False)
    with pytest.raises(ValueError, match="fp8"):
        net.SpatialClipNet("ViT-B-16-gene", None, precision="fp8", lock_image=True)
    with pytest.raises(ValueError, match="fp8"):
        net.SpatialClipNet("ViT-B-32", None, precision="fp8-mixed", lock_text=True)
    with pytest.raises(ValueError, match="text"):
        net.SpatialClipNet("ViT-B-16-gene", None, lock_text=True)
    with pytest.raises(ValueError, match="text"):
        net.SpatialClipNet("ViT-L-14-genetr", None, lock_text=True, lock_text_unlocked_layers=1)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="lock_image_unlocked_groups"):
            net.SpatialClipNet("ViT-B-16-gene", None, lock_image=True, lock_image_unlocked_groups=bad)
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    with pytest.raises(ValueError, match="SC_GRAD_EXCHANGE"):
        net.SpatialClipNet("ViT-B-16-gene", None, lock_image=True)


def test_lock_methods_refuse_on_a_built_net_object(monkeypatch):
    """The methods' own refusals, on a net object that skipped construction (no device here)."""
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import net, towers  # noqa: F401
    monkeypatch.delenv("SC_GRAD_EXCHANGE", raising=False)

    def bare(cfg, precision="bf16"):
        n = net.SpatialClipNet.__new__(net.SpatialClipNet)
        torch.nn.Module.__init__(n)
        n.cfg, n.precision, n.model_name, n.store = cfg, precision, "tiny", _store(cfg)

        class _Tower:
            unlocked = "never set"

            def set_lock(self, unlocked):
                self.unlocked = unlocked
        n.vision, n.second = _Tower(), _Tower()
        return n

    gene = bare(_tiny_cfg(gene=True))
    with pytest.raises(ValueError, match="gene tower"):
        gene.lock_text_tower()
    text = bare(_tiny_cfg())
    with pytest.raises(AssertionError, match="LayerNorm"):
        text.lock_text_tower(1, freeze_layer_norm=False)
    with pytest.raises(ValueError, match="fp8"):
        bare(_tiny_cfg(), "fp8").lock_image_tower()
    monkeypatch.setenv("SC_GRAD_EXCHANGE", "sharded")
    with pytest.raises(ValueError, match="SC_GRAD_EXCHANGE"):
        text.lock_image_tower()
    monkeypatch.delenv("SC_GRAD_EXCHANGE")
    text.lock_image_tower(2, freeze_bn_stats=True)       # accepted and ignored
    text.lock_text_tower(1)
    man = _manifest()
    assert sorted(text.trainable_names()) == sorted(set(man["image"]["2"]) & set(man["text"]["1"]))
    assert (text.vision.unlocked, text.second.unlocked) == (2, 1)
    # once an optimiser was built for the net, both methods raise RuntimeError
    from spatial_clip_amd import optim
    optim.FusedAdamW(list(text.store.params.values()))
    for call in (text.lock_image_tower, text.lock_text_tower):
        with pytest.raises(RuntimeError, match="optimiser"):
            call(0)
    assert (text.vision.unlocked, text.second.unlocked) == (2, 1)


def test_sharded_exchange_refuses_a_locked_store():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm, optim
    cfg = _tiny_cfg()
    st = _store(cfg)
    _lock(st, cfg, image=0)
    opt = optim.FusedAdamW(list(st.params.values()))
    ex = comm.ShardedGradExchange.__new__(comm.ShardedGradExchange)
    with pytest.raises(ValueError, match="sharded"):
        opt.attach_exchange(ex)


def test_lit_experiment_composes(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import hydra_lite as H
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lit"])
    base = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    n = cfg["model"]["net"]
    assert n["model_name"] == "ViT-B-16-gene" and n["lock_image"] is True and int(n["lock_image_unlocked_groups"]) == 0
    assert cfg.data.batch_size == base.data.batch_size == 256
    assert "lock_image" not in base["model"]["net"] and "lock_text" not in n
    over = H.compose("train.yaml", ["experiment=vitb16_gene_b256_lit", "model.net.lock_image_unlocked_groups=2"])
    assert int(over["model"]["net"]["lock_image_unlocked_groups"]) == 2
    text = H.compose("train.yaml", ["experiment=vitb32_text_b32", "+model.net.lock_text=true",
                                    "+model.net.lock_text_unlocked_layers=3"])
    assert text["model"]["net"]["lock_text"] is True and int(text["model"]["net"]["lock_text_unlocked_layers"]) == 3


def test_optimiser_moments_cover_the_trainable_floats_and_checkpoints_keep_the_full_layout():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import optim
    cfg = _tiny_cfg()
    free, locked = _store(cfg), _store(cfg)
    _lock(locked, cfg, image=1, text=2)
    ranges = locked.trainable_ranges()
    assert len(ranges) == 2
    o_free = optim.FusedAdamW(list(free.params.values()))
    o_lock = optim.FusedAdamW(list(locked.params.values()))          # all parameters, as Lightning passes them
    assert o_free.exp_avg.numel() == free.total and o_free.ranges == [(0, free.total)]
    assert o_lock.exp_avg.numel() == o_lock.exp_avg_sq.numel() == locked.trainable_floats() < locked.total
    with pytest.raises(ValueError):
        optim.FusedAdamW(list(locked.params.values())[1:])
    g = torch.Generator().manual_seed(3)
    o_lock.exp_avg.copy_(torch.randn(o_lock.exp_avg.shape, generator=g))
    o_lock.exp_avg_sq.copy_(torch.rand(o_lock.exp_avg_sq.shape, generator=g))
    o_lock.step_count = 7
    sd = o_lock.state_dict()
    # locked -> file: the full flat layout, zeros in the locked ranges
    assert sd["exp_avg"].numel() == sd["exp_avg_sq"].numel() == locked.total and sd["step"] == 7
    mask = torch.zeros(locked.total, dtype=torch.bool)
    pos = 0
    for lo, hi in ranges:
        mask[lo:hi] = True
        assert torch.equal(sd["exp_avg"][lo:hi], o_lock.exp_avg[pos:pos + hi - lo])
        assert torch.equal(sd["exp_avg_sq"][lo:hi], o_lock.exp_avg_sq[pos:pos + hi - lo])
        pos += hi - lo
    assert pos == o_lock.exp_avg.numel()
    assert float(sd["exp_avg"][~mask].abs().max()) == 0.0 and float(sd["exp_avg_sq"][~mask].abs().max()) == 0.0
    # file -> unlocked optimiser: loads as it is
    o_free.load_state_dict(sd)
    assert o_free.step_count == 7 and torch.equal(o_free.exp_avg, sd["exp_avg"]) and torch.equal(o_free.exp_avg_sq, sd["exp_avg_sq"])
    # unlocked -> file -> locked optimiser: takes the trainable slices; and round-trips to the same file
    o_free.exp_avg.copy_(torch.randn(o_free.exp_avg.shape, generator=g))
    o_free.exp_avg_sq.copy_(torch.rand(o_free.exp_avg_sq.shape, generator=g))
    full = o_free.state_dict()
    other = _store(cfg)
    _lock(other, cfg, image=1, text=2)
    o2 = optim.FusedAdamW(list(other.params.values()))
    o2.load_state_dict(full)
    back = o2.state_dict()
    assert torch.equal(back["exp_avg"][mask], full["exp_avg"][mask]) and torch.equal(back["exp_avg_sq"][mask], full["exp_avg_sq"][mask])
    assert float(back["exp_avg"][~mask].abs().max()) == 0.0
    o3 = optim.FusedAdamW(list(_locked_again(cfg).params.values()))
    o3.load_state_dict(back)
    assert torch.equal(o3.exp_avg, o2.exp_avg) and torch.equal(o3.exp_avg_sq, o2.exp_avg_sq)


def _locked_again(cfg):
    st = _store(cfg)
    _lock(st, cfg, image=1, text=2)
    return st


def test_accumulator_folds_only_the_trainable_ranges():
    """Host expressions of ops.grad_accumulate: the locked part of the gradient buffer and of the running sum is never touched."""
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import optim
    cfg = _tiny_cfg()
    st = _store(cfg)
    _lock(st, cfg, image=0, text=1)
    ranges = st.trainable_ranges()
    mask = torch.zeros(st.total, dtype=torch.bool)
    for lo, hi in ranges:
        mask[lo:hi] = True
    acc = optim.GradAccumulator(st, 2)
    assert acc.sumsq_partial().numel() == 1024 * len(ranges)
    st.grad.fill_(2.0)                       # (a backward never writes the locked part; the sentinel shows nothing reads it)
    acc.fold(True, False)
    assert torch.equal(acc.acc[mask], torch.full((int(mask.sum()),), 1.0)) and float(acc.acc[~mask].abs().max()) == 0.0
    st.grad.fill_(4.0)
    hook = acc.hook(False, True)
    hook(*ranges[-1])
    acc.fold_rest(False, True)
    assert torch.equal(st.grad[mask], torch.full((int(mask.sum()),), 3.0))
    assert torch.equal(st.grad[~mask], torch.full((int((~mask).sum()),), 4.0))


def _reducer_worker(rank, world, port, ret):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import comm
    ranges = [(128, 320), (512, 640), (896, 1024)]
    out = {}
    # (a) backward announces part of what is trainable (and, wrongly, a range that straddles a locked one): finish() reduces
    # the complement WITHIN the trainable ranges
    flat = torch.arange(1024, dtype=torch.float32) * (rank + 1)
    comm.reset_stats()
    red = comm.GradBucketReducer(flat, bucket_floats=256, ranges=ranges)
    for lo, hi in ((960, 1024), (600, 900), (192, 256)):
        red.bucket_ready(lo, hi)
    red.finish()
    out["a"] = flat.numpy()
    out["a_bytes"] = sum(v[1] for k, v in comm.STATS.items() if k.startswith("all_reduce(gradient"))
    # (b) nothing announced at all
    flat = torch.arange(1024, dtype=torch.float32) * (rank + 1)
    comm.reset_stats()
    red = comm.GradBucketReducer(flat, bucket_floats=256, ranges=ranges)
    red.finish()
    out["b"] = flat.numpy()
    out["b_bytes"] = sum(v[1] for k, v in comm.STATS.items() if k.startswith("all_reduce(gradient"))
    # (c) one whole-buffer range is the reducer of a net without locks
    assert comm.GradBucketReducer(flat, 256, ranges=[(0, 1024)]).ranges is None
    ret[rank] = out
    dist.destroy_process_group()


def test_reducer_never_reduces_a_locked_float():
    import numpy as np
    world = 2
    mp.set_start_method("spawn", force=True)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_reducer_worker, args=(world, 29641, ret), nprocs=world, join=True)
        res = dict(ret)
    base = np.arange(1024, dtype=np.float32)
    mask = np.zeros(1024, dtype=bool)
    for lo, hi in ((128, 320), (512, 640), (896, 1024)):
        mask[lo:hi] = True
    for r in range(world):
        want = np.where(mask, base * 3, base * (r + 1))      # trainable: the sum over both ranks; locked: this rank's own values
        for case in ("a", "b"):
            np.testing.assert_array_equal(res[r][case], want)
            assert res[r][case + "_bytes"] == 4 * int(mask.sum())
