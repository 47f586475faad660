"""The training step as one hipGraph (spatial_clip_amd/graph.py): replaying the captured step must give the eager step's
bits -- same kernels, same values, same order -- while the learning-rate schedule and Adam's bias correction advance through
the device-side triple, and everything the capture cannot take (other batch shapes, multi-rank, e4m3) stays eager."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pkg():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, graph, losses, model_configs as mc, module, net, optim
    return data, graph, losses, mc, module, net, optim


def _build(cfg, loss_kind, seed=3):
    data, graph, losses, mc, module, net, optim = _pkg()
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=seed)
    if loss_kind == "clip":
        loss_fn = losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True)
    else:
        loss_fn = losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                     neighbor_alpha_scale=0.5, float32_logits=True)
    m = module.SpatialClipLitModule(
        n, loss_fn, functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=3))

    class T:
        max_steps, max_epochs, estimated_stepping_batches = 40, None, 40
    m.trainer = T()
    oc = m.configure_optimizers()
    return n, m, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _batches(cfg, B, n, text):
    data, *_ = _pkg()
    out = []
    for s in range(n):
        b = data.synthetic_batch(B, cfg.vision.image_size, 200, K=4, step=s)
        if text:
            b["texts"] = data.synthetic_captions(B, cfg.text.context_length, cfg.text.vocab_size, seed=s)
        out.append({k: v.cuda() for k, v in b.items()})
    return out


@pytest.mark.parametrize("second,loss_kind,overlap", [("gene", "spatial", "1"), ("text", "clip", "1"), ("gene", "clip", "0")])
def test_graph_replay_is_bit_identical_to_the_eager_step(second, loss_kind, overlap, monkeypatch):
    data, graph, losses, mc, module, net, optim = _pkg()
    monkeypatch.setenv("SC_OVERLAP", overlap)           # pinned schedule: nothing left to decide before the capture
    text = second == "text"
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32),
                      text=mc.TextCfg(16, 97, 64, 2, 2) if text else None, gene=None if text else mc.GeneCfg(200, 64))
    B, steps = 24, 6
    batches = _batches(cfg, B, steps, text)
    ragged = {k: v[:10].contiguous() for k, v in batches[2].items()}        # another shape in the middle: must run eagerly
    res = {}
    for mode in ("eager", "graph"):
        n, m, opt, sched = _build(cfg, loss_kind)
        step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
        ls = []
        for i in range(steps):
            b = batches[i]
            loss = step.eager(b) if mode == "eager" else step(b)
            sched.step()
            ls.append(float(loss.detach()))
            if i == 2:
                loss = step.eager(ragged) if mode == "eager" else step(ragged)
                sched.step()
                ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        res[mode] = dict(loss=ls, w=n.store.master.detach().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                         metrics=m.train_metrics.compute(), steps=opt.step_count, lr=opt.param_groups[0]["lr"],
                         replays=step.replays, failed=step.failed)
    assert res["graph"]["failed"] is None, res["graph"]["failed"]
    assert res["graph"]["replays"] == steps - 1          # first call eager (warms the shape), second captures AND replays; the ragged batch ran eagerly
    assert res["eager"]["replays"] == 0
    assert res["eager"]["steps"] == res["graph"]["steps"] == steps + 1
    assert res["eager"]["lr"] == res["graph"]["lr"]
    # (bitwise for the text tower too since round 6: its embedding scatter-add no longer uses float atomics)
    assert res["eager"]["loss"] == res["graph"]["loss"], (res["eager"]["loss"], res["graph"]["loss"])
    for k in ("w", "m", "v"):
        assert torch.equal(res["eager"][k], res["graph"][k]), f"{k}: graph replay differs from the eager step"
    assert res["eager"]["metrics"] == res["graph"]["metrics"]
    assert res["eager"]["loss"][-1] < res["eager"]["loss"][0]       # and it trains


def test_graph_refuses_what_it_cannot_capture(monkeypatch):
    data, graph, losses, mc, module, net, optim = _pkg()
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    monkeypatch.delenv("SC_OVERLAP", raising=False)     # auto: the schedule trials use timing events -> not before they are done
    n, m, opt, sched = _build(cfg, "clip")
    step = graph.GraphedTrainStep(m, opt, max_norm=1.0)
    assert "not decided" in step.capturable()
    b = _batches(cfg, 16, 1, False)[0]
    from spatial_clip_amd import towers
    need = sum(towers.TransformerStack.OVERLAP_TRIAL_CALLS[1:]) * 2 + towers.TransformerStack.OVERLAP_TRIAL_CALLS[0] + 1
    for i in range(need):
        assert step.graph is None
        step(b)
        sched.step()
    assert step.capturable() is None
    step(b)
    assert step.graph is not None and step.failed is None and step.replays == 1     # (the shape had run eagerly before)


@pytest.mark.parametrize("second", ["text", "genetr"])
def test_towers_side_by_side_give_the_bits_of_the_sequential_order(second, monkeypatch):
    """net.py (round 6): the second tower on its own stream beside the vision tower -- same kernels on the same values, so
    losses, gradients and the weights after optimiser steps are bit-identical to the sequential order (SC_TOWER_OVERLAP=0),
    with the optimiser's update still running behind the forward on a third stream."""
    data, graph, losses, mc, module, net, optim = _pkg()
    text = second == "text"
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32),
                      text=mc.TextCfg(16, 97, 64, 2, 2) if text else None,
                      gene=None if text else mc.GeneCfg(512, 64, kind="transformer", patch=64, width=64, layers=2, head_width=32))
    B, steps = 24, 4
    batches = []
    for s in range(steps):
        b = data.synthetic_batch(B, 32, 512, K=4, step=s)
        if text:
            b["texts"] = data.synthetic_captions(B, 16, 97, seed=s)
        batches.append({k: v.cuda() for k, v in b.items()})
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SC_TOWER_OVERLAP", mode)
        n, m, opt, sched = _build(cfg, "spatial")
        ls = []
        for i in range(steps):
            loss = m.training_step(batches[i], i)
            loss.backward(m.root_gradient(loss))
            if i == 0:
                g0 = n.store.grad.clone()
            opt.step(grad_scale=1.0, max_norm=1.0)
            sched.step()
            ls.append(float(loss.detach()))
        n.store.wait_all()
        torch.cuda.synchronize()
        assert n.second.stack.no_side_stream == (mode == "1")
        res[mode] = (ls, g0, n.store.master.detach().clone(), opt.exp_avg.clone())
    assert res["0"][0] == res["1"][0]
    for k in (1, 2, 3):
        assert torch.equal(res["0"][k], res["1"][k])


def test_trainer_fit_with_the_graphed_step_equals_the_enqueued_fit(monkeypatch, tmp_path):
    """Trainer.fit on the reference's pairing in miniature (vision tower + CLIP text tower, towers side by side), two epochs with
    validation, a mid-run checkpoint and a ragged last batch: SC_GRAPH=1 (capture as soon as possible) and SC_GRAPH=0 end with
    the same weights, Adam moments and validation record, bit for bit -- and the graph really ran."""
    data, graph, losses, mc, module, net, optim = _pkg()
    from spatial_clip_amd.trainer import Trainer
    monkeypatch.setenv("SC_OVERLAP", "1")
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=mc.TextCfg(16, 97, 64, 2, 2), gene=None)

    class TextDM(data.SyntheticSpatialDataModule):
        def _loader(self, n, offset):
            for s in range(n):
                B = self.batch_size if s + 1 < n else self.batch_size - 5           # ragged last batch of the epoch
                b = data.synthetic_batch(B, self.image_size, 64, self.k_neighbors, offset + s)
                b["texts"] = data.synthetic_captions(B, 16, 97, seed=offset + s)
                yield b

    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SC_GRAPH", mode)
        n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=5)
        m = module.SpatialClipLitModule(
            n, losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                  neighbor_alpha_scale=0.5, float32_logits=True),
            functools.partial(optim.FusedAdamW, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1),
            functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=2))
        dm = TextDM(batch_size=16, image_size=32, n_genes=64, k_neighbors=4, steps_per_epoch=6, val_steps=2)
        tr = Trainer(max_epochs=2, enable_checkpointing=True, default_root_dir=str(tmp_path / mode), log_every_n_steps=1)
        tr.fit(m, dm)
        torch.cuda.synchronize()
        gs = tr.graphed_step
        res[mode] = dict(w=n.store.master.detach().clone(), m=tr.optimizer.exp_avg.clone(), hist=[
            {k: v for k, v in h.items() if k != "time_s"} for h in tr.history], replays=0 if gs is None else gs.replays,
            failed=None if gs is None else gs.failed, side=n.second.stack.no_side_stream)
    assert res["0"]["replays"] == 0 and res["1"]["failed"] is None
    assert res["1"]["replays"] == 2 * 5 - 1          # every full-size batch but the first (it warms the shape); the ragged ones run eagerly
    assert res["0"]["side"] and res["1"]["side"]     # towers side by side in both runs
    assert res["0"]["hist"] == res["1"]["hist"], (res["0"]["hist"], res["1"]["hist"])
    assert torch.equal(res["0"]["w"], res["1"]["w"]) and torch.equal(res["0"]["m"], res["1"]["m"])


def test_train_entry_reference_pairing_vitb32_text_tower(monkeypatch, tmp_path):
    """`python -m spatial_clip_amd.train experiment=vitb32_text_b32` -- the reference's own model (configs/model/spatial_clip.yaml:10:
    ViT-B-32 + CLIP text tower) at the batch size of its medium experiments, through the Hydra surface: the synthetic datamodule
    hands token ids to the text tower, the step runs with the towers side by side and (SC_GRAPH=1) as one hipGraph."""
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    monkeypatch.setenv("SC_GRAPH", "1")      # capture as soon as the schedule is decided (auto decides by a timing: not for a test)
    monkeypatch.delenv("SC_OVERLAP", raising=False)
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import hydra_lite, train
    cfg = hydra_lite.compose("train.yaml", ["experiment=vitb32_text_b32", "data.steps_per_epoch=40", "data.val_steps=1", "trainer.log_every_n_steps=10"])
    metrics, objects = train.train(cfg)
    net_ = objects["model"].net
    assert net_.cfg.text is not None and net_.cfg.text.vocab_size == 49408 and net_.cfg.vision.patch_size == 32
    gs = objects["trainer"].graphed_step
    assert gs is not None and gs.replays > 0, (gs.failed if gs is not None else None)
    assert net_.second.stack.no_side_stream                              # towers side by side
    assert metrics["train/loss"] == metrics["train/loss"] and "val/loss" in metrics
    assert 0.0 <= metrics["val/R@10"] <= 1.0
