"""SC_WGRAD_GROUP: every weight-gradient launch mode of the transformer stack (auto, 0 = one launch per Linear, 1 = attention
branch grouped, 2 / 3 = both branches grouped, 4 = all four of a block in one launch) on one small model: vision (image 48,
patch 16, width 128, 3 layers, head 64) + gene MLP at B = 64 -- 640 token rows = 10 K tiles, so the grouped launches run at
split-K 2.  The modes differ only in how the four weight matrices of a full-width block (and the two biases fused into their
launches) are summed; every other gradient must not move by a bit.  Measured (profiles/stack_refactor_trace.txt): in every
mode the worst written gradient sits at 2.5 % of its max-abs against the fp32 oracle (out_proj.weight of block 1), bound 3 %."""
import pytest
import torch

from oracle import spatial_clip_oracle as O
from tests.test_gpu_model import _pkg, perturb, tiny_cfgs

pytestmark = pytest.mark.gpu

MODES = ("auto", "0", "1", "2", "3", "4")
B, IMAGE, LAYERS = 64, 48, 3
WRITTEN_LEAVES = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_fc.bias",
                  "mlp.c_proj.weight")


def _written():
    """Gradients a weight-gradient launch of a full-width block writes (the class-token last block has launches of its own)."""
    return {f"visual.transformer.resblocks.{i}.{leaf}" for i in range(LAYERS - 1) for leaf in WRITTEN_LEAVES}


def _grads(mode, monkeypatch):
    """Gradients of two forward / backward runs of one net with SC_WGRAD_GROUP = ``mode`` (side stream on)."""
    data, losses, mc, module, net, optim = _pkg()
    monkeypatch.setenv("SC_OVERLAP", "1")
    monkeypatch.setenv("SC_WGRAD_GROUP", mode)
    cfg, _ = tiny_cfgs(128, 64, LAYERS, IMAGE, 16)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
    perturb(n)
    m = module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True), None, None)
    batch = {k: v.cuda() for k, v in data.synthetic_batch(B, IMAGE, cfg.gene.n_genes, K=4, step=0).items()}
    runs = []
    for _ in range(2):
        m.model_step(batch)["loss"].backward()
        torch.cuda.synchronize()
        runs.append({k: n.store.g(k).detach().cpu().clone() for k in n.state_dict()})
    return runs


@pytest.fixture(scope="module")
def oracle_grads():
    """fp32 CPU oracle on the same parameters and batch, computed once for all modes."""
    data, losses, mc, module, net, optim = _pkg()
    cfg, ocfg = tiny_cfgs(128, 64, LAYERS, IMAGE, 16)
    n = net.SpatialClipNet("custom", None, model_cfg=cfg, seed=3)
    perturb(n)
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in n.state_dict().items()}
    batch = data.synthetic_batch(B, IMAGE, cfg.gene.n_genes, K=4, step=0)
    f = O.net_forward(batch["images"], batch["texts"], p, ocfg)
    O.clip_loss(f["image_features"], f["text_features"], f["logit_scale"]).backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}


@pytest.fixture(scope="module")
def mode0_grads():
    mp = pytest.MonkeyPatch()
    try:
        return _grads("0", mp)[0]
    finally:
        mp.undo()


@pytest.mark.parametrize("mode", MODES)
def test_wgrad_group_mode(mode, monkeypatch, oracle_grads, mode0_grads):
    a, b = _grads(mode, monkeypatch)
    for k in a:                                     # within a mode: run to run, bit for bit
        assert torch.equal(a[k], b[k]), (mode, k)
    written = _written()
    assert written <= set(a)
    for k in a:                                     # across modes: what no weight-gradient launch writes does not move
        if k not in written:
            assert torch.equal(a[k], mode0_grads[k]), (mode, k)
    worst = (0.0, None)
    for k in sorted(written):                       # the written ones: 3 % of the tensor's max-abs against the fp32 oracle
        ref = oracle_grads[k]
        rel = float((a[k] - ref).abs().max() / ref.abs().max())
        worst = max(worst, (rel, k))
    print(f"SC_WGRAD_GROUP={mode}: worst written gradient {worst[0]:.4f} of max-abs ({worst[1]})")
    assert worst[0] <= 0.03, (mode, worst)
