"""Full-set retrieval ranks on the device (``sc_retrieval_ranks`` / ``ops.retrieval_ranks`` / ``metrics.RetrievalMetrics``)
against the float64 oracle of tests/_retrieval_oracle.py, and the wiring through the module and the trainer.

The kernel works on 128 x 128 tiles over 32-deep K slices: N = 129, 130, 257, 1000, 2049 and D = 3, 5, 33, 96 put a pair on
every M / N / K edge, N = 257 gives more than one row panel and column tile, D = 512 many K slices."""
import functools

import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as RO

pytestmark = pytest.mark.gpu


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _run(fi, ft, **kw):
    r_i, r_t = _ops().retrieval_ranks(fi.cuda(), ft.cuda(), **kw)
    return r_i.cpu().numpy().astype(np.int64), r_t.cpu().numpy().astype(np.int64)


def _plant(fi, ft):
    """Duplicates across the 128-row tile boundary and rows of zeros, wherever N has room for them."""
    N = fi.shape[0]
    fi, ft = fi.clone(), ft.clone()
    if N > 200:
        ft[200] = ft[3]                 # text row 200 == text row 3: row 3 and row 200 each see an exact tie with their diagonal
        ft[5] = ft[250]                 # ... and the other way round
        fi[140] = fi[7]                 # the same for image rows (ties in the columns)
        fi[9] = fi[230]
        fi[50] = 0
        ft[60] = 0
        fi[70] = 0
        ft[70] = 0
    elif N > 16:
        ft[16] = ft[2]
        fi[1] = fi[15]
        fi[4] = 0
        ft[6] = 0
        fi[8] = 0
        ft[8] = 0
    return fi, ft


@functools.lru_cache(maxsize=None)
def _exact(N, D):
    fi, ft = _plant(*RO.exact_case(N, D))
    return fi, ft, RO.ranks(fi.numpy(), ft.numpy())


@pytest.mark.parametrize("N,D", [(1, 1), (1, 16), (17, 5), (129, 3), (257, 16)])
def test_exact_inputs_match_the_oracle_ties_included(N, D):
    fi, ft, (want_i, want_t) = _exact(N, D)
    got_i, got_t = _run(fi, ft)
    if N > 16:      # the case does hold ties with a diagonal, in both directions
        z = RO.similarities(fi.numpy(), ft.numpy())
        off = ~np.eye(N, dtype=bool)
        assert ((z == np.diagonal(z)[:, None]) & off).any() and ((z == np.diagonal(z)[None, :]) & off).any()
    assert np.array_equal(got_i, want_i), np.flatnonzero(got_i != want_i)[:8]
    assert np.array_equal(got_t, want_t), np.flatnonzero(got_t != want_t)[:8]
    if N == 1:
        assert got_i.tolist() == [0] and got_t.tolist() == [0]


def test_duplicate_text_rows_tie_exactly():
    """Random (non-exact) unit features, text row 200 a bitwise copy of row 3: z[3, 200] and d_3 = z[3, 3] are the same
    function of the same bits, so must tie -- column 200 is NOT counted for row 3 (tie, larger index) and column 3 IS counted
    for row 200 (tie, smaller index).  A diagonal formed with another summation order breaks one of the two."""
    N, D = 257, 33
    fi, ft = RO.random_unit_case(N, D)
    ft = ft.clone()
    ft[200] = ft[3]
    got_i, _ = _run(fi, ft)
    far = ft.clone()
    far[200] = -fi[3]                   # z[3, 200] = -1: certainly not counted for row 3
    ref3, _ = _run(fi, far)
    assert got_i[3] == ref3[3]
    far = ft.clone()
    far[3] = -fi[200]                   # z[200, 3] = -1: certainly not counted for row 200 (d_200 is unchanged)
    ref200, _ = _run(fi, far)
    assert got_i[200] == ref200[200] + 1
    # the same through a strided, unaligned view (the guarded staging path)
    wide_i, wide_t = torch.zeros(N, 41).cuda(), torch.zeros(N, 47).cuda()
    wide_i[:, 3:3 + D] = fi.cuda()
    wide_t[:, 5:5 + D] = ft.cuda()
    r_i, _ = _ops().retrieval_ranks(wide_i[:, 3:3 + D], wide_t[:, 5:5 + D])
    assert np.array_equal(r_i.cpu().numpy(), got_i)


@functools.lru_cache(maxsize=None)
def _random(N, D):
    fi, ft = RO.random_unit_case(N, D)
    z = RO.similarities(fi.numpy(), ft.numpy())
    return fi, ft, RO.ranks_from_z(z), RO.allowances(z, RO.fp32_margin(D))


@pytest.mark.parametrize("N,D", RO.RANDOM_CASES)
def test_random_unit_features_against_float64(N, D):
    fi, ft, (want_i, want_t), (a_i, a_t) = _random(N, D)
    got_i, got_t = _run(fi, ft)
    print(f"N={N} D={D}: rows with an allowance {np.mean(a_i > 0):.3%} (max {a_i.max()}), columns {np.mean(a_t > 0):.3%} "
          f"(max {a_t.max()}); rows that differ {int((got_i != want_i).sum())}, columns {int((got_t != want_t).sum())}")
    assert np.mean(a_i > 0) <= 0.15 and np.mean(a_t > 0) <= 0.15
    bad_i, bad_t = np.abs(got_i - want_i) > a_i, np.abs(got_t - want_t) > a_t
    assert not bad_i.any(), (np.flatnonzero(bad_i)[:8], got_i[bad_i][:8], want_i[bad_i][:8])
    assert not bad_t.any(), (np.flatnonzero(bad_t)[:8], got_t[bad_t][:8], want_t[bad_t][:8])


def test_strides_blocks_and_reproducibility():
    ops = _ops()
    N, D = 257, 33
    fi, ft = RO.random_unit_case(N, D)
    fi_d, ft_d = fi.cuda(), ft.cuda()
    r_i, r_t = ops.retrieval_ranks(fi_d, ft_d)
    again_i, again_t = ops.retrieval_ranks(fi_d, ft_d)
    assert torch.equal(r_i, again_i) and torch.equal(r_t, again_t)
    assert r_i.dtype == torch.int32 and r_i.shape == (N,) and r_t.shape == (N,)
    # ld > D: an aligned view (16-byte loads, K edge in the second slice) and an unaligned one (guarded staging)
    for ld_i, o_i, ld_t, o_t in ((48, 8, 40, 4), (41, 3, 35, 1)):
        wi, wt = torch.full((N, ld_i), 7.0).cuda(), torch.full((N, ld_t), -7.0).cuda()
        wi[:, o_i:o_i + D] = fi_d
        wt[:, o_t:o_t + D] = ft_d
        s_i, s_t = ops.retrieval_ranks(wi[:, o_i:o_i + D], wt[:, o_t:o_t + D])
        assert torch.equal(s_i, r_i) and torch.equal(s_t, r_t), (ld_i, ld_t)
    # three row blocks into one cnt_t2i == the single launch, bit for bit; the counts are ADDED onto what is there
    cnt = torch.zeros(N, dtype=torch.int32).cuda()
    parts = []
    for row0, M in ((0, 100), (100, 100), (200, 57)):
        rank = torch.full((M,), -1, dtype=torch.int32).cuda()
        out_rank, out_cnt = ops.retrieval_ranks(fi_d, ft_d, row0=row0, M=M, rank_i2t=rank, cnt_t2i=cnt)
        assert out_rank is rank and out_cnt is cnt
        parts.append(rank)
    assert torch.equal(torch.cat(parts), r_i) and torch.equal(cnt, r_t)
    ops.retrieval_ranks(fi_d, ft_d, row0=200, cnt_t2i=cnt)           # M defaults to the rest
    _, tail = ops.retrieval_ranks(fi_d, ft_d, row0=200, M=57)
    assert torch.equal(cnt, r_t + tail)
    # RetrievalMetrics: ragged updates, buffer growth, reset
    from spatial_clip_amd import metrics
    m = metrics.RetrievalMetrics("val/", ks=(1, 5, 300))
    for a, b in ((0, 100), (100, 101), (101, 257)):
        m.update(fi_d[a:b], ft_d[a:b])
    got = m.compute()
    assert got == RO.summary(r_i.cpu().numpy(), r_t.cpu().numpy(), ks=(1, 5, 300), prefix="val/")
    assert got["val/image_to_text_R@300"] == 1.0 and got["val/retrieval_num_samples"] == 257.0
    m.reset()
    m.update(fi_d[:17], ft_d[:17])
    small = m.compute()
    w_i, w_t = ops.retrieval_ranks(fi_d[:17], ft_d[:17])
    assert small == RO.summary(w_i.cpu().numpy(), w_t.cpu().numpy(), ks=(1, 5, 300), prefix="val/")


def test_bad_arguments():
    ops = _ops()
    from spatial_clip_amd._lib import SpatialClipHipError
    fi, ft = (t.cuda() for t in RO.random_unit_case(17, 5))
    with pytest.raises(SpatialClipHipError, match=r"sc_retrieval_ranks: row block \[10, 10 \+ 8\) outside \[0, 17\)"):
        ops.retrieval_ranks(fi, ft, row0=10, M=8)
    with pytest.raises(ValueError, match="row0"):
        ops.retrieval_ranks(fi, ft, row0=-1, M=2)
    with pytest.raises(ValueError, match="one shape"):
        ops.retrieval_ranks(fi, ft[:16])
    with pytest.raises(TypeError, match="image_feat"):
        ops.retrieval_ranks(fi.double(), ft)
    with pytest.raises(SpatialClipHipError, match="device tensor"):
        ops.retrieval_ranks(fi.cpu(), ft)
    with pytest.raises(ValueError, match="contiguous"):
        ops.retrieval_ranks(fi.t().contiguous().t(), ft)
    with pytest.raises(ValueError, match="cnt_t2i"):
        ops.retrieval_ranks(fi, ft, cnt_t2i=torch.zeros(16, dtype=torch.int32).cuda())
    with pytest.raises(TypeError, match="rank_i2t"):
        ops.retrieval_ranks(fi, ft, rank_i2t=torch.zeros(17).cuda())
    r_i, r_t = ops.retrieval_ranks(fi, ft, row0=17, M=0)             # an empty block launches nothing
    assert r_i.numel() == 0 and int(r_t.abs().sum()) == 0


def test_non_finite_diagonal_ranks_last():
    N, D = 257, 16
    fi, ft = (t.clone() for t in RO.exact_case(N, D, seed=1))
    fi[77] = float("nan")
    ft[140, 3] = float("inf")           # z[i, 140] = +-inf or nan: d_140 is not finite either
    want_i, want_t = RO.ranks(fi.numpy(), ft.numpy())
    assert want_i[77] == N - 1 and want_t[77] == N - 1 and want_i[140] == N - 1 and want_t[140] == N - 1
    got_i, got_t = _run(fi, ft)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_t, want_t)
    # ... and it composes over row blocks
    cnt = torch.zeros(N, dtype=torch.int32).cuda()
    for row0, M in ((0, 77), (77, 1), (78, 179)):
        _ops().retrieval_ranks(fi.cuda(), ft.cuda(), row0=row0, M=M, cnt_t2i=cnt)
    assert np.array_equal(cnt.cpu().numpy(), want_t)


# ----------------------------------------------------------------------------------------------------------- wiring
class _Batches:
    """Validation / test data of three batches, the last one ragged."""

    def __init__(self, sizes=(12, 12, 7)):
        from spatial_clip_amd import data
        self.batches = [data.synthetic_batch(B, 32, 200, K=4, step=50 + i) for i, B in enumerate(sizes)]
        self.preprocess_fn = self.tokenizer = object()

    def val_dataloader(self):
        return self.batches

    test_dataloader = val_dataloader


def _module(n, full_retrieval):
    from spatial_clip_amd import losses, module
    return module.SpatialClipLitModule(n, losses.ClipLoss(local_loss=True, gather_with_grad=True), None, None,
                                       full_retrieval=full_retrieval)


def _tiny_net():
    from spatial_clip_amd import model_configs as mc, net
    cfg = mc.ModelCfg(embed_dim=64, vision=mc.VisionCfg(32, 8, 64, 2, 32), text=None, gene=mc.GeneCfg(200, 64))
    return net.SpatialClipNet("custom", None, model_cfg=cfg, seed=5)


def test_module_and_trainer_wiring():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import metrics, ops
    from spatial_clip_amd.trainer import Trainer
    n = _tiny_net()
    dm = _Batches()
    m_off, m_on = _module(n, None), _module(n, {"ks": [1, 5, 10]})
    assert m_off.val_retrieval is None and m_off.test_retrieval is None
    assert isinstance(m_on.val_retrieval, metrics.RetrievalMetrics) and m_on.test_retrieval.prefix == "test/"
    tr_off, tr_on = Trainer(callbacks={}), Trainer(callbacks={})
    m_off.trainer, m_on.trainer = tr_off, tr_on
    off = tr_off._validate_pass(m_off, dm)
    assert sorted(off) == ["val/R@1", "val/R@10", "val/R@5", "val/loss"]

    feats = []
    step = m_on.model_step

    def recording_step(batch, metrics=None):
        out = step(batch, metrics)
        feats.append((out["image_features"].detach().float().clone(), out["text_features"].detach().float().clone()))
        return out

    m_on.model_step = recording_step
    names = [f"{d}_{q}" for d in ("image_to_text", "text_to_image") for q in ("mean_rank", "median_rank", "R@1", "R@5", "R@10")]
    for prefix, run in (("val/", lambda: tr_on._validate_pass(m_on, dm)), ("test/", lambda: tr_on.test(m_on, dm)[0]),
                        ("val/", lambda: tr_on._validate_pass(m_on, dm))):      # the second pass starts from a reset
        feats.clear()
        on = run()
        assert sorted(on) == sorted([prefix + k for k in ["R@1", "R@5", "R@10", "loss", "retrieval_num_samples"] + names])
        fi, ft = torch.cat([f[0] for f in feats]), torch.cat([f[1] for f in feats])
        assert fi.shape == (31, 64) and on[prefix + "retrieval_num_samples"] == 31.0
        # what the pass reports is the summary of the kernel's ranks of exactly the features the steps produced ...
        r_i, r_t = (r.cpu().numpy() for r in ops.retrieval_ranks(fi, ft))
        direct = RO.summary(r_i, r_t, prefix=prefix)
        assert {k: on[k] for k in direct} == direct
        # ... and those ranks are the float64 oracle's, up to the pairs fp32 cannot order
        z = RO.similarities(fi.cpu().numpy(), ft.cpu().numpy())
        want_i, want_t = RO.ranks_from_z(z)
        a_i, a_t = RO.allowances(z, RO.fp32_margin(64))
        assert (np.abs(r_i - want_i) <= a_i).all() and (np.abs(r_t - want_t) <= a_t).all()
        if not a_i.any() and not a_t.any():
            assert {k: on[k] for k in direct} == RO.summary(want_i, want_t, prefix=prefix)
        if prefix == "val/":        # the in-batch metric is untouched by the feature, bit for bit
            assert all(on[k] == off[k] for k in ("val/R@1", "val/R@5", "val/R@10"))
            assert on["val/loss"] == pytest.approx(off["val/loss"], rel=1e-6)
        else:
            assert all(tr_on.callback_metrics[k] == v for k, v in on.items())


def test_fit_monitors_a_full_retrieval_metric(tmp_path):
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import data, losses, module, optim
    from spatial_clip_amd.trainer import Trainer
    m = module.SpatialClipLitModule(
        _tiny_net(), losses.ClipLoss(local_loss=True, gather_with_grad=True),
        functools.partial(optim.FusedAdamW, lr=1e-3, weight_decay=0.1),
        functools.partial(optim.get_cosine_schedule_with_warmup, num_warmup_steps=100), full_retrieval=True)
    dm = data.SyntheticSpatialDataModule(batch_size=12, image_size=32, n_genes=200, k_neighbors=4, steps_per_epoch=2, val_steps=2)
    tr = Trainer(max_epochs=1, enable_checkpointing=True, default_root_dir=str(tmp_path), log_every_n_steps=1,
                 callbacks={"model_checkpoint": {"dirpath": str(tmp_path / "ck"), "monitor": "val/image_to_text_R@5",
                                                 "mode": "max"}})
    tr.fit(m, dm)
    rec = tr.history[-1]
    assert rec["val/retrieval_num_samples"] == 24.0 and 0.0 <= rec["val/image_to_text_R@5"] <= 1.0
    assert tr.callback_metrics["val/image_to_text_R@5"] == rec["val/image_to_text_R@5"]
    assert tr.callback_metrics["val/text_to_image_median_rank"] == rec["val/text_to_image_median_rank"]
    assert tr.checkpoint_callback.monitor == "val/image_to_text_R@5"
    assert tr.checkpoint_callback.best_model_score == rec["val/image_to_text_R@5"] and tr.checkpoint_callback.best_model_path
