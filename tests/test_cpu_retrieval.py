"""Full-set retrieval metrics, host side: the float64 oracle against the reference's ``get_clip_metrics`` (fixture
tests/golden/retrieval_ref.npz, written by tests/golden/make_golden_retrieval.py from the reference itself), the numpy
summary, the module's ``full_retrieval`` argument, the header and the config."""
import inspect
import os

import numpy as np
import pytest

from tests import _retrieval_oracle as RO


@pytest.fixture(scope="module")
def fixture(golden_dir):
    f = np.load(os.path.join(golden_dir, "retrieval_ref.npz"))
    return {"fi": f["image_features"], "ft": f["text_features"], "scale": float(f["logit_scale"]),
            "ref": {str(k): float(v) for k, v in zip(f["names"], f["values"])}}


def test_fixture_shape(fixture):
    assert fixture["fi"].shape == fixture["ft"].shape == (300, 16) and fixture["fi"].dtype == np.float32
    assert len(fixture["ref"]) == 10 and fixture["scale"] > 0
    # ranks spread over the range: the fixture is not a trivial all-hits case
    assert 0.0 < fixture["ref"]["image_to_text_R@1"] < 0.5 and fixture["ref"]["image_to_text_mean_rank"] > 10


def test_oracle_reproduces_the_reference(fixture):
    r_i, r_t = RO.ranks(fixture["fi"], fixture["ft"])
    got = RO.summary(r_i, r_t)
    for k, v in fixture["ref"].items():
        assert got[k] == v, (k, got[k], v)
    assert got["retrieval_num_samples"] == 300.0


def test_retrieval_summary_reproduces_the_reference(fixture):
    from spatial_clip_amd import metrics
    r_i, r_t = RO.ranks(fixture["fi"], fixture["ft"])
    got = metrics.retrieval_summary(r_i.astype(np.int32), r_t.astype(np.int32), (1, 5, 10))
    for k, v in fixture["ref"].items():
        assert got[k] == v, (k, got[k], v)
    assert got == RO.summary(r_i, r_t)
    pre = metrics.retrieval_summary(r_i, r_t, (1, 5, 10), prefix="val/")
    assert pre == {"val/" + k: v for k, v in got.items()}
    assert list(pre)[:5] == ["val/image_to_text_mean_rank", "val/image_to_text_median_rank", "val/image_to_text_R@1",
                             "val/image_to_text_R@5", "val/image_to_text_R@10"]
    assert all(isinstance(v, float) for v in pre.values())


def test_retrieval_summary_median_floor_and_large_k():
    from spatial_clip_amd import metrics
    # even N: median of {0, 1, 2, 5} is 1.5 -> floor 1 -> +1 = 2 ; of {0, 3} is 1.5 too
    s = metrics.retrieval_summary([5, 0, 2, 1], [3, 0, 0, 3], ks=(1, 3, 100))
    assert s["image_to_text_median_rank"] == 2.0 and s["image_to_text_mean_rank"] == 3.0
    assert s["text_to_image_median_rank"] == 2.0 and s["text_to_image_mean_rank"] == 2.5
    assert s["image_to_text_R@1"] == 0.25 and s["image_to_text_R@3"] == 0.75
    assert s["image_to_text_R@100"] == 1.0 and s["text_to_image_R@100"] == 1.0          # k > N: every pair is a hit
    assert s["text_to_image_R@1"] == 0.5 and s["retrieval_num_samples"] == 4.0
    assert "image_to_text_R@5" not in s
    one = metrics.retrieval_summary([0], [0])
    assert one["image_to_text_mean_rank"] == 1.0 and one["text_to_image_median_rank"] == 1.0 and one["image_to_text_R@1"] == 1.0
    with pytest.raises(ValueError, match="ranks"):
        metrics.retrieval_summary([0, 1], [0])
    for bad in ((), (0,), (1.5,), (True,)):
        with pytest.raises(ValueError, match="ks"):
            metrics.retrieval_summary([0], [0], ks=bad)


def test_oracle_tie_rule_and_non_finite():
    # rows 0 and 2 of the text side are equal: pair 0 and pair 2 tie exactly in row 0 / row 2 and are ordered by index
    fi = np.array([[1, 0], [0, 1], [1, 0]], dtype=np.float32)
    ft = np.array([[1, 0], [0, 1], [1, 0]], dtype=np.float32)
    r_i, r_t = RO.ranks(fi, ft)
    assert r_i.tolist() == [0, 0, 1] and r_t.tolist() == [0, 0, 1]
    fi[1] = np.nan
    r_i, r_t = RO.ranks(fi, ft)
    assert r_i.tolist() == [0, 2, 1] and r_t.tolist() == [0, 2, 1]


@pytest.mark.parametrize("N,D", RO.RANDOM_CASES)
def test_fp32_matmul_stays_within_the_allowances(N, D):
    """The bound the device test holds the kernel to, applied to an fp32 ``torch`` matmul: a rank may differ from the float64
    one by at most the number of candidates within ``fp32_margin(D)`` of the diagonal, and few rows have any."""
    import torch
    fi, ft = RO.random_unit_case(N, D)
    z = RO.similarities(fi.numpy(), ft.numpy())
    want_i, want_t = RO.ranks_from_z(z)
    a_i, a_t = RO.allowances(z, RO.fp32_margin(D))
    print(f"N={N} D={D}: rows with an allowance {np.mean(a_i > 0):.3%}, columns {np.mean(a_t > 0):.3%}, "
          f"max {max(a_i.max(), a_t.max())}")
    assert np.mean(a_i > 0) <= 0.15 and np.mean(a_t > 0) <= 0.15
    got_i, got_t = RO.ranks_from_z((fi @ ft.t()).numpy())
    assert (np.abs(got_i - want_i) <= a_i).all() and (np.abs(got_t - want_t) <= a_t).all()


def test_full_retrieval_argument():
    from spatial_clip_amd import metrics, module
    assert "full_retrieval" in inspect.signature(module.SpatialClipLitModule.__init__).parameters
    assert inspect.signature(module.SpatialClipLitModule.__init__).parameters["full_retrieval"].default is None
    assert module.check_full_retrieval_cfg(None) is None and module.check_full_retrieval_cfg(False) is None
    assert module.check_full_retrieval_cfg(True) == (1, 5, 10)
    assert module.check_full_retrieval_cfg({"ks": [1, 20]}) == (1, 20) and module.check_full_retrieval_cfg({}) == (1, 5, 10)
    for bad in ("yes", 1, [1, 5], {"k": [1]}, {"ks": []}, {"ks": [0]}):
        with pytest.raises(ValueError, match="full_retrieval"):
            module.check_full_retrieval_cfg(bad)
        with pytest.raises(ValueError, match="full_retrieval"):        # checked before the module touches its net
            module.SpatialClipLitModule(None, None, None, None, full_retrieval=bad)
    m = metrics.RetrievalMetrics("val/", ks=(1, 2))
    assert m.prefix == "val/" and m.ks == (1, 2) and m.n == 0
    empty = m.compute()                       # nothing accumulated: no device is touched
    assert empty["val/retrieval_num_samples"] == 0.0 and np.isnan(empty["val/image_to_text_R@1"])


def test_header_declares_the_entry_point():
    from spatial_clip_amd import _lib
    decl = _lib.parse_header()
    assert "sc_retrieval_ranks" in decl
    restype, argtypes = decl["sc_retrieval_ranks"]
    assert len(argtypes) == 11
    src = open(_lib.HEADER_PATH).read()
    assert "int sc_abi_version(void);" in src
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().sc_abi_version() == 1


def test_config_key_and_experiment(monkeypatch):
    from spatial_clip_amd import hydra_lite as H
    monkeypatch.setenv("PROJECT_ROOT", "/tmp/proj")
    base = H.compose("train.yaml", ["experiment=vitb16_gene_b256"])
    assert "full_retrieval" in base.model and base.model.full_retrieval is None
    cfg = H.compose("train.yaml", ["experiment=vitb16_gene_b256_full_retrieval"])
    assert cfg.model.full_retrieval is True
    assert cfg.callbacks.model_checkpoint.monitor == "val/image_to_text_R@5" and cfg.callbacks.model_checkpoint.mode == "max"
    assert cfg.callbacks.early_stopping.monitor == "val/image_to_text_R@5"
    assert cfg.data.batch_size == base.data.batch_size and cfg.model.net.model_name == base.model.net.model_name
