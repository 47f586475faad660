"""Float64 restatement of the full-set retrieval metrics (the reference's ``get_clip_metrics``,
src/open_clip_train/train.py:383-400) with a DEFINED tie rule: the rank of pair i is the 0-based position of its ground
truth under a stable descending sort, i.e. the number of other candidates that score higher, or equal with a smaller index.
A diagonal that is not finite is ranked last (N - 1).  Shared by tests/test_cpu_retrieval.py and tests/test_gpu_retrieval.py."""
import numpy as np


def similarities(image_features, text_features) -> np.ndarray:
    """z[i, j] = <image_i, text_j> in float64 (raw cosines: no logit_scale)."""
    a = np.asarray(image_features, dtype=np.float64)
    b = np.asarray(text_features, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return a @ b.T


def ranks_from_z(z: np.ndarray):
    """(rank_i2t, rank_t2i), int64 [N] each, from a square similarity matrix."""
    n = z.shape[0]
    idx = np.arange(n)
    d = np.diagonal(z).copy()
    off = idx[:, None] != idx[None, :]
    with np.errstate(invalid="ignore"):
        # image -> text: row i against d_i, ties to the smaller column index
        above_r = (z > d[:, None]) | ((z == d[:, None]) & (idx[None, :] < idx[:, None]))
        # text -> image: column j against d_j, ties to the smaller row index
        above_c = (z > d[None, :]) | ((z == d[None, :]) & (idx[:, None] < idx[None, :]))
    bad = ~np.isfinite(d)
    above_r |= bad[:, None]
    above_c |= bad[None, :]
    return (above_r & off).sum(axis=1).astype(np.int64), (above_c & off).sum(axis=0).astype(np.int64)


def ranks(image_features, text_features):
    return ranks_from_z(similarities(image_features, text_features))


def allowances(z: np.ndarray, margin: float):
    """Per row / per column: how many other candidates lie within ``margin`` of the diagonal (the pairs whose order an
    fp32 evaluation of the two dot products may legitimately flip)."""
    n = z.shape[0]
    d = np.diagonal(z)
    off = ~np.eye(n, dtype=bool)
    a_row = ((np.abs(z - d[:, None]) < margin) & off).sum(axis=1)
    a_col = ((np.abs(z - d[None, :]) < margin) & off).sum(axis=0)
    return a_row, a_col


RANDOM_CASES = ((1, 8), (17, 5), (129, 33), (257, 64), (130, 512), (1000, 64), (2049, 96))


def fp32_margin(D: int) -> float:
    """Worst-case difference between the fp32 errors of two dot products of unit vectors of length D: each is off by at
    most D * 2^-24 (D roundings of partial sums of magnitude <= 1), so a gap below twice that may legitimately flip."""
    return 2.0 * D * 2.0 ** -24


def random_unit_case(N: int, D: int):
    """Unit features with ranks spread over 1..N: text = normalize(image + noise * randn), drawn in float64 and cast to fp32."""
    import torch
    g = torch.Generator().manual_seed(1000 + N + D)
    noise = 3.0 if D == 512 else 0.7
    fi = torch.nn.functional.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=-1)
    ft = torch.nn.functional.normalize(fi + noise * torch.randn(N, D, generator=g, dtype=torch.float64), dim=-1)
    return fi.float(), ft.float()


def exact_case(N: int, D: int, seed: int = 0):
    """Entries from {-1, -0.5, 0, 0.5, 1} * 2^-k, k in 0..3, D <= 16: every product is a multiple of 2^-8 of magnitude <= 1
    and every partial sum of up to 16 of them is exact in fp32 in any order -- the float64 oracle and the device see the same
    numbers, ties included."""
    import torch
    assert D <= 16
    g = torch.Generator().manual_seed(4000 + 7 * N + D + seed)
    m = torch.randint(-2, 3, (2, N, D), generator=g).to(torch.float32) * 0.5
    k = torch.randint(0, 4, (2, N, D), generator=g).to(torch.float32)
    f = m * torch.pow(2.0, -k)
    return f[0].clone(), f[1].clone()


def summary(rank_i2t, rank_t2i, ks=(1, 5, 10), prefix: str = ""):
    """The reference's ten quantities under its names (+ ``retrieval_num_samples``), from 0-based ranks."""
    out = {}
    for name, r in (("image_to_text", rank_i2t), ("text_to_image", rank_t2i)):
        r = np.asarray(r, dtype=np.int64)
        out[f"{prefix}{name}_mean_rank"] = float(r.mean() + 1)
        out[f"{prefix}{name}_median_rank"] = float(np.floor(np.median(r)) + 1)
        for k in ks:
            out[f"{prefix}{name}_R@{k}"] = float(np.mean(r < k))
    out[f"{prefix}retrieval_num_samples"] = float(len(rank_i2t))
    return out
