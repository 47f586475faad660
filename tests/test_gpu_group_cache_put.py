"""sc_group_cache_put (the group cache of Trainer accum_freq): one micro-batch's features, tile ids, neighbour ids and alphas
into row block j of the caches, against a NumPy restatement, bit for bit, with sentinels around every row block."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3
BIG = (1 << 40) + 12345         # ids above 2^32: both 4-byte halves carry bits


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import _lib, ops
    return _lib, ops


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.int32) if a.dtype == np.float32 else a


def _strided(rng, B, D, pad, off):
    """fp32 [B, D] rows inside a [B, off + D + pad] buffer: row stride above D, start ``off`` floats into each row."""
    big = rng.standard_normal((B, off + D + pad)).astype(np.float32)
    return big, (off, off + D)


def _case(B, D, K, j, pad, off, with_ids, rng):
    _, ops = _ops()
    dev = torch.device("cuda", torch.cuda.current_device())
    G = N * B
    img_big, (a, b) = _strided(rng, B, D, pad, off)
    txt_big, _ = _strided(rng, B, D, pad, off)
    src = {"image": img_big[:, a:b], "text": txt_big[:, a:b]}
    img_d, txt_d = torch.from_numpy(img_big).to(dev)[:, a:b], torch.from_numpy(txt_big).to(dev)[:, a:b]
    assert img_d.stride(0) == off + D + pad
    cache = {"image": np.full((G, D), np.nan, np.float32), "text": np.full((G, D), np.nan, np.float32)}
    kw = {}
    if with_ids:
        ids_i = rng.integers(-1000, 1000, B).astype(np.int64) + np.where(np.arange(B) % 2 == 0, BIG, -BIG)
        ids_t = ids_i[::-1].copy() - 7
        nb = rng.integers(-5, 5, (B, K)).astype(np.int64) * BIG - 3
        al = rng.standard_normal((B, K)).astype(np.float32)
        src.update(ids_i=ids_i, ids_t=ids_t, nb=nb, al=al)
        cache.update(ids_i=np.full(G, -1, np.int64), ids_t=np.full(G, -1, np.int64), nb=np.full((G, K), -1, np.int64),
                     al=np.full((G, K), np.nan, np.float32))
        kw = dict(image_tile_ids=torch.from_numpy(ids_i).to(dev), text_tile_ids=torch.from_numpy(ids_t).to(dev),
                  neighbor_tile_ids=torch.from_numpy(nb).to(dev), neighbor_alphas=torch.from_numpy(al).to(dev))
    dcache = {k: torch.from_numpy(v).to(dev) for k, v in cache.items()}
    if with_ids:
        kw.update(image_id_cache=dcache["ids_i"], text_id_cache=dcache["ids_t"], neighbor_id_cache=dcache["nb"],
                  neighbor_alpha_cache=dcache["al"])
    ops.group_cache_put(img_d, txt_d, dcache["image"], dcache["text"], j, N, **kw)
    torch.cuda.synchronize()
    bad = []
    for k, want in cache.items():
        want[j * B:(j + 1) * B] = src[k]            # the NumPy restatement: row block j, nothing else
        got = dcache[k].cpu().numpy()
        if not np.array_equal(_bits(got), _bits(want)):
            bad.append(k)
    return bad


@pytest.mark.parametrize("D", [1, 6, 32, 513])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_row_block_j_and_nothing_else(B, D):
    rng = np.random.default_rng(1000 * B + D)
    fails = []
    for K in (0, 1, 8):
        for j in (0, 1, 2):                     # first, middle and last slot
            for pad, off in ((0, 0), (3, 0), (4, 0), (7, 1), (4, 4)):       # compact; strides / starts off and on 16 bytes
                bad = _case(B, D, K, j, pad, off, True, rng)
                if bad:
                    fails.append((K, j, pad, off, bad))
    assert not fails, f"B={B} D={D}: (K, j, pad, off, caches with wrong bits or touched sentinels): {fails[:6]}"


@pytest.mark.parametrize("B,D", [(1, 1), (3, 6), (64, 32), (3, 513)])
def test_without_ids_and_neighbours(B, D):
    """ClipLoss / SigLipLoss: every id / neighbour pointer NULL."""
    rng = np.random.default_rng(B + D)
    for j in (0, 1, 2):
        assert not _case(B, D, 0, j, 3, 1, False, rng)


def test_null_neighbours_leave_their_caches_alone():
    """Ids given, neighbour pointers NULL: the neighbour caches keep their sentinels."""
    _lib, ops = _ops()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, D, K = 3, 6, 2
    f = torch.randn(B, D, device=dev)
    ci, ct = torch.full((N * B, D), float("nan"), device=dev), torch.full((N * B, D), float("nan"), device=dev)
    ids = torch.tensor([BIG, -BIG, 5], device=dev)
    idc_i, idc_t = torch.full((N * B,), -1, dtype=torch.int64, device=dev), torch.full((N * B,), -1, dtype=torch.int64, device=dev)
    nbc = torch.full((N * B, K), -1, dtype=torch.int64, device=dev)
    alc = torch.full((N * B, K), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().sc_group_cache_put(f.data_ptr(), D, f.data_ptr(), D, ids.data_ptr(), ids.data_ptr(), None, None, ci.data_ptr(),
                                       ct.data_ptr(), idc_i.data_ptr(), idc_t.data_ptr(), nbc.data_ptr(), alc.data_ptr(), B, D, K, 1,
                                       N, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(idc_i[B:2 * B], ids) and torch.equal(idc_t[B:2 * B], ids) and torch.equal(ci[B:2 * B], f)
    assert bool((idc_i[:B] == -1).all()) and bool((idc_i[2 * B:] == -1).all())
    assert bool((nbc == -1).all()) and bool(torch.isnan(alc).all())


def test_bad_shapes_return_an_error_and_launch_nothing():
    _lib, ops = _ops()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, D = 3, 6
    f = torch.randn(B, D, device=dev)
    ci, ct = torch.full((N * B, D), float("nan"), device=dev), torch.full((N * B, D), float("nan"), device=dev)
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream

    def put(B_, D_, K_, j_, N_, ld=D, img=f.data_ptr(), cache=ci.data_ptr()):
        return l.sc_group_cache_put(img, ld, f.data_ptr(), ld, None, None, None, None, cache, ct.data_ptr(), None, None, None,
                                    None, B_, D_, K_, j_, N_, st)

    for args in ((0, D, 0, 0, N), (-1, D, 0, 0, N), (B, 0, 0, 0, N), (B, -2, 0, 0, N), (B, D, 0, N, N), (B, D, 0, N + 1, N),
                 (B, D, 0, -1, N), (B, D, -1, 0, N), (B, D, 0, 0, 0)):
        assert put(*args) != 0, args
        assert b"sc_group_cache_put" in l.sc_last_error()
    assert put(B, D, 0, 0, N, ld=D - 1) != 0 and b"stride" in l.sc_last_error()
    assert put(B, D, 0, 0, N, img=None) != 0 and b"null" in l.sc_last_error()
    assert put(B, D, 0, 0, N, cache=None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ci).all()) and bool(torch.isnan(ct).all())
    with pytest.raises(ValueError, match="image_cache"):
        ops.group_cache_put(f, f, ci[:B], ct, 0, N)
    with pytest.raises(ValueError, match="cache"):
        ops.group_cache_put(f, f, ci, ct, 0, N, image_tile_ids=torch.zeros(B, dtype=torch.int64, device=dev))
    assert put(B, D, 0, N - 1, N) == 0                       # and the same call with good arguments does run
    torch.cuda.synchronize()
    assert torch.equal(ci[(N - 1) * B:], f) and bool(torch.isnan(ci[:(N - 1) * B]).all())
