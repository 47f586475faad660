"""Plan against launch: for the boundary shapes of tests/_gemmpaths.py (LAUNCHES), the kernel that ran
(``ops.gemm_last_path`` / ``ops.gemm_last_tail``) is the one ``ops.gemm_plan`` names for the device's CU count, it is the one
the library reported before the planner existed (tests/golden/gemm_paths_parent.json, recorded with
tools/record_gemm_paths.py), and the result agrees with ``torch.matmul`` in float64 of the bf16 operands at the tolerances
of tests/test_gpu_gemm.py.  K is one to three K tiles, so every launch is short; the persistent-kernel shapes' 128 MiB output
is the largest allocation.  The switches are flipped inside this one process."""
import json
import os

import pytest
import torch

from tests import _gemmpaths as P

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_paths_parent.json")


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


def _rand(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _close(got, ref64, atol, rtol):
    torch.testing.assert_close(got.double(), ref64, atol=atol, rtol=rtol)


def _bf16(ref64):
    return ref64.to(torch.bfloat16).double()


def run_launch(ops, case):
    """Run one entry of P.LAUNCHES under the environment already in place and check its result; returns what the library
    recorded: (GemmPath as a list, [nfull, rem])."""
    entry, mode, epi_name, M, N, K, splitk, _ = case
    epi = getattr(ops, "EPI_" + epi_name)
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
    if entry == "gemm" and mode == P.NT:
        a, b = _rand((M, K), g), _rand((N, K), g, 0.1)
        ref = a.double() @ b.double().t()
    else:
        # dY, X: rows padded to the 16 bytes the library asks of every leading dimension
        a, b = _rand((K, (M + 7) // 8 * 8), g)[:, :M], _rand((K, (N + 7) // 8 * 8), g, 0.1)[:, :N]
        ref = a.double().t() @ b.double()
    f32 = epi_name in ("F32", "F32_BIAS_RES")
    out = torch.full((M, N), 7.0, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
    bias_tol = 2e-3 * max(1.0, K ** 0.5 / 8)
    if entry == "gemm":
        kw, u = {}, None
        if epi_name in ("BF16_BIAS", "GELU_GRAD_PAIR"):
            kw["bias"] = torch.randn(N, generator=g, device="cuda")
            ref = ref + kw["bias"].double()
        if epi_name == "GELU_GRAD_PAIR":
            kw["out2"] = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
            u = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")     # the kernel's own u, from the u-storing pair
            ops.gemm(mode, ops.EPI_GELU_PAIR, a, b, u, M=M, N=N, K=K, bias=kw["bias"], out2=torch.empty_like(u))
        ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True)
        ops.gemm(mode, epi, a, b, out, M=M, N=N, K=K, splitk=splitk, **kw)
        rec = (ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True))
        if epi_name == "GELU_GRAD_PAIR":
            _close(u, _bf16(ref), 2e-2, 2e-2)
            x = u.double().requires_grad_(True)
            y = torch.nn.functional.gelu(x)
            y.sum().backward()
            _close(kw["out2"], _bf16(y.detach()), 8e-3, 8e-3)
            _close(out, _bf16(x.grad), 4e-3, 8e-3)
        elif f32:
            _close(out, ref, 1e-3, 1e-3)
        else:
            _close(out, _bf16(ref), 2e-2, 2e-2)
    elif entry == "wgrad_bias":
        db = torch.full((M,), 7.0, dtype=torch.float32, device="cuda")
        ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True)
        ops.gemm_wgrad_bias(a, b, out, db, M=M, N=N, K=K, splitk=splitk)
        rec = (ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True))
        _close(out, ref, 1e-3, 1e-3)
        _close(db, a.double().sum(0), bias_tol, 1e-4)
    else:                                                        # wgrad_group: this problem with a bias gradient + its N x M twin
        db = torch.full((M,), 7.0, dtype=torch.float32, device="cuda")
        out2 = torch.full((N, M), 7.0, dtype=torch.float32, device="cuda")
        ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True)
        ops.gemm_wgrad_group([(a, b, out, db, M, N), (b, a, out2, None, N, M)], K=K, splitk=splitk)
        rec = (ops.gemm_last_path(reset=True), ops.gemm_last_tail(reset=True))
        _close(out, ref, 1e-3, 1e-3)
        _close(out2, ref.t(), 1e-3, 1e-3)
        _close(db, a.double().sum(0), bias_tol, 1e-4)
    return [list(rec[0]), list(rec[1])]


def _set(monkeypatch, env):
    for k in P.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _planned(ops, case, slots):
    entry, mode, epi_name, M, N, K, splitk, _ = case
    has_slabs = True
    if entry == "gemm":                  # ops.gemm passes slabs, and the split-K request, only where K has tiles to split
        from spatial_clip_amd import _lib
        has_slabs = _lib.lib().sc_gemm_slab_floats(M, N, K, splitk) > 0
        splitk = splitk if has_slabs else 1
    return ops.gemm_plan(mode, getattr(ops, "EPI_" + epi_name), M, N, K, splitk=splitk, has_slabs=has_slabs,
                         colsum=entry == "wgrad_bias", slots=slots)


@pytest.mark.parametrize("case", P.LAUNCHES, ids=P.launch_key)
def test_launch_is_the_plan_and_the_parent_table(monkeypatch, case):
    ops = _ops()
    _set(monkeypatch, case[7])
    slots = torch.cuda.get_device_properties(0).multi_processor_count
    path, tail = run_launch(ops, case)
    plan, plan_tail = _planned(ops, case, slots)
    with open(GOLDEN) as f:
        golden = json.load(f)
    if case[0] == "wgrad_group":
        # the group plan is the per-problem big-tile rule over every problem and the single split-K plan
        if path[5] == "one_launch":
            assert plan.path == "tn8p" and path[:5] == ["tn8p_group", False, 0, plan.splitk, "fused"], (path, plan)
        else:                            # per problem: the record is the last problem's, the N x M twin without a bias gradient
            twin = ("gemm", P.TN, "F32", case[4], case[3], case[5], case[6], case[7])
            assert path == list(_planned(ops, twin, slots)[0])[:5] + ["per_problem"], (path, plan)
    else:
        assert path == list(plan) and tail == list(plan_tail), (path, tail, plan, plan_tail)
    if slots == golden["slots"]:
        assert [path, tail] == golden["launches"][P.launch_key(case)], (path, tail)
    else:
        assert path == golden["launches"][P.launch_key(case)][0], path


def test_the_switches_move_the_path_inside_one_process(monkeypatch):
    """SC_GEMM_FORCE, SC_GEMM_PERSIST and SC_GEMM_SMALL_TILES are read per call: one process sees every setting, in either
    order."""
    ops = _ops()
    want = {"gemm NT BF16 2560x2560x128 sk1 -": "nt8p", "gemm NT BF16 2560x2560x128 sk1 SC_GEMM_FORCE=128": "nt128",
            "gemm NT BF16 8192x8192x192 sk1 -": "nt8p_persistent", "gemm NT BF16 8192x8192x192 sk1 SC_GEMM_PERSIST=0": "nt8p",
            "gemm NT BF16 2552x2560x128 sk1 -": "nt128", "gemm NT BF16 2552x2560x128 sk1 SC_GEMM_SMALL_TILES=0": "nt8p",
            "gemm TN F32 512x1024x192 sk2 -": "tn8p", "gemm TN F32 512x1024x192 sk2 SC_GEMM_FORCE=256": "tn256",
            "gemm TN F32 512x1024x192 sk2 SC_GEMM_FORCE=128": "tn128"}
    cases = [c for c in P.LAUNCHES if P.launch_key(c) in want]
    assert len(cases) == len(want)
    for case in cases + cases[::-1]:
        _set(monkeypatch, case[7])
        assert run_launch(ops, case)[0][0] == want[P.launch_key(case)], P.launch_key(case)


@pytest.mark.parametrize("mode,name", [(P.NT, "nt256"), (P.TN, "tn256")])
def test_two_stage_kernel(monkeypatch, mode, name):
    """The 256x256 two-stage LDS-DMA kernel (SC_GEMM_FORCE=256): ragged M and N, three K tiles in two split-K slices (an
    unsplit NT launch of nine tiles would go to the 128x128 kernel), against float64."""
    ops = _ops()
    _set(monkeypatch, {"SC_GEMM_FORCE": "256"})
    M, N, K = 256 * 3 + 40, 256 * 3 - 24, 192
    g = torch.Generator(device="cuda").manual_seed(256)
    if mode == P.NT:
        a, b = _rand((M, K), g), _rand((N, K), g, 0.1)
        ref = a.double() @ b.double().t()
    else:
        a, b = _rand((K, M), g), _rand((K, N), g, 0.1)
        ref = a.double().t() @ b.double()
    out = torch.full((M, N), 7.0, dtype=torch.float32, device="cuda")
    ops.gemm_last_path(reset=True)
    ops.gemm(mode, ops.EPI_F32, a, b, out, M=M, N=N, K=K, splitk=2)
    p = ops.gemm_last_path(reset=True)
    assert p == ops.gemm_plan(mode, ops.EPI_F32, M, N, K, splitk=2, has_slabs=True)[0]
    assert (p.path, p.splitk) == (name, 2), p
    _close(out, ref, 1e-3, 1e-3)
