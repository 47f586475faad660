"""Every attention kernel behind sc_attn_fwd / sc_attn_bwd, forced one at a time by the dispatcher's environment switches,
at every length it accepts, against the float64 references and bounds of tests/_attnbounds.py (per-row bf16 rule, the fp32
lse rule, the delta chain rule, exact conditions on what stays unwritten, two bit-identical launches).  ``ops.attn_last_path()``
is asserted on every call: a path that declines a shape must fall back to the kernel the dispatcher documents, by name.

One test per (direction, path, head dim, causal); the lengths are looped inside and every failing (case, output, ratio) is
collected before the assertion.  Inside a path's accepted range every length runs on all three input families; outside it,
the boundary lengths run (the fallback, by name).  q_rows in {1, 15, 16, 17, L - 1} runs at the boundary lengths (``mixed``
family) on every path, accepted or declined.  The backward kernels get the model's forward results (see _attnbounds).

``expected_fwd`` / ``expected_bwd`` (tests/_attnpaths.py) restate the dispatcher's predicates (file:line beside each)."""
import pytest
import torch

from tests import _attnbounds as A
from tests._attnpaths import BWD_ENV, DEFAULT, FWD_ENV, SWITCHES, expected_bwd, expected_fwd, fused_fits

pytestmark = pytest.mark.gpu


def _ops():
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))          # the CPU references work on [6, L, L] operands
    yield
    torch.set_num_threads(n)


def test_fused_backward_stops_at_288_tokens_at_head_dim_64():
    """The LDS predicate of the fused backward, in numbers: 288 is the last length at head dim 64; head dim 32 always fits."""
    assert [L for L in range(1, 321) if fused_fits(64, L)][-1] == 288 and all(fused_fits(32, L) for L in range(1, 321))


# ---------------------------------------------------------------------------------------------------------- running one case
WORST = {}


def _note(key, family, ratios, L):
    for k, v in ratios.items():
        w = WORST.setdefault(key + (family,), {})
        if not v <= w.get(k, (-1.0, 0))[0]:
            w[k] = (v, L)


def _report(key):
    for k, w in sorted(WORST.items()):
        if k[:len(key)] == key:
            print("SWEEP", *k, " ".join(f"{n} {v:.3g}@L{L}" for n, (v, L) in sorted(w.items())))


def run_fwd(ops, c, want, fails):
    Bc, L, Hc, dh = c.dims
    nq = c.nq
    qd = c.qkv.cuda()
    res = []
    for fill in (7.0, 3.0):
        out = torch.full((Bc * L, Hc * dh), fill, dtype=torch.bfloat16, device="cuda")
        lse = torch.full((Bc, Hc, L), fill, device="cuda")
        ops.attn_fwd(qd, Bc, L, Hc, dh, c.causal, out=out, lse=lse, q_rows=c.q_rows)
        got = ops.attn_last_path()[0]
        if got != want:
            fails.append((c.tag(), "path", got, want))
        res.append((A.heads(out, Bc, L, Hc, dh).cpu(), lse.cpu()))
    (o, l), (o2, l2) = res
    r = {"out": c.ratio_out(o), "lse": c.ratio_lse(l)}
    print(c.tag(), want, " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k, v in r.items():
        if not v <= 1.0:
            fails.append((c.tag(), k, v))
    if not (torch.equal(o[:, :, :nq], o2[:, :, :nq]) and torch.equal(l[:, :, :nq], l2[:, :, :nq])):
        fails.append((c.tag(), "two launches differ"))
    if not (bool((o[:, :, nq:] == 7.0).all()) and bool((l[:, :, nq:] == 7.0).all())):
        fails.append((c.tag(), "rows >= q_rows of out / lse were written"))
    return r


def writes_all_of_dqkv(path):
    """ops.attn_bwd's docstring: at head dim 80 and on the long-sequence path (both: stream) and with q_rows == 1 (cls)."""
    return path in ("stream", "cls")


def run_bwd(ops, c, want, fails):
    Bc, L, Hc, dh = c.dims
    nq = c.nq
    qd, od, gd, ld = c.qkv.cuda(), c.out_in.cuda(), c.dout.cuda(), c.lse_in.cuda()
    res = []
    for fill in (7.0, 3.0):
        dqkv = torch.full((Bc * L, 3 * Hc * dh), fill, dtype=torch.bfloat16, device="cuda")
        delta = torch.full((Bc, Hc, L), fill, device="cuda")
        ops.attn_bwd(qd, od, gd, ld, Bc, L, Hc, dh, c.causal, dqkv=dqkv, delta=delta, q_rows=c.q_rows)
        got = ops.attn_last_path()[1]
        if got != want:
            fails.append((c.tag(), "path", got, want))
        res.append((A.grad_heads(dqkv, Bc, L, Hc, dh).cpu(), delta.cpu()))
    (g, dl), (g2, _) = res
    r = c.ratio_grads(g)
    r["delta"] = c.ratio_delta(dl[:, :, :nq])
    print(c.tag(), want, " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k, v in r.items():
        if not v <= 1.0:
            fails.append((c.tag(), k, v))
    if not (torch.equal(g[0][:, :, :nq], g2[0][:, :, :nq]) and torch.equal(g[1:], g2[1:])):
        fails.append((c.tag(), "two launches differ"))
    if nq < L and not c.dq_tail(g, None if writes_all_of_dqkv(want) else 7.0):
        fails.append((c.tag(), "dQ rows >= q_rows are neither zero nor (where nothing promises a write) untouched"))
    return r


def sweep(direction, path, dh, causal, monkeypatch):
    """All of a (direction, path, dh, causal): see the module docstring."""
    ops = _ops()
    env = {**DEFAULT, **(FWD_ENV if direction == "fwd" else BWD_ENV)[path]}
    for k in SWITCHES:
        monkeypatch.setenv(k, env[k])
    expected, run = (expected_fwd, run_fwd) if direction == "fwd" else (expected_bwd, run_bwd)
    grads = direction == "bwd"
    key = (direction, path, dh, causal)
    fails, accepted, specs = [], 0, []
    for L in list(range(1, A.MAXL + 1)) + (A.STREAM_LONG_LENGTHS if path == "stream" and dh == 64 else []):
        boundary = L in A.BOUNDARY_LENGTHS
        want = expected(env, dh, L, causal, L)
        if want == path or boundary:
            specs += [(fam, fam, L, 0, want) for fam in A.FAMILIES]
        if boundary:
            specs += [("mixed+q_rows", "mixed", L, r, expected(env, dh, L, causal, r)) for r in A.q_rows_at(L)]
    for label, fam, L, r, want in specs:
        accepted += want == path
        _note(key, label, run(ops, A.Case(fam, dh, L, causal, q_rows=r, want_grads=grads), want, fails), L)
    torch.cuda.synchronize()
    _report(key)
    assert accepted > 0, f"{path} never ran"
    assert not fails, (len(fails), fails[:25])


# ---------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("path,dh,causal", [("persistent", 64, False), ("persistent", 64, True),
                                            ("persistent2", 64, False), ("persistent2", 64, True),
                                            ("per_head", 64, False), ("per_head", 64, True),
                                            ("per_head", 32, False), ("per_head", 32, True),
                                            ("stream", 64, False), ("stream", 80, False), ("stream", 80, True)])
def test_forward_sweep(path, dh, causal, monkeypatch):
    sweep("fwd", path, dh, causal, monkeypatch)


@pytest.mark.parametrize("path,dh,causal", [("ring", 64, False), ("ring8", 64, False), ("single_pass", 64, False),
                                            ("persistent", 64, False), ("persistent", 64, True),
                                            ("fused", 64, False), ("fused", 64, True), ("fused", 32, False), ("fused", 32, True),
                                            ("dq_dkv", 64, False), ("dq_dkv", 64, True),
                                            ("dq_dkv", 32, False), ("dq_dkv", 32, True),
                                            ("stream", 64, False), ("stream", 80, False), ("stream", 80, True)])
def test_backward_sweep(path, dh, causal, monkeypatch):
    sweep("bwd", path, dh, causal, monkeypatch)


@pytest.mark.parametrize("dh", [32, 64, 80])
@pytest.mark.parametrize("causal", [False, True])
def test_backward_cls_sweep(dh, causal, monkeypatch):
    """q_rows = 1 at every L >= 2 (the rank-one kernel of sc_attention_cls.hip), all three families."""
    ops = _ops()
    for k in SWITCHES:
        monkeypatch.setenv(k, DEFAULT[k])
    fails = []
    for L in range(2, A.MAXL + 1):
        for fam in A.FAMILIES:
            _note(("bwd", "cls", dh, causal), fam, run_bwd(ops, A.Case(fam, dh, L, causal, q_rows=1), "cls", fails), L)
    _report(("bwd", "cls", dh, causal))
    assert not fails, (len(fails), fails[:25])


# ---------------------------------------------------------------------------------------------------------- head walking
WALK_B, WALK_PERIOD, WALK_H = 266, 7, 2       # 532 heads (more than twice the CUs); the batches repeat with period 7


@pytest.mark.parametrize("direction,path", [("fwd", "persistent"), ("fwd", "persistent2"), ("fwd", "stream"), ("bwd", "ring"),
                                            ("bwd", "ring8"), ("bwd", "single_pass"), ("bwd", "persistent"), ("bwd", "stream")])
def test_persistent_kernels_walk_heads_at_the_boundary_lengths(direction, path, monkeypatch):
    """B * H = 532 heads at every boundary length a persistent kernel accepts: each workgroup carries its LDS state from one
    head into the next.  The batches repeat with period 7 (14 distinct heads; the stride by which a workgroup walks, the CU
    count, is no multiple of 14, so consecutive heads of a workgroup differ): the first period is checked against the
    bounds, and every later period must reproduce it bit for bit, whichever workgroup computed it and after whichever head."""
    ops = _ops()
    env = {**DEFAULT, **(FWD_ENV if direction == "fwd" else BWD_ENV)[path]}
    for k in SWITCHES:
        monkeypatch.setenv(k, env[k])
    assert torch.cuda.get_device_properties(0).multi_processor_count % (WALK_PERIOD * WALK_H) != 0
    dh, causal, Hc = 64, False, WALK_H
    reps = WALK_B // WALK_PERIOD
    fails, ran = [], 0
    for L in A.BOUNDARY_LENGTHS:
        want = (expected_fwd if direction == "fwd" else expected_bwd)(env, dh, L, causal, L)
        if want != path:
            continue
        ran += 1
        c = A.Case("mixed", dh, L, causal, B=WALK_PERIOD, H=Hc, want_grads=direction == "bwd")
        rep = lambda t: t.view(WALK_PERIOD, -1).repeat(reps, 1).view(-1, t.shape[-1]).cuda()     # noqa: E731
        qd = rep(c.qkv)
        if direction == "fwd":
            out, lse = ops.attn_fwd(qd, WALK_B, L, Hc, dh, causal)
            got = ops.attn_last_path()[0]
            o1 = out.view(reps, WALK_PERIOD * L, Hc * dh)
            l1 = lse.view(reps, WALK_PERIOD, Hc, L)
            same = bool((o1 == o1[:1]).all()) and bool((l1 == l1[:1]).all())
            r = {"out": c.ratio_out(A.heads(o1[0], WALK_PERIOD, L, Hc, dh).cpu()), "lse": c.ratio_lse(l1[0].cpu())}
        else:
            lse_in = c.lse_in.repeat(reps, 1, 1).cuda()
            delta = torch.empty(WALK_B, Hc, L, device="cuda")
            dqkv = ops.attn_bwd(qd, rep(c.out_in), rep(c.dout), lse_in, WALK_B, L, Hc, dh, causal, delta=delta)
            got = ops.attn_last_path()[1]
            g1 = dqkv.view(reps, WALK_PERIOD * L, 3 * Hc * dh)
            d1 = delta.view(reps, WALK_PERIOD, Hc, L)
            same = bool((g1 == g1[:1]).all()) and bool((d1 == d1[:1]).all())
            r = c.ratio_grads(A.grad_heads(g1[0], WALK_PERIOD, L, Hc, dh).cpu())
            r["delta"] = c.ratio_delta(d1[0].cpu())
        print(c.tag(), got, " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        _note((direction, path + "+walk", dh, causal), "mixed", r, L)
        fails += [(c.tag(), k, v) for k, v in r.items() if not v <= 1.0]
        if got != path:
            fails.append((c.tag(), "path", got, path))
        if not same:
            fails.append((c.tag(), "a later period of heads differs from the first"))
    _report((direction, path + "+walk", dh, causal))
    assert ran > 0 and not fails, (ran, len(fails), fails[:25])
