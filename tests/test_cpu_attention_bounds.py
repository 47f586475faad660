"""CPU-side check of the attention sweep's bounds (tests/_attnbounds.py) on the exact inputs of
tests/test_gpu_attention_sweep.py: the bound is fair (a second, differently ordered emulation of a bf16 attention kernel
passes every bound) and it has teeth (every mutant of the float64 mathematics fails on every case where it changes the
result).  No GPU, no project kernel.

Lengths: every boundary length of the sweep (``BOUNDARY_LENGTHS``), every 32nd length from 5 on (5, 37, ..., 293: the
lengths that end a tile or exceed one by a token are at the boundary lengths already; the whole 1..320 range takes minutes
here), and at head dim
64, non-causal, three of the streamed kernels' long lengths (321, 577, 1025).  q_rows: every value of the sweep, at the
boundary lengths, on the ``mixed`` family."""
import math

import pytest
import torch

from tests import _attnbounds as A

COMBOS = [(64, False), (64, True), (32, False), (32, True), (80, False), (80, True)]
LENGTHS = sorted(set(A.BOUNDARY_LENGTHS) | set(range(5, 321, 32)) | {1})
LONG = [321, 577, 1025]

MUTANTS = ["scale", "drop_last", "drop_stray", "mask+1", "mask-1", "no_delta", "stale_max", "zero_last_dkv", "ignore_q_rows"]


@pytest.fixture(autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))          # [6, L, L] operands: more threads only wait for each other
    yield
    torch.set_num_threads(n)


def cases(dh, causal):
    for L in LENGTHS + (LONG if (dh == 64 and not causal) else []):
        for fam in A.FAMILIES:
            yield A.Case(fam, dh, L, causal)
        if L in A.BOUNDARY_LENGTHS:
            for r in A.q_rows_at(L):
                yield A.Case("mixed", dh, L, causal, q_rows=r)


def all_ratios(c, out, lse, g, delta=None):
    r = {"out": c.ratio_out(out), "lse": c.ratio_lse(lse)}
    r.update(c.ratio_grads(g))
    r["dq_tail"] = 0.0 if c.dq_tail(g) else math.inf         # dQ rows >= q_rows: exactly zero
    if delta is not None:
        r["delta"] = c.ratio_delta(delta)
    return r


def test_manual_formulas_are_the_autograd_reference():
    """The hand-written float64 formulas (the base of the model and of the mutants) against autograd, unmutated."""
    for dh, L, causal, q_rows in [(64, 33, False, 0), (32, 65, True, 0), (80, 17, True, 5), (64, 77, False, 16)]:
        c = A.Case("mixed", dh, L, causal, q_rows)
        B, _, H, _ = c.dims
        out, lse = A.manual_fwd(c.qkv, B, L, H, dh, causal, torch.float64, False)
        g, _ = A.manual_bwd(c.qkv, out, c.dout, lse, B, L, H, dh, causal, q_rows, torch.float64, False)
        torch.testing.assert_close(out, c.out64, atol=1e-12, rtol=1e-12)
        torch.testing.assert_close(lse, c.lse64, atol=1e-12, rtol=1e-12)
        torch.testing.assert_close(g, c.g64, atol=1e-11, rtol=1e-11)


def test_peaked_family_peaks_at_the_last_visible_key():
    for dh, causal in COMBOS:
        for L in (2, 17, 197, 257, 320):
            c = A.Case("peaked", dh, L, causal, want_grads=False)
            assert A.peak_property(c.qkv, *c.dims, causal), c.tag()
            q, k, _ = A.split_heads(c.qkv.double(), *c.dims)
            s = (q @ k.transpose(-1, -2)) * A.scale_f32(dh)
            if L >= 197:
                assert 55 < float(s.max()) < 90 and float(s.min()) < -25, (c.tag(), float(s.max()), float(s.min()))


@pytest.mark.parametrize("dh,causal", COMBOS)
def test_bound_is_fair_to_a_tiled_online_softmax_emulation(dh, causal):
    """Flash-style emulation (online softmax over 64-key tiles, exp2 domain, P recomputed from lse in the backward, other
    summation orders than the model's) must pass every bound: a legitimate reordering fits within REF_FACTOR."""
    fails, worst = [], {}
    for c in cases(dh, causal):
        B, L, H, _ = c.dims
        out, lse = A.tiled_fwd(c.qkv, B, L, H, dh, causal)
        g, delta = A.tiled_bwd(c.qkv, c.m_out, c.dout, c.m_lse, B, L, H, dh, causal, c.q_rows)
        r = all_ratios(c, out, lse, g, delta[:, :, :c.nq])
        print(c.tag(), " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        for k, v in r.items():
            if not v <= 1.0:
                fails.append((c.tag(), k, v))
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, c.tag())
    print("FAIR", f"dh{dh} causal={causal}", {k: (round(v, 3), t) for k, (v, t) in worst.items()})
    assert not fails, fails[:20]


def mutant_outputs(c, mut):
    """The float64 mathematics with one mutation: out, lse, d(qkv) (the backward on the mutant's own out / lse)."""
    B, L, H, dh = c.dims
    out, lse = A.manual_fwd(c.qkv, B, L, H, dh, c.causal, torch.float64, False, mut)
    lse_b = lse - 1e-3 if mut == "stale_max" else lse          # (the stale maximum spoils the lse output only)
    g, _ = A.manual_bwd(c.qkv, out, c.dout, lse_b, B, L, H, dh, c.causal, c.q_rows, torch.float64, False, mut)
    return out, lse, g


def changes_the_mathematics(c, mut, out, lse, g) -> bool:
    """A mutant applies to a case when fp32 arithmetic with correctly rounded outputs could show it.  Somewhere in what the
    API defines, its float64 result must be away from the reference's by more than

    * lse: half an fp32 ulp plus E32, what PyTorch's own fp32 logsumexp loses on these inputs;
    * out, gradients: half a bf16 ulp of the row's largest element (per row, like the rule under test) plus, for a
      gradient, the derived fp32 floor of that row (``fp32_floor``: what dP - delta loses in fp32 whatever the kernel).

    What this leaves out: the causal mask shifted up by one on the causal ``peaked`` family.  The added key lies 40 to 70
    below the row maximum: it moves lse by 3e-6 at most (E32 is 1.4e-5 there), out by 1e-5 and gradient rows that sit
    under a cancellation of size 1e-4 by 2e-5."""
    nq = c.nq

    def far(a, r, floor=0.0):
        return bool(((a - r).abs() > 0.5 * A.ulp(r.abs().amax(-1, keepdim=True), A.BF) + floor).any())

    r = c.lse64[:, :, :nq]
    far_lse = bool(((lse[:, :, :nq] - r).abs() > 0.5 * A.ulp(r, torch.float32) + c.lse_ref.e32).any())
    return far_lse or far(out[:, :, :nq], c.out64[:, :, :nq]) or far(g, c.g64, c.floor_g.unsqueeze(-1))


@pytest.mark.parametrize("dh,causal", COMBOS)
def test_bound_has_teeth(dh, causal):
    """Every mutant of the float64 reference fails on every case where it changes the mathematics; the worst ratio of each
    under the old 2e-2 / 4e-2 rule is printed beside the new one."""
    slipped, table = [], {}
    for c in cases(dh, causal):
        for mut in MUTANTS:
            if (mut in ("mask+1", "mask-1") and not causal) or (mut == "ignore_q_rows" and not c.q_rows) or \
                    (mut == "drop_stray" and c.L % 16 != 1):
                continue
            out, lse, g = mutant_outputs(c, mut)
            if not changes_the_mathematics(c, mut, out, lse, g):
                continue
            r = all_ratios(c, out, lse, g)
            new = max(math.inf if math.isnan(v) else v for v in r.values())
            old = c.old_rule(out, g)
            print(f"MUTANT {mut:14s} {c.tag():40s} new {new:9.3g} old {old:7.3g}")
            t = table.setdefault(mut, {"n": 0, "new_min": math.inf, "old_min": math.inf, "old_pass": 0, "at": ""})
            t["n"] += 1
            t["old_min"] = min(t["old_min"], old)
            t["old_pass"] += old <= 1.0
            if new < t["new_min"]:
                t["new_min"], t["at"] = new, c.tag()
            if new <= 1.0:
                slipped.append((mut, c.tag(), round(new, 3)))
    for mut, t in table.items():
        print(f"TEETH dh{dh} causal={causal} {mut:14s} cases {t['n']:4d}  smallest ratio, new rule {t['new_min']:8.3g} "
              f"({t['at']})  old rule {t['old_min']:8.3g}; passed the old rule on {t['old_pass']} cases")
    assert not slipped, (len(slipped), slipped[:30])
