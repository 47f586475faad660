#!/usr/bin/env python3
"""Golden vectors for optimiser parameter groups: the REFERENCE's tiny CLIP trained for three steps by the train3 recipe of
make_golden.py (same batch, SpatialLoss arguments, betas (0.9, 0.98), eps 1e-6, clip 1.0, warm-up 2 of 10 steps) with
``torch.optim.AdamW`` over TWO parameter groups, each with its own learning rate and weight decay.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_param_groups.py

The split is the usual one of CLIP training -- gains, biases and scalars apart from the matrices -- by the predicate
``is_no_decay`` below; the list of the first group's names is stored as ``no_decay``.  The SCALARS of the two groups are not
open_clip's (0 / 0.1): they are chosen so that the fixture tells a grouped optimiser from an un-grouped one and from one that
mixes the two groups up, which the script ASSERTS before it writes anything -- the reference's own ``p3`` (a) with every
tensor in one group at the base scalars and (b) with the scalars of the two groups swapped must each leave at least one
tensor 5 x outside the bound the test applies (3e-3, i.e. a distance of 1.5e-2).

How they are chosen.  The schedule gives the three steps 0, 1/2 and 1 times the learning rate, so a tensor moves by at most
about 1.5 lr through Adam's term.  Telling the runs apart through the learning rate would need lr >= 1e-2 in one group -- and
in its first updates Adam moves every element by lr * sign(g) whatever |g| is, so each element whose gradient lies within the
bf16 noise of zero lands up to 2 * 1.5 lr = 3e-2 away in a run that computes in bf16, the reference's own autocast run
included: the comparison would measure which elements happen to flip (a first fixture with lr 2e-2 showed exactly that,
profiles/param_groups_parity.txt).  The decoupled weight decay has no such sensitivity: it moves p by lr * wd * p, a
function of the weight alone.  The LayerNorm gains start at exactly 1, so (lr 1e-3, wd 12) moves them by 1.5e-3 * 12 = 1.8e-2
where (1e-3, 0.1) moves them by 1.5e-4: 1.78e-2 apart, past 1.5e-2, while the sign-sensitive part stays what it is in every
other train3 fixture (lr 1e-3).  The second group also trains at half the learning rate, so both scalars differ per group.

Writes ``train3_tiny_text_groups.npz``: the three losses, the three pre-clip gradient norms, ``p3.<name>`` for every tensor,
``no_decay`` (JSON list of the first group's names), ``groups`` (JSON: the two groups' lr and weight_decay and the base
scalars) and ``ac_rel_p3`` (JSON) -- per tensor, max|p3_autocast - p3_fp32| of the same recipe under
``torch.autocast("cpu", dtype=torch.bfloat16)``, the reference's own bf16 policy: the yardstick of a weight that misses the
3e-3 bound.  The starting weights are the ``p0.*`` of ``train3_tiny_text.npz`` and are not stored again; ``p0_sha256``
(make_golden_accum.p0_digest) pins them.

``param_groups_manifest.json``: for the reference's ViT-B-16, ViT-B-32 and ViT-L-14 (the models of state_dict_manifest.json)
the names ``is_no_decay`` puts into the first group, from the reference model's own ``named_parameters()``.  Only data is
written; no reference source is copied."""
import sys

sys.dont_write_bytecode = True
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_accum as MA  # noqa: E402

BASE = {"lr": 1e-3, "weight_decay": 0.1}                      # the train3 recipe's un-grouped scalars
GROUPS = {"vectors": {"lr": 1e-3, "weight_decay": 12.0},      # gains, biases, scalars (the names in ``no_decay``)
          "matrices": {"lr": 5e-4, "weight_decay": 0.1}}      # matrices and embeddings
FRAGMENTS = ("bn", "ln", "bias", "logit_scale")
WEIGHT_BOUND = 3e-3


def is_no_decay(name, p):
    """Vectors and scalars, and anything named like a norm layer, a bias or the temperature, train without weight decay."""
    return p.ndim <= 1 or any(f in name for f in FRAGMENTS)


def train(model, ref_losses, tiny, p0, z, grouping, autocast):
    """``grouping``: None (one group at BASE) or (no_decay scalars, decay scalars)."""
    clip = model.CLIP(**tiny)
    clip.load_state_dict(p0)
    named = list(clip.named_parameters())
    first = [n for n, p in named if is_no_decay(n, p)]
    if grouping is None:
        opt = torch.optim.AdamW(clip.parameters(), betas=(0.9, 0.98), eps=1e-6, **BASE)
    else:
        opt = torch.optim.AdamW([{"params": [p for n, p in named if n in first], **grouping[0]},
                                 {"params": [p for n, p in named if n not in first], **grouping[1]}],
                                betas=(0.9, 0.98), eps=1e-6, **BASE)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, MA.lam)
    crit = ref_losses.SpatialLoss(local_loss=True, gather_with_grad=True, cap_logit_scale=40.0, temp_reg_weight=0.05,
                                  neighbor_alpha_scale=0.5, float32_logits=True)
    images, texts = torch.from_numpy(z["images"]), torch.from_numpy(z["texts"])
    ids, nb, al = torch.from_numpy(z["ids"]), torch.from_numpy(z["nb"]), torch.from_numpy(z["alpha"])
    losses, norms = [], []
    for step in range(3):
        opt.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f_i = clip.encode_image(images, normalize=True)
            f_t = clip.encode_text(texts, normalize=True)
            l = crit(f_i, f_t, clip.logit_scale.exp(), ids, ids.clone(), nb, al)["contrastive_loss"]
        l.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(clip.parameters(), 1.0)))
        opt.step()
        sched.step()
        losses.append(float(l.detach()))
    return losses, norms, first, {k: v.detach().clone().float() for k, v in clip.state_dict().items()}


def manifest(model):
    """The first group's names for the full-size models, from the reference's own parameter lists (meta device: no memory)."""
    with open(os.path.join(HERE, "state_dict_manifest.json")) as f:
        shapes = json.load(f)
    out = {}
    for name in sorted(shapes):
        with open(f"{MG.REF}/src/open_clip/model_configs/{name}.json") as f:
            cfg = json.load(f)
        with torch.device("meta"):
            clip = model.CLIP(**cfg)
        named = list(clip.named_parameters())
        assert {n: list(p.shape) for n, p in named} == {n: s for n, s in shapes[name].items() if n in dict(named)}
        out[name] = {"no_decay": [n for n, p in named if is_no_decay(n, p)], "parameters": len(named)}
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, _, ref_losses = MG.import_reference()
    z = np.load(os.path.join(HERE, "train3_tiny_text.npz"), allow_pickle=False)
    tiny = json.loads(str(z["cfg"]))
    assert int(z["warmup"]) == MA.WARM and int(z["total"]) == MA.TOTAL
    p0 = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0.")}
    pair = (GROUPS["vectors"], GROUPS["matrices"])
    losses, norms, first, p3 = train(model, ref_losses, tiny, p0, z, pair, autocast=False)
    _, _, _, ac_p3 = train(model, ref_losses, tiny, p0, z, pair, autocast=True)
    ac_rel = {k: float((ac_p3[k] - p3[k]).abs().max()) for k in p3}
    bound = {k: max(WEIGHT_BOUND, 1.5 * ac_rel[k]) for k in p3}
    # the un-grouped recipe reproduces train3_tiny_text.npz (same reference, same batch): the recipe here is that recipe
    one_losses, _, _, one_p3 = train(model, ref_losses, tiny, p0, z, None, autocast=False)
    assert np.allclose(one_losses, z["losses"], rtol=0, atol=1e-6), (one_losses, z["losses"])
    _, _, _, swapped_p3 = train(model, ref_losses, tiny, p0, z, (pair[1], pair[0]), autocast=False)
    for tag, wrong in (("no grouping", one_p3), ("scalars swapped", swapped_p3)):
        ratio = {k: float((wrong[k] - p3[k]).abs().max()) / bound[k] for k in p3}
        worst = max(ratio, key=ratio.get)
        print(f"{tag}: {sum(r >= 5 for r in ratio.values())} of {len(ratio)} tensors >= 5 x their bound; furthest {worst} "
              f"at {ratio[worst]:.1f} x")
        assert ratio[worst] >= 5.0, f"{tag}: the fixture does not tell this run from the grouped one; choose other scalars"
    assert sorted(first) != sorted(p3) and first, "both groups must be populated"
    arrs = {"cfg": json.dumps(tiny), "warmup": MA.WARM, "total": MA.TOTAL, "p0_from": "train3_tiny_text.npz",
            "p0_sha256": MA.p0_digest(z), "no_decay": json.dumps(first),
            "groups": json.dumps({"base": BASE, **GROUPS}), "losses": np.array(losses), "grad_norms": np.array(norms),
            "ac_rel_p3": json.dumps(ac_rel)}
    for k, v in p3.items():
        arrs["p3." + k] = v
    name = "train3_tiny_text_groups.npz"
    MG.npz(name, **arrs)
    size = os.path.getsize(os.path.join(HERE, name))
    print("losses", losses, "norms", norms, "no_decay", len(first), "of", len(p3), "bytes", size)
    print("autocast distance in p3: max", max(ac_rel.values()), "tensors past 2e-3:", sum(v > 2e-3 for v in ac_rel.values()))
    assert size < 1024 * 1024, f"{name}: {size} bytes is past the limit for a committed file"
    with open(os.path.join(HERE, "param_groups_manifest.json"), "w") as f:
        json.dump(manifest(model), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
