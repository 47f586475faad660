"""The pure parts of the transformer stack's scheduling (spatial_clip_amd.stack), no GPU and no HIP call: the slot layout of the
fp8 delayed-scaling table and the weight-gradient launch decision, against values computed from the functions they replaced
(the index arithmetic spelled at every use; _group_ok / _splitk_for / _splitk_for_group called per branch)."""
import pytest

import spatial_clip_amd  # noqa: F401
from spatial_clip_amd.stack import Fp8Scales, wgrad_plan


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_scale_table_slots(layers):
    t = Fp8Scales(layers, "cpu")
    assert t.scale.shape == (4 * layers,) and t.scale_inv.shape == (4 * layers,) and t.amax.shape == (4 * layers, 64)
    assert t.hist.shape == (Fp8Scales.HISTORY, 4 * layers) and not t.ready and t.step == 0
    seen = set()
    for i in range(layers):
        for slot, k in ((t.h(i), 2 * i), (t.dU(i), 2 * i + 1), (t.a2(i), 2 * layers + 2 * i), (t.g(i), 2 * layers + 2 * i + 1)):
            scale, scale_inv, amax = slot
            assert scale.shape == (1,) and scale.storage_offset() == k and scale.data_ptr() == t.scale[k:k + 1].data_ptr()
            assert scale_inv.shape == (1,) and scale_inv.storage_offset() == k and scale_inv.data_ptr() == t.scale_inv[k:k + 1].data_ptr()
            assert amax.shape == (64,) and amax.storage_offset() == 64 * k and amax.data_ptr() == t.amax[k].data_ptr()
            seen.add(k)
    assert seen == set(range(4 * layers))           # every slot has exactly one name
    if layers > 1:                                  # the slot LayerNorm-1 backward of block i fills is block i - 1's g
        assert t.g(0)[0].storage_offset() == 2 * layers + 2 * (1 - 1) + 1


def _branches(d, mlp):
    return [(d, d), (3 * d, d)], [(d, mlp), (mlp, d)]          # (out_proj, in_proj), (c_proj, c_fc)


@pytest.mark.parametrize("d,mlp,K,attn_auto,mlp_auto,mode4,per_linear", [
    (768, 3072, 50432, ("group", 7), "each", 7, (28, 9, 7, 7)),             # ViT-B/16, B = 256
    (1024, 4096, 65792, "each", "each", 4, (16, 5, 4, 4)),                  # ViT-L/14
    (512, 2048, 19712, ("group", 16), ("group", 8), None, (32, 21, 16, 16)),  # CLIP text tower
])
def test_wgrad_plan_per_shape(d, mlp, K, attn_auto, mlp_auto, mode4, per_linear):
    attn, mlp_ = _branches(d, mlp)
    each = {"attn": ("each", list(per_linear[:2])), "mlp": ("each", list(per_linear[2:]))}
    for branch, shapes, want in (("attn", attn, attn_auto), ("mlp", mlp_, mlp_auto)):
        assert wgrad_plan("auto", branch, shapes, K) == (each[branch] if want == "each" else want)
        assert wgrad_plan("0", branch, shapes, K) == each[branch]
    assert wgrad_plan("1", "mlp", mlp_, K) == each["mlp"] and wgrad_plan("1", "attn", attn, K)[0] == "group"
    if mode4 is not None:
        assert wgrad_plan("4", "block", mlp_ + attn, K) == ("group", mode4)


def test_wgrad_plan_modes_2_and_3_group_both_branches():
    attn, mlp_ = _branches(768, 3072)
    assert wgrad_plan("2", "attn", attn, 50432) == ("group", 7) and wgrad_plan("2", "mlp", mlp_, 50432) == ("group", 7)
    assert wgrad_plan("3", "attn", attn, 50432) == ("group", 7) and wgrad_plan("3", "mlp", mlp_, 50432) == ("group", 3)


def test_class_token_launches_are_never_grouped_or_split():
    for mode in ("auto", "0", "1", "2", "3", "4"):
        assert wgrad_plan(mode, "cls", [(768, 3072), (3072, 768)], 1024) == ("each", [1, 1])
