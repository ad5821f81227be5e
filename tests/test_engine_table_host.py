"""CPU: the named slots of the backbone's pointer tables (ucod_dpl_amd/native.py) against the numbers include/ucod_dpl.h gives them, and the one builder of a layer's
row (vit_engine.layer_row) on CPU tensors with identity conversions."""
import os
import re

import pytest
import torch

from conftest import ROOT
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import layer_row

VECTORS = ("ln1_g", "ln1_b", "qkv_b", "proj_b", "ls1", "ln2_g", "ln2_b", "fc1_b", "fc2_b", "ls2")


def test_slot_names_sit_at_the_numbers_of_the_header():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert int(re.search(r"#define UCOD_VIT_LAYER_STRIDE (\d+)", header).group(1)) == N.VIT_LAYER_STRIDE == len(N.VIT_LAYER_SLOTS) == 16
    assert int(re.search(r"#define UCOD_VIT_TRAIN_STRIDE (\d+)", header).group(1)) == N.VIT_TRAIN_STRIDE == len(N.VIT_TRAIN_SLOTS) == 7
    # include/ucod_dpl.h, ucod_vit_forward: "+0 ln1_g +1 ln1_b +2 qkv_w +3 qkv_b +4 proj_w +5 proj_b +6 ls1 +7 ln2_g +8 ln2_b +9 fc1_w +10 fc1_b +11 fc2_w +12 fc2_b +13 ls2
    # +14 qkv_colsum +15 fc1_colsum"; ucod_vit_forward_split: "+14 the K rows of qkv_w as an A-side operand"
    numbers = dict(ln1_g=0, ln1_b=1, qkv_w=2, qkv_b=3, proj_w=4, proj_b=5, ls1=6, ln2_g=7, ln2_b=8, fc1_w=9, fc1_b=10, fc2_w=11, fc2_b=12, ls2=13)
    assert len(set(N.VIT_LAYER_SLOTS)) == 16
    for name, at in numbers.items():
        assert N.VIT_LAYER_SLOTS[at] == name and getattr(N, name.upper()) == at, name
        assert re.search(rf"\+{at} {name}\b", header), (name, at)         # the header says so in these words
    assert (N.AUX0, N.AUX1) == (14, 15)
    assert (N.QKV_COLSUM, N.FC1_COLSUM) == (14, 15) and (N.KEY_ROWS_A, N.SPLIT_UNUSED) == (14, 15)      # both meanings of each
    assert re.search(r"\+14 qkv_colsum \[3D\]\s+\+15 fc1_colsum", header) and re.search(r"\+14 the K rows of qkv_w as an A-side operand", header)
    # ucod_vit_forward_train: "+0 qkv_w_aug +1 qkv_wT_aug +2 proj_w^T +3 fc1_w^T +4 fc2_w^T +5 LoRA parameters +6 LoRA gradients"
    assert N.VIT_TRAIN_SLOTS == ("qkv_w_aug", "qkv_wt_aug", "proj_wt", "fc1_wt", "fc2_wt", "lora", "lora_grad")
    assert (N.T_QKV_W_AUG, N.T_QKV_WT_AUG, N.T_PROJ_WT, N.T_FC1_WT, N.T_FC2_WT, N.T_LORA, N.T_LORA_GRAD) == (0, 1, 2, 3, 4, 5, 6)
    for at, words in enumerate((r"qkv_w_aug", r"qkv_wT_aug", r"proj_w\^T", r"fc1_w\^T", r"fc2_w\^T", r"LoRA parameters", r"LoRA gradients")):
        assert re.search(rf"\+{at} {words}", header), (at, words)


def canonical_layer(D=8, F=16, layer_scale=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(ln1_g=r(D), ln1_b=r(D), qkv_w=r(3 * D, D), qkv_b=r(3 * D), proj_w=r(D, D), proj_b=r(D), ls1=r(D) if layer_scale else None,
                ln2_g=r(D), ln2_b=r(D), fc1_w=r(F, D), fc1_b=r(F), fc2_w=r(D, F), fc2_b=r(D), ls2=r(D) if layer_scale else None)


def identity(t, name=None):
    return t


def test_row_without_scales_is_the_source_tensors_in_table_order():
    l = canonical_layer()
    seen = []
    row = layer_row(l, lambda t, name: seen.append(name) or t, identity)
    assert len(row) == N.VIT_LAYER_STRIDE and row[N.AUX0] is None and row[N.AUX1] is None
    for at, name in enumerate(N.VIT_LAYER_SLOTS[:14]):
        assert row[at] is l[name], name                               # the very tensors: nothing is multiplied without scales
    assert seen == ["qkv_w", "proj_w", "fc1_w", "fc2_w"]              # the weight conversion sees the four matrices, by name, and nothing else
    # a checkpoint without LayerScale (DINOv1): ones of the model width, through the vector conversion
    l1 = canonical_layer(layer_scale=False)
    row1 = layer_row(l1, identity, lambda t: t.double())
    for at in (N.LS1, N.LS2):
        assert torch.equal(row1[at], torch.ones(8, dtype=torch.float64))
    for name in VECTORS:
        assert row1[N.VIT_LAYER_SLOTS.index(name)].dtype == torch.float64
    for name in ("qkv_w", "proj_w", "fc1_w", "fc2_w"):
        assert row1[N.VIT_LAYER_SLOTS.index(name)] is l1[name]


@pytest.mark.parametrize("layer_scale", [True, False])
def test_row_with_scales_multiplies_the_biases_and_divides_the_layer_scales(layer_scale):
    l = canonical_layer(layer_scale=layer_scale, seed=1)
    S = dict(qkv=2.0 ** 20, proj=2.0 ** 17, fc1=2.0 ** 21, fc2=2.0 ** 9)                 # powers of two: every product below is exact
    a0, a1 = torch.zeros(3), torch.zeros(5)
    row = layer_row(l, identity, identity, scales=(S["qkv"], S["proj"], S["fc1"], S["fc2"]), aux=(a0, a1))
    assert len(row) == N.VIT_LAYER_STRIDE and row[N.AUX0] is a0 and row[N.AUX1] is a1       # the aux slots hold what the caller passed
    ones = torch.ones(8)
    want = {N.QKV_B: l["qkv_b"] * S["qkv"], N.PROJ_B: l["proj_b"] * S["proj"], N.FC1_B: l["fc1_b"] * S["fc1"], N.FC2_B: l["fc2_b"] * S["fc2"],
            N.LS1: (l["ls1"] if layer_scale else ones) / S["proj"], N.LS2: (l["ls2"] if layer_scale else ones) / S["fc2"]}
    for at, name in enumerate(N.VIT_LAYER_SLOTS[:14]):
        if at in want:
            assert torch.equal(row[at], want[at]) and not torch.equal(row[at], want[at] * 2), name
        else:
            assert torch.equal(row[at], l[name]) and row[at] is l[name], name                # everything else untouched
