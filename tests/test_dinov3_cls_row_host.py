"""CPU: the host side of the CLS attention row on DINOv3 (``forward_with_cls_attention(img, allow_rope=True)``, ucod_cls_attention_rope) -- the f64 restatement
tests/dinov3_cls_row_ref.py against the G25 goldens recorded from transformers (tests/golden/make_golden_dinov3_cls_row.py), the stored fault distances, the
regrouped score formula against ``dinov3_ref.rotate``, and the surface: the keyword, the refusal's message, the symbol."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine
from ucod_dpl_amd.generate_pseudo_label import PseudoLabelGenerator
import dinov3_ref as R3
import dinov3_cls_row_ref as C3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = sorted(R3.G22)


@functools.lru_cache(maxsize=None)
def golden(tag):
    z = np.load(os.path.join(GOLDEN, C3.GOLDEN_NAME.format(tag=tag)))
    sd = R3.g22_state_dict(tag)
    return z, sd, R3.g22_input(tag)


@functools.lru_cache(maxsize=None)
def restated(tag):
    z, sd, x = golden(tag)
    return C3.forward_f64(x, sd, R3.G22[tag]["heads"])


@pytest.mark.parametrize("tag", TAGS)
def test_weights_are_the_goldens(tag):
    z, sd, _ = golden(tag)
    m = R3.G22[tag]
    assert R3.weights_sha256(sd) == str(z["sd_sha256"]), "random_dinov3_state_dict no longer draws the weights the goldens were made with"
    g22 = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    assert str(g22["sd_sha256"]) == str(z["sd_sha256"]) and int(z["n_reg"]) == m["R"]
    n = m["grid"][0] * m["grid"][1]
    assert z["att"].shape == (R3.G22_B, m["heads"], n) and z["lead"].shape == (R3.G22_B, m["heads"], 1 + m["R"]) and z["att"].dtype == np.float64
    assert np.abs(z["att"].sum(-1) + z["lead"].sum(-1) - 1).max() < 1e-14          # one softmax row


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_g25_goldens(tag):
    z, _, _ = golden(tag)
    key, att, lead = restated(tag)
    assert R3.rel_l2(att, torch.from_numpy(z["att"])) < 1e-10 and R3.rel_l2(lead, torch.from_numpy(z["lead"])) < 1e-10
    g22 = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    assert R3.rel_l2(key, torch.from_numpy(g22["key"])) < 1e-10


@pytest.mark.parametrize("tag", TAGS)
def test_each_fault_lands_at_its_stored_distance_and_above_its_floor(tag):
    z, sd, x = golden(tag)
    m = R3.G22[tag]
    assert {k[6:] for k in z.files if k.startswith("fault_")} == set(C3.faults_for(m["R"]))
    widest = C3.widest_bound(tag, z)
    for f in C3.faults_for(m["R"]):
        d = R3.rel_l2(C3.forward_f64(x, sd, m["heads"], fault=f)[1], torch.from_numpy(z["att"]))
        want = float(z["fault_" + f])
        assert abs(d - want) <= 1e-6 * want, (f, d, want)
        assert want >= C3.fault_floor(tag, f, z), (f, want)
        assert ((tag, f) in C3.UNDER_TEN_WIDEST) == (want < 10 * widest), (f, want, widest)     # the list of exceptions is exactly the pairs that miss 10 x widest


def test_the_issue_figures_on_g46():
    """transformers' own error on the row, and the fault that is today's kernel, as the feature's issue recorded them"""
    z, _, _ = golden("g46")
    assert 7e-7 < float(z["err_f32"]) < 9e-7 and 8.6e-4 < float(z["err_f16ac"]) < 1.1e-3 and 7.5e-3 < float(z["err_bf16ac"]) < 1.2e-2
    assert 0.72 < float(z["fault_unrotated_keys"]) < 0.74 and 1.03 < float(z["fault_sin_sign"]) < 1.05


@pytest.mark.parametrize("tag", TAGS)
def test_the_regrouped_formula_is_the_rotation(tag):
    """cls_row (what the kernel evaluates: no rotated key is formed) against the model's own order -- rotate the keys with dinov3_ref.rotate, then one product"""
    _, sd, x = golden(tag)
    m = R3.G22[tag]
    q, k_lead, key, tab = C3.last_layer_operands_f64(x, sd, m["heads"])
    att, lead = C3.cls_row(q, k_lead, key, tab, m["heads"])
    _, att_m, lead_m = restated(tag)
    assert float((att - att_m).abs().max()) < 1e-14 and float((lead - lead_m).abs().max()) < 1e-14
    # and on the scores themselves, on random operands
    g = torch.Generator().manual_seed(7)
    B, heads, hw = 2, 2, 35
    qr, kr = torch.randn(B, heads * 64, generator=g, dtype=torch.float64), torch.randn(B, heads * 64, hw, generator=g, dtype=torch.float64)
    t = C3.table(5, 7)
    rot = R3.rotate(kr.reshape(B, heads, 64, hw).permute(0, 3, 1, 2), t[:, :32], t[:, 32:])                  # [B, hw, heads, 64]
    want = torch.softmax(torch.cat((torch.zeros(B, heads, 1, dtype=torch.float64), torch.einsum("bhd,bjhd->bhj", qr.reshape(B, heads, 64), rot) * 0.125), -1), -1)
    got, _ = C3.cls_row(qr, torch.zeros(B, 1, heads * 64, dtype=torch.float64), kr, t, heads)
    assert float((got - want[..., 1:]).abs().max()) < 1e-14
    ident = torch.cat((torch.ones(hw, 32), torch.zeros(hw, 32)), 1)
    assert torch.equal(C3.cls_row(qr, torch.zeros(B, 1, heads * 64, dtype=torch.float64), kr, ident, heads)[0].float(),
                       C3.cls_row(qr, torch.zeros(B, 1, heads * 64, dtype=torch.float64), kr, None, heads)[0].float())


@pytest.mark.parametrize("tag", C3.GENERATOR_TAGS)
def test_generator_fields(tag):
    z, _, _ = golden(tag)
    gh, gw = R3.G22[tag]["grid"]
    th, row, mask = float(z["th"]), z["cos_row"], z["mask"]
    assert row.shape == mask.shape == (R3.G22_B, gh, gw)
    assert np.array_equal(mask, (row > th).astype(np.float64)) and 0.1 <= mask.mean() <= 0.9
    assert (np.abs(row - th) > 1e-5).mean() >= 0.95
    g22 = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    own_mask, own_row = C3.bkg_seg(torch.from_numpy(z["att"]), torch.from_numpy(g22["key"]), th)
    assert np.array_equal(own_mask.numpy(), mask) and np.abs(own_row.numpy() - row).max() < 1e-14


def test_allow_rope_is_a_keyword_with_default_false():
    for fn in (PseudoLabelGenerator.__init__, ViTEngine.forward_with_cls_attention, SplitViTEngine.forward_with_cls_attention):
        p = inspect.signature(fn).parameters["allow_rope"]
        assert p.default is False and p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD


@pytest.mark.parametrize("cls", [ViTEngine, SplitViTEngine])
def test_the_refusal_names_the_keyword(cls):
    eng = object.__new__(cls)
    eng.rope = True
    for kw in ({}, dict(allow_rope=False)):
        with pytest.raises(NotImplementedError, match="DINOv3.*RoPE") as e:
            eng.forward_with_cls_attention(torch.zeros(1, 3, 32, 32), **kw)
        assert "allow_rope=True" in str(e.value) and "ROTATED patch keys" in str(e.value)


def test_the_generator_hands_the_flag_on():
    class Engine:
        device = "cpu"

        def forward_with_cls_attention(self, img, allow_rope=False):
            raise KeyError(allow_rope)

    for flag in (False, True):
        gen = PseudoLabelGenerator(Engine(), allow_rope=flag)
        assert gen.allow_rope is flag
        with pytest.raises(KeyError, match=str(flag)):
            gen.raw_masks(torch.zeros(1, 3, 32, 32))


def test_the_symbol():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert re.search(r"int ucod_cls_attention_rope\(const float\* q_cls, const float\* k_lead, const float\* key_map, const float\* cos_sin, float\* att, int B, "
                     r"int heads, int hw, int n_reg,\s+float scale, void\* stream\);", header)
    assert "#define UCOD_ABI_VERSION 5" in header and N.ABI_VERSION == 5
    assert len(N.SIGNATURES["ucod_cls_attention_rope"][1]) == len(N.SIGNATURES["ucod_cls_attention_reg"][1]) + 1
    for half in ("bf16", "f16"):
        lib = N.load(half)
        assert hasattr(lib, "ucod_cls_attention_rope")
        p = 4096                                                 # argument validation runs before any launch: no pointer is followed
        assert lib.ucod_cls_attention_rope(p, p, p, None, p, 1, 2, 24, 4, 0.125, None) == -1
        assert lib.ucod_cls_attention_rope(None, p, p, p, p, 1, 2, 24, 4, 0.125, None) == -1
        assert lib.ucod_cls_attention_rope(p, p, p, p, p, 1, 2, 12001, 4, 0.125, None) == -1
        assert lib.ucod_cls_attention_rope(p, p, p, p, p, 1, 2, 24, 1024, 0.125, None) == -1
        assert lib.ucod_cls_attention_rope(p, p, p, p + 4, p, 1, 2, 24, 4, 0.125, None) == -1
