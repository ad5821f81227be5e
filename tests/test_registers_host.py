"""CPU: the host side of DINOv2 with registers (HF Dinov2WithRegistersModel) -- the restatement tests/registers_ref.py against the G21 goldens recorded from
transformers (tests/golden/make_golden_registers.py), the proof that those goldens tell a dropped register / a missing antialias apart, checkpoint normalisation,
the architecture table and the config.json cross-check."""
import json
import os

import numpy as np
import pytest
import torch

from ucod_dpl_amd.vit_engine import normalize_state_dict, _interp_pos_dinov2
from ucod_dpl_amd.data.utils import feature_extractor as FE
import registers_ref as RR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# the bound tests/test_swiglu_host.py holds its restatement to against G20 (f32 restatement vs transformers' f32)
KEY_TOL, ATT_TOL = dict(rtol=1e-5, atol=1e-5), dict(rtol=1e-5, atol=1e-6)


def golden(tag):
    z = np.load(os.path.join(GOLDEN, f"g21_dinov2_registers_{tag}.npz"))
    sd = RR.g21_state_dict(tag)
    assert RR.weights_sha256(sd) == str(z["sd_sha256"]), "random_registers_state_dict no longer draws the weights the goldens were made with"
    (H, W), pre, R = RR.G21[tag]
    assert int(z["image_size"]) == pre and int(z["n_reg"]) == R and z["x"].shape == (RR.G21_B, 3, H, W)
    return z, sd


def excess(got, ref, rtol, atol):
    """the largest |got - ref| in units of the bound atol + rtol |ref| (<= 1: inside)"""
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


@pytest.mark.parametrize("tag", sorted(RR.G21))
def test_restatement_matches_the_g21_goldens(tag):
    z, sd = golden(tag)
    R = RR.G21[tag][2]
    last, key, att = RR.forward(torch.from_numpy(z["x"]), sd, heads=RR.G21_HEADS)
    gh, gw = z["x"].shape[2] // 14, z["x"].shape[3] // 14
    assert key.shape == (RR.G21_B, RR.G21_D, gh, gw) and last.shape == (RR.G21_B, 1 + R + gh * gw, RR.G21_D) and att.shape == (RR.G21_B, RR.G21_HEADS, gh * gw)
    torch.testing.assert_close(key, torch.from_numpy(z["key"]), **KEY_TOL)
    torch.testing.assert_close(last, torch.from_numpy(z["last_hidden_state"]), **KEY_TOL)
    torch.testing.assert_close(att, torch.from_numpy(z["cls_att"]), **ATT_TOL)
    # the patch columns do not sum to one: CLS and the registers hold the rest of the softmax
    assert float(att.sum(-1).max()) < 1.0


@pytest.mark.parametrize("tag", sorted(RR.G21))
def test_the_pin_tells_a_dropped_register_apart(tag):
    z, sd = golden(tag)
    _, key, att = RR.forward(torch.from_numpy(z["x"]), sd, heads=RR.G21_HEADS, drop_registers=True)
    assert excess(key, torch.from_numpy(z["key"]), **KEY_TOL) >= 100.0
    assert excess(att, torch.from_numpy(z["cls_att"]), **ATT_TOL) >= 100.0


def test_the_pin_tells_a_missing_antialias_apart():
    z, sd = golden("down")
    _, key, att = RR.forward(torch.from_numpy(z["x"]), sd, heads=RR.G21_HEADS, antialias=False)
    assert excess(key, torch.from_numpy(z["key"]), **KEY_TOL) >= 100.0
    # (measured while writing this: the upsampled grid tells the flag apart as well -- torch's antialiased bicubic kernel has a = -0.5, the plain one a = -0.75 --
    # so the flag matters on EVERY interpolated grid, not only where the target is smaller; the native grid interpolates nothing)
    z, sd = golden("native")
    _, key_n, _ = RR.forward(torch.from_numpy(z["x"]), sd, heads=RR.G21_HEADS, antialias=False)
    torch.testing.assert_close(key_n, torch.from_numpy(z["key"]), **KEY_TOL)


def test_the_engines_position_builder_takes_the_flag():
    pos = RR.g21_state_dict("down")["embeddings.position_embeddings"]
    assert torch.equal(_interp_pos_dinov2(pos, 5, 5, antialias=True), RR.pos_embed(pos, 5, 5, True))
    assert torch.equal(_interp_pos_dinov2(pos, 5, 5), RR.pos_embed(pos, 5, 5, False))
    assert not torch.equal(_interp_pos_dinov2(pos, 5, 5, antialias=True), _interp_pos_dinov2(pos, 5, 5))


def test_normalize_state_dict_returns_the_registers():
    sd = RR.g21_state_dict("native")
    c = normalize_state_dict(sd)
    assert c["kind"] == "dinov2" and c["pos_antialias"] is True
    assert tuple(c["reg"].shape) == (4, 128) and torch.equal(c["reg"], sd["embeddings.register_tokens"][0])
    assert float(c["reg"].abs().max()) > 0.1
    c1 = normalize_state_dict(RR.g21_state_dict("r1"))
    assert tuple(c1["reg"].shape) == (1, 128)
    # the "dinov2." prefix of a task-model checkpoint
    cp = normalize_state_dict({"dinov2." + k: v for k, v in sd.items()})
    assert torch.equal(cp["reg"], c["reg"])
    # R = 0 written as an empty tensor
    sd0 = dict(sd)
    sd0["embeddings.register_tokens"] = torch.zeros(1, 0, 128)
    c0 = normalize_state_dict(sd0)
    assert c0["reg"] is None and c0["pos_antialias"] is True
    # a plain DINOv2 dict: no trace of either entry (R = 0, no antialias)
    plain = normalize_state_dict({k: v for k, v in sd.items() if "register_tokens" not in k})
    assert plain.get("reg") is None and not plain.get("pos_antialias", False)
    with pytest.raises(ValueError, match="register_tokens"):
        normalize_state_dict(dict(sd, **{"embeddings.register_tokens": torch.zeros(1, 4, 64)}))


def test_dinov1_with_registers_raises():
    sd = {k: v for k, v in RR.g21_state_dict("native").items() if "layer_scale" not in k}      # an HF ViTModel-like dict (no LayerScale) is DINOv1 here
    with pytest.raises(ValueError, match="DINOv1"):
        normalize_state_dict(sd)
    from conftest import load_golden, sub
    v1 = sub(load_golden("g8_dinov1_native"), "sd.")
    assert "cls_token" in v1                                     # the in-repo VisionTransformer layout
    with pytest.raises(ValueError, match="DINOv1"):
        normalize_state_dict(dict(v1, register_tokens=torch.zeros(1, 4, v1["cls_token"].shape[-1])))


def test_register_archs():
    assert FE.REGISTER_ARCHS == {f"dinov2_vit{s}14_reg": 4 for s in "sblg"}
    for name, R in FE.REGISTER_ARCHS.items():
        assert len(FE.ARCHS[name]) == 6 and FE.ARCHS[name] == FE.ARCHS[name[:-4]]
    for size, s in (("small", "s"), ("base", "b"), ("large", "l"), ("giant", "g")):
        assert FE.HUB_TO_ARCH[f"facebook/dinov2-with-registers-{size}"] == f"dinov2_vit{s}14_reg"
    assert "dinov2_vitg14_reg" in FE.SWIGLU_ARCHS and "dinov2_vitb14_reg" not in FE.SWIGLU_ARCHS
    sd = FE.random_state_dict("dinov2_vits14_reg", seed=3, image_size=70)
    reg = sd["embeddings.register_tokens"]
    assert tuple(reg.shape) == (1, 4, 384)
    assert float((reg != 0).float().mean()) > 0.99               # drawn, not HF's zeros
    plain = FE.random_state_dict("dinov2_vits14", seed=3, image_size=70)
    assert all(torch.equal(sd[k], v) for k, v in plain.items())   # the plain sibling's draws are untouched
    tl = FE.trained_like_state_dict("dinov2_vits14_reg", seed=3, image_size=70)
    assert float(tl["embeddings.register_tokens"].abs().max()) > 0.0
    meta = FE.random_state_dict("dinov2_vitg14_reg", device="meta")
    assert all(v.device.type == "meta" for v in meta.values())
    assert tuple(meta["embeddings.register_tokens"].shape) == (1, 4, 1536) and "encoder.layer.39.mlp.weights_in.weight" in meta


def test_register_arch_matches_the_hf_layout():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Dinov2WithRegistersConfig(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, image_size=518, patch_size=14, mlp_ratio=4,
                                                 num_register_tokens=4)
    with torch.device("meta"):
        hf = transformers.Dinov2WithRegistersModel(cfg)
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if k != "embeddings.mask_token"}
    got = {k: tuple(v.shape) for k, v in FE.random_state_dict("dinov2_vitb14_reg", device="meta").items()}
    assert got == want


@pytest.mark.parametrize("said", [0, 1, 8])
def test_config_json_register_count_mismatch_raises(tmp_path, said):
    from ucod_dpl_amd.engine.config import CfgNode
    sd = RR.g21_state_dict("native")
    torch.save(sd, tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="dinov2_with_registers", num_attention_heads=2, num_register_tokens=said)))
    cfg = CfgNode(dict(backbone_type="huggingface", type="dinov2", backbone="facebook/dinov2-with-registers-small", backbone_weights=str(tmp_path)))
    with pytest.raises(ValueError, match="num_register_tokens"):
        FE.backbone(cfg, device="cpu")


def test_config_json_without_the_key_means_the_hf_default_of_four(tmp_path):
    """model_type "dinov2_with_registers" without num_register_tokens is 4 registers (Dinov2WithRegistersConfig's default): a checkpoint beside it that has no
    embeddings.register_tokens must not load as plain DINOv2."""
    from ucod_dpl_amd.engine.config import CfgNode
    sd = {k: v for k, v in RR.g21_state_dict("native").items() if "register_tokens" not in k}
    torch.save(sd, tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="dinov2_with_registers", num_attention_heads=2)))
    cfg = CfgNode(dict(backbone_type="huggingface", type="dinov2", backbone="facebook/dinov2-with-registers-small", backbone_weights=str(tmp_path)))
    with pytest.raises(ValueError, match="num_register_tokens = 4"):
        FE.backbone(cfg, device="cpu")
