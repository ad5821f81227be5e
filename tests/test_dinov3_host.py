"""CPU: the host side of DINOv3 (HF DINOv3ViTModel: rotary position embedding on the patch tokens' q and k) -- the f64 restatement tests/dinov3_ref.py against the
G22 goldens recorded from transformers (tests/golden/make_golden_dinov3.py), the proof that those goldens tell each fault of a rotary pass apart and that every
engine bound of tests/test_gpu_dinov3.py lies under half the smallest fault, checkpoint normalisation, the rotary table, the architecture table, the refusals and
the new symbol."""
import os
import math
import re

import numpy as np
import pytest
import torch

from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import normalize_state_dict, rope_table, is_dinov3, ViTEngine, SplitViTEngine, ViTLoRAEngine
from ucod_dpl_amd.data.utils import feature_extractor as FE
import dinov3_ref as R3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(tag):
    z = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    sd = R3.g22_state_dict(tag)
    assert R3.weights_sha256(sd) == str(z["sd_sha256"]), "random_dinov3_state_dict no longer draws the weights the goldens were made with"
    gh, gw = R3.G22[tag]["grid"]
    assert int(z["n_reg"]) == R3.G22[tag]["R"] and z["x"].shape == (R3.G22_B, 3, 16 * gh, 16 * gw) and z["key"].dtype == np.float64
    assert np.array_equal(z["x"], R3.g22_input(tag).numpy())
    return z, sd


@pytest.mark.parametrize("tag", sorted(R3.G22))
def test_restatement_matches_the_g22_goldens(tag):
    z, sd = golden(tag)
    key = R3.forward_f64(torch.from_numpy(z["x"]), sd, R3.G22[tag]["heads"])
    assert key.shape == z["key"].shape
    assert R3.rel_l2(key, torch.from_numpy(z["key"])) < 1e-10


@pytest.mark.parametrize("fault", R3.FAULTS)
@pytest.mark.parametrize("tag", sorted(R3.G22))
def test_each_fault_lands_at_its_stored_distance(tag, fault):
    z, sd = golden(tag)
    d = R3.rel_l2(R3.forward_f64(torch.from_numpy(z["x"]), sd, R3.G22[tag]["heads"], fault=fault), torch.from_numpy(z["key"]))
    want = float(z["fault_" + fault])
    assert abs(d - want) <= 0.1 * want, (d, want)


@pytest.mark.parametrize("precision,tag", R3.ENGINE_ROWS)
def test_every_engine_bound_is_under_half_the_smallest_fault(precision, tag):
    """A condition, not a measurement: a pass with one of the four faults is at least the fault's distance minus the engine's own error away from the golden, so with
    bound < (smallest fault) / 2 it cannot stay inside the bound.  (bf16 meets it on the D = 256 golden only, which is where its row runs.)"""
    z = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    smallest = min(float(z["fault_" + f]) for f in R3.FAULTS)
    assert R3.engine_bound(precision, z) < 0.5 * smallest, (precision, tag, R3.engine_bound(precision, z), smallest)


def test_the_engine_rows_cover_every_golden_and_engine():
    for tag in R3.G22:
        for p in R3.SPLIT_ROWS + R3.F16_ROWS:
            assert (p, tag) in R3.ENGINE_ROWS
    assert ("bf16", "d256") in R3.ENGINE_ROWS and ("f16_fold", "d256") in R3.ENGINE_ROWS
    # fp16 and the split rows hold the condition on every golden; bf16 does not at D = 128 (why its row is the D = 256 one)
    z = np.load(os.path.join(GOLDEN, "g22_dinov3_g46.npz"))
    assert R3.engine_bound("bf16", z) > 0.5 * min(float(z["fault_" + f]) for f in R3.FAULTS)


def hf_model(**kw):
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "DINOv3ViTModel"):
        pytest.skip("this transformers has no DINOv3ViTModel")
    cfg = transformers.DINOv3ViTConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=16, num_register_tokens=4, **kw)
    torch.manual_seed(3)
    return transformers.DINOv3ViTModel(cfg).eval()


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("prefix", ["model.layer.", "layer."])
def test_normalize_state_dict_on_a_real_dinov3_model(prefix, gated):
    m = hf_model(intermediate_size=384, use_gated_mlp=gated, hidden_act="silu" if gated else "gelu")
    with torch.no_grad():
        m.embeddings.register_tokens.normal_()
    sd = {k.replace("model.layer.", prefix): v for k, v in m.state_dict().items()}
    assert is_dinov3(sd) and not any("k_proj.bias" in k for k in sd)
    c = normalize_state_dict(sd)
    assert c["kind"] == "dinov3" and c["rope"] is True and c["pos"] is None and len(c["layers"]) == 2
    assert torch.equal(c["reg"], sd["embeddings.register_tokens"][0]) and tuple(c["reg"].shape) == (4, 128)
    assert torch.equal(c["patch_w"], sd["embeddings.patch_embeddings.weight"]) and torch.equal(c["cls"], sd["embeddings.cls_token"].reshape(-1))
    for i, l in enumerate(c["layers"]):
        p = f"{prefix}{i}."
        assert tuple(l["qkv_w"].shape) == (384, 128) and torch.equal(l["qkv_w"][128:256], sd[p + "attention.k_proj.weight"])
        assert torch.equal(l["qkv_b"][:128], sd[p + "attention.q_proj.bias"]) and torch.equal(l["qkv_b"][256:], sd[p + "attention.v_proj.bias"])
        assert bool((l["qkv_b"][128:256] == 0).all())           # k_proj has no bias
        assert torch.equal(l["ls1"], sd[p + "layer_scale1.lambda1"]) and torch.equal(l["fc2_w"], sd[p + "mlp.down_proj.weight"])
        if gated:
            assert c["mlp"] == "swiglu" and tuple(l["fc1_w"].shape) == (768, 128)
            assert torch.equal(l["fc1_w"][:384], sd[p + "mlp.gate_proj.weight"]) and torch.equal(l["fc1_w"][384:], sd[p + "mlp.up_proj.weight"])     # gate rows first
            assert torch.equal(l["fc1_b"], torch.cat((sd[p + "mlp.gate_proj.bias"], sd[p + "mlp.up_proj.bias"])))
        else:
            assert "mlp" not in c and torch.equal(l["fc1_w"], sd[p + "mlp.up_proj.weight"])
    # a missing bias anywhere is zeros; R = 0 is reg None; a DINOv2 dict is not DINOv3
    sd2 = {k: v for k, v in sd.items() if not k.endswith("o_proj.bias")}
    sd2["embeddings.register_tokens"] = torch.zeros(1, 0, 128)
    c2 = normalize_state_dict(sd2)
    assert c2["reg"] is None and bool((c2["layers"][0]["proj_b"] == 0).all())
    assert not is_dinov3(FE.random_state_dict("dinov2_vits14_reg", device="meta"))


@pytest.mark.parametrize("gh,gw", [(4, 6), (6, 4), (14, 14), (32, 32)])
def test_rope_table_is_the_models_table_bit_for_bit(gh, gw):
    m = hf_model()
    cos, sin = m.rope_embeddings(torch.zeros(1, 3, 16 * gh, 16 * gw))
    t = rope_table(gh, gw, theta=100.0)
    assert t.dtype == torch.float32 and tuple(t.shape) == (gh * gw, 64) and t.is_contiguous()
    assert torch.equal(t[:, :32], cos[:, :32]) and torch.equal(t[:, 32:], sin[:, :32])
    assert torch.equal(cos[:, 32:], cos[:, :32]) and torch.equal(sin[:, 32:], sin[:, :32])      # the tiled duplicate that is not stored
    c, s = R3.cos_sin(gh, gw)                                    # the reference's own builder agrees
    assert torch.equal(t[:, :32], c) and torch.equal(t[:, 32:], s)
    assert not torch.equal(rope_table(gh, gw, theta=10.0), t)


def test_dinov3_archs():
    want = {"dinov3_vits16": (384, 6, 12, 16, 224), "dinov3_vitb16": (768, 12, 12, 16, 224), "dinov3_vitl16": (1024, 16, 24, 16, 224),
            "dinov3_vits16plus": (384, 6, 12, 16, 224), "dinov3_vith16plus": (1280, 20, 32, 16, 224)}
    for name, tup in want.items():
        assert FE.ARCHS[name][:5] == tup and len(FE.ARCHS[name]) == 6 and FE.DINOV3_ARCHS[name] == 4
        assert (name in FE.SWIGLU_ARCHS) == name.endswith("plus")
    assert not any("7b" in k for k in FE.ARCHS)                  # head dimension 128: not built
    for size in ("vits16", "vits16plus", "vitb16", "vitl16", "vith16plus"):
        assert FE.HUB_TO_ARCH[f"facebook/dinov3-{size}-pretrain-lvd1689m"] == "dinov3_" + size
    meta = FE.random_state_dict("dinov3_vits16plus", device="meta")
    assert all(v.device.type == "meta" for v in meta.values())
    assert tuple(meta["embeddings.register_tokens"].shape) == (1, 4, 384) and tuple(meta["embeddings.patch_embeddings.weight"].shape) == (384, 3, 16, 16)
    assert tuple(meta["model.layer.11.mlp.gate_proj.weight"].shape) == (1536, 384) and tuple(meta["model.layer.11.mlp.down_proj.weight"].shape) == (384, 1536)
    assert "model.layer.0.attention.k_proj.bias" not in meta and "embeddings.position_embeddings" not in meta
    big = FE.random_state_dict("dinov3_vith16plus", device="meta")
    assert tuple(big["model.layer.31.mlp.up_proj.weight"].shape) == (5120, 1280)


def test_random_state_dict_matches_the_hf_layout():
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "DINOv3ViTModel"):
        pytest.skip("this transformers has no DINOv3ViTModel")
    for arch, gated in (("dinov3_vits16", False), ("dinov3_vits16plus", True)):
        cfg = transformers.DINOv3ViTConfig(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, intermediate_size=1536, num_register_tokens=4,
                                           use_gated_mlp=gated, hidden_act="silu" if gated else "gelu")
        with torch.device("meta"):
            hf = transformers.DINOv3ViTModel(cfg)
        want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if k != "embeddings.mask_token"}
        got = {k: tuple(v.shape) for k, v in FE.random_state_dict(arch, device="meta").items()}
        assert got == want


def test_random_and_trained_like_weights():
    sd = FE.random_state_dict("dinov3_vits16", seed=3)
    reg = sd["embeddings.register_tokens"]
    assert float((reg != 0).float().mean()) > 0.99               # drawn, not zeros
    c = normalize_state_dict(sd)
    assert c["rope"] and tuple(c["reg"].shape) == (4, 384) and c["layers"][0]["fc1_w"].shape[0] == 1536
    tl = FE.trained_like_state_dict("dinov3_vits16", seed=3)
    assert torch.equal(tl["model.layer.0.attention.k_proj.weight"], 4.0 * sd["model.layer.0.attention.k_proj.weight"])
    assert torch.equal(tl["model.layer.0.attention.q_proj.bias"], 4.0 * sd["model.layer.0.attention.q_proj.bias"])
    assert float(tl["model.layer.3.layer_scale1.lambda1"].max()) < 1.0 and float(tl["model.layer.3.layer_scale1.lambda1"].min()) >= 0.1
    # no position table: the massive channels sit in the CLS and register tokens
    assert float(tl["embeddings.cls_token"][0, 0, 5]) == 200.0 and float(tl["embeddings.register_tokens"][0, 3, 288]) == -150.0
    assert normalize_state_dict(FE.trained_like_state_dict("dinov3_vits16plus", seed=1))["mlp"] == "swiglu"


def test_lora_mode_is_refused_before_any_gpu_call():
    sd = R3.g22_state_dict("g46")
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        ViTLoRAEngine(sd, 2, device="cpu")
    from ucod_dpl_amd.models.modules.full_model import load_lora
    from ucod_dpl_amd.engine.config import CfgNode
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4)), sd, 2, device="cpu")


@pytest.mark.parametrize("cls", [ViTEngine, SplitViTEngine])
def test_cls_attention_row_is_refused_before_any_gpu_call(cls):
    """The refusal is the first statement of the method: an engine marked as a DINOv3 one raises before it looks at the image (a CPU tensor here) or the device."""
    eng = object.__new__(cls)
    eng.rope = True
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        eng.forward_with_cls_attention(torch.zeros(1, 3, 32, 32))


def test_fp8_attention_is_refused_before_any_gpu_call():
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        ViTEngine(R3.g22_state_dict("g46"), 2, device="cpu", attn_variant=8)


def test_the_new_symbol_and_descriptor_field():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert re.search(r"int ucod_rope_qk\(void\* qkv, int elem, const float\* cos_sin, int B, int tok, int n_reg, int heads, void\* stream\);", header)
    assert re.search(r"const float\* rope;", header) and "#define UCOD_ABI_VERSION 5" in header
    assert "ucod_rope_qk" in N.SIGNATURES and len(N.SIGNATURES["ucod_rope_qk"][1]) == 8
    assert N.VitDesc._fields_[-1][0] == "rope" and N.VitDesc().rope is None           # the zero-filled descriptor of every existing caller: no RoPE
    assert (N.ROPE_ELEM_HALF, N.ROPE_ELEM_F32) == (0, 1) and N.ABI_VERSION == 5
    for half in ("bf16", "f16"):
        lib = N.load(half)
        assert hasattr(lib, "ucod_rope_qk")
        # argument validation runs before any launch: a null buffer, a bad element type, no patch token left, a misaligned buffer
        assert lib.ucod_rope_qk(None, 0, None, 1, 10, 4, 2, None) == -1
        assert lib.ucod_rope_qk(4096, 2, 4096, 1, 10, 4, 2, None) == -1
        assert lib.ucod_rope_qk(4096, 0, 4096, 1, 5, 4, 2, None) == -1
        assert lib.ucod_rope_qk(4100, 0, 4096, 1, 10, 4, 2, None) == -1


def test_training_descriptors_carry_the_field():
    """VitTrainDesc embeds the descriptor: its LoRA fields sit behind the pointer, as in the header's struct."""
    import ctypes as C
    assert C.sizeof(N.VitDesc) == 80 and N.VitDesc.rope.offset == 72
    assert N.VitTrainDesc.lora_r.offset == 80


def test_the_dinov3_config_is_the_dinov2_config_with_another_backbone():
    from ucod_dpl_amd.engine.config import CfgNode
    load = lambda name: CfgNode.load_with_base(os.path.join(ROOT, "configs", "uscod", name))  # noqa: E731
    v2, v3 = load("UCOD-DPL_dinov2.py"), load("UCOD-DPL_dinov3.py")
    fe = v3["dataset_cfg"]["feature_extractor_cfg"]
    assert fe["type"] == "dinov3" and fe["backbone"] == "facebook/dinov3-vitb16-pretrain-lvd1689m" and FE.HUB_TO_ARCH[fe["backbone"]] == "dinov3_vitb16"
    assert tuple(v3["dataset_cfg"]["trainset_cfg"]["image_size"]) == (512, 512) and tuple(v3["dataset_cfg"]["valset_cfg"]["image_size"]) == (512, 512)

    def strip(t):
        t = {k: (strip(v) if isinstance(v, dict) else v) for k, v in dict(t).items()}
        for k in ("exp_name", "image_size", "type", "backbone"):
            t.pop(k, None)
        return t

    assert strip(v2) == strip(v3)


def test_from_state_dict_picks_the_checkpoints_layernorm_eps(monkeypatch):
    """backbone.from_state_dict without ``eps``: 1e-5 for a DINOv3 state dict (DINOv3ViTConfig's default), 1e-6 for every other; an explicit value is kept."""
    seen = {}

    def fake_engine(self, precision, engine_kw):
        seen["eps"] = self._src[2]
        return "f16", None

    monkeypatch.setattr(FE.backbone, "_make_engine", fake_engine)
    v3, v2 = FE.random_state_dict("dinov3_vits16", device="meta"), FE.random_state_dict("dinov2_vits14", device="meta")
    FE.backbone.from_state_dict(v3, heads=6, device="cpu")
    assert seen["eps"] == 1e-5
    FE.backbone.from_state_dict(v2, heads=6, device="cpu")
    assert seen["eps"] == 1e-6
    FE.backbone.from_state_dict(v3, heads=6, eps=1e-6, device="cpu")
    assert seen["eps"] == 1e-6


@pytest.mark.parametrize("gh,gw", [(4, 6), (6, 4), (14, 14), (32, 32)])
def test_rope_table_without_transformers(gh, gw):
    """What stays checked where transformers is missing: the table against the reference's own builder bit for bit, and against the formula in f64 -- row r gw + c
    holds cos | sin of 2 pi y theta^-(j / 16) (16 values) then 2 pi x theta^-(j / 16), y = 2 (r + 0.5) / gh - 1, x = 2 (c + 0.5) / gw - 1 -- to f32 rounding of the
    angle (|angle| <= 2 pi, so 2 pi 2^-23 suffices with room)."""
    t = rope_table(gh, gw)
    c, s = R3.cos_sin(gh, gw)
    assert torch.equal(t[:, :32], c) and torch.equal(t[:, 32:], s)
    r, cc = torch.arange(gh, dtype=torch.float64).repeat_interleave(gw), torch.arange(gw, dtype=torch.float64).repeat(gh)
    y, x = 2 * (r + 0.5) / gh - 1, 2 * (cc + 0.5) / gw - 1
    f = 100.0 ** (-torch.arange(16, dtype=torch.float64) / 16)
    ang = 2 * math.pi * torch.cat((y[:, None] * f, x[:, None] * f), 1)
    assert float((t[:, :32].double() - torch.cos(ang)).abs().max()) < 4e-6 and float((t[:, 32:].double() - torch.sin(ang)).abs().max()) < 4e-6
