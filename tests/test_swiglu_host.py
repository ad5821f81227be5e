"""CPU: the host side of DINOv2 ViT-g/14's SwiGLU MLP (transformers modeling_dinov2.py:300-315) -- the SwiGLU restatement of the forward (tests/swiglu_ref.py)
against transformers' own Dinov2Model, the pad + interleave helper (ucod_dpl_amd/swiglu.py) in f64, checkpoint normalisation, the giant architecture's
state-dict layout, and the backbone-backward engine's refusal."""
import pytest
import torch

from ucod_dpl_amd import swiglu
from ucod_dpl_amd.vit_engine import normalize_state_dict, _prepare_mlp, ViTLoRAEngine
from ucod_dpl_amd.data.utils.feature_extractor import ARCHS, HUB_TO_ARCH, random_state_dict
from swiglu_ref import dinov2_swiglu_forward, random_swiglu_state_dict, swiglu_hidden


def hf_swiglu_chunk(x, w_in, b_in):
    """HF's formula: (x1, x2) = weights_in(x).chunk(2); silu(x1) * x2."""
    x1, x2 = (x @ w_in.t() + b_in).chunk(2, dim=-1)
    return torch.nn.functional.silu(x1) * x2


@pytest.mark.parametrize("F0", [344, 4096])
def test_pad_and_interleave_equal_the_chunk_formula_in_f64(F0):
    g = torch.Generator().manual_seed(F0)
    D = 64
    w_in, b_in, w_out = torch.randn(2 * F0, D, generator=g, dtype=torch.float64), torch.randn(2 * F0, generator=g, dtype=torch.float64), \
        torch.randn(D, F0, generator=g, dtype=torch.float64)
    x = torch.randn(7, D, generator=g, dtype=torch.float64)
    wp, bp, wo = swiglu.prepare(w_in, b_in, w_out)
    F = swiglu.padded_hidden(F0)
    assert F % 128 == 0 and wp.shape == (2 * F, D) and bp.shape == (2 * F,) and wo.shape == (D, F)
    hidden = swiglu.swiglu_interleaved(x @ wp.t() + bp)            # the epilogue's blockwise product on the permuted GEMM output
    ref = hf_swiglu_chunk(x, w_in, b_in)
    torch.testing.assert_close(hidden[:, :F0], ref, rtol=1e-13, atol=1e-12)                    # (f64 BLAS may sum the permuted rows in another order)
    assert torch.equal(hidden[:, F0:], torch.zeros(7, F - F0, dtype=torch.float64))
    torch.testing.assert_close(hidden @ wo.t(), ref @ w_out.t(), rtol=1e-13, atol=1e-12)


def test_interleave_layout_is_blocks_of_four():
    perm = swiglu.interleave_perm(8)
    assert perm.tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def test_hf_swiglu_width_and_padding():
    assert swiglu_hidden(1536) == 4096 and swiglu_hidden(128) == 344
    assert swiglu.padded_hidden(344) == 384 and swiglu.padded_hidden(4096) == 4096


def test_normalize_detects_swiglu_and_leaves_gelu_dicts_alone():
    sd = random_swiglu_state_dict(128, 2, 2, seed=3)
    c = normalize_state_dict(sd)
    assert c["mlp"] == "swiglu" and c["kind"] == "dinov2"
    assert c["layers"][1]["fc1_w"] is sd["encoder.layer.1.mlp.weights_in.weight"] and c["layers"][1]["fc2_w"] is sd["encoder.layer.1.mlp.weights_out.weight"]
    kind, cp = _prepare_mlp(c)
    assert kind == 1 and cp["layers"][0]["fc1_w"].shape == (768, 128) and cp["layers"][0]["fc2_w"].shape == (128, 384)
    g = random_state_dict("dinov2_vitb14", seed=1, image_size=28)
    cg = normalize_state_dict(g)
    assert set(cg) == {"layers", "patch_w", "patch_b", "cls", "pos", "kind"}
    assert set(cg["layers"][0]) == {"ln1_g", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2"}
    assert cg["layers"][3]["fc1_w"] is g["encoder.layer.3.mlp.fc1.weight"] and cg["layers"][3]["fc2_b"] is g["encoder.layer.3.mlp.fc2.bias"]
    assert _prepare_mlp(cg) == (0, cg)


def test_giant_arch_entries():
    assert ARCHS["dinov2_vitg14"] == (1536, 24, 40, 14, 518, True)
    assert HUB_TO_ARCH["facebook/dinov2-giant"] == "dinov2_vitg14"


def test_giant_state_dict_matches_the_hf_giant_layout():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Dinov2Config(hidden_size=1536, num_hidden_layers=40, num_attention_heads=24, image_size=518, patch_size=14, mlp_ratio=4,
                                    use_swiglu_ffn=True)
    with torch.device("meta"):
        hf = transformers.Dinov2Model(cfg)
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if k != "embeddings.mask_token"}   # (mask_token: unused at inference, no arch emits it)
    got = {k: tuple(v.shape) for k, v in random_state_dict("dinov2_vitg14", device="meta").items()}
    assert got == want
    assert got["encoder.layer.0.mlp.weights_in.weight"] == (8192, 1536) and got["encoder.layer.39.mlp.weights_out.weight"] == (1536, 4096)


@pytest.mark.parametrize("tag,img,pre", [("native", 70, 70), ("interp", 70, 56)])
def test_restatement_matches_transformers(tag, img, pre):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(20)
    cfg = transformers.Dinov2Config(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, image_size=pre, patch_size=14, mlp_ratio=4,
                                    layerscale_value=1.0, use_swiglu_ffn=True, attn_implementation="eager")
    m = transformers.Dinov2Model(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            if "position_embeddings" in n or "cls_token" in n:
                p.mul_(0.05)
    keys = {}
    m.encoder.layer[-1].attention.attention.key.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o.detach()))
    x = torch.randn(2, 3, img, img)
    with torch.no_grad():
        out = m(x, output_attentions=True)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    last, key, att = dinov2_swiglu_forward(x, sd, heads=2)
    g = img // 14
    k_hf = keys["k"][:, 1:].reshape(2, g, g, -1).permute(0, 3, 1, 2)
    torch.testing.assert_close(key, k_hf, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(last, out.last_hidden_state, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(att, out.attentions[-1][:, :, 0, 1:], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("tag,pre", [("native", 70), ("interp", 56)])
def test_restatement_matches_the_g20_goldens(tag, pre):
    """tests/golden/make_golden_swiglu.py: transformers' Dinov2Model (use_swiglu_ffn=True) on random_swiglu_state_dict(128, 2, 3, seed=20) weights, recorded; the
    weights are regenerated here and must hash to what the generator hashed (otherwise the comparison would be against other weights)."""
    import hashlib
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"g20_dinov2_swiglu_{tag}.npz"))
    sd = random_swiglu_state_dict(128, 2, 3, image_size=int(z["image_size"]), seed=int(z["seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].to(torch.float32).contiguous().numpy().tobytes())
    assert h.hexdigest() == str(z["sd_sha256"]), "random_swiglu_state_dict no longer draws the weights the goldens were made with"
    assert int(z["image_size"]) == pre
    last, key, att = dinov2_swiglu_forward(torch.from_numpy(z["x"]), sd, heads=2)
    torch.testing.assert_close(key, torch.from_numpy(z["key"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(last, torch.from_numpy(z["last_hidden_state"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(att, torch.from_numpy(z["cls_att"]), rtol=1e-5, atol=1e-6)


def test_lora_engine_refuses_a_swiglu_checkpoint():
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        ViTLoRAEngine(random_swiglu_state_dict(128, 2, 2), heads=2, device="cpu")
