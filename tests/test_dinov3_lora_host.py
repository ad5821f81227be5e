"""CPU: backbone-backward (LoRA) mode on a DINOv3 checkpoint, the host side -- the f64 restatement tests/dinov3_lora_ref.py against the G23 goldens recorded from
transformers (tests/golden/make_golden_dinov3_lora.py), the proof that those goldens tell each fault of a rotary BACKWARD apart under the bars of
tests/test_gpu_dinov3_lora.py, and the constructor contract of ViTLoRAEngine / load_lora before any GPU call: the allow_rope switch, target names, key names, the
descriptor field and the new symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTLoRAEngine, lora_modules, lora_targets, lora_targets_dinov3
import dinov3_ref as R3
import dinov3_lora_ref as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LAST = R3.G22_LAYERS - 1


def golden(tag):
    z = np.load(os.path.join(GOLDEN, f"g23_dinov3_lora_{tag}.npz"))
    sd, lora = R3.g22_state_dict(tag), RL.g23_lora(tag)
    assert R3.weights_sha256(sd) == str(z["sd_sha256"]), "random_dinov3_state_dict no longer draws the weights the goldens were made with"
    x, dkey = RL.g23_inputs(tag)
    assert int(z["input_seed"]) == RL.G23_INPUT_SEED[tag]
    assert np.array_equal(z["x"], x.numpy()) and np.array_equal(z["dkey"], dkey.numpy()) and z["key"].dtype == np.float64
    assert sorted(k[5:] for k in z.files if k.startswith("lora/")) == sorted(lora)
    for n, v in lora.items():
        assert np.array_equal(z["lora/" + n], v.numpy()), n
    return z, sd, lora, x, dkey


def grad_names(z, zero=False):
    return sorted(k[5:] for k in z.files if k.startswith("grad/") and (float(np.abs(z[k]).max()) == 0.0) == zero)


@pytest.mark.parametrize("tag", RL.G23_TAGS)
def test_restatement_matches_the_g23_goldens(tag):
    z, sd, lora, x, dkey = golden(tag)
    key, grads = RL.lora_grads(x, {**sd, **lora}, R3.G22[tag]["heads"], dkey, RL.G23_SCALE)
    assert key.shape == z["key"].shape and R3.rel_l2(key, torch.from_numpy(z["key"])) < 1e-9
    assert sorted(grads) == sorted(lora) and len(grads) == 2 * 3 * R3.G22_LAYERS
    for n in grad_names(z):
        assert z["grad/" + n].dtype == np.float64 and R3.rel_l2(grads[n], torch.from_numpy(z["grad/" + n])) < 1e-9, n
    # structurally zero: the last layer's q_proj and v_proj never reach the key hook -- exactly zero in the golden and in the restatement
    zeros = grad_names(z, zero=True)
    assert zeros == sorted(f"model.layer.{LAST}.attention.{nm}.lora_{ab}.weight" for nm in ("q_proj", "v_proj") for ab in "AB")
    for n in zeros:
        assert float(grads[n].abs().max()) == 0.0, n


@pytest.mark.parametrize("fault", RL.BWD_FAULTS)
@pytest.mark.parametrize("tag", RL.G23_TAGS)
def test_each_backward_fault_lands_at_its_stored_distance_and_twice_above_the_bar(tag, fault):
    """The condition that keeps the GPU test from hiding a fault: every q / k gradient of a rotating layer whose projection the fault touches lies at least
    twice above the bar that tensor is held to (the larger, with-dropout bar), so an engine with the fault is at least (distance - bar) > bar away."""
    z, sd, lora, x, dkey = golden(tag)
    _, bad = RL.lora_grads(x, {**sd, **lora}, R3.G22[tag]["heads"], dkey, RL.G23_SCALE, bwd_fault=fault)
    touched = [n for n in grad_names(z) if int(n.split(".")[2]) != LAST and n.split(".")[4] in RL.TOUCHES[fault]]
    assert len(touched) == 2 * (R3.G22_LAYERS - 1) * len(RL.TOUCHES[fault])
    for n in grad_names(z):
        d, want = R3.rel_l2(bad[n], torch.from_numpy(z["grad/" + n])), float(z[f"bf_{fault}/{n}"])
        assert abs(d - want) <= 1e-6 * max(want, 1e-12) + 1e-12, (n, d, want)
    for n in touched:
        assert float(z[f"bf_{fault}/{n}"]) >= 2.0 * RL.grad_bar(z, n, p_drop=0.05), (n, float(z[f"bf_{fault}/{n}"]), RL.grad_bar(z, n, 0.05))
    # the last layer runs no rotation: a backward fault leaves its k_proj gradient alone; everything upstream of a rotating layer moves
    for ab in "AB":
        assert float(z[f"bf_{fault}/model.layer.{LAST}.attention.k_proj.lora_{ab}.weight"]) < 1e-12
        assert float(z[f"bf_{fault}/model.layer.0.attention.v_proj.lora_{ab}.weight"]) > 1e-2


@pytest.mark.parametrize("tag", RL.G23_TAGS)
def test_bars_and_the_key_bound(tag):
    z = np.load(os.path.join(GOLDEN, f"g23_dinov3_lora_{tag}.npz"))
    for n in grad_names(z):
        ebf = float(z["ebf/" + n])
        assert 1e-3 < ebf < 5e-2, (n, ebf)                        # bf16 arithmetic: per cent, not more
        assert RL.grad_bar(z, n) == max(4e-2, 3 * ebf) and RL.grad_bar(z, n, 0.05) == max(5e-2, 3 * ebf)
    for n in grad_names(z, zero=True):
        assert "ebf/" + n not in z.files
    # the key map: the engine's bound (3 x transformers under bf16 autocast) under half the smallest forward fault -- a pass that rotates wrongly cannot stay inside
    assert 5 * float(z["err_f32"]) < float(z["err_bf16ac"])
    assert R3.engine_bound("bf16", z) < 0.5 * min(float(z["fault_" + f]) for f in R3.FAULTS)


# ================================================================================================ the constructor contract, before any GPU call
def test_allow_rope_is_the_switch():
    sd = R3.g22_state_dict("g46")
    with pytest.raises(NotImplementedError, match=r"DINOv3.*RoPE.*allow_rope=True$"):
        ViTLoRAEngine(sd, 2, device="cpu")
    # with the flag the constructor goes on to the device step: the first tensor it hands to the library is not on a GPU
    with pytest.raises(RuntimeError, match="not on a GPU"):
        ViTLoRAEngine(sd, 2, device="cpu", allow_rope=True, eps=1e-5)
    # the flag does not replace allow_swiglu on a gated-MLP checkpoint
    with pytest.raises(NotImplementedError, match="allow_swiglu=True"):
        ViTLoRAEngine(R3.g22_state_dict("gated"), 2, device="cpu", allow_rope=True)
    from ucod_dpl_amd.models.modules.full_model import load_lora
    from ucod_dpl_amd.engine.config import CfgNode
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, allow_rope=False)), sd, 2, device="cpu")
    with pytest.raises(RuntimeError, match="not on a GPU"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, allow_rope=True, rope_theta=100.0)), sd, 2, device="cpu")
    with pytest.raises(RuntimeError, match="not on a GPU"):       # (gated: load_lora passes allow_swiglu itself)
        load_lora(CfgNode(dict(r=2, lora_alpha=4, allow_rope=True)), R3.g22_state_dict("gated"), 2, device="cpu")


def test_target_names_of_a_dinov3_checkpoint():
    T = lora_targets_dinov3
    assert T(None, False, 3) == (True, True, True)
    assert T(["q_proj", "k_proj", "v_proj"], True, 3) == (True, True, True)
    assert T(["q_proj", "v_proj"], False, 3) == (True, False, True) and T(["attention.k_proj"], False, 3) == (False, True, False)
    with pytest.raises(NotImplementedError, match="no Linear module"):
        T(["proj"], False, 3)                                     # peft's rule is ".<target>" or equality, not a substring
    with pytest.raises(ValueError, match="empty"):
        T([], False, 3)
    with pytest.raises(NotImplementedError, match="regular expression"):
        T("q_proj", False, 3)
    for leaf, why in (("o_proj", "attention kernel"), ("down_proj", "drain"), ("up_proj", "not built yet"), ("gate_proj", "two peft modules")):
        with pytest.raises(NotImplementedError, match=why):
            T(["q_proj", leaf], True, 3)
    with pytest.raises(NotImplementedError, match="two peft modules"):
        T(["gate_proj"], False, 3)                                # (the plain MLP has no such module: refused with the name's own reason all the same)
    with pytest.raises(NotImplementedError, match="same modules"):
        T(["model.layer.0.attention.q_proj"], False, 3)
    assert T(["layer.0.attention.q_proj", "layer.1.attention.q_proj"], False, 2, "layer.") == (True, False, False)
    # DINOv2's names on a DINOv3 checkpoint: a ValueError that names the right ones
    for name in ("query", "key", "value", "fc1", "weights_in", "dense"):
        with pytest.raises(ValueError, match="q_proj / k_proj / v_proj"):
            T([name], False, 3)
    sd = R3.g22_state_dict("g46")
    with pytest.raises(ValueError, match="q_proj / k_proj / v_proj"):
        ViTLoRAEngine(sd, 2, device="cpu", allow_rope=True, target_modules=["query", "key", "value"])
    with pytest.raises(NotImplementedError, match="o_proj"):
        ViTLoRAEngine(sd, 2, device="cpu", allow_rope=True, target_modules=["o_proj"])
    # lora_targets with its present arguments returns what it returned
    assert lora_targets(None) == ((True, True, True), None) and lora_targets(["query", "fc1"], "gelu", 2) == ((True, False, False), "fc1")
    assert lora_targets(["key", "weights_in"], "swiglu", 1) == ((False, True, False), "weights_in")


def host_engine(tag, layer_path, targets=(True, True, True), r=2, family="dinov3"):
    """A ViTLoRAEngine as its constructor leaves the host side for a DINOv3 checkpoint, with the arena on the CPU (no library call is made by what is tested)."""
    m = R3.G22[tag]
    eng = object.__new__(ViTLoRAEngine)
    eng.L, eng.D, eng.r, eng.scaling, eng.mlp = R3.G22_LAYERS, m["D"], r, 2.0, N.UCOD_MLP_GELU
    eng._adopt(layer_path, lora_modules(family, "gelu", m["D"], m["F"], m["F"], r, targets + (False, False, False)))
    eng.lora = torch.arange(eng.L * eng.qkv_numel, dtype=torch.float32).reshape(eng.L, eng.qkv_numel)
    eng.lora_grad = -eng.lora
    eng.lora_dropout = 0.05
    return eng


@pytest.mark.parametrize("layer_path", ["model.layer.", "layer."])
def test_lora_state_dict_uses_the_checkpoints_names(layer_path, tmp_path):
    eng = host_engine("g46", layer_path, targets=(True, False, True))
    lsd = eng.lora_state_dict()
    assert sorted(lsd) == sorted(f"{layer_path}{i}.attention.{nm}.lora_{ab}.weight" for i in range(3) for nm in ("q_proj", "v_proj") for ab in "AB")
    a, b = lsd[f"{layer_path}1.attention.v_proj.lora_A.weight"], lsd[f"{layer_path}1.attention.v_proj.lora_B.weight"]
    assert tuple(a.shape) == (2, 128) and tuple(b.shape) == (128, 2)
    sa, sb = eng._slices(2)
    assert torch.equal(a.reshape(-1), eng.lora[1, sa]) and torch.equal(b.reshape(-1), eng.lora[1, sb])
    assert torch.equal(eng.lora_state_dict(grads=True)[f"{layer_path}1.attention.v_proj.lora_A.weight"], -a)
    assert [n for n, _ in eng._targeted()] == ["attention.q_proj", "attention.v_proj"]
    # the prefix in front of the layer number in the base state dict, and the adapter folder's names
    sd = {k.replace("model.layer.", layer_path): v for k, v in R3.g22_state_dict("g46").items()}
    assert ViTLoRAEngine._hf_prefix(sd) == layer_path and ViTLoRAEngine._hf_prefix({"backbone." + k: v for k, v in sd.items()}) == "backbone." + layer_path
    from ucod_dpl_amd.models.modules import full_model as M
    import json
    from safetensors.torch import load_file
    M.save_lora_adapter(eng, str(tmp_path))
    saved = load_file(str(tmp_path / M.ADAPTER_WEIGHTS))
    assert sorted(saved) == sorted("base_model.model.ViT." + k for k in lsd)
    assert all(torch.equal(saved["base_model.model.ViT." + k], v) for k, v in lsd.items())
    cfg = json.loads((tmp_path / M.ADAPTER_CONFIG).read_text())
    assert cfg["target_modules"] == ["q_proj", "v_proj"] and cfg["r"] == 2 and cfg["lora_alpha"] == 4 and cfg["bias"] == "none"
    # a key of an untargeted module is refused before anything is written
    with pytest.raises(KeyError, match="does not target"):
        eng.load_lora_state_dict({**lsd, f"{layer_path}0.attention.k_proj.lora_A.weight": torch.zeros(2, 128)})


def test_a_dinov2_engine_keeps_its_names():
    eng = host_engine("g46", "encoder.layer.", family="dinov2")
    assert sorted(eng.lora_state_dict())[0] == "encoder.layer.0.attention.attention.key.lora_A.weight"
    assert ViTLoRAEngine._hf_prefix({"dinov2.encoder.layer.0.attention.attention.query.weight": 0}) == "dinov2.encoder.layer."
    from ucod_dpl_amd.models.modules import full_model as M
    assert M._adapter_prefix(eng) == M.ADAPTER_PREFIX and M._adapter_targets(eng) == ["query", "key", "value"]


def test_the_descriptor_field_and_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert re.search(r"int ucod_rope_qk_ld\(void\* buf, int elem, const float\* cos_sin, int B, int tok, int n_reg, int heads, int ld, int inverse, void\* stream\);", header)
    assert re.search(r"unsigned long long seed;[^\n]*\n\s*int allow_rope;", header) and "#define UCOD_ABI_VERSION 5" in header
    names = [f[0] for f in N.VitTrainDesc._fields_]
    assert names[-2:] == ["seed", "allow_rope"] and N.VitTrainDesc().allow_rope == 0          # the zero-filled descriptor of every existing caller refuses a table
    assert N.VitTrainDesc.lora_r.offset == 80 and N.VitTrainDesc.seed.offset == 96 and N.VitTrainDesc.allow_rope.offset == 104 and C.sizeof(N.VitTrainDesc) == 112
    assert len(N.SIGNATURES["ucod_rope_qk_ld"][1]) == 10 and N.ABI_VERSION == 5
    for half in ("bf16", "f16"):
        lib = N.load(half)
        call = lambda buf=4096, elem=0, tab=4096, B=1, tok=10, R=4, heads=2, ld=384, inv=1: lib.ucod_rope_qk_ld(buf, elem, tab, B, tok, R, heads, ld, inv, None)  # noqa: E731
        # argument validation runs before any launch (there is no device here): each of these is UCOD_EINVAL
        assert call(buf=None) == -1 and call(tab=None) == -1 and call(elem=2) == -1 and call(inv=2) == -1 and call(inv=-1) == -1
        assert call(ld=383) == -1 and call(ld=376) == -1          # ld < 3 D
        assert call(ld=388) == -1 and call(ld=386, elem=1) == -1   # ld * sizeof(element) not a multiple of 16 (16-bit: 8 elements; f32: 4)
        assert call(R=9) == -1 and call(R=10) == -1 and call(tok=5) == -1 and call(R=-1) == -1       # n_reg >= tok - 1: no patch row left
        assert call(buf=4100) == -1 and call(tab=4100) == -1 and call(B=0) == -1 and call(heads=0) == -1
        # the size helpers of the training passes: a table is refused without the flag, before any launch
        t = N.VitTrainDesc()
        v = t.vit
        v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps, v.attn_variant, v.n_reg = 2, 3, 64, 96, 16, 128, 2, 512, 3, 768, 1e-5, 2, 4
        t.lora_r, t.lora_scaling = 2, 2.0
    libb = N.load("bf16")
    plain = (libb.ucod_vit_train_workspace_bytes(C.byref(t)), libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)))
    assert plain[0] > 0 and plain[1] > 0
    t.allow_rope = 1                                              # with a NULL table the flag changes nothing
    assert (libb.ucod_vit_train_workspace_bytes(C.byref(t)), libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t))) == plain
    t.vit.rope = 4096                                             # (never dereferenced by the size helpers) the plan does not change with a table
    assert (libb.ucod_vit_train_workspace_bytes(C.byref(t)), libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t))) == plain
    assert libb.ucod_vit_train_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_SWIGLU) > 0
    for flag in (0, 2, -1):
        t.allow_rope = flag
        assert libb.ucod_vit_train_workspace_bytes(C.byref(t)) == 0 and libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) == 0
