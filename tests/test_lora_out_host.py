"""CPU: the host side of LoRA on the output projections (``attention.output.dense`` / ``mlp.fc2``; ``o_proj`` / ``down_proj`` on a DINOv3 checkpoint;
models/modules/full_model.py:47-72 hands ``target_modules`` to peft) -- the opt-in ``allow_out`` of the target parsers, the new names of native.py against
include/ucod_dpl.h, the workspace helpers, and the f64 restatement tests/lora_out_ref.py: that the cases the GPU tests run give their bars teeth (a pass that ignores the
new modules, or drops their ``t A`` term, lands at least three bars away), that peft's zero init gives exact zeros, and that the DINOv3 restatement is transformers'
own G23 values when the new modules' B is zero."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, sub
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import _REFUSED, _REFUSED3, lora_targets, lora_targets_dinov3
import dinov3_ref as R3
import dinov3_lora_ref as RL
import lora_targets_ref as R
import lora_out_ref as RO


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------ target parsing
@pytest.mark.parametrize("targets,want", [
    (["dense"], ((False, False, False), None, ("dense",))),
    (["fc2"], ((False, False, False), None, ("fc2",))),
    (["query", "value", "dense", "fc2"], ((True, False, True), None, ("dense", "fc2"))),
    (["fc2", "dense", "key"], ((False, True, False), None, ("dense", "fc2"))),
    (["query", "key", "value", "fc1", "dense", "fc2"], ((True, True, True), "fc1", ("dense", "fc2"))),
    (["output.dense"], ((False, False, False), None, ("dense",))),
    (["attention.output.dense", "mlp.fc2", "attention.value"], ((False, False, True), None, ("dense", "fc2"))),
    (["query", "key", "value"], ((True, True, True), None, ())),
])
def test_flag_on_accepts_the_output_projections(targets, want):
    assert lora_targets(targets, "gelu", 3, allow_out=True) == want
    assert lora_targets(None, "gelu", 3, allow_out=True) == ((True, True, True), None, ())


@pytest.mark.parametrize("targets,want", [
    (["o_proj"], ((False, False, False), ("o_proj",))),
    (["q_proj", "o_proj", "down_proj"], ((True, False, False), ("o_proj", "down_proj"))),
    (["mlp.down_proj", "attention.v_proj"], ((False, False, True), ("down_proj",))),
    (["q_proj", "k_proj", "v_proj"], ((True, True, True), ())),
])
@pytest.mark.parametrize("layer_path", ["model.layer.", "layer."])
def test_flag_on_accepts_o_proj_and_the_non_gated_down_proj(targets, want, layer_path):
    assert lora_targets_dinov3(targets, False, 3, layer_path, allow_out=True) == want
    assert lora_targets_dinov3(None, False, 3, layer_path, allow_out=True) == ((True, True, True), ())


def test_swiglu_output_projections_stay_refused_with_a_true_reason():
    for call in (lambda: lora_targets(["query", "weights_out"], "swiglu", 2, allow_out=True),
                 lambda: lora_targets_dinov3(["q_proj", "down_proj"], True, 2, allow_out=True)):
        with pytest.raises(NotImplementedError, match="not built") as e:
            call()
        assert "recomputed from the interleaved, padded [M, 2F] pre-activation" in str(e.value) and "leading-dimension" not in str(e.value)
    # the gated MLP keeps its o_proj; up_proj, gate_proj and the patch embedding stay refused as ever, flag or no flag
    assert lora_targets_dinov3(["o_proj", "v_proj"], True, 2, allow_out=True) == ((False, False, True), ("o_proj",))
    assert lora_targets(["dense", "weights_in"], "swiglu", 2, allow_out=True) == ((False, False, False), "weights_in", ("dense",))
    for name in ("up_proj", "gate_proj", "patch_embeddings"):
        for flag in (False, True):
            with pytest.raises(NotImplementedError) as e:
                lora_targets_dinov3(["q_proj", name], True, 2, allow_out=flag)
            assert _REFUSED3[name] in str(e.value)
    for flag in (False, True):
        with pytest.raises(NotImplementedError) as e:
            lora_targets(["query", "projection"], "gelu", 2, allow_out=flag)
        assert _REFUSED["projection"] in str(e.value)


def test_flag_off_is_todays_surface():
    """Return shapes, exceptions and messages without the flag (tests/test_lora_targets_host.py and tests/test_dinov3_lora_host.py pin the rest)."""
    assert lora_targets(["query", "fc1"], "gelu", 2) == ((True, False, False), "fc1") and lora_targets(None) == ((True, True, True), None)
    assert lora_targets_dinov3(["q_proj"], False, 2) == (True, False, False) and lora_targets_dinov3(None) == (True, True, True)
    for name in ("dense", "fc2"):
        with pytest.raises(NotImplementedError) as e:
            lora_targets(["query", name], "gelu", 2)
        assert str(e.value) == (f"LoRA target module {name!r} (encoder.layer.0.{RO.PATHS[name]}) is not built: {_REFUSED[name]}") and "leading-dimension" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        lora_targets(["weights_out"], "swiglu", 2)
    assert _REFUSED["weights_out"] in str(e.value) and "leading-dimension" in str(e.value)
    for name in ("o_proj", "down_proj"):
        with pytest.raises(NotImplementedError) as e:
            lora_targets_dinov3(["q_proj", name], False, 2)
        assert str(e.value) == f"LoRA target module {name!r} (model.layer.0.{RO.PATHS[name]}) is not built: {_REFUSED3[name]}"


# ------------------------------------------------------------------------------------------------ names and sizes of the C ABI
OUT_ENTRY_POINTS = ("ucod_lora_out_grad_workspace_bytes", "ucod_lora_out_fwd", "ucod_lora_out_grad_s", "ucod_lora_out_grad_x", "ucod_vit_train_workspace_bytes_lora_out",
                    "ucod_vit_forward_train_lora_out", "ucod_vit_backward_lora_out", "ucod_vit_lora_infer_workspace_bytes_lora_out", "ucod_vit_forward_lora_infer_lora_out")


def test_new_names_sit_at_the_numbers_of_the_header():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert int(re.search(r"#define UCOD_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION == 5
    assert int(re.search(r"#define UCOD_VIT_TRAIN_OUT_STRIDE (\d+)", header).group(1)) == N.VIT_TRAIN_OUT_STRIDE == len(N.VIT_TRAIN_OUT_SLOTS) == 4
    assert N.VIT_TRAIN_OUT_SLOTS == ("lora_dense", "lora_dense_grad", "lora_fc2", "lora_fc2_grad")
    assert (N.O_LORA_DENSE, N.O_LORA_DENSE_GRAD, N.O_LORA_FC2, N.O_LORA_FC2_GRAD) == (0, 1, 2, 3)
    for at, words in enumerate((r"dense parameters", r"dense gradients", r"fc2 parameters", r"fc2 gradients")):
        assert re.search(rf"\+{at} {words}", header), (at, words)
    assert int(re.search(r"#define UCOD_LORA_OUT_W (\d+)", header).group(1)) == N.LORA_OUT_W == N.LORA_MLP_MAX_R == 8
    assert int(re.search(r"#define UCOD_LORA_OUT_ACT_IDENTITY (\d+)", header).group(1)) == N.LORA_OUT_ACT_IDENTITY == 0
    assert int(re.search(r"#define UCOD_LORA_OUT_ACT_GELU (\d+)", header).group(1)) == N.LORA_OUT_ACT_GELU == 1
    # the old strides did not move
    assert (N.VIT_TRAIN_STRIDE, N.VIT_TRAIN_MLP_STRIDE, N.VIT_LAYER_STRIDE) == (7, 3, 16)
    lib = N.load()
    for name in OUT_ENTRY_POINTS:
        assert name in N.SIGNATURES and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    # the header says where the modules come from, what peft computes and which dropout keys they take
    block = header[header.index("LoRA on the output projections as well"):header.index("#define UCOD_VIT_TRAIN_OUT_STRIDE")]
    assert "full_model.py:47-72" in block and "result = base(x) + scaling * B(A(dropout(x)))" in block
    assert "2 L + l" in block and "3 L + l" in block


def train_desc(D=128, heads=2, F=512, L=3, r=2):
    td = N.VitTrainDesc()
    v = td.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps = 2, 3, 70, 70, 14, D, heads, F, L, 640, 1e-6
    td.lora_r, td.lora_scaling = r, 2.0
    return td


def test_workspace_helpers_add_nothing_without_the_table_and_the_plan_with_it():
    """The size helpers run on the host.  The table's pointers are never dereferenced by them; they are made up."""
    lib = N.load()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert lib.ucod_lora_out_grad_workspace_bytes(2, 768, 768) == 4 * max(512 * 768 * 2, 256 * 2 * 768)
    assert lib.ucod_lora_out_grad_workspace_bytes(2, 3072, 768) == 4 * 256 * 2 * 3072
    for r, K, D in ((0, 512, 128), (9, 512, 128), (2, 64, 128), (2, 4224, 128), (2, 8192, 128), (2, 576, 128), (2, 512, 1664), (2, 512, 192)):
        assert lib.ucod_lora_out_grad_workspace_bytes(r, K, D) == 0, (r, K, D)
    td = train_desc()
    M, D, F, L, r = 2 * 26, 128, 512, 3, 2
    TM = (C.c_void_p * 9)(*([4096] * 9))
    table = lambda o, f: (C.c_void_p * 12)(*([4096 if o else None] * 2 + [4096 if f else None] * 2) * 3)  # noqa: E731
    for tm in (None, TM):
        base = lib.ucod_vit_train_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, tm)
        assert base > 0 and lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_GELU, tm, None) == base
        ibase = lib.ucod_vit_lora_infer_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, tm)
        assert ibase > 0
        for o, f in ((True, False), (False, True), (True, True)):
            gw = max(lib.ucod_lora_out_grad_workspace_bytes(r, D, D) if o else 0, lib.ucod_lora_out_grad_workspace_bytes(r, F, D) if f else 0)
            want = base + (int(o) + int(f)) * up(M * 32) * (L - 1) + up(M * 32) + up(gw)        # u per layer and module (M * 32 bytes), t, the partials
            assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_GELU, tm, table(o, f)) == want, (o, f)
            assert lib.ucod_vit_lora_infer_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_GELU, tm, table(o, f)) == ibase       # the no-grad pass saves nothing
    # refused: a table that names no module, fc2 on the SwiGLU MLP, a rank beyond 8 (taken without the table: 3 r <= 64 as ever)
    assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_GELU, None, table(False, False)) == 0
    assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_SWIGLU, None, table(False, True)) == 0
    assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), N.UCOD_MLP_SWIGLU, None, table(True, False)) > 0
    td9 = train_desc(r=9)
    assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td9), N.UCOD_MLP_GELU, None, table(True, True)) == 0
    assert lib.ucod_vit_lora_infer_workspace_bytes_lora_out(C.byref(td9), N.UCOD_MLP_GELU, None, table(True, True)) == 0
    assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td9), N.UCOD_MLP_GELU, None, None) > 0


# ------------------------------------------------------------------------------------------------ the restatement, and the strength of the GPU cases
@functools.lru_cache(maxsize=None)
def checkpoint(D):
    """(state dict, heads, L, image size, batch) of the two models tests/test_gpu_lora_out.py runs: G8's native DINOv2 (D = 128) and the D = 256 GELU model."""
    if D == 128:
        sd = sub(load_golden("g8_dinov2_native"), "sd.")
        return sd, 2, 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer.")), 70, 2
    return RO.d256_state_dict()


def test_without_the_new_modules_the_restatement_is_the_old_one():
    sd, heads, L, image, B = checkpoint(128)
    img, dkey = RO.case_inputs(B, 128, image)
    lora = RO.lora_for(sd, ("query", "value", "fc1"))
    k0, g0 = R.lora_grads(img, {**sd, **lora}, heads, dkey, 2.0)
    k1, g1 = RO.lora_grads(img, {**sd, **lora}, heads, dkey, 2.0)
    assert torch.equal(k0, k1) and all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("targets", RO.TARGET_SETS)
@pytest.mark.parametrize("D", [128, 256])
def test_the_gpu_cases_have_teeth(D, targets):
    """With B of the output modules at lora_out_ref.OUT_B_STD, in f64, on the GPU tests' checkpoints and inputs:
    (a) a forward without the new modules' term moves the key map by at least 3 x the key bar (3e-2 max(1, |key|max): 3.0e-2 / 4.2e-2);
    (b) a backward without their ``t A`` term moves every non-zero q / k / v / fc1 gradient below the last layer by at least 3 x the gradient bar (4e-2 at D = 128,
        5e-2 at D = 256, relative L2); the new modules' own gradients below the topmost module move too (printed, held to no distance)."""
    sd, heads, L, image, B = checkpoint(D)
    img, dkey = RO.case_inputs(B, D, image)
    lora = RO.lora_for(sd, targets)
    key, g = RO.lora_grads(img, {**sd, **lora}, heads, dkey, 2.0)
    plain = {k: v.double() for k, v in {**sd, **RO.without_out_modules(lora)}.items() if v.is_floating_point()}
    key_plain = RO.forward(img.double(), plain, heads, 2.0)
    key_bar = 3e-2 * max(1.0, key.abs().max().item())
    moved = (key - key_plain).abs().max().item()
    _, g_cut = RO.lora_grads(img, {**sd, **lora}, heads, dkey, 2.0, cut_input_grad=True)
    bar = 4e-2 if D == 128 else 5e-2
    is_out = lambda k: any(f".{RO.PATHS[t]}." in k for t in RO.OUT_NAMES)  # noqa: E731
    layer = lambda k: int(k.split(".")[2])  # noqa: E731
    old = {k: rel_l2(g_cut[k], g[k]) for k in g if not is_out(k) and layer(k) < L - 1 and float(g[k].abs().max()) != 0.0}
    # a module's own dB never sees its own t A; below the topmost targeted layer (L - 2) both of its gradients see the terms of the layers above
    new = {k: rel_l2(g_cut[k], g[k]) for k in g if is_out(k) and layer(k) < L - 2}
    print(f"D={D} {targets}: key moves {moved:.3e} (3 x bar {3 * key_bar:.3e}); t A dropped: q/k/v/fc1 gradients move >= {min(old.values()) if old else None}, "
          f"the new modules' >= {min(new.values()):.3e} (3 x bar {3 * bar:.2e})")
    assert moved >= 3 * key_bar, (moved, key_bar)
    assert len(old) == 2 * (L - 1) * sum(t not in RO.OUT_NAMES for t in targets)
    for k, d in old.items():
        assert d >= 3 * bar, (k, d)
    assert all(d > 1e-3 for d in new.values())                  # (reached, but held to no distance: the issue's condition is on q / k / v / fc1)
    # the last layer's new modules never reach the key map: exact zeros; everything below is non-zero
    for k in g:
        if is_out(k):
            assert (float(g[k].abs().max()) == 0.0) == (layer(k) == L - 1), k


@pytest.mark.parametrize("D", [128, 256])
def test_pefts_zero_init_gives_exact_zeros(D):
    """B = 0 on the output modules: their term vanishes -- the key map is the forward's without them, bit for bit -- and so does dA (t = s B = 0); dB does not."""
    sd, heads, L, image, B = checkpoint(D)
    img, dkey = RO.case_inputs(B, D, image)
    lora = RO.lora_for(sd, ("query", "key", "value", "fc1", "dense", "fc2"), out_b_std=0.0)
    key, g = RO.lora_grads(img, {**sd, **lora}, heads, dkey, 2.0)
    key_plain, g_plain = R.lora_grads(img, {**sd, **RO.without_out_modules(lora)}, heads, dkey, 2.0)
    assert torch.equal(key, key_plain)
    for k, v in g.items():
        if k in g_plain:
            assert torch.equal(v, g_plain[k]), k
        elif k.endswith("lora_A.weight"):
            assert float(v.abs().max()) == 0.0, k
        else:
            assert (float(v.abs().max()) > 0.0) == (int(k.split(".")[2]) < L - 1), k


def test_dinov3_restatement_is_the_g23_golden_when_the_new_b_is_zero():
    """tests/test_gpu_lora_out.py compares the engine on G23's ``g46`` model against lora_out_ref.forward_dinov3; with B = 0 on o_proj / down_proj that forward and
    its q / k / v gradients are transformers' own f64 values of the golden (as tests/test_dinov3_lora_host.py holds dinov3_lora_ref to them)."""
    tag = "g46"
    z = np.load(os.path.join(ROOT, "tests", "golden", f"g23_dinov3_lora_{tag}.npz"))
    sd, lora = R3.g22_state_dict(tag), RL.g23_lora(tag)
    assert R3.weights_sha256(sd) == str(z["sd_sha256"])
    x, dkey = RL.g23_inputs(tag)
    extra = RO.lora_for(sd, ("o_proj", "down_proj"), out_b_std=0.0, seed=5)
    key, g = RO.lora_grads(x, {**sd, **lora, **extra}, R3.G22[tag]["heads"], dkey, RL.G23_SCALE, dinov3=True)
    assert rel_l2(key, torch.from_numpy(z["key"])) < 1e-9
    for k in z.files:
        if k.startswith("grad/"):
            ref = torch.from_numpy(z[k])
            if float(ref.abs().max()) == 0.0:
                assert float(g[k[5:]].abs().max()) == 0.0, k
            else:
                assert rel_l2(g[k[5:]], ref) < 1e-9, k
    for k in extra:
        if k.endswith("lora_A.weight"):
            assert float(g[k].abs().max()) == 0.0, k
    # ... and with B at the test's scale the DINOv3 case has the same teeth (bars of tests/test_gpu_dinov3_lora.py: the key bound, 5e-2 per gradient)
    full = {**sd, **lora, **RO.lora_for(sd, ("o_proj", "down_proj"), seed=5)}
    key2, g2 = RO.lora_grads(x, full, R3.G22[tag]["heads"], dkey, RL.G23_SCALE, dinov3=True)
    assert rel_l2(key, key2) >= 3 * R3.engine_bound("bf16", z)
    _, g_cut = RO.lora_grads(x, full, R3.G22[tag]["heads"], dkey, RL.G23_SCALE, dinov3=True, cut_input_grad=True)
    for k in lora:
        if int(k.split(".")[2]) < R3.G22_LAYERS - 1:
            assert rel_l2(g_cut[k], g2[k]) >= 3 * RL.grad_bar(z, k, 0.05), k
