"""CPU: the host side of LoRA on the SwiGLU MLP's output projection (``mlp.weights_out`` on DINOv2 ViT-g/14, ``mlp.down_proj`` on a gated DINOv3 checkpoint;
models/modules/full_model.py:47-72 hands ``target_modules`` to peft) -- the new names of native.py against include/ucod_dpl.h, the _ex size helpers, the opt-in
``allow_swiglu_out`` of the target parsers, the f64 restatement tests/lora_swiglu_out_ref.py against transformers' own G24 values with the strength of the three
faults, and the padded arena against the unpadded state dict."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import _REFUSED, _REFUSED3, lora_targets, lora_targets_dinov3
import lora_swiglu_out_ref as RS

EX_ENTRY_POINTS = ("ucod_vit_train_workspace_bytes_lora_out_ex", "ucod_vit_forward_train_lora_out_ex", "ucod_vit_backward_lora_out_ex",
                   "ucod_vit_lora_infer_workspace_bytes_lora_out_ex", "ucod_vit_forward_lora_infer_lora_out_ex")


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------ header and bindings
def test_new_names_sit_at_the_numbers_of_the_header():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert int(re.search(r"#define UCOD_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION == 5
    assert C.sizeof(N.VitTrainDesc) == 112
    assert int(re.search(r"#define UCOD_LORA_OUT_ACT_SWIGLU (\d+)", header).group(1)) == N.LORA_OUT_ACT_SWIGLU == 2
    assert int(re.search(r"#define UCOD_LORA_OUT_SWIGLU (\d+)", header).group(1)) == N.LORA_OUT_SWIGLU == 1
    assert (N.LORA_OUT_ACT_IDENTITY, N.LORA_OUT_ACT_GELU, N.VIT_TRAIN_OUT_STRIDE) == (0, 1, 4)
    lib = N.load()
    assert lib.ucod_abi_version() == 5
    # the SwiGLU form's own way into the kernel: ucod_lora_out_grad_x with one int of flags behind `act`
    assert re.search(r"\bucod_lora_out_grad_x_ex\s*\(", header) and hasattr(lib, "ucod_lora_out_grad_x_ex")
    res, args = N.SIGNATURES["ucod_lora_out_grad_x_ex"]
    res0, args0 = N.SIGNATURES["ucod_lora_out_grad_x"]
    assert res is res0 and args == args0[:2] + [C.c_int] + args0[2:]
    for name in EX_ENTRY_POINTS:
        assert name in N.SIGNATURES and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
        # one int more than the form it extends, right behind `mlp`
        res, args = N.SIGNATURES[name]
        res0, args0 = N.SIGNATURES[name[:-3]]
        assert res is res0 and args == args0[:2] + [C.c_int] + args0[2:], name


# ------------------------------------------------------------------------------------------------ the size helpers
def train_desc(D=128, heads=2, F=384, L=3, r=2):
    td = N.VitTrainDesc()
    v = td.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps = 2, 3, 70, 70, 14, D, heads, F, L, 640, 1e-6
    td.lora_r, td.lora_scaling = r, 2.0
    return td


def test_ex_size_helpers():
    """Host only: the tables' pointers are made up and never dereferenced."""
    lib = N.load()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    SW, GE, FL = N.UCOD_MLP_SWIGLU, N.UCOD_MLP_GELU, N.LORA_OUT_SWIGLU
    M, D, F, L, r = 2 * 26, 128, 384, 3, 2
    td = train_desc(D=D, F=F, L=L, r=r)
    TM = (C.c_void_p * 9)(*([4096] * 9))
    table = lambda o, f: (C.c_void_p * 12)(*([4096 if o else None] * 2 + [4096 if f else None] * 2) * 3)  # noqa: E731
    train, infer = lib.ucod_vit_train_workspace_bytes_lora_out_ex, lib.ucod_vit_lora_infer_workspace_bytes_lora_out_ex
    for tm in (None, TM):
        base = lib.ucod_vit_train_workspace_bytes_lora_mlp(C.byref(td), SW, tm)
        ibase = lib.ucod_vit_lora_infer_workspace_bytes_lora_mlp(C.byref(td), SW, tm)
        assert base > 0 and ibase > 0
        gw = lib.ucod_lora_out_grad_workspace_bytes(r, F, D)
        assert gw > 0
        assert train(C.byref(td), SW, FL, tm, table(False, True)) == base + up(M * 32) * (L - 1) + up(M * 32) + up(gw)
        assert infer(C.byref(td), SW, FL, tm, table(False, True)) == ibase
        both = max(gw, lib.ucod_lora_out_grad_workspace_bytes(r, D, D))
        assert train(C.byref(td), SW, FL, tm, table(True, True)) == base + 2 * up(M * 32) * (L - 1) + up(M * 32) + up(both)
        # flags 0 (the form that is pinned to refuse), an unknown bit
        for flags in (0, 2, FL | 2, FL | 0x100):
            assert train(C.byref(td), SW, flags, tm, table(False, True)) == 0, flags
            assert infer(C.byref(td), SW, flags, tm, table(False, True)) == 0, flags
        assert lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), SW, tm, table(False, True)) == 0
        # a NULL table: every _ex size is its _lora_out size, with either known flag word; on the GELU MLP the flag changes nothing
        for mlp in (SW, GE):
            for flags in (0, FL):
                assert train(C.byref(td), mlp, flags, tm, None) == lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), mlp, tm, None) > 0
                assert infer(C.byref(td), mlp, flags, tm, None) == lib.ucod_vit_lora_infer_workspace_bytes_lora_out(C.byref(td), mlp, tm, None) > 0
        for o, f in ((True, False), (False, True), (True, True)):
            for flags in (0, FL):
                assert train(C.byref(td), GE, flags, tm, table(o, f)) == lib.ucod_vit_train_workspace_bytes_lora_out(C.byref(td), GE, tm, table(o, f)) > 0
    # vith16plus's hidden width, a width that is no multiple of 128, a rank beyond 8
    for bad in (train_desc(D=1280, heads=20, F=5120), train_desc(F=344), train_desc(r=9)):
        assert train(C.byref(bad), SW, FL, None, table(False, True)) == 0 and infer(C.byref(bad), SW, FL, None, table(False, True)) == 0
    # ViT-g and vits16plus are inside the limits
    for ok in (train_desc(D=1536, heads=24, F=4096), train_desc(D=384, heads=6, F=1536)):
        assert train(C.byref(ok), SW, FL, None, table(False, True)) > 0


# ------------------------------------------------------------------------------------------------ target parsing
ALL = dict(allow_out=True, allow_swiglu_out=True)


@pytest.mark.parametrize("targets,want", [
    (["weights_out"], ((False, False, False), None, ("weights_out",))),
    (["dense", "weights_out"], ((False, False, False), None, ("dense", "weights_out"))),
    (["query", "key", "value", "weights_in", "dense", "weights_out"], ((True, True, True), "weights_in", ("dense", "weights_out"))),
    (["mlp.weights_out", "attention.value"], ((False, False, True), None, ("weights_out",))),
    (["query", "key", "value"], ((True, True, True), None, ())),
])
def test_all_opt_ins_accept_weights_out(targets, want):
    assert lora_targets(targets, "swiglu", 3, **ALL) == want
    assert lora_targets(targets, "swiglu", 3, hidden=4096, **ALL) == want
    assert lora_targets(None, "swiglu", 3, **ALL) == ((True, True, True), None, ())
    # on a GELU checkpoint the new flag changes nothing
    assert lora_targets(["dense", "fc2"], "gelu", 3, **ALL) == lora_targets(["dense", "fc2"], "gelu", 3, allow_out=True)


@pytest.mark.parametrize("layer_path", ["model.layer.", "layer."])
def test_all_opt_ins_accept_the_gated_down_proj(layer_path):
    assert lora_targets_dinov3(["q_proj", "o_proj", "down_proj"], True, 3, layer_path, **ALL) == ((True, False, False), ("o_proj", "down_proj"))
    assert lora_targets_dinov3(["down_proj"], True, 3, layer_path, hidden=1536, **ALL) == ((False, False, False), ("down_proj",))
    assert lora_targets_dinov3(["down_proj"], False, 3, layer_path, **ALL) == lora_targets_dinov3(["down_proj"], False, 3, layer_path, allow_out=True)
    assert lora_targets_dinov3(None, True, 3, layer_path, **ALL) == ((True, True, True), ())


def test_allow_out_alone_keeps_todays_refusal():
    for call in (lambda: lora_targets(["query", "weights_out"], "swiglu", 2, allow_out=True),
                 lambda: lora_targets_dinov3(["q_proj", "down_proj"], True, 2, allow_out=True)):
        with pytest.raises(NotImplementedError, match="not built") as e:
            call()
        assert "recomputed from the interleaved, padded [M, 2F] pre-activation" in str(e.value) and "leading-dimension" not in str(e.value)
        assert "allow_swiglu_out" in str(e.value)                  # ... and names the way in
    # everything off: the message of old
    with pytest.raises(NotImplementedError) as e:
        lora_targets(["weights_out"], "swiglu", 2)
    assert _REFUSED["weights_out"] in str(e.value) and "leading-dimension" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        lora_targets_dinov3(["q_proj", "down_proj"], True, 2)
    assert str(e.value) == f"LoRA target module 'down_proj' (model.layer.0.mlp.down_proj) is not built: {_REFUSED3['down_proj']}"


def test_the_new_opt_in_needs_allow_out():
    for call in (lambda: lora_targets(["weights_out"], "swiglu", 2, allow_swiglu_out=True), lambda: lora_targets(None, "swiglu", 2, allow_swiglu_out=True),
                 lambda: lora_targets_dinov3(["down_proj"], True, 2, allow_swiglu_out=True)):
        with pytest.raises(ValueError, match="allow_out"):
            call()


def test_what_this_work_does_not_build_stays_refused():
    for name in ("up_proj", "gate_proj", "patch_embeddings"):
        with pytest.raises(NotImplementedError) as e:
            lora_targets_dinov3(["q_proj", name], True, 2, **ALL)
        assert _REFUSED3[name] in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        lora_targets(["query", "projection"], "swiglu", 2, **ALL)
    assert _REFUSED["projection"] in str(e.value)
    # vith16plus: hidden width 5120, refused by the parser -- before anything touches a device -- with the true reason
    with pytest.raises(NotImplementedError, match=r"K = 5120") as e:
        lora_targets_dinov3(["q_proj", "down_proj"], True, 2, hidden=5120, **ALL)
    assert "4096" in str(e.value) and "pre-activation" not in str(e.value)
    with pytest.raises(NotImplementedError, match=r"K = 4224"):
        lora_targets(["weights_out"], "swiglu", 2, hidden=4100, **ALL)
    assert lora_targets_dinov3(["q_proj", "o_proj"], True, 2, hidden=5120, **ALL) == ((True, False, False), ("o_proj",))      # (its o_proj is fine)


# ------------------------------------------------------------------------------------------------ the restatement and the goldens
def golden(tag):
    return np.load(os.path.join(ROOT, "tests", "golden", f"g24_lora_swiglu_out_{tag}.npz"))


@pytest.mark.parametrize("tag", RS.G24_TAGS)
def test_restatement_equals_transformers(tag):
    import dinov3_ref as R3
    z = golden(tag)
    assert str(z["sd_sha256"]) == R3.weights_sha256(RS.g24_state_dict(tag)) and int(z["input_seed"]) == RS.G24_INPUT_SEED[tag]
    lora = RS.g24_lora(tag)
    x, dkey = RS.g24_inputs(tag)
    assert np.array_equal(z["x"], x.numpy()) and np.array_equal(z["dkey"], dkey.numpy())
    names = sorted(k[5:] for k in z.files if k.startswith("grad/"))
    assert names == sorted(lora) and all(np.array_equal(z["lora/" + n], lora[n].numpy()) for n in names)
    # every module this work makes reachable is in the file, with HF shapes (A of the MLP output projection [r, F0], unpadded)
    lay = RS.layer_path(lora)
    for t in RS.G24_TARGETS[tag]:
        assert f"{lay}0.{RS.PATHS[t]}.lora_A.weight" in lora, t
    out_leaf = RS.OUT_LEAVES[RS.G24_FAMILY[tag]][1]
    F0 = {"dinov2": 344, "gated": 384}[tag]
    assert tuple(lora[f"{lay}0.{RS.PATHS[out_leaf]}.lora_A.weight"].shape) == (RS.G24_R, F0)
    key, grads = RS.g24_grads(tag, x, lora, dkey)
    assert rel_l2(key, torch.from_numpy(z["key"])) < 1e-9
    for n in names:
        g = torch.from_numpy(z["grad/" + n])
        if float(g.abs().max()) == 0.0:
            assert float(grads[n].abs().max()) == 0.0, n
        else:
            assert rel_l2(grads[n], g) < 1e-9, n


@pytest.mark.parametrize("tag", RS.G24_TAGS)
def test_fault_distances_are_three_gpu_bars(tag):
    """The stored distance of every fault on the tensors it touches against the bar the GPU test holds that tensor to (lora_swiglu_out_ref.grad_bar); one fault is
    recomputed to show that the stored figures are the restatement's."""
    z = golden(tag)
    names = sorted(k[5:] for k in z.files if k.startswith("grad/"))
    for f in RS.FAULTS:
        hit = RS.touched(tag, f, names)
        assert hit or not RS.TOUCHES[RS.G24_FAMILY[tag]][f]
        for n in hit:
            assert float(z[f"f_{f}/{n}"]) >= 3.0 * RS.grad_bar(z, n), (f, n, float(z[f"f_{f}/{n}"]), RS.grad_bar(z, n))
    assert RS.touched(tag, "no_forward", names) and RS.touched(tag, "da_silu", names)
    assert bool(RS.touched(tag, "no_dg", names)) == (tag == "dinov2")
    x, dkey = RS.g24_inputs(tag)
    _, bad = RS.g24_grads(tag, x, RS.g24_lora(tag), dkey, fault="da_silu")
    for n in RS.touched(tag, "da_silu", names):
        assert abs(rel_l2(bad[n], torch.from_numpy(z["grad/" + n])) - float(z[f"f_da_silu/{n}"])) < 1e-9


def test_mask_helper_draws_over_the_padded_width():
    m = RS.out_masks(5, 3, 52, 128, 344, 0.5)
    assert m[(1, "weights_out")].shape[-1] == 384 and m[(1, "dense")].shape[-1] == 128 and RS.padded(344) == 384 and RS.padded(384) == 384
    # the restatement takes the first F0 columns: the same forward as with the mask cut by hand
    x1, x2 = torch.randn(52, 344, dtype=torch.float64), torch.randn(52, 344, dtype=torch.float64)
    sd = {"w.weight": torch.randn(128, 344, dtype=torch.float64), "w.bias": torch.zeros(128, dtype=torch.float64),
          "w.lora_A.weight": torch.randn(2, 344, dtype=torch.float64), "w.lora_B.weight": torch.randn(128, 2, dtype=torch.float64)}
    full = m[(1, "weights_out")].reshape(52, 384)
    assert torch.equal(RS.swiglu_out_linear(x1, x2, sd, "w", 2.0, full), RS.swiglu_out_linear(x1, x2, sd, "w", 2.0, full[:, :344].contiguous()))


# ------------------------------------------------------------------------------------------------ the state dict
def arena_only_engine(sd, targets, seed):
    """A ViTLoRAEngine with the arena and the names its state-dict methods use, and nothing else: the constructor uploads the backbone to a GPU, which this
    machine may not have.  Layout as the constructor lays it out (tests/test_gpu_lora_swiglu_out.py checks the real engine against the same dict)."""
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine, lora_layout
    from ucod_dpl_amd.swiglu import padded_hidden
    e = object.__new__(ViTLoRAEngine)
    e.device, e.D, e.L, e.r, e.mlp = torch.device("cpu"), 128, 3, 2, N.UCOD_MLP_SWIGLU
    e.F = padded_hidden(sd["encoder.layer.0.mlp.weights_out.weight"].shape[1])
    e._adopt(*lora_layout(sd, e.r, targets, **ALL))
    e.lora = torch.randn(e.L, e.numel, generator=torch.Generator().manual_seed(seed))  # (every element nonzero: a column the loader does not write shows)
    e.lora_grad = torch.zeros_like(e.lora)
    e.repack = lambda: None
    return e


def test_state_dict_round_trip_with_a_padded_hidden_width():
    """F0 = 344 in a padded arena row of F = 384: the padded columns load as zeros and are absent from the dict."""
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine
    sd = RS.g24_state_dict("dinov2")
    targets = ["value", "weights_in", "dense", "weights_out"]
    eng = arena_only_engine(sd, targets, 1)
    D, r, L = 128, 2, 3
    assert (eng.F, eng._F0, eng.out_targets) == (384, 344, (True, True))
    assert eng.lora.shape == (L, 6 * r * D + r * (D + 2 * 384) + r * 2 * D + r * (384 + D))
    assert eng.out_off[1] == eng.lora.shape[1] - r * (384 + D)                  # behind everything the row held
    sa, sb = eng._out_slices(1)
    lora = RS.lora_for(sd, ("value", "weights_in", "dense", "weights_out"), seed=9)
    assert sorted(eng.lora_state_dict()) == sorted(lora)
    assert eng.lora_state_dict()["encoder.layer.1.mlp.weights_out.lora_A.weight"].shape == (r, 344)
    eng.load_lora_state_dict(lora)
    a1 = eng.lora[:, sa].reshape(L, r, 384)
    assert float(a1[:, :, 344:].abs().max()) == 0.0 and torch.equal(a1[1, :, :344], lora["encoder.layer.1.mlp.weights_out.lora_A.weight"])
    got = eng.lora_state_dict()
    for k, v in lora.items():
        assert got[k].shape == v.shape and torch.equal(got[k], v), k
    assert got["encoder.layer.1.mlp.weights_out.lora_A.weight"].shape == (r, 344) and got["encoder.layer.1.mlp.weights_out.lora_B.weight"].shape == (D, r)
    grads = eng.lora_state_dict(grads=True)
    assert grads["encoder.layer.0.mlp.weights_out.lora_A.weight"].shape == (r, 344)
    other = arena_only_engine(sd, targets, 2)
    other.load_lora_state_dict(got)
    for m in (0, 1):
        for sl in eng._out_slices(m):
            assert torch.equal(other.lora[:, sl], eng.lora[:, sl])
    bad = dict(lora)
    bad["encoder.layer.0.mlp.weights_out.lora_A.weight"] = torch.zeros(r, 384)    # the padded shape is not a state-dict shape
    with pytest.raises(ValueError, match="lora_A has shape"):
        eng.load_lora_state_dict(bad)
    with pytest.raises(KeyError, match="does not target"):
        arena_only_engine(sd, ["value", "dense"], 3).load_lora_state_dict(lora)
    # the constructor's opt-ins (all raised before anything touches a device): every one of them is needed, and without the new one the refusal of old stands
    with pytest.raises(ValueError, match="allow_out"):
        ViTLoRAEngine(sd, heads=2, device="cpu", allow_swiglu=True, target_modules=targets, allow_swiglu_out=True)
    with pytest.raises(ValueError, match="allow_swiglu"):
        ViTLoRAEngine(sd, heads=2, device="cpu", target_modules=targets, **ALL)
    with pytest.raises(NotImplementedError, match="pre-activation"):
        ViTLoRAEngine(sd, heads=2, device="cpu", allow_swiglu=True, target_modules=targets, allow_out=True)
    import dinov3_ref as R3
    with pytest.raises(ValueError, match="allow_rope"):
        ViTLoRAEngine(R3.g22_state_dict("gated"), heads=2, device="cpu", eps=1e-5, allow_swiglu=True, target_modules=["down_proj"], **ALL)
