"""CPU: the host side of LoRA ``bias="lora_only"`` (models/modules/full_model.py:53,66 hands ``bias`` to peft) -- the refusals of ``load_lora``, the new names of
native.py against include/ucod_dpl.h, the size helpers, the arena layout (which slots exist, their order, zeros where no gradient can arrive), the SwiGLU bias in
and out of the engine's padded order, the adapter folder, and the strength of tests/lora_bias_ref.py's measure against the four faults a bias backward can have."""
import ctypes as C
import json
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_golden, sub
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTLoRAEngine, _prepare_mlp, check_lora_bias, lora_layout, normalize_state_dict
import dinov3_ref as R3
import lora_bias_ref as RB
import lora_out_ref as RO
import lora_swiglu_out_ref as RS
import registers_ref as RR

NEW = ("ucod_colsum_det_workspace_bytes", "ucod_colsum_det", "ucod_vit_train_workspace_bytes_lora_bias", "ucod_vit_backward_lora_bias")


# ------------------------------------------------------------------------------------------------ refusals
def test_load_lora_refuses_all_and_unknown_modes_before_any_device_call():
    """(the state dict is None: anything that touched it, let alone a device, would fail in another way)"""
    from ucod_dpl_amd.models.modules.full_model import load_lora
    with pytest.raises(NotImplementedError, match="LayerNorm backward.*no gradient of beta"):
        load_lora(types.SimpleNamespace(bias="all"), None, heads=2)
    with pytest.raises(ValueError, match="must be one of.*'typo'"):
        load_lora(types.SimpleNamespace(bias="typo"), None, heads=2)
    with pytest.raises(NotImplementedError, match="bias='all' is not built"):
        ViTLoRAEngine(None, heads=2, device="cpu", bias="all")
    with pytest.raises(ValueError, match="LoraConfig.bias"):
        ViTLoRAEngine(None, heads=2, device="cpu", bias=None)
    assert check_lora_bias("none") == "none" and check_lora_bias("lora_only") == "lora_only"


# ------------------------------------------------------------------------------------------------ header, bindings, size helpers
def test_new_names_sit_at_the_numbers_of_the_header():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert int(re.search(r"#define UCOD_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION == 5
    assert int(re.search(r"#define UCOD_VIT_TRAIN_BIAS_STRIDE (\d+)", header).group(1)) == N.VIT_TRAIN_BIAS_STRIDE == len(N.VIT_TRAIN_BIAS_SLOTS) == 6
    assert N.VIT_TRAIN_BIAS_SLOTS == ("gb_q", "gb_k", "gb_v", "gb_m", "gb_o", "gb_2")
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
        assert "full_model.py:53,66" in header[:header.index(name + "(")].rsplit("*/", 2)[-2], name          # the comment in front of the declaration cites the reference
    # the new tier = the _lora_out_ex form plus one table, behind the output modules' one
    for new, old in (("ucod_vit_train_workspace_bytes_lora_bias", "ucod_vit_train_workspace_bytes_lora_out_ex"), ("ucod_vit_backward_lora_bias", "ucod_vit_backward_lora_out_ex")):
        (res, args), (res0, args0) = N.SIGNATURES[new], N.SIGNATURES[old]
        k = args0.index(C.c_void_p) if C.c_void_p in args0 else len(args0)
        assert res is res0 and args == args0[:k] + [C.POINTER(C.c_void_p)] + args0[k:], new


def train_desc(D=128, heads=2, F=512, L=3, r=2):
    td = N.VitTrainDesc()
    v = td.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps = 2, 3, 70, 70, 14, D, heads, F, L, 640, 1e-6
    td.lora_r, td.lora_scaling = r, 2.0
    return td


def test_size_helpers_and_host_side_refusals():
    """Host only: the tables' pointers are made up and never dereferenced; every refused call returns before a launch."""
    lib = N.load()
    size, run = lib.ucod_colsum_det_workspace_bytes, lib.ucod_colsum_det
    # slabs = min(128, ceil(M / 64)), a function of M alone
    for M, slabs in ((1, 1), (64, 1), (65, 2), (111, 2), (2740, 43), (8192, 128), (8193, 128), (43840, 128)):
        for n in (8, 128, 2304):
            assert size(M, n) == slabs * n * 4, (M, n)
    for M, n in ((0, 128), (-1, 128), (4, 0), (4, 4), (4, 12), (4, 129), (4, -8)):
        assert size(M, n) == 0, (M, n)
    p, wb = 4096, size(111, 128)
    ok = dict(x=p, elem=N.ROPE_ELEM_HALF, M=111, n=128, ld=192, scale=None, out=p, ws=p, wb=wb)
    call = lambda **kw: run(*[{**ok, **kw}[k] for k in ("x", "elem", "M", "n", "ld", "scale", "out", "ws", "wb")], None)  # noqa: E731
    bad = {"null x": dict(x=None), "null out": dict(out=None), "null workspace": dict(ws=None), "M < 1": dict(M=0), "N % 8": dict(n=100), "N = 0": dict(n=0),
           "ld < N": dict(ld=120), "misaligned ld": dict(ld=132), "misaligned ld, f32": dict(elem=N.ROPE_ELEM_F32, ld=130), "small workspace": dict(wb=wb - 4),
           "unknown elem": dict(elem=2), "misaligned x": dict(x=p + 8), "misaligned out": dict(out=p + 2)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    # the driver's tier: a NULL table is the _lora_out_ex size; a table adds the partials of the wider of the two buffer shapes, behind everything else
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    M, D, F, L = 2 * 26, 128, 512, 3
    td = train_desc(D=D, F=F, L=L)
    TB = (C.c_void_p * (6 * L))(*([4096] * (6 * L)))
    TM = (C.c_void_p * 9)(*([4096] * 9))
    TO = (C.c_void_p * 12)(*([4096] * 12))
    ex, new = lib.ucod_vit_train_workspace_bytes_lora_out_ex, lib.ucod_vit_train_workspace_bytes_lora_bias
    for mlp, n1 in ((N.UCOD_MLP_GELU, F), (N.UCOD_MLP_SWIGLU, 2 * F)):
        for tm in (None, TM):
            for to in (None, TO):
                flags = N.LORA_OUT_SWIGLU if (to is not None and mlp == N.UCOD_MLP_SWIGLU) else 0
                base = ex(C.byref(td), mlp, flags, tm, to)
                assert base > 0 and new(C.byref(td), mlp, flags, tm, to, None) == base
                assert new(C.byref(td), mlp, flags, tm, to, TB) == base + up(max(size(M, 3 * D), size(M, n1)))
    assert new(C.byref(td), 7, 0, None, None, TB) == 0 and new(C.byref(td), N.UCOD_MLP_GELU, 2, None, None, TB) == 0       # unknown MLP kind / flag bit, as ever
    assert lib.ucod_vit_backward_lora_bias(C.byref(td), 0, 0, None, None, None, None, TB, None, None, 0, None) == -1


# ------------------------------------------------------------------------------------------------ the arena
def host_engine(sd, targets, bias="lora_only", seed=1, **allow):
    """A ViTLoRAEngine with what the constructor derives on the host -- its own ``lora_layout`` / ``_adopt`` / ``_bias_init_arena`` -- and its arena and bias
    vectors on the CPU: the constructor itself uploads the backbone to a GPU, which this machine may not have (tests/test_gpu_lora_bias.py checks real engines
    against the same expectations)."""
    e = object.__new__(ViTLoRAEngine)
    e.mlp, c = _prepare_mlp(normalize_state_dict(sd))
    e.device, e.r, e.L, e.D, e.F = torch.device("cpu"), 2, len(c["layers"]), c["patch_w"].shape[0], c["layers"][0]["fc2_w"].shape[1]
    e._adopt(*lora_layout(sd, e.r, targets, bias, **allow), bias)
    e.base_numel = e.numel - e.bias_numel
    if e.bias_numel:
        e._bias_flat = torch.stack([torch.cat([l[k].float() for k in ("qkv_b", "fc1_b", "proj_b", "fc2_b")]) for l in c["layers"]])
    e.lora = torch.randn(e.L, e.numel, generator=torch.Generator().manual_seed(seed))     # (every element nonzero: a slot the constructor's code does not write shows)
    e._bias_init_arena()
    e.lora_grad = torch.zeros_like(e.lora)
    e.lora_dropout, e.scaling = 0.05, 2.0
    e.repack = e._repack_bias                    # (the host half of repack(): arena -> bias vectors)
    return e, c


def G8():
    """The D = 128 GELU model of the LoRA tests (3 layers, hidden width 512)."""
    return sub(load_golden("g8_dinov2_native"), "sd.")


@pytest.mark.parametrize("targets,allow,want", [
    (["query", "key", "value"], {}, (True, True, True, False, False, False)),
    (["key"], {}, (False, True, False, False, False, False)),
    (["query", "value", "dense"], dict(allow_out=True), (True, False, True, False, True, False)),
    (["query", "key", "value", "fc1", "dense", "fc2"], dict(allow_out=True), (True,) * 6),
    (["fc1", "value"], {}, (False, False, True, True, False, False)),
])
def test_arena_layout_on_dinov2(targets, allow, want):
    """The row grows behind everything it held; slots exist for the targeted modules only, in the order q, k, v, MLP input, attention output, MLP output; they start
    at the checkpoint's values, except the last layer's non-key slots, which hold zeros."""
    sd = G8()
    e, c = host_engine(sd, targets, **allow)
    D, F, L = 128, 512, 3
    sizes = (D, D, D, F, D, D)
    assert (e.D, e.N1, e.L) == (D, F, L) and e.bias == "lora_only"
    assert tuple(o is not None for o in e.bias_off) == want
    expect, at = [], e.base_numel
    for on, n in zip(want, sizes):
        expect.append(at if on else None)
        at += n if on else 0
    assert list(e.bias_off) == expect and e.lora.shape == (L, at) and e.bias_numel == at - e.base_numel
    none, _ = host_engine(sd, targets, bias="none", **allow)
    assert none.lora.shape == (L, e.base_numel) and none.bias == "none" and none.bias_numel == 0 and none._bias_table(none.lora_grad) is None
    src = ("qkv_b", "qkv_b", "qkv_b", "fc1_b", "proj_b", "fc2_b")
    for j, o in enumerate(e.bias_off):
        if o is None:
            continue
        for i in range(L):
            ck = c["layers"][i][src[j]].float()
            ck = ck[j * D:(j + 1) * D] if j < 3 else ck
            if i == L - 1 and j != 1:
                assert float(e.lora[i, o:o + sizes[j]].abs().max()) == 0.0 and e._bias_frozen(i, j), (i, j)
                assert torch.equal(e._bias_value(i, j), ck), (i, j)                  # ... and every reader takes the checkpoint's value
            else:
                assert torch.equal(e.lora[i, o:o + sizes[j]], ck) and not e._bias_frozen(i, j), (i, j)
    # what lies in front of the biases is untouched by the new code
    assert torch.equal(e.lora[:, :e.base_numel], torch.randn(L, e.lora.shape[1], generator=torch.Generator().manual_seed(1))[:, :e.base_numel])
    # state dict: the LoRA matrices plus {layer path}{i}.{module}.bias of the trained ones; the frozen slots read as the checkpoint
    got = e.lora_state_dict()
    bias_keys = sorted(k for k in got if k.endswith(".bias"))
    assert bias_keys == sorted(RB.bias_names(sd, [t.split(".")[-1] for t in targets]))
    for k in bias_keys:
        assert torch.equal(got[k], sd[k]), k
    grads = e.lora_state_dict(grads=True)
    assert sorted(grads) == sorted(got) and all(float(grads[k].abs().max()) == 0.0 for k in bias_keys)
    # round trip through a perturbed dict, into an engine with another arena
    moved = {**got, **RB.perturbed_biases(sd, [t.split(".")[-1] for t in targets])}
    other, _ = host_engine(sd, targets, seed=2, **allow)
    other.load_lora_state_dict(moved)
    back = other.lora_state_dict()
    assert all(torch.equal(back[k], moved[k]) for k in moved)
    for j, o in enumerate(other.bias_off):                                           # a frozen slot's arena entry stays an exact zero whatever was loaded
        if o is not None and j != 1:
            assert float(other.lora[L - 1, o:o + sizes[j]].abs().max()) == 0.0
    with pytest.raises(KeyError):
        other.load_lora_state_dict({k: v for k, v in moved.items() if k != bias_keys[0]})
    with pytest.raises(ValueError, match="has shape"):
        other.load_lora_state_dict({**moved, bias_keys[0]: torch.zeros(7)})


def test_a_module_without_a_bias_gets_no_parameter():
    """DINOv3 ``k_proj`` (key_bias = False): [k_proj] with bias="lora_only" is the engine without the argument; [q, k, v, o_proj, down_proj] trains four biases."""
    sd = R3.g22_state_dict("g46")
    assert "model.layer.0.attention.k_proj.bias" not in sd and "model.layer.0.attention.q_proj.bias" in sd
    e, _ = host_engine(sd, ["k_proj"])
    none, _ = host_engine(sd, ["k_proj"], bias="none")
    assert e.bias_off == (None,) * 6 and e.bias_numel == 0 and e._bias_flat is None and e._bias_table(e.lora_grad) is None
    assert e.lora.shape == none.lora.shape and torch.equal(e.lora, none.lora) and sorted(e.lora_state_dict()) == sorted(none.lora_state_dict())
    e, _ = host_engine(sd, ["q_proj", "k_proj", "v_proj", "o_proj", "down_proj"], allow_out=True)
    assert tuple(o is not None for o in e.bias_off) == (True, False, True, False, True, True)
    assert sorted(k for k in e.lora_state_dict() if k.endswith(".bias")) == sorted(RB.bias_names(sd, ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")))
    assert not any("k_proj.bias" in k for k in e.lora_state_dict())
    # the whole last layer is frozen there: no bias of it can receive a gradient
    for j, o in enumerate(e.bias_off):
        if o is not None:
            assert float(e.lora[e.L - 1, o:o + 128].abs().max()) == 0.0


def test_swiglu_bias_round_trip_with_zero_padding():
    """F0 = 344 in the engine's padded (384), interleaved order: the arena slot holds 2 x 384 values with zeros on the padding; outside it is HF's [688]."""
    sd = RS.g24_state_dict("dinov2")
    targets = ["value", "weights_in", "weights_out"]
    e, c = host_engine(sd, targets, allow_out=True, allow_swiglu_out=True)
    assert (e.F, e._F0, e.N1) == (384, 344, 768) and tuple(o is not None for o in e.bias_off) == (False, False, True, True, False, True)
    o = e.bias_off[3]
    assert torch.equal(e.lora[0, o:o + 768], c["layers"][0]["fc1_b"].float())
    pad = e.lora[0, o:o + 768].reshape(-1, 2, 4)[344 // 4:]                           # blocks of 4 hidden units: x1 | x2; units 344 .. 383 are padding
    assert pad.shape == (10, 2, 4) and float(pad.abs().max()) == 0.0
    got = e.lora_state_dict()
    name = "encoder.layer.1.mlp.weights_in.bias"
    assert got[name].shape == (688,) and torch.equal(got[name], sd[name]) and torch.equal(got["encoder.layer.1.mlp.weights_out.bias"], sd["encoder.layer.1.mlp.weights_out.bias"])
    new = torch.randn(688, generator=torch.Generator().manual_seed(4))
    e.load_lora_state_dict({**got, name: new})
    row = e.lora[1, o:o + 768].reshape(-1, 2, 4)
    assert float(row[86:].abs().max()) == 0.0 and torch.equal(row[:86, 0].reshape(-1), new[:344]) and torch.equal(row[:86, 1].reshape(-1), new[344:])
    assert torch.equal(e.lora_state_dict()[name], new)
    with pytest.raises(ValueError, match="has shape"):
        e.load_lora_state_dict({**got, name: torch.zeros(768)})                     # the padded shape is not a state-dict shape


# ------------------------------------------------------------------------------------------------ the adapter folder
def test_adapter_round_trip_and_mismatch(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.models.modules.full_model import load_lora_adapter, save_lora_adapter
    sd = G8()
    targets = ["query", "value", "dense"]
    e, _ = host_engine(sd, targets, allow_out=True)
    e.load_lora_state_dict({**e.lora_state_dict(), **RB.perturbed_biases(sd, ("query", "value", "dense"))})
    folder = save_lora_adapter(e, str(tmp_path / "lora"))
    cfg = json.load(open(os.path.join(folder, "adapter_config.json")))
    assert cfg["bias"] == "lora_only" and cfg["target_modules"] == ["query", "value", "dense"]
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    pre = "base_model.model.ViT.encoder.layer."
    assert sorted(tensors) == sorted(pre + k[len("encoder.layer."):] for k in e.lora_state_dict())
    assert torch.equal(tensors[pre + "1.attention.output.dense.bias"], e.lora_state_dict()["encoder.layer.1.attention.output.dense.bias"])
    other, _ = host_engine(sd, targets, seed=9, allow_out=True)
    assert not torch.equal(other.lora, e.lora)
    load_lora_adapter(other, folder)
    a, b = other.lora_state_dict(), e.lora_state_dict()              # (the random host arenas differ where no module is targeted: compare what is)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in b)
    assert torch.equal(other.lora[:, e.base_numel:], e.lora[:, e.base_numel:]) and torch.equal(other._bias_flat, e._bias_flat)
    none, _ = host_engine(sd, targets, bias="none", allow_out=True)
    with pytest.raises(ValueError, match=r"bias is 'lora_only' .* 'none' in the engine"):
        load_lora_adapter(none, folder)
    plain = save_lora_adapter(none, str(tmp_path / "plain"))
    assert json.load(open(os.path.join(plain, "adapter_config.json")))["bias"] == "none"
    assert not any(k.endswith(".bias") for k in load_file(os.path.join(plain, "adapter_model.safetensors")))
    with pytest.raises(ValueError, match=r"bias is 'none' .* 'lora_only' in the engine"):
        load_lora_adapter(other, plain)


# ------------------------------------------------------------------------------------------------ the checker
def test_the_measure_tells_the_four_faults_from_the_truth():
    """On the reference alone (f64, CPU), the R = 4 registers model with all six modules targeted: each fault lands at least three bars (3 x 4e-2) from the truth
    under ``lora_bias_ref.errors``; the truth itself is at zero; the key bias below the last layer has a zero gradient (softmax ignores a constant added to all
    keys), the last layer's is the largest of all."""
    sd = RR.g21_state_dict("native")
    targets = ("query", "key", "value", "fc1", "dense", "fc2")
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen)
    full = {**sd, **RO.lora_for(sd, targets)}
    key, lg, rows = RB.grads(img, full, 2, dkey, 2.0, targets)
    tok, lead = RB.geometry(img, sd)
    assert (tok, lead) == (30, 5) and len(rows) == 18 and all(v.shape[:2] == (3, 30) for v in rows.values())
    # the LoRA gradients and the key are those of the restatement without bias leaves
    key0, lg0 = RO.lora_grads(img, full, 2, dkey, 2.0)
    assert torch.equal(key, key0) and all(torch.equal(lg[k], lg0[k]) for k in lg0)
    ref = RB.bias_grads(rows, full, lead)
    assert max(RB.errors(ref, ref, full).values()) == 0.0
    norm = {k: float(v.norm()) for k, v in ref.items()}
    layer = max(norm[k] for k in norm if k.startswith("encoder.layer.0."))
    assert norm["encoder.layer.0.attention.attention.key.bias"] < 1e-12 * layer and norm["encoder.layer.1.attention.attention.key.bias"] < 1e-12 * layer
    assert norm["encoder.layer.2.attention.attention.key.bias"] == max(norm.values())
    for k in norm:
        if k.startswith("encoder.layer.2.") and ".key." not in k:
            assert norm[k] == 0.0, k
    for fault in RB.FAULTS:
        e = RB.errors(RB.bias_grads(rows, full, lead, fault), ref, full)
        worst = max(e, key=e.get)
        print(f"{fault}: {e[worst]:.3f} ({worst})")
        assert e[worst] >= 3 * RB.BAR, (fault, e[worst])
