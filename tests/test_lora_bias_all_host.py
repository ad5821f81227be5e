"""CPU: the library side of LoRA ``bias="all"`` (models/modules/full_model.py:53,66) as far as it runs without a GPU -- the bindings, the size helpers, the refusals
that return before any launch, the workspace rule of the new backward tier, the name rule of the f64 restatement (tests/lora_bias_all_ref.py), the opt-in
(``check_lora_bias(bias, allow_bias_all)``: without it the refusal tests/test_lora_bias_host.py pins is unchanged) and ``lora_layout`` under "all"."""
import ctypes as C
import types

import pytest
import torch

from conftest import load_golden, sub

from ucod_dpl_amd import native as N
from ucod_dpl_amd import vit_engine as V
from ucod_dpl_amd.vit_engine import ViTLoRAEngine, check_lora_bias
from ucod_dpl_amd.models.modules.full_model import load_lora
import dinov3_ref as R3
import lora_bias_ref as RB
import lora_bias_all_ref as RA

NEW = ("ucod_colsum_det_lora_workspace_bytes", "ucod_colsum_det_lora", "ucod_colsum_det_tok_workspace_bytes", "ucod_colsum_det_tok",
       "ucod_vit_train_workspace_bytes_lora_bias_ex", "ucod_vit_backward_lora_bias_ex")


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_bound_in_both_builds(lib):
    f16 = N.load("f16")
    for name in NEW:
        assert name in N.SIGNATURES and hasattr(lib, name) and hasattr(f16, name), name
    assert lib.ucod_abi_version() == 5 and N.VIT_TRAIN_BIAS_STRIDE == 6


def test_all_needs_the_opt_in():
    """Without ``allow_bias_all`` the refusal is what tests/test_lora_bias_host.py pins; with it "all" passes, and the other two values are untouched by it."""
    for pattern in ("LayerNorm backward.*no gradient of beta", "bias='all' is not built"):
        with pytest.raises(NotImplementedError, match=pattern):
            check_lora_bias("all")
        with pytest.raises(NotImplementedError, match=pattern):
            check_lora_bias("all", allow_bias_all=False)
    assert check_lora_bias("all", allow_bias_all=True) == "all"
    for flag in (False, True):
        assert check_lora_bias("none", flag) == "none" and check_lora_bias("lora_only", allow_bias_all=flag) == "lora_only"
        with pytest.raises(ValueError, match="must be one of.*'typo'"):
            check_lora_bias("typo", flag)
    with pytest.raises(NotImplementedError, match="bias='all' is not built"):
        load_lora(types.SimpleNamespace(bias="all"), None, heads=2)
    with pytest.raises(NotImplementedError, match="bias='all' is not built"):
        ViTLoRAEngine(None, heads=2, device="cpu", bias="all")


@pytest.mark.parametrize("targets", [("key",), ("query", "key", "value"), ("query", "key", "value", "fc1", "dense", "fc2")])
def test_lora_layout_under_all(targets):
    """Under "all" every module with a bias in the checkpoint has an offset, targeted or not, and [beta1 | beta2 | b_patch] stand behind them; for the other two
    values the layout is what it was (no norm block, the row as long as before)."""
    sd = sub(load_golden("g8_dinov2_native"), "sd.")
    D, F = 128, sd["encoder.layer.0.mlp.fc1.weight"].shape[0]
    for bias in ("none", "lora_only"):
        _, mods = V.lora_layout(sd, 2, list(targets), bias, allow_out=True)
        assert V.lora_norm_offsets(mods, bias) is None and V.lora_row_numel(mods, bias) == V.lora_row_numel(mods)
        assert [m.bias_off is not None for m in mods] == [bias == "lora_only" and m.targeted for m in mods]
    _, plain = V.lora_layout(sd, 2, list(targets), "none", allow_out=True)
    _, mods = V.lora_layout(sd, 2, list(targets), "all", allow_out=True)
    assert [(m.a, m.b, m.targeted) for m in mods] == [(m.a, m.b, m.targeted) for m in plain]           # the matrices stay where they were
    at = V.lora_row_numel(plain)
    for m, n in zip(mods, (D, D, D, F, D, D)):
        assert m.bias_off == at and m.nb == n
        at += n
    assert V.lora_norm_offsets(mods, "all") == (at, at + D, at + 2 * D) and V.lora_row_numel(mods, "all") == at + 3 * D


def test_lora_layout_under_all_dinov3():
    """DINOv3: k_proj has no bias and gets no offset; the gated MLP's two input modules share the fused slot, and without one of them targeted the mode is refused."""
    sd = R3.g22_state_dict("gated")
    qkv = ["q_proj", "k_proj", "v_proj"]
    _, mods = V.lora_layout(sd, 2, qkv + ["gate_proj"], "all", allow_mlp_in=True)
    assert len(mods) == 7 and mods[1].bias_off is None and all(m.bias_off is not None for j, m in enumerate(mods) if j != 1)
    assert mods[3].bias_off == mods[6].bias_off and (mods[3].targeted, mods[6].targeted) == (True, False)
    with pytest.raises(NotImplementedError, match="gate_proj or up_proj targeted"):
        V.lora_layout(sd, 2, qkv, "all", allow_mlp_in=True)
    with pytest.raises(NotImplementedError, match="gate_proj or up_proj targeted"):
        V.lora_layout(sd, 2, qkv, "all")
    _, mods = V.lora_layout(R3.g22_state_dict("g46"), 2, qkv, "all")
    assert len(mods) == 6 and [m.bias_off is None for m in mods] == [False, True, False, False, False, False]


@pytest.mark.parametrize("M", [1, 64, 65, 2740, 8192, 8193, 43840])
def test_size_helpers(lib, M):
    slabs = min(128, -(-M // 64))
    for D in (128, 384, 768, 1536):
        assert lib.ucod_colsum_det_lora_workspace_bytes(M, D) == slabs * D * 4 == lib.ucod_colsum_det_workspace_bytes(M, D)
    for bad in ((0, 128), (M, 0), (M, 64), (M, 320), (-1, 128)):
        assert lib.ucod_colsum_det_lora_workspace_bytes(*bad) == 0
    for B, tok, first in ((1, M + 1, 1), (2, M + 5, 5), (1, M, 0)):
        assert lib.ucod_colsum_det_tok_workspace_bytes(B, tok, first, 384) == min(128, -(-B * (tok - first) // 64)) * 384 * 4
    for bad in ((0, 30, 1, 128), (2, 30, -1, 128), (2, 30, 30, 128), (2, 30, 31, 128), (2, 30, 1, 100), (2, 0, 0, 128), (65536, 65536, 1, 128)):
        assert lib.ucod_colsum_det_tok_workspace_bytes(*bad) == 0


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns UCOD_EINVAL from the argument check: no device is needed to see it (the pointers are never followed)."""
    M, D = 111, 384
    wsb = lib.ucod_colsum_det_lora_workspace_bytes(M, D)
    drop, bad_p = N.LoraDropout(0.05, 1, 0), N.LoraDropout(1.0, 1, 0)
    ok = dict(dy=0x1000, flags=1, M=M, D=D, t=0x2000, ldt=64, a=0x3000, np=3, r=2, drop=C.byref(drop), out=0x4000, ws=0x5000, wb=wsb)
    order = ("dy", "flags", "M", "D", "t", "ldt", "a", "np", "r", "drop", "out", "ws", "wb")
    bad = {"null dy": dict(dy=None), "null out": dict(out=None), "null workspace": dict(ws=None), "null lora": dict(a=None), "M < 1": dict(M=0), "D % 128": dict(D=320),
           "np = 0": dict(np=0), "np = 4": dict(np=4), "r = 0": dict(r=0), "r = 22, np = 3": dict(r=22), "r = 9, np = 1": dict(np=1, r=9), "r = 9, np = 2": dict(np=2, r=9),
           "ldt < np r": dict(ldt=5), "p = 1": dict(drop=C.byref(bad_p)), "small workspace": dict(wb=wsb - 4), "unknown flag": dict(flags=4), "misaligned dy": dict(dy=0x1002),
           "misaligned lora": dict(a=0x3004), "misaligned out": dict(out=0x4002)}
    for name, kw in bad.items():
        assert lib.ucod_colsum_det_lora(*[{**ok, **kw}[k] for k in order], None) == -1, name
    wst = lib.ucod_colsum_det_tok_workspace_bytes(3, 30, 5, D)
    ok = dict(x=0x1000, elem=N.ROPE_ELEM_HALF, B=3, tok=30, first=5, n=D, ld=448, scale=None, out=0x4000, ws=0x5000, wb=wst)
    order = ("x", "elem", "B", "tok", "first", "n", "ld", "scale", "out", "ws", "wb")
    bad = {"null x": dict(x=None), "null out": dict(out=None), "null workspace": dict(ws=None), "B < 1": dict(B=0), "N % 8": dict(n=380), "ld < N": dict(ld=376),
           "misaligned ld": dict(ld=452), "small workspace": dict(wb=wst - 4), "unknown elem": dict(elem=2), "first < 0": dict(first=-1), "first = tok": dict(first=30),
           "misaligned x": dict(x=0x1008)}
    for name, kw in bad.items():
        assert lib.ucod_colsum_det_tok(*[{**ok, **kw}[k] for k in order], None) == -1, name


def desc(B=2, D=128, heads=2, F=512, L=3, n_reg=0):
    t = N.VitTrainDesc()
    v = t.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps, v.n_reg = B, 3, 70, 70, 14, D, heads, F, L, 640, 1e-6, n_reg
    t.lora_r, t.lora_scaling, t.lora_dropout, t.seed = 2, 2.0, 0.05, 7
    return t


@pytest.mark.parametrize("n_reg", [0, 4])
def test_workspace_of_the_new_tier(lib, n_reg):
    """A NULL norm table adds no byte to the _lora_bias size; with the bias table the norm table's partials fit what that table counted; alone it brings its own
    (the widest of its calls: M rows by D columns)."""
    t = desc(n_reg=n_reg)
    L, D = t.vit.L, t.vit.D
    M = t.vit.B * (26 + n_reg)
    some = (C.c_void_p * (6 * L))(*([0x1000] * (6 * L)))
    TN = (C.c_void_p * (1 + 2 * L))(*([0x1000] * (1 + 2 * L)))
    lead = (C.byref(t), N.UCOD_MLP_GELU, 0, None, None)
    n_ex = lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, None)
    n_tb = lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, some)
    assert 0 < n_ex < n_tb
    assert lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, None, None) == n_ex
    assert lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, some, None) == n_tb
    assert lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, some, TN) == n_tb
    n_tn = lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, None, TN)
    pad = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert n_tn == n_ex + pad(lib.ucod_colsum_det_lora_workspace_bytes(M, D))
    # the refusals of the pass come before anything is enqueued: no image, no workspace
    assert lib.ucod_vit_backward_lora_bias_ex(*lead[:3], None, None, None, None, some, TN, None, None, 0, None) == -1


def test_trained_names_is_pefts_rule_minus_the_final_norm():
    sd = sub(load_golden("g8_dinov2_native"), "sd.")
    lay, L = RB.layer_path(sd), RB.n_layers(sd)
    names = RA.trained_names(sd)
    assert "layernorm.bias" in sd and "layernorm.bias" not in names
    want = [RA.patch_bias_name(sd)] + [f"{lay}{i}.{p}.bias" for i in range(L) for p in
                                       ("norm1", "norm2", "attention.attention.query", "attention.attention.key", "attention.attention.value", "attention.output.dense",
                                        "mlp.fc1", "mlp.fc2")]
    assert names == sorted(want)
    assert set(RA.norm_names(sd)) <= set(names) and len(RA.norm_names(sd)) == 1 + 2 * L
    assert not any("weight" in k or "lambda" in k or "token" in k or "position" in k for k in names)
    sd3 = R3.g22_state_dict("gated")                                # DINOv3: k_proj has no bias; the gated MLP has three Linear modules
    names3 = RA.trained_names(sd3)
    assert not any("k_proj" in k for k in names3) and RA.patch_bias_name(sd3) == "embeddings.patch_embeddings.bias" in names3
    assert "norm.bias" in sd3 and "norm.bias" not in names3
    assert all(torch.is_tensor(sd3[k]) and sd3[k].dim() == 1 for k in names3)


import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def fault_model(tag):
    """(state dict, heads, lora scale, inputs, LoRA matrices with B at 0.5 randn, masks at dropout 0.05 under the driver's keys, targeted paths, the DINOv3 forward?)
    of one test model with q / k / v and the MLP input targeted -- the six models of tests/test_gpu_lora_bias_all.py."""
    from oracle import vit as OV
    import lora_out_ref as RO
    import lora_swiglu_out_ref as RS
    import registers_ref as RR
    import dinov3_lora_mlp_in_ref as RM
    v3 = tag in ("g46", "gated")
    if v3:
        sd, heads, scale = R3.g22_state_dict(tag), R3.G22[tag]["heads"], RM.G26_SCALE
        leaves = ("q_proj", "k_proj", "v_proj") + (("gate_proj", "up_proj") if tag == "gated" else ("up_proj",))
        x, dkey = RM.g26_inputs(tag)
        lora = RM.g26_lora(tag, leaves)
        masks = RM.g26_masks(tag, leaves, x.shape[0] * RB.geometry(x, sd)[0], 99, 0.05)
        paths = tuple(RM.module_path(l) for l in leaves)
    else:
        if tag == "g8":
            sd, heads, x_dkey = sub(load_golden("g8_dinov2_native"), "sd."), 2, RO.case_inputs(2, 128, 70)
        elif tag == "d256":
            sd, heads, L, image, B = RO.d256_state_dict()
            x_dkey = RO.case_inputs(B, 256, image)
        elif tag == "swiglu":
            sd, heads, x_dkey = RS.g24_state_dict("dinov2"), 2, RO.case_inputs(2, 128, 70)
        else:
            gen = torch.Generator().manual_seed(7)
            sd, heads, x_dkey = RR.g21_state_dict("native"), 2, (torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen))
        x, dkey = x_dkey
        scale, mlp_in = 2.0, ("weights_in" if tag == "swiglu" else "fc1")
        leaves = ("query", "key", "value", mlp_in)
        lora = (RS if tag == "swiglu" else RO).lora_for(sd, leaves)
        L, D, rows = RB.n_layers(sd), sd["embeddings.cls_token"].shape[-1], x.shape[0] * RB.geometry(x, sd)[0]
        masks = {(i, nm): OV.lora_dropout_mask(99, i, p, rows, D, 0.05) for i in range(L) for p, nm in enumerate(leaves[:3])}
        masks.update({(i, mlp_in): OV.lora_dropout_mask(99, L + i, 0, rows, D, 0.05) for i in range(L)})
        paths = tuple(RB.PATHS[l] for l in leaves)
    g = torch.Generator().manual_seed(4)
    lora = {k: (0.5 * torch.randn(v.shape, generator=g) if "lora_B" in k else v) for k, v in lora.items()}
    return sd, heads, scale, x, dkey, lora, masks, paths, v3


@functools.lru_cache(maxsize=None)
def fault_distances(tag):
    """{fault: its distance in bars (the looser bar, 5e-2) in the measure the engine is held to} on one model, from f64 autograd alone"""
    sd, heads, scale, x, dkey, lora, masks, paths, v3 = fault_model(tag)
    full = {**sd, **lora}
    lead_names = [k for k in RA.LEAD_TOKENS if k in sd]
    _, g = RA.all_grads(x, full, heads, dkey, scale, masks=masks, gated=v3, extra=lead_names)
    ref = {k: v for k, v in g.items() if k not in lead_names}
    assert max(RA.errors(ref, ref, sd).values()) == 0.0
    branch = RA.lora_branch_of_beta(x, full, heads, dkey, scale, masks=masks, gated=v3)
    lay, L = RB.layer_path(sd), RB.n_layers(sd)
    assert sorted(branch) == sorted([f"{lay}{i}.norm1.bias" for i in range(L)] + [f"{lay}{i}.norm2.bias" for i in range(L - 1)])
    out = {}
    for fault in RA.FAULTS:
        errs = RA.errors(RA.with_fault(ref, sd, paths, fault, branch=branch, lead={k: g[k] for k in lead_names}), ref, sd)
        out[fault] = max(errs.values()) / RB.BAR_LOOSE
    return out


FAULT_MODELS = ("g8", "d256", "swiglu", "reg", "g46", "gated")
# the model each fault is shown on (chosen from the table this test prints: the first on which it lands at least three bars away)
SHOWN = {"beta_without_lora_term": "g8", "patch_all_rows": "g8", "beta1_layer0_dropped": "g8", "last_beta1_dropped": "g8", "untargeted_dropped": "g8"}


def test_the_branch_of_beta_vanishes_with_a():
    """``lora_branch_of_beta`` (the term the fault leaves out) is linear in A: zero at A = 0, non-zero for every LayerNorm with an adapter behind it at the model's A."""
    sd, heads, scale, x, dkey, lora, masks, paths, v3 = fault_model("g8")
    zero_a = {k: (torch.zeros_like(v) if "lora_A" in k else v) for k, v in lora.items()}
    branch0 = RA.lora_branch_of_beta(x, {**sd, **zero_a}, heads, dkey, scale, masks=masks)
    assert all(float(v.abs().max()) == 0.0 for v in branch0.values())
    branch = RA.lora_branch_of_beta(x, {**sd, **lora}, heads, dkey, scale, masks=masks)
    assert all(float(v.abs().max()) > 0.0 for v in branch.values())


@pytest.mark.parametrize("fault", RA.FAULTS)
def test_the_measure_sees_every_fault(fault):
    """On the reference alone (f64; B of the LoRA modules at 0.5 randn, dropout 0.05 under the driver's mask keys, q / k / v and the MLP input targeted): the
    distance of each fault, in bars of 5e-2 (the looser of the two), in the measure tests/test_gpu_lora_bias_all.py holds the engine to, on every test model; on
    the model it is shown on (SHOWN) it is at least three bars.  Recorded:
        beta_without_lora_term   g8 20.0  d256 19.5  swiglu 20.0  reg 20.1  g46 20.0  gated 19.1
        patch_all_rows           g8 72.7  d256 39.7  swiglu  2.1  reg  1.9  g46  2.8  gated  1.6
        the three dropped ones   20.0 on every model (a tensor written as zeros, judged singly)
    patch_all_rows does not reach three bars at pass level on swiglu, reg, g46 and gated (the CLS / register rows carry little of the first state's cotangent
    there): on those models its check is the kernel test, tests/test_gpu_lora_bias_all.py::test_colsum_tok_exact, which holds ucod_colsum_det_tok to f64 bit for bit
    with the excluded rows sixteen times larger than the summed ones."""
    table = {tag: fault_distances(tag)[fault] for tag in FAULT_MODELS}
    print(f"{fault}: " + "  ".join(f"{t} {v:.1f}" for t, v in table.items()) + " bars")
    assert table[SHOWN[fault]] >= 3.0, (fault, table)


# ---- G27: transformers' own module trees (tests/golden/make_golden_lora_bias_all.py)
@pytest.mark.parametrize("tag", RA.G27_TAGS)
def test_trained_names_are_transformers_bias_parameters(tag):
    """peft's rule on HF's own ``named_parameters()``: the helper's names, and the names the engine's module table gives a slot, are the golden's list minus the
    final LayerNorm -- DINOv3's k_proj (no bias), the patch embedding's key and the gated MLP's three Linear modules included.  What torch gives grad = None is what
    the engine treats as frozen: the final LayerNorm and the last layer's biases other than the key's and norm1's."""
    z, sd, heads, lora, scale, x, dkey, v3 = RA.g27(tag)
    assert R3.weights_sha256(sd) == str(z["sd_sha256"]), "the state dict is no longer what the golden was made with"
    names = [str(n) for n in z["names"]]
    final = [n for n in names if n in RA.FINAL_NORMS]
    assert len(final) == 1 and sorted(n for n in names if n not in final) == RA.trained_names(sd)
    assert sorted(names) == sorted(k for k in sd if "bias" in k)
    assert not any("k_proj.bias" in n for n in names) or tag == "dinov2"
    lay, L = RB.layer_path(sd), RB.n_layers(sd)
    none = sorted(n for n in names if int(z["none/" + n]))
    live_last = ("norm1", "key", "k_proj")
    assert none == sorted(final + [n for n in names if n.startswith(f"{lay}{L - 1}.") and RB.leaf_of(n) not in live_last])
    # the engine's module table (host only): every Linear bias of the golden has a slot, and nothing else does
    targets = sorted({k.rsplit(".", 3)[-3] for k in lora})
    lp, mods = V.lora_layout(sd, 2, targets, "all", allow_out=True, allow_swiglu_out=True, allow_mlp_in=True)
    slots = sorted(f"{lp}{i}.{m.path}.bias" for i in range(L) for m in mods if m.bias_off is not None)
    assert slots == sorted(n for n in names if n.startswith(lay) and ".norm" not in n)


@pytest.mark.parametrize("tag", RA.G27_TAGS)
def test_the_restatement_reproduces_g27(tag):
    """tests/lora_bias_all_ref.py's f64 autograd over the project's own forwards against transformers' f64 gradients: to f64 rounding (1e-9 in the
    measure the engine is held to), zeros where torch returns None."""
    z, sd, heads, lora, scale, x, dkey, v3 = RA.g27(tag)
    key, g = RA.all_grads(x, {**sd, **lora}, heads, dkey, scale, gated=v3)
    assert R3.rel_l2(key, torch.from_numpy(z["key"])) < 1e-10
    want = RA.g27_grads(z)
    assert sorted(want) == RA.trained_names(sd)
    for n, w in want.items():
        if int(z["none/" + n]):
            assert float(g[n].abs().max()) == 0.0 and float(w.abs().max()) == 0.0, n
    # (the measure of the GPU tests: each layer's vector, every tensor with at least 1e-3 of it, the patch bias.  Without RoPE the key bias below the last layer
    # has a mathematically zero gradient -- 5e-17 in both, a cancelled sum -- and is judged within its layer's vector, as tests/lora_bias_ref.py explains)
    worst = max(RA.errors({k: v.cpu() for k, v in g.items()}, want, sd).values())
    print(f"G27 {tag}: the restatement's bias gradients, worst rel-L2 {worst:.2e}")
    assert worst < 1e-9
