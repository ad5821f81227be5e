"""CPU: the host side of LoRA ``target_modules`` (models/modules/full_model.py:47-72 hands the list to peft) -- target parsing, the SwiGLU row order of the MLP
module's B matrix, and the f64 restatement the GPU tests compare against (tests/lora_targets_ref.py), pinned on the oracle and on merged-weight autograd."""
import pytest
import torch

from conftest import load_golden, sub
from ucod_dpl_amd import swiglu
from ucod_dpl_amd.vit_engine import lora_targets
import lora_targets_ref as R
from swiglu_ref import random_swiglu_state_dict, swiglu_hidden


# ------------------------------------------------------------------------------------------------ target parsing
def test_default_and_any_order_of_qkv_are_the_same_targets():
    want = ((True, True, True), None)
    assert lora_targets(None) == want
    for order in (["query", "key", "value"], ["value", "query", "key"], ("key", "value", "query"), ["query", "query", "key", "value"]):
        assert lora_targets(order) == want
        assert lora_targets(order, "swiglu", 4) == want


@pytest.mark.parametrize("targets,mlp,want", [
    (["query", "value"], "gelu", ((True, False, True), None)),
    (["value", "query"], "gelu", ((True, False, True), None)),
    (["key"], "gelu", ((False, True, False), None)),
    (["query"], "swiglu", ((True, False, False), None)),
    (["query", "key", "value", "fc1"], "gelu", ((True, True, True), "fc1")),
    (["fc1", "value"], "gelu", ((False, False, True), "fc1")),
    (["value", "weights_in"], "swiglu", ((False, False, True), "weights_in")),
])
def test_accepted_subsets(targets, mlp, want):
    assert lora_targets(targets, mlp, 3) == want


def test_peft_suffix_matching():
    """A module is targeted when its name equals the target or ends in '.' + target."""
    assert lora_targets(["attention.query", "attention.attention.value"], "gelu", 2) == ((True, False, True), None)
    assert lora_targets(["mlp.fc1", "key"], "gelu", 2) == ((False, True, False), "fc1")
    assert lora_targets(["mlp.weights_in", "key"], "swiglu", 2) == ((False, True, False), "weights_in")
    with pytest.raises(NotImplementedError, match="uery"):      # 'uery' is no suffix at a dot: no module has that name
        lora_targets(["uery"])
    with pytest.raises(NotImplementedError, match="every layer"):
        lora_targets(["layer.0.attention.attention.query"], "gelu", 2)
    with pytest.raises(NotImplementedError, match="output.dense"):           # the suffix resolves to the refused module
        lora_targets(["query", "output.dense"])


@pytest.mark.parametrize("name,mlp", [("dense", "gelu"), ("fc2", "gelu"), ("weights_out", "swiglu"), ("weights_out", "gelu"), ("fc2", "swiglu"),
                                      ("projection", "gelu"), ("classifier", "gelu")])
def test_refused_names_raise_with_the_module_named(name, mlp):
    with pytest.raises(NotImplementedError, match=name) as e:
        lora_targets(["query", "key", "value", name], mlp, 2)
    assert "not built" in str(e.value)
    if name in ("dense", "fc2", "weights_out"):
        assert "leading-dimension" in str(e.value)              # ... and the reason


def test_wrong_mlp_key_for_the_mlp_kind_is_a_value_error():
    with pytest.raises(ValueError, match="weights_in"):
        lora_targets(["query", "fc1"], "swiglu")
    with pytest.raises(ValueError, match="fc1"):
        lora_targets(["query", "weights_in"], "gelu")
    with pytest.raises(ValueError, match="empty"):
        lora_targets([])
    with pytest.raises(NotImplementedError, match="regular expression"):
        lora_targets("query")


def test_load_lora_refuses_before_it_touches_the_device():
    """load_lora hands target_modules to the engine, whose first act is the parse: no GPU needed for a refusal; bias and r == 0 stay as they were."""
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.models.modules.full_model import load_lora
    sd = sub(load_golden("g8_dinov2_native"), "sd.")
    with pytest.raises(NotImplementedError, match="dense"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, target_modules=["dense"])), sd, heads=2, device="cpu")
    with pytest.raises(ValueError, match="weights_in"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, target_modules=["query", "weights_in"])), sd, heads=2, device="cpu")
    with pytest.raises(ValueError, match="r == 0"):
        load_lora(CfgNode(dict(r=0, target_modules=["query"])), sd, heads=2, device="cpu")


# ------------------------------------------------------------------------------------------------ SwiGLU row order of B_m
@pytest.mark.parametrize("F0", [344, 4096])
def test_swiglu_lora_b_round_trip_and_zero_padding(F0):
    r = 3
    F = swiglu.padded_hidden(F0)
    assert (F0, F) in ((344, 384), (4096, 4096))
    b = torch.randn(2 * F0, r, generator=torch.Generator().manual_seed(F0))
    e = swiglu.lora_b_to_engine(b)
    assert e.shape == (2 * F, r)
    assert torch.equal(swiglu.lora_b_from_engine(e, F0), b)
    # the engine's rows are those of the weight ``prepare`` permutes: row 8k + e <- x1 unit 4k + e, 8k + 4 + e <- x2 unit 4k + e; padded units are zero rows
    z = e.reshape(F // 4, 2, 4, r)
    units = torch.arange(F).reshape(F // 4, 4)
    live = units < F0
    assert torch.equal(z[:, 0][live], b[:F0]) and torch.equal(z[:, 1][live], b[F0:])
    assert float(z[:, 0][~live].abs().sum()) == 0.0 and float(z[:, 1][~live].abs().sum()) == 0.0
    assert int((~live).sum()) == F - F0
    # the same permutation as the weight's: B rows follow weights_in's rows
    w = torch.randn(2 * F0, 8)
    w_eng, _, _ = swiglu.prepare(w, torch.zeros(2 * F0), torch.zeros(8, F0))
    assert torch.equal(swiglu.lora_b_to_engine(w), w_eng)


# ------------------------------------------------------------------------------------------------ the f64 restatement
def test_restatement_with_qkv_only_equals_the_oracle_on_g12():
    from oracle import vit as OV
    g = load_golden("g12_lora_backbone")
    sd = sub(g, "sd.")
    key_o, g_o = OV.dinov2_lora_grads(g["x"], sd, heads=2, dkey=g["dkey"], lora_scale=2.0)
    key_r, g_r = R.lora_grads(g["x"], sd, 2, g["dkey"], 2.0)
    assert (key_r - key_o.double()).abs().max().item() < 2e-5 * max(1.0, key_o.abs().max().item())
    assert sorted(g_r) == sorted(g_o) and len(g_r) == 18
    for k, ref in g_o.items():
        if float(ref.abs().max()) == 0.0:
            assert float(g_r[k].abs().max()) == 0.0, k
        else:
            assert ((g_r[k] - ref.double()).norm() / ref.double().norm()).item() < 1e-4, k      # f32 rounding of the oracle's own pass
    # ... and on the golden's HF autograd gradients
    for k, v in g_r.items():
        ref = g["grad." + k].double()
        assert (v - ref).norm().item() <= 1e-4 * max(ref.norm().item(), 1e-30), k


def _with_lora(sd, L, D, mods, r, seed):
    gen = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for i in range(L):
        for mod in mods:
            rows = out[f"encoder.layer.{i}.{mod}.weight"].shape[0]
            out[f"encoder.layer.{i}.{mod}.lora_A.weight"] = torch.randn(r, D, generator=gen) / D ** 0.5
            out[f"encoder.layer.{i}.{mod}.lora_B.weight"] = 0.05 * torch.randn(rows, r, generator=gen)
    return out


@pytest.mark.parametrize("kind", ["gelu", "swiglu"])
def test_restatement_with_mlp_lora_equals_merged_weight_autograd(kind):
    D, heads, L, r = 128, 2, 3, 2
    if kind == "swiglu":
        base = random_swiglu_state_dict(D, heads, L, seed=3)
        mods = ("attention.attention.value", "mlp.weights_in")
        assert base["encoder.layer.0.mlp.weights_in.weight"].shape[0] == 2 * swiglu_hidden(D)
    else:
        base = sub(load_golden("g8_dinov2_native"), "sd.")
        mods = ("attention.attention.query", "attention.attention.key", "attention.attention.value", "mlp.fc1")
    sd = _with_lora(base, L, D, mods, r, seed=5)
    gen = torch.Generator().manual_seed(9)
    img, dkey = torch.randn(2, 3, 70, 70, generator=gen), torch.randn(2, D, 5, 5, generator=gen)
    key_a, g_a = R.lora_grads(img, sd, heads, dkey, 2.0)
    key_b, g_b = R.merged_grads(img, sd, heads, dkey, 2.0)
    assert (key_a - key_b).abs().max().item() < 1e-11
    assert len(g_a) == 2 * L * len(mods)
    nonzero = 0
    for k in g_a:
        last = f"layer.{L - 1}." in k and ".key." not in k
        if last:
            assert float(g_a[k].abs().max()) == 0.0 and float(g_b[k].abs().max()) == 0.0, k      # the last layer's query / value / MLP never reach the key map
        else:
            assert float(g_a[k].abs().max()) > 0.0, k
            assert ((g_a[k] - g_b[k]).norm() / g_b[k].norm()).item() < 1e-10, k
            nonzero += 1
    assert nonzero > 0
    # a mask changes the MLP module's answer (the merged route cannot express it): dropout reaches the restatement
    mlp_name = mods[-1].split(".")[-1]
    masks = {(0, mlp_name): (torch.rand(2 * 26, D, generator=gen) > 0.3).double() / 0.7}
    _, g_m = R.lora_grads(img, sd, heads, dkey, 2.0, masks=masks)
    k0 = f"encoder.layer.0.{mods[-1]}.lora_A.weight"
    assert ((g_m[k0] - g_a[k0]).norm() / g_a[k0].norm()).item() > 0.05
