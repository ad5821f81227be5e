"""Host (no GPU): LoRA on DINOv3's MLP input -- ``up_proj``, and ``gate_proj`` / ``up_proj`` of the gated MLP as a pair -- behind ``allow_mlp_in``.

1  The G26 goldens (tests/golden/make_golden_dinov3_lora_mlp_in.py) are what their generator draws, and the restatement tests/dinov3_lora_mlp_in_ref.py reproduces
   transformers' f64 key maps and gradients in them.
2  Every bar the GPU tests use lies under half of the smallest distance that a wrong block structure of the pair (shared_mask, halves_swapped, dense_b) puts
   between the gradients it touches and the truth: a pass with such a fault cannot stay inside.
3  The flag-off surface is today's, word for word; the target resolution, the ``lora_only`` refusal and the width refusal with the flag; the arena layout; the
   HF <-> engine round trip of B per module; the header's and ``native.SIGNATURES``' new entries and the size / refusal paths that run without a device.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from ucod_dpl_amd import native as N
from ucod_dpl_amd import vit_engine as V
from ucod_dpl_amd.swiglu import lora_b_from_engine, lora_b_to_engine, padded_hidden
import dinov3_ref as R3
import dinov3_lora_ref as RL
import dinov3_lora_mlp_in_ref as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
QKV = ["q_proj", "k_proj", "v_proj"]
# the gradients a fault of the pair reaches DIRECTLY, in the layers whose MLP runs (the last layer's does not)
TOUCHES = {"shared_mask": ("up_proj",), "halves_swapped": RM.PAIR, "dense_b": RM.PAIR}


@functools.lru_cache(maxsize=None)
def golden(tag):
    return np.load(os.path.join(GOLDEN, f"g26_dinov3_lora_mlp_in_{tag}.npz")), R3.g22_state_dict(tag)


def set_lora(z, tag, tset):
    names = [k for k in RM.g26_lora(tag, RM.g26_targets(tag, tset))]
    return {k: torch.from_numpy(z["lora/" + k]) for k in names}


# ================================================================================================ 1. the goldens
@pytest.mark.parametrize("tag,tset", [(t, s) for t in RM.G26_TAGS for s in RM.G26_SETS[t]])
def test_goldens_are_what_the_generator_draws_and_the_restatement_meets_them(tag, tset):
    z, sd = golden(tag)
    m = R3.G22[tag]
    x, dkey = RM.g26_inputs(tag)
    assert np.array_equal(z["x"], x.numpy()) and np.array_equal(z["dkey"], dkey.numpy()) and int(z["drop_seed"]) == RM.G26_DROP_SEED
    lora = RM.g26_lora(tag, RM.g26_targets(tag, tset))
    assert all(np.array_equal(z["lora/" + k], v.numpy()) for k, v in lora.items())
    # (the weights are pinned through the key map, not byte for byte: trunc_normal_'s erfinv differs in the last bit between CPU instruction sets)
    key, g = RM.grads(x, {**sd, **lora}, m["heads"], dkey, RM.G26_SCALE)
    assert R3.rel_l2(key, torch.from_numpy(z["key/" + tset])) < 1e-6
    assert sorted(g) == sorted(k[len(f"grad/{tset}/"):] for k in z.files if k.startswith(f"grad/{tset}/"))
    last = f"model.layer.{R3.G22_LAYERS - 1}."
    for n, v in g.items():
        ref = torch.from_numpy(z[f"grad/{tset}/{n}"])
        if n.startswith(last) and "k_proj" not in n:                 # only the key projection of the last layer reaches the key map
            assert float(ref.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and f"ebf/{tset}/{n}" not in z.files
        else:
            assert R3.rel_l2(v, ref) < 1e-6, n
            assert 0.0 < float(z[f"ebf/{tset}/{n}"]) < 5e-2
    assert float(z["err_f32/" + tset]) < 2e-6 and 1e-3 < float(z["err_bf16ac/" + tset]) < 1e-2
    # the MLP input modules matter: their gradients are there and not small
    for leaf in RM.G26_SETS[tag][tset]:
        for ab in "AB":
            assert float(np.abs(z[f"grad/{tset}/model.layer.0.mlp.{leaf}.lora_{ab}.weight"]).max()) > 1e-3


def test_one_of_the_pair_alone_is_the_both_run_with_the_other_at_zero():
    """What the engine relies on: an untargeted module of the pair is A = 0, B = 0 -- the same function as the state dict without it."""
    z, sd = golden("gated")
    x, dkey = RM.g26_inputs("gated")
    lora = set_lora(z, "gated", "both")
    zeroed = {k: (torch.zeros_like(v) if "up_proj" in k else v) for k, v in lora.items()}
    key, g = RM.grads(x, {**sd, **zeroed}, 2, dkey, RM.G26_SCALE)
    assert R3.rel_l2(key, torch.from_numpy(z["key/gate"])) < 1e-6
    for n in (k[len("grad/gate/"):] for k in z.files if k.startswith("grad/gate/")):
        ref = torch.from_numpy(z["grad/gate/" + n])
        assert float(ref.abs().max()) == 0.0 or R3.rel_l2(g[n], ref) < 1e-6
    assert all(float(g[n].abs().max()) == 0.0 for n in g if "up_proj" in n)        # t = 0 gives dA = 0, u = 0 gives dB = 0


# ================================================================================================ 2. bars against fault distances
@pytest.mark.parametrize("fault", RM.PAIR_FAULTS)
def test_each_pair_fault_is_stored_and_lies_twice_above_every_bar(fault):
    z, sd = golden("gated")
    m = R3.G22["gated"]
    x, dkey = RM.g26_inputs("gated")
    lora = set_lora(z, "gated", "both")
    p_drop = RM.G26_P_DROP if fault == "shared_mask" else 0.0
    tok = 1 + m["R"] + m["grid"][0] * m["grid"][1]
    masks = RM.g26_masks("gated", RM.g26_targets("gated", "both"), RM.G26_B * tok) if p_drop else None
    _, bad = RM.grads(x, {**sd, **lora}, m["heads"], dkey, RM.G26_SCALE, masks=masks, fault=fault)
    if p_drop:                                                    # the truth of the dropout run is stored too, and differs from the run without dropout
        _, true = RM.grads(x, {**sd, **lora}, m["heads"], dkey, RM.G26_SCALE, masks=masks)
        n0 = "model.layer.0.mlp.up_proj.lora_A.weight"
        assert R3.rel_l2(true[n0], torch.from_numpy(z["drop/" + n0])) < 1e-6 and R3.rel_l2(true[n0], torch.from_numpy(z["grad/both/" + n0])) > 0.05
        assert not torch.equal(masks[(0, "gate_proj")], masks[(0, "up_proj")])
    touched = 0
    for n, v in bad.items():
        assert R3.rel_l2(v, torch.from_numpy(z[f"fault/{fault}/{n}"])) < 1e-6 or float(v.abs().max()) == 0.0, n
        layer, leaf = int(n.split(".")[2]), n.split(".")[4]
        if layer == R3.G22_LAYERS - 1 or leaf not in TOUCHES[fault]:
            continue
        truth = torch.from_numpy(z[("drop/" if p_drop else "grad/both/") + n])
        dist, bar = R3.rel_l2(v, truth), RM.grad_bar(z, "both", n, p_drop)
        assert bar < 0.5 * dist, (fault, n, dist, bar)
        touched += 1
    assert touched == 2 * (R3.G22_LAYERS - 1) * len(TOUCHES[fault])
    # the kernel-level bars (tests/test_gpu_lora_mlp_pair.py: 2e-4 relative to max(1, |ref|max)) are absolute figures three orders under these distances


def test_every_bar_of_the_pass_tests_comes_from_the_golden():
    for tag in RM.G26_TAGS:
        z, _ = golden(tag)
        for tset in RM.G26_SETS[tag]:
            for k in (k for k in z.files if k.startswith(f"ebf/{tset}/")):
                n = k[len(f"ebf/{tset}/"):]
                assert RM.grad_bar(z, tset, n) == max(4e-2, 3 * float(z[k])) and RM.grad_bar(z, tset, n, 0.05) == max(5e-2, 3 * float(z[k]))
            bound = R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/" + tset]})
            assert bound == 3.0 * float(z["err_bf16ac/" + tset]) < 2e-2


# ================================================================================================ 3. the host surface
def test_flag_off_surface_is_todays():
    for name in ("up_proj", "gate_proj"):
        for gated in (False, True):
            with pytest.raises(NotImplementedError) as e:
                V.lora_targets_dinov3(QKV + [name], gated=gated, n_layers=2)
            assert V._REFUSED3[name] in str(e.value)
            with pytest.raises(NotImplementedError) as e:
                V.lora_targets_dinov3([name], gated=gated, n_layers=2, allow_out=True, allow_swiglu_out=True)
            assert V._REFUSED3[name] in str(e.value)
    with pytest.raises(NotImplementedError, match="allow_mlp_in=True"):       # the way in stands behind the old text
        V.lora_targets_dinov3(["up_proj"])
    assert V.lora_targets_dinov3(QKV) == (True, True, True) and V.lora_targets_dinov3(["q_proj", "o_proj"], allow_out=True) == ((True, False, False), ("o_proj",))
    z, sd = golden("gated")
    with pytest.raises(NotImplementedError) as e:
        V.lora_layout(sd, 2, QKV + ["gate_proj"])
    assert V._REFUSED3["gate_proj"] in str(e.value)
    _, mods = V.lora_layout(sd, 2, QKV)
    assert len(mods) == 6 and mods[3].path == "mlp.up_proj" and not mods[3].targeted and mods[3].a is None and all(m.part is None for m in mods)
    assert [m.path for m in V.lora_layout(sd, 2, QKV, allow_mlp_in=True)[1]] == [m.path for m in mods]         # the flag alone changes no table
    # DINOv2: the MLP input never needed the flag, and the flag changes nothing there
    assert V.lora_targets(["query", "fc1"]) == ((True, False, False), "fc1")


def test_target_resolution_with_the_flag():
    T = V.lora_targets_dinov3
    assert T(QKV + ["up_proj"], allow_mlp_in=True) == ((True, True, True), ("up_proj",))
    assert T(["up_proj"], gated=True, allow_mlp_in=True) == ((False, False, False), ("up_proj",))
    assert T(["model.layer.0.mlp.gate_proj", "layer.1.mlp.gate_proj"], gated=True, n_layers=2, allow_mlp_in=True) == ((False, False, False), ("gate_proj",))
    assert T(QKV + ["up_proj", "gate_proj"], gated=True, allow_mlp_in=True) == ((True, True, True), ("gate_proj", "up_proj"))
    assert T(QKV, gated=True, allow_mlp_in=True) == ((True, True, True), ()) and T(None, gated=True, allow_mlp_in=True) == ((True, True, True), ())
    every = QKV + ["o_proj", "gate_proj", "up_proj", "down_proj"]
    assert T(every, gated=True, allow_out=True, allow_swiglu_out=True, allow_mlp_in=True, hidden=1536) == ((True, True, True), ("o_proj", "down_proj"), ("gate_proj", "up_proj"))
    assert T(QKV + ["o_proj", "up_proj", "down_proj"], allow_out=True, allow_mlp_in=True, hidden=4096) == ((True, True, True), ("o_proj", "down_proj"), ("up_proj",))
    with pytest.raises(NotImplementedError) as e:                  # gate_proj on a plain MLP: no such module, its old reason
        T(["gate_proj"], allow_mlp_in=True)
    assert V._REFUSED3["gate_proj"] in str(e.value)
    with pytest.raises(NotImplementedError, match="down_proj"):   # the other opt-ins stay their own
        T(["up_proj", "down_proj"], allow_mlp_in=True)
    with pytest.raises(NotImplementedError, match="same modules"):
        T(["layer.0.mlp.up_proj"], n_layers=2, allow_mlp_in=True)
    for name in ("up_proj", "gate_proj"):                         # dinov3_vith16plus: refused by name, N1 = 10240 against 8192
        with pytest.raises(NotImplementedError, match=r"N1 = 10240.*8192.*dinov3_vith16plus"):
            T([name], gated=True, allow_mlp_in=True, hidden=5120)
    assert T(["up_proj"], gated=True, allow_mlp_in=True, hidden=4096) == ((False, False, False), ("up_proj",))      # 2 x 4096 = 8192 is covered
    assert T(["up_proj"], allow_mlp_in=True, hidden=8192)[1] == ("up_proj",)
    with pytest.raises(NotImplementedError, match="N1 = 8320"):
        T(["up_proj"], allow_mlp_in=True, hidden=8320)


def test_lora_only_needs_both_of_the_pair_or_neither():
    z, sd = golden("gated")
    for one in ("gate_proj", "up_proj"):
        with pytest.raises(NotImplementedError, match="fused bias"):
            V.lora_layout(sd, 2, QKV + [one], bias="lora_only", allow_mlp_in=True)
        assert len(V.lora_layout(sd, 2, QKV + [one], bias="none", allow_mlp_in=True)[1]) == 7
    _, mods = V.lora_layout(sd, 2, QKV + list(RM.PAIR), bias="lora_only", allow_mlp_in=True)
    g, u = mods[V._MLP_IN], mods[V._MLP_IN2]
    assert g.bias_off is not None and g.bias_off == u.bias_off and g.bias_cols == u.bias_cols and g.nb == u.nb == 768
    assert V.lora_row_numel(mods) == g.bias_off + 768              # q (128), v (128) -- k_proj has no bias --, then the ONE fused bias, last
    assert [m.bias_off for m in mods[:3]] == [g.bias_off - 256, None, g.bias_off - 128]
    _, plain = V.lora_layout(golden("g46")[1], 2, ["up_proj"], bias="lora_only", allow_mlp_in=True)
    assert len(plain) == 6 and plain[3].bias_off == plain[3].b.stop and plain[3].nb == 512


@pytest.mark.parametrize("tset", list(RM.G26_SETS["gated"]))
def test_arena_layout_of_the_pair(tset):
    z, sd = golden("gated")
    r, D, F = 2, 128, 384
    lp, mods = V.lora_layout(sd, r, RM.g26_targets("gated", tset), allow_mlp_in=True)
    assert lp == "model.layer." and len(mods) == 7
    assert [m.path for m in mods] == ["attention.q_proj", "attention.k_proj", "attention.v_proj", "mlp.gate_proj", "attention.o_proj", "mlp.down_proj", "mlp.up_proj"]
    g, u = mods[V._MLP_IN], mods[V._MLP_IN2]
    assert (g.targeted, u.targeted) == ("gate_proj" in RM.G26_SETS["gated"][tset], "up_proj" in RM.G26_SETS["gated"][tset])
    q0 = 6 * r * D                                                # [A_g | A_u | B_m (N1 x r)] where [A_m | B_m] would stand: whichever of the two is targeted
    assert (g.a, u.a) == (slice(q0, q0 + r * D), slice(q0 + r * D, q0 + 2 * r * D)) and g.b == u.b == slice(q0 + 2 * r * D, q0 + 2 * r * D + 2 * F * r)
    assert (g.part, u.part) == (0, 1) and (g.k, g.n, g.k_hf, g.n_hf, g.nb) == (D, F, D, F, 2 * F) == (u.k, u.n, u.k_hf, u.n_hf, u.nb)
    assert (g.w_slot, g.b_slot, g.c_slot, g.ln, g.row0) == (N.FC1_W, N.FC1_B, N.FC1_COLSUM, (N.LN2_G, N.LN2_B), 0) == (u.w_slot, u.b_slot, u.c_slot, u.ln, u.row0)
    assert V.lora_row_numel(mods) == g.b.stop and mods[4].a is None and mods[5].a is None
    # the plain MLP: up_proj fills the existing MLP-input row, [A_m | B_m]
    _, plain = V.lora_layout(golden("d256")[1], r, QKV + ["up_proj"], allow_mlp_in=True)
    assert len(plain) == 6 and plain[3].path == "mlp.up_proj" and plain[3].targeted and plain[3].part is None
    assert plain[3].a == slice(6 * r * 256, 7 * r * 256) and plain[3].b == slice(7 * r * 256, 7 * r * 256 + 1024 * r) and (plain[3].n, plain[3].nb) == (1024, 1024)
    with pytest.raises(ValueError, match="seventh"):
        V.lora_modules("dinov2", "swiglu", D, F, F, r, (True,) * 7)


@pytest.mark.parametrize("F0", [384, 200])
def test_b_round_trip_per_module_is_the_fused_one_split(F0):
    """``LoRAModule.get_rows`` / ``set_rows`` of the two parts against swiglu.lora_b_{to,from}_engine on the fused [2 F0, r] matrix = cat(gate, up)."""
    r, D, F = 3, 128, padded_hidden(F0)
    mods = V.lora_modules("dinov3", "swiglu", D, F, F0, r, (True, True, True, True, False, False, True))
    g, u = mods[V._MLP_IN], mods[V._MLP_IN2]
    gen = torch.Generator().manual_seed(5)
    bg, bu = torch.randn(F0, r, generator=gen), torch.randn(F0, r, generator=gen)
    eng = lora_b_to_engine(torch.cat((bg, bu), 0))                 # [2 F, r]: padded, 4-interleaved
    assert torch.equal(g.get_rows(eng), bg) and torch.equal(u.get_rows(eng), bu)
    block = torch.full((2 * F, r), 7.0)
    g.set_rows(block, bg)
    assert bool((block.view(F // 4, 2, 4, r)[:, 1] == 7.0).all())   # the partner's rows are not touched
    u.set_rows(block, bu)
    assert torch.equal(block, eng) and torch.equal(lora_b_from_engine(block, F0), torch.cat((bg, bu), 0))
    rows = torch.arange(2 * F)
    assert torch.equal(g.get_rows(rows.view(-1, 1).float()).view(-1), torch.tensor([8 * (i // 4) + i % 4 for i in range(F0)]).float())
    assert torch.equal(u.get_rows(rows.view(-1, 1).float()).view(-1), torch.tensor([8 * (i // 4) + 4 + i % 4 for i in range(F0)]).float())
    if F0 != F:                                                    # padded rows are zeros in the engine
        assert bool((eng.view(F // 4, 2, 4, r)[:, 0].reshape(F, r)[F0:] == 0).all())


def test_header_signatures_and_the_paths_that_need_no_device():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert "#define UCOD_ABI_VERSION 5" in header and N.ABI_VERSION == 5
    assert "#define UCOD_LORA_MLP_PAIR 4" in header and N.LORA_MLP_PAIR == 4 and "#define UCOD_LORA_OUT_SWIGLU 1" in header
    new = ("ucod_layernorm_lora_mlp_pair", "ucod_lora_mlp_pair_pack", "ucod_lora_mlp_pair_grad_workspace_bytes", "ucod_lora_mlp_pair_grad", "ucod_layernorm_bwd_lora_mlp_pair")
    old = ("ucod_layernorm_lora_mlp", "ucod_lora_mlp_pack", "ucod_lora_mlp_grad_workspace_bytes", "ucod_lora_mlp_grad", "ucod_layernorm_bwd_lora_mlp")
    lib = N.load("bf16")
    for a, b in zip(new, old):
        assert re.search(r"\b(int|size_t) " + a + r"\(", header) and hasattr(lib, a)
        assert N.SIGNATURES[a][0] is N.SIGNATURES[b][0] and N.SIGNATURES[a][1] == N.SIGNATURES[b][1]       # the single module's argument lists
        comment = header[:header.index(" " + a + "(")].rsplit("/*", 1)[1]
        assert "full_model.py:47-72" in comment, a
    assert re.search(r"UCOD_LORA_MLP_PAIR\s+\(full_model\.py:47-72\)", header)
    # sizes and refusals before any launch
    W, W1 = lib.ucod_lora_mlp_pair_grad_workspace_bytes, lib.ucod_lora_mlp_grad_workspace_bytes
    assert W(3072, 384) == 512 * 2 * (2 * 384 + 3072) * 4 and W(8192, 1536) == 256 * 2 * (2 * 1536 + 8192) * 4 and W(768, 128) == W1(768, 128) + 512 * 2 * 128 * 4
    assert W(8320, 128) == 0 and W(10240, 1280) == 0 and W(1024, 1664) == 0 and W(1000, 128) == 0 and W(1024, 192) == 0 and W(0, 128) == 0
    p = 4096
    grad = lambda **k: lib.ucod_lora_mlp_pair_grad(*[k.get(a, d) for a, d in (("dpre", p), ("h", p), ("lora", p), ("r", 2), ("s", 2.0), ("g", p), ("t", p), ("ws", p),  # noqa: E731
                                                                              ("wsb", 1 << 30), ("rows", 8), ("N1", 1024), ("D", 128), ("drop", None), ("st", None))])
    assert grad(N1=8320) == -1 and grad(D=1664) == -1 and grad(r=9) == -1 and grad(r=0) == -1 and grad(rows=0) == -1 and grad(wsb=W(1024, 128) - 1) == -2
    for a in ("dpre", "h", "lora", "g", "t", "ws"):
        assert grad(**{a: None}) == -1
    assert lib.ucod_lora_mlp_pair_pack(p, 9, 2.0, p, 1024, 128, None) == -1 and lib.ucod_lora_mlp_pair_pack(p, 2, 2.0, p, 8320, 128, None) == -1
    assert lib.ucod_lora_mlp_pair_pack(None, 2, 2.0, p, 1024, 128, None) == -1 and lib.ucod_lora_mlp_pair_pack(p, 2, 2.0, p, 1020, 128, None) == -1
    assert lib.ucod_layernorm_lora_mlp_pair(p, 0, p, p, p, 9, p, 8, 128, 1e-5, None, None) == -1 and lib.ucod_layernorm_lora_mlp_pair(p, 0, p, p, None, 2, p, 8, 128, 1e-5, None, None) == -1
    assert lib.ucod_layernorm_bwd_lora_mlp_pair(p, p, 0, p, None, None, p, None, 8, 128, 1e-5, p, 3, p, 2, None, None) == -1       # ldt < 2 r
    assert N.load("f16").ucod_lora_mlp_pair_grad(p, p, p, 2, 2.0, p, p, p, 1 << 30, 8, 1024, 128, None, None) != 0                 # bf16 library only
    # the pass drivers: the bit is valid only with the SwiGLU MLP and an MLP table
    t = N.VitTrainDesc()
    v = t.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps, v.attn_variant, v.n_reg = 2, 3, 64, 96, 16, 128, 2, 384, 3, 768, 1e-5, 2, 4
    t.lora_r, t.lora_scaling = 2, 2.0
    TM = (C.c_void_p * 9)(*[p] * 9)
    size, isize = lib.ucod_vit_train_workspace_bytes_lora_out_ex, lib.ucod_vit_lora_infer_workspace_bytes_lora_out_ex
    single, pair = size(C.byref(t), N.UCOD_MLP_SWIGLU, 0, TM, None), size(C.byref(t), N.UCOD_MLP_SWIGLU, N.LORA_MLP_PAIR, TM, None)
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert single > 0 and pair == single - up(W1(768, 128)) + up(W(768, 128))
    assert isize(C.byref(t), N.UCOD_MLP_SWIGLU, N.LORA_MLP_PAIR, TM, None) == isize(C.byref(t), N.UCOD_MLP_SWIGLU, 0, TM, None) > 0
    for mlp, tm in ((N.UCOD_MLP_GELU, TM), (N.UCOD_MLP_SWIGLU, None)):
        assert size(C.byref(t), mlp, N.LORA_MLP_PAIR, tm, None) == 0 and isize(C.byref(t), mlp, N.LORA_MLP_PAIR, tm, None) == 0
        for fn in (lib.ucod_vit_forward_train_lora_out_ex, lib.ucod_vit_forward_lora_infer_lora_out_ex):
            assert fn(C.byref(t), mlp, N.LORA_MLP_PAIR, TM, TM, tm, None, p, p, p, 1 << 30, None) == -1
        assert lib.ucod_vit_backward_lora_out_ex(C.byref(t), mlp, N.LORA_MLP_PAIR, TM, TM, tm, None, p, p, 1 << 30, None) == -1
    assert size(C.byref(t), N.UCOD_MLP_SWIGLU, 2, TM, None) == 0 and size(C.byref(t), N.UCOD_MLP_SWIGLU, N.LORA_MLP_PAIR | 8, TM, None) == 0    # unknown bits (2 is pinned as one)
    v.F = 5120                                                     # dinov3_vith16plus: N1 = 10240
    assert size(C.byref(t), N.UCOD_MLP_SWIGLU, N.LORA_MLP_PAIR, TM, None) == 0
