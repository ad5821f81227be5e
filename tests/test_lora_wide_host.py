"""Host (no GPU): LoRA on MLP modules wider than the register-resident row kernels take -- DINOv3 ViT-H+/16's gate_proj / up_proj (N1 = 10240) and down_proj
(K = 5120) -- behind ``allow_wide_mlp`` / UCOD_LORA_WIDE.

1  The G28 golden (tests/golden/make_golden_dinov3_lora_wide.py) is what its generator's seeds draw, and the restatement tests/lora_wide_ref.py reproduces transformers'
   f64 key maps and gradients in it; the two stored mutations (a pass without the MLP modules' forward term; t summed over the first 8192 columns only) lie outside
   the bars the GPU tests use.
2  The parser with and without the opt-in at hidden 4200 (padded 4224, N1 = 8448), 5120 and one step past the wide ceilings; without it the messages are today's.
3  The header's constants and ``native``'s; the wide size functions against the narrow ones; every refusal that needs no launch; the pass drivers' flag bit.
4  The case lists of tests/test_gpu_lora_wide.py reach every instantiation the wide launch functions can select (the dispatch of csrc/vit_train.hip, restated).
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
import dinov3_ref as R3
import dinov3_lora_mlp_in_ref as RM
import lora_wide_ref as RW
import lora_wide_cases as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QKV = ["q_proj", "k_proj", "v_proj"]
EVERY = QKV + ["o_proj", "gate_proj", "up_proj", "down_proj"]
ALL = dict(gated=True, allow_out=True, allow_swiglu_out=True, allow_mlp_in=True)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g28_dinov3_lora_wide.npz")), RW.g28_state_dict()


def key_bound(z, tset):
    return R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/" + tset]})


# ================================================================================================ 1. the golden
@pytest.mark.parametrize("tset", list(RW.G28_SETS))
def test_the_restatement_reproduces_the_golden(tset):
    z, sd = golden()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g28_dinov3_lora_wide.npz")) < 1 << 20
    assert (int(z["seed"]), int(z["input_seed"]), int(z["lora_seed"])) == (RW.G28_SEED, RW.G28_INPUT_SEED, RW.G28_LORA_SEED)
    assert sd["model.layer.0.mlp.gate_proj.weight"].shape == (5120, 128) and sd["model.layer.0.mlp.down_proj.weight"].shape == (128, 5120)
    x, dkey = RW.g28_inputs()
    lora = RW.g28_lora(RW.G28_SETS[tset])
    # (the weights are pinned through the key map, not byte for byte: trunc_normal_'s erfinv differs in the last bit between CPU instruction sets)
    key, g = RW.grads(x, {**sd, **lora}, dkey)
    assert R3.rel_l2(key, torch.from_numpy(z["key/" + tset])) < 1e-6           # (f32 storage)
    assert sorted(g) == sorted(lora) == sorted(k[len(f"grad/{tset}/"):] for k in z.files if k.startswith(f"grad/{tset}/"))
    for n, v in g.items():
        ref = torch.from_numpy(z[f"grad/{tset}/{n}"])
        if n.startswith("model.layer.1.") and "k_proj" not in n:     # only the key projection of the last layer reaches the key map
            assert float(ref.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and f"ebf/{tset}/{n}" not in z.files
        else:
            assert R3.rel_l2(v, ref) < 1e-6, n
            assert 0.0 < float(z[f"ebf/{tset}/{n}"]) < 5e-2
    assert float(z["err_f32/" + tset]) < 2e-6 and 1e-3 < float(z["err_bf16ac/" + tset]) < 1e-2
    for leaf in set(RW.G28_SETS[tset]) & set(RW.WIDE_LEAVES):       # the wide modules matter: their gradients are there and not small
        for ab in "AB":
            assert float(np.abs(z[f"grad/{tset}/model.layer.0.mlp.{leaf}.lora_{ab}.weight"]).max()) > 1e-3


@pytest.mark.parametrize("tset", list(RW.G28_SETS))
def test_the_mutations_are_stored_and_lie_outside_the_bars(tset):
    z, sd = golden()
    x, dkey = RW.g28_inputs()
    both = {**sd, **RW.g28_lora(RW.G28_SETS[tset])}
    truth = {k[len(f"grad/{tset}/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"grad/{tset}/")}
    # a pass without the MLP modules' forward term: the key map is outside the engines' bound
    key, _ = RW.grads(x, both, dkey, mutation="no_forward")
    d = R3.rel_l2(key, torch.from_numpy(z["key/" + tset]))
    assert abs(d - float(z[f"mut/no_forward/{tset}/key"])) < 1e-5 and d > 2 * key_bound(z, tset), (d, key_bound(z, tset))
    if tset == "down":                                              # no MLP input module, no t
        assert not any(k.startswith("mut/t_8192/down/") for k in z.files)
        return
    # t over the first 8192 columns only: the forward is the true one; dA of gate_proj / up_proj is outside its bar several times over, and dB untouched
    key, bad = RW.grads(x, both, dkey, mutation="t_8192")
    assert R3.rel_l2(key, torch.from_numpy(z["key/" + tset])) < 1e-6 and float(z[f"mut/t_8192/{tset}/key"]) < 1e-12
    for leaf in RM.PAIR:
        n = f"model.layer.0.mlp.{leaf}.lora_A.weight"
        d = R3.rel_l2(bad[n], truth[n])
        # (1024 of a module's 5120 terms of t are missing: about sqrt(1024 / 5120) = 0.45 of its norm, nine times the bar with dropout)
        assert abs(d - float(z[f"mut/t_8192/{tset}/{n}"])) < 1e-5 and 0.35 < d < 0.6 and d > 5 * RW.grad_bar(z, tset, n, 0.05), (n, d)
        assert float(z[f"mut/t_8192/{tset}/model.layer.0.mlp.{leaf}.lora_B.weight"]) < 1e-12
    # (it reaches q / k / v / o of layer 0 only through LayerNorm 2's cotangent, where it is one small term among many: those distances are stored, and they are
    #  INSIDE the bars -- the check of t itself is the kernel test, tests/test_gpu_lora_wide.py::test_lora_mlp_grad_wide, which compares t against this very sum)
    if tset == "every":
        via_ln2 = [float(z[f"mut/t_8192/every/model.layer.0.attention.{leaf}.lora_{ab}.weight"]) for leaf in ("q_proj", "k_proj", "v_proj", "o_proj") for ab in "AB"]
        assert 0.0 < max(via_ln2) < 4e-2


# ================================================================================================ 2. the parser
def test_the_parser_without_the_opt_in_is_todays():
    T = V.lora_targets_dinov3
    for name in ("up_proj", "gate_proj"):                         # (tests/test_dinov3_lora_mlp_in_host.py's patterns)
        with pytest.raises(NotImplementedError, match=r"N1 = 10240.*8192.*dinov3_vith16plus"):
            T([name], gated=True, allow_mlp_in=True, hidden=5120)
        with pytest.raises(NotImplementedError, match=r"N1 = 8448.*8192") as e:
            T([name], gated=True, allow_mlp_in=True, hidden=4200)
        assert "allow_wide_mlp=True" in str(e.value)               # the way in stands behind the old text
    with pytest.raises(NotImplementedError, match="N1 = 8320"):
        T(["up_proj"], allow_mlp_in=True, hidden=8320)
    for hidden, k in ((5120, 5120), (4200, 4224)):
        with pytest.raises(NotImplementedError, match=rf"K = {k}.*K <= 4096.*registers") as e:
            T(["down_proj"], hidden=hidden, **ALL)
        assert "allow_wide_mlp=True" in str(e.value)
    with pytest.raises(NotImplementedError, match=r"N1 = 10496.*8192") as e:     # past the wide ceiling the opt-in is no way in, and is not offered
        T(["up_proj"], gated=True, allow_mlp_in=True, hidden=5248)
    assert "allow_wide_mlp" not in str(e.value)
    assert T(["up_proj"], gated=True, allow_mlp_in=True, hidden=4096) == ((False, False, False), ("up_proj",))      # the narrow widths: as ever
    assert T(EVERY, hidden=4096, **ALL) == T(EVERY, hidden=4096, allow_wide_mlp=True, **ALL)


def test_the_parser_with_the_opt_in():
    T = V.lora_targets_dinov3
    want = ((True, True, True), ("o_proj", "down_proj"), ("gate_proj", "up_proj"))
    for hidden in (4200, 5120):
        assert T(EVERY, hidden=hidden, allow_wide_mlp=True, **ALL) == want
        assert T(["down_proj"], hidden=hidden, allow_wide_mlp=True, **ALL) == ((False, False, False), ("down_proj",), ())
    assert T(["up_proj"], allow_mlp_in=True, allow_wide_mlp=True, hidden=N.LORA_WIDE_MAX_N1)[1] == ("up_proj",)          # the plain MLP: N1 = hidden
    assert T(["down_proj"], hidden=N.LORA_WIDE_MAX_K, allow_wide_mlp=True, **ALL)[1] == ("down_proj",)              # (alone: the pair would have 2 x 8192 rows)
    with pytest.raises(NotImplementedError, match=rf"N1 = 10496.*N1 <= {N.LORA_WIDE_MAX_N1}"):
        T(["gate_proj"], hidden=5248, allow_wide_mlp=True, **ALL)
    with pytest.raises(NotImplementedError, match=rf"N1 = {N.LORA_WIDE_MAX_N1 + 128}"):
        T(["up_proj"], allow_mlp_in=True, allow_wide_mlp=True, hidden=N.LORA_WIDE_MAX_N1 + 128)
    with pytest.raises(NotImplementedError, match=rf"K = {N.LORA_WIDE_MAX_K + 128}.*K <= {N.LORA_WIDE_MAX_K}"):
        T(["down_proj"], hidden=N.LORA_WIDE_MAX_K + 100, allow_wide_mlp=True, **ALL)
    # the opt-in accepts no name of its own: every other refusal stays
    with pytest.raises(NotImplementedError) as e:
        T(["up_proj"], gated=True, hidden=5120, allow_wide_mlp=True)
    assert V._REFUSED3["up_proj"] in str(e.value)
    with pytest.raises(NotImplementedError, match="allow_swiglu_out=True"):
        T(["down_proj"], gated=True, allow_out=True, hidden=5120, allow_wide_mlp=True)


def test_lora_layout_threads_the_opt_in_through():
    z, sd = golden()
    for targets in (list(RM.PAIR), ["down_proj"], EVERY):
        with pytest.raises(NotImplementedError, match="allow_wide_mlp=True"):
            V.lora_layout(sd, 2, targets, allow_out=True, allow_swiglu_out=True, allow_mlp_in=True)
    lp, mods = V.lora_layout(sd, 2, EVERY, allow_out=True, allow_swiglu_out=True, allow_mlp_in=True, allow_wide_mlp=True)
    assert lp == "model.layer." and len(mods) == 7 and all(m.targeted for m in mods)
    g, u, d = mods[V._MLP_IN], mods[V._MLP_IN2], mods[V._MLP_OUT]
    assert (g.nb, u.nb, g.n, d.k, d.k_hf) == (10240, 10240, 5120, 5120, 5120) and g.b == u.b and g.b.stop - g.b.start == 10240 * 2
    # with narrow targets only the opt-in changes no table
    a, b = V.lora_layout(sd, 2, QKV + ["o_proj"], allow_out=True)[1], V.lora_layout(sd, 2, QKV + ["o_proj"], allow_out=True, allow_wide_mlp=True)[1]
    assert a == b


# ================================================================================================ 3. constants, sizes, refusals
def test_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert "#define UCOD_ABI_VERSION 5" in header and N.ABI_VERSION == 5
    for name, val in (("UCOD_LORA_WIDE", N.LORA_WIDE), ("UCOD_LORA_WIDE_MAX_N1", N.LORA_WIDE_MAX_N1), ("UCOD_LORA_WIDE_MAX_K", N.LORA_WIDE_MAX_K)):
        assert re.search(rf"#define {name} {val}\b", header), name
    assert N.LORA_WIDE == 16 and N.LORA_WIDE_MAX_N1 >= 10240 and N.LORA_WIDE_MAX_K >= 5120 and N.LORA_WIDE_MAX_N1 % 128 == 0 and N.LORA_WIDE_MAX_K % 128 == 0
    assert N.LORA_WIDE & (N.LORA_OUT_SWIGLU | N.LORA_MLP_PAIR | 2 | 8) == 0        # (2 and 8 are pinned as unknown bits by the existing tests)
    lib = N.load("bf16")
    pairs = {"ucod_lora_mlp_pack_wide": "ucod_lora_mlp_pack", "ucod_lora_mlp_pair_pack_wide": "ucod_lora_mlp_pair_pack",
             "ucod_lora_mlp_grad_workspace_bytes_wide": "ucod_lora_mlp_grad_workspace_bytes", "ucod_lora_mlp_pair_grad_workspace_bytes_wide": "ucod_lora_mlp_pair_grad_workspace_bytes",
             "ucod_lora_mlp_grad_wide": "ucod_lora_mlp_grad", "ucod_lora_mlp_pair_grad_wide": "ucod_lora_mlp_pair_grad", "ucod_lora_out_fwd_wide": "ucod_lora_out_fwd",
             "ucod_lora_out_grad_s_wide": "ucod_lora_out_grad_s", "ucod_lora_out_grad_workspace_bytes_wide": "ucod_lora_out_grad_workspace_bytes"}
    for a, b in pairs.items():
        assert re.search(r"\b(int|size_t) " + a + r"\(", header) and hasattr(lib, a)
        assert N.SIGNATURES[a][0] is N.SIGNATURES[b][0] and N.SIGNATURES[a][1] == N.SIGNATURES[b][1]       # the narrow forms' argument lists
    comment = header[:header.index(" ucod_lora_mlp_pack_wide(")].rsplit("/*", 1)[1]
    assert "full_model.py:47-72" in comment
    assert re.search(r"UCOD_LORA_WIDE\s+\(defined above; full_model\.py:47-72\)", header)


def test_wide_size_functions_against_the_narrow_ones():
    lib = N.load("bf16")
    for mods, narrow, wide in ((1, lib.ucod_lora_mlp_grad_workspace_bytes, lib.ucod_lora_mlp_grad_workspace_bytes_wide),
                               (2, lib.ucod_lora_mlp_pair_grad_workspace_bytes, lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide)):
        for n1 in (768, 1024, 3072, 4096, 4224, 6144, 8192):        # the narrow widths the existing tests name
            for d in (128, 384, 768, 1280, 1536):
                assert wide(n1, d) == narrow(n1, d) > 0
        for n1, d in ((8320, 128), (10240, 1280), (8448, 128), (N.LORA_WIDE_MAX_N1, 1536)):
            assert narrow(n1, d) == 0 and wide(n1, d) == 256 * (mods * d + n1) * 4            # one rank per pass, 256 blocks
        for n1, d in ((N.LORA_WIDE_MAX_N1 + 128, 128), (10240, 1664), (10240, 192), (10200, 128), (0, 128)):
            assert wide(n1, d) == 0
    narrow, wide = lib.ucod_lora_out_grad_workspace_bytes, lib.ucod_lora_out_grad_workspace_bytes_wide
    for r in (1, 2, 8):
        for k in (128, 384, 512, 1024, 1536, 3072, 4096):
            for d in (128, 256, 1280, 1536):
                assert wide(r, k, d) == narrow(r, k, d) > 0
        for k in (4224, 5120, 8192, N.LORA_WIDE_MAX_K):
            assert narrow(r, k, 128) == 0 and wide(r, k, 1280) == max(512 * 1280 * r, 256 * r * k) * 4
        assert wide(r, N.LORA_WIDE_MAX_K + 128, 128) == 0 and wide(r, 5100, 128) == 0 and wide(r, 5120, 1664) == 0
    assert wide(9, 5120, 128) == 0 and wide(0, 5120, 128) == 0


def test_refusals_before_any_launch():
    lib, p = N.load("bf16"), 4096
    W2 = lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide
    for fn in (lib.ucod_lora_mlp_grad_wide, lib.ucod_lora_mlp_pair_grad_wide):
        grad = lambda **k: fn(*[k.get(a, d) for a, d in (("dpre", p), ("h", p), ("lora", p), ("r", 2), ("s", 2.0), ("g", p), ("t", p), ("ws", p),  # noqa: E731,B023
                                                         ("wsb", 1 << 30), ("rows", 8), ("N1", 10240), ("D", 128), ("drop", None), ("st", None))])
        assert grad(N1=N.LORA_WIDE_MAX_N1 + 128) == -1 and grad(N1=10200) == -1 and grad(D=1664) == -1 and grad(r=9) == -1 and grad(r=0) == -1 and grad(rows=0) == -1
        for a in ("dpre", "h", "lora", "g", "t", "ws"):
            assert grad(**{a: None}) == -1
    assert lib.ucod_lora_mlp_pair_grad_wide(p, p, p, 2, 2.0, p, p, p, W2(10240, 128) - 1, 8, 10240, 128, None, None) == -2      # a workspace one byte short
    for pack in (lib.ucod_lora_mlp_pack_wide, lib.ucod_lora_mlp_pair_pack_wide):
        assert pack(p, 9, 2.0, p, 10240, 128, None) == -1 and pack(p, 2, 2.0, p, N.LORA_WIDE_MAX_N1 + 128, 128, None) == -1 and pack(None, 2, 2.0, p, 10240, 128, None) == -1
        assert pack(p, 2, 2.0, None, 10240, 128, None) == -1
    fwd = lambda **k: lib.ucod_lora_out_fwd_wide(*[k.get(a, d) for a, d in (("x", p), ("lora", p), ("r", 2), ("s", 2.0), ("lam", None), ("xs", p), ("h16", 0), ("u", p),  # noqa: E731
                                                                            ("rows", 8), ("K", 5120), ("D", 128), ("drop", None), ("st", None))])
    assert fwd(K=N.LORA_WIDE_MAX_K + 128) == -1 and fwd(K=5100) == -1 and fwd(D=1664) == -1 and fwd(r=9) == -1 and fwd(h16=2) == -1
    assert fwd(x=None) == -1 and fwd(lora=None) == -1 and fwd(xs=None) == -1
    wo = lib.ucod_lora_out_grad_workspace_bytes_wide(2, 5120, 128)
    gs = lambda **k: lib.ucod_lora_out_grad_s_wide(*[k.get(a, d) for a, d in (("s", p), ("u", p), ("lora", p), ("r", 2), ("sc", 2.0), ("g", p), ("t", p), ("ws", p),  # noqa: E731
                                                                              ("wsb", 1 << 30), ("rows", 8), ("K", 5120), ("D", 128), ("st", None))])
    assert gs(K=N.LORA_WIDE_MAX_K + 128) == -1 and gs(D=1664) == -1 and gs(r=9) == -1 and gs(s=None) == -1 and gs(u=None) == -1 and gs(wsb=wo - 1) == -2
    gx = lambda **k: lib.ucod_lora_out_grad_x_ex(*[k.get(a, d) for a, d in (("x", p), ("act", N.LORA_OUT_ACT_GELU), ("fl", N.LORA_WIDE), ("cot", p), ("t", p), ("lora", p),  # noqa: E731
                                                                            ("r", 2), ("g", p), ("ws", p), ("wsb", 1 << 30), ("rows", 8), ("K", 5120), ("D", 128),
                                                                            ("drop", None), ("st", None))])
    assert gx(fl=0) == -1 and gx(fl=N.LORA_WIDE | 2) == -1 and gx(fl=N.LORA_WIDE | 8) == -1 and gx(fl=N.LORA_WIDE | 32) == -1     # an unknown bit beside 16
    assert gx(act=N.LORA_OUT_ACT_SWIGLU) == -1 and gx(act=N.LORA_OUT_ACT_SWIGLU, fl=N.LORA_OUT_SWIGLU) == -1                       # (K = 5120 needs both bits)
    assert gx(K=N.LORA_WIDE_MAX_K + 128) == -1 and gx(K=5100) == -1 and gx(D=1664) == -1 and gx(r=9) == -1 and gx(x=None) == -1 and gx(cot=None) == -1 and gx(wsb=wo - 1) == -2
    f16 = N.load("f16")                                            # bf16 library only
    assert f16.ucod_lora_mlp_pair_grad_wide(p, p, p, 2, 2.0, p, p, p, 1 << 30, 8, 10240, 128, None, None) != 0
    assert f16.ucod_lora_out_fwd_wide(p, p, 2, 2.0, None, p, 0, p, 8, 5120, 128, None, None) != 0


def test_the_pass_drivers_take_the_bit_only_where_a_table_needs_it():
    lib, p = N.load("bf16"), 4096
    t = N.VitTrainDesc()
    v = t.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps, v.attn_variant, v.n_reg = 3, 3, 64, 96, 16, 128, 2, 5120, 2, 768, 1e-5, 2, 4
    t.lora_r, t.lora_scaling = 2, 2.0
    TM = (C.c_void_p * 6)(*[p] * 6)
    TO_f = (C.c_void_p * 8)(*[None, None, p, p] * 2)               # fc2 / down_proj alone
    TO_o = (C.c_void_p * 8)(*[p, p, None, None] * 2)               # dense / o_proj alone
    size, isize = lib.ucod_vit_train_workspace_bytes_lora_out_ex, lib.ucod_vit_lora_infer_workspace_bytes_lora_out_ex
    SW, PAIR, WIDE, G = N.LORA_OUT_SWIGLU, N.LORA_MLP_PAIR, N.LORA_WIDE, N.UCOD_MLP_SWIGLU
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    ref = lambda: C.byref(t)  # noqa: E731
    # today's refusals at F = 5120 with today's flag values
    assert size(ref(), G, PAIR, TM, None) == 0 and size(ref(), G, 0, TM, None) == 0 and size(ref(), G, SW, None, TO_f) == 0 and size(ref(), G, SW | PAIR, TM, TO_f) == 0
    # with the bit: non-zero, and the MLP / out blocks are the wide size functions'
    base = size(ref(), G, 0, None, None)
    pair, single, down = size(ref(), G, PAIR | WIDE, TM, None), size(ref(), G, WIDE, TM, None), size(ref(), G, SW | WIDE, None, TO_f)
    assert base > 0 and pair > single > base and down > base and size(ref(), G, SW | PAIR | WIDE, TM, TO_f) > pair
    assert pair - single == up(lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide(10240, 128)) - up(lib.ucod_lora_mlp_grad_workspace_bytes_wide(10240, 128))
    assert isize(ref(), G, PAIR | WIDE, TM, None) > 0 and isize(ref(), G, SW | WIDE, None, TO_f) > 0
    # an unknown bit beside 16; the bit without a table that needs it
    for bad in (WIDE | 2, WIDE | 8, WIDE | 32, PAIR | WIDE | 2):
        assert size(ref(), G, bad, TM, None) == 0 and isize(ref(), G, bad, TM, None) == 0
    assert size(ref(), G, WIDE, None, None) == 0 and size(ref(), G, WIDE, None, TO_o) == 0 and size(ref(), N.UCOD_MLP_GELU, WIDE, None, None) == 0
    bias = lib.ucod_vit_train_workspace_bytes_lora_bias
    TB = (C.c_void_p * 12)(*[p] * 12)
    assert bias(ref(), G, PAIR, TM, None, TB) == 0 and bias(ref(), G, PAIR | WIDE, TM, None, TB) > pair and bias(ref(), G, PAIR | WIDE | 8, TM, None, TB) == 0
    for fn in (lib.ucod_vit_forward_train_lora_out_ex, lib.ucod_vit_forward_lora_infer_lora_out_ex):
        assert fn(ref(), G, WIDE, TM, TM, None, None, p, p, p, 1 << 40, None) == -1 and fn(ref(), G, WIDE | 2, TM, TM, TM, None, p, p, p, 1 << 40, None) == -1
        assert fn(ref(), G, PAIR | WIDE, TM, TM, TM, None, p, p, p, pair - 1 if fn is lib.ucod_vit_forward_train_lora_out_ex else 1, None) == -2
    assert lib.ucod_vit_backward_lora_out_ex(ref(), G, WIDE, TM, TM, None, None, p, p, 1 << 40, None) == -1
    assert lib.ucod_vit_backward_lora_out_ex(ref(), G, PAIR | WIDE, TM, TM, TM, None, p, p, pair - 1, None) == -2
    v.F = 4096                                                     # a width the narrow forms cover: the bit has no table that needs it (N1 = 8192, K = 4096)
    assert size(ref(), G, PAIR, TM, None) > 0 and size(ref(), G, PAIR | WIDE, TM, None) == 0 and size(ref(), G, SW | WIDE, None, TO_f) == 0
    v.F = 5248                                                     # one step past the wide ceiling of the pair: N1 = 10496
    assert size(ref(), G, PAIR | WIDE, TM, None) == 0 and size(ref(), G, SW | WIDE, None, TO_f) > 0
    v.F, v.D, v.heads = 5120, 1664, 26
    assert size(ref(), G, PAIR | WIDE, TM, None) == 0
    v.D, v.heads, t.lora_r = 128, 2, 9
    assert size(ref(), G, PAIR | WIDE, TM, None) == 0


# ================================================================================================ 4. the GPU file's cases against the dispatch
def test_the_gpu_cases_reach_every_wide_instantiation():
    """csrc/vit_train.hip, restated: mlp_grad launches <modules, nvt, npt, rw> with nvt = ceil(N1 / 8 / 256) (3 runs as 4), npt = ceil(D / 2 / 256), rw = 1 where
    nvt > 4 (then r passes) else 2; out_fwd launches <nvt, rw, h16, nt> with nt = 512 where K > 4096 (then nvt = 2), rw = 2 for r <= 2 else 8."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    nvt, npt = (lambda n1: cdiv(n1 // 8, 256)), (lambda d: cdiv(d // 2, 256))
    wide_n1 = range(8192 + 128, N.LORA_WIDE_MAX_N1 + 1, 128)
    assert {nvt(n) for n in wide_n1} == {5}                         # every wide width is the one five-vector form
    cases = CS.WIDE_GRAD_CASES
    assert all(8192 < c[0] <= N.LORA_WIDE_MAX_N1 for c in cases)
    assert {(nvt(c[0]), npt(c[1])) for c in cases} == {(5, p) for p in (1, 2, 3)}
    n1s = {c[0] for c in cases}
    assert n1s == {8448, 10240, N.LORA_WIDE_MAX_N1} and {c[1] for c in cases} >= {128, 1280, 1536}
    for n1 in n1s:
        mine = [c for c in cases if c[0] == n1]
        assert {npt(c[1]) for c in mine} == {1, 2, 3} and {c[2] for c in mine} == {1, 2, 3, 8}
        assert {c[3] for c in mine} == {37, 4 * 256 + 5} and {c[4] for c in mine} == {0.0, 0.05}      # 256 blocks of 4 rows: one group above the cap
    assert (8448 // 8) % 256 != 0 and 8448 // 8 > 4 * 256                                            # the fifth vector partly empty
    # the forward: K > 4096 is <2, rw, h16, 512> for rw in {2, 8}; the test runs every shape with every rank and both stream types
    assert all(4096 < k <= N.LORA_WIDE_MAX_K and cdiv(k // 8, 512) <= 2 for _, k, _ in CS.WIDE_FWD_SHAPES)
    assert {2 if r <= 2 else 8 for r in CS.WIDE_FWD_RANKS} == {2, 8} and set(CS.WIDE_FWD_RANKS) == {1, 2, 8}
    assert CS.WIDE_FWD_SHAPES == [(111, 4224, 128), (111, 5120, 1280), (2053, N.LORA_WIDE_MAX_K, 1536)] and 2053 > 2048
    # grad_s / grad_x: <npt, rw> and <rw> (x GELU / SwiGLU), K spread over blockIdx.y
    assert {k for _, k, _, _ in CS.WIDE_OUT_GRAD_SHAPES} == {4224, 5120} and {2 if r <= 2 else 8 for r in CS.WIDE_OUT_GRAD_RANKS} == {2, 8}
    assert any(k0 < k for _, k, _, k0 in CS.WIDE_OUT_GRAD_SHAPES)                                   # padded units
