"""CPU only: the references of tests/refiner_outputs_ref.py agree with the golden vectors of the real reference (G29) and with one another, the kink
margin holds on every kernel case, and the bounds of tests/test_gpu_refiner_outputs.py hide no lost term."""
import os
import sys

import pytest
import torch

from conftest import load_golden
import refiner_outputs_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_golden_refiner_outputs as MG29  # noqa: E402  (importing it runs nothing: constants and the probe recipe)


def f32_bound(f32, f64):
    """bound on the distance between the real reference (f32) and the f64 oracle: 4 x the f32 oracle's own distance from it, floor 1e-6 (another
    summation order of f32 terms)"""
    return max(4.0 * R.rel_l2(f32, f64), 1e-6)


@pytest.mark.parametrize("tag", ("full", "partial"))
def test_f64_reference_reproduces_g29(tag):
    """autograd_outputs in f64 against the real reference module's gradients (G29, f32).  Bounds: the oracle's own f32-versus-f64 difference (f32_bound).
    On this fixture the smallest |z| of the fuser's pre-activations in f32 is 7.2e-5 (full) / 3.9e-5 (partial), no pair is below 1e-5: f32 and f64 agree
    on every gate m_k, which is asserted -- so no whole term separates the two."""
    g = load_golden("g29_refiner_outputs_grad")
    ref, f32 = R.autograd_outputs(tag), R.autograd_outputs(tag, "prob", "f32")
    assert ref["mask_ok"] and torch.equal(g["G"], R.cotangent()) and MG29.G_SEED == R.G_SEED
    zmin = float(g[tag + ".z_f32_min"])
    assert abs(zmin - (7.2e-5 if tag == "full" else 3.9e-5)) < 1e-6 and float(g[tag + ".z_f32_below_1e-5"]) == 0
    assert ref["z"].numel() == 41472 and float(g[tag + ".z_f32_below_1e-3"]) == (35 if tag == "full" else 20)       # 8.4e-4 of the pairs on `full`
    assert torch.equal(g[tag + ".z_f32_gate"].bool(), ref["z"] > 0) and torch.equal(f32["z"] > 0, ref["z"] > 0)
    for which in R.LOSSES:
        k = f"{tag}.{which}."
        assert float(g[k + "alpha_has_grad"]) == 0.0
        a, b = ref[which], f32[which]
        assert R.rel_l2(g[k + "d_window_preds"], a["d_window_preds"]) < f32_bound(b["d_window_preds"], a["d_window_preds"])
        assert len(a["grads"]) == 22
        for i, name in enumerate(a["grads"]):
            want, mine = a["grads"][name], b["grads"][name]
            bound = f32_bound(mine, want)
            if want.dim() == 1 or name.startswith("GE."):
                assert R.rel_l2(g[k + name], want) < bound, (name, R.rel_l2(g[k + name], want), bound)
            else:
                pr = MG29.probe(i, want.shape)
                assert abs(float(g[k + name + ".norm"]) - float(want.norm())) < bound * float(want.norm()), name
                assert abs(float(g[k + name + ".probe"]) - float((want * pr).sum())) < bound * float(want.norm()) * float(pr.norm()), name   # Cauchy-Schwarz


@pytest.mark.parametrize("tag", ("full", "partial"))
def test_hand_written_formulas_equal_autograd(tag):
    """ge_bwd in f64 plus the gather equals torch autograd of oracle.refiner.gated_ensembler o concat_windows in window_preds and the fuser: 1e-12."""
    from oracle import refiner as OR
    fx, ref = R.RT.fixture(tag, "prob"), R.autograd_outputs(tag)
    G = R.cotangent().double()
    coords, img = R.window_cells(tag)
    counts = [int((img == b).sum()) for b in range(2)]
    sd = {k: fx["sd"][k].double().clone().requires_grad_(True) for k in R.FUSER}
    wp = ref["window_preds"].clone().requires_grad_(True)
    with R._all_f64(True):
        out, w = OR.gated_ensembler(fx["preds"].double(), OR.concat_windows(wp, coords, counts, 3), sd)
        want = torch.autograd.grad((out * G).sum(), [wp] + [sd[k] for k in R.FUSER])
        l1 = R.torch_bilinear(fx["preds"].double(), 18, 18)
    a, c, d = sd[R.FUSER[0]].detach().reshape(64), sd[R.FUSER[1]].detach(), sd[R.FUSER[2]].detach().reshape(64)
    got = R.ge_bwd(l1, ref["h_preds"], w.detach(), a, c, d, G)
    dwin = R.gather(got["dl2"], coords, img, 6, 6, 3)
    assert dwin.shape[0] == (18 if tag == "full" else 6)
    for mine, ref_t in zip((dwin, got["d_a"], got["d_c"], got["d_d"], got["d_b"]), want):
        assert R.rel_l2(mine.reshape(-1), ref_t.reshape(-1)) < 1e-12
    assert R.rel_l2(dwin, ref["out"]["d_window_preds"]) < 1e-12


def small_bound(f32, f64):
    """the GPU kernel test's bound (tests/test_gpu_refiner_outputs.py)"""
    return max(4.0 * R.rel_l2(f32, f64), 1e-5)


GATHER_BOUND = 2.0 ** -22          # the GPU gather test's bound: one f32 rounding of the divisor and one of the quotient


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_fault_exceeds_a_bound(fault):
    """Each lost term moves at least one output of a kernel case beyond the bound the GPU test uses for it."""
    if fault in ("no_div", "wrong_cell"):
        case = R.GATHER_CASES[0]
        dl2, _, coords, img = R.gather_inputs(case)
        ws, H, W = case[:3]
        assert R.rel_l2(R.gather(dl2, coords, img, H, W, ws, fault=fault), R.gather(dl2, coords, img, H, W, ws)) > (2 if fault == "no_div" else 1e5) * GATHER_BOUND
        return
    case = (2, 18, 18, "mixed")
    x = R.kernel_inputs(case)
    ref, f32 = R.kernel_expected(case)
    bad = R.ge_bwd(**x, fault=fault)
    over = {k: R.rel_l2(bad[k], ref[k]) / small_bound(f32[k], ref[k]) for k in R.GE_OUT if R.rel_l2(bad[k], ref[k]) > small_bound(f32[k], ref[k])}
    assert over, fault
    if fault == "ge_gate":                                               # the dead channel: z_k == 0 exactly at every pixel, subgradient 0
        assert float(ref["d_c"][5]) == 0.0 and float(bad["d_c"][5]) != 0.0


@pytest.mark.parametrize("case", R.GE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_kink_margin_holds_on_every_kernel_case(case):
    x = R.kernel_inputs(case)                                            # asserts it
    assert int(R.kink_pairs(x["l1"], x["l2"], x["w"], x["a"], x["c"]).sum()) == 0
    ref, f32 = R.kernel_expected(case)
    for k in R.GE_OUT:
        assert R.rel_l2(f32[k], ref[k]) < 1e-5, (k, R.rel_l2(f32[k], ref[k]))      # f32 and f64 agree on every gate: no whole term apart
    if case[3] == "onesided":
        y, z = R.pre_activation(x["l1"], x["l2"], x["w"], x["a"], x["c"], torch.float64)
        dead = (z <= 0).all(1, keepdim=True)
        assert 50 < int(dead.sum()) < dead.numel() - 50 and bool((ref["dl2"][dead] == 0).all())
    sizes = {(1, 6, 6): 1, (2, 18, 18): 2 * 2, (3, 12, 21): 3, (1, 16, 16): 1, (3, 63, 63): 3 * 16}
    assert sizes[case[:3]] == case[0] * -(-case[1] * case[2] // 256)    # workgroups: every tile walk the cases were chosen for


def test_config_key_defaults_to_off():
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.models.UDLR import SparseRefiner
    m = SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015)))
    assert m.train_outputs is False and m.csf_backward_calls == 0
    assert SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015, train_outputs=True))).train_outputs is True
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in SparseRefiner(None, 3, 0.0015, train_outputs=True).named_parameters()]


def test_descent_reference_decreases():
    """the f64 losses the GPU descent check quotes: every step gains more than SGD_OUT_FACTOR x the f32 noise on the loss"""
    losses = R.fuser_sgd_losses(R.SGD_OUT_LR)
    assert all(abs(a - b) < 5e-6 for a, b in zip(losses, R.SGD_OUT_F64)), losses
    assert min(a - b for a, b in zip(losses, losses[1:])) > R.SGD_OUT_FACTOR * R.SGD_OUT_NOISE
    assert set(R.descent_target().unique().tolist()) == {0.0, 1.0}
