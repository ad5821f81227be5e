"""CPU: the f64 restatement that tests/test_gpu_disc_feature_grad.py holds the gradient into the features against (tests/disc_feature_grad_ref.py) is
itself right: it reproduces the real module's probabilities (G3b), torch autograd through binary_cross_entropy_with_logits' target and clamp gives the closed
forms ucod_apm_bce_gprob computes (and a wrong closed form leaves the GPU test's bound), the index map of ucod_conv3x3_dgrad_weights is the adjoint of the
convolution, and the discriminator's share of the LoRA gradients in the step test is far outside that test's bar."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub, maxdiff

import disc_feature_grad_ref as R


def test_restatement_reproduces_the_real_modules_probabilities():
    """G3b: the reference module's two calls (dis_use_features=True, dim 32, fs 20) -- to the 1e-5 the GPU test of the forward already uses"""
    g = load_golden("g3b_discriminator_features")
    sd = R.to64(sub(g, "sd0."))
    for tag, mk, fk in (("prob", "mask", "feature"), ("prob2", "mask2", "feature2")):
        p = R.disc_prob(g[mk].double(), g[fk].double(), sd)
        assert maxdiff(p.view(-1, 1), g[tag]) < 1e-5, (tag, maxdiff(p.view(-1, 1), g[tag]))
    assert int(sd["featureConv.layers.1.num_batches_tracked"]) == int(g["sd0.featureConv.layers.1.num_batches_tracked"]) + 2


GPROB_GRID = list(itertools.product((7, 144, 257), (0.0, 0.6), (0, 1), (1.0, 0.5)))


@pytest.mark.parametrize("HW,epoch_frac,finetune,gscale", GPROB_GRID)
def test_closed_forms_of_gprob_are_what_autograd_gives(HW, epoch_frac, finetune, gscale):
    pl, teacher, fg, bg, p_s, p_p = R.gprob_cases(HW, torch.Generator().manual_seed(HW))
    ref_s, ref_p = R.gprob_autograd(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
    got_s, got_p, bound = R.gprob_closed_form(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
    tol = 1e-12 * (1 + ref_s.abs())
    assert bool(((got_s - ref_s).abs() <= tol).all()) and bool(((got_p - ref_p).abs() <= 1e-12 * (1 + ref_p.abs())).all())
    # the case list holds what it says: image 2 has D = 0 exactly (target part 0 on both sides); at epoch_frac 0.6 images 0-3 are clamped, image 4 is not
    assert float(ref_p[2]) == 0.0
    if epoch_frac:
        assert all(float(ref_p[i]) == 0.0 for i in (0, 1, 2, 3)) and float(ref_p[4]) != 0.0
    else:
        assert float(ref_p[0]) != 0.0 and float(ref_p[1]) != 0.0
    if not finetune:                                              # p_s = 1 exactly: the 1e-12 denominator
        assert abs(float(ref_s[5]) + gscale * 1e12 / 6) < 1e-3 * 1e12


@pytest.mark.parametrize("HW,epoch_frac,finetune,gscale", GPROB_GRID)
def test_a_wrong_closed_form_leaves_the_gpu_tests_bound(HW, epoch_frac, finetune, gscale):
    pl, teacher, fg, bg, p_s, p_p = R.gprob_cases(HW, torch.Generator().manual_seed(HW))
    ref_s, ref_p = R.gprob_autograd(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
    _, _, bound = R.gprob_closed_form(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
    for mutate in ("no_target", "gp_p_sign", "no_1_over_B"):
        if mutate == "no_1_over_B" and finetune:
            continue                                              # (the dis_loss part is absent: nothing to get wrong)
        mut_s, mut_p, _ = R.gprob_closed_form(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune, mutate=mutate)
        outside = ((mut_s - ref_s).abs() > bound) | ((mut_p - ref_p).abs() > bound)
        assert bool(outside.any()), mutate
        live = 4 if epoch_frac else 0                             # an image whose target part is not clamped away
        assert bool(outside[live]), (mutate, live)


@pytest.mark.parametrize("Cout,Cin,H,W", [(16, 16, 6, 5), (40, 5, 7, 3), (136, 23, 4, 4), (3, 2, 1, 5)])
def test_dgrad_weight_index_map_is_the_adjoint(Cout, Cin, H, W):
    """<conv(x; W), g> = <x, conv(g; Wd)> in f64 with Wd read as the [Cin,Cout,3,3] weight its columns stand for"""
    gen = torch.Generator().manual_seed(Cout)
    Wt = torch.randn(Cout, Cin, 3, 3, generator=gen, dtype=torch.float64)
    x = torch.randn(2, Cin, H, W, generator=gen, dtype=torch.float64)
    g = torch.randn(2, Cout, H, W, generator=gen, dtype=torch.float64)
    wd = R.dgrad_weights_index(Wt)
    assert wd.shape == (Cin, (9 * Cout + 15) // 16 * 16) and float(wd[:, 9 * Cout:].abs().max() if wd.shape[1] > 9 * Cout else 0.0) == 0.0
    lhs = (F.conv2d(x, Wt, None, 1, 1) * g).sum()
    gx = F.conv2d(g, R.wd_as_conv_weight(wd, Cout), None, 1, 1)
    rhs = (x * gx).sum()
    assert abs(float(lhs - rhs)) < 1e-10 * max(1.0, abs(float(lhs)))
    ref, _ = R.conv3x3_dgrad_f64(g, Wt)
    assert maxdiff(gx, ref) < 1e-10


def test_conv_bound_covers_an_f32_convolution():
    gen = torch.Generator().manual_seed(3)
    x, Wt = torch.randn(2, 23, 7, 9, generator=gen), torch.randn(40, 23, 3, 3, generator=gen)
    ref, bound = R.conv3x3_f64(x, Wt)
    err = (F.conv2d(x, Wt, None, 1, 1).double() - ref).abs()
    assert bool((err <= bound).all()) and float(bound.max()) < 1e-3 * float(ref.abs().max())


def rel_l2(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_discriminators_share_of_the_lora_gradients_is_outside_the_step_tests_bar():
    """the step test holds the LoRA gradients to 8e-2 rel-L2 against f64 autograd of the whole step.  At the chosen seed and scales (R.STEP_*) the same
    autograd WITHOUT the discriminator's term (detached features: the frozen-backbone graph) misses that bar by an order of magnitude -- on
    encoder.layer.1.attention.attention.key.lora_A.weight, and with the dis_loss part gone (finetune) on layer 1's query.lora_A -- so a step that dropped the
    new gradient could not pass; and image 1 has 0 < u < 1 well inside (the target path is live)."""
    case = R.step_case()
    for finetune, name in ((False, "encoder.layer.1.attention.attention.key.lora_A.weight"), (True, "encoder.layer.1.attention.attention.query.lora_A.weight")):
        full = R.full_step_lora_grads(case, finetune=finetune, with_disc=True)
        part = R.full_step_lora_grads(case, finetune=finetune, with_disc=False)
        assert torch.equal(full["p_s"], part["p_s"]) and float(full["loss"]) == float(part["loss"])
        assert rel_l2(part["grads"][name], full["grads"][name]) > 10 * 8e-2, (name, rel_l2(part["grads"][name], full["grads"][name]))
        assert 0.05 < float(full["u"][1]) < 0.95 and 0.0 < float(full["u"][0]) < 1.0, full["u"]
