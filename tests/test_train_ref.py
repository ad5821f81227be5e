"""CPU: the references and the bound of tests/test_gpu_train_kernels.py (tests/train_ref.py).

(1) The cap: on every listed case, every compared slice of the f32 reference is within 1e-4 of the f64 one (relative to the slice's
    max|ref64|), so a bound relative to the reference's own rounding is meaningful there.  No case is skipped.
(2) Sensitivity: wrong variants of the f64 reference -- each a bug a kernel could have -- fail the bound e_k <= 8 max(e_32, 2^-23) against the
    true f64 reference with the case's own e_32, so the slicing and the bound would catch that bug in a kernel.
"""
import math

import pytest
import torch

import train_ref as TR
from oracle import decoder as OD

F64, F32 = torch.float64, torch.float32


def _cap_ok(e32):
    return bool((e32 <= TR.CAP).all())


def _decoder_case(case_id):
    return next(c for c in TR.DECODER_CASES if c["id"] == case_id)


def test_compare_slices_and_zero_slices():
    ref = torch.tensor([[1.0, -2.0], [1e-6, 0.0], [0.0, 0.0]], dtype=F64)
    k = ref + torch.tensor([[1e-7, 0.0], [1e-12, 0.0], [0.0, 0.0]], dtype=F64)
    ek, e32 = TR.compare(k, ref, ref.float(), 1)
    assert torch.allclose(ek, torch.tensor([5e-8, 1e-6, 0.0], dtype=F64))
    assert float(e32[2]) == 0.0
    k[2, 1] = 1e-30                                              # a zero slice of ref64 must be EXACTLY zero in the kernel
    ek, _ = TR.compare(k, ref, ref.float(), 1)
    assert ek[2] == math.inf and not TR.passes(ek, e32)
    k[0, 0] = math.nan
    ek, _ = TR.compare(k, ref, ref.float(), 0)
    assert not TR.passes(ek, e32[:1])
    assert TR.bound(0.0) == 8 * 2.0 ** -23 and TR.bound(1e-6) == 8e-6


# ----------------------------------------------------------------------------------------------------------- (1) the cap
@pytest.mark.parametrize("case", TR.DECODER_CASES, ids=[c["id"] for c in TR.DECODER_CASES])
def test_decoder_reference_within_cap(case):
    inp = TR.decoder_inputs(case)
    r64 = TR.decoder_ref(inp, case["c0"], F64)
    r32 = TR.decoder_ref(inp, case["c0"], F32)
    for k, s in TR.DECODER_FWD_SLICES.items():
        _, e32 = TR.compare(r32[k], r64[k], r32[k], s)
        assert _cap_ok(e32), (k, float(e32.max()))
    for mode in inp["modes"]:
        for k, s in TR.DECODER_BWD_SLICES.items():
            _, e32 = TR.compare(r32[mode][k], r64[mode][k], r32[mode][k], s)
            assert _cap_ok(e32), (mode, k, float(e32.max()))
    if case["clamp"]:                                            # the clamped-norm branch is taken: gfeat / 1e-12 dominates those gd rows
        for r in TR.CLAMPED_ROWS:
            assert float(r64["norm"][:, r].max()) == OD.NORM_EPS
            assert r64["orth"]["gd"][:, r].abs().max() > 1e3 * r64["orth"]["gd"][:, r + 1].abs().max()



@pytest.mark.parametrize("fs,B", TR.DISC_CASES)
def test_discriminator_reference_within_cap(fs, B):
    sd, masks, gprobs = TR.disc_inputs(fs, B)
    r64 = TR.disc_ref(sd, masks, gprobs, F64)
    r32 = TR.disc_ref(sd, masks, gprobs, F32)
    for c in range(2):
        _, e32 = TR.compare(r32["prob"][c], r64["prob"][c], r32["prob"][c], 0)
        assert _cap_ok(e32), ("prob", c, float(e32.max()))
        for k in TR.DISC_RUNNING:
            _, e32 = TR.compare(r32["running"][c][k], r64["running"][c][k], r32["running"][c][k], 0)
            assert _cap_ok(e32), (k, c, float(e32.max()))
    for k in TR.DISC_GRADS:
        a, b = TR.disc_grad_view(k, r32["grads"][k], fs), TR.disc_grad_view(k, r64["grads"][k], fs)
        _, e32 = TR.compare(a, b, a, TR.DISC_GRAD_SLICES.get(k, 0))
        assert _cap_ok(e32), (k, float(e32.max()))
    assert r64["nbt"] == r32["nbt"] == [int(sd[k]) + 2 for k in TR.NBT_KEYS]


@pytest.mark.parametrize("B", TR.BCE_BATCHES)
def test_bce_reference_within_cap(B):
    ps, pp = TR.bce_inputs(B)
    r64, r32 = TR.bce_ref(ps, pp, F64), TR.bce_ref(ps, pp, F32)
    for k, s in (("g_student", 1), ("g_pseudo", 1), ("loss", 0)):
        _, e32 = TR.compare(r32[k], r64[k], r32[k], s)
        assert _cap_ok(e32), (k, float(e32.max()))


@pytest.mark.parametrize("frac", TR.APM_FRACS)
def test_apm_reference_within_cap(frac):
    inp = TR.apm_inputs()
    r64, r32 = TR.apm_ref(inp, frac, TR.APM_GSCALE, F64), TR.apm_ref(inp, frac, TR.APM_GSCALE, F32)
    for k, s in TR.APM_SLICES.items():
        _, e32 = TR.compare(r32[k], r64[k], r32[k], s)
        assert _cap_ok(e32), (k, float(e32.max()))


# ----------------------------------------------------------------------------------------------------------- (2) sensitivity
def _decoder_fails(case_id, bug, mode, key, modes=None):
    case = _decoder_case(case_id)
    inp = TR.decoder_inputs(case)
    r64 = TR.decoder_ref(inp, case["c0"], F64, modes=modes)
    r32 = TR.decoder_ref(inp, case["c0"], F32, modes=modes)
    wrong = TR.decoder_ref(inp, case["c0"], F64, bug=bug, modes=modes)
    pick = (lambda r: r[key]) if mode is None else (lambda r: r[mode][key])
    slices = TR.DECODER_FWD_SLICES[key] if mode is None else TR.DECODER_BWD_SLICES[key]
    ek, e32 = TR.compare(pick(wrong), pick(r64), pick(r32), slices)
    assert _cap_ok(e32)
    return not TR.passes(ek, e32), float(ek.max()), float(TR.bound(e32).max())


def test_sensitivity_orth_coefficient_normalised_by_b_hw():
    """orthogonality-only upstream gradient: a coefficient 2 gextra / (B HW) instead of 2 gextra / (B HW^2)"""
    fails, ek, b = _decoder_fails("b3_c384_h23", "orth_bhw", "orth", "gd", modes=("orth",))
    assert fails, (ek, b)


def test_sensitivity_gram_missing_the_last_pixel_at_hw_4624():
    """each image's last pixel missing from the Gram sums at HW = 4624 (ten 512-pixel chunks, a 16-pixel tail): caught per (image, branch)"""
    fails, ek, b = _decoder_fails("b32_c768_h68", "gram_drop_last", None, "gram", modes=())
    assert fails, (ek, b)


def test_sensitivity_gate_derivative_without_the_residual_term():
    """the gate term of gd without the +1 of d(sigmoid(f d) + d)/dd"""
    fails, ek, b = _decoder_fails("b3_c384_h16", "gate_no_residual", "gate", "gd", modes=("gate",))
    assert fails, (ek, b)


def _disc_fails(fs, B, bug, keys, drop_image=0):
    sd, masks, gprobs = TR.disc_inputs(fs, B)
    r64 = TR.disc_ref(sd, masks, gprobs, F64)
    r32 = TR.disc_ref(sd, masks, gprobs, F32)
    wrong = TR.disc_ref(sd, masks, gprobs, F64, bug=bug, drop_image=drop_image)
    out = {}
    for k in keys:
        if k in TR.DISC_RUNNING:
            ek, e32 = TR.compare(wrong["running"][0][k], r64["running"][0][k], r32["running"][0][k], 0)
        else:
            ek, e32 = TR.compare(TR.disc_grad_view(k, wrong["grads"][k], fs), TR.disc_grad_view(k, r64["grads"][k], fs),
                                 TR.disc_grad_view(k, r32["grads"][k], fs), TR.DISC_GRAD_SLICES.get(k, 0))
        assert _cap_ok(e32)
        out[k] = not TR.passes(ek, e32)
    return out


def test_sensitivity_first_layer_wgrad_missing_the_last_image_of_a_chunk_at_b37():
    """B = 37: the first layer's weight gradient is split into chunks_for(32) image chunks; the last image of chunk 5 left out"""
    B = 37
    chunks = TR.chunks_for(32, B)
    lo, hi = TR.chunk_range(B, chunks, 5)
    assert hi > lo
    fails = _disc_fails(37, B, "w1_drop_image", ("w1",), drop_image=hi - 1)
    assert fails["w1"]


def test_sensitivity_stride2_dgrad_missing_the_far_boundary_taps_at_fs37():
    """37 -> 19 -> 10: the input gradient of the stride-2 convs without the taps into the bottom row / right column"""
    fails = _disc_fails(37, 37, "dgrad_no_far_taps", ("w1", "w2"))
    assert fails["w1"] and fails["w2"], fails


def test_sensitivity_running_var_with_the_biased_variance_at_fs4_b2():
    """n = 32 and 8 values per channel in the first two layers (the third conv of this case is scaled down, train_ref.disc_inputs, so that its
    batch variance is ~1e-5 against running_var ~1: the factor n / (n - 1) = 2 moves rv3 by ~5e-7, inside the bound)"""
    fails = _disc_fails(4, 2, "running_var_biased", ("rv1", "rv2"))
    assert fails["rv1"] and fails["rv2"], fails


def test_sensitivity_batchnorm_backward_without_the_mean_term():
    fails = _disc_fails(28, 4, "bn_bwd_no_mean", ("w1", "w2", "w3"))
    assert all(fails.values()), fails


def test_sensitivity_disc_bce_gradient_without_the_clamp_at_p1():
    ps, pp = TR.bce_inputs(7)
    assert float(ps[0]) == 1.0
    r64, r32, wrong = TR.bce_ref(ps, pp, F64), TR.bce_ref(ps, pp, F32), TR.bce_ref(ps, pp, F64, bug="no_clamp")
    ek, e32 = TR.compare(wrong["g_student"][:1], r64["g_student"][:1], r32["g_student"][:1], 1)
    assert _cap_ok(e32) and not TR.passes(ek, e32), (ek, e32)
