"""CPU: what makes the LoRA row-kernel tests of tests/test_gpu_lora_rows.py legitimate, and what they can see.

1. lora_rows_ref.ln_bwd_closed_form (the kernel header's formula, f64) and the LoRA branch against f64 torch autograd, a massive-activation row included.
2. The rounding model with its roundings switched off is the reference.
3. Coverage: lora_rows_ref.ln_bwd_instance / ln_lora_instance restate launch_ln_bwd / launch_ln_lora of csrc/vit_train.hip; the case lists reach every
   instantiation those can reach (12 widths x 9 forms of ln_bwd_kernel, 9 widths x 4 forms of ln_lora*), and the refused widths are refused.
4. The mask restatement: thresholds 0 / 307 / 1023 at p = 0.0005 / 0.3 / 0.9995, fields of the three projections independent, kept elements unbiased.
5. The yardstick: every case's model error is non-zero and below its floor-free bound, so no GPU check can pass vacuously.
6. Checker sensitivity: a projection's mask taken from another 10-bit field, the branch left out of one projection, a rank read at the wrong offset, a
   dropped chunk of the row -- each injected into the model -- are rejected by the same checks the GPU outputs go through.
"""
import pytest
import torch

import lora_rows_ref as R
from oracle import vit as OV


# ================================================================================================ 1. reference against autograd
@pytest.mark.parametrize("rows,D,kind,lora", [(5, 128, "randn", 0), (7, 384, "massive", 3), (3, 256, "massive", 1), (4, 640, "randn", 3)])
def test_closed_form_backward_equals_f64_autograd(rows, D, kind, lora):
    g = torch.Generator().manual_seed(rows + D)
    x = R.make_x(rows, D, kind, g).double().requires_grad_(True)
    gam, bet = torch.randn(D, generator=g).double(), torch.randn(D, generator=g).double()
    dy, dres = torch.randn(rows, D, generator=g).double(), torch.randn(rows, D, generator=g).double()
    y = OV.layer_norm(x, gam, bet, R.EPS)
    cot = dy
    t = A = drop = None
    if lora:
        r = 3
        drop = R.drop_of(0.3)
        _, mats = R.arena(r, D, g, lora)
        A = [a for a, _ in mats]
        t = torch.randn(rows, lora * r, generator=g).double()
        m = R.masks(drop, rows, D, lora)
        # the branch as the forward has it: u_p = (y mask_p) A_p^T, with cotangent t_p
        loss_lora = sum((((y * m[p]) @ A[p].double().t()) * t[:, p * r:(p + 1) * r]).sum() for p in range(lora))
    else:
        loss_lora = 0.0
    (gx,) = torch.autograd.grad((y * cot).sum() + loss_lora, x)
    got = R.ln_bwd(dy, x.detach(), gam, dres, None, t, A, drop)["dx"]
    err = float((got - (gx + dres)).abs().max() / (gx + dres).abs().max())
    assert err < 1e-12, err


def test_forward_reference_equals_the_oracle_layer_norm_and_projection():
    case = R.FwdCase("lora", 384, 5, 2, 0.3, "massive")
    i = R.fwd_inputs(case)
    ref, _ = R.fwd_expected(case)
    y = OV.layer_norm(i["x"].double(), i["gamma"].double(), i["beta"].double(), R.EPS)
    assert float((ref["y"] - y).abs().max()) < 1e-12
    for p, (A, _) in enumerate(i["mats"]):
        m = OV.lora_dropout_mask(R.SEED, 3, p, case.rows, case.D, 0.3).double()
        assert float((ref["u"][:, p * 2:(p + 1) * 2] - (y * m) @ A.double().t()).abs().max()) < 1e-12


# ================================================================================================ 2. model without rounding == reference
def test_model_with_rounding_switched_off_is_the_reference():
    for case in R.FWD_CASES[::7]:
        i = R.fwd_inputs(case)
        A = [a for a, _ in i["mats"]]
        off = R.ln_lora(i["x"], i["gamma"], i["beta"], A, R.drop_of(case.p), rnd=R._exact)
        ref, _ = R.fwd_expected(case)
        assert torch.equal(off["y"], ref["y"]) and torch.equal(off["u"], ref["u"])
    for case in R.BWD_CASES[::7]:
        i = R.bwd_inputs(case)
        A = [a for a, _ in i["mats"]] if i["mats"] else None
        off = R.ln_bwd(i["dy"], i["x"], i["gamma"], i["dres"], i["scale"], i["t"], A, R.drop_of(case.p), rnd_dx=R._exact, rnd_s=R._exact)
        ref, _ = R.bwd_expected(case)
        assert torch.equal(off["dx"], ref["dx"]) and torch.equal(off["s"], ref["s"])


# ================================================================================================ 3. coverage
def test_case_lists_reach_every_reachable_instantiation():
    widths = range(128, 2049, 128)
    reach_bwd = {R.ln_bwd_instance(e, D, f) for e, (_, fl) in R.LN_BWD_ENTRIES.items() for f in fl for D in widths} - {None}
    assert reach_bwd == R.ALL_LN_BWD and len(reach_bwd) == 12 * 9                   # the restated table reaches all the launch function instantiates
    have_bwd = {R.ln_bwd_instance(c.entry, c.D, c.flags, c.r) for c in R.BWD_CASES}
    assert None not in have_bwd
    assert have_bwd == R.ALL_LN_BWD, sorted(R.ALL_LN_BWD - have_bwd)
    reach_fwd = {R.ln_lora_instance(e, D, 2) for e in R.LN_LORA_ENTRIES for D in widths} - {None}
    assert reach_fwd == R.ALL_LN_LORA and len(reach_fwd) == 9 * 4
    have_fwd = {R.ln_lora_instance(c.entry, c.D, c.r) for c in R.FWD_CASES}
    assert have_fwd == R.ALL_LN_LORA, sorted(R.ALL_LN_LORA - have_fwd)
    # every entry point of the issue's list is driven by at least one case, each plain entry with and without dres / next_scale, each LoRA entry with p = 0 and 0.3
    for entry in R.LN_BWD_ENTRIES:
        mine = [c for c in R.BWD_CASES if c.entry == entry]
        assert {c.dres for c in mine} == {False, True} and {c.scale for c in mine} == {False, True} and {c.rows for c in mine} == set(R.ROWS), entry
        if R.LN_BWD_ENTRIES[entry][0]:
            assert {c.p for c in mine} == {0.0, 0.3}, entry
    for entry in R.LN_LORA_ENTRIES:
        mine = [c for c in R.FWD_CASES if c.entry == entry]
        assert {c.p for c in mine} == {0.0, 0.3} and {c.rows for c in mine} == set(R.ROWS) and {c.kind for c in mine} == {"randn", "massive"}, entry
    # rank: the three unrolled branches and the generic loop, for both LORA forms
    for entry, ranks in (("bwd_lora_ex", {1, 2, 3, 4, 5, 8, 21}), ("bwd_lora_mlp", {1, 2, 3, 4, 8})):
        assert {c.r for c in R.RANK_BWD_CASES if c.entry == entry} == ranks


def test_refusals_of_the_restated_dispatch():
    for D in R.LN_LORA_REFUSED_D:
        assert all(R.ln_lora_instance(e, D, 2) is None for e in R.LN_LORA_ENTRIES), D
    assert R.ln_bwd_instance("bwd_ex", 1664, 1) is None and R.ln_bwd_instance("bwd", 1664, None) is None
    assert R.ln_bwd_instance("bwd_ex", 768, 2) is None and R.ln_bwd_instance("bwd_lora_ex", 768, 2) is None and R.ln_bwd_instance("bwd_lora_mlp", 768, 2) is None
    assert R.ln_bwd_instance("bwd_lora_ex", 768, 1, 22) is None and R.ln_bwd_instance("bwd_lora_mlp", 768, 1, 9) is None
    assert R.ln_lora_instance("lora", 128, 22) is None and R.ln_lora_instance("lora_mlp", 128, 9) is None
    # the LDS boundary: 3 r D 4 bytes against one workgroup's 160 KiB
    want = {(768, 7): True, (768, 8): True, (768, 17): True, (768, 18): False, (1024, 6): True, (1536, 4): True, (1536, 8): True, (1536, 9): False}
    assert set(want) == set(R.LDS_CASES)
    for (D, r), fits in want.items():
        assert (R.ln_lora_instance("lora", D, r) is not None) == fits, (D, r)
    asks = {(D, r) for D, r in R.LDS_CASES if 3 * r * D * 4 > R.LDS_ASK}
    assert asks == set(R.LDS_CASES) - {(768, 7)}


def test_edge_rows_hold_the_turn_of_the_second_trip():
    assert R.edge_rows(1) == [0] and R.edge_rows(9) == [0, 1, 7, 8]
    e = R.edge_rows(32769)
    assert set(range(16383, 16393)) <= set(e) and {0, 32768, 8191, 8193, 16376}.issubset(e) and len(e) < 64


# ================================================================================================ 4. the mask
def test_mask_thresholds_and_unbiasedness():
    assert [R.drop_threshold(p) for p in (0.0005, 0.3, 0.9995)] == [0, 307, 1023]
    rows, D = 512, 256
    for p, T in ((0.0005, 0), (0.3, 307), (0.9995, 1023)):
        ms = [OV.lora_dropout_mask(R.SEED, 3, proj, rows, D, p).double() for proj in range(3)]
        inv = 1.0 / (1.0 - T / 1024.0)
        for m in ms:
            assert set(m.unique().tolist()) <= {0.0, float(torch.tensor(inv, dtype=torch.float32))}
        if T == 0:
            assert all(bool((m == 1.0).all()) for m in ms)                      # below 1 / 1024: no dropout at all
            assert all(bool((a == 1.0).all()) for a in R.masks(R.drop_of(p), 4, 128, 3))
            continue
        n = rows * D
        for m in ms:
            keep = float((m > 0).double().mean())
            sigma = (T / 1024.0 * (1 - T / 1024.0) / n) ** 0.5
            assert abs(keep - (1 - T / 1024.0)) < 5 * sigma, (p, keep)          # the kept fraction is 1 - T / 1024 ...
            assert abs(float(m.mean()) - 1.0) < 5 * sigma * inv, (p, float(m.mean()))   # ... and the mask has mean 1
        if T == 307:                                                            # three fields of one mix: pairwise different, pairwise uncorrelated
            for a, b in ((0, 1), (0, 2), (1, 2)):
                both = float(((ms[a] > 0) & (ms[b] > 0)).double().mean())
                assert abs(both - (1 - T / 1024.0) ** 2) < 5e-3, (a, b, both)
    assert not torch.equal(OV.lora_dropout_mask(R.SEED, 3, 0, 8, 128, 0.3), OV.lora_dropout_mask(R.SEED, 4, 0, 8, 128, 0.3))     # the layer is part of the key


# ================================================================================================ 5. the yardstick
def test_model_error_is_non_zero_and_below_the_bounds_in_every_case():
    n = 0
    for case in R.FWD_CASES + R.RANK_FWD_CASES:
        ref, model = R.fwd_expected(case)
        for name in ("y", "u"):
            e = float(R.row_err(model[name], ref[name]).max())
            top = float(ref[name].abs().max())
            assert 0 < e <= 2.0 ** -8 * top * (1 + 1e-9), (case, name, e)                       # one bf16 rounding: at most half an ulp, 2^-8 of the largest value
            assert bool((R.row_err(model[name], ref[name]) <= R.bf16_row_bound(ref[name], model[name], floor=False)).all())
            n += 1
    for case in R.BWD_CASES + R.RANK_BWD_CASES:
        ref, model = R.bwd_expected(case)
        e = float(R.row_err(model["s"], ref["s"]).max())
        assert 0 < e <= 2.0 ** -8 * float(ref["s"].abs().max()) * (1 + 1e-9), (case, e)
        edx = R.row_err(model["dx"], ref["dx"]) / ref["dx"].abs().amax(1).clamp_min(1.0)
        assert 0 < float(edx.max()) < R.DX_TOL / 100, (case, float(edx.max()))                   # f32 rounding: two orders below the bar the kernel is held to
        n += 1
    for case in R.GRAD_CASES:
        i = R.grad_inputs(case)
        B = [b for _, b in i["mats"]]
        t_ref, t_model = R.lora_t(i["dqkv"], B, i["scaling"]), R.lora_t(i["dqkv"], B, i["scaling"], rnd=R.bf16_round)
        assert 0 < float(R.row_err(t_model, t_ref).max()) <= 2.0 ** -8 * float(t_ref.abs().max()) * (1 + 1e-9)
        dA, dB = R.lora_grads(i["dqkv"], i["h"], i["u"], t_model, i["scaling"], R.drop_of(case.p))
        dAm, dBm = R.lora_grads(i["dqkv"], i["h"], i["u"], t_model, i["scaling"], R.drop_of(case.p), rnd=R.f32_round)
        for ref, model in zip(dA + dB, dAm + dBm):
            e = R.row_err(model, ref) / ref.abs().amax(1).clamp_min(1.0)
            assert float(e.max()) < R.GRAD_TOL / 100
        # (one row: every gradient element is a single product of two bf16 values, exact in f32 -- the model's error is rightly zero there)
        assert case.rows == 1 or any(float(R.row_err(m, r_).max()) > 0 for r_, m in zip(dA + dB, dAm + dBm))
        n += 1
    print(f"{n} (case, output) yardsticks checked")


# ================================================================================================ 6. what the checker rejects
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_checker_rejects_the_faults_the_gpu_cases_are_there_for():
    # forward, p = 0.3: the key projection's mask read from another 10-bit field; no dropout at all (the "far off" claim of the GPU test)
    case = R.FwdCase("lora", 384, 37, 2, 0.3, "randn")
    i = R.fwd_inputs(case)
    ref, model = R.fwd_expected(case)
    R.check_bf16("ok", model["u"], ref["u"], model["u"], audit=False)
    A = [a for a, _ in i["mats"]]
    plain = R.ln_lora(i["x"], i["gamma"], i["beta"], A, None, rnd=R.bf16_round)
    _rejected(lambda: R.check_bf16("undropped", plain["u"], ref["u"], model["u"], audit=False))
    assert float(R.row_err(plain["u"], ref["u"]).max()) > 50 * float(R.bf16_row_bound(ref["u"], model["u"]).max())        # far off: not a near miss
    swapped = model["u"].clone()
    y = ref["y"]
    m = R.masks(R.drop_of(0.3), case.rows, case.D, 3)
    swapped[:, 2:4] = R.bf16_round((y * m[2]) @ A[1].double().t())                           # the key projection under the value projection's field
    _rejected(lambda: R.check_bf16("wrong field", swapped, ref["u"], model["u"], audit=False))
    # a dropped chunk of the row (NCH off by one at D = 1280): the mean moves, every element of y is off
    case = R.FwdCase("lora", 1280, 5, 2, 0.0, "massive")
    i = R.fwd_inputs(case)
    ref, model = R.fwd_expected(case)
    short = R.ln_lora(i["x"][:, :1024], i["gamma"][:1024], i["beta"][:1024], [a[:, :1024] for a, _ in i["mats"]], None, rnd=R.bf16_round)
    _rejected(lambda: R.check_bf16("chunk", short["y"], ref["y"][:, :1024], model["y"][:, :1024], audit=False))
    # backward: the generic-rank loop reading p R with the wrong R (the value module's t taken one column early), and ldt without the 64 (the next row's t
    # shifted by 64 columns: here, a t that belongs to another row)
    case = R.BwdCase("bwd_lora_ex", 1, 768, 5, 3, True, True, 0.3, "randn")
    i = R.bwd_inputs(case)
    ref, model = R.bwd_expected(case)
    A = [a for a, _ in i["mats"]]
    R.check_f32("ok", model["dx"], ref["dx"], R.DX_TOL, audit=False)
    for name, t_bad in (("wrong R", torch.cat((i["t"][:, :6], i["t"][:, 5:8]), 1)), ("wrong row", i["t"].roll(1, 0))):
        bad = R.ln_bwd(i["dy"], i["x"], i["gamma"], i["dres"], i["scale"], t_bad, A, R.drop_of(case.p), rnd_dx=R.f32_round, rnd_s=R.bf16_round)
        _rejected(lambda: R.check_f32(name, bad["dx"], ref["dx"], R.DX_TOL, audit=False))
        _rejected(lambda: R.check_bf16(name, bad["s"], ref["s"], model["s"], audit=False))
