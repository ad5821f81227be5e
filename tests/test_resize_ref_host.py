"""CPU: what makes tests/test_gpu_resize.py legitimate.

   1  the weight model of resize_ref.py is ATen's: F.interpolate(mode="bilinear", align_corners=False) in f32 lies within the forward bound of it at every
      forward case, and f32 autograd of that call within the adjoint bound plus ATen's own rounding at every adjoint case;
   2  the case lists reach every value of every axis that fwd_class / adj_class record over a grid of shapes, the launch function's tap estimate holds the
      taps the model really produces at every accepted shape, and adjoint_taps' candidate window contains them;
   3  an f32 emulation of the kernels' operation order stays within the bounds (they are not too tight), and the checker rejects each injected fault at
      every case where the fault changes the result; which of them the earlier bars (1e-5 / 2e-5 absolute, square shapes only) let through is printed.
"""
import itertools

import numpy as np
import pytest
import torch

import resize_ref as R


def _aten(x, oh, ow):
    return torch.nn.functional.interpolate(torch.from_numpy(np.array(x))[None], size=(oh, ow), mode="bilinear", align_corners=False)[0]


# ================================================================================================ 1. the model is ATen's
@pytest.mark.parametrize("c", R.FWD_CASES + R.THRESHOLD_CASES[1:2], ids=R.case_id)
def test_forward_model_is_atens(c):
    ref, bound = R.fwd_expected(c)
    r = R.ratio(_aten(R.fwd_input(c), c.oh, c.ow).numpy(), ref, bound)
    print(f"\nRATIO aten-fwd:{R.case_id(c)}  {r:.3f}")
    assert r < 1, (c, r)


@pytest.mark.parametrize("c", R.ADJ_CASES, ids=R.case_id)
def test_adjoint_model_is_atens(c):
    """f32 autograd scatters ny nx products per source pixel one after the other, each the rounded product of two weights times g: (ny nx + 2) u of the
    same magnitude sum on top of the model's own bound.  (f64 autograd is no reference: its weights are f64 and differ from the f32 ones by ~4e-5.)"""
    ref, bound = R.adj_expected(c)
    ny, nx = R.max_taps(c.ih, c.oh), R.max_taps(c.iw, c.ow)
    per_u = bound / (ny + nx + 2)
    x = torch.zeros(c.planes, c.ih, c.iw, requires_grad=True)
    (torch.nn.functional.interpolate(x[None], size=(c.oh, c.ow), mode="bilinear", align_corners=False)[0] * torch.from_numpy(np.array(R.adj_input(c)))).sum().backward()
    r = R.ratio(x.grad.numpy(), ref, bound + (ny * nx + 2) * per_u)
    print(f"\nRATIO aten-adj:{R.case_id(c)}  {r:.3f}")
    assert r < 1, (c, r)


@pytest.mark.parametrize("c", R.DYADIC_CASES, ids=R.case_id)
def test_dyadic_cases_are_exact(c):
    """integer inputs at power-of-two ratios: model, ATen f32 and the f32 emulation agree bit for bit in both directions, ties at 0.5 included"""
    for n_in, n_out in ((c.ih, c.oh), (c.iw, c.ow)):
        r = n_in / n_out
        assert r == 1 or np.log2(r) == int(np.log2(r)), c
    for kind in R.DYADIC_KINDS:
        ref, _ = R.fwd_expected(c, kind)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the model itself is not an f32 value"
        assert np.array_equal(_aten(R.fwd_input(c, kind), c.oh, c.ow).numpy(), ref)
        assert np.array_equal(R.emulate_forward(R.fwd_input(c, kind), c.oh, c.ow), ref)
        aref, _ = R.adj_expected(c, kind)
        assert np.array_equal(aref.astype(np.float32).astype(np.float64), aref)
        assert np.array_equal(R.emulate_adjoint(R.adj_input(c, kind), c.ih, c.iw), aref)
    ref, _ = R.fwd_expected(c, "mask")
    if c.oh < c.ih or c.ow < c.iw:
        assert (ref == 0.5).any(), "no tie at the threshold to decide"
    if c.oh * 2 == c.ih and c.ow * 2 == c.iw:                                  # 2x shrinking of a mask: every output is k / 4
        assert set(np.unique(ref)) <= {0.0, 0.25, 0.5, 0.75, 1.0}


def test_threshold_cases_compare_enough():
    for c in R.THRESHOLD_CASES:
        ref, _ = R.fwd_expected(c, "mask")
        _, share = R.threshold_compare(ref, ref, 0.5)
        print(f"\nSHARE {R.case_id(c)}  {share:.4f}")
        assert share >= R.THRESHOLD_SHARE, (c, share)


def test_binarize_reference():
    x = R.binarize_specials()
    out, decided = R.binarize_ref(x, False)
    assert decided.all() and out.tolist()[:8] == [0, 1, 0, 0, 0, 1, 0, 0]
    out, decided = R.binarize_ref(x, True)
    assert out.tolist()[:8] == [1, 1, 1, 0, 0, 1, 0, 0] and decided.sum() == len(x) - 1     # only 1e-30 lies in the undecided band
    t = torch.from_numpy(x)
    sig = (torch.sigmoid(t.double()) > 0.5).float().numpy()                   # the f64 sigmoid agrees wherever the reference decides
    assert np.array_equal(sig[decided], out[decided])


# ================================================================================================ 2. coverage
IN_SIZES = (1, 2, 4, 7, 12, 16, 37, 48, 68, 128, 130, 300)
OUT_SIZES = (1, 3, 4, 8, 20, 30, 31, 67, 68, 96, 256, 1024, 1028)
PLANES = (1, 63, 64, 511, 512, 2047, 2048)
LISTED = R.FWD_CASES + R.ADJ_CASES + R.ADJ_REFUSED + R.DYADIC_CASES + R.THRESHOLD_CASES


def _grid():
    for ih, iw, oh, ow in itertools.product(IN_SIZES, IN_SIZES, OUT_SIZES, OUT_SIZES):
        for p in PLANES:
            yield (p, ih, iw, oh, ow, 0)
        yield (64, ih, iw, oh, ow, 1)
    for c in LISTED:
        for p in PLANES + (c.planes,):
            for off in {0, 1, c.off}:
                yield (p, c.ih, c.iw, c.oh, c.ow, off)


def _axes(classes):
    """{(kernel, axis): set of values}; a frozenset value counts as each of its members, "several" reasons as none"""
    seen = {}
    for cl in classes:
        for k, v in cl.items():
            if k == "kernel" or k == "taps" or v == "several":
                continue
            seen.setdefault(("launch" if k == "taps_edge" else cl["kernel"], k), set()).update(v if isinstance(v, frozenset) else [v])
    return seen


def _report(name, grid, cases):
    missing = []
    for key in sorted(grid, key=str):
        lack = grid[key] - cases.get(key, set())
        print(f"COVER {name} {key[0]:7s} {key[1]:13s} grid {sorted(grid[key], key=str)}  cases {sorted(cases.get(key, ()), key=str)}")
        if lack:
            missing.append((key, sorted(lack, key=str)))
    return missing


def test_case_lists_reach_every_dispatch_class():
    shapes = set(_grid())
    print(f"\n{len(shapes)} shapes")
    fwd_grid = _axes(R.fwd_class(*s) for s in shapes)
    adj_grid = _axes(R.adj_class(*s) for s in shapes)
    assert {k for k, _ in fwd_grid} == {"elem", "lds"} and {k for k, _ in adj_grid} == {"elem", "sep", "launch"}
    assert not _report("fwd", fwd_grid, _axes(R.fwd_class(*c) for c in R.FWD_CASES))
    assert not _report("adj", adj_grid, _axes(R.adj_class(*c) for c in R.ADJ_CASES))
    # the lists are in the class they are filed under
    assert all(R.fwd_class(*c)["kernel"] == "elem" for c in R.FWD_ELEM_CASES) and all(R.fwd_class(*c)["kernel"] == "lds" for c in R.FWD_LDS_CASES)
    assert all(R.adj_class(*c)["kernel"] == "elem" for c in R.ADJ_ELEM_CASES) and all(R.adj_class(*c)["kernel"] == "sep" for c in R.ADJ_SEP_CASES)
    assert all(R.adj_class(*c)["kernel"] == "refused" for c in R.ADJ_REFUSED)
    for c in R.DYADIC_CASES:                                                  # the dyadic cases run in both dispatch classes
        assert R.fwd_class(*c)["kernel"] == ("lds" if c.planes >= 64 else "elem") and R.adj_class(*c)["kernel"] == ("sep" if c.planes >= 64 else "elem")
    # the cases named for a boundary sit on it
    assert R.fwd_class(64, 48, 64, 48, 64)["kernel"] == "lds" and 4 * 48 * 64 * 4 == 48 * 1024 and R.fwd_class(64, 48, 68, 48, 68)["why"] == "src"
    assert R.fwd_class(8, 68, 68, 600, 900)["grid_stride"] and not R.fwd_class(1, 518, 518, 1024, 683)["grid_stride"]
    assert R.adj_class(3, 4, 8, 14, 28)["taps_edge"] == "at8" and R.adj_class(3, 4, 8, 14, 28)["maxt"] == 8 and R.adj_class(3, 4, 4, 15, 15)["maxt"] == 16
    assert R.adj_class(3, 4, 4, 30, 30)["taps_edge"] == "at16" and R.adj_class(64, 50, 50, 100, 100)["why"] == "lds"


def test_tap_estimate_holds_the_taps_the_model_produces():
    """adjoint_taps drops a tap silently once n == MAXT: the launch function's estimate must be an upper bound on the nonzeros of a column of W at every
    shape it accepts.  Where it refuses, one axis really has more than 14 taps (the estimate is ceil(2 / scale) + 1 against a true count above 2 / scale - 1:
    a refusal is never off by more than two), and no shape that 16 taps would hold is refused merely because the estimate ignores the axis' length."""
    pairs = {(s[1], s[3]) for s in _grid()} | {(s[2], s[4]) for s in _grid()}
    worst = {}
    for n_in, n_out in sorted(pairs):
        true = R.max_taps(n_in, n_out)
        est = R.adjoint_tap_estimate(n_in, n_in, n_out, n_out)
        assert true <= est, (n_in, n_out, true, est)
        assert true <= n_out
        if est > 16:
            assert true > 14, (n_in, n_out, true, est)
        worst[est - true] = (n_in, n_out)
        W = R.axis_matrix(n_in, n_out)                                        # the window adjoint_taps scans holds every tap
        for i in range(n_in):
            nz = np.nonzero(W[:, i])[0]
            lo, hi = R.adjoint_window(i, n_in, n_out)
            assert len(nz) == 0 or (lo <= nz[0] and nz[-1] <= hi), (n_in, n_out, i, lo, hi, nz)
    print(f"\nestimate - true taps over {len(pairs)} axis pairs: {sorted(worst.items())}")
    for s in set(_grid()):
        cl = R.adj_class(*s)
        true = max(R.max_taps(s[1], s[3]), R.max_taps(s[2], s[4]))
        if cl["kernel"] == "refused":
            assert cl["taps"] > 16 and true > 14, (s, cl, true)
        else:
            assert true <= cl["maxt"], (s, cl, true)
    assert R.adj_class(5, 7, 1, 1, 9)["kernel"] == "elem" and R.max_taps(1, 9) == 9     # 9 outputs over one source column: 9 taps, not the 19 of 2 / scale + 1
    for c in R.ADJ_REFUSED:
        print(f"refused {R.case_id(c)}: estimate {R.adj_class(*c)['taps']}, true {max(R.max_taps(c.ih, c.oh), R.max_taps(c.iw, c.ow))}")


# ================================================================================================ 3. sensitivity
OLD_FWD_BAR, OLD_ADJ_BAR = 1e-5, 2e-5


def _sensitivity(direction, cases, faults):
    """-> {fault: [acted, rejected, square cases the old bar accepts]}"""
    table = {f: [0, 0, []] for f in faults}
    for c in cases:
        if direction == "fwd":
            data, (ref, bound), cls, bar = R.fwd_input(c), R.fwd_expected(c), R.fwd_class(*c), OLD_FWD_BAR
            run = lambda f: R.emulate_forward(data, c.oh, c.ow, f, cls)
        else:
            data, (ref, bound), cls, bar = R.adj_input(c), R.adj_expected(c), R.adj_class(*c), OLD_ADJ_BAR
            run = lambda f: R.emulate_adjoint(data, c.ih, c.iw, f, cls)
        clean = run(None)
        r = R.ratio(clean, ref, bound)
        assert r < 1, (direction, c, "the emulation of the kernel's own order misses the bound", r)
        for f in faults:
            bad = run(f)
            acts = R.fault_moves_a_weight(c, f) if f in R.WEIGHT_FAULTS else bad is not None and not np.array_equal(bad, clean, equal_nan=True)
            if not acts:
                continue                                                       # nothing for this fault to act on at this shape
            table[f][0] += 1
            rb = R.ratio(bad, ref, bound)
            assert rb > 1, (direction, c, f, "not rejected", rb)
            table[f][1] += 1
            square = c.ih == c.iw and c.oh == c.ow
            if square and np.isfinite(bad).all() and np.abs(bad - ref).max() < bar:
                table[f][2].append(R.case_id(c))
    return table


SMALL = 300_000                                                                # the emulation gathers: the three large planes are left to the GPU test


def test_the_checker_rejects_the_faults_the_cases_are_there_for():
    fwd = _sensitivity("fwd", [c for c in R.FWD_CASES if c.planes * c.oh * c.ow <= SMALL] + [R.Case(1, 37, 37, 68, 68), R.Case(4, 16, 16, 68, 68)], R.FWD_FAULTS)
    adj = _sensitivity("adj", [c for c in R.ADJ_CASES if c.planes * c.oh * c.ow <= SMALL] + [R.Case(1, 37, 37, 68, 68), R.Case(4, 10, 10, 68, 68)], R.ADJ_FAULTS)
    print()
    for name, table in (("fwd", fwd), ("adj", adj)):
        for f, (acted, rejected, old_ok) in table.items():
            print(f"FAULT {name} {f:22s} acted at {acted:2d} cases, rejected at {rejected:2d}; the old bar accepts it at square cases: {old_ok or 'none'}")
            assert acted > 0 and rejected == acted, (name, f)
    # a swapped pair of scales or pitches is invisible at the square shapes the earlier tests were confined to
    for c in (R.Case(3, 37, 37, 68, 68), R.Case(3, 16, 16, 68, 68)):
        x, g = R.fwd_input(c), R.adj_input(c)
        for f in ("swap_scales", "swap_pitch"):
            assert np.array_equal(R.emulate_forward(x, c.oh, c.ow, f), R.emulate_forward(x, c.oh, c.ow))
            assert np.array_equal(R.emulate_adjoint(g, c.ih, c.iw, f), R.emulate_adjoint(g, c.ih, c.iw))
