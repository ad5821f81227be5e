"""CPU: what tests/test_gpu_cod_metrics.py rests on.  The oracle's blocked nearest-foreground search equals the one-shot search it
replaces, and every input that the GPU tests build is well conditioned: no measure of the oracle sits on a branch or a threshold that
rounding could move, so a GPU comparison that fails means the kernel is wrong.  The oracle's cost per case is bounded here too."""
import time

import numpy as np
import pytest
import torch

from oracle import cod_metrics as OM
from test_gpu_cod_metrics import (CURVES, DISPATCH, FLAT_KINDS, FLAT_LEVELS, FLAT_SIZES, KEYS, ROUNDING, dispatch_case, flat_cases,
                                  reference)

MARGIN = 1e-6
ORACLE_SECONDS = 5.0


def nearest_foreground_one_shot(g):
    """oracle.cod_metrics.nearest_foreground as it was: all pixels against all candidates at once, [h, w, n_fg] in memory."""
    h, w = g.shape
    fr, fc = np.nonzero(g)
    order = np.lexsort((fr, fc))
    fr, fc = fr[order], fc[order]
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy[..., None] - fr) ** 2 + (xx[..., None] - fc) ** 2
    k = d2.argmin(axis=-1)
    return np.sqrt(d2.min(axis=-1).astype(np.float64)), fr[k], fc[k]


def masks():
    rng = np.random.default_rng(11)
    for i in range(16):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        g = rng.random((h, w)) < (0.02, 0.2, 0.5, 0.9)[i % 4]
        g[rng.integers(h), rng.integers(w)] = True
        yield f"random{i}_{h}x{w}", g
    stripes = np.zeros((30, 30), bool)
    stripes[::5] = True
    stripes[:, ::7] = True
    yield "stripes", stripes
    yield "columns", np.tile(np.arange(37) % 4 == 0, (23, 1))
    yield "checkerboard", np.indices((40, 40)).sum(0) % 2 == 0
    yield "coarse_checkerboard", (np.indices((40, 39)) // 3).sum(0) % 2 == 0
    yield "full", np.ones((7, 9), bool)
    yield "one_pixel", np.arange(40 * 40).reshape(40, 40) == 777


@pytest.mark.parametrize("block", [OM.NEAREST_BLOCK, 997, 1])
def test_blocked_nearest_foreground_equals_the_one_shot_search(block, monkeypatch):
    """Same candidates in the same (col, row) order, the same argmin: identical indices and bit-equal distances, whether the
    background pixels go in one block, in many, or one by one."""
    monkeypatch.setattr(OM, "NEAREST_BLOCK", block)
    for name, g in masks():
        dist, ir, ic = OM.nearest_foreground(g)
        dist0, ir0, ic0 = nearest_foreground_one_shot(g)
        assert dist.shape == dist0.shape == g.shape and dist.dtype == dist0.dtype == np.float64, name
        assert np.array_equal(ir, ir0) and np.array_equal(ic, ic0), name
        assert dist.tobytes() == dist0.tobytes(), name


def timed_reference(pred, gt):
    t0 = time.perf_counter()
    ref = reference(pred, gt)
    dt = time.perf_counter() - t0
    assert dt < ORACLE_SECONDS, dt
    return ref


def threshold_margin(p):
    """distance of the oracle's 2 * mean(p) from the nearest value that p takes"""
    return float(np.min(np.abs(np.unique(p) - 2 * p.mean())))


def quadrants(g):
    """the S-measure's four quadrants as oracle.cod_metrics.s_measure cuts them"""
    h, w = g.shape
    rows, cols = np.nonzero(g)
    cx, cy = int(np.round(cols.mean())) + 1, int(np.round(rows.mean())) + 1
    return cx, cy, ((slice(0, cy), slice(0, cx)), (slice(0, cy), slice(cx, w)), (slice(cy, h), slice(0, cx)), (slice(cy, h), slice(cx, w)))


def ssim_alpha(a, b):
    """`al` of the oracle's ssim"""
    m, xa, xb = a.size, a.mean(), b.mean()
    return 4 * xa * xb * ((a - xa) * (b - xb)).sum() / (m - 1)


@pytest.mark.parametrize("h,w", FLAT_SIZES)
def test_flat_region_inputs_are_well_conditioned(h, w):
    names = []
    for name, pred, gt in flat_cases(h, w):
        names.append(name)
        kind = name.rsplit("_", 1)[0]
        p, g = OM.prepare(pred.numpy(), gt.numpy())
        assert not (g[0].any() or g[-1].any() or g[:, 0].any() or g[:, -1].any()), name          # the rectangle touches no border
        assert p.min() == 0.0 and p.max() == 1.0, name
        region = {"flat_fg": [g], "flat_bg": [~g], "both": [g, ~g]}[kind]
        levels = [np.unique(p[r]) for r in region]
        assert all(lv.size == 1 for lv in levels), name                                          # flat where the name says so ...
        if kind == "both":
            assert np.unique(p).size == 2, name
        else:
            assert 0.05 < levels[0][0] < 0.95 and np.unique(p).size > 100, name                  # ... at a fractional level, random elsewhere
        assert threshold_margin(p) >= MARGIN, (name, threshold_margin(p))
        for q in quadrants(g)[2]:
            assert g[q].any() and (~g[q]).any(), (name, q)
            if kind == "both":
                assert abs(ssim_alpha(p[q], g[q].astype(np.float64))) > MARGIN, (name, q)
            else:
                assert np.unique(p[q]).size >= 2, (name, q)
        ref = timed_reference(pred, gt)
        assert all(np.all(np.isfinite(ref[k])) for k in KEYS + CURVES), name
        inverted = name == f"both_{FLAT_LEVELS[0]}"                                              # foreground at the lowest level, background at the highest
        assert ref["sm"] == 0.0 if inverted else ref["sm"] > 0.05, (name, ref["sm"])              # otherwise far from the max(0, .) that would hide a NaN
    assert sorted(names) == sorted(f"{kind}_{k}" for kind in FLAT_KINDS for k in FLAT_LEVELS)


@pytest.mark.parametrize("h,w,kind", DISPATCH)
def test_dispatch_inputs(h, w, kind):
    pred, gt = dispatch_case(h, w, kind)
    n_fg = int(gt.sum())
    assert n_fg == {"sparse": min(8, max(1, h * w // 2)), "empty": 0, "full": h * w}[kind]
    ref = timed_reference(pred, gt)
    if (h, w) == (1, 1):                                      # why the GPU test keeps 1x1: nothing the oracle returns for it is non-finite
        assert all(np.all(np.isfinite(ref[k])) for k in KEYS + CURVES)


@pytest.mark.parametrize("name", sorted(ROUNDING))
def test_rounding_inputs_are_well_conditioned(name):
    pred, gt = ROUNDING[name]()
    p, g = OM.prepare(pred.numpy(), gt.numpy())
    h, w = g.shape
    assert g.any() and not g.all()
    timed_reference(pred, gt)
    if name.startswith("clamp"):
        assert 2 * p.mean() >= 1 + MARGIN
        at_max = p >= 1.0
        assert np.count_nonzero(at_max) == 1 and bool(g[at_max][0]) == (name == "clamp_max_in_fg") and p.min() == 0.0
        return
    assert threshold_margin(p) >= MARGIN, threshold_margin(p)
    rows, cols = np.nonzero(g)
    cx, cy, quads = quadrants(g)
    if name.startswith("hist_edges"):
        k = np.rint(p * 255)
        assert np.array_equal(np.unique(k), np.arange(256)) and float(np.max(np.abs(p * 255 - k))) < 1e-4       # every pixel on a bin edge
        assert (pred.min().item() != 0.0) == ("shifted" in name) and gt.max().item() == 255.0
    elif name.startswith("centroid"):
        want = {"centroid_rows_3_4": (3.5, None), "centroid_rows_4_5": (4.5, None), "centroid_cols_3_4": (None, 3.5),
                "centroid_cols_4_5": (None, 4.5), "centroid_both_half": (3.5, 4.5)}[name]
        for mean, half in zip((rows.mean(), cols.mean()), want):              # exactly .5 where the name says so, a whole number elsewhere
            assert mean == (half if half is not None else int(mean)), (name, mean)
        assert (cy, cx) == tuple({3.5: 4, 4.5: 4}.get(v, int(v)) + 1 for v in (rows.mean(), cols.mean()))      # half-even: both go to 4
    elif name == "bottom_row":
        assert cy == h and 1 < cx < w
    elif name == "blank_quadrant":
        assert 0 < cy < h and 0 < cx < w and not g[quads[3]].any() and not p[quads[3]].any() and p.min() == 0.0
