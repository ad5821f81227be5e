"""COD measures (row N4): the HIP kernels behind the `statistics` mirror against the reference's own numbers (golden G16: the real
class on 18 seeded cases) and against the float64 oracle on larger and degenerate inputs: regions where the prediction is flat at a
fractional level (A), every chunk-dispatch case (B), the rounding rules (C) and the library's argument checks (D).

The input builders (flat_cases, dispatch_case, the ROUNDING table) touch no GPU: tests/test_cod_metrics_host.py imports them and checks
on the CPU that every input is well conditioned, so that a comparison failing here means the kernel is wrong."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("mae", "acc", "iou", "sm", "wfm", "adp_em", "adp_fm")
TOL = 1e-9                                                       # float64 on both sides; only the order of the sums differs


CURVES = ("em_curve", "fm_curve", "p_curve", "r_curve")


def raw(pred, gt):
    from ucod_dpl_amd import ops
    return ops.cod_metrics(torch.as_tensor(pred, dtype=torch.float32)[None].to(DEV), torch.as_tensor(gt, dtype=torch.float32)[None].to(DEV))[0]


def as_dict(r):
    r = r.cpu().numpy()
    d = {k: r[i] for i, k in enumerate(KEYS)}
    d.update(em_curve=r[8:264], fm_curve=r[264:520], p_curve=r[520:776], r_curve=r[776:1032])
    return d


def record(pred, gt):
    return as_dict(raw(pred, gt))


_nearest = {}


def reference(pred, gt):
    """oracle.cod_metrics.image_measures.  Its cost is nearest_foreground, which depends on the mask alone: the result for the last
    mask is kept, so that the cases that share a mask (part A: 15 per size) pay for it once."""
    from oracle import cod_metrics as OM
    plain = OM.nearest_foreground

    def shared(g):
        key = (g.shape, g.tobytes())
        if _nearest.get("key") != key:
            _nearest.update(key=key, value=plain(g))
        return _nearest["value"]

    OM.nearest_foreground = shared
    try:
        with np.errstate(all="ignore"):
            return OM.image_measures(np.asarray(pred, np.float32), np.asarray(gt, np.float32))
    finally:
        OM.nearest_foreground = plain


def mismatches(got, ref):
    """[(measure, what)] where a record differs from the oracle: every measure and all four curves, non-finite values in the same
    places with the same values, everything else within TOL."""
    bad = []
    for k in KEYS + CURVES:
        a, b = np.atleast_1d(np.asarray(got[k], np.float64)), np.atleast_1d(np.asarray(ref[k], np.float64))
        fa, fb = np.isfinite(a), np.isfinite(b)
        if not (np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb], equal_nan=True)):
            bad.append((k, "non-finite pattern", a[~(fa & fb)][:4].tolist(), b[~(fa & fb)][:4].tolist()))
        elif fa.any() and not float(np.max(np.abs(a[fa] - b[fb]))) < TOL:
            i = int(np.argmax(np.abs(np.where(fa, a - b, 0.0))))
            bad.append((k, float(np.max(np.abs(a[fa] - b[fb]))), float(a[i]), float(b[i])))
    return bad


# ---- A: regions where the prediction is flat at a fractional level ------------------------------------------------------------
FLAT_SIZES = ((48, 56), (97, 131), (181, 240))                   # 1, 2 and 6 chunks
FLAT_LEVELS = (26, 77, 128, 179, 230)
FLAT_KINDS = ("flat_fg", "flat_bg", "both")
LEVELS = torch.arange(256).float() / 255                         # k / 255 as f32


def flat_rect(h, w):
    """The ground-truth rectangle: strictly inside the image and off its centre, a quarter of each side."""
    return slice(h // 3, h // 3 + h // 4), slice(w // 4, w // 4 + w // 4)


def flat_cases(h, w):
    """(name, pred, gt): a uint8-quantised random prediction holding 0 and 1, then the ground-truth rectangle (flat_fg), everything
    outside it (flat_bg) or each of the two at its own level (both: a two-level prediction) painted flat.  The two forced pixels
    lie in the part that stays random."""
    ys, xs = flat_rect(h, w)
    gt = torch.zeros(h, w)
    gt[ys, xs] = 1
    fg = gt > 0
    for j, k in enumerate(FLAT_LEVELS):
        for c, kind in enumerate(FLAT_KINDS):
            g = torch.Generator().manual_seed(h * w + 3 * k + c)
            pred = torch.randint(0, 256, (h, w), generator=g).float() / 255
            lo, hi = ((ys.start, xs.start), (ys.stop - 1, xs.stop - 1)) if kind == "flat_bg" else ((0, 0), (h - 1, w - 1))
            pred[lo], pred[hi] = 0.0, 1.0
            if kind != "flat_bg":
                pred[fg] = LEVELS[k]
            if kind != "flat_fg":
                pred[~fg] = LEVELS[k] if kind == "flat_bg" else LEVELS[FLAT_LEVELS[j - 1]]      # both: the next lower level; for the lowest, the highest (an inverted map: S-measure 0)
            yield f"{kind}_{k}", pred, gt


# ---- B: chunk dispatch ----------------------------------------------------------------------------------------------------------
DISPATCH = [(725, 727, "sparse"),                                # n = 527075 > 524288: 64 chunks at the cap, 8236 pixels each
            (725, 727, "empty"), (725, 727, "full"),             # every n_fg == 0 / n_fg == n branch with 64 chunks
            (8193, 1, "sparse"), (1, 8193, "sparse"),            # 2 chunks of 4097 (the tail chunk one short); one column / one row: the 7x7 window is mostly padding
            (3, 5, "sparse"), (6, 6, "sparse"), (1, 2, "sparse"),  # fewer pixels than threads, smaller than the window
            (128, 64, "sparse"),                                 # n = 8192: the last size with one chunk
            (1, 1, "sparse")]                                    # kept: the oracle's values are all finite there (E-measure 1 / eps included)


def dispatch_case(h, w, kind):
    """(pred, gt): a soft random prediction; ground truth of 8 seeded pixels (at most half the image), none, or all."""
    g = torch.Generator().manual_seed(h * 10007 + w)
    pred = torch.rand(h, w, generator=g)
    gt = torch.zeros(h, w)
    if kind == "sparse":
        gt.view(-1)[torch.randperm(h * w, generator=g)[:min(8, max(1, h * w // 2))]] = 1
    elif kind == "full":
        gt[:] = 1
    return pred, gt


# ---- C: rounding rules ----------------------------------------------------------------------------------------------------------
def hist_edge_case(h, w, shifted):
    """Every pixel on a histogram bin edge: the prediction takes all 256 levels k / 255 (f32), the lower levels more often so that
    the adaptive threshold lies far from 1; shifted: 3 p - 1, so that the normalisation subtracts and divides.  Ground truth: a blob
    in 0 / 255 scale."""
    n = h * w
    g = torch.Generator().manual_seed(n + int(shifted))
    k = torch.arange(n) % 256
    k[n // 2:] //= 3                                             # (// 2 would put 2 * mean(p) at 191 / 255 exactly when 256 divides n / 2)
    pred = LEVELS[k[torch.randperm(n, generator=g)]].view(h, w)
    if shifted:
        pred = 3 * pred - 1
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    gt = 255.0 * ((((yy - 0.45 * h) / (0.3 * h)) ** 2 + ((xx - 0.55 * w) / (0.25 * w)) ** 2) < 1).float()
    return pred, gt


def boxed_case(h, w, ys, xs, seed):
    pred = torch.rand(h, w, generator=torch.Generator().manual_seed(seed))
    gt = torch.zeros(h, w)
    gt[ys, xs] = 1
    return pred, gt


def clamp_case(max_in_fg):
    """2 * mean(p) > 1: the adaptive threshold is clamped to 1 and only the single maximum pixel, inside or outside the ground
    truth, passes it."""
    pred, gt = boxed_case(40, 50, slice(10, 30), slice(15, 40), 77)
    pred = 1 - 0.2 * pred
    pred[7, 9] = 0.0
    pred[(20, 20) if max_in_fg else (2, 3)] = 1.0
    return pred, gt


def blank_quadrant_case():
    """An L-shaped ground truth whose right-bottom S-measure quadrant holds no foreground, under a prediction that is exactly 0
    there: the quadrant's similarity is the reference's 1.0 only if its variance comes out exactly 0."""
    pred, gt = boxed_case(40, 48, slice(5, 30), slice(5, 10), 78)
    gt[5:10, 5:30] = 1
    pred[12:, 12:] = 0.0
    return pred, gt


ROUNDING = {
    "hist_edges_64x64": lambda: hist_edge_case(64, 64, False), "hist_edges_97x131": lambda: hist_edge_case(97, 131, False),
    "hist_edges_shifted_64x64": lambda: hist_edge_case(64, 64, True), "hist_edges_shifted_97x131": lambda: hist_edge_case(97, 131, True),
    # centroid: np.round is half-even; mean row 3.5 -> 4, 4.5 -> 4, the same for columns, and both at once
    "centroid_rows_3_4": lambda: boxed_case(20, 24, slice(3, 5), slice(5, 10), 1), "centroid_rows_4_5": lambda: boxed_case(20, 24, slice(4, 6), slice(5, 10), 2),
    "centroid_cols_3_4": lambda: boxed_case(20, 24, slice(5, 10), slice(3, 5), 3), "centroid_cols_4_5": lambda: boxed_case(20, 24, slice(5, 10), slice(4, 6), 4),
    "centroid_both_half": lambda: boxed_case(20, 24, slice(3, 5), slice(4, 6), 5),
    "bottom_row": lambda: boxed_case(33, 40, slice(32, 33), slice(5, 25), 6),          # cy == H: the two lower quadrants are empty
    "clamp_max_in_fg": lambda: clamp_case(True), "clamp_max_in_bg": lambda: clamp_case(False),
    "blank_quadrant": blank_quadrant_case,
}


def test_every_measure_matches_the_reference_class():
    g = load_golden("g16_cod_metrics")
    for i in range(int(g["n"])):
        got = record(g[f"pred{i}"], g[f"gt{i}"])
        for k in KEYS + ("em_curve", "fm_curve", "p_curve", "r_curve"):
            d = float(np.max(np.abs(np.asarray(got[k]) - g[f"{k}{i}"].numpy())))
            assert d < TOL, (i, k, d)


def test_statistics_mirror_reproduces_get_result():
    from ucod_dpl_amd.engine.utils.metrics import statistics
    g = load_golden("g16_cod_metrics")
    st = statistics()
    for i in range(int(g["n"])):
        st.step(g[f"gt{i}"][None, None].to(DEV), g[f"pred{i}"][None, None].to(DEV))
    res = st.get_result()
    assert sorted(res) == sorted(k[6:] for k in g if k.startswith("final."))
    for k, v in res.items():
        assert abs(v - float(g["final." + k])) < TOL, (k, v, float(g["final." + k]))
    st.reset()
    assert st._records == []
    with pytest.raises(RuntimeError):
        st.step(g["gt0"][None, None], g["pred0"][None, None])       # host tensors: no CPU path


@pytest.mark.parametrize("h,w,kind", [(97, 131, "soft"), (240, 180, "binary"), (64, 64, "sparse"), (50, 75, "one_pixel"), (33, 40, "column"),
                                      (30, 30, "stripes")])
def test_against_the_float64_oracle(h, w, kind):
    """Sizes and shapes the golden set does not hold: a larger soft map, a binary mask, a few scattered foreground pixels (long
    nearest-pixel walks with many ties), a single foreground pixel (sample std of one element: the S-measure collapses to 0 as in the
    reference), foreground only in the last column (an empty S-measure quadrant), and regular stripes (every distance tied)."""
    from oracle import cod_metrics as OM
    g = torch.Generator().manual_seed(h * w)
    pred = torch.rand(h, w, generator=g)
    if kind == "soft":
        gt = (torch.rand(h, w, generator=g) > 0.6).float()
        gt[10:60, 20:90] = 1
    elif kind == "binary":
        gt = torch.zeros(h, w); gt[40:200, 30:150] = 1
        pred = (gt + (torch.rand(h, w, generator=g) > 0.9).float()).clamp(0, 1)
    elif kind == "sparse":
        gt = (torch.rand(h, w, generator=g) > 0.995).float()
        gt[5, 7] = 1
    elif kind == "one_pixel":
        gt = torch.zeros(h, w); gt[20, 30] = 1
    elif kind == "column":
        gt = torch.zeros(h, w); gt[5:25, w - 1] = 1
    else:
        gt = torch.zeros(h, w); gt[::5] = 1; gt[:, ::7] = 1
    ref = OM.image_measures(pred.numpy(), gt.numpy())
    got = record(pred, gt)
    for k in KEYS + ("em_curve", "fm_curve", "p_curve", "r_curve"):
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (kind, k)
        d = float(np.nanmax(np.abs(a - b))) if a.size else 0.0
        assert d < TOL, (kind, k, d)


def test_batch_equals_one_by_one_and_is_repeatable():
    from ucod_dpl_amd import ops
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(6, 48, 56, generator=g).to(DEV)
    gt = (torch.rand(6, 48, 56, generator=g) > 0.7).float().to(DEV)
    gt[3] = 0
    both = ops.cod_metrics(pred, gt)
    assert torch.equal(both, ops.cod_metrics(pred, gt))
    for i in range(6):
        assert torch.equal(both[i], ops.cod_metrics(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous())[0])
    assert float(both[3, 4]) == 0.0                                   # empty ground truth: weighted F is defined as 0


@pytest.mark.parametrize("h,w", FLAT_SIZES)
def test_flat_regions_at_a_fractional_level(h, w):
    """A: over a region where the prediction is constant the sample variance is 0; formed from one-pass sums it is rounding noise
    of either sign, and the S-measure then comes out as NaN -> 0, or off by the square root of the noise.  With the one-pass
    moments this kernel had first, 13 of the 15 flat_bg cases failed (10 with S-measure 0 against the oracle's 0.06 to 0.73, 3 off
    by about 2e-9) and flat_fg was off by up to 1.6e-10; about the region's mean (pass 3) every case agrees to the last bits."""
    bad = []
    for name, pred, gt in flat_cases(h, w):
        got, ref = record(pred, gt), reference(pred, gt)
        print(f"{h}x{w} {name}: sm {got['sm']!r} oracle {ref['sm']!r}")
        if not np.isfinite(got["sm"]):
            bad.append((name, "sm", float(got["sm"])))
        bad += [(name,) + m for m in mismatches(got, ref)]
    assert not bad, bad


@pytest.mark.parametrize("h,w,kind", DISPATCH)
def test_every_chunk_dispatch_case(h, w, kind):
    """B: 1, 2 and 64 chunks, the chunk cap, the tail chunk, images smaller than a workgroup and than the Gaussian window; the same
    record from two calls.  1x1 is kept: the oracle's values for it are all finite (tests/test_cod_metrics_host.py), the E-measure's
    1 / eps included.  A 725x727 call, its nearest-pixel walk of up to 725 rows per pixel included, takes about 2 ms."""
    pred, gt = dispatch_case(h, w, kind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = raw(pred, gt).cpu()
    t1 = time.perf_counter()
    again = raw(pred, gt).cpu()
    print(f"{h}x{w} {kind}: first call {1e3 * (t1 - t0):.2f} ms, second {1e3 * (time.perf_counter() - t1):.2f} ms (upload, eleven launches, download)")
    assert torch.equal(first, again)                                 # (a record holds no NaN: the S-measure's ends as 0)
    bad = mismatches(as_dict(first), reference(pred, gt))
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(ROUNDING))
def test_rounding_rules(name):
    """C: uint8(p * 255) with every pixel on a bin edge, half-even centroids, the centroid on the bottom row, the clamped adaptive
    threshold, an exactly blank quadrant."""
    pred, gt = ROUNDING[name]()
    bad = mismatches(record(pred, gt), reference(pred, gt))
    assert not bad, bad


def test_argument_checks():
    """D: what the library refuses, it refuses before it launches or writes anything."""
    from ucod_dpl_amd import native, ops
    lib = native.load()
    EINVAL, ENOMEM = -1, -2
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(9)
    pred = torch.rand(B, H, W, generator=g).to(DEV)
    gt = (torch.rand(B, H, W, generator=g) > 0.5).float().to(DEV)
    need = lib.ucod_cod_metrics_workspace_bytes(B, H, W)
    assert need > 0
    for shape in ((0, H, W), (B, 0, W), (B, H, 0), (-1, H, W), (B, -1, W), (B, H, -1)):
        assert lib.ucod_cod_metrics_workspace_bytes(*shape) == 0, shape
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((B, native.COD_RECORD), -7.0, dtype=torch.float64, device=DEV)
    P, G, O, S = pred.data_ptr(), gt.data_ptr(), out.data_ptr(), ws.data_ptr()

    def call(p, g_, b, h, w, o, s, nbytes):
        return lib.ucod_cod_metrics(p, g_, b, h, w, o, s, ctypes.c_size_t(nbytes), native.stream())

    for args in ((None, G, B, H, W, O, S, need), (P, None, B, H, W, O, S, need), (P, G, B, H, W, None, S, need), (P, G, B, H, W, O, None, need),
                 (P, G, 0, H, W, O, S, need), (P, G, B, 0, W, O, S, need), (P, G, B, H, 0, O, S, need),
                 (P, G, -1, H, W, O, S, need), (P, G, B, -1, W, O, S, need), (P, G, B, H, -1, O, S, need),
                 (P, G, 1, 32769, 32768, O, S, need)):                                      # H * W = 2^30 + 2^15
        assert call(*args) == EINVAL, args
    assert call(P, G, B, H, W, O, S, need - 1) == ENOMEM
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(P, G, B, H, W, O, S, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.cod_metrics(pred, gt))
    with pytest.raises(ValueError):
        ops.cod_metrics(pred, gt[:, :, :-1].contiguous())
    with pytest.raises(ValueError):
        ops.cod_metrics(pred, gt[:1])
