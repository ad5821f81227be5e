"""Reference, error bounds, dispatch restatement and case lists for ucod_bilinear_resize, ucod_bilinear_resize_adjoint and ucod_binarize
(csrc/elementwise.hip).  CPU only (numpy); test_resize_ref_host.py shows that the lists reach every dispatch class and that the checker sees the
faults the cases are there for, test_gpu_resize.py runs the kernels against it through the C ABI.

Weight model (one per axis, used for both directions; it restates src_index() with its f32 roundings):
    scale = f32(in) / f32(out);  s = f32(scale * (o + 0.5) - 0.5) with ONE rounding (the kernel's fmaf; evaluated in f64, where the product of a 24-bit
    scale and a 13-bit o + 0.5 is exact for sizes below 4096);  s = max(s, 0);  i0 = min(int(s), in - 1);  i1 = i0 + (i0 < in - 1);
    l1 = f32(s - i0);  w0 = f32(1 - l1);  W[o, i0] += w0;  W[o, i1] += l1   (f64; both taps land on in - 1 at the far edge, hence +=).
With u = 2^-24:
    forward  Wy X Wx^T,   |error| <= 4.5 u (|Wy| |X| |Wx|^T)   -- the longest path through lerp2 passes four f32 roundings: rn(v11 lx), the fma giving `bot`,
             rn(bot ly) and the final fma; the half absorbs the second-order terms;
    adjoint  Wy^T G Wx,   |error| <= (ny + nx + 2) u (|Wy|^T |G| |Wx|)   -- ny, nx: the largest numbers of nonzeros in a column of Wy, Wx; the kernels sum nx
             then ny sequential fmas, and a source index that both taps of an output reach has its weight summed in f32 (one more rounding per axis).
The bounds are derived, not measured; profiles/resize_tests.txt records what the hardware measured against them.
"""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
F32 = np.float32
FWD_ROUNDINGS = 4.5

# (planes, ih, iw, oh, ow); off: the input starts `off` floats past a 16-byte boundary (a view into a larger buffer)
Case = namedtuple("Case", "planes ih iw oh ow off", defaults=(0,))


def case_id(c):
    return "-".join(str(v) for v in c[:5]) + (f"+{c.off}" if c.off else "")


# ================================================================================================ the weight model
Taps = namedtuple("Taps", "i0 i1 w0 l1")


def axis_scale(n_in, n_out):
    return F32(n_in) / F32(n_out)


def src_index(o, scale, n_in, clamp_neg=True, clamp_i1=True):
    """src_index() of elementwise.hip for an array of output indices; -> Taps (f32 weights).  The two flags drop a clamp (the faults of the host test)."""
    s = (np.float64(scale) * (np.asarray(o, dtype=np.float64) + 0.5) - 0.5).astype(F32)
    if clamp_neg:
        s = np.maximum(s, F32(0))
    i0 = np.minimum(np.trunc(s).astype(np.int64), n_in - 1)
    i1 = i0 + ((i0 < n_in - 1) if clamp_i1 else 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    return Taps(i0, i1, (F32(1) - l1).astype(F32), l1)


@functools.lru_cache(maxsize=None)
def axis_taps(n_in, n_out):
    assert 0 < n_in < 4096 and 0 < n_out < 4096
    return src_index(np.arange(n_out), axis_scale(n_in, n_out), n_in)


@functools.lru_cache(maxsize=None)
def axis_matrix(n_in, n_out):
    """dense W[out, in] in f64"""
    t = axis_taps(n_in, n_out)
    W = np.zeros((n_out, n_in), dtype=np.float64)
    o = np.arange(n_out)
    np.add.at(W, (o, t.i0), t.w0.astype(np.float64))
    np.add.at(W, (o, t.i1), t.l1.astype(np.float64))
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def max_taps(n_in, n_out):
    """the largest number of outputs that reach one source index with a nonzero weight: what adjoint_taps has to hold"""
    return int((axis_matrix(n_in, n_out) != 0).sum(0).max())


def forward_ref(x, oh, ow):
    """x [planes, ih, iw] -> (reference f64 [planes, oh, ow], bound f64)"""
    x = np.asarray(x, dtype=np.float64)
    Wy, Wx = axis_matrix(x.shape[1], oh), axis_matrix(x.shape[2], ow)
    ref = Wy @ x @ Wx.T
    mag = np.abs(Wy) @ np.abs(x) @ np.abs(Wx).T
    return ref, FWD_ROUNDINGS * U * mag


def adjoint_ref(g, ih, iw):
    """g [planes, oh, ow] -> (reference f64 [planes, ih, iw], bound f64)"""
    g = np.asarray(g, dtype=np.float64)
    oh, ow = g.shape[1:]
    Wy, Wx = axis_matrix(ih, oh), axis_matrix(iw, ow)
    ref = Wy.T @ g @ Wx
    mag = np.abs(Wy).T @ np.abs(g) @ np.abs(Wx)
    return ref, (max_taps(ih, oh) + max_taps(iw, ow) + 2) * U * mag


def ratio(got, ref, bound):
    """the largest |got - ref| / bound; inf where an element is not finite, or is off where the bound is zero.  A result passes when this is below 1."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    zero = bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


# ================================================================================================ dispatch restatement
def cdiv(a, b):
    return -(-a // b)


def fwd_class(planes, ih, iw, oh, ow, off=0):
    """ucod_bilinear_resize's choice and the branches the chosen kernel takes.  `why` (element kernel): the one condition of the LDS form that fails, or
    "several"."""
    why = []
    if planes < 64:
        why.append("planes")
    if ow % 4 or ow < 4:
        why.append("ow4")
    if ow > 1024:
        why.append("ow1024")
    if 4 * ih * iw * 4 > 48 * 1024:
        why.append("src")
    if oh * ow < ih * iw:
        why.append("shrinks")
    if why:
        return {"kernel": "elem", "why": why[0] if len(why) == 1 else "several", "grid_stride": cdiv(planes * oh * ow, 256) > 16384}
    G = ow // 4
    S = 256 // G
    last = planes % 4 or 4
    aligned = off % 4 == 0                                                  # workgroup b's source starts 4 b planes on: as aligned as the base
    return {"kernel": "lds", "G": "min" if G == 1 else "max" if G == 256 else "mid", "S": "one" if S == 1 else "all" if S == 256 else "some",
            "idle_threads": 256 % G != 0, "ragged": planes % 4 != 0, "staging": "vector" if aligned else "scalar",
            "tail": aligned and (last * ih * iw) % 4 != 0, "trips": "many" if cdiv(4 * oh, S) > 1 else "one", "axis_shrinks": oh < ih or ow < iw}


def adjoint_tap_estimate(ih, iw, oh, ow):
    """what ucod_bilinear_resize_adjoint sizes its tap arrays by: per axis ceil(2 / scale) + 1 in f32, and never more than the axis has outputs"""
    def one(n_in, n_out):
        return min(int(np.ceil(F32(2) / axis_scale(n_in, n_out)) + F32(1)), n_out)
    return max(one(ih, oh), one(iw, ow))


ADJ_LDS_FLOATS = 15360


def adj_class(planes, ih, iw, oh, ow, off=0):
    taps = adjoint_tap_estimate(ih, iw, oh, ow)
    if taps > 16:
        return {"kernel": "refused", "taps": taps}
    maxt = 16 if taps > 8 else 8
    edge = "at8" if taps == 8 else "at16" if taps == 16 else "in"
    n_in = oh * ow
    lds = ((n_in + 3) & ~3) + oh * iw + ih * (2 * maxt + 1)
    why = []
    if lds > ADJ_LDS_FLOATS:
        why.append("lds")
    if planes < 64:
        why.append("planes")
    if iw > 128:
        why.append("iw")
    if why:
        return {"kernel": "elem", "maxt": maxt, "taps_edge": edge, "why": why[0] if len(why) == 1 else "several", "plane_stride": planes > 1024,
                "blocks": "many" if ih * iw > 256 else "one"}
    ppw = 4 if planes >= 2048 else 2 if planes >= 512 else 1
    if n_in <= 5120 and n_in % 4 == 0 and off % 4 == 0:
        staging = frozenset(["piped"])
    else:
        staging = frozenset("vector" if (off + p * n_in) % 4 == 0 else "scalar" for p in range(min(planes, 4)))
    S = 256 // iw
    return {"kernel": "sep", "maxt": maxt, "taps_edge": edge, "ppw": ppw, "ragged": planes % ppw != 0, "staging": staging,
            "tail": "vector" in staging and n_in % 4 != 0, "table_loop": ih > 256, "idle_threads": 256 % iw != 0, "iw_max": iw == 128,
            "trips": "many" if cdiv(oh, S) > 1 else "one"}


def adjoint_window(i, n_in, n_out):
    """the candidate range [lo, hi] adjoint_taps scans for source index i, with its f32 roundings"""
    scale = axis_scale(n_in, n_out)
    lo = int(np.floor(F32(F32(F32(i) - F32(0.5)) / scale) - F32(0.5))) - 1
    hi = int(np.ceil(F32(F32(F32(i) + F32(1.5)) / scale) - F32(0.5))) + 1
    return max(lo, 0), min(hi, n_out - 1)


# ================================================================================================ case lists
FWD_ELEM_CASES = [Case(*c) for c in (
    (3, 20, 10, 10, 40), (70, 9, 13, 21, 30), (64, 60, 60, 120, 120), (64, 24, 40, 12, 20), (64, 3, 300, 3, 1028), (64, 48, 65, 48, 65),
    (1, 68, 68, 427, 640), (1, 518, 518, 427, 640), (8, 68, 68, 600, 900), (5, 1, 7, 5, 1), (5, 7, 1, 1, 9), (2, 1, 1, 3, 3), (6, 7, 5, 7, 5))]
FWD_LDS_CASES = [Case(*c) for c in (
    (64, 37, 37, 68, 68), (67, 37, 37, 68, 68), (65, 5, 7, 12, 4), (64, 2, 3, 2, 1024), (66, 20, 10, 10, 40), (64, 48, 64, 48, 64),
    (64, 37, 37, 68, 68, 37 * 37))]
FWD_CASES = FWD_ELEM_CASES + FWD_LDS_CASES

ADJ_ELEM_CASES = [Case(*c) for c in (
    (3, 37, 37, 68, 68), (5, 10, 16, 68, 68), (3, 20, 10, 10, 40), (3, 4, 8, 14, 28), (3, 4, 4, 15, 15), (3, 4, 4, 30, 30), (1100, 2, 130, 2, 260),
    (64, 2, 129, 2, 258), (64, 68, 68, 136, 136), (64, 50, 50, 100, 100), (5, 1, 7, 5, 1), (5, 7, 1, 1, 9), (6, 7, 5, 7, 5))]
ADJ_SEP_CASES = [Case(*c) for c in (
    (64, 37, 37, 68, 68), (513, 12, 12, 20, 20), (2050, 6, 6, 12, 12), (64, 37, 37, 67, 67), (64, 40, 40, 80, 80), (64, 48, 48, 96, 96),
    (64, 16, 16, 68, 68), (64, 10, 16, 68, 68), (64, 300, 4, 300, 8), (64, 2, 128, 2, 256), (64, 68, 68, 37, 37), (64, 12, 12, 20, 20, 1))]
ADJ_CASES = ADJ_ELEM_CASES + ADJ_SEP_CASES
ADJ_REFUSED = [Case(3, 4, 4, 31, 31), Case(3, 4, 40, 31, 20)]

IDENTITY_CASES = [c for c in FWD_CASES + ADJ_CASES if (c.ih, c.iw) == (c.oh, c.ow)]

# in / out is 1 or a power of two on each axis: with integer inputs every weight, product and sum is exact in f32
DYADIC_CASES = [Case(2, 68, 68, 34, 34), Case(2, 16, 16, 64, 64), Case(64, 12, 20, 24, 80), Case(64, 34, 20, 17, 80)]
DYADIC_KINDS = ("int8", "mask")

THRESHOLD_CASES = [Case(1, 518, 518, 427, 640), Case(1, 518, 518, 1024, 683), Case(1, 68, 68, 427, 640), Case(8, 16, 16, 68, 68)]
THRESHOLD_MARGIN = 2.0 ** -20
THRESHOLD_SHARE = 0.97
MASK_DENSITY = 0.4
COMPOSITION_CASE = Case(1, 68, 68, 427, 640)

BINARIZE_LONG = 4096 * 256 + 77                                        # binarize_kernel: at most 4096 workgroups of 256, so 77 elements of a second trip


# The compared share of the thresholds test counts the outputs that are not exact ties at 0.5.  At 16 -> 68 an i.i.d. mask of density 0.4 leaves
# 0.970 +- 0.003 of them over seeds, right at the 0.97 that test asks for: the masks are drawn from a stream where it is 0.974 (the host test asserts it).
MASK_STREAM = 4


def _seed(c, salt, kind):
    return [MASK_STREAM if kind == "mask" else 0, salt] + [int(v) for v in c]


@functools.lru_cache(maxsize=None)
def fwd_input(c, kind="randn"):
    """the source planes of case c, f32 [planes, ih, iw] (read-only; shared by the tests)"""
    return _make(np.random.default_rng(_seed(c, 1, kind)), (c.planes, c.ih, c.iw), kind)


@functools.lru_cache(maxsize=None)
def adj_input(c, kind="randn"):
    """the output-side gradient of case c, f32 [planes, oh, ow]"""
    return _make(np.random.default_rng(_seed(c, 2, kind)), (c.planes, c.oh, c.ow), kind)


def _make(rng, shape, kind):
    if kind == "randn":
        a = rng.standard_normal(shape, dtype=np.float32) + F32(0.5)
    elif kind == "int8":
        a = rng.integers(-8, 9, size=shape).astype(np.float32)
    elif kind == "mask":
        a = (rng.random(shape) < MASK_DENSITY).astype(np.float32)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=64)
def fwd_expected(c, kind="randn"):
    ref, bound = forward_ref(fwd_input(c, kind), c.oh, c.ow)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


@functools.lru_cache(maxsize=64)
def adj_expected(c, kind="randn"):
    ref, bound = adjoint_ref(adj_input(c, kind), c.ih, c.iw)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def threshold_compare(got, model, level, margin=THRESHOLD_MARGIN):
    """(got > level) against (model > level) where |model - level| > margin; -> (mismatches, compared share)"""
    far = np.abs(model - level) > margin
    return int(((np.asarray(got) > level) != (model > level))[far].sum()), float(far.mean())


def binarize_ref(x, logits):
    """None where the test asserts nothing: 0 < x < 2^-20 with logits (there the rounding of 1 / (1 + expf(-x)) decides)"""
    x = np.asarray(x, dtype=np.float32)
    if not logits:
        return (x > F32(0.5)).astype(np.float32), np.ones(x.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        decided = ~((x > 0) & (x < F32(THRESHOLD_MARGIN)))
        return (x >= F32(THRESHOLD_MARGIN)).astype(np.float32), decided


def binarize_specials():
    half = F32(0.5)
    return np.array([0.5, np.nextafter(half, F32(1)), np.nextafter(half, F32(-1)), 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.25, 0.75,
                     THRESHOLD_MARGIN, np.nextafter(F32(THRESHOLD_MARGIN), F32(1)), -THRESHOLD_MARGIN, -1e-30, 1e-30, 88.0, -88.0, 104.0, -104.0, 3e38, -3e38],
                    dtype=np.float32)


# ================================================================================================ f32 emulation of the kernels, with faults to inject
def _fma(a, b, c):
    """f32 fma through f64: the product is exact, the sum is rounded to 53 bits and then to 24 (a double rounding moves the result by at most one f32
    ulp, and only on a near-tie of the 53-bit sum)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


FWD_FAULTS = ("swap_scales", "swap_pitch", "i1_unclamped", "no_negative_clamp", "ragged_plane_skipped", "stale_tail")
ADJ_FAULTS = ("swap_scales", "swap_pitch", "i1_unclamped", "no_negative_clamp", "tap_dropped", "ragged_plane_skipped", "stale_tail")
STALE = F32(-3.25)                                                       # what a staging slot holds that no load reached


def _fault_taps(n_in, n_out, other, fault):
    scale = axis_scale(*other) if fault == "swap_scales" else axis_scale(n_in, n_out)
    return src_index(np.arange(n_out), scale, n_in, clamp_neg=fault != "no_negative_clamp", clamp_i1=fault != "i1_unclamped")


WEIGHT_FAULTS = ("swap_scales", "i1_unclamped", "no_negative_clamp")


def fault_moves_a_weight(c, fault):
    """whether a fault of WEIGHT_FAULTS changes any weight of either axis by more than 2^-20 (far above rounding, far below what such a fault does when it
    acts): e.g. a dropped negative clamp on a 1-wide axis puts 1 - l1 and l1 on the same element and changes nothing"""
    for n_in, n_out, other in ((c.ih, c.oh, (c.iw, c.ow)), (c.iw, c.ow, (c.ih, c.oh))):
        t = _fault_taps(n_in, n_out, other, fault)
        W = np.zeros((n_out, n_in + 1))                                      # one more column: what an unclamped i1 reads past the edge
        o = np.arange(n_out)
        np.add.at(W, (o, np.clip(t.i0, 0, n_in)), t.w0.astype(np.float64))
        np.add.at(W, (o, np.clip(t.i1, 0, n_in)), t.l1.astype(np.float64))
        W[:, :n_in] -= axis_matrix(n_in, n_out)
        if np.abs(W).max() > 2.0 ** -20:
            return True
    return False


def emulate_forward(x, oh, ow, fault=None, cls=None):
    """lerp2 in its own order, f32, on the flat buffer (so that a wrong index reads what the kernel would read, clipped to the buffer).  Returns None where
    the fault has nothing to act on (no ragged workgroup, no staging tail)."""
    P, ih, iw = x.shape
    ty, tx = _fault_taps(ih, oh, (iw, ow), fault), _fault_taps(iw, ow, (ih, oh), fault)
    flat = np.array(x, dtype=np.float32).reshape(-1)
    if fault == "stale_tail":
        if not (cls and cls["kernel"] == "lds" and cls["tail"]):
            return None
        n = (P % 4) * ih * iw
        flat[flat.size - n % 4:] = STALE
    pitch = ih if fault == "swap_pitch" else iw
    base = (np.arange(P) * ih * iw)[:, None, None]

    def at(yi, xi):
        return flat[np.clip(base + yi[None, :, None] * pitch + xi[None, None, :], 0, flat.size - 1)]
    lx, ly = tx.l1[None, None, :], ty.l1[None, :, None]
    wx, wy = tx.w0[None, None, :], ty.w0[None, :, None]
    top = _fma(at(ty.i0, tx.i0), wx, (at(ty.i0, tx.i1) * lx).astype(F32))
    bot = _fma(at(ty.i1, tx.i0), wx, (at(ty.i1, tx.i1) * lx).astype(F32))
    out = _fma(top, wy, (bot * ly).astype(F32))
    if fault == "ragged_plane_skipped":
        if not (cls and cls["kernel"] == "lds" and cls["ragged"]):
            return None
        out[-1] = np.nan
    return out


def _tap_table(n_in, n_out, taps):
    """per source index the outputs that reach it, in increasing order, with the f32 weight adjoint_taps forms (both taps of an output on one index: an f32
    sum).  -> (idx [in, T], w [in, T]) padded with weight 0"""
    rows = [[] for _ in range(n_in)]
    for o in range(n_out):
        i0, i1 = int(taps.i0[o]), int(taps.i1[o])
        w0, l1 = taps.w0[o], taps.l1[o]
        if i0 == i1:
            contrib = [(i0, F32(w0 + l1))]
        else:
            contrib = [(i0, w0), (i1, l1)]
        for i, w in contrib:
            if 0 <= i < n_in and w != 0:
                rows[i].append((o, w))
    T = max(1, max(len(r) for r in rows))
    idx = np.zeros((n_in, T), dtype=np.int64)
    w = np.zeros((n_in, T), dtype=np.float32)
    for i, r in enumerate(rows):
        for k, (o, wt) in enumerate(r):
            idx[i, k], w[i, k] = o, wt
    return idx, w


def emulate_adjoint(g, ih, iw, fault=None, cls=None):
    """x taps inside, y taps outside, sequential fmas in increasing output order, f32"""
    P, oh, ow = g.shape
    yi, yw = _tap_table(ih, oh, _fault_taps(ih, oh, (iw, ow), fault))
    xi, xw = _tap_table(iw, ow, _fault_taps(iw, ow, (ih, oh), fault))
    if fault == "tap_dropped":                                               # the heaviest tap of the middle source column
        i = iw // 2
        k = int(np.argmax(xw[i]))
        xw[i, k] = 0
    flat = np.array(g, dtype=np.float32).reshape(-1)
    sep = bool(cls) and cls["kernel"] == "sep"
    if fault == "stale_tail":
        if not (sep and cls["tail"]):
            return None
        flat[oh * ow - (oh * ow) % 4:oh * ow] = STALE                      # plane 0 is the one that is 16-byte aligned
    pitch = oh if fault == "swap_pitch" else ow
    base = (np.arange(P) * oh * ow)[:, None, None]
    row = np.zeros((P, oh, iw), dtype=np.float32)
    for b in range(xi.shape[1]):
        v = flat[np.clip(base + (np.arange(oh) * pitch)[None, :, None] + xi[None, None, :, b], 0, flat.size - 1)]
        row = _fma(np.broadcast_to(xw[None, None, :, b], v.shape), v, row)
    acc = np.zeros((P, ih, iw), dtype=np.float32)
    for a in range(yi.shape[1]):
        acc = _fma(np.broadcast_to(yw[None, :, None, a], acc.shape), row[:, yi[:, a], :], acc)
    if fault == "ragged_plane_skipped":
        if not (sep and cls["ragged"]):
            return None
        acc[-1] = np.nan
    return acc
