"""CPU references for the CORAL refiner's forward kernels (csrc/refiner.hip: ucod_entropy_scores, ucod_gather_tokens, ucod_dwconv7_maskdec,
ucod_window_scatter, ucod_gated_ensemble, ucod_window_loss), their case tables, seeded inputs and bounds.

Test infrastructure only: nothing here is the code under test, nothing here imports it, and nothing here reads GPU output to set a bound.

Every reference takes a ``dtype`` (float64: the reference; float32: the same formula on the CPU, whose distance from float64 sets the bound) and a
``fault`` (None, or the name of one wrong reading of the formula; tests/test_refiner_fwd_host.py shows that the bounds catch each).  The formulas restate
the kernel comments of csrc/refiner.hip and oracle/refiner.py in plain torch.

Bounds (none of them is tuned from what the kernels give):
* ``small_bound``: the project's rule for a small f32 kernel (tests/test_gpu_refiner_train.py): per tensor, relative L2 <= max(4 x the relative L2 of the
  same formula in f32 on the CPU against f64, 1e-5); the floor covers another summation order over the f32 terms.
* ``pointwise_bound``: the same rule per element (the IoU of each window of ucod_window_loss: a lost pixel of one window must not hide in an L2 norm).
* ucod_gather_tokens is a permutation: torch.equal.  ucod_window_scatter: GATHER_BOUND = 2^-22 per element (one f32 rounding of the divisor 1 + 1e-6 and
  one of the quotient, the bound of its adjoint ucod_window_gather), exact zeros elsewhere.

The margin of ucod_window_loss.  The kernel binarises l = sigmoid(l_up) > 0.5 and t' > 0.5 in f32; the reference in f64.  Apart from the planted exact
ties (l_up == 0 and t' == 0.5, where both give "not above": sigmoid(0) is exactly 0.5 in either format), no pixel of a case has |l_up| <= MARGIN or
|t' - 0.5| <= MARGIN, MARGIN = 1e-5 -- 80 ulp of 0.5 in f32, far beyond the few ulp of an f32 sigmoid.  So both binarise alike, and the intersection and
union counts are exact integers in both.  ``window_loss_inputs`` asserts it; WL_SEEDS records the first seed offset per case that satisfies it.
"""
import functools

import torch
import torch.nn.functional as F

from refiner_outputs_ref import GE_CASES, GATHER_CASES, gather, gather_inputs, kernel_inputs, _ge_inputs  # noqa: F401

TILE = 64                   # ucod_gather_tokens: 64 x 64 LDS tiles over (C, HW)
WG = 256                    # threads per workgroup of every kernel here: the stride of the strided loops, the pixels per workgroup of the ensembler
HALF = 9                    # half-width of the ensembler's 19 x 19 window
GATHER_BOUND = 2.0 ** -22
MARGIN = 1e-5


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def small_bound(f32, f64):
    return max(4.0 * rel_l2(f32, f64), 1e-5)


def pointwise_error(x, ref):
    x, ref = x.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return (x - ref).abs() / ref.abs().clamp_min(1e-30)


def pointwise_bound(f32, f64):
    return (4.0 * pointwise_error(f32, f64)).clamp_min(1e-5)


# ================================================================================================ ucod_entropy_scores
# (B, H, W, ws): divisible (no overlap); overlap in both axes; the same with H != W and ws = 4; one bin of 400 > 256 pixels; 1-pixel bins; the production
# size; 20 x 19 = 380 > 256 pixels per bin with overlap in both axes; overlap in the columns only (6 % 3 == 0, 7 % 3 != 0)
ENTROPY_CASES = ((2, 6, 6, 3), (2, 7, 7, 3), (1, 10, 13, 4), (1, 20, 20, 1), (2, 5, 5, 5), (1, 37, 37, 3), (1, 58, 55, 3), (1, 6, 7, 3))
ENTROPY_KINDS = ("logit", "prob")
ENTROPY_FAULTS = ("floor_bins", "no_clamp", "sum_not_mean")


def bin_edges(n, ws, floor_end=False):
    """[(start, end)] of adaptive_avg_pool2d's ``ws`` bins over ``n``: floor(i n / ws) .. ceil((i + 1) n / ws)"""
    return [((i * n) // ws, ((i + 1) * n) // ws if floor_end else -(-(i + 1) * n // ws)) for i in range(ws)]


def entropy_inputs(case, kind):
    """preds [B,1,H,W] f32.  "logit": randn * 2 with -14 (p = 8e-7 < 1e-5: the clamp) and +14 (p -> 1) planted; "prob": rand in (0, 1) with exactly 0.0 and
    1.0 planted (use_sigmoid = 0)."""
    B, H, W, ws = case
    g = torch.Generator().manual_seed(4100 + 1000 * B + 10 * H + W + ws + (500 if kind == "prob" else 0))
    lo, hi = (-14.0, 14.0) if kind == "logit" else (0.0, 1.0)
    preds = torch.randn(B, 1, H, W, generator=g) * 2 if kind == "logit" else torch.rand(B, 1, H, W, generator=g) * 0.998 + 0.001
    flat = preds.view(-1)
    n = flat.numel()
    flat[0], flat[n // 2], flat[n // 3], flat[n - 1] = lo, lo, hi, hi
    return preds


def entropy_scores(preds, ws, use_sigmoid, dtype=torch.float64, fault=None):
    """ucod_entropy_scores -> (entropy [B,1,H,W], scores [B,ws,ws]).  ``fault``: "floor_bins" (non-overlapping bins: the end edge floored), "no_clamp"
    (log(p) in place of log(max(p, 1e-5))), "sum_not_mean" (the bin's sum)."""
    assert fault is None or fault in ENTROPY_FAULTS
    p = preds.to(dtype)
    if use_sigmoid:
        p = torch.sigmoid(p)
    e = -p * torch.log(p if fault == "no_clamp" else p.clamp_min(1e-5))
    B, _, H, W = e.shape
    scores = torch.zeros(B, ws, ws, dtype=dtype)
    for i, (y0, y1) in enumerate(bin_edges(H, ws, fault == "floor_bins")):
        for j, (x0, x1) in enumerate(bin_edges(W, ws, fault == "floor_bins")):
            cell = e[:, 0, y0:y1, x0:x1]
            scores[:, i, j] = cell.sum((1, 2)) if fault == "sum_not_mean" else cell.sum((1, 2)) / ((y1 - y0) * (x1 - x0))
    return e, scores


# ================================================================================================ ucod_gather_tokens
# (n, nsrc, C, HW, indices): the suite's old shape; 1 x 1; one below / one above a tile in C, one below in HW; exactly one tile with a repeated index; two
# tiles plus 2 in C, two tiles plus 1 in HW; the production HW (49 tiles)
TOKEN_CASES = ((3, 5, 768, 30, (3, 0, 4)), (1, 1, 1, 1, (0,)), (2, 3, 65, 63, (2, 0)), (4, 2, 64, 64, (1, 0, 1, 1)), (2, 4, 130, 129, (3, 1)),
               (2, 3, 96, 3136, (2, 1)))


def token_inputs(case):
    n, nsrc, C, HW, idx = case
    src = torch.randn(nsrc, C, HW, generator=torch.Generator().manual_seed(4200 + C + HW))
    return src, torch.tensor(idx, dtype=torch.int32)


def gather_tokens(src, idx, dtype=None, fault=None):
    """ucod_gather_tokens: out[(i HW + p) C + c] = src[idx[i]][c][p] -> [n HW, C]; a permutation, exact in any dtype"""
    assert fault is None
    out = src[idx.long()].permute(0, 2, 1).reshape(-1, src.shape[1])
    return out if dtype is None else out.to(dtype)


# ================================================================================================ ucod_dwconv7_maskdec
# (n, H, W, C): the suite's old shape; one pixel (only the centre tap lands); H, W < 7 and H != W; W < 7 <= H with C = 96 < 256; H < 7 <= W with
# C = 300 = 256 + 44 (the strided channel loop's tail); H, W >= 7, H != W
DWCONV_CASES = ((2, 9, 9, 768), (1, 1, 1, 768), (2, 3, 5, 768), (1, 7, 4, 96), (1, 6, 9, 300), (1, 12, 10, 768))
DWCONV_FAULTS = ("tap_transposed", "no_bias", "hw_swapped")


def dwconv_inputs(case):
    n, H, W, C = case
    g = torch.Generator().manual_seed(4300 + 100 * n + 10 * H + W + C)
    return dict(x=torch.randn(n, H, W, C, generator=g), dwT=torch.randn(49, C, generator=g) * 0.15, dwb=torch.randn(C, generator=g) * 0.3,
                w1=torch.randn(C, generator=g) * 0.1, b1=0.37)


def dwconv_maskdec(x, dwT, dwb, w1, b1, dtype=torch.float64, fault=None):
    """ucod_dwconv7_maskdec: x [n,H,W,C] token-major, dwT [49,C] tap-major -> out [n,1,H,W] = b1 + sum_c w1[c] (dwb[c] + (dw[c] * x[c])(y, x)), the 7 x 7
    cross-correlation zero-padded by 3.  ``fault``: "tap_transposed" (ky / kx exchanged), "no_bias" (dwb dropped), "hw_swapped" (the rows of x and of out
    read as [W, H])."""
    assert fault is None or fault in DWCONV_FAULTS
    x, dwT, dwb, w1 = (v.to(dtype) for v in (x, dwT, dwb, w1))
    n, H, W, C = x.shape
    wgt = dwT.t().reshape(C, 1, 7, 7)
    if fault == "tap_transposed":
        wgt = wgt.transpose(2, 3)
    if fault == "hw_swapped":
        x = x.reshape(n, W, H, C)
    y = F.conv2d(x.permute(0, 3, 1, 2), wgt, None if fault == "no_bias" else dwb, padding=3, groups=C)
    return ((y * w1.view(1, C, 1, 1)).sum(1, keepdim=True) + b1).reshape(n, 1, H, W)


# ================================================================================================ ucod_window_scatter
def scatter(win, coords, img, B, H, W, ws, dtype=torch.float64, fault=None):
    """ucod_window_scatter, oracle.refiner.concat_windows for distinct cells: [B,1,ws H,ws W], window i / (1 + 1e-6) at cell coords[i] = (cy, cx) of
    image img[i], zeros elsewhere.  Cases and inputs: GATHER_CASES / gather_inputs of its adjoint (the windows are their ``g0``)."""
    assert fault is None
    out = torch.zeros(B, 1, ws * H, ws * W, dtype=dtype)
    for i, ((cy, cx), b) in enumerate(zip(coords.tolist(), img.tolist())):
        out[b, 0, cy * H:(cy + 1) * H, cx * W:(cx + 1) * W] = win[i, 0].to(dtype) / (1 + 1e-6)
    return out


# ================================================================================================ ucod_gated_ensemble
# GE_CASES' shapes (1 partial workgroup; 2 per image; non-square with B = 3; exactly 1; 16 per image) plus a map one row high and one five columns wide:
# narrower than the window's half-width in one axis (every window of that axis is cut on both sides) and wider than the window in the other
GE_FWD_CASES = GE_CASES + ((1, 1, 40, "mixed"), (2, 30, 5, "mixed"))
GE_FAULTS = ("replicate_pad", "win17", "enmax_per_image", "psum_over_batch")
GE_B = -0.21                # fuser.2.bias


def ge_inputs(case):
    """{l1, l2, a, c, d, b}: the (seeded) inputs of the backward's kernel case of that shape"""
    x = kernel_inputs(case) if case in GE_CASES else _ge_inputs(case, 0)
    return dict(l1=x["l1"], l2=x["l2"], a=x["a"], c=x["c"], d=x["d"], b=GE_B)


def gated_ensemble(l1, l2, a, c, d, b, dtype=torch.float64, fault=None):
    """ucod_gated_ensemble -> (out, weight), both [B,1,h,w]: p = sigmoid(l1); m = the 19 x 19 sum of p around the pixel, zero beyond the map, / 361;
    en = -m log(max(m, 1e-5)); weight = ((1 - en / max en over the WHOLE batch) + mean of p over the image) / 2; y = l1 weight + l2 (1 - weight);
    out = b + sum_k d_k relu(a_k y + c_k).  ``fault``: "replicate_pad" (the border repeated), "win17" (a 17 x 17 window / 289), "enmax_per_image",
    "psum_over_batch" (the mean of p over the batch)."""
    assert fault is None or fault in GE_FAULTS
    l1, l2, a, c, d = (v.to(dtype) for v in (l1, l2, a, c, d))
    p = torch.sigmoid(l1)
    g = p.mean() if fault == "psum_over_batch" else p.mean(dim=(1, 2, 3), keepdim=True)
    r = 8 if fault == "win17" else HALF
    pp = F.pad(p, (r, r, r, r), mode="replicate") if fault == "replicate_pad" else F.pad(p, (r, r, r, r))
    m = F.conv2d(pp, torch.ones(1, 1, 2 * r + 1, 2 * r + 1, dtype=dtype)) / (2 * r + 1) ** 2
    en = -m * torch.log(m.clamp_min(1e-5))
    enmax = en.amax(dim=(1, 2, 3), keepdim=True) if fault == "enmax_per_image" else en.max()
    wgt = ((1 - en / enmax) + g) / 2
    y = l1 * wgt + l2 * (1 - wgt)
    z = a.view(1, 64, 1, 1) * y + c.view(1, 64, 1, 1)
    return (d.view(1, 64, 1, 1) * z.clamp_min(0)).sum(1, keepdim=True) + b, wgt


# ================================================================================================ ucod_window_loss
# (n, B, H, W, ws, the selected windows' flat indices b ws^2 + j): one window; non-square windows, windows off the diagonal of their image; all 18 of the
# G9 geometry; H W = 272 > 256 (the strided pixel loops take a second turn); ws = 1 with a 3 x 3 window
WL_CASES = ((1, 2, 6, 6, 3, (11,)), (3, 2, 9, 7, 3, (1, 5, 15)), (18, 2, 6, 6, 3, tuple(range(18))), (2, 1, 17, 16, 2, (1, 2)), (1, 1, 3, 3, 1, (0,)))
WL_KINDS = ("prob", "logit")
WL_FAULTS = ("ge_not_gt", "no_half", "l_from_wrong_cell")
WL_EMPTY = ((3, 2, 9, 7, 3, (1, 5, 15)), 1)              # (case, window): target and l both empty there: union 0, iou 0
WL_SEEDS = {(c, k): 0 for c in WL_CASES for k in WL_KINDS}          # the first seed offset that keeps the margin (window_loss_inputs asserts it)


def _cell(flat, ws):
    b, j = divmod(flat, ws * ws)
    return (b,) + divmod(j, ws)


def _wl_inputs(case, kind, offset):
    n, B, H, W, ws, flats = case
    g = torch.Generator().manual_seed(4500 + 1000 * offset + 100 * n + 10 * H + W + ws + (50 if kind == "logit" else 0))
    x = torch.randn(n, 1, H, W, generator=g) * 3
    x.view(-1)[0], x.view(-1)[-1] = 30.0, -30.0                                     # the stable form of BCEWithLogits: exp(-|x|) underflows to nothing
    t = torch.rand(B * ws * ws, 1, H, W, generator=g)
    t[::2, :, :(H + 1) // 2] = (t[::2, :, :(H + 1) // 2] > 0.4).float()           # a mix of hard and soft pixels (tests/golden/refiner_init.py)
    l_up = torch.randn(B, 1, ws * H, ws * W, generator=g) * 2
    ties = torch.zeros(B * ws * ws, 1, H, W, dtype=torch.bool), torch.zeros_like(l_up, dtype=torch.bool)
    if (case, 1) == WL_EMPTY:
        b, wy, wx = _cell(flats[1], ws)
        t[flats[1]] = t[flats[1]] * 0.45
        l_up[b, 0, wy * H:(wy + 1) * H, wx * W:(wx + 1) * W] = -l_up[b, 0, wy * H:(wy + 1) * H, wx * W:(wx + 1) * W].abs() - 0.01
    if kind == "logit":
        t = (t - 0.5) * 9.0
    b, wy, wx = _cell(flats[0], ws)                                                 # the exact ties, in the first selected window
    t[flats[0], 0, H - 1, 0] = 0.5 if kind == "prob" else 0.0
    ties[0][flats[0], 0, H - 1, 0] = True
    l_up[b, 0, wy * H, wx * W + W - 1] = 0.0
    ties[1][b, 0, wy * H, wx * W + W - 1] = True
    return dict(x=x, h_targets=t, flat=torch.tensor(flats, dtype=torch.int32), l_up=l_up, logits=int(kind == "logit")), ties


def margin_violations(inp, ties):
    """how many pixels other than the planted ties lie within MARGIN of a threshold"""
    t = inp["h_targets"].double()
    tp = torch.sigmoid(t) if inp["logits"] else t
    return int((((tp - 0.5).abs() <= MARGIN) & ~ties[0]).sum()) + int(((inp["l_up"].double().abs() <= MARGIN) & ~ties[1]).sum())


@functools.lru_cache(maxsize=None)
def window_loss_inputs(case, kind):
    inp, ties = _wl_inputs(case, kind, WL_SEEDS[(case, kind)])
    bad = margin_violations(inp, ties)
    assert bad == 0, (case, kind, bad, "pixels inside the margin: pick another seed offset")
    assert int(inp["logits"]) == int(float(inp["h_targets"][inp["flat"].long()].max()) > 1)       # the caller's "max > 1" heuristic says the same
    return inp


def window_loss(x, h_targets, flat, l_up, logits, dtype=torch.float64, fault=None):
    """ucod_window_loss -> (loss 0-d, iou [n], part [n]).  Window i is cell (wy, wx) = divmod(flat[i] % ws^2, ws) of image flat[i] // ws^2:
    l = sigmoid(l_up's block) > 0.5, t = h_targets[flat[i]], t' = sigmoid(t) if ``logits`` else t; iou = |t' > 0.5 and l| / (|t' > 0.5 or l| + 1e-6);
    w = clamp(1.5 iou, 0, 1); part = sum over pixels of w BCEWithLogits(x, t) + (1 - w) BCEWithLogits(x, l); loss = sum part / (2 n H W).
    ``fault``: "ge_not_gt" (>= 0.5 in both comparisons), "no_half" (/ (n H W)), "l_from_wrong_cell" (wy and wx exchanged)."""
    assert fault is None or fault in WL_FAULTS
    x, h_targets, l_up = (v.to(dtype) for v in (x, h_targets, l_up))
    n, _, H, W = x.shape
    ws = l_up.shape[-1] // W
    above = (lambda v: v >= 0.5) if fault == "ge_not_gt" else (lambda v: v > 0.5)
    iou, part = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    for i, f in enumerate(flat.tolist()):
        b, wy, wx = _cell(f, ws)
        if fault == "l_from_wrong_cell":
            wy, wx = wx, wy
        lb = above(torch.sigmoid(l_up[b, 0, wy * H:(wy + 1) * H, wx * W:(wx + 1) * W]))
        t = h_targets[f, 0]
        tb = above(torch.sigmoid(t) if logits else t)
        iou[i] = (tb & lb).sum().to(dtype) / ((tb | lb).sum().to(dtype) + 1e-6)
        w = (1.5 * iou[i]).clamp(0, 1)
        xi = x[i, 0]
        sp = xi.clamp_min(0) + torch.log1p(torch.exp(-xi.abs()))
        part[i] = (w * (sp - xi * t) + (1 - w) * (sp - xi * lb.to(dtype))).sum()
    return part.sum() / ((1 if fault == "no_half" else 2) * n * H * W), iou, part


# ================================================================================================ (f64, f32) per case: computed once, shared, never modified
@functools.lru_cache(maxsize=None)
def expected(kernel, case, kind=None):
    """(f64 reference, the same formula in f32 on the CPU) as tuples of tensors"""
    if kernel == "entropy":
        args = (entropy_inputs(case, kind), case[3], int(kind == "logit"))
        return entropy_scores(*args), entropy_scores(*args, dtype=torch.float32)
    if kernel == "dwconv":
        x = dwconv_inputs(case)
        return (dwconv_maskdec(**x),), (dwconv_maskdec(**x, dtype=torch.float32),)
    if kernel == "ge":
        x = ge_inputs(case)
        return gated_ensemble(**x), gated_ensemble(**x, dtype=torch.float32)
    if kernel == "window_loss":
        x = window_loss_inputs(case, kind)
        return window_loss(**x), window_loss(**x, dtype=torch.float32)
    raise KeyError(kernel)
