"""CPU only: the references of tests/refiner_fwd_ref.py agree with oracle/refiner.py and with torch's functional forms in f64, every named fault moves an
output beyond ten times the bound tests/test_gpu_refiner_fwd.py uses for it, the case tables reach the kernels' edges, and the margin of the window loss
holds for the recorded seeds."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import refiner as OR
import refiner_fwd_ref as R
import refiner_outputs_ref as RO

ids = lambda c: "-".join(str(x) for x in c[:5] if not isinstance(x, tuple))  # noqa: E731


def counts_of(img, B):
    return [int((img == b).sum()) for b in range(B)]


# ================================================================================================ the references against the oracle and torch
@pytest.mark.parametrize("kind", R.ENTROPY_KINDS)
@pytest.mark.parametrize("case", R.ENTROPY_CASES, ids=ids)
def test_entropy_reference_is_the_oracle(case, kind):
    preds, ws = R.entropy_inputs(case, kind), case[3]
    inside = bool(((preds >= 0) & (preds <= 1)).all())
    assert inside == (kind == "prob")                                           # the selector's "already a probability?" test takes the branch meant
    lo, hi = (-14.0, 14.0) if kind == "logit" else (0.0, 1.0)
    assert int((preds == lo).sum()) >= 2 and int((preds == hi).sum()) >= 2     # the planted values: the clamp, and p -> 1
    e, s = R.expected("entropy", case, kind)[0]
    oe, omask, _, _ = OR.entropy_select(preds.double(), ws, 0.0015)
    pooled = F.adaptive_avg_pool2d(oe, (ws, ws))
    assert R.rel_l2(e, oe) < 1e-14 and R.rel_l2(s, pooled[:, 0]) < 1e-13
    assert torch.equal(omask[:, 0], s > 0.0015)
    assert not bool(torch.isnan(e).any()) and float(e.min()) >= 0.0
    p = torch.sigmoid(preds.double()) if kind == "logit" else preds.double()
    assert int((p < 1e-5).sum()) >= 2                                           # the clamp is taken


def test_gather_tokens_reference_is_the_index_formula():
    for case in R.TOKEN_CASES[:5]:
        n, nsrc, C, HW, idx = case
        src, ix = R.token_inputs(case)
        out = R.gather_tokens(src, ix)
        assert out.shape == (n * HW, C) and len(idx) == n and max(idx) < nsrc
        g = torch.Generator().manual_seed(C)
        for _ in range(50):
            i, p, c = (int(torch.randint(0, m, (1,), generator=g)) for m in (n, HW, C))
            assert float(out.view(-1)[(i * HW + p) * C + c]) == float(src.reshape(-1)[(idx[i] * C + c) * HW + p])
    assert len(set(R.TOKEN_CASES[3][4])) < len(R.TOKEN_CASES[3][4])             # the repeated index


@pytest.mark.parametrize("case", R.DWCONV_CASES, ids=ids)
def test_dwconv_reference_is_the_oracle_and_the_tap_sum(case):
    x = R.dwconv_inputs(case)
    n, H, W, C = case
    ref = R.expected("dwconv", case)[0][0]
    xd = x["x"].double().permute(0, 3, 1, 2)
    y = F.conv2d(xd, x["dwT"].double().t().reshape(C, 1, 7, 7), x["dwb"].double(), padding=3, groups=C)           # oracle.refiner.csf's last two lines
    assert R.rel_l2(ref, F.conv2d(y, x["w1"].double().view(1, C, 1, 1), torch.tensor([x["b1"]], dtype=torch.float64))) < 1e-13
    # the kernel comment's own sum: out = b1 + sum_c w1[c] (dwb[c] + sum_taps dwT[ky * 7 + kx][c] x[y + ky - 3][x + kx - 3][c])
    xp = F.pad(x["x"].double(), (0, 0, 3, 3, 3, 3))
    acc = x["dwb"].double().expand(n, H, W, C).clone()
    for ky in range(7):
        for kx in range(7):
            acc += x["dwT"].double()[ky * 7 + kx] * xp[:, ky:ky + H, kx:kx + W]
    assert R.rel_l2(ref, ((acc * x["w1"].double()).sum(-1) + x["b1"]).view(n, 1, H, W)) < 1e-13


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=lambda c: f"ws{c[0]}-{c[1]}x{c[2]}-B{c[3]}-n{len(c[4])}")
def test_scatter_reference_is_the_oracle_and_the_adjoint_of_gather(case):
    ws, H, W, B, cells = case
    dl2, win, coords, img = R.gather_inputs(case)
    out = R.scatter(win, coords, img, B, H, W, ws)
    with RO._all_f64(True):
        ref = OR.concat_windows(win.double(), coords, counts_of(img, B), ws)
    assert out.shape == ref.shape == (B, 1, ws * H, ws * W) and torch.equal(out, ref)
    assert int((out != 0).sum()) == len(cells) * H * W
    # <scatter(x), y> == <x, gather(y)>
    lhs, rhs = float((out * dl2.double()).sum()), float((win.double() * R.gather(dl2, coords, img, H, W, ws)).sum())
    assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs))
    if not cells:
        assert float(out.abs().max()) == 0.0


@pytest.mark.parametrize("case", R.GE_FWD_CASES, ids=ids)
def test_gated_ensemble_reference_is_the_oracle(case):
    x = R.ge_inputs(case)
    out, w = R.expected("ge", case)[0]
    sd = {"GE.fuser.0.weight": x["a"].double().view(64, 1, 1, 1), "GE.fuser.0.bias": x["c"].double(), "GE.fuser.2.weight": x["d"].double().view(1, 64, 1, 1),
          "GE.fuser.2.bias": torch.tensor([x["b"]], dtype=torch.float64)}
    o_out, o_w = OR.gated_ensembler(x["l1"].double(), x["l2"].double(), sd)     # (its local average is f32 by construction: `p.float()`)
    assert R.rel_l2(w, o_w) < 2e-6 and R.rel_l2(out, o_out) < 2e-6
    # the torch functional form in f64
    p = torch.sigmoid(x["l1"].double())
    loc = F.avg_pool2d(p, 19, padding=9, stride=1)
    en = -loc * torch.log(loc.clamp(1e-5))
    wf = ((1 - en / en.max()) + p.mean(dim=(1, 2, 3), keepdim=True)) / 2
    y = x["l1"].double() * wf + x["l2"].double() * (1 - wf)
    of = F.conv2d(torch.relu(F.conv2d(y, sd["GE.fuser.0.weight"], sd["GE.fuser.0.bias"])), sd["GE.fuser.2.weight"], sd["GE.fuser.2.bias"])
    assert R.rel_l2(w, wf) < 1e-13 and R.rel_l2(out, of) < 1e-13
    assert float(en.max()) > 0.0 and 0.0 <= float(w.min()) and float(w.max()) <= 1.0


@pytest.mark.parametrize("kind", R.WL_KINDS)
@pytest.mark.parametrize("case", R.WL_CASES, ids=ids)
def test_window_loss_reference_is_the_oracle(case, kind):
    n, B, H, W, ws, flats = case
    x = R.window_loss_inputs(case, kind)
    loss, iou, part = R.expected("window_loss", case, kind)[0]
    mask = torch.zeros(B * ws * ws, dtype=torch.bool)
    mask[list(flats)] = True
    with RO._all_f64(True):
        o_loss, o_t, o_w = OR.cal_ex_loss(x["l_up"].double(), x["x"].double(), mask.view(B, 1, ws, ws), x["h_targets"].double(), ws)
    lb = torch.stack([(x["l_up"][b, :, wy * H:(wy + 1) * H, wx * W:(wx + 1) * W] > 0) for b, wy, wx in (R._cell(f, ws) for f in flats)])
    t, w = x["h_targets"].double()[list(flats)], (1.5 * iou).clamp(0, 1).view(-1, 1, 1, 1)
    # binary_iou returns f32, so the oracle's weights w carry f32 roundings, |dw| <= 2^-22 (two roundings of a value <= 1.5), and the loss moves by
    # dw d loss / d w = dw sum_pixels x (l - t) / (2 n H W) per window
    slack = float((2.0 ** -22 * (x["x"].double() * (lb.double() - t)).sum((1, 2, 3)).abs()).sum()) / (2 * n * H * W)
    assert abs(float(loss) - float(o_loss)) < slack + 1e-13 * abs(float(o_loss)) and torch.equal(o_t, t)
    assert float((w.view(-1) - o_w).abs().max()) < 2.0 ** -22
    assert float((iou - OR.binary_iou(x["h_targets"][list(flats)], lb.float())).abs().max()) < 2.0 ** -23
    # torch's functional form in f64 with the f64 weights
    bce = lambda z: F.binary_cross_entropy_with_logits(x["x"].double(), z, reduction="none")  # noqa: E731
    assert abs(float((w * bce(t) + (1 - w) * bce(lb.double())).mean() / 2) - float(loss)) < 1e-13 * abs(float(loss))
    assert abs(float(part.sum()) / (2 * n * H * W) - float(loss)) < 1e-15
    assert float(x["x"].max()) == 30.0 and float(x["x"].min()) == -30.0


# ================================================================================================ the margin, the ties and the empty union
@pytest.mark.parametrize("kind", R.WL_KINDS)
@pytest.mark.parametrize("case", R.WL_CASES, ids=ids)
def test_window_loss_margin_and_planted_values(case, kind):
    n, B, H, W, ws, flats = case
    assert R.WL_SEEDS[(case, kind)] == 0                                         # recorded: the first offset already keeps the margin
    inp, ties = R._wl_inputs(case, kind, R.WL_SEEDS[(case, kind)])
    assert R.margin_violations(inp, ties) == 0
    assert int(ties[0].sum()) == 1 and int(ties[1].sum()) == 1
    t, l = inp["h_targets"][ties[0]], inp["l_up"][ties[1]]
    assert float(l) == 0.0 and float(torch.sigmoid(t.double()) if kind == "logit" else t) == 0.5
    assert float(torch.sigmoid(torch.zeros(1))) == 0.5 and float(torch.sigmoid(torch.zeros(1, dtype=torch.float64))) == 0.5
    # f32 and f64 binarise alike, so the intersection and union counts are the same integers: the f32 form's iou is the f64 one up to two roundings
    (_, iou, _), (_, iou32, _) = R.expected("window_loss", case, kind)
    assert float(R.pointwise_error(iou32, iou).max()) < 4 * 2.0 ** -24
    if (case, 1) == R.WL_EMPTY:
        assert float(iou[1]) == 0.0 and float(iou32[1]) == 0.0 and float(iou[0]) > 0.0


# ================================================================================================ every fault is beyond ten times a bound
def excess(bad, ref, f32, pointwise=()):
    """the largest error / bound over the outputs; a NaN counts as infinite (the GPU test refuses a NaN outright)"""
    worst = 0.0
    for k, (b, r, f) in enumerate(zip(bad, ref, f32)):
        ratio = (R.pointwise_error(b, r) / R.pointwise_bound(f, r)).max() if k in pointwise else torch.tensor(R.rel_l2(b, r) / R.small_bound(f, r))
        worst = max(worst, math.inf if bool(torch.isnan(ratio)) else float(ratio))
    return worst


FAULT_TABLE = ([("entropy", f) for f in R.ENTROPY_FAULTS] + [("dwconv", f) for f in R.DWCONV_FAULTS] + [("ge", f) for f in R.GE_FAULTS] +
               [("window_loss", f) for f in R.WL_FAULTS])


def faulty(kernel, case, kind, fault):
    if kernel == "entropy":
        return R.entropy_scores(R.entropy_inputs(case, kind), case[3], int(kind == "logit"), fault=fault)
    if kernel == "dwconv":
        return (R.dwconv_maskdec(**R.dwconv_inputs(case), fault=fault),)
    if kernel == "ge":
        return R.gated_ensemble(**R.ge_inputs(case), fault=fault)
    return R.window_loss(**R.window_loss_inputs(case, kind), fault=fault)


TABLES = dict(entropy=(R.ENTROPY_CASES, R.ENTROPY_KINDS), dwconv=(R.DWCONV_CASES, (None,)), ge=(R.GE_FWD_CASES, (None,)), window_loss=(R.WL_CASES, R.WL_KINDS))


@pytest.mark.parametrize("kernel,fault", FAULT_TABLE, ids=lambda v: v)
def test_every_fault_exceeds_ten_times_a_bound(kernel, fault):
    cases, kinds = TABLES[kernel]
    over = {}
    for case in cases:
        for kind in kinds:
            ref, f32 = R.expected(kernel, case, kind)
            over[(case[:5], kind)] = excess(faulty(kernel, case, kind, fault), ref, f32, pointwise=(1,) if kernel == "window_loss" else ())
    caught = {k: v for k, v in over.items() if v > 10.0}
    print(f"{kernel}.{fault}: error / bound per case:", {k: f"{v:.3g}" for k, v in over.items()})
    assert caught, (kernel, fault, over)
    if fault == "floor_bins":                                                    # invisible where H % ws == 0: what the suite ran before these cases
        for kind in kinds:
            good, bad = R.expected("entropy", (2, 6, 6, 3), kind)[0], faulty("entropy", (2, 6, 6, 3), kind, fault)
            assert all(torch.equal(a, b) for a, b in zip(good, bad))
        assert all(over[(c[:5], k)] > 10.0 for c in R.ENTROPY_CASES for k in kinds if c[1] % c[3] or c[2] % c[3])
    if fault == "hw_swapped":                                                    # invisible on a square map
        assert over[((2, 9, 9, 768), None)] == 0.0
    if fault in ("enmax_per_image", "psum_over_batch"):                          # invisible with one image; the old fixture's size leaves little
        assert over[((1, 16, 16, "mixed"), None)] == 0.0 and over[((3, 12, 21, "mixed"), None)] > 100.0


def test_f32_forms_sit_below_the_floor():
    """the f32 CPU forms of the entropy and ensembler references are far enough below 1e-5 / 4 that the floor governs their bounds"""
    worst = 0.0
    for kernel in ("entropy", "ge"):
        cases, kinds = TABLES[kernel]
        for case in cases:
            for kind in kinds:
                ref, f32 = R.expected(kernel, case, kind)
                worst = max([worst] + [R.rel_l2(f, r) for f, r in zip(f32, ref)])
    print("largest f32-vs-f64 relative L2 of the entropy and ensembler references:", worst)
    assert worst < 1e-6


# ================================================================================================ the case tables reach the edges
def test_case_tables_reach_the_edges():
    T, WG, HALF = 64, 256, 9                                                     # gather tile; threads (= pixels) per workgroup; the window's half-width
    assert (R.TILE, R.WG, R.HALF) == (T, WG, HALF)
    Cs, HWs = {c[2] for c in R.TOKEN_CASES}, {c[3] for c in R.TOKEN_CASES}
    for sizes in (Cs, HWs):                                                      # per axis: below a tile, exactly one, one element into the next, more than two
        assert T in sizes and any(s < T for s in sizes) and any(s > T and s % T == 1 for s in sizes) and any(s > 2 * T for s in sizes)
    assert {T - 1, T, T + 1} <= HWs | Cs and 65 in Cs and 63 in HWs and 64 in Cs & HWs and 130 in Cs and 129 in HWs and 3136 in HWs
    # pooling bins: overlap in one axis, in both, none; a bin above one workgroup's 256 threads; 1-pixel bins
    area = lambda c: max(y1 - y0 for y0, y1 in R.bin_edges(c[1], c[3])) * max(x1 - x0 for x0, x1 in R.bin_edges(c[2], c[3]))  # noqa: E731
    overlap = lambda n, ws: any(a[1] > b[0] for a, b in zip(R.bin_edges(n, ws), R.bin_edges(n, ws)[1:]))  # noqa: E731
    kinds = {(overlap(c[1], c[3]), overlap(c[2], c[3])) for c in R.ENTROPY_CASES}
    assert {(False, False), (True, True)} <= kinds and ((True, False) in kinds or (False, True) in kinds)
    assert sum(area(c) > WG for c in R.ENTROPY_CASES) >= 2 and any(area(c) == 1 for c in R.ENTROPY_CASES) and (1, 37, 37, 3) in R.ENTROPY_CASES
    assert any(area(c) > WG and overlap(c[1], c[3]) and overlap(c[2], c[3]) for c in R.ENTROPY_CASES)
    # the window loss: above 256 pixels per workgroup, a rectangle, ws = 1
    assert any(c[2] * c[3] > WG for c in R.WL_CASES) and any(c[2] != c[3] for c in R.WL_CASES) and any(c[4] == 1 for c in R.WL_CASES)
    assert all(len(c[5]) == c[0] and max(c[5]) < c[1] * c[4] ** 2 and list(c[5]) == sorted(set(c[5])) for c in R.WL_CASES)
    assert any(R._cell(f, c[4])[1] != R._cell(f, c[4])[2] for c in R.WL_CASES for f in c[5])        # a window off the diagonal: wy != wx
    # the depthwise conv: C below 256 and C no multiple of 256; H or W below 7; H != W
    assert any(c[3] < WG for c in R.DWCONV_CASES) and any(c[3] > WG and c[3] % WG for c in R.DWCONV_CASES)
    assert any(c[1] < 7 <= c[2] for c in R.DWCONV_CASES) and any(c[2] < 7 <= c[1] for c in R.DWCONV_CASES) and any(c[1] < 7 and c[2] < 7 and c[1] != c[2] for c in R.DWCONV_CASES)
    assert any(c[1] > 7 and c[2] > 7 and c[1] != c[2] for c in R.DWCONV_CASES) and (1, 1, 1, 768) in R.DWCONV_CASES
    # the ensembler: >= 3 workgroups per image (where an order of arrival exists), exactly one; h and w on both sides of 10 and 19
    wgs = [-(-c[1] * c[2] // WG) for c in R.GE_FWD_CASES]
    assert max(wgs) >= 3 and any(c[1] * c[2] == WG for c in R.GE_FWD_CASES) and any(c[0] > 1 and g >= 3 for c, g in zip(R.GE_FWD_CASES, wgs))
    for axis in (1, 2):
        sizes = {c[axis] for c in R.GE_FWD_CASES}
        assert min(sizes) < HALF + 1 < 2 * HALF + 1 < max(sizes) and any(HALF + 1 <= s < 2 * HALF + 1 for s in sizes)
    assert any(c[1] != c[2] for c in R.GE_FWD_CASES)
    # the scatter: rectangles, an image without a window, n = 0
    assert any(c[1] != c[2] for c in R.GATHER_CASES) and any(len(c[4]) == 0 for c in R.GATHER_CASES)
