"""GPU: the CORAL refiner's forward kernels (csrc/refiner.hip) one by one against f64 on their own inputs, at the tile, workgroup and window edges, every
launch twice for bit identity, every output between canary rows on a NaN payload; then SparseRefiner.eval() on a rectangular geometry whose pooling bins
overlap.  References, case tables, seeded inputs and bounds: tests/refiner_fwd_ref.py (none of them is GPU output; tests/test_refiner_fwd_host.py shows
that the bounds catch every named fault and that the tables reach the edges)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import maxdiff, within

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import refiner_init as RI  # noqa: E402
import refiner_fwd_ref as R  # noqa: E402
from oracle import refiner as OR  # noqa: E402
from test_gpu_refiner_outputs import DEV, Guarded, bits, twice  # noqa: E402  (the guarded buffers and the two-run comparison: one copy)
from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.engine.config import CfgNode  # noqa: E402
from ucod_dpl_amd.models.UDLR import SparseRefiner  # noqa: E402

ids = lambda c: "-".join(str(x) for x in c if not isinstance(x, tuple))  # noqa: E731


def sync():
    torch.cuda.synchronize()


def check(kernel, names, got, ref, f32, case):
    """every output's relative L2 against f64 within small_bound (4 x the f32 CPU form's, floor 1e-5)"""
    for name, r, f in zip(names, ref, f32):
        e, b = R.rel_l2(got[name].cpu().reshape(r.shape), r), R.small_bound(f, r)
        print(f"{kernel} {case} {name}: {e:.3e} (bound {b:.3e})")
        within(f"refiner_fwd:{kernel}:{name}", e, b)


# ================================================================================================ ucod_entropy_scores
@pytest.mark.parametrize("kind", R.ENTROPY_KINDS)
@pytest.mark.parametrize("case", R.ENTROPY_CASES, ids=ids)
def test_entropy_scores(case, kind):
    """Entropy and pooled scores against f64, on logits (sigmoid inside) and on probabilities.  Every entropy pixel is written -- the pixels two or four
    overlapping bins cover as well -- and none outside; -14 / 0.0 take the clamp, +14 / 1.0 give p -> 1."""
    B, H, W, ws = case
    lib, st = N.load(), N.stream()
    preds = R.entropy_inputs(case, kind)
    pd = preds.to(DEV)

    def launch():
        e, s = Guarded(B * H, W), Guarded(B, ws * ws)
        assert lib.ucod_entropy_scores(N.ptr(pd), int(kind == "logit"), e.ptr(), s.ptr(), B, H, W, ws, st) == 0
        sync()
        return dict(entropy=e.get(), scores=s.get())            # get(): canaries intact, no NaN left

    got = twice(launch)
    check("entropy_scores", ("entropy", "scores"), got, *R.expected("entropy", case, kind), (case, kind))
    if kind == "prob":                                          # p == 0 (clamped: 0 * log(1e-5)) and p == 1 (log 1): exactly zero entropy
        assert bool((got["entropy"].cpu().view(-1)[(preds.view(-1) == 0.0) | (preds.view(-1) == 1.0)] == 0.0).all())


# ================================================================================================ ucod_gather_tokens
@pytest.mark.parametrize("case", R.TOKEN_CASES, ids=ids)
def test_gather_tokens(case):
    n, nsrc, C, HW, _ = case
    lib, st = N.load(), N.stream()
    src, idx = R.token_inputs(case)
    sd, ixd = src.to(DEV), idx.to(DEV)

    def launch():
        out = Guarded(n * HW, C)
        assert lib.ucod_gather_tokens(N.ptr(sd), N.ptr(ixd), out.ptr(), n, C, HW, st) == 0
        sync()
        return dict(out=out.get())

    assert torch.equal(twice(launch)["out"].cpu(), R.gather_tokens(src, idx))


# ================================================================================================ ucod_dwconv7_maskdec
@pytest.mark.parametrize("case", R.DWCONV_CASES, ids=ids)
def test_dwconv7_maskdec(case):
    n, H, W, C = case
    lib, st = N.load(), N.stream()
    x = R.dwconv_inputs(case)
    dev = {k: v.contiguous().to(DEV) for k, v in x.items() if k != "b1"}

    def launch():
        out = Guarded(n * H, W)
        assert lib.ucod_dwconv7_maskdec(*[N.ptr(dev[k]) for k in ("x", "dwT", "dwb", "w1")], x["b1"], out.ptr(), n, H, W, C, st) == 0
        sync()
        return dict(out=out.get())

    check("dwconv7_maskdec", ("out",), twice(launch), *R.expected("dwconv", case), case)


# ================================================================================================ ucod_window_scatter
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=lambda c: f"ws{c[0]}-{c[1]}x{c[2]}-B{c[3]}-n{len(c[4])}")
def test_window_scatter(case):
    """Each window / (1 + 1e-6) at its cell to GATHER_BOUND per element (the bound of the adjoint), exact zeros everywhere else; n = 0: all zeros, and the
    three inputs may be NULL."""
    ws, H, W, B, cells = case
    lib, st, n = N.load(), N.stream(), len(cells)
    _, win, coords, img = R.gather_inputs(case)
    ref = R.scatter(win, coords, img, B, H, W, ws)
    wd, cd, im = win.to(DEV), coords.to(torch.int32).to(DEV), img.to(torch.int32).to(DEV)

    def launch():
        out = Guarded(B * ws * H, ws * W)
        assert lib.ucod_window_scatter(*([N.ptr(wd), N.ptr(cd), N.ptr(im)] if n else [None, None, None]), out.ptr(), n, B, H, W, ws, st) == 0
        sync()
        return dict(out=out.get())

    got = twice(launch)["out"].cpu().double().view(ref.shape)
    assert bool((got[ref == 0] == 0).all())
    if n == 0:
        assert float(got.abs().max()) == 0.0
        return
    live = ref != 0
    assert int(live.sum()) == n * H * W
    within("refiner_fwd:window_scatter:max_rel", float(((got[live] - ref[live]).abs() / ref[live].abs()).max()), R.GATHER_BOUND)


# ================================================================================================ ucod_gated_ensemble
def run_gated_ensemble(case):
    B, h, w, _ = case
    lib, st = N.load(), N.stream()
    x = R.ge_inputs(case)
    dev = {k: v.contiguous().to(DEV) for k, v in x.items() if k != "b"}
    nbytes = lib.ucod_gated_ensemble_workspace_bytes(B, h, w)
    assert nbytes == 4 * (2 * B * h * w + B * -(-h * w // 256) + 1)

    def launch():
        out, wgt, wsb = Guarded(B * h, w), Guarded(B * h, w), Guarded(1, nbytes // 4)           # the workspace starts as NaN: nothing in it is assumed
        assert lib.ucod_gated_ensemble(*[N.ptr(dev[k]) for k in ("l1", "l2", "a", "c", "d")], x["b"], out.ptr(), wgt.ptr(), wsb.ptr(), B, h, w, st) == 0
        sync()
        assert wsb.intact(), "wrote outside its workspace"
        return dict(out=out.get(), weight=wgt.get())

    return twice(launch)


@pytest.mark.parametrize("case", R.GE_FWD_CASES, ids=ids)
def test_gated_ensemble(case):
    """out and weight against f64; two runs bit-identical at every size -- (3, 63, 63) has 16 workgroups per image, where a sum in order of arrival
    would not be."""
    check("gated_ensemble", ("out", "weight"), run_gated_ensemble(case), *R.expected("ge", case), case)


# ================================================================================================ ucod_window_loss
@pytest.mark.parametrize("kind", R.WL_KINDS)
@pytest.mark.parametrize("case", R.WL_CASES, ids=ids)
def test_window_loss(case, kind):
    """loss and part in relative L2, the IoU of every window on its own (pointwise_bound); the window with an empty union has iou exactly 0; the planted
    ties count as "not above" (the reference's strict comparison: with >= the IoU of the first window moves by a whole pixel); iou_out may be NULL."""
    n, B, H, W, ws, _ = case
    lib, st = N.load(), N.stream()
    x = R.window_loss_inputs(case, kind)
    dev = [x[k].contiguous().to(DEV) for k in ("x", "h_targets", "flat", "l_up")]

    def launch(with_iou=True):
        part, iou, loss = Guarded(1, n), Guarded(1, n), Guarded(1, 1)
        assert lib.ucod_window_loss(*[N.ptr(v) for v in dev], x["logits"], part.ptr(), iou.ptr() if with_iou else None, loss.ptr(), n, B, H, W, ws, st) == 0
        sync()
        if not with_iou:
            assert iou.intact() and bool(torch.isnan(iou.payload).all())
            return dict(loss=loss.get(), part=part.get())
        return dict(loss=loss.get(), iou=iou.get(), part=part.get())

    got = twice(launch)
    ref, f32 = R.expected("window_loss", case, kind)
    check("window_loss", ("loss", "iou", "part"), got, ref, f32, (case[:5], kind))
    err, bound = R.pointwise_error(got["iou"], ref[1]), R.pointwise_bound(f32[1], ref[1])
    i = int((err / bound).argmax())
    print(f"window_loss {case[:5]} {kind}: worst window {i}: iou error {float(err[i]):.3e} (bound {float(bound[i]):.3e})")
    within("refiner_fwd:window_loss:iou_per_window", float(err[i]), float(bound[i]))
    if (case, 1) == R.WL_EMPTY:
        assert float(got["iou"].view(-1)[1]) == 0.0
    if case == R.WL_CASES[1]:
        alone = launch(with_iou=False)
        assert all(torch.equal(bits(alone[k]), bits(got[k])) for k in ("loss", "part"))


# ================================================================================================ argument validation: a refusal writes nothing
def refusals(fn, order, base, outs, bads):
    """``fn(*[base[k] for k in order], stream)`` succeeds; with each of ``bads`` (a dict of replacements) it returns non-zero, and afterwards no output
    buffer of ``outs`` (Guarded, named in ``base`` by their pointers) has been touched"""
    st = N.stream()
    call = lambda **kw: fn(*[kw.get(k, base[k]) for k in order], st)  # noqa: E731
    assert call() == 0
    sync()
    for o in outs:
        o.get()
        o.payload.fill_(float("nan"))
    for bad in bads:
        assert call(**bad) != 0, bad
    sync()
    for o in outs:
        assert o.intact() and bool(torch.isnan(o.payload).all()), "a refused call wrote"


def test_forward_kernels_argument_validation():
    lib = N.load()
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    fp, ip = N.ptr(f), N.ptr(i)
    null = lambda *names: [{k: None} for k in names]  # noqa: E731
    nonpos = lambda *names: [{k: v} for k in names for v in (0, -1)]  # noqa: E731
    # ucod_gather_tokens(src, idx, out, n, C, HW)
    out = Guarded(2 * 3, 5)
    refusals(lib.ucod_gather_tokens, ("src", "idx", "out", "n", "C", "HW"), dict(src=fp, idx=ip, out=out.ptr(), n=2, C=5, HW=3), [out],
             null("src", "idx", "out") + nonpos("n", "C", "HW"))
    # ucod_entropy_scores(preds, use_sigmoid, entropy, scores, B, H, W, ws)
    e, s = Guarded(2 * 4, 5), Guarded(2, 9)
    refusals(lib.ucod_entropy_scores, ("preds", "sig", "entropy", "scores", "B", "H", "W", "ws"),
             dict(preds=fp, sig=1, entropy=e.ptr(), scores=s.ptr(), B=2, H=4, W=5, ws=3), [e, s],
             null("preds", "entropy", "scores") + nonpos("B", "H", "W", "ws") + [dict(ws=5), dict(ws=6), dict(H=2), dict(W=2)])       # ws > H, ws > W
    # ucod_dwconv7_maskdec(x, dwT, dwb, w1, b1, out, n, H, W, C)
    out = Guarded(2 * 3, 4)
    refusals(lib.ucod_dwconv7_maskdec, ("x", "dwT", "dwb", "w1", "b1", "out", "n", "H", "W", "C"),
             dict(x=fp, dwT=fp, dwb=fp, w1=fp, b1=0.5, out=out.ptr(), n=2, H=3, W=4, C=8), [out], null("x", "dwT", "dwb", "w1", "out") + nonpos("n", "H", "W", "C"))
    # ucod_window_scatter(windows, coords, img, out, n, B, H, W, ws): n = 0 is valid (test_window_scatter), n > 0 needs its three inputs
    out = Guarded(2 * 2 * 3, 2 * 4)
    refusals(lib.ucod_window_scatter, ("win", "coords", "img", "out", "n", "B", "H", "W", "ws"),
             dict(win=fp, coords=ip, img=ip, out=out.ptr(), n=2, B=2, H=3, W=4, ws=2), [out],
             null("win", "coords", "img", "out") + nonpos("B", "H", "W", "ws") + [dict(n=-1)])
    # ucod_gated_ensemble(l1, l2, f0w, f0b, f2w, f2b, out, weight, workspace, B, h, w)
    o, w = Guarded(2 * 5, 7), Guarded(2 * 5, 7)
    wsb = torch.zeros(lib.ucod_gated_ensemble_workspace_bytes(2, 5, 7) // 4, dtype=torch.float32, device=DEV)
    refusals(lib.ucod_gated_ensemble, ("l1", "l2", "a", "c", "d", "b", "out", "weight", "wsp", "B", "h", "w"),
             dict(l1=fp, l2=fp, a=fp, c=fp, d=fp, b=0.1, out=o.ptr(), weight=w.ptr(), wsp=N.ptr(wsb), B=2, h=5, w=7), [o, w],
             null("l1", "l2", "a", "c", "d", "out", "weight", "wsp") + nonpos("B", "h", "w"))
    # ucod_gated_ensemble_workspace_bytes refuses nothing: the size of the layout (include/ucod_dpl.h), growing with the workgroups per image
    size = lambda B, h, w: lib.ucod_gated_ensemble_workspace_bytes(B, h, w)  # noqa: E731
    assert size(1, 16, 16) == 4 * (512 + 1 + 1) and size(1, 16, 17) == 4 * (544 + 2 + 1) and size(2, 168, 168) == 4 * (2 * 2 * 28224 + 2 * 111 + 1)
    # ucod_window_loss(window_preds, h_targets, win_flat, l_up, targets_are_logits, part, iou_out, loss_out, n, B, H, W, ws): iou_out may be NULL
    part, iou, loss = Guarded(1, 2), Guarded(1, 2), Guarded(1, 1)
    refusals(lib.ucod_window_loss, ("x", "t", "flat", "l_up", "logits", "part", "iou", "loss", "n", "B", "H", "W", "ws"),
             dict(x=fp, t=fp, flat=ip, l_up=fp, logits=0, part=part.ptr(), iou=iou.ptr(), loss=loss.ptr(), n=2, B=1, H=3, W=4, ws=2), [part, iou, loss],
             null("x", "t", "flat", "l_up", "part", "loss") + nonpos("n", "B", "H", "W", "ws"))


# ================================================================================================ the whole module on a rectangle
THRESHOLD = 0.0015


def rect_inputs():
    """preds 7 x 8 with ws = 3 (bins overlap in both axes, differently), features 5 x 4; as RI.make_inputs(True): confident regions, so that only some
    windows pass the threshold"""
    g = torch.Generator().manual_seed(97)
    l, h = torch.randn(2, 768, 5, 4, generator=g), torch.randn(2, 9, 768, 5, 4, generator=g)
    preds = torch.randn(2, 1, 7, 8, generator=g) * 2
    preds[0, :, :4, :] = 14.0
    preds[1, :, :, 3:] = -14.0
    return l, h, preds


def test_sparse_refiner_eval_on_a_rectangle():
    """SparseRefiner.eval() with H != W everywhere and H % ws != 0 against oracle.refiner.sparse_refiner_forward on the CPU: mask and coords equal, the
    tolerances of test_sparse_refiner_matches_reference (the same quantities against the same oracle).  The oracle's pooled scores all lie further than
    1e-4 from the threshold, so no rounding can flip the mask."""
    torch.manual_seed(RI.SEED)
    m = RI.perturb_(SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=THRESHOLD)))).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    l, h, preds = rect_inputs()
    ref_out, ref = OR.sparse_refiner_forward(l, h, preds, sd, 3, THRESHOLD)
    scores = F.adaptive_avg_pool2d(ref["entropy"], (3, 3))
    assert float((scores - THRESHOLD).abs().min()) > 1e-4
    nsel = int(ref["mask"].sum())
    assert 0 < nsel < 18 and all(0 < int(mk.sum()) < 9 for mk in ref["mask"])
    assert ref_out.shape == (2, 1, 15, 12) and ref["window_preds"].shape == (nsel, 1, 5, 4)
    m = m.to(DEV)
    with torch.no_grad():
        out, ex, opt = m(l.to(DEV), h.to(DEV), preds.to(DEV))
    assert ex == 0
    assert torch.equal(opt["mask"].cpu(), ref["mask"]) and torch.equal(opt["coords_list"].cpu(), ref["coords_list"])
    assert maxdiff(opt["entropy"].cpu(), ref["entropy"]) < 1e-5
    wp, wref = opt["window_preds"].cpu(), ref["window_preds"]
    assert wp.shape == wref.shape
    within("refiner_fwd:module:window_preds", R.rel_l2(wp, wref), 3.5e-3)          # bf16 projections + bf16 attention probabilities vs the f32 oracle
    assert maxdiff(opt["h_preds"].cpu(), ref["h_preds"]) < 0.05 * wref.abs().max().item()
    assert maxdiff(opt["GE_w"].cpu(), ref["GE_w"]) < 1e-4
    within("refiner_fwd:module:outputs", R.rel_l2(out, ref_out), 5e-4)
