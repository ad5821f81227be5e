"""CPU references for the gradient through the CORAL refiner's `outputs` (models/UDLR.py: _RefinerFunction, SparseRefiner(train_outputs=True);
csrc/refiner_train.hip: ucod_gated_ensemble_bwd, ucod_window_gather).

Test infrastructure only: nothing here is the code under test, and nothing here reads GPU output to set a bound.

* ``ge_bwd`` / ``gather``: the formulas of include/ucod_dpl.h in any dtype, with named faults for the host test.
* ``tau`` / ``kink_pairs``: the kink margin of the fuser's ReLU (derivation below); ``kernel_inputs`` asserts it on every kernel case.
* ``gate_bound``: what a flipped gate can change, for the whole-module tests (where the GPU's own h_preds decides the gates).
* ``autograd_outputs``: oracle.refiner.sparse_refiner_forward + cal_ex_loss under torch autograd on the G9 fixture, for the losses <G, outputs> and
  <G, outputs> + ex_loss -- the construction of refiner_train_ref.autograd_grads, extended to the 4 fuser parameters.
* ``csf_functional``: d (<c, csf(params)> [+ ex_loss]) / d HRE.CSF parameters, in f64 or under bf16 autocast.
* the descent check of the fuser: ``fuser_sgd_losses`` (f64), ``SGD_OUT_LR`` / ``SGD_OUT_F64``.

The kink margin.  The kernel evaluates, in f32,  y = fl(fl(l1 w) + fl(l2 fl(1 - w)))  and  z_k = fl(fl(a_k y) + c_k)  (a fused multiply-add only removes
roundings).  With u = 2^-24 and to first order: each of the two products of y carries at most 2 u relative (its own rounding, and the one of 1 - w), the
sum one more, so |dy| <= 3 u (|l1 w| + |l2 (1 - w)|); a_k y adds u, the last sum u on |a_k y| + |c_k|:
    |dz_k| <= 5 u |a_k| (|l1 w| + |l2 (1 - w)|) + u |c_k|  <=  tau_k := 8 u (|a_k| (|l1 w| + |l2 (1 - w)|) + |c_k|).
Where |z_k| >= tau_k the f32 kernel and the f64 reference agree on m_k = [z_k > 0]; where z_k == 0 exactly because a_k == c_k == 0, tau_k == 0 and both
give 0.  A disagreement would change d a_k, d c_k and dl2 by a whole term, so the kernel cases (inputs fixed by seed, on the CPU) are chosen so that no
pair (pixel, k) has |z_k| < tau_k.
"""
import contextlib
import functools
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import refiner as OR
from oracle.resize import torch_bilinear
import refiner_train_ref as RT
from refiner_train_ref import RI, CSF, rel_l2, split_thirds  # noqa: F401

U = 2.0 ** -24
G_SEED = 29
LOSSES = ("out", "both")
FUSER = ("GE.fuser.0.weight", "GE.fuser.0.bias", "GE.fuser.2.weight", "GE.fuser.2.bias")
GE_OUT = ("dl2", "d_a", "d_c", "d_d", "d_b")
FAULTS = ("no_omw", "no_gate", "ge_gate", "swap_ad", "no_div", "wrong_cell")


# ================================================================================================ the two kernels' formulas
def pre_activation(l1, l2, w, a, c, dtype):
    """(y [B,1,h,w], z [B,64,h,w]) of the fuser's first layer"""
    l1, l2, w, a, c = (v.to(dtype) for v in (l1, l2, w, a, c))
    y = l1 * w + l2 * (1 - w)
    return y, a.view(1, 64, 1, 1) * y + c.view(1, 64, 1, 1)


def ge_bwd(l1, l2, w, a, c, d, G, dtype=torch.float64, fault=None):
    """ucod_gated_ensemble_bwd: {"dl2" [B,1,h,w], "d_a" [64], "d_c" [64], "d_d" [64], "d_b" [1]}.  ``fault``: "no_omw" ((1 - w) dropped from dl2),
    "no_gate" (m_k dropped), "ge_gate" (m_k = [z_k >= 0]), "swap_ad" (a_k in place of d_k in d a_k and d c_k); the gather's faults pass through."""
    assert fault is None or fault in FAULTS
    y, z = pre_activation(l1, l2, w, a, c, dtype)
    w, a, d, G = w.to(dtype), a.to(dtype).view(1, 64, 1, 1), d.to(dtype).view(1, 64, 1, 1), G.to(dtype)
    m = (z >= 0 if fault == "ge_gate" else z > 0).to(dtype)
    if fault == "no_gate":
        m = torch.ones_like(m)
    dl2 = G * (1 if fault == "no_omw" else (1 - w)) * (d * a * m).sum(1, keepdim=True)
    wa = a if fault == "swap_ad" else d                                       # the factor of the two first-layer gradients
    return dict(dl2=dl2, d_a=(G * wa * m * y).sum((0, 2, 3)), d_c=(G * wa * m).sum((0, 2, 3)), d_d=(G * z.clamp_min(0)).sum((0, 2, 3)), d_b=G.sum().reshape(1))


def gather(dl2, coords, img, H, W, ws, dtype=torch.float64, fault=None):
    """ucod_window_gather, the adjoint of oracle.refiner.concat_windows for distinct cells: dwin [n,1,H,W].  ``fault``: "no_div" (the (1 + 1e-6) of the
    forward dropped), "wrong_cell" (the cell's row and column exchanged)."""
    assert fault is None or fault in FAULTS
    dl2 = dl2.to(dtype)
    out = torch.zeros(len(coords), 1, H, W, dtype=dtype)
    for i, ((cy, cx), b) in enumerate(zip(coords.tolist(), img.tolist())):
        if fault == "wrong_cell":
            cy, cx = cx, cy
        out[i, 0] = dl2[b, 0, cy * H:(cy + 1) * H, cx * W:(cx + 1) * W]
    return out if fault == "no_div" else out / (1 + 1e-6)


# ================================================================================================ the kink margin
def tau(l1, l2, w, a, c):
    """tau [B,64,h,w] in f64 (module docstring)"""
    l1, l2, w, a, c = (v.double() for v in (l1, l2, w, a, c))
    mag = (l1 * w).abs() + (l2 * (1 - w)).abs()
    return 8 * U * (a.abs().view(1, 64, 1, 1) * mag + c.abs().view(1, 64, 1, 1))


def kink_pairs(l1, l2, w, a, c, factor=1.0):
    """bool [B,64,h,w]: the pairs (pixel, k) whose gate an f32 evaluation may decide differently, |z_k| < factor * tau_k"""
    _, z = pre_activation(l1, l2, w, a, c, torch.float64)
    return z.abs() < factor * tau(l1, l2, w, a, c)


def gate_bound(l1, l2, w, a, c, d, G, factor=2.0):
    """{output: absolute L2 widening}: over the pairs with |z_k| < factor tau_k, the sizes of the terms a flipped gate changes -- |G d_k y| for d a_k,
    |G d_k| for d c_k, |G (1 - w) d_k a_k| for dl2 (per pixel; returned as the L2 norm over pixels); d d_k = sum G max(z_k, 0) is continuous in z, a flip
    moves it by at most |G| factor tau_k; the bias does not see the gates.  Also "pairs": how many."""
    y, z = pre_activation(l1, l2, w, a, c, torch.float64)
    t = tau(l1, l2, w, a, c)
    near = (z.abs() < factor * t).double()
    Gd, wd, av, dv = G.double(), w.double(), a.double().view(1, 64, 1, 1), d.double().view(1, 64, 1, 1)
    return dict(pairs=int(near.sum()), d_a=float((near * (Gd * dv * y).abs()).sum((0, 2, 3)).norm()), d_c=float((near * (Gd * dv).abs()).sum((0, 2, 3)).norm()),
                d_d=float((near * Gd.abs() * factor * t).sum((0, 2, 3)).norm()), dl2=float((near * (Gd * (1 - wd) * dv * av).abs()).sum(1).norm()), d_b=0.0)


# ================================================================================================ kernel cases (inputs fixed by seed, on the CPU)
# (B, h, w, fuser).  Sizes: a single partial workgroup; the G9 size (two workgroups per image, one partial); non-square, B = 3; exactly one full tile;
# 16 workgroups per image, 48 partials.  fuser "mixed": randn weights, d_k = 0 for k % 8 == 3, channel 5 dead with a_k = c_k = 0 (z_k == 0 exactly: the
# subgradient at 0 is 0); "onesided": a_k > 0 and c_k < 0 for every k, so that every pixel with y <= 0 has all z_k <= 0 and dl2 exactly 0 there.
GE_CASES = ((1, 6, 6, "mixed"), (2, 18, 18, "mixed"), (3, 12, 21, "mixed"), (1, 16, 16, "mixed"), (3, 63, 63, "mixed"), (2, 18, 18, "onesided"))
GE_SEEDS = {c: 0 for c in GE_CASES}          # the first seed offset at which no pair is inside the kink margin (test_refiner_outputs_host.py asserts it)


def _ge_inputs(case, offset):
    B, h, w, fuser = case
    g = torch.Generator().manual_seed(2900 + 1000 * offset + 100 * B + 10 * h + w + (7 if fuser == "onesided" else 0))
    l1, l2 = torch.randn(B, 1, h, w, generator=g) * 2, torch.randn(B, 1, h, w, generator=g) * 2
    wt = torch.rand(B, 1, h, w, generator=g) * 0.9 + 0.05
    a, c, d = torch.randn(64, generator=g) * 0.5, torch.randn(64, generator=g) * 0.3, torch.randn(64, generator=g) * 0.5
    G = torch.randn(B, 1, h, w, generator=g)
    if fuser == "onesided":
        a, c = a.abs() + 0.05, -c.abs() - 0.01
    else:
        a[5], c[5] = 0.0, 0.0
    d[3::8] = 0.0
    return dict(l1=l1, l2=l2, w=wt, a=a, c=c, d=d, G=G)


@functools.lru_cache(maxsize=None)
def kernel_inputs(case):
    """the inputs of a kernel case; asserts the kink margin: NO pair (pixel, k) has |z_k| < tau_k"""
    x = _ge_inputs(case, GE_SEEDS[case])
    n = int(kink_pairs(x["l1"], x["l2"], x["w"], x["a"], x["c"]).sum())
    assert n == 0, (case, n, "pairs inside the kink margin: pick another seed offset")
    return x


@functools.lru_cache(maxsize=None)
def kernel_expected(case):
    """(f64 reference, the same formulas in f32) of a kernel case: computed once, shared, never modified"""
    x = kernel_inputs(case)
    return ge_bwd(**x, dtype=torch.float64), ge_bwd(**x, dtype=torch.float32)


# (ws, H, W, B, the selected cells as (image, cy, cx) in b-major raster order): ws 3 and 2, an image without a window, non-square windows, n = 0
GATHER_CASES = ((3, 6, 6, 2, ((0, 0, 0), (0, 1, 2), (0, 2, 1), (1, 0, 1), (1, 2, 2))), (2, 5, 7, 3, ((0, 0, 1), (0, 1, 0), (2, 1, 1))),
                (3, 4, 9, 2, ((1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 2, 0), (1, 2, 1), (1, 2, 2))), (3, 6, 6, 2, ()),
                (2, 17, 16, 1, ((0, 0, 0), (0, 1, 1))))


def gather_inputs(case):
    ws, H, W, B, cells = case
    g = torch.Generator().manual_seed(31 * ws + H + W + len(cells))
    dl2 = torch.randn(B, 1, ws * H, ws * W, generator=g)
    g0 = torch.randn(len(cells), 1, H, W, generator=g)
    coords = torch.tensor([[cy, cx] for _, cy, cx in cells], dtype=torch.int64).reshape(-1, 2)
    img = torch.tensor([b for b, _, _ in cells], dtype=torch.int64)
    return dl2, g0, coords, img


# ================================================================================================ the G9 fixture under autograd, through `outputs`
def cotangent():
    return torch.randn(2, 1, 18, 18, generator=torch.Generator().manual_seed(G_SEED))


@contextlib.contextmanager
def _all_f64(on):
    """the oracle builds its scatter buffers with torch.zeros(...) in the default dtype: float64 as the default keeps a float64 run float64 throughout
    (and refiner_train_ref._UnfoldF64 does the same for the thresholded label of cal_ex_loss)"""
    if not on:
        yield
        return
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with mock.patch.object(OR, "F", RT._UnfoldF64()):
            yield
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def autograd_outputs(tag, kind="prob", mode="f64"):
    """{"outputs", "ex_loss", "window_preds", "h_preds", "GE_w", "z" (the fuser's pre-activations [B,64,h,w]), "mask_ok",
    "out" / "both": {"d_window_preds", "grads": {name: gradient}}} for the losses <G, outputs> and <G, outputs> + ex_loss; names are the 18 HRE.CSF.* and
    the 4 GE.fuser.* state-dict keys.  mode "f64": everything in float64; "f32": the oracle as it is, in float32."""
    fx = RT.fixture(tag, kind)
    dt = torch.float64 if mode == "f64" else torch.float32
    names = fx["names"] + list(FUSER)
    sd = {k: v.to(dt).clone().requires_grad_(k in names) for k, v in fx["sd"].items()}
    G = cotangent().to(dt)
    with _all_f64(mode == "f64"):
        outputs, opt = OR.sparse_refiner_forward(fx["l"].to(dt), fx["h"].to(dt), fx["preds"].to(dt), sd)
        ex, _, _ = OR.cal_ex_loss(fx["preds"].to(dt), opt["window_preds"], opt["mask"], fx["ht"].to(dt), 3)
        res = dict(outputs=outputs.detach(), ex_loss=float(ex.detach()), window_preds=opt["window_preds"].detach(), h_preds=opt["h_preds"].detach(),
                   GE_w=opt["GE_w"].detach(), mask_ok=bool(torch.equal(opt["mask"], fx["mask"])))
        y = torch_bilinear(fx["preds"].to(dt), 18, 18) * opt["GE_w"] + opt["h_preds"].detach() * (1 - opt["GE_w"])
        res["z"] = F.conv2d(y, sd[FUSER[0]].detach(), sd[FUSER[1]].detach())
        for which in LOSSES:
            loss = (outputs * G).sum() + (ex if which == "both" else 0)
            got = torch.autograd.grad(loss, [sd[k] for k in names] + [opt["window_preds"]], retain_graph=True)
            res[which] = dict(d_window_preds=got[-1].detach().double(), grads={k: g.detach().double() for k, g in zip(names, got[:-1])})
    return res


def csf_functional(tag, kind, c, with_loss, mode="f64"):
    """{HRE.CSF name (without the prefix): d (<c, csf(params)> [+ ex_loss]) / d parameter}: the functional whose gradient the CSF chain returns when the
    window cotangent of `outputs` is ``c`` [n,1,H,W] (a constant).  mode "f64" or "autocast" (f32 parameters under bf16 autocast, the project's yardstick)."""
    fx = RT.fixture(tag, kind)
    dt = torch.float64 if mode == "f64" else torch.float32
    sd = {k: v.to(dt).clone().requires_grad_(k.startswith(CSF)) for k, v in fx["sd"].items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=(mode == "autocast")), _all_f64(mode == "f64"):
        wp = OR.csf(fx["l_sel"].to(dt), fx["h_sel"].to(dt), sd)
        loss = (wp.to(dt) * c.to(dt)).sum()
        if with_loss:
            loss = loss + OR.cal_ex_loss(fx["preds"].to(dt), wp.to(dt), fx["mask"], fx["ht"].to(dt), 3)[0]
    grads = torch.autograd.grad(loss, [sd[k] for k in fx["names"]])
    return {k[len(CSF):]: g.detach().double() for k, g in zip(fx["names"], grads)}


def csf_errors(got, tag, kind, c, with_loss):
    """({tensor: error of ``got``}, {tensor: bound}): relative L2 against f64 autograd of the functional, bound 3 x the error of the same functional under
    CPU bf16 autocast; for the zero-reference tensor (the key third of in_proj_bias) the norm, against 3 x the norm the autocast run returns."""
    ref, ac = split_thirds(csf_functional(tag, kind, c, with_loss)), split_thirds(csf_functional(tag, kind, c, with_loss, "autocast"))
    got = split_thirds(got)
    zero = RT.ZERO_REFERENCE
    err = {k: (float(got[k].double().norm()) if k == zero else rel_l2(got[k], ref[k])) for k in ref}
    bound = {k: 3.0 * (float(ac[k].norm()) if k == zero else rel_l2(ac[k], ref[k])) for k in ref}
    return err, bound


def window_cells(tag, kind="prob"):
    """(coords [n,2], image index [n]) of the selected windows, in the module's order"""
    fx = RT.fixture(tag, kind)
    _, mask, coords, counts = OR.entropy_select(fx["preds"], 3, 0.0015)
    return coords, torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))


# ================================================================================================ descent check of the fuser (f64, CPU)
def descent_target():
    """T [2,1,18,18]: the binarised window targets of make_h_targets("prob") placed at their cells"""
    ht = (RI.make_h_targets("prob") > 0.5).float()
    T = torch.zeros(2, 1, 18, 18)
    for j in range(18):
        b, cy, cx = j // 9, (j % 9) // 3, j % 3
        T[b, 0, cy * 6:(cy + 1) * 6, cx * 6:(cx + 1) * 6] = ht[j, 0]
    return T


# Scanned in f64 (fuser_sgd_losses): 0.01 ... 0.5 all decrease monotonically; at 0.1 the smallest of the four gains is 5.2e-4, at 0.5 the last ones
# shrink to 1e-5.  The f32 noise on the loss (a mean of 648 f32 BCE terms near 0.69, each a few ulp) is below 5e-7: every gain exceeds it 1000 times.
SGD_OUT_LR = 0.1
SGD_OUT_F64 = (0.699093, 0.696591, 0.695110, 0.694235, 0.693716)      # fuser_sgd_losses(SGD_OUT_LR)
SGD_OUT_NOISE, SGD_OUT_FACTOR = 5e-7, 1000.0


def fuser_sgd_losses(lr, steps=5, tag="full"):
    """BCEWithLogits(outputs, T) at the start of each of ``steps`` SGD steps on the 4 GE.fuser parameters in float64, h_preds held fixed (HRE.CSF frozen)."""
    fx, ref = RT.fixture(tag, "prob"), autograd_outputs(tag)
    sd = {k: v.double().clone().requires_grad_(k in FUSER) for k, v in fx["sd"].items()}
    T = descent_target().double()
    out = []
    with _all_f64(True):
        for _ in range(steps):
            o, _ = OR.gated_ensembler(fx["preds"].double(), ref["h_preds"], sd)
            loss = F.binary_cross_entropy_with_logits(o, T)
            out.append(float(loss.detach()))
            grads = torch.autograd.grad(loss, [sd[k] for k in FUSER])
            with torch.no_grad():
                for k, g in zip(FUSER, grads):
                    sd[k] -= lr * g
    return out
