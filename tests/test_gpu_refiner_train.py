"""GPU: training of the CORAL refiner's window branch -- the new kernels against f64 on their own inputs, then d ex_loss / d HRE.CSF.* through the
drop-in module against f64 autograd through the oracle.  References, rounding models, cases and bounds: tests/refiner_train_ref.py (none of them is GPU
output; tests/test_refiner_train_host.py shows that the bounds hide no lost term)."""
import pytest
import torch

from conftest import load_golden, maxdiff, within

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import refiner_train_ref as R  # noqa: E402
from refiner_train_ref import RI  # noqa: E402
from ucod_dpl_amd import native as N, ops  # noqa: E402
from ucod_dpl_amd.engine.config import CfgNode  # noqa: E402
from ucod_dpl_amd.models.UDLR import SparseRefiner  # noqa: E402

DEV = torch.device("cuda", 0)
GUARD_ROWS, CANARY = 4, 1234.0


class Guarded:
    """[rows, cols] of ``dtype`` between GUARD_ROWS canary rows on either side; the payload starts as NaN (an element no store reached shows) in its first
    ``width`` columns and as the canary in the columns behind them (a leading dimension above the width: they must stay)."""

    def __init__(self, rows, cols, dtype, width=None):
        self.rows, self.cols, self.width = rows, cols, cols if width is None else width
        self.buf = torch.full((rows + 2 * GUARD_ROWS, cols), CANARY, dtype=dtype, device=DEV)
        self.payload = self.buf[GUARD_ROWS:GUARD_ROWS + rows]
        self.payload[:, :self.width].fill_(float("nan"))

    def ptr(self):
        return self.payload.data_ptr()

    def intact(self):
        return (bool((self.buf[:GUARD_ROWS] == CANARY).all()) and bool((self.buf[GUARD_ROWS + self.rows:] == CANARY).all())
                and bool((self.payload[:, self.width:] == CANARY).all()))

    def get(self):
        assert self.intact(), "wrote outside its output"
        out = self.payload[:, :self.width]
        assert not bool(torch.isnan(out.float()).any()), "an element was not written"
        return out.clone()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def twice(launch):
    """run ``launch() -> {name: tensor}`` twice; every output bit-identical; -> the first"""
    a, b = launch(), launch()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{k}: two runs differ"
    return a


def small_bound(f32, f64):
    """per tensor: relative L2 <= max(4 x the relative L2 of the same formula in f32 on the CPU against f64, 1e-5); the floor covers another summation
    order over up to M * 49 f32 terms"""
    return max(4.0 * R.rel_l2(f32, f64), 1e-5)


# ================================================================================================ head_dim-96 attention: LSE forward and backward
def run_attention(case):
    B, Nq, Nk, heads, kind = case
    lib, D = N.load(), heads * R.HD
    qs, k, v, do = R.attn_inputs(case)
    ldq = D + 64 if kind == "ldq" else D
    lddq, lddkv = (D + 32, 2 * D + 64) if kind == "ldout" else (D, 2 * D)
    q_d = torch.full((B * Nq, ldq), 7.0, dtype=torch.bfloat16, device=DEV)
    q_d[:, :D] = qs.reshape(B * Nq, D).to(DEV)
    kv_d = torch.cat([k.reshape(B * Nk, D), v.reshape(B * Nk, D)], 1).contiguous().to(DEV)
    do_d = do.reshape(B * Nq, D).contiguous().to(DEV)
    kp, vp = kv_d.data_ptr(), kv_d.data_ptr() + D * 2

    def launch():
        plain, out = Guarded(B * Nq, D, torch.bfloat16), Guarded(B * Nq, D, torch.bfloat16)
        lse, delta = Guarded(B * heads, Nq, torch.float32), Guarded(B * heads, Nq, torch.float32)
        dq, dkv = Guarded(B * Nq, lddq, torch.bfloat16, D), Guarded(B * Nk, lddkv, torch.bfloat16, 2 * D)
        assert lib.ucod_cross_attention96_fwd(N.ptr(q_d), ldq, kp, vp, 2 * D, plain.ptr(), B, Nq, Nk, heads, N.stream()) == 0
        assert lib.ucod_cross_attention96_fwd_lse(N.ptr(q_d), ldq, kp, vp, 2 * D, out.ptr(), lse.ptr(), B, Nq, Nk, heads, N.stream()) == 0
        assert lib.ucod_cross_attention96_bwd(N.ptr(q_d), ldq, kp, vp, 2 * D, out.ptr(), N.ptr(do_d), lse.ptr(), delta.ptr(), dq.ptr(), lddq, dkv.ptr(),
                                              dkv.ptr() + D * 2, lddkv, B, Nq, Nk, heads, N.stream()) == 0
        torch.cuda.synchronize()
        return dict(plain=plain.get(), out=out.get(), lse=lse.get(), delta=delta.get(), dq=dq.get(), dkv=dkv.get())

    return twice(launch)


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_cross_attention96_lse_and_backward(case):
    """ucod_cross_attention96_fwd_lse / ucod_cross_attention96_bwd against f64 per (window, head).  Bounds: dq / dk / dv by R.attn_check (F = 2 x the CPU
    rounding model's own error, per slab and per row); lse by the bound of ucod_attention_fwd_lse's test (tests/test_gpu_vit_train.py:241); `out` with the
    lse pointer given is bit-identical to `out` without it, and meets the bounds of test_cross_attention_head_dim_96."""
    B, Nq, Nk, heads, kind = case
    D = heads * R.HD
    got = run_attention(case)
    ref, model = R.attn_expected(case)
    assert torch.equal(bits(got["out"]), bits(got["plain"]))
    out = got["out"].cpu().double().view(B, Nq, heads, R.HD).transpose(1, 2)
    assert R.rel_l2(out, ref["out"]) < 1e-2 and (kind == "peaked" or maxdiff(out, ref["out"]) < 3e-2)      # (the 3e-2 belongs to the randn * 1.5 scaling)
    lse = got["lse"].cpu().double().view(B, heads, Nq)
    within("attn96:lse_abs_natural", float((lse - ref["lse"]).abs().max()) / R.LOG2E, R.lse_bound(ref["lse"]))
    heads_of = lambda t, n: t.cpu().double().view(B, n, heads, R.HD).transpose(1, 2)  # noqa: E731
    grads = dict(dq=heads_of(got["dq"], Nq), dk=heads_of(got["dkv"][:, :D], Nk), dv=heads_of(got["dkv"][:, D:], Nk))
    R.attn_check("-".join(str(x) for x in case), grads, ref, model, floor=R.zero_floor(case))


def test_cross_attention96_argument_validation():
    lib, st = N.load(), N.stream()
    t = torch.zeros(256, 192, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p, fp = N.ptr(t), N.ptr(f)
    ok = lambda **kw: lib.ucod_cross_attention96_bwd(*[kw.get(n, d) for n, d in (("q", p), ("ldq", 96), ("k", p), ("v", p), ("ldkv", 96), ("out", p),  # noqa: E731
                                                       ("dout", p), ("lse", fp), ("delta", fp), ("dq", p), ("lddq", 96), ("dk", p), ("dv", p), ("lddkv", 96),
                                                       ("B", 1), ("Nq", 8), ("Nk", 8), ("heads", 1))], st)
    assert ok() == 0
    for bad in (dict(q=None), dict(lse=None), dict(delta=None), dict(dv=None), dict(ldq=100), dict(lddq=88), dict(lddkv=100), dict(Nq=0), dict(Nk=-1), dict(heads=0),
                dict(heads=2), dict(dq=p + 2), dict(B=70000)):
        assert ok(**bad) != 0, bad
    assert lib.ucod_cross_attention96_fwd_lse(p, 96, p, p, 96, p, None, 1, 8, 8, 1, st) != 0
    assert lib.ucod_transpose_pad_bf16(p, 2, 8, 8, 8, p, st) != 0 and lib.ucod_transpose_pad_bf16(p, 0, 8, 16, 8, p, st) != 0
    assert lib.ucod_layernorm_param_grad(fp, 0, fp, fp, fp, fp, 1 << 20, 4, 100, 1e-5, st) != 0          # D % 64
    assert lib.ucod_layernorm_param_grad(fp, 0, fp, fp, fp, fp, 8, 4, 64, 1e-5, st) != 0                 # workspace too small
    assert lib.ucod_dwconv7_maskdec_bwd(fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, 16, 1, 3, 3, 64, st) != 0
    assert lib.ucod_window_loss_grad(fp, fp, fp, fp, None, None, fp, 1, 1, 3, 3, 3, st) != 0
    torch.cuda.synchronize()


# ================================================================================================ the transposed operand of a weight-gradient GEMM
@pytest.mark.parametrize("M,cols,ld", [(648, 768, 768), (1, 8, 8), (130, 1536, 1600), (3136, 96, 96)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_transpose_pad_bf16(M, cols, ld, dtype):
    g = torch.Generator().manual_seed(M + cols)
    src = (torch.randn(M, ld, generator=g) * 3).to(dtype)
    src_d = src.to(DEV)
    Mp = ops.pad_rows64(M)
    assert Mp == max(128, 64 * -(-M // 64))

    def launch():
        dst = Guarded(cols, Mp, torch.bfloat16)
        assert N.load().ucod_transpose_pad_bf16(N.ptr(src_d), int(dtype == torch.bfloat16), M, cols, ld, dst.ptr(), N.stream()) == 0
        torch.cuda.synchronize()
        return dict(dst=dst.get())

    dst = twice(launch)["dst"].cpu()
    assert torch.equal(bits(dst[:, :M]), bits(src[:, :cols].to(torch.bfloat16).t()))
    assert bool((bits(dst[:, M:]) == 0).all())                                  # exact (positive) zeros in the pad
    assert torch.equal(bits(ops.transpose_pad_bf16(src_d, cols).cpu()), bits(dst))


# ================================================================================================ the f32 kernels against f64 on random inputs
SHAPES = [(6, 6), (9, 7), (3, 3)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_window_loss_grad(n, H, W):
    B, ws = 2, 3
    g = torch.Generator().manual_seed(10 * n + H)
    x = torch.randn(n, 1, H, W, generator=g) * 2
    ht = torch.rand(B * ws * ws, 1, H, W, generator=g)
    l_up = torch.randn(B, 1, ws * H, ws * W, generator=g) * 2
    flat = torch.randperm(B * ws * ws, generator=g)[:n].sort().values.to(torch.int32)
    iou = torch.rand(n, generator=g)
    up = torch.tensor([0.7])
    l = torch.stack([l_up[int(f) // 9, :, (int(f) % 9 // 3) * H:(int(f) % 9 // 3 + 1) * H, (int(f) % 3) * W:(int(f) % 3 + 1) * W] for f in flat]) > 0
    w = (iou * 1.5).clamp(0, 1)
    t = ht[flat.long()]
    ref, f32 = (R.loss_grad(x, t, l.float(), w, 0.7, dt) for dt in (torch.float64, torch.float32))
    dev = [v.to(DEV) for v in (x, ht, flat, l_up, iou, up)]

    def launch():
        out = Guarded(n, H * W, torch.float32)
        assert N.load().ucod_window_loss_grad(*[N.ptr(v) for v in dev], out.ptr(), n, B, H, W, ws, N.stream()) == 0
        torch.cuda.synchronize()
        return dict(g=out.get())

    got = twice(launch)["g"].cpu().view(n, 1, H, W)
    within("refiner_train:window_loss_grad", R.rel_l2(got, ref), small_bound(f32, ref))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_dwconv7_maskdec_bwd(n, H, W):
    C = R.C
    g = torch.Generator().manual_seed(100 * n + H)
    gr = torch.randn(n, H, W, generator=g) * 1e-3
    x2 = torch.randn(n, H, W, C, generator=g)
    dwT, dwb, w1 = torch.randn(49, C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    names = ("d_dw", "d_dwb", "d_w1", "d_b1", "dx2")
    ref, f32 = (dict(zip(names, R.dwconv_bwd(gr, x2, dwT, dwb, w1, dt))) for dt in (torch.float64, torch.float32))
    dev = [v.contiguous().to(DEV) for v in (gr, x2, dwT, dwb, w1)]
    wsn = min(n * H, 64) * 49 * C

    def launch():
        outs = [Guarded(C, 49, torch.float32), Guarded(1, C, torch.float32), Guarded(1, C, torch.float32), Guarded(1, 1, torch.float32),
                Guarded(n * H * W, C, torch.float32)]
        wsb = torch.full((wsn,), float("nan"), dtype=torch.float32, device=DEV)
        assert N.load().ucod_dwconv7_maskdec_bwd(*[N.ptr(v) for v in dev], *[o.ptr() for o in outs], N.ptr(wsb), wsn * 4, n, H, W, C, N.stream()) == 0
        torch.cuda.synchronize()
        return {k: o.get() for k, o in zip(names, outs)}

    got = twice(launch)
    for k in names:
        within(f"refiner_train:dwconv_bwd:{k}", R.rel_l2(got[k].cpu().reshape(ref[k].shape), ref[k]), small_bound(f32[k], ref[k]))


@pytest.mark.parametrize("rows", [1, 9, 63, 255, 648])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layernorm_param_grad(rows, dtype):
    C = R.C
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    dy = (torch.randn(rows, C, generator=g) * 1e-2).to(dtype)
    names = ("dgamma", "dbeta")
    ref, f32 = (dict(zip(names, R.ln_param_grad(dy, x, R.LN_EPS, dt))) for dt in (torch.float64, torch.float32))
    x_d, dy_d = x.to(DEV), dy.to(DEV)
    wsn = min(128, -(-rows // 64)) * 2 * C

    def launch():
        outs = [Guarded(1, C, torch.float32), Guarded(1, C, torch.float32)]
        wsb = torch.full((wsn,), float("nan"), dtype=torch.float32, device=DEV)
        assert N.load().ucod_layernorm_param_grad(N.ptr(dy_d), N.LNB_DY_BF16 if dtype == torch.bfloat16 else 0, N.ptr(x_d), outs[0].ptr(), outs[1].ptr(),
                                                  N.ptr(wsb), wsn * 4, rows, C, R.LN_EPS, N.stream()) == 0
        torch.cuda.synchronize()
        return {k: o.get() for k, o in zip(names, outs)}

    got = twice(launch)
    for k in names:
        within(f"refiner_train:ln_param_grad:{k}", R.rel_l2(got[k].cpu().reshape(-1), ref[k]), small_bound(f32[k], ref[k]))


# ================================================================================================ the whole branch through the module
def make_module():
    torch.manual_seed(RI.SEED)
    return RI.perturb_(SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015)))).train().to(DEV)


def batch(tag, kind):
    l, h, preds = RI.make_inputs(tag == "partial")
    return l.to(DEV), h.to(DEV), preds.to(DEV), RI.make_h_targets(kind).to(DEV)


def csf_grads(m):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.HRE.CSF.named_parameters()}


def step(m, tag="full", kind="prob", scale=None):
    out, ex, opt = m(*batch(tag, kind))
    (ex if scale is None else scale * ex).backward()
    return out, ex, opt


@pytest.mark.parametrize("tag", R.TAGS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_window_branch_gradients_match_f64_autograd(tag, kind):
    """ex_loss.backward() leaves d ex_loss / d parameter in .grad of the 18 HRE.CSF parameters: per tensor (the q / k / v thirds of in_proj_* apart)
    relative L2 against f64 autograd through the oracle <= 3 x the error of the CPU oracle under bf16 autocast; the key third of in_proj_bias has a zero
    reference, there the norm is bounded by 3 x the norm the autocast run returns.  The grad-mode forward meets the bounds of the no-grad one."""
    g, g9 = load_golden("g9b_refiner_train"), load_golden("g9_refiner")
    m = make_module()
    out, ex, opt = step(m, tag, kind)
    assert ex.requires_grad and ex.dim() == 0 and not out.requires_grad and not opt["window_preds"].requires_grad
    want = float(g[f"{tag}.{kind}.ex_loss"])
    within("refiner_train:ex_loss_rel", abs(float(ex.detach()) - want) / want, 5e-4)
    within("refiner_train:window_preds", R.rel_l2(opt["window_preds"], g9[tag + ".window_preds"]), 3.5e-3)
    assert torch.equal(opt["window_targets"].cpu(), g[f"{tag}.{kind}.window_targets"])
    grads = csf_grads(m)
    assert len(grads) == 18 and all(v is not None and v.shape == p.shape and v.dtype == p.dtype for v, (_, p) in zip(grads.values(), m.HRE.CSF.named_parameters()))
    assert all(p.grad is None for p in m.GE.parameters())
    err, bound = R.branch_error({k: v.cpu() for k, v in grads.items()}, tag, kind), R.branch_bounds(tag, kind)
    for k in err:
        print(f"{tag}.{kind} {k}: {err[k]:.3e} (bound {bound[k]:.3e}, ratio to the autocast error {3 * err[k] / bound[k]:.2f})")
    for k in err:
        within(f"refiner_train:grad:{k}", err[k], bound[k])


def test_window_branch_autograd_contract():
    """Scaling by the upstream scalar, accumulation into .grad, requires_grad=False, two runs bit-identical, and the paths that stay as they were."""
    m = make_module()
    out1, ex1, opt1 = step(m)
    g1 = csf_grads(m)
    m2 = make_module()
    out2, ex2, _ = step(m2)
    g2 = csf_grads(m2)
    assert torch.equal(bits(ex1.detach()), bits(ex2.detach())) and torch.equal(bits(out1), bits(out2))
    for k in g1:
        assert torch.equal(bits(g1[k]), bits(g2[k])), f"{k}: two runs differ"
    step(m)                                                                      # a second backward on a fresh forward accumulates
    for k, v in csf_grads(m).items():
        assert R.rel_l2(v, 2 * g1[k]) < 1e-6, k
    m3 = make_module()
    step(m3, scale=2.0)                                                          # (2 ex_loss).backward(): twice the gradient, within f32 rounding
    for k, v in csf_grads(m3).items():
        assert R.rel_l2(v, 2 * g1[k]) < 1e-6, k
    m4 = make_module()
    frozen = ("attn.attn.out_proj.weight", "attn.norm_kv.bias", "depthwise_conv.weight")
    for k, p in m4.HRE.CSF.named_parameters():
        p.requires_grad_(k not in frozen)
    step(m4)
    for k, v in csf_grads(m4).items():
        assert (v is None) if k in frozen else torch.equal(bits(v), bits(g1[k])), k
    # no HRE.CSF parameter requires grad / no_grad / eval / no window selected / no h_targets: the plain forward, as before
    for p in m4.HRE.CSF.parameters():
        p.requires_grad_(False)
    _, ex, _ = m4(*batch("full", "prob"))
    assert not ex.requires_grad and abs(float(ex) - float(ex1.detach())) < 1e-3 * float(ex1.detach())
    with torch.no_grad():
        out_ng, ex_ng, opt_ng = m(*batch("full", "prob"))
    assert not ex_ng.requires_grad and abs(float(ex_ng) - float(ex1.detach())) < 1e-3 * float(ex1.detach())
    within("refiner_train:window_preds_grad_vs_nograd", R.rel_l2(opt1["window_preds"], opt_ng["window_preds"]), 1e-3)
    l, h, preds, ht = batch("full", "prob")
    _, ex, opt = m(l, h, torch.full_like(preds, 14.0), ht)
    assert ex == 0 and isinstance(ex, int) and "window_targets" not in opt
    with pytest.raises(ValueError):
        m(l, h, preds)
    _, ex, _ = m.eval()(l, h, preds, ht)
    assert ex == 0 and isinstance(ex, int)


def test_window_branch_sgd_descends():
    """Five steps of torch.optim.SGD(lr = R.SGD_LR = 0.5) on the HRE.CSF parameters, on the fixed full.prob batch: ex_loss decreases strictly.  The f64
    reference on the CPU (R.sgd_losses, asserted by test_refiner_train_host.py) gives 0.352857, 0.342116, 0.335993, 0.330636, 0.325683: every step gains
    more than 4.9e-3, fifty times the 16-bit noise on the loss."""
    m = make_module()
    opt = torch.optim.SGD(m.HRE.CSF.parameters(), lr=R.SGD_LR)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        _, ex, _ = step(m)
        losses.append(float(ex.detach()))
        opt.step()
    print("ex_loss over five SGD steps:", losses, "f64:", R.SGD_F64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
