"""CPU references for the training of the CORAL refiner's window branch (models/UDLR.py: _WindowBranchFunction; csrc/attention96_bwd.hip,
csrc/refiner_train.hip, the LSE form of attn_cross96_kernel).

Test infrastructure only: nothing here is the code under test, and nothing here reads GPU output to set a bound.

* ``autograd_grads``: oracle.refiner.csf + oracle.refiner.cal_ex_loss under torch autograd on the G9 fixture, in float64 (the reference) or in f32 under
  ``torch.autocast("cpu", dtype=torch.bfloat16)`` (the yardstick of the project's "3 x the reference under 16-bit autocast" rule).
* ``chain``: a hand-written restatement of the backward the kernels implement (token-major, the formulas of include/ucod_dpl.h), in any dtype, with
  named faults for the host test.
* ``loss_grad`` / ``dwconv_bwd`` / ``ln_param_grad``: the small kernels' formulas on their own inputs, in any dtype.
* the head_dim-96 attention: f64 reference, rounding model, cases and checker -- the idiom of tests/attn_bwd_ref.py restated for separate Nq / Nk.
"""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

from conftest import within

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import refiner_init as RI  # noqa: E402
from oracle import refiner as OR  # noqa: E402

C = 768
HEADS = 8
HD = 96
LN_EPS = 1e-5
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
C_Q = HD ** -0.5 * LOG2E
CSF = "HRE.CSF."
TAGS, KINDS = ("full", "partial"), ("prob", "logit")


# ================================================================================================ the G9 fixture under autograd
@functools.lru_cache(maxsize=None)
def fixture(tag, kind):
    """The module of G9 (seeded default init + perturb_), its inputs and targets, and the windows the selector takes: everything on the CPU, f32."""
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.models.UDLR import SparseRefiner
    torch.manual_seed(RI.SEED)
    m = RI.perturb_(SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015))))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    l, h, preds = RI.make_inputs(tag == "partial")
    ht = RI.make_h_targets(kind)
    _, mask, _, counts = OR.entropy_select(preds, 3, 0.0015)
    sel = mask.flatten()
    return dict(sd=sd, l=l, h=h, preds=preds, ht=ht, mask=mask, h_sel=h.flatten(0, 1)[sel], l_sel=torch.repeat_interleave(l, torch.tensor(counts), dim=0),
                names=[k for k in sd if k.startswith(CSF)])


class _UnfoldF64:
    """torch.nn.functional with ``unfold`` taking its input to float64.  cal_ex_loss builds the thresholded first-stage label l with ``.float()``, and
    ATen's BCEWithLogits then evaluates the whole l term in f32 (in place on the f32 ``1 - target``): 1e-8 relative on the loss and on every gradient of
    an otherwise float64 run.  With l (values 0 / 1) carried in float64 the same oracle code is float64 throughout."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def unfold(x, *args, **kwargs):
        return F.unfold(x.double(), *args, **kwargs)


@functools.lru_cache(maxsize=None)
def autograd_grads(tag, kind, mode="f64"):
    """{"loss", "w" (the IoU weights), "window_preds", "grads": {name: d loss / d HRE.CSF parameter}}.  mode "f64": everything in float64 (see
    _UnfoldF64); "autocast": f32 parameters under torch.autocast("cpu", dtype=torch.bfloat16), the oracle untouched."""
    import contextlib
    from unittest import mock
    fx = fixture(tag, kind)
    dt = torch.float64 if mode == "f64" else torch.float32
    sd = {k: v.to(dt).clone().requires_grad_(k.startswith(CSF)) for k, v in fx["sd"].items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=(mode == "autocast")), \
            (mock.patch.object(OR, "F", _UnfoldF64()) if mode == "f64" else contextlib.nullcontext()):
        wp = OR.csf(fx["l_sel"].to(dt), fx["h_sel"].to(dt), sd)
        loss, _, w = OR.cal_ex_loss(fx["preds"].to(dt), wp.to(dt), fx["mask"], fx["ht"].to(dt), 3)
    grads = torch.autograd.grad(loss, [sd[k] for k in fx["names"]])
    return dict(loss=float(loss.detach()), w=w.detach(), window_preds=wp.detach(), grads={k[len(CSF):]: g.detach().double() for k, g in zip(fx["names"], grads)})


def split_thirds(grads):
    """the q / k / v thirds of in_proj_weight and in_proj_bias as tensors of their own"""
    out = {}
    for k, g in grads.items():
        if "in_proj" in k:
            for i, t in enumerate("qkv"):
                out[f"{k}.{t}"] = g[i * C:(i + 1) * C]
        else:
            out[k] = g
    return out


ZERO_REFERENCE = "attn.attn.in_proj_bias.k"          # a shift of every key cancels in the softmax: the exact gradient is 0


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ================================================================================================ the small kernels' formulas
def loss_constants(fx):
    """(w [n], l [n,1,h,w], t [n,1,h,w]) of cal_ex_loss (UDLR.py:62-75): none of them carries gradient"""
    preds, mask, ht = fx["preds"], fx["mask"], fx["ht"]
    h, w = ht.shape[-2:]
    l = F.interpolate(preds, size=(h * 3, w * 3), mode="bilinear").sigmoid() > 0.5
    l = F.unfold(l.float(), kernel_size=(h, w), stride=(h, w)).reshape(-1, 1, h, w, 9).permute(0, 4, 1, 2, 3).flatten(0, 1)[mask.flatten()]
    t = ht[mask.flatten()]
    return (OR.binary_iou(t, l) * 1.5).clamp(0, 1), l, t


def loss_grad(x, t, l, w, up, dtype):
    """ucod_window_loss_grad: g = up / (2 n H W) (sigmoid(x) - (w t + (1 - w) l)), written as the derivative of the two BCE terms cal_ex_loss adds
    (w + fl32(1 - w) is 1 only to f32 rounding, and autograd sees the two terms)."""
    x, t, l = (v.to(dtype) for v in (x, t, l))
    n, _, H, W = x.shape
    w, omw = w.view(-1, 1, 1, 1).to(dtype), (1 - w).view(-1, 1, 1, 1).to(dtype)       # 1 - w in w's own precision (f32), as cal_ex_loss forms it
    return (w * (torch.sigmoid(x) - t) + omw * (torch.sigmoid(x) - l)) * (up / (2.0 * n * H * W))


def dwconv_bwd(g, x2, dwT, dwb, w1, dtype, drop_tap=None, drop_w1=False):
    """ucod_dwconv7_maskdec_bwd: g [n,H,W], x2 [n,H,W,C], dwT [49,C] -> (d_dw [C,49], d_dwb [C], d_w1 [C], d_b1 [1], dx2 [n,H,W,C])."""
    g, x2, dwT, dwb, w1 = (v.to(dtype) for v in (g, x2, dwT, dwb, w1))
    n, H, W, Cc = x2.shape
    xp = F.pad(x2, (0, 0, 3, 3, 3, 3))
    gp = F.pad(g, (3, 3, 3, 3))
    S = torch.zeros(49, Cc, dtype=dtype)
    dx = torch.zeros_like(x2)
    for ky in range(7):
        for kx in range(7):
            tap = ky * 7 + kx
            if tap == drop_tap:
                continue
            S[tap] = torch.einsum("nhw,nhwc->c", g, xp[:, ky:ky + H, kx:kx + W])
            dx += gp[:, 6 - ky:6 - ky + H, 6 - kx:6 - kx + W].unsqueeze(-1) * dwT[tap]
    G = g.sum()
    d_dw = (S if drop_w1 else w1 * S).t().contiguous()
    return d_dw, w1 * G, dwb * G + (dwT * S).sum(0), G.reshape(1), dx * w1


def ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd, rstd


def ln_param_grad(dy, x, eps, dtype):
    """ucod_layernorm_param_grad: (dgamma, dbeta)"""
    dy, x = dy.to(dtype), x.to(dtype)
    xhat, _ = ln_stats(x, eps)
    return (dy * xhat).sum(0), dy.sum(0)


def ln_input_grad(dy, x, gamma, eps):
    xhat, rstd = ln_stats(x, eps)
    dyg = dy * gamma
    return rstd * (dyg - dyg.mean(-1, keepdim=True) - xhat * (dyg * xhat).mean(-1, keepdim=True))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ================================================================================================ the hand-written chain
FAULTS = ("delta", "ln2", "scale", "resid", "no_l", "tap", "w1", "window")


def chain(tag, kind, dtype=torch.float64, fault=None):
    """{"loss", "grads"}: forward and backward of the window branch as the kernels form it -- token-major rows, M = n H W -- in ``dtype``.
    ``fault``: "delta" (delta dropped from dS), "ln2" / "scale" (the factor of dK / dQ dropped), "resid" (the residual cotangent not added in front of
    norm_mlp), "no_l" (the (1 - w) l term of the loss gradient dropped), "tap" (one conv tap dropped), "w1" (w1 dropped from d dw), "window" (the rows
    of window 0 dropped from the fc2 weight gradient)."""
    assert fault is None or fault in FAULTS
    fx = fixture(tag, kind)
    sd = {k[len(CSF):]: v.to(dtype) for k, v in fx["sd"].items() if k.startswith(CSF)}
    n, _, H, W = fx["h_sel"].shape
    HW, M = H * W, n * H * W
    q_tok = fx["h_sel"].to(dtype).flatten(2, 3).permute(0, 2, 1).reshape(M, C)
    c_tok = fx["l_sel"].to(dtype).flatten(2, 3).permute(0, 2, 1).reshape(M, C)
    w, l, t = loss_constants(fx)
    # ---- forward (CSF.py:38-43, mlp.py:134-148)
    ln = lambda x, p: ln_stats(x, LN_EPS)[0] * sd[p + ".weight"] + sd[p + ".bias"]  # noqa: E731
    qn, cn = ln(q_tok, "attn.norm_q"), ln(c_tok, "attn.norm_kv")
    Wi, bi = sd["attn.attn.in_proj_weight"], sd["attn.attn.in_proj_bias"]
    Q = qn @ Wi[:C].t() + bi[:C]
    K = cn @ Wi[C:2 * C].t() + bi[C:2 * C]
    V = cn @ Wi[2 * C:].t() + bi[2 * C:]
    hv = lambda x: x.view(n, HW, HEADS, HD).transpose(1, 2)                        # noqa: E731  [n, heads, HW, 96]
    unhv = lambda x: x.transpose(1, 2).reshape(M, C)                               # noqa: E731
    Qs, Kh, Vh = hv(Q) * C_Q, hv(K), hv(V)                                         # Q' = Q 96^-0.5 log2 e
    S = Qs @ Kh.transpose(2, 3)
    L = torch.log2(torch.exp2(S - S.amax(-1, keepdim=True)).sum(-1, keepdim=True)) + S.amax(-1, keepdim=True)
    P = torch.exp2(S - L)
    O = P @ Vh
    att = unhv(O)
    Wo, bo = sd["attn.attn.out_proj.weight"], sd["attn.attn.out_proj.bias"]
    x = q_tok + att @ Wo.t() + bo
    hn = ln(x, "attn.norm_mlp")
    W1, b1, W2, b2 = sd["attn.mlp.0.weight"], sd["attn.mlp.0.bias"], sd["attn.mlp.2.weight"], sd["attn.mlp.2.bias"]
    pre = hn @ W1.t() + b1
    gact = 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2.0)))
    x2 = x + gact @ W2.t() + b2
    dw = sd["depthwise_conv.weight"].reshape(C, 49)
    dwT, dwb, mw, mb = dw.t().contiguous(), sd["depthwise_conv.bias"], sd["mask_dec.weight"].reshape(C), sd["mask_dec.bias"]
    xp = F.pad(x2.view(n, H, W, C), (0, 0, 3, 3, 3, 3))
    z = dwb + sum(dwT[ky * 7 + kx] * xp[:, ky:ky + H, kx:kx + W] for ky in range(7) for kx in range(7))
    win = (mb + (z * mw).sum(-1)).view(n, 1, H, W)
    wv, lt, tt = w.to(dtype).view(-1, 1, 1, 1), l.to(dtype), t.to(dtype)
    sp = win.clamp_min(0) + torch.log1p(torch.exp(-win.abs()))
    loss = (wv * (sp - win * tt) + (1 - w).view(-1, 1, 1, 1).to(dtype) * (sp - win * lt)).mean() / 2
    # ---- backward
    g = loss_grad(win, tt, lt, w, 1.0, dtype)
    if fault == "no_l":                                                             # keep w t, lose (1 - w) l
        g = (torch.sigmoid(win) - wv * tt) / (2.0 * M)
    d_dw, d_dwb, d_mw, d_mb, dx2 = dwconv_bwd(g.view(n, H, W), x2.view(n, H, W, C), dwT, dwb, mw, dtype, drop_tap=10 if fault == "tap" else None,
                                             drop_w1=fault == "w1")
    dx2 = dx2.reshape(M, C)
    G = {}
    G["depthwise_conv.weight"], G["depthwise_conv.bias"] = d_dw.view(C, 1, 7, 7), d_dwb
    G["mask_dec.weight"], G["mask_dec.bias"] = d_mw.view(1, C, 1, 1), d_mb
    rows = slice(HW, None) if fault == "window" else slice(None)
    G["attn.mlp.2.bias"], G["attn.mlp.2.weight"] = dx2.sum(0), dx2[rows].t() @ gact[rows]
    dpre = (dx2 @ W2) * gelu_grad(pre)
    G["attn.mlp.0.bias"], G["attn.mlp.0.weight"] = dpre.sum(0), dpre.t() @ hn
    dhn = dpre @ W1
    G["attn.norm_mlp.weight"], G["attn.norm_mlp.bias"] = ln_param_grad(dhn, x, LN_EPS, dtype)
    dx = ln_input_grad(dhn, x, sd["attn.norm_mlp.weight"], LN_EPS) + (0 if fault == "resid" else dx2)
    G["attn.attn.out_proj.bias"], G["attn.attn.out_proj.weight"] = dx.sum(0), dx.t() @ att
    dO = hv(dx @ Wo)
    dP = dO @ Vh.transpose(2, 3)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - (0 if fault == "delta" else delta))
    dQ = unhv((1.0 if fault == "scale" else HD ** -0.5) * (dS @ Kh))
    dK = unhv((1.0 if fault == "ln2" else LN2) * (dS.transpose(2, 3) @ Qs))
    dV = unhv(P.transpose(2, 3) @ dO)
    G["attn.attn.in_proj_weight"] = torch.cat([dQ.t() @ qn, dK.t() @ cn, dV.t() @ cn])
    G["attn.attn.in_proj_bias"] = torch.cat([dQ.sum(0), dK.sum(0), dV.sum(0)])
    G["attn.norm_q.weight"], G["attn.norm_q.bias"] = ln_param_grad(dQ @ Wi[:C], q_tok, LN_EPS, dtype)
    G["attn.norm_kv.weight"], G["attn.norm_kv.bias"] = ln_param_grad(dK @ Wi[C:2 * C] + dV @ Wi[2 * C:], c_tok, LN_EPS, dtype)
    return dict(loss=float(loss), grads={k: v.double() for k, v in G.items()})


@functools.lru_cache(maxsize=None)
def branch_bounds(tag, kind):
    """{tensor: bound} of the whole-branch GPU test: 3 x the relative L2 error, against the f64 autograd gradient, of the same tensor from the CPU oracle
    under bf16 autocast; for the tensor with a zero reference (the key third of in_proj_bias) 3 x the NORM of what the autocast run returns there."""
    ref, ac = split_thirds(autograd_grads(tag, kind)["grads"]), split_thirds(autograd_grads(tag, kind, "autocast")["grads"])
    return {k: 3.0 * (float(ac[k].norm()) if k == ZERO_REFERENCE else rel_l2(ac[k], ref[k])) for k in ref}


def branch_error(got, tag, kind):
    """{tensor: the quantity branch_bounds bounds} of a gradient dict ``got``"""
    ref, got = split_thirds(autograd_grads(tag, kind)["grads"]), split_thirds(got)
    return {k: (float(got[k].double().norm()) if k == ZERO_REFERENCE else rel_l2(got[k], ref[k])) for k in ref}


# ================================================================================================ descent check (f64, CPU)
SGD_LR = 0.5                                                           # scanned in f64: 0.5 and 1.0 decrease monotonically, 2.0 diverges; 0.5 has the margin
SGD_F64 = (0.352857, 0.342116, 0.335993, 0.330636, 0.325683)           # sgd_losses(SGD_LR): every step gains more than 4.9e-3


def sgd_losses(lr, steps=5, tag="full", kind="prob"):
    """ex_loss at the start of each of ``steps`` SGD steps on the HRE.CSF parameters in float64, the selected windows and loss constants held fixed (the
    batch is fixed, and the first stage is frozen)."""
    fx = fixture(tag, kind)
    sd = {k: v.double().clone().requires_grad_(k.startswith(CSF)) for k, v in fx["sd"].items()}
    out = []
    for _ in range(steps):
        loss, _, _ = OR.cal_ex_loss(fx["preds"].double(), OR.csf(fx["l_sel"].double(), fx["h_sel"].double(), sd), fx["mask"], fx["ht"].double(), 3)
        out.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, [sd[k] for k in fx["names"]])
        with torch.no_grad():
            for k, g in zip(fx["names"], grads):
                sd[k] -= lr * g
    return out


# ================================================================================================ head_dim-96 attention: tiles, cases, inputs
WT = 128                # rows (queries or keys) owned by one workgroup: 4 waves x 32      (attention96_bwd.hip: WT; attention.hip: QT)
ST = 64                 # rows per streamed tile                                            (attention96_bwd.hip: ST; attention.hip: KT)
WAVE_ROWS = 32          # rows owned by one wave
DEFER_THR = 8.0         # attention.hip: DEFER_THR
F_MODEL = 2.0           # kernel error / model error, both against the f64 reference (tests/attn_bwd_ref.py::check)
GRADS = ("dq", "dk", "dv")

# (B, Nq, Nk, heads, kind).  The dQ kernel owns queries and streams keys, the dK/dV kernel owns keys and streams queries, so Nq and Nk both have to reach
# every edge of a wave (32), a streamed tile (64) and a workgroup (128): test_refiner_train_host.py asserts it from the constants above.
ATTN_CASES = (
    (1, 36, 36, 8, "randn"), (2, 200, 77, 2, "randn"), (1, 1, 1, 1, "randn"), (1, 31, 65, 1, "randn"), (1, 32, 64, 1, "randn"), (1, 33, 63, 1, "randn"),
    (1, 129, 128, 2, "randn"), (2, 64, 129, 8, "randn"), (1, 96, 3136, 1, "randn"),
    (1, 63, 127, 1, "randn"), (1, 65, 31, 1, "randn"), (1, 127, 32, 1, "randn"), (1, 128, 33, 1, "randn"),      # the edges the list above leaves out
    (2, 70, 45, 2, "peaked"),            # q x 4: peaked rows, so that lse matters
    (2, 70, 45, 2, "ldq"),               # q rows inside a wider buffer (ldq > D)
    (2, 70, 45, 2, "ldout"),             # dq / [dk | dv] leading dimensions above their widths
)


def heads_of(t, heads):
    B, n, D = t.shape
    return t.double().view(B, n, heads, HD).transpose(1, 2)


def bf16_round(x):
    return x.to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def attn_inputs(case):
    """(qs, k, v, do): qs [B, Nq, D] bf16 = bf16(bf16(q) * C_Q) as the q projection's epilogue leaves it, k / v [B, Nk, D], do [B, Nq, D]; the randn * 1.5
    scaling of test_cross_attention_head_dim_96."""
    B, Nq, Nk, heads, kind = case
    D = heads * HD
    g = torch.Generator().manual_seed(1000 * Nq + Nk + B)
    q = torch.randn(B, Nq, D, generator=g) * 1.5 * (4.0 if kind == "peaked" else 1.0)
    k = torch.randn(B, Nk, D, generator=g) * 1.5
    v = torch.randn(B, Nk, D, generator=g) * 1.5
    do = torch.randn(B, Nq, D, generator=g)
    bf = lambda t: t.to(torch.bfloat16)                                     # noqa: E731
    return bf(bf(q).float() * C_Q), bf(k), bf(v), bf(do)


def forward_running_max(S):
    """m_run of attn_cross96_kernel when each probability is rounded: the maximum of the row's first 32 keys, then per 32-key block raised to the block's
    maximum for all 32 queries of a wave when ANY of them has a score more than DEFER_THR above its own m_run.  [B,h,Nq,Nk] -> [B,h,Nq,blocks]."""
    B, H, Nq, Nk = S.shape
    pad = -Nq % WAVE_ROWS
    m, per_block = None, []
    for k0 in range(0, Nk, WAVE_ROWS):
        top = S[..., k0:k0 + WAVE_ROWS].amax(-1)
        if m is None:
            m = top
        else:
            over = F.pad(top - m > DEFER_THR, (0, pad))
            fire = over.view(B, H, -1, WAVE_ROWS).any(-1, keepdim=True).expand(-1, -1, -1, WAVE_ROWS).reshape(B, H, Nq + pad)[..., :Nq]
            m = torch.where(fire, torch.maximum(m, top), m)
        per_block.append(m)
    return torch.stack(per_block, -1)


def attn_backward(qs, k, v, do, heads, rnd):
    """The closed formulas, every sum in f64, ``rnd`` at the points the kernel sources document.  The forward (attn_cross96_kernel) rounds its
    unnormalised probabilities 2^(S - m_run) in front of BOTH the P V product and the denominator (which it forms on the matrix pipe from the rounded
    values), so `out` = sum rnd(p) v / sum rnd(p) and lse = m_run + log2 sum rnd(p); the backward takes that lse, rounds `out` (stored bf16) in delta,
    forms dS from the f32 P, rounds P and dS separately in front of their products, and rounds dq / dk / dv once after scaling."""
    Q, K, V, dO = (heads_of(t, heads) for t in (qs, k, v, do))
    S = Q @ K.transpose(2, 3)
    mb = forward_running_max(S)
    m = mb.repeat_interleave(WAVE_ROWS, -1)[..., :S.shape[-1]]                 # per key: the m_run its probability was rounded under
    m_fin = mb[..., -1:]
    pr = rnd(torch.exp2(S - m)) * torch.exp2(m - m_fin)
    den = pr.sum(-1, keepdim=True)
    O = (pr @ V) / den
    L = m_fin + torch.log2(den)
    P = torch.exp2(S - L)
    delta = (dO * rnd(O)).sum(-1, keepdim=True)
    dS = P * (dO @ V.transpose(2, 3) - delta)
    dq = rnd(HD ** -0.5 * (rnd(dS) @ K))
    dk = rnd(LN2 * (rnd(dS).transpose(2, 3) @ Q))
    dv = rnd(rnd(P).transpose(2, 3) @ dO)
    return {"out": O, "lse": L.squeeze(-1), "dq": dq, "dk": dk, "dv": dv}


@functools.lru_cache(maxsize=None)
def attn_expected(case):
    """(f64 reference, rounding model) of attn_inputs(case): computed once, shared, never modified"""
    ops = attn_inputs(case)
    return attn_backward(*ops, case[3], lambda x: x), attn_backward(*ops, case[3], bf16_round)


def lse_bound(lse_ref):
    """absolute bound, in natural-log units, on the log-sum-exp of an LSE forward: the one tests/test_gpu_vit_train.py:241 puts on ucod_attention_fwd_lse
    (2e-3 x max(1, largest |lse|)); ``lse_ref`` is base 2"""
    return 2e-3 * max(1.0, float(lse_ref.abs().max()) / LOG2E)


def slab_error(x, ref):
    return (x - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2).clamp_min(1e-300)


def row_error(x, ref):
    rms = ref.norm(dim=3).pow(2).mean(dim=2).sqrt().clamp_min(1e-300)
    return (x - ref).norm(dim=3).amax(dim=2) / rms


def zero_floor(case):
    """Absolute bound per element on dq / dk of a slab whose exact gradient is ZERO (one key: P = 1 and dP = delta, so dS = 0), where a relative error
    does not exist.  The kernel forms dP on the matrix pipe and delta in a VALU chain, both in f32: they differ by at most 2^-23 sum_d |dO_d| |v_d|
    <= 2^-23 * 96 * max|dO| * max|v|, sum_j P_j = 1, and dq = 96^-0.5 dS k, dk = ln 2 dS q'.  A lost delta leaves dS = dP, five orders above this."""
    qs, k, v, do = attn_inputs(case)
    mx = lambda t: float(t.float().abs().max())                              # noqa: E731
    return 2.0 ** -23 * HD * mx(do) * mx(v) * max(mx(k), mx(qs))


def attn_ratios(got, ref, model, floor=0.0):
    out = {}
    for name in GRADS:
        live = ref[name].flatten(2).norm(dim=2) > 0                              # slabs with an exactly zero reference: bounded by ``floor`` instead
        dead = (got[name].double().abs().flatten(2).amax(dim=2) * ~live).max()
        assert float(dead) <= floor, (name, "zero-reference slab", float(dead), floor)
        for bound, fn in (("slab", slab_error), ("row", row_error)):
            e_got, e_model = fn(got[name].double(), ref[name]), fn(model[name], ref[name])
            r = torch.where(e_model > 0, e_got / e_model, torch.where(e_got > 0, torch.full_like(e_got, math.inf), torch.zeros_like(e_got)))
            out[name, bound] = float(torch.where(live, r, torch.zeros_like(r)).max())
    return out


def attn_check(name, got, ref, model, audit=True, floor=0.0):
    """tests/attn_bwd_ref.py::check restated: for dq, dk, dv and each (window, head) slab, the relative L2 error against ``ref`` and the largest per-row
    error over the slab's RMS row norm are below F_MODEL x the rounding model's.  Never GPU output on the right-hand side.  A slab whose reference is
    exactly zero has no relative error: its elements are bounded by ``floor`` (zero_floor)."""
    r = attn_ratios(got, ref, model, floor)
    for (grad, bound), value in r.items():
        label = f"attn96_bwd:{name}:{grad}:{bound}_error_over_model"
        if audit:
            within(label, value, F_MODEL)
        else:
            assert value < F_MODEL, (label, value, F_MODEL)
    return r
