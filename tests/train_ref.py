"""Test helper: high-precision references of the decoder (DBA) and discriminator (APM) training kernels, the per-slice comparison and the case
lists that tests/test_train_ref.py (CPU) and tests/test_gpu_train_kernels.py (GPU) share.

Every reference is AUTOGRAD of the oracle's forward (oracle/decoder.py, oracle/discriminator.py, oracle/apm.py) run in a chosen dtype on the
CPU -- never the closed-form backward the kernels implement (oracle.decoder.rev_decoder_backward), which would share their derivation.

The bound (per compared slice):  e_k <= 8 * max(e_32, 2^-23), where
  e_k  = max|kernel - ref64| / max|ref64|   and   e_32 = max|ref32 - ref64| / max|ref64|,
ref32 being the same autograd graph run in float32 on identical inputs.  The kernels sum in orders different from ATen's (MFMA f32 chains,
block trees, f32 atomics across workgroups, chunked partials reduced in a fixed order): rounding of the same kind as the reference's with
other constants -- three bits cover that; the floor of one f32 ulp at the slice's scale covers slices the f32 reference happens to round
exactly.  A bound relative to the reference's rounding means nothing where the reference is unstable, so every slice of every case must also
have e_32 <= CAP.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import apm as OAPM, decoder as OD, discriminator as ODISC

FACTOR = 8
ULP = 2.0 ** -23
CAP = 1e-4
EMB = OD.EMB


def bound(e32):
    """The per-slice bound: FACTOR * max(e_32, 2^-23) (tensor or float)."""
    if torch.is_tensor(e32):
        return FACTOR * e32.clamp_min(ULP)
    return FACTOR * max(e32, ULP)


# ----------------------------------------------------------------------------------------------------------- comparison
def compare(kernel, ref64, ref32, slices):
    """(e_k, e_32), each a 1-d f64 tensor with one entry per slice.  ``slices`` = how many leading dimensions of ``ref64`` index a slice
    (0: the whole tensor, 1: per row of dim 0, 2: per (dim 0, dim 1) pair).  A slice whose ref64 is all zeros normalises nothing: there the
    kernel's (and the f32 reference's) slice must be exactly zero -- e = 0 if it is, inf if not.  NaN anywhere gives NaN (fails every bound)."""
    r = ref64.detach().double().cpu()
    k = torch.as_tensor(kernel).detach().double().cpu().reshape(r.shape)
    r32 = ref32.detach().double().cpu().reshape(r.shape)
    n = 1
    for s in r.shape[:slices]:
        n *= s
    r, k, r32 = r.reshape(n, -1), k.reshape(n, -1), r32.reshape(n, -1)
    scale = r.abs().amax(1)
    zero = scale == 0

    def rel(a):
        dv = (a - r).abs().amax(1)
        return torch.where(zero, torch.where(dv == 0, torch.zeros_like(dv), torch.full_like(dv, math.inf)), dv / torch.where(zero, 1.0, scale))

    return rel(k), rel(r32)


def worst(ek, e32):
    """(index, e_k, bound) of the slice closest to (or furthest past) its bound; a NaN slice counts as the worst."""
    b = bound(e32)
    ratio = torch.where(torch.isnan(ek), torch.full_like(ek, math.inf), ek / b)
    i = int(torch.argmax(ratio))
    return i, float(ek[i]), float(b[i])


def passes(ek, e32):
    """every slice within its bound (NaN fails)"""
    return bool((ek <= bound(e32)).all())


# ----------------------------------------------------------------------------------------------------------- case lists
# Decoder chain dba_project -> dba_colnorm -> dba_heads -> orth_gram -> dba_bwd -> dba_wgrad.  (B, C, H): H x H map, HW = H^2.
# HW = 1 is not a case (the orthogonality loss and its gradient are exactly zero there, a relative bound is undefined); HW = 4 is the smallest.
#   exact: the dba_project / dba_wgrad paths to run (None = the default dispatch; True = f32 MFMA; False = the three-way bf16 split)
#   clamp: two decoupling rows and their biases zeroed, one in each branch (different channel indices, so that the other branch's Gram row
#          is non-zero and the clamped-norm gradient gfeat / 1e-12 is not zero)
#   c0:    128 = the teacher half of a 256-row shared projection (student | teacher)
DECODER_CASES = [
    dict(id="b1_c384_h2", B=1, C=384, H=2, exact=(None,), clamp=False, c0=0),
    dict(id="b2_c768_h5", B=2, C=768, H=5, exact=(None,), clamp=False, c0=0),
    dict(id="b3_c384_h16", B=3, C=384, H=16, exact=(None,), clamp=False, c0=0),
    dict(id="b3_c384_h23", B=3, C=384, H=23, exact=(None,), clamp=False, c0=0),
    dict(id="b2_c1024_h37", B=2, C=1024, H=37, exact=(True, False), clamp=False, c0=0),
    dict(id="b4_c1536_h37", B=4, C=1536, H=37, exact=(None,), clamp=False, c0=0),
    dict(id="b32_c768_h68", B=32, C=768, H=68, exact=(True, False), clamp=False, c0=0),
    dict(id="b2_c768_h37_clamped", B=2, C=768, H=37, exact=(None,), clamp=True, c0=0),
    dict(id="b3_c384_h23_teacher", B=3, C=384, H=23, exact=(None,), clamp=False, c0=128),
]
CLAMPED_ROWS = (5, EMB + 40)
# upstream gradients, run separately so that neither term can hide the other: the gate term alone at the step's magnitude (~1/(B HW)), the
# orthogonality term alone, and both with gextra = 1000 as in the golden g1_decoder_*
DECODER_MODES = (("gate", True, 0.0), ("orth", False, 1.0), ("both", True, 1000.0))

# discriminator (fs, B): chunks_for at B = 32 gives 32 / 4 / 16 weight-gradient chunks, B = 37 and 100 split into uneven image ranges,
# fs = 37 runs 37 -> 19 -> 10 through the stride-2 boundary taps, fs = 4 gives 2 x 2 and 1 x 1 layers
DISC_CASES = [(4, 2), (5, 5), (28, 4), (37, 37), (68, 32), (68, 64), (28, 100)]

BCE_BATCHES = (1, 7, 256, 300)
BCE_SPECIAL = (1.0, 1e-30, 0.0, 1.0 - 2.0 ** -24)

APM_SHAPE = (32, 68 * 68)
APM_GSCALE = 1.0 / 8
APM_FRACS = (0.0, 0.5, 1.0)


def case_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


# ----------------------------------------------------------------------------------------------------------- decoder
def decoder_inputs(case):
    """f32 CPU tensors: x [B,C,H,H], W [Nout,C], b [Nout] (Nout = c0 + 128), emb [128], head_w [128], head_b [2], and the upstream
    gradients of each mode: {mode: (gfg [B,HW] | None, gbg | None, gextra)}."""
    g = torch.Generator().manual_seed(case_seed(case["id"]))
    B, C, H, c0 = case["B"], case["C"], case["H"], case["c0"]
    HW = H * H
    x = torch.randn(B, C, H, H, generator=g)
    Ws, bs = [], []
    for _ in range(c0 // 128 + 1):
        p = OD.init_params(C, g)
        Ws.append(p["decoupling.weight"].reshape(2 * EMB, C))
        bs.append(p["decoupling.bias"])
    W, b = torch.cat(Ws).contiguous(), torch.cat(bs).contiguous()
    if case["clamp"]:
        for r in CLAMPED_ROWS:
            W[c0 + r] = 0.0
            b[c0 + r] = 0.0
    emb = p["learnable_embedding"].reshape(2 * EMB).contiguous()
    head_w = torch.cat((p["conv_out_fg.weight"].reshape(EMB), p["conv_out_bg.weight"].reshape(EMB)))
    head_b = torch.cat((p["conv_out_fg.bias"], p["conv_out_bg.bias"]))
    gfg = torch.randn(B, HW, generator=g) / (B * HW)
    gbg = torch.randn(B, HW, generator=g) / (B * HW)
    modes = {name: ((gfg, gbg) if gate else (None, None)) + (gextra,) for name, gate, gextra in DECODER_MODES}
    return dict(x=x, W=W, b=b, emb=emb, head_w=head_w, head_b=head_b, modes=modes)


def decoder_ref(inp, c0, dtype, bug=None, modes=None):
    """Autograd of the oracle decoder in ``dtype``.  d = W[c0:c0+128] x + b[c0:c0+128] is computed in ``dtype`` and made a leaf; the
    oracle's _branches runs on it through an identity projection (exact in any dtype), then orth_loss_gram and the two heads as in
    rev_decoder_forward.  Per mode, L = sum(fg gfg) + sum(bg gbg) + gextra * extra is differentiated w.r.t. d and the four head tensors;
    gW = sum_{b,p} gd x and g_dec_bias = sum_{b,p} gd in the same dtype.

    ``bug`` (wrong variants for the sensitivity tests only): "orth_bhw" normalises the orthogonality loss by B HW instead of B HW^2,
    "gram_drop_last" leaves each image's last pixel out of the Gram sums, "gate_no_residual" drops the +1 residual term of the gate's derivative.
    ``modes``: the upstream-gradient modes to differentiate (default: all of ``inp["modes"]``; () = the forward alone)."""
    x = inp["x"]
    B, C, H, Wd = x.shape
    HW = H * Wd
    X = x.to(dtype).reshape(B, C, HW)
    W = inp["W"][c0:c0 + 128].to(dtype)
    bias = inp["b"][c0:c0 + 128].to(dtype)
    with torch.no_grad():
        d = torch.einsum("nc,bcp->bnp", W, X) + bias.view(1, -1, 1)
    d.requires_grad_(True)
    p = {"decoupling.weight": torch.eye(2 * EMB, dtype=dtype).view(2 * EMB, 2 * EMB, 1, 1), "decoupling.bias": torch.zeros(2 * EMB, dtype=dtype),
         "learnable_embedding": inp["emb"].to(dtype).view(2, EMB)}
    hw = inp["head_w"].to(dtype)
    hb = inp["head_b"].to(dtype)
    wf, wb = hw[:EMB].clone().requires_grad_(True), hw[EMB:].clone().requires_grad_(True)
    bf, bb = hb[0:1].clone().requires_grad_(True), hb[1:2].clone().requires_grad_(True)
    d1, d2, f1, f2, n1, n2 = OD._branches(d.view(B, 2 * EMB, H, Wd), p)
    extra = OD.orth_loss_gram(f1.transpose(1, 2), f2.transpose(1, 2))
    if bug == "orth_bhw":
        extra = extra * HW
    r1, r2 = (d1.detach(), d2.detach()) if bug == "gate_no_residual" else (d1, d2)
    a1 = torch.sigmoid(f1 * d1) + r1                      # DBA.py:48-49, as rev_decoder_forward
    a2 = torch.sigmoid(f2 * d2) + r2
    fg = torch.einsum("c,bcp->bp", wf, a1) + bf
    bg = torch.einsum("c,bcp->bp", wb, a2) + bb
    with torch.no_grad():
        gf1, gf2 = (f1[..., :-1], f2[..., :-1]) if bug == "gram_drop_last" else (f1, f2)
        out = dict(fg=fg.detach(), bg=bg.detach(), loss=extra.detach().reshape(1),
                   norm=torch.cat((n1, n2), 1).reshape(B, 2 * EMB),
                   gram=torch.stack((torch.bmm(gf1, gf1.transpose(1, 2)), torch.bmm(gf2, gf2.transpose(1, 2))), 1),
                   sdiag=((f1 * f2).sum(1) ** 2).sum(1))
    leaves = [d, wf, bf, wb, bb]
    names = list(inp["modes"]) if modes is None else list(modes)
    for i, name in enumerate(names):
        gfg, gbg, gextra = inp["modes"][name]
        L = gextra * extra
        if gfg is not None:
            L = L + (fg * gfg.to(dtype)).sum() + (bg * gbg.to(dtype)).sum()
        gs = torch.autograd.grad(L, leaves, retain_graph=i + 1 < len(names), allow_unused=True)
        gd, gwf, gbf, gwb, gbb = (torch.zeros_like(t) if gr is None else gr for gr, t in zip(gs, leaves))   # (no head in the graph: zero)
        with torch.no_grad():
            out[name] = dict(gd=gd, g_head_w=torch.stack((gwf, gwb)), g_head_b=torch.cat((gbf, gbb)), g_dec_bias=gd.sum((0, 2)),
                             gW=torch.einsum("bnp,bcp->nc", gd, X))
    return out


# slices per decoder output: per image fg, bg, norm; per (image, branch) gram; per (image, channel) row gd; per output row gW; else whole
DECODER_FWD_SLICES = dict(fg=1, bg=1, norm=1, gram=2, sdiag=0, loss=0)
DECODER_BWD_SLICES = dict(gd=2, gW=1, g_head_w=0, g_head_b=0, g_dec_bias=0)


# ----------------------------------------------------------------------------------------------------------- discriminator
DISC_NAMES = {"w1": "maskConv.layers.0.weight", "g1": "maskConv.layers.1.weight", "b1": "maskConv.layers.1.bias",
              "w2": "convs.0.layers.0.weight", "g2": "convs.0.layers.1.weight", "b2": "convs.0.layers.1.bias",
              "w3": "convs.1.layers.0.weight", "g3": "convs.1.layers.1.weight", "b3": "convs.1.layers.1.bias",
              "lin_w": "linear.weight", "lin_b": "linear.bias",
              "rm1": "maskConv.layers.1.running_mean", "rv1": "maskConv.layers.1.running_var",
              "rm2": "convs.0.layers.1.running_mean", "rv2": "convs.0.layers.1.running_var",
              "rm3": "convs.1.layers.1.running_mean", "rv3": "convs.1.layers.1.running_var"}
DISC_GRADS = ("w1", "g1", "b1", "w2", "g2", "b2", "w3", "g3", "b3", "lin_w", "lin_b")     # reference order (ops.DISC_GRAD_SHAPES)
DISC_RUNNING = ("rm1", "rv1", "rm2", "rv2", "rm3", "rv3")
NBT_KEYS = tuple(f"{n}.layers.1.num_batches_tracked" for n, _, _, _ in ODISC.BLOCKS)
# per output channel: the conv weight gradients; per channel: lin_w (viewed [8, s3^2]); whole tensor: the rest
DISC_GRAD_SLICES = dict(w1=1, w2=1, w3=1, lin_w=1)


def chunks_for(pairs, B):
    """csrc/disc.hip ucod_disc_bwd: how many image chunks the weight gradient of a layer with ``pairs`` (co, ci) pairs is split into."""
    return max(1, min(2048 // pairs, B))


def chunk_range(B, chunks, y):
    """conv3x3_wgrad_kernel: images [b_lo, b_hi) of chunk y."""
    return B * y // chunks, B * (y + 1) // chunks


def disc_inputs(fs, B, seed=7919):
    """The discriminator state (BatchNorm affine terms perturbed away from 1 / 0, running buffers away from 0 / 1) and two calls' inputs,
    pseudo label first, then student: binary masks with per-image densities, a few all-empty and all-full images inside mixed batches
    (B >= 5), and gprob of mixed signs.  (The two calls' gradients are summed: inputs where they nearly cancel make the sum ill-conditioned
    -- the seed offset 0 gives e_32 = 3e-4 on one entry of (68, 32); test_train_ref.py asserts the cap on every case.)"""
    g = torch.Generator().manual_seed(1000 * fs + B + seed)
    sd = ODISC.init_state(fs, g)
    for name, _, cout, _ in ODISC.BLOCKS:
        sd[f"{name}.layers.1.weight"] = 1.0 + 0.3 * (2 * torch.rand(cout, generator=g) - 1)
        sd[f"{name}.layers.1.bias"] = 0.2 * torch.randn(cout, generator=g)
        sd[f"{name}.layers.1.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.layers.1.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{name}.layers.1.num_batches_tracked"] = torch.tensor(3, dtype=torch.long)
    s3 = ((fs - 1) // 2) // 2 + 1
    if B * s3 * s3 < 4:
        # the last BatchNorm normalises B s3^2 = 2 values per channel: its output is +-gamma |d| / sqrt(d^2 + eps) + beta (d = half their
        # difference), whose derivative eps / (d^2 + eps)^1.5 the reference's backward forms by cancellation, losing a factor (d^2 + eps) / eps:
        # 6.5e-4 of f32 error at the default initialisation (d ~ 0.3).  A third conv scaled to d^2 ~ eps keeps every slice near 1e-6.
        sd["convs.1.layers.0.weight"] = sd["convs.1.layers.0.weight"] * 0.01
    masks, gprobs = [], []
    for call in range(2):
        dens = 0.2 + 0.6 * torch.rand(B, 1, 1, 1, generator=g)
        m = (torch.rand(B, 1, fs, fs, generator=g) < dens).float()
        if B >= 5:
            m[1 + call] = 0.0
            m[3 - call] = 1.0
        masks.append(m)
        gprobs.append(torch.randn(B, generator=g))
    return sd, masks, gprobs


@contextlib.contextmanager
def _oracle_conv_block(fn):
    saved = ODISC.conv_block
    ODISC.conv_block = fn
    try:
        yield
    finally:
        ODISC.conv_block = saved


def _conv_block_bug(bug, drop_image):
    """A wrong variant of oracle.discriminator.conv_block (sensitivity tests only); every variant leaves the forward values as they are.
    "w1_drop_image": the first layer's weight gradient without image ``drop_image``; "dgrad_no_far_taps": no input gradient through the
    bottom row / right column of a stride-2 conv's input; "bn_bwd_no_mean": BatchNorm backward without the mean(gh) term (the batch mean
    is a constant to the backward); "running_var_biased": running_var updated with the biased variance."""
    def block(x, sd, name, stride, update_running=True):
        w = sd[f"{name}.layers.0.weight"]
        if bug == "w1_drop_image" and name == "maskConv":
            j = drop_image
            y = torch.cat((F.conv2d(x[:j], w, None, stride=stride, padding=1), F.conv2d(x[j:j + 1], w.detach(), None, stride=stride, padding=1),
                           F.conv2d(x[j + 1:], w, None, stride=stride, padding=1)))
        elif bug == "dgrad_no_far_taps" and stride == 2:
            keep = torch.ones_like(x)
            keep[..., -1, :] = 0.0
            keep[..., :, -1] = 0.0
            y = F.conv2d(x * keep + x.detach() * (1 - keep), w, None, stride=stride, padding=1)
        else:
            y = F.conv2d(x, w, None, stride=stride, padding=1)
        n = y.numel() // y.shape[1]
        mean = y.mean((0, 2, 3))
        var = ((y - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        if update_running:
            with torch.no_grad():
                unb = var if bug == "running_var_biased" else var * (n / max(n - 1, 1))
                rm, rv = f"{name}.layers.1.running_mean", f"{name}.layers.1.running_var"
                sd[rm] = (1 - ODISC.BN_MOMENTUM) * sd[rm] + ODISC.BN_MOMENTUM * mean.detach()
                sd[rv] = (1 - ODISC.BN_MOMENTUM) * sd[rv] + ODISC.BN_MOMENTUM * unb.detach()
                sd[f"{name}.layers.1.num_batches_tracked"] = sd[f"{name}.layers.1.num_batches_tracked"] + 1
        mc = mean.detach() if bug == "bn_bwd_no_mean" else mean
        yh = (y - mc.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + ODISC.BN_EPS)
        yh = yh * sd[f"{name}.layers.1.weight"].view(1, -1, 1, 1) + sd[f"{name}.layers.1.bias"].view(1, -1, 1, 1)
        return torch.where(yh >= 0, yh, yh * ODISC.LRELU)
    return block


def disc_ref(sd0, masks, gprobs, dtype, bug=None, drop_image=0):
    """Autograd of oracle.discriminator.discriminator_forward on sum(gprob * prob), in ``dtype``, for the calls in sequence on ONE state
    dict (running buffers mutate between calls), gradients summed over the calls.  -> dict(prob=[per call], grads={name: tensor},
    running=[{name: tensor} after each call], nbt=[3 counters after the last call])."""
    sd = {k: (v.clone() if v.dtype == torch.long else v.to(dtype).clone()) for k, v in sd0.items()}
    for k in DISC_GRADS:
        sd[DISC_NAMES[k]].requires_grad_(True)
    leaves = [sd[DISC_NAMES[k]] for k in DISC_GRADS]
    grads = [torch.zeros_like(t) for t in leaves]
    probs, running = [], []
    ctx = _oracle_conv_block(_conv_block_bug(bug, drop_image)) if bug else contextlib.nullcontext()
    with ctx:
        for m, gp in zip(masks, gprobs):
            prob = ODISC.discriminator_forward(m.to(dtype), sd).reshape(-1)
            gs = torch.autograd.grad((prob * gp.to(dtype)).sum(), leaves)
            grads = [a + b for a, b in zip(grads, gs)]
            probs.append(prob.detach())
            running.append({k: sd[DISC_NAMES[k]].detach().clone() for k in DISC_RUNNING})
    return dict(prob=probs, grads={k: v.detach() for k, v in zip(DISC_GRADS, grads)}, running=running, nbt=[int(sd[k]) for k in NBT_KEYS])


def disc_grad_view(name, t, fs):
    """the layout the slices are taken over: lin_w [1, 8 s3^2] -> [8, s3^2]"""
    if name == "lin_w":
        s3 = ((fs - 1) // 2) // 2 + 1
        return t.reshape(8, s3 * s3)
    return t


# ----------------------------------------------------------------------------------------------------------- losses
def bce_inputs(B):
    """f32 student / pseudo-label probabilities, the special values 1, 1e-30, 0 and 1 - 2^-24 at the front of each (reversed for the
    pseudo labels), the rest uniform in (0, 1)."""
    g = torch.Generator().manual_seed(7 * B + 1)
    ps, pp = torch.rand(B, generator=g), torch.rand(B, generator=g)
    k = min(len(BCE_SPECIAL), B)
    ps[:k] = torch.tensor(BCE_SPECIAL[:k])
    pp[:k] = torch.tensor(BCE_SPECIAL[::-1][:k])
    return ps, pp


def bce_ref(ps, pp, dtype, bug=None):
    """nn.BCELoss(cat(student, pseudo), [0 .. 0, 1 .. 1]) (mean over 2B, loop_UCOD_DPL.py:246-247) in ``dtype`` on the SAME f32 probabilities,
    and its gradient w.r.t. the probabilities (torch's backward divides by max(p (1 - p), 1e-12)).  ``bug`` = "no_clamp" (sensitivity test
    only): the gradient (p - t) / (p (1 - p)) without the clamp."""
    B = ps.numel()
    p = torch.cat((ps, pp)).to(dtype).requires_grad_(True)
    t = torch.cat((torch.zeros(B, dtype=dtype), torch.ones(B, dtype=dtype)))
    loss = F.binary_cross_entropy(p, t)
    (gp,) = torch.autograd.grad(loss, p)
    if bug == "no_clamp":
        with torch.no_grad():
            gp = (p - t) / (p * (1 - p)) / (2 * B)
    return dict(g_student=gp[:B].detach(), g_pseudo=gp[B:].detach(), loss=loss.detach().reshape(1))


def apm_inputs():
    B, HW = APM_SHAPE
    g = torch.Generator().manual_seed(31)
    pl = torch.rand(B, HW, generator=g)
    teacher, fg, bg = (2 * torch.randn(B, HW, generator=g) for _ in range(3))
    p_s, p_p = torch.rand(B, generator=g), torch.rand(B, generator=g)
    return dict(pl=pl, teacher=teacher, fg=fg, bg=bg, p_s=p_s, p_p=p_p)


def apm_ref(inp, epoch_frac, gscale, dtype):
    """oracle.apm in ``dtype``: w = clamp(apm_weight(...) with cur_epoch / (max_epoch + start_finetune) = epoch_frac), merged = pl (1 - w) +
    [sigmoid(teacher) > 0.5] w, the two BCE-with-logits means and the discriminator BCE of the student (loop_UCOD_DPL.py:161-173,257-272);
    gfg / gbg = gscale * autograd of the two BCE-with-logits terms."""
    c = {k: v.to(dtype) for k, v in inp.items()}
    w = torch.clamp(0.5 * (1 + torch.cos(torch.abs(c["p_s"] - c["p_p"]) * math.pi)) + epoch_frac, 0, 1)
    pt = (torch.sigmoid(c["teacher"]) > 0.5).to(dtype)
    merged = c["pl"] * (1 - w.view(-1, 1)) + pt * w.view(-1, 1)
    x, y = c["fg"].clone().requires_grad_(True), c["bg"].clone().requires_grad_(True)
    l1 = OAPM.bce_with_logits_mean(x, merged)
    l2 = OAPM.bce_with_logits_mean(y, 1 - merged)
    gx, gy = torch.autograd.grad(l1 + l2, (x, y))
    l3 = OAPM.bce_mean(c["p_s"], torch.zeros_like(c["p_s"]))
    return dict(w=w, merged=merged, gfg=gx * gscale, gbg=gy * gscale, l1=l1.detach().reshape(1), l2=l2.detach().reshape(1), l3=l3.reshape(1))


APM_SLICES = dict(w=1, merged=1, gfg=1, gbg=1, l1=0, l2=0, l3=0)
