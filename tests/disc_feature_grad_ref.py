"""f64 restatement of everything the gradient INTO the features of the feature-branch discriminator is checked against (test infrastructure; shared by
tests/test_disc_feature_grad_host.py and tests/test_gpu_disc_feature_grad.py):

* the feature-branch discriminator with train-mode BatchNorm (oracle/discriminator.py) under torch autograd, in f64;
* the step's scalar  S(feats) = BCEWithLogits(fg, merged) + BCEWithLogits(bg, 1 - merged) - [not finetune] BCE(p_s, 0)  with fg, bg, teacher, pl and the binarised
  masks held constant: merged = pl (1 - w) + tb w,  w = clamp(0.5 (1 + cos(pi |p_s - p_p|)) + epoch_frac, 0, 1)  (loop_UCOD_DPL.py:160-171, 257-272);
* the closed forms of d(S)/d(p_s, p_p) that ucod_apm_bce_gprob computes, with the error bound its GPU test holds it to;
* f64 conv2d with the bound |err| <= (K + 1) 2^-24 sum |w x| of a K-term f32 dot product accumulated in any order (every product rounded once, at most K
  additions each rounding once: (1 + 2^-24)^(K+1) - 1 ~ (K + 1) 2^-24 relative to the sum of magnitudes);
* the index map of ucod_conv3x3_dgrad_weights.
"""
import math

import torch
import torch.nn.functional as F

from oracle import discriminator as OD
from oracle.resize import torch_bilinear

EPS32 = 2.0 ** -24


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ discriminator
def init_feature_disc_state(dim, fs, gen, affine_scale=0.0, linear_scale=None):
    """state dict of Discriminator(dis_use_features=True): nn.Conv2d's default bound for the convolutions; BatchNorm affines 1 / 0 (``affine_scale`` = 0) or
    drawn N(0, affine_scale^2); Linear at nn.Linear's default bound or N(0, linear_scale^2)"""
    sd = {}
    indim = dim + 32
    for name, cin, cout in (("maskConv", 1, 32), ("featureConv", dim, dim), ("convs.0", indim, indim // 2), ("convs.1", indim // 2, indim // 4)):
        bound = 1.0 / math.sqrt(cin * 9)
        sd[f"{name}.layers.0.weight"] = (torch.rand(cout, cin, 3, 3, generator=gen) * 2 - 1) * bound
        if affine_scale:
            sd[f"{name}.layers.1.weight"] = torch.randn(cout, generator=gen) * affine_scale
            sd[f"{name}.layers.1.bias"] = torch.randn(cout, generator=gen) * affine_scale
        else:
            sd[f"{name}.layers.1.weight"], sd[f"{name}.layers.1.bias"] = torch.ones(cout), torch.zeros(cout)
        sd[f"{name}.layers.1.running_mean"], sd[f"{name}.layers.1.running_var"] = torch.zeros(cout), torch.ones(cout)
        sd[f"{name}.layers.1.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    nin = indim // 4 * ((fs + 3) // 4) ** 2
    if linear_scale is None:
        bound = 1.0 / math.sqrt(nin)
        sd["linear.weight"] = (torch.rand(1, nin, generator=gen) * 2 - 1) * bound
        sd["linear.bias"] = (torch.rand(1, generator=gen) * 2 - 1) * bound
    else:
        sd["linear.weight"] = torch.randn(1, nin, generator=gen) * linear_scale
        sd["linear.bias"] = torch.randn(1, generator=gen) * linear_scale
    return sd


def disc_prob(mask, feat, sd):
    """[B] probabilities of the feature-branch module in the dtype of its arguments; ``sd`` is mutated as the always-train-mode module mutates itself"""
    return OD.discriminator_forward_with_features(mask, feat, sd).reshape(-1)


def disc_linear_form_grad(sd, masks, feat, rs):
    """f64 autograd of sum_calls sum_b r[b] D(mask, f)[b] with respect to f -> (dfeat, [prob per call])"""
    sd = to64(sd)
    f = feat.double().clone().requires_grad_(True)
    probs = [disc_prob(m.double(), f, sd) for m in masks]
    total = sum((r.double().reshape(-1) * p).sum() for r, p in zip(rs, probs))
    (g,) = torch.autograd.grad(total, f)
    return g, [p.detach() for p in probs]


# ------------------------------------------------------------------------------------------------ the step's scalar
def binarize_teacher(teacher):
    """sigmoid(teacher) > 0.5 on f32 logits, as ucod_apm_bce does (callers keep |teacher| away from the one-rounding neighbourhood of 0)"""
    return (torch.sigmoid(teacher.float()) > 0.5).double()


def step_scalar(p_s, p_p, fg, bg, tb, pl, epoch_frac, finetune):
    """S as a function of the two probability vectors [B]; fg, bg, tb, pl [B,HW] f64 constants.  torch differentiates BCEWithLogits w.r.t. its target."""
    w = torch.clamp(0.5 * (1 + torch.cos(torch.abs(p_s - p_p) * math.pi)) + epoch_frac, 0, 1).unsqueeze(1)
    merged = pl * (1 - w) + tb * w
    s = F.binary_cross_entropy_with_logits(fg, merged) + F.binary_cross_entropy_with_logits(bg, 1 - merged)
    if not finetune:
        s = s - F.binary_cross_entropy(p_s, torch.zeros_like(p_s))
    return s


def gprob_autograd(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune):
    """gscale * dS/d(p_s, p_p) by f64 autograd through binary_cross_entropy_with_logits' target and clamp -> (gp_s, gp_p) f64 [B]"""
    ps = p_s.double().clone().requires_grad_(True)
    pp = p_p.double().clone().requires_grad_(True)
    s = step_scalar(ps, pp, fg.double(), bg.double(), binarize_teacher(teacher), pl.double(), epoch_frac, finetune)
    gs, gp = torch.autograd.grad(s, [ps, pp])
    return gs * gscale, gp * gscale


def gprob_closed_form(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune, mutate=None):
    """the formulas of ucod_apm_bce_gprob (include/ucod_dpl.h) in f64 -> (gp_s, gp_p, bound): ``bound`` [B] is what the GPU test allows the f32 kernel,
    (HW + 8) 2^-24 sum_p |term| |dw/dD| gscale + 4 ulp (f32) of the dis_loss part.  ``mutate``: a deliberately wrong variant (the host test shows that each one
    leaves the bound): "no_target" (target path dropped), "gp_p_sign", "no_1_over_B"."""
    B, HW = pl.shape
    ps, pp = p_s.double(), p_p.double()
    term = (bg.double() - fg.double()) * (binarize_teacher(teacher) - pl.double()) / (B * HW)
    gw = term.sum(1)
    d = ps - pp
    u = 0.5 * (1 + torch.cos(math.pi * d.abs())) + epoch_frac
    dwd = torch.where((u >= 0) & (u <= 1), -0.5 * math.pi * torch.sin(math.pi * d.abs()) * torch.sign(d), torch.zeros_like(d))
    tgt = gscale * gw * dwd
    if mutate == "no_target":
        tgt = torch.zeros_like(tgt)
    floor = float(torch.tensor(1e-12, dtype=torch.float32))         # torch's EPSILON is an f32 constant in every dtype's BCELoss backward
    dis = gscale * (1.0 / (1 if mutate == "no_1_over_B" else B)) * ps / torch.clamp(ps * (1 - ps), min=floor)
    if finetune:
        dis = torch.zeros_like(dis)
    gp_s = tgt - dis
    gp_p = tgt if mutate == "gp_p_sign" else -tgt
    dis32 = dis.float().abs()
    ulp = (torch.nextafter(dis32, torch.full_like(dis32, float("inf"))) - dis32).double()
    ulp = torch.where(dis32 > 0, ulp, torch.zeros_like(ulp))
    bound = (HW + 8) * EPS32 * term.abs().sum(1) * dwd.abs() * gscale + 4 * ulp
    return gp_s, gp_p, bound


def step_scalar_of_features(feat, sd, mask_s, mask_p, fg, bg, teacher, pl, epoch_frac, finetune):
    """S(feats) in f64: the discriminator on (mask_s, feats) then (mask_p, feats) -- the loop's order -- feeding step_scalar -> (S, p_s, p_p)"""
    sd = to64(sd)
    p_s = disc_prob(mask_s.double(), feat, sd)
    p_p = disc_prob(mask_p.double(), feat, sd)
    return step_scalar(p_s, p_p, fg.double(), bg.double(), binarize_teacher(teacher), pl.double(), epoch_frac, finetune), p_s, p_p


def bilinear_adjoint_f64(g, ih, iw):
    """the transpose of F.interpolate(bilinear, align_corners=False) from (ih, iw) to g's grid, applied to g, in f64"""
    x = torch.zeros(*g.shape[:-2], ih, iw, dtype=torch.float64, requires_grad=True)
    (out,) = torch.autograd.grad((torch_bilinear(x, *g.shape[-2:]) * g.double()).sum(), x)
    return out


# ------------------------------------------------------------------------------------------------ convolution
def wmat_of(weight, kpad=None):
    """conv weight [Nout,C,3,3] -> the GEMM's [Nout,Kpad] (column c*9 + ky*3 + kx, zero-padded to a multiple of 16)"""
    nout, K = weight.shape[0], weight.shape[1] * 9
    kpad = (K + 15) // 16 * 16 if kpad is None else kpad
    out = torch.zeros(nout, kpad, dtype=weight.dtype)
    out[:, :K] = weight.reshape(nout, K)
    return out


def conv3x3_f64(x, weight):
    """-> (y, bound): f64 pad-1 conv2d and the f32 bound (K + 1) 2^-24 sum |w x| per output element, K = 9 C, the sum taken in f64"""
    y = F.conv2d(x.double(), weight.double(), None, 1, 1)
    mag = F.conv2d(x.double().abs(), weight.double().abs(), None, 1, 1)
    return y, (9 * x.shape[1] + 1) * EPS32 * mag


def conv3x3_dgrad_f64(gy, weight):
    """-> (gx, bound): f64 autograd of conv2d(x; weight) against the cotangent gy, and the same bound with K = 9 Cout terms per element"""
    x = torch.zeros(gy.shape[0], weight.shape[1], *gy.shape[2:], dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad((F.conv2d(x, weight.double(), None, 1, 1) * gy.double()).sum(), x)
    xm = torch.zeros_like(x, requires_grad=True)
    (mag,) = torch.autograd.grad((F.conv2d(xm, weight.double().abs(), None, 1, 1) * gy.double().abs()).sum(), xm)
    return gx, (9 * weight.shape[0] + 1) * EPS32 * mag


def dgrad_weights_index(weight):
    """the index formula of ucod_conv3x3_dgrad_weights: Wd[ci][co*9 + t] = W[co][ci][8 - t], columns >= 9 Cout zero, Kpad = 16 ceil(9 Cout / 16)"""
    cout, cin = weight.shape[:2]
    kpad = (9 * cout + 15) // 16 * 16
    wd = torch.zeros(cin, kpad, dtype=weight.dtype)
    flipped = weight.reshape(cout, cin, 9).flip(2)                  # [co][ci][t] = W[co][ci][8 - t]
    wd[:, :9 * cout] = flipped.permute(1, 0, 2).reshape(cin, 9 * cout)
    return wd


def wd_as_conv_weight(wd, cout):
    """Wd [Cin,Kpad] read back as the conv weight [Cin,Cout,3,3] it stands for (column co*9 + ky*3 + kx)"""
    return wd[:, :9 * cout].reshape(wd.shape[0], cout, 3, 3)


# ------------------------------------------------------------------------------------------------ the gprob case list
def gprob_cases(HW, gen):
    """B = 6 images, one each: D > 0; D < 0; D = 0 exactly; small |D| (clamped at epoch_frac = 0.6); |D| ~ 0.9 (unclamped at 0.6); p_s = 1.0 exactly.
    Teacher logits keep |x| >= 0.05 so that the binarisation cannot depend on one rounding."""
    B = 6
    p_s = torch.tensor([0.70, 0.20, 0.40, 0.52, 0.95, 1.00])
    p_p = torch.tensor([0.30, 0.65, 0.40, 0.50, 0.05, 0.35])
    pl = torch.rand(B, HW, generator=gen)
    teacher = torch.randn(B, HW, generator=gen)
    teacher = torch.where(teacher.abs() < 0.05, torch.full_like(teacher, 0.05), teacher)
    fg = torch.randn(B, HW, generator=gen) * 2
    bg = torch.randn(B, HW, generator=gen) * 2
    return pl, teacher, fg, bg, p_s, p_p


# ------------------------------------------------------------------------------------------------ the whole step (G12 backbone, dim 128, fs 8)
STEP_FS, STEP_DIM = 8, 128
STEP_SEED, STEP_AFFINE_SCALE, STEP_LINEAR_SCALE = 5, 1.0, 0.25


def step_case(seed=STEP_SEED, affine_scale=STEP_AFFINE_SCALE, linear_scale=STEP_LINEAR_SCALE):
    """the inputs of the step test: G12's backbone and images, a drawn student / teacher decoder, a feature-branch discriminator whose BatchNorm affines and
    Linear are drawn at unit scale (N(0, affine_scale^2), N(0, linear_scale^2)) so that its probabilities spread and its share of the gradient is visible"""
    from conftest import load_golden, sub
    from oracle import decoder as D
    g = load_golden("g12_lora_backbone")
    gen = torch.Generator().manual_seed(seed)
    dec, ema = D.init_params(STEP_DIM, gen), D.init_params(STEP_DIM, gen)
    disc = init_feature_disc_state(STEP_DIM, STEP_FS, gen, affine_scale, linear_scale)
    pl = (torch.rand(2, 1, 16, 16, generator=gen) > 0.5).float()
    return dict(x=g["x"], sd=sub(g, "sd."), dec=dec, ema=ema, disc=disc, pl=pl)


def full_step_lora_grads(case, finetune=False, with_disc=True, epoch_frac=0.0, masks=None):
    """f64 autograd of the whole step (oracle ViT + LoRA -> key map -> resize -> decoder -> APM with the feature-branch discriminator -> loss) down to the LoRA
    matrices -> dict(grads {name: tensor}, loss, p_s, p_p, u).  ``with_disc=False``: the discriminator sees detached features (the frozen-backbone step's
    graph: what the loop computed before it had the gradient into the features).  ``masks`` = (mask_s, mask_p, tb): binarised maps to use instead of the
    reference's own (the GPU test hands over the device's, so that no binarisation can flip between the two sides)."""
    from oracle import decoder as D
    from oracle import vit as OV
    sd = to64(case["sd"])
    names = [k for k in sd if ".lora_" in k]
    leaf = {k: sd[k].clone().requires_grad_(True) for k in names}
    sd.update(leaf)
    _, key = OV.dinov2_forward(case["x"].double(), sd, heads=2, full_last_layer=False, lora_scale=2.0)
    B = key.shape[0]
    feats = torch_bilinear(key, STEP_FS, STEP_FS)
    pl = torch_bilinear(case["pl"].double(), STEP_FS, STEP_FS)
    with torch.no_grad():
        teacher = D.rev_decoder_forward(feats, to64(case["ema"]), ema=True)[0]
    fg, bg, extra = D.rev_decoder_forward(feats, to64(case["dec"]), ema=False, orth="gram")
    if masks is None:
        mask_s, mask_p, tb = (torch.sigmoid(fg.detach()) > 0.5).double(), (pl > 0.5).double(), (torch.sigmoid(teacher) > 0.5).double().view(B, -1)
    else:
        mask_s, mask_p, tb = (m.double() for m in masks)
    fd = feats if with_disc else feats.detach()
    dsd = to64(case["disc"])
    p_s = disc_prob(mask_s.view(B, 1, STEP_FS, STEP_FS), fd, dsd)
    p_p = disc_prob(mask_p.view(B, 1, STEP_FS, STEP_FS), fd, dsd)
    u = 0.5 * (1 + torch.cos(math.pi * (p_s - p_p).abs())) + epoch_frac
    w = torch.clamp(u, 0, 1).unsqueeze(1)
    merged = pl.view(B, -1) * (1 - w) + tb.view(B, -1) * w
    loss = F.binary_cross_entropy_with_logits(fg.view(B, -1), merged) + F.binary_cross_entropy_with_logits(bg.view(B, -1), 1 - merged) + extra
    if not finetune:
        loss = loss - F.binary_cross_entropy(p_s, torch.zeros_like(p_s))
    gl = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(leaf[k]) if g is None else g) for k, g in zip(names, gl)}
    return dict(grads=grads, loss=loss.detach(), p_s=p_s.detach(), p_p=p_p.detach(), u=u.detach())
