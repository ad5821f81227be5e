"""GPU: the gradient into the features of the feature-branch discriminator (backbone-backward mode with dis_use_features=True), layer by layer:
ucod_conv3x3_f32 (bit-identical to ucod_unfold3x3 + ucod_dba_project), ucod_conv3x3_dgrad_weights, ucod_apm_bce_gprob, Discriminator.input_grad_features,
the module under autograd, and TrainLoop._process_batch_full -- each against the f64 restatement of tests/disc_feature_grad_ref.py."""
import copy
import functools
import types

import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops  # noqa: E402
from ucod_dpl_amd.engine.config import CfgNode  # noqa: E402
from ucod_dpl_amd.models.discriminator import Discriminator  # noqa: E402
import disc_feature_grad_ref as R  # noqa: E402

DEV = "cuda:0"
EINVAL = -1


def two_launch_conv(x, wmat):
    """the existing route: ucod_unfold3x3 (stride 1) + ucod_dba_project with a zero bias"""
    lib = N.load()
    B, C, H, W = x.shape
    nout, kpad = wmat.shape
    cols = torch.empty(B, kpad, H * W, device=x.device)
    N.check(lib.ucod_unfold3x3(N.ptr(x), N.ptr(cols), B, C, H, W, 1, kpad, N.stream()), "ucod_unfold3x3")
    y = torch.empty(B, nout, H * W, device=x.device)
    zero = torch.zeros(nout, device=x.device)
    N.check(lib.ucod_dba_project(N.ptr(cols), N.ptr(wmat), N.ptr(zero), N.ptr(y), B, kpad, H * W, nout, N.stream()), "ucod_dba_project")
    return y.view(B, nout, H, W)


# ------------------------------------------------------------------------------------------------ 1. ucod_conv3x3_f32
CONV_CASES = [(2, 16, 12, 12, 16),     # 9C a multiple of 16
              (1, 1, 9, 7, 32),        # K = 9, padded to 16
              (2, 23, 7, 9, 136),      # 9C = 207 padded to 208; a second 128-row block, a last wave with 8 live rows
              (1, 5, 1, 65, 40),       # H = 1; a pixel tile of 65, HW % 4 != 0
              (1, 5, 63, 1, 40),       # W = 1; 63 pixels
              (1, 3, 8, 8, 127)]       # HW = 64 exactly


@pytest.mark.parametrize("B,C,H,W,Nout", CONV_CASES)
def test_conv3x3_equals_the_two_launch_route_bit_for_bit(B, C, H, W, Nout):
    gen = torch.Generator().manual_seed(B * 1000 + C * 10 + Nout)
    x = torch.randn(B, C, H, W, generator=gen)
    weight = torch.randn(Nout, C, 3, 3, generator=gen)
    wmat = R.wmat_of(weight).to(DEV)
    xd = x.to(DEV)
    ref2 = two_launch_conv(xd, wmat)
    # canary rows either side of y
    n, pad = B * Nout * H * W, 2 * H * W
    buf = torch.full((n + 2 * pad,), 7.0, device=DEV)
    lib = N.load()
    rc = lib.ucod_conv3x3_f32(N.ptr(xd), N.ptr(wmat), buf.data_ptr() + 4 * pad, B, C, H, W, Nout, wmat.shape[1], N.stream())
    assert rc == 0
    y = buf[pad:pad + n].view(B, Nout, H, W)
    assert torch.equal(y, ref2)
    assert bool((buf[:pad] == 7.0).all()) and bool((buf[pad + n:] == 7.0).all())
    assert torch.equal(ops.conv3x3(xd, wmat), ref2)
    # against f64 conv2d within the bound of a K-term f32 dot product
    ref, bound = R.conv3x3_f64(x, weight)
    err = (y.cpu().double() - ref).abs()
    print(f"conv3x3 {B, C, H, W, Nout}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def test_conv3x3_refusals_leave_y_unwritten():
    lib = N.load()
    B, C, H, W, Nout = 1, 3, 5, 4, 8
    x = torch.randn(B, C, H, W, device=DEV)
    wbuf = torch.randn(Nout * 32 + 4, device=DEV)            # 16-byte aligned base; + 1 float = misaligned
    assert wbuf.data_ptr() % 16 == 0
    y = torch.full((B, Nout, H, W), 7.0, device=DEV)
    px, pw, py, s = N.ptr(x), wbuf.data_ptr(), N.ptr(y), N.stream()
    assert lib.ucod_conv3x3_f32(px, pw, py, B, C, H, W, Nout, 32, s) == 0
    torch.cuda.synchronize()
    y.fill_(7.0)
    bad = [(None, pw, py, B, C, H, W, Nout, 32), (px, None, py, B, C, H, W, Nout, 32), (px, pw, None, B, C, H, W, Nout, 32)]
    for i in range(3, 9):                                     # a zero and a negative value of every size
        for v in (0, -1):
            a = [px, pw, py, B, C, H, W, Nout, 32]
            a[i] = v
            bad.append(tuple(a))
    bad += [(px, pw, py, B, C, H, W, Nout, 40),                # Kpad % 16 != 0
            (px, pw, py, B, C, H, W, Nout, 16),                # Kpad < 9C
            (px, pw + 4, py, B, C, H, W, Nout, 32)]            # Wmat not 16-byte aligned
    for a in bad:
        assert lib.ucod_conv3x3_f32(*a, s) == EINVAL, a
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert lib.ucod_conv3x3_dgrad_weights(None, py, 4, 4, 48, s) == EINVAL and lib.ucod_conv3x3_dgrad_weights(px, py, 4, 4, 32, s) == EINVAL
    assert lib.ucod_apm_bce_gprob(None, px, px, px, px, px, 0.0, 1.0, 0, py, py, 1, 4, s) == EINVAL
    assert lib.ucod_apm_bce_gprob(px, px, px, px, px, px, 0.0, 1.0, 0, py, py, 0, 4, s) == EINVAL


# ------------------------------------------------------------------------------------------------ 2. ucod_conv3x3_dgrad_weights
def _small_disc(dim=8, fs=9):
    return Discriminator(CfgNode(dict(dim=dim, feature_size=fs, ema_weight=0.99, dis_use_features=True))).to(DEV)


@pytest.mark.parametrize("Cout,Cin", [(16, 16), (40, 5), (136, 23)])
def test_dgrad_weights_and_the_data_gradient(Cout, Cin):
    gen = torch.Generator().manual_seed(Cout + Cin)
    B, H, W = 2, 7, 9
    weight = torch.randn(Cout, Cin, 3, 3, generator=gen)
    gy = torch.randn(B, Cout, H, W, generator=gen)
    wd = ops.conv3x3_dgrad_weights(weight.to(DEV))
    assert torch.equal(wd.cpu(), R.dgrad_weights_index(weight))
    gx = ops.conv3x3(gy.to(DEV), wd)
    ref, bound = R.conv3x3_dgrad_f64(gy, weight)
    err = (gx.cpu().double() - ref).abs()
    print(f"dgrad {Cout, Cin}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # the existing route: W^T GEMM into [B, 9 Cin, HW], then ucod_fold3x3
    K = 9 * Cin
    kpad = (K + 15) // 16 * 16
    rec = dict(wmat=R.wmat_of(weight).to(DEV), geom=(B, Cin, H, W, Cout, H, W, 1, K, kpad))
    old = _small_disc()._conv_dgrad_fold(rec, gy.to(DEV).reshape(B, Cout, H * W).contiguous())
    assert bool(((gx - old).cpu().double().abs() <= 2 * bound).all())


# ------------------------------------------------------------------------------------------------ 3. ucod_apm_bce_gprob
@pytest.mark.parametrize("HW", [7, 144, 257])
def test_gprob_against_f64_autograd(HW):
    pl, teacher, fg, bg, p_s, p_p = R.gprob_cases(HW, torch.Generator().manual_seed(HW))
    dev = [t.to(DEV).contiguous() for t in (pl, teacher, fg, bg, p_s, p_p)]
    for epoch_frac in (0.0, 0.6):
        for finetune in (0, 1):
            for gscale in (1.0, 0.5):
                gs, gp = ops.apm_bce_gprob(*dev, epoch_frac, gscale=gscale, finetune=finetune)
                gs2, gp2 = ops.apm_bce_gprob(*dev, epoch_frac, gscale=gscale, finetune=finetune)
                assert torch.equal(gs, gs2) and torch.equal(gp, gp2)
                ref_s, ref_p = R.gprob_autograd(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
                _, _, bound = R.gprob_closed_form(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune)
                es, ep = (gs.cpu().double() - ref_s).abs(), (gp.cpu().double() - ref_p).abs()
                print(f"gprob HW {HW} frac {epoch_frac} finetune {finetune} gscale {gscale}: err_s {es.tolist()} err_p {ep.tolist()} bound {bound.tolist()}")
                assert bool((es <= bound).all()) and bool((ep <= bound).all()), (epoch_frac, finetune, gscale)
                # D = 0 exactly, and the clamped images at epoch_frac 0.6: the target part is exactly 0
                zero = (2,) if not epoch_frac else (0, 1, 2, 3)
                assert all(float(gp[i]) == 0.0 for i in zero)


# ------------------------------------------------------------------------------------------------ 4. Discriminator.input_grad_features
def _disc_case(dim, fs, B, seed):
    gen = torch.Generator().manual_seed(seed)
    if dim == 16:
        sd = sub(load_golden("g6b_discriminator_features_step"), "disc0.")
    else:
        sd = R.init_feature_disc_state(dim, fs, gen)
        for k in sd:                                            # BatchNorm affines away from (1, 0)
            if k.endswith("layers.1.weight") or k.endswith("layers.1.bias"):
                sd[k] = sd[k] + 0.3 * torch.randn(sd[k].shape, generator=gen)
    d = Discriminator(CfgNode(dict(dim=dim, feature_size=fs, ema_weight=0.99, dis_use_features=True)))
    d.load_state_dict(sd, strict=True)
    mask_s = (torch.rand(B, 1, fs, fs, generator=gen) > 0.5).float()
    mask_p = (torch.rand(B, 1, fs, fs, generator=gen) > 0.5).float()
    feat = torch.randn(B, dim, fs, fs, generator=gen)
    r_s, r_p = torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    return d.to(DEV), sd, mask_s, mask_p, feat, r_s, r_p


def _bar(ref):
    return 1e-6 + 2e-3 * float(ref.abs().max())


@pytest.mark.parametrize("dim,fs,B", [(16, 12, 3), (8, 9, 2), (104, 9, 2)])
def test_input_grad_features_against_f64_autograd(dim, fs, B):
    from ucod_dpl_amd.engine.runner import TrainLoop
    d, sd, mask_s, mask_p, feat, r_s, r_p = _disc_case(dim, fs, B, seed=dim + fs)
    twin = copy.deepcopy(d)
    ms, mp, f = mask_s.to(DEV), mask_p.to(DEV), feat.to(DEV)
    p_s, rec_s = d.forward_features(ms, f, save="input")
    p_p, rec_p = d.forward_features(mp, f, save="input")
    # the saving forward is the frozen-backbone step's forward: same probabilities, running buffers and counters, bit for bit
    fake = types.SimpleNamespace(runner=types.SimpleNamespace(discriminator=twin), deterministic=False)
    q_s, q_p = TrainLoop._disc_probs(fake, ms, mp, f, fs)
    assert torch.equal(p_s, q_s) and torch.equal(p_p, q_p)
    for (k, a), (_, b) in zip(d.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(d.featureConv.layers[1].num_batches_tracked) == int(sd["featureConv.layers.1.num_batches_tracked"]) + 2
    for rec in (rec_s, rec_p):                                     # no unfold kept, nothing of maskConv
        assert rec["mask"] is None and all("cols" not in rec[k] for k in ("feat", "c0", "c1"))
    grs, grp = r_s.to(DEV), r_p.to(DEV)
    got = d.input_grad_features([rec_s, rec_p], [grs, grp])
    ref, probs = R.disc_linear_form_grad(sd, [mask_s, mask_p], feat, [r_s, r_p])
    assert maxdiff(p_s.cpu(), probs[0]) < 1e-5 and maxdiff(p_p.cpu(), probs[1]) < 1e-5
    print(f"input_grad_features dim {dim} fs {fs}: max err {maxdiff(got.cpu(), ref):.3e} bar {_bar(ref):.3e}")
    assert got.shape == (B, dim, fs, fs) and maxdiff(got.cpu(), ref) < _bar(ref)
    # the shared tail: summing the calls' cotangents before the feature block == running it per call and adding
    per_call = d.input_grad_features([rec_s], [grs]) + d.input_grad_features([rec_p], [grp])
    assert maxdiff(per_call.cpu(), got.cpu()) < _bar(ref)
    assert all(p.grad is None for p in d.parameters())
    assert torch.equal(d.input_grad_features([rec_s, rec_p], [grs, grp]), got)


def test_input_grad_features_allocates_no_unfold_sized_buffer():
    dim, fs, B = 64, 32, 4
    d, sd, mask_s, mask_p, feat, r_s, r_p = _disc_case(dim, fs, B, seed=1)
    ms, mp, f = mask_s.to(DEV), mask_p.to(DEV), feat.to(DEV)
    _, rec_s = d.forward_features(ms, f, save="input")
    _, rec_p = d.forward_features(mp, f, save="input")
    grs, grp = r_s.to(DEV), r_p.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = d.input_grad_features([rec_s, rec_p], [grs, grp])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"input_grad_features peak rise {rise} bytes; an unfold of the feature block is {B * 9 * dim * fs * fs * 4}")
    assert rise < B * 9 * dim * fs * fs * 4
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ 5. the module under autograd
def test_module_under_autograd_returns_the_feature_gradient():
    from oracle import discriminator as OD
    d, sd, mask_s, _, feat, r_s, _ = _disc_case(16, 12, 3, seed=2)
    ms, r = mask_s.to(DEV), r_s.to(DEV).view(-1, 1)
    ref, _ = R.disc_linear_form_grad(sd, [mask_s], feat, [r_s])
    # every parameter frozen: the autograd path is taken for the feature map alone
    f = feat.to(DEV).requires_grad_()
    (d(ms, f) * r).sum().backward()
    assert f.grad is not None and maxdiff(f.grad.cpu(), ref) < _bar(ref)
    assert all(p.grad is None for p in d.parameters())
    # every parameter trainable: the feature gradient AND the parameter gradients
    for p in d.parameters():
        p.requires_grad = True
    f = feat.to(DEV).requires_grad_()
    (d(ms, f) * r).sum().backward()
    assert maxdiff(f.grad.cpu(), ref) < _bar(ref)
    sd64 = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    prob = OD.discriminator_forward_with_features(mask_s.double(), feat.double(), dict(sd64)).reshape(-1)
    (prob * r_s.double()).sum().backward()
    for n, p in d.named_parameters():
        pref = sd64[n].grad
        assert maxdiff(p.grad.cpu(), pref) < 1e-6 + 2e-3 * pref.abs().max().item(), n
    # no gradient asked for: the plain forward
    with torch.no_grad():
        assert not d(ms, feat.to(DEV)).requires_grad


# ------------------------------------------------------------------------------------------------ 6. the step
def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _build_step(use_features, deterministic):
    from test_gpu_train_step import make_cfg
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine
    case = R.step_case()
    cfg = make_cfg(C=R.STEP_DIM, fs=R.STEP_FS)
    cfg.model_cfg["dis_use_features"] = use_features
    if deterministic:
        cfg.train_cfg["deterministic"] = True
    torch.manual_seed(3)
    runner = StandardRunner(cfg)
    runner.model.decoder.load_state_dict({k: v.to(runner.device) for k, v in case["dec"].items()}, strict=True)
    runner.model.decoder_ema.load_state_dict({k: v.to(runner.device) for k, v in case["ema"].items()}, strict=True)
    if use_features:
        runner.discriminator.load_state_dict({k: v.to(runner.device) for k, v in case["disc"].items()}, strict=True)
    loop = TrainLoop(runner.config, runner)
    base = {k: v for k, v in case["sd"].items() if ".lora_" not in k}
    eng = ViTLoRAEngine(base, heads=2, r=2, lora_alpha=4, device=DEV)
    eng.load_lora_state_dict(case["sd"])
    loop.attach_lora_backbone(eng)                               # (raised NotImplementedError with dis_use_features=True before the gradient existed)
    return case, runner, loop, eng


@functools.lru_cache(maxsize=None)
def _run_step(use_features=True, finetune=False, deterministic=False, tag=0):
    """one TrainLoop._process_batch_full from the fixed state -> everything the checks read, on the CPU (``tag`` tells repeated runs apart)"""
    case, runner, loop, eng = _build_step(use_features, deterministic)
    loop.finetune = finetune
    loss = loop._process_batch_full(case["x"], case["pl"])
    torch.cuda.synchronize()
    last = loop.last
    fs = R.STEP_FS
    B = case["x"].shape[0]
    pl = ops.bilinear_resize(case["pl"].to(DEV), fs, fs)          # the step's own launches on the same inputs: the same bits
    out = dict(case=case, loss=float(loss), keys=sorted(last.keys()), lora_grad=eng.lora_grad.detach().cpu().clone(), arena_g=runner.arena.g.detach().cpu().clone(),
               grads={k: v.detach().cpu() for k, v in eng.lora_state_dict(grads=True).items()},
               ws_bytes=sum(int(w.numel()) for w in eng._tside_ws if w is not None),
               pl=pl.view(B, -1).cpu(), mask_s=ops.binarize(last["fg"], logits=True).view(B, -1).cpu(), mask_p=ops.binarize(pl, logits=False).view(B, -1).cpu())
    for k in ("fg", "bg", "teacher", "p_s", "p_p", "w", "feat_s", "dfeat_disc"):
        if k in last:
            out[k] = last[k].detach().cpu().clone()
    return out


def _reference_dfeat_disc(o, finetune):
    """f64 autograd of S with respect to the step's own feat_s (native grid: through the f64 bilinear resize, whose adjoint autograd applies), fed the device's own
    fg, bg, teacher, pl and masks"""
    from oracle.resize import torch_bilinear
    fs, B = R.STEP_FS, o["fg"].shape[0]
    assert float(o["teacher"].abs().min()) > 1e-6                   # (no teacher logit within one rounding of the binarisation threshold)
    f = o["feat_s"].double().clone().requires_grad_(True)
    feats = torch_bilinear(f, fs, fs) if tuple(f.shape[-2:]) != (fs, fs) else f
    S, p_s, p_p = R.step_scalar_of_features(feats, o["case"]["disc"], o["mask_s"].view(B, 1, fs, fs), o["mask_p"].view(B, 1, fs, fs), o["fg"].view(B, -1),
                                            o["bg"].view(B, -1), o["teacher"].view(B, -1), o["pl"], 0.0, finetune)
    (g,) = torch.autograd.grad(S, f)
    return g, p_s.detach(), p_p.detach()


def test_step_discriminator_share_of_the_key_map_cotangent():
    o = _run_step(True, False)
    assert "feat_s" in o["keys"] and "dfeat_disc" in o["keys"]
    assert tuple(o["feat_s"].shape[-2:]) == (5, 5) and o["dfeat_disc"].shape == o["feat_s"].shape      # the key map's own (native) grid
    ref, p_s, p_p = _reference_dfeat_disc(o, False)
    assert maxdiff(o["p_s"], p_s) < 1e-4 and maxdiff(o["p_p"], p_p) < 1e-4
    u = 0.5 * (1 + torch.cos(torch.pi * (p_s - p_p).abs()))
    assert bool(((u > 0) & (u < 1)).any()), u                       # the target path is live on the reference's values
    print(f"step dfeat_disc: max err {maxdiff(o['dfeat_disc'], ref):.3e} bar {_bar(ref):.3e} |ref|max {float(ref.abs().max()):.3e}; u {u.tolist()}")
    assert maxdiff(o["dfeat_disc"], ref) < _bar(ref)


def test_step_in_finetune_keeps_the_target_part_only():
    o, o0 = _run_step(True, True), _run_step(True, False)
    ref, _, _ = _reference_dfeat_disc(o, True)
    assert float(ref.abs().max()) > 0
    print(f"step dfeat_disc (finetune): max err {maxdiff(o['dfeat_disc'], ref):.3e} bar {_bar(ref):.3e}")
    assert maxdiff(o["dfeat_disc"], ref) < _bar(ref)
    assert maxdiff(o["dfeat_disc"], o0["dfeat_disc"]) > _bar(ref)   # the dis_loss part is gone
    assert torch.equal(o["p_s"], o0["p_s"]) and torch.equal(o["feat_s"], o0["feat_s"])


@pytest.mark.parametrize("finetune", [False, True])
def test_step_lora_gradients_against_f64_autograd_of_the_whole_step(finetune):
    """8e-2 rel-L2, the bar of test_gpu_vit_train.py::test_fused_full_step_against_oracle.  Without the discriminator's term the reference itself is an order of
    magnitude outside it (tests/test_disc_feature_grad_host.py: layer 1's key.lora_A / query.lora_A)."""
    o = _run_step(True, finetune)
    B, fs = o["fg"].shape[0], R.STEP_FS
    ref = R.full_step_lora_grads(o["case"], finetune=finetune, masks=(o["mask_s"], o["mask_p"], R.binarize_teacher(o["teacher"].view(B, -1))))
    assert abs(o["loss"] - float(ref["loss"])) < 2e-2 * max(1.0, abs(float(ref["loss"])))
    checked = 0
    for k, g in ref["grads"].items():
        if float(g.abs().max()) == 0.0:
            assert float(o["grads"][k].abs().max()) == 0.0, k
        else:
            print(f"step LoRA grad {k}: rel-L2 {rel_l2(o['grads'][k], g):.3e}")
            assert rel_l2(o["grads"][k], g) < 8e-2, (k, rel_l2(o["grads"][k], g))
            checked += 1
    assert checked >= 14


def test_step_is_bit_identical_run_to_run():
    a, b = _run_step(True, False, True, 0), _run_step(True, False, True, 1)
    assert torch.equal(a["dfeat_disc"], b["dfeat_disc"]) and torch.equal(a["lora_grad"], b["lora_grad"]) and torch.equal(a["arena_g"], b["arena_g"])
    assert float(a["lora_grad"].abs().max()) > 0


def test_step_without_the_feature_branch_never_enters_the_new_path(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("dis_use_features=False must not reach the feature-gradient path")
    for name in ("apm_bce_gprob", "conv3x3", "conv3x3_dgrad_weights"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(Discriminator, "input_grad_features", refuse)
    monkeypatch.setattr(Discriminator, "forward_features", refuse)
    a, b = _run_step(False, False, True, 0), _run_step(False, False, True, 1)
    assert "feat_s" not in a["keys"] and "dfeat_disc" not in a["keys"]
    assert a["loss"] == b["loss"] and torch.equal(a["lora_grad"], b["lora_grad"]) and torch.equal(a["arena_g"], b["arena_g"])
    assert a["ws_bytes"] == b["ws_bytes"] > 0
    # the same step WITH the feature branch: the same backbone workspace, another LoRA gradient
    monkeypatch.undo()
    c = _run_step(True, False, True, 0)
    assert c["ws_bytes"] == a["ws_bytes"] and not torch.equal(c["lora_grad"], a["lora_grad"])
