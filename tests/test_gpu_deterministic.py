"""GPU: the deterministic forms of the training step (include/ucod_dpl.h, "Deterministic forms"): no floating-point atomics, every reduction an ordered sum of
per-workgroup partials.  Kernel by kernel -- repeatable bits, the documented order read back from the workspace, the outputs the default forms compute without
an atomic bit-identical to theirs, accuracy held to the bounds the default forms are held to -- and the whole step: two freshly built runners are torch.equal."""
import ctypes as C

import pytest
import torch

from conftest import load_golden, sub, maxdiff
import train_ref as TR

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops  # noqa: E402
from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
P = N.ptr
GUARD = 4096                       # bytes behind ws_bytes that no kernel may touch
GUARD_BYTE = 0xA5


def guarded_ws(nbytes):
    assert nbytes > 0
    return torch.full((nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)


def guard_intact(ws, nbytes):
    return bool((ws[nbytes:] == GUARD_BYTE).all())


def ordered_sum(planes, start=None):
    """((start + planes[0]) + planes[1]) + ... in f32 on the host: the documented order of the deterministic reductions"""
    s = torch.zeros_like(planes[0]) if start is None else start.clone()
    for q in range(planes.shape[0]):
        s = s + planes[q]
    return s


def within_tr(tag, kernel, r64, r32, slices):
    ek, e32 = TR.compare(kernel, r64, r32, slices)
    i, k, b = TR.worst(ek, e32)
    print(f"{tag}: worst slice {i} e_k {k:.3e} bound {b:.3e}")
    assert bool((e32 <= TR.CAP).all()), (tag, float(e32.max()))
    assert TR.passes(ek, e32), (tag, i, k, b)


# ----------------------------------------------------------------------------------------------------------- weight gradient
WGRAD_SHAPES = [(3, 48, 1369), (2, 256, 4624), (8, 768, 1369)]


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("B,Cc,HW", WGRAD_SHAPES)
def test_wgrad_det(B, Cc, HW, exact):
    lib = N.load()
    g = torch.Generator().manual_seed(5 + B + Cc)
    gd = torch.randn(B, 128, HW, generator=g).to(DEV)
    x = torch.randn(B, Cc, HW, generator=g).to(DEV)
    need = lib.ucod_dba_wgrad_det_workspace_bytes(B, Cc, HW, exact)
    plane = 128 * Cc
    assert need > 0 and need % (4 * plane) == 0
    Q = need // (4 * plane)
    assert Q % B == 0                                         # Q = B * nchunk
    ws = guarded_ws(need)

    def run(fill):
        gW = torch.full((128, Cc), fill, device=DEV)
        N.check(lib.ucod_dba_wgrad_det(P(gd), P(x), P(gW), B, Cc, HW, exact, P(ws), need, N.stream()), "ucod_dba_wgrad_det")
        return gW

    outs = [run(0.0) for _ in range(5)]                        # (a)
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert torch.equal(run(float("nan")), outs[0])             # (b)
    with ops.prezeroed():
        assert torch.equal(run(float("nan")), outs[0]) and torch.equal(run(0.0), outs[0])
    planes = ws[:need].view(torch.float32).view(Q, 128, Cc).cpu()    # (c)
    assert torch.equal(outs[0].cpu(), ordered_sum(planes))
    ref = gd.double().transpose(0, 1).reshape(128, -1) @ x.double().transpose(0, 1).reshape(Cc, -1).t()     # (d)
    err = maxdiff(outs[0].cpu(), ref.cpu()) / ref.abs().max().item()
    print(f"wgrad_det B{B} C{Cc} HW{HW} exact{exact}: Q {Q}, error vs f64 {err:.3e}")
    assert err <= 2e-5
    assert guard_intact(ws, need)                              # (e)
    # (f) refusals leave the outputs unwritten
    gW = torch.full((128, Cc), 7.0, device=DEV)
    ws2 = guarded_ws(need)
    assert lib.ucod_dba_wgrad_det(P(gd), P(x), P(gW), B, Cc, HW, exact, P(ws2), need - 4, N.stream()) == -1
    assert lib.ucod_dba_wgrad_det(None, P(x), P(gW), B, Cc, HW, exact, P(ws2), need, N.stream()) == -1
    assert lib.ucod_dba_wgrad_det(P(gd), None, P(gW), B, Cc, HW, exact, P(ws2), need, N.stream()) == -1
    assert lib.ucod_dba_wgrad_det(P(gd), P(x), None, B, Cc, HW, exact, P(ws2), need, N.stream()) == -1
    assert lib.ucod_dba_wgrad_det(P(gd), P(x), P(gW), B, Cc, HW, exact, None, need, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((gW == 7.0).all()) and bool((ws2 == GUARD_BYTE).all())
    # the wrapper takes the same kernel choice as the default form and gives the same bits as the entry point
    assert torch.equal(ops.dba_wgrad(gd, x, exact=bool(exact), deterministic=True), outs[0])


def test_conv_wgrad_f32_det_accumulates_onto_a_known_gradient():
    lib = N.load()
    B, Cc, HW, Nout = 2, 144, 36, 200
    g = torch.Generator().manual_seed(17)
    gd = torch.randn(B, Nout, HW, generator=g).to(DEV)
    cols = torch.randn(B, Cc, HW, generator=g).to(DEV)
    cols[:, 140:] = 0.0                                        # the zero rows of the padded unfold
    base = torch.randn(Nout, Cc, generator=g)
    need = lib.ucod_conv_wgrad_f32_det_workspace_bytes(B, Cc, HW, Nout)
    Q = need // (4 * Nout * Cc)
    assert need == Q * 4 * Nout * Cc and Q % B == 0
    ws = guarded_ws(need)
    outs = {}
    for acc in (0, 1):
        gW = base.clone().to(DEV) if acc else torch.full((Nout, Cc), float("nan"), device=DEV)
        N.check(lib.ucod_conv_wgrad_f32_det(P(gd), P(cols), P(gW), B, Cc, HW, Nout, acc, P(ws), need, N.stream()), "ucod_conv_wgrad_f32_det")
        outs[acc] = gW.cpu()
        planes = ws[:need].view(torch.float32).view(Q, Nout, Cc).cpu()
        assert torch.equal(outs[acc], ordered_sum(planes, base if acc else None)), acc
    assert guard_intact(ws, need)
    ref = gd.double().transpose(0, 1).reshape(Nout, -1) @ cols.double().transpose(0, 1).reshape(Cc, -1).t()
    assert maxdiff(outs[0], ref.cpu()) <= 2e-5 * ref.abs().max().item()
    gW = torch.full((Nout, Cc), 7.0, device=DEV)
    assert lib.ucod_conv_wgrad_f32_det(P(gd), P(cols), P(gW), B, Cc, HW, Nout, 0, P(ws), need - 4, N.stream()) == -1
    assert lib.ucod_conv_wgrad_f32_det(P(gd), P(cols), P(gW), B, Cc, HW, 0, 0, P(ws), need, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((gW == 7.0).all())


# ----------------------------------------------------------------------------------------------------------- decoder: heads and backward
_DECODER = {}


def decoder_case(H):
    """One small decoder case per map size (B = 3, C = 48), its f64 / f32 autograd references (tests/train_ref.py) and the default forms' outputs, computed once."""
    if H not in _DECODER:
        case = dict(id=f"det_b3_c48_h{H}", B=3, C=48, H=H, exact=(None,), clamp=False, c0=0)
        inp = TR.decoder_inputs(case)
        r64, r32 = TR.decoder_ref(inp, 0, F64), TR.decoder_ref(inp, 0, F32)
        t = {k: inp[k].to(DEV) for k in ("x", "W", "b", "emb", "head_w", "head_b")}
        d = ops.dba_project(t["x"], t["W"], t["b"])
        norm = ops.dba_colnorm(d, 0, t["emb"])
        fg, bg, sdiag = ops.dba_heads(d, 0, t["emb"], norm, t["head_w"], t["head_b"], want_sdiag=True)
        _, gram = ops.orth_gram(d, 0, t["emb"], norm, sdiag)
        _DECODER[H] = dict(case=case, inp=inp, r64=r64, r32=r32, t=t, d=d, norm=norm, fg=fg, bg=bg, sdiag=sdiag, gram=gram)
    return _DECODER[H]


@pytest.mark.parametrize("H", [37, 68])                        # HW = 1369 (6 workgroups, the last ragged) and 4624
def test_heads_det(H):
    lib = N.load()
    c = decoder_case(H)
    t, d, norm = c["t"], c["d"], c["norm"]
    B, HW = 3, H * H
    need = lib.ucod_dba_heads_fwd_det_workspace_bytes(B, HW)
    nblk = (HW + 255) // 256
    assert need == B * nblk * 4
    ws = guarded_ws(need)
    runs = []
    for _ in range(5):
        fg, bg, sdiag = ops.dba_heads(d, 0, t["emb"], norm, t["head_w"], t["head_b"], want_sdiag=True, sdiag=torch.full((B,), float("nan"), device=DEV),
                                      deterministic=True, ws=ws)
        runs.append((fg, bg, sdiag))
    assert all(torch.equal(r[2], runs[0][2]) for r in runs[1:])
    assert torch.equal(runs[0][0], c["fg"]) and torch.equal(runs[0][1], c["bg"])
    part = ws[:need].view(torch.float32).view(B, nblk).cpu()
    assert torch.equal(runs[0][2].cpu(), ordered_sum(part.t().contiguous()))
    assert guard_intact(ws, need)
    within_tr(f"det/heads/h{H}/sdiag", runs[0][2].cpu(), c["r64"]["sdiag"], c["r32"]["sdiag"], TR.DECODER_FWD_SLICES["sdiag"])
    within_tr(f"det/heads/h{H}/sdiag_default", c["sdiag"].cpu(), c["r64"]["sdiag"], c["r32"]["sdiag"], TR.DECODER_FWD_SLICES["sdiag"])
    # without sdiag no workspace is needed; a workspace that is too small is refused with the outputs unwritten
    fg, _, _ = ops.dba_heads(d, 0, t["emb"], norm, t["head_w"], t["head_b"], want_bg=False, deterministic=True)
    assert torch.equal(fg, c["fg"])
    fg7, sd7 = torch.full((B, HW), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    assert lib.ucod_dba_heads_fwd_det(P(d), 128, 0, P(t["emb"]), P(norm), P(t["head_w"]), P(t["head_b"]), P(fg7), None, P(sd7), P(ws), need - 4, B, HW,
                                      N.stream()) == -1
    assert lib.ucod_dba_heads_fwd_det(P(d), 128, 0, P(t["emb"]), P(norm), P(t["head_w"]), P(t["head_b"]), P(fg7), None, P(sd7), None, need, B, HW,
                                      N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((fg7 == 7.0).all()) and bool((sd7 == 7.0).all())


@pytest.mark.parametrize("H", [37, 68])
def test_dba_bwd_det(H):
    lib = N.load()
    c = decoder_case(H)
    t, d, norm, gram = c["t"], c["d"], c["norm"], c["gram"]
    B, HW = 3, H * H
    need = lib.ucod_dba_bwd_det_workspace_bytes(B, HW)
    assert need == lib.ucod_dba_bwd_workspace_bytes(B, HW) + B * 258 * 4
    zero = torch.zeros(B, HW, device=DEV)
    for mode, (gfg, gbg, gextra) in c["inp"]["modes"].items():
        gfg_d = zero if gfg is None else gfg.to(DEV)
        gbg_d = zero if gbg is None else gbg.to(DEV)
        gd0, _, _, _ = ops.dba_bwd(d, 0, t["emb"], norm, t["head_w"], gram, gfg_d, gbg_d, gextra)
        ws = guarded_ws(need)
        runs = []
        for fill in (float("nan"), 0.0, 7.0):
            arena = torch.full((258,), fill, device=DEV)
            out = ops.dba_bwd(d, 0, t["emb"], norm, t["head_w"], gram, gfg_d, gbg_d, gextra, g_dec_bias=arena[:128], g_head_w=arena[128:256].view(2, 64),
                              g_head_b=arena[256:258], deterministic=True, ws=ws)
            runs.append((out[0], arena))
        assert all(torch.equal(r[1], runs[0][1]) for r in runs[1:]), mode
        assert torch.equal(runs[0][0], gd0), mode
        part = ws[need - B * 258 * 4:need].view(torch.float32).view(B, 258).cpu()
        assert torch.equal(runs[0][1].cpu(), ordered_sum(part)), mode
        assert guard_intact(ws, need)
        a = runs[0][1].cpu()
        got = dict(g_dec_bias=a[:128], g_head_w=a[128:256].view(2, 64), g_head_b=a[256:258])
        for k in ("g_dec_bias", "g_head_w", "g_head_b"):
            within_tr(f"det/dba_bwd/h{H}/{mode}/{k}", got[k], c["r64"][mode][k], c["r32"][mode][k], TR.DECODER_BWD_SLICES[k])
    a7 = torch.full((258,), 7.0, device=DEV)
    gd7 = torch.full((B, 128, HW), 7.0, device=DEV)
    assert lib.ucod_dba_bwd_det(P(d), 128, 0, P(t["emb"]), P(norm), P(t["head_w"]), P(gram), P(zero), P(zero), 1.0, P(gd7), P(a7[128:256]), P(a7[256:]),
                                P(a7[:128]), P(ws), need - 4, B, HW, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((a7 == 7.0).all()) and bool((gd7 == 7.0).all())


# ----------------------------------------------------------------------------------------------------------- APM
def apm_inputs(B, HW):
    g = torch.Generator().manual_seed(31 + B + HW)
    pl = torch.rand(B, HW, generator=g)
    teacher, fg, bg = (2 * torch.randn(B, HW, generator=g) for _ in range(3))
    return dict(pl=pl, teacher=teacher, fg=fg, bg=bg, p_s=torch.rand(B, generator=g), p_p=torch.rand(B, generator=g))


@pytest.mark.parametrize("HW", [144, 4624])
@pytest.mark.parametrize("B", [5, 32])
def test_apm_bce_det(B, HW):
    lib = N.load()
    inp = apm_inputs(B, HW)
    frac = 0.5
    r64, r32 = TR.apm_ref(inp, frac, TR.APM_GSCALE, F64), TR.apm_ref(inp, frac, TR.APM_GSCALE, F32)
    d = {k: v.to(DEV) for k, v in inp.items()}
    args = (d["pl"], d["teacher"], d["fg"], d["bg"], d["p_s"], d["p_p"], frac)
    w0, merged0, gfg0, gbg0, _ = ops.apm_bce(*args, gscale=TR.APM_GSCALE)
    need = lib.ucod_apm_bce_det_workspace_bytes(B)
    assert need == B * 3 * 4
    ws = guarded_ws(need)
    runs = [ops.apm_bce(*args, gscale=TR.APM_GSCALE, losses=torch.full((4,), float("nan"), device=DEV), deterministic=True, ws=ws) for _ in range(20)]
    assert all(torch.equal(r[4], runs[0][4]) for r in runs[1:])
    w, merged, gfg, gbg, losses = runs[0]
    assert torch.equal(w, w0) and torch.equal(merged, merged0) and torch.equal(gfg, gfg0) and torch.equal(gbg, gbg0)
    part = ws[:need].view(torch.float32).view(B, 3).cpu()
    ls = losses.cpu()
    assert torch.equal(ls[:3], ordered_sum(part)) and float(ls[3]) == 0.0
    assert guard_intact(ws, need)
    for i, k in enumerate(("l1", "l2", "l3")):
        within_tr(f"det/apm_bce/b{B}_hw{HW}/{k}", ls[i:i + 1], r64[k], r32[k], TR.APM_SLICES[k])
    l7 = torch.full((4,), 7.0, device=DEV)
    assert lib.ucod_apm_bce_det(P(d["pl"]), P(d["teacher"]), P(d["fg"]), P(d["bg"]), P(d["p_s"]), P(d["p_p"]), frac, 1.0, P(w), P(merged), P(gfg), P(gbg),
                                P(l7), P(ws), need - 4, B, HW, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((l7 == 7.0).all())


# ----------------------------------------------------------------------------------------------------------- discriminator
def _disc_tensors(sd):
    t = {k: sd[v].clone().float().contiguous().to(DEV) for k, v in TR.DISC_NAMES.items()}
    t["nbt"] = torch.tensor([int(sd[k]) for k in TR.NBT_KEYS], dtype=torch.int64, device=DEV)
    return t


def _disc_two_calls(sd, masks, gprobs, fs, B, deterministic):
    """pseudo label, then student (forward + backward each, the second backward accumulating) from the state ``sd`` -> everything the calls leave behind"""
    lib = N.load()
    t = _disc_tensors(sd)
    grads = [torch.full(t["lin_w"].shape if shp is None else shp, float("nan"), device=DEV) for _, shp in ops.DISC_GRAD_SHAPES]
    s2 = (fs - 1) // 2 + 1
    s3 = (s2 - 1) // 2 + 1
    nstat = B * (32 * fs * fs + 16 * s2 * s2 + 8 * s3 * s3) + 112     # y1 | y2 | y3 | (mean, rstd) of the three layers, as floats
    assert 4 * nstat + 112 * 8 <= lib.ucod_disc_saved_bytes(B, fs)
    out = dict(prob=[], saved=[])
    kw = dict(deterministic=True) if deterministic else {}
    for c in range(2):
        prob, saved = ops.disc_fwd(masks[c], t, **kw)
        ops.disc_bwd(masks[c], t, saved, gprobs[c], grads, accumulate=c == 1, **kw)
        out["prob"].append(prob)
        out["saved"].append(saved[:4 * nstat].view(torch.float32).clone())
    out["running"] = {k: t[k] for k in TR.DISC_RUNNING}
    out["nbt"] = t["nbt"]
    out["grads"] = grads
    return out


@pytest.mark.parametrize("fs", [12, 20])
def test_discriminator_det(fs):
    lib = N.load()
    B = 3
    sd, masks, gprobs = TR.disc_inputs(fs, B)
    m_d, gp_d = [m.to(DEV) for m in masks], [g.to(DEV) for g in gprobs]
    a = _disc_two_calls(sd, m_d, gp_d, fs, B, True)
    b = _disc_two_calls(sd, m_d, gp_d, fs, B, True)
    dflt = _disc_two_calls(sd, m_d, gp_d, fs, B, False)
    nbt0 = [int(sd[k]) for k in TR.NBT_KEYS]
    assert a["nbt"].cpu().tolist() == dflt["nbt"].cpu().tolist() == [n + 2 for n in nbt0]
    for c in range(2):
        assert torch.equal(a["prob"][c], b["prob"][c]) and torch.equal(a["saved"][c], b["saved"][c]), c
        assert maxdiff(a["prob"][c].cpu(), dflt["prob"][c].cpu()) < 2e-5
        assert maxdiff(a["saved"][c][-112:].cpu(), dflt["saved"][c][-112:].cpu()) < 2e-5 * max(1.0, dflt["saved"][c][-112:].abs().max().item())
    for k in TR.DISC_RUNNING:
        assert torch.equal(a["running"][k], b["running"][k]), k
        assert maxdiff(a["running"][k].cpu(), dflt["running"][k].cpu()) < 2e-5, k
    for (name, _), ga, gb, g0 in zip(ops.DISC_GRAD_SHAPES, a["grads"], b["grads"], dflt["grads"]):
        assert torch.equal(ga, gb), name
        assert maxdiff(ga.cpu(), g0.cpu()) < 1e-6 + 2e-3 * g0.abs().max().item(), name
    # held to the f64 autograd reference like the default form (tests/test_gpu_train_kernels.py)
    r64, r32 = TR.disc_ref(sd, masks, gprobs, F64), TR.disc_ref(sd, masks, gprobs, F32)
    for c in range(2):
        within_tr(f"det/disc/fs{fs}/call{c}/prob", a["prob"][c].cpu(), r64["prob"][c], r32["prob"][c], 0)
    for name, g in zip(TR.DISC_GRADS, a["grads"]):
        within_tr(f"det/disc/fs{fs}/grad/{name}", TR.disc_grad_view(name, g.cpu(), fs), TR.disc_grad_view(name, r64["grads"][name], fs),
                  TR.disc_grad_view(name, r32["grads"][name], fs), TR.DISC_GRAD_SLICES.get(name, 0))
    # the two forms alternate on ONE zero-allocated saved buffer under ops.prezeroed(): the deterministic form leaves the f64 sums at its end zero
    saved = torch.zeros(lib.ucod_disc_saved_bytes(B, fs), dtype=torch.uint8, device=DEV)
    t = _disc_tensors(sd)
    with ops.prezeroed():
        p_det, _ = ops.disc_fwd(m_d[0], t, saved=saved, deterministic=True)
        assert bool((saved[-112 * 8:] == 0).all())
        p_dflt, _ = ops.disc_fwd(m_d[1], t, saved=saved)
        assert bool((saved[-112 * 8:] == 0).all())
        p_det2, _ = ops.disc_fwd(m_d[1], _disc_tensors(sd), saved=saved, deterministic=True)
    assert torch.equal(p_det, a["prob"][0])
    assert maxdiff(p_dflt.cpu(), dflt["prob"][1].cpu()) < 1e-6
    # refusals
    need = lib.ucod_disc_fwd_det_workspace_bytes(B, fs)
    ws = guarded_ws(need)
    ps = ops.disc_params_struct(t)
    prob7 = torch.full((B,), 7.0, device=DEV)
    assert lib.ucod_disc_fwd_det(P(m_d[0]), C.byref(ps), P(prob7), P(saved), B, fs, 1, P(ws), need - 8, N.stream()) == -1
    assert lib.ucod_disc_fwd_det(P(m_d[0]), C.byref(ps), P(prob7), P(saved), B, fs, 1, None, need, N.stream()) == -1
    N.check(lib.ucod_disc_fwd_det(P(m_d[0]), C.byref(ps), P(prob7), P(saved), B, fs, 0, P(ws), need, N.stream()), "ucod_disc_fwd_det")
    torch.cuda.synchronize()
    assert guard_intact(ws, need) and not bool((prob7 == 7.0).any())


# ----------------------------------------------------------------------------------------------------------- whole steps
def _g18_runner(g, deterministic):
    from test_deterministic_host import g18_cfg
    runner = StandardRunner(g18_cfg(deterministic=True) if deterministic else g18_cfg())
    runner.model.load_state_dict({k: v.to(runner.device) for k, v in sub(g, "model0.").items()}, strict=True)
    runner.discriminator.load_state_dict({k: v.to(runner.device) for k, v in sub(g, "disc0.").items()}, strict=True)
    loop = TrainLoop(runner.config, runner)
    assert loop.deterministic is deterministic
    return runner, loop


def _frozen_steps(g, deterministic):
    """three _process_batch steps and one _discriminator_batch from the G18 initial state -> every tensor the steps leave behind"""
    runner, loop = _g18_runner(g, deterministic)
    lasts, grads = [], []
    for i in range(3):
        batch = {"pseudo_label": g[f"pl{i}"], "label_tensor": torch.zeros(1), "features": g[f"features{i}"], "img_path": ["x"]}
        loop._process_batch(batch)
        loop.global_step += 1
        lasts.append({k: v.clone() for k, v in loop.last.items()})
        grads.append(runner.arena.g.clone())
    loop._discriminator_batch({"pseudo_label": g["pl0"], "label_tensor": torch.zeros(1), "features": g["features0"], "img_path": ["x"]})
    lasts.append({k: v.clone() for k, v in loop.last.items()})
    torch.cuda.synchronize()
    A, DA = runner.arena, runner.disc_arena
    return dict(p=A.p.clone(), ema=A.ema.clone(), m=A.m.clone(), v=A.v.clone(), dp=DA.p.clone(), dg=DA.g.clone(), dm=DA.m.clone(), dv=DA.v.clone(),
                disc={k: v.clone() for k, v in runner.discriminator.state_dict().items()}, lasts=lasts, grads=grads,
                lr=runner.optimizer.param_groups[0]["lr"])


def test_frozen_step_is_bit_reproducible():
    g = load_golden("g18_train_schedule")
    a, b = _frozen_steps(g, True), _frozen_steps(g, True)
    for k in ("p", "ema", "m", "v", "dp", "dg", "dm", "dv"):
        assert torch.equal(a[k], b[k]), k
    assert sorted(a["disc"]) == sorted(b["disc"]) and all(torch.equal(a["disc"][k], b["disc"][k]) for k in a["disc"])
    for i, (la, lb) in enumerate(zip(a["lasts"], b["lasts"])):
        assert sorted(la) == sorted(lb)
        for k in la:
            assert torch.equal(la[k], lb[k]), (i, k)
    for ga, gb in zip(a["grads"], b["grads"]):
        assert torch.equal(ga, gb)
    # against the default (atomic) step, to the tolerances of tests/test_gpu_train_step.py::test_process_batch_three_steps_match_reference
    d = _frozen_steps(g, False)
    C_ = 128
    oW, ob = 128, 128 + 128 * C_
    noisy = torch.zeros(128 * C_, dtype=torch.bool, device=DEV)
    for i in range(3):
        assert abs(a["lasts"][i]["loss"].item() - d["lasts"][i]["loss"].item()) < 2e-5, i
        ref_gw = d["grads"][i][oW:ob]
        assert maxdiff(a["grads"][i][oW:ob].cpu(), ref_gw.cpu()) < 2e-3 * ref_gw.abs().max().item(), i
        noisy = noisy | (ref_gw.abs() < 1e-4 * ref_gw.abs().max())
    assert int(noisy.sum()) < 0.02 * noisy.numel()
    for k in ("p", "ema"):
        ours, ref = a[k], d[k]
        assert maxdiff(ours[oW:ob][~noisy].cpu(), ref[oW:ob][~noisy].cpu()) < 5e-5, k
        assert maxdiff(ours[oW:ob].cpu(), ref[oW:ob].cpu()) < 2.0 * 6e-4 * 3, k
        assert maxdiff(ours[ob:].cpu(), ref[ob:].cpu()) < 5e-5 and maxdiff(ours[:oW].cpu(), ref[:oW].cpu()) < 5e-5, k
    for k, v in d["disc"].items():
        if "num_batches" in k:
            assert torch.equal(a["disc"][k], v), k
            continue
        tol = 3e-4 if ("running_mean" in k or "running_var" in k) else 2e-3
        assert maxdiff(a["disc"][k].cpu(), v.cpu()) < tol, (k, maxdiff(a["disc"][k].cpu(), v.cpu()))


def _lora_steps(tmp_path, tag):
    from test_gpu_lora_merge import model_case, runner_cfg
    from test_gpu_lora_targets import targeted_engine
    _, sd, heads, img, _, _ = model_case("gelu")
    path = tmp_path / tag
    path.mkdir()
    cfg = runner_cfg(path, sd)
    cfg.train_cfg["deterministic"] = True
    torch.manual_seed(3)
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    assert loop.deterministic is True
    eng = targeted_engine(sd, heads, ["query", "key", "value", "fc1"])
    loop.attach_lora_backbone(eng)
    pl = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(11)) > 0.5).float()
    losses = []
    for _ in range(2):
        losses.append(loop._process_batch_full(img, pl).clone())
        losses.append(loop.last["dis_loss"].clone())
        losses.append(loop.last["extra"].clone())
    torch.cuda.synchronize()
    return dict(lora=eng.lora.clone(), lora_ema=loop.lora_engine_ema.lora.clone(), p=runner.arena.p.clone(), ema=runner.arena.ema.clone(),
                g=runner.arena.g.clone(), losses=losses)


def test_lora_step_is_bit_reproducible(tmp_path):
    a, b = _lora_steps(tmp_path, "a"), _lora_steps(tmp_path, "b")
    for k in ("lora", "lora_ema", "p", "ema", "g"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["losses"], b["losses"]))
    assert all(bool(torch.isfinite(x).all()) for x in a["losses"])


def _feature_branch_batch(g):
    from test_gpu_train_step import make_cfg
    cfg = make_cfg()
    cfg.model_cfg["dim"], cfg.model_cfg["feature_size"], cfg.model_cfg["dis_use_features"] = 16, 12, True
    cfg.train_cfg["deterministic"] = True
    runner = StandardRunner(cfg)
    runner.model.load_state_dict({k: v.to(runner.device) for k, v in sub(g, "model0.").items()}, strict=True)
    runner.discriminator.load_state_dict({k: v.to(runner.device) for k, v in sub(g, "disc0.").items()}, strict=True)
    loop = TrainLoop(runner.config, runner)
    assert loop.deterministic is True and runner.discriminator.use_features
    loss = loop._discriminator_batch({"pseudo_label": g["pl"], "label_tensor": torch.zeros(1), "features": g["features"], "img_path": ["x"]})
    torch.cuda.synchronize()
    return loss.clone(), [v.clone() for v in runner.disc_arena.grad_views], runner.disc_arena.p.clone()


def test_feature_branch_discriminator_batch_is_bit_reproducible():
    g = load_golden("g6b_discriminator_features_step")
    la, ga, pa = _feature_branch_batch(g)
    lb, gb, pb = _feature_branch_batch(g)
    assert len(ga) == 14 and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    ref = g["grad.maskConv.layers.0.weight"]                    # and still the reference's gradients (tests/test_gpu_train_step.py, G6b)
    assert maxdiff(ga[0].cpu(), ref) < 1e-6 + 2e-3 * ref.abs().max().item()
