"""GPU: the decoder (DBA) and discriminator (APM) training kernels against f64 AUTOGRAD of the oracle (tests/train_ref.py), at the step's sizes.

Every compared slice must satisfy  e_k <= 8 * max(e_32, 2^-23)  with e_32 the f32 reference's own error on that exact case (train_ref's
docstring: why a factor of 8, why per-slice normalisation), and e_32 <= 1e-4 (the cap: test_train_ref.py).  The worst slice of every
(case, output family) is recorded through conftest.within (profiles/r08_train_kernels_tolerance_audit.jsonl).

Decoder chain dba_project -> dba_colnorm -> dba_heads(want_sdiag) -> orth_gram -> dba_bwd -> dba_wgrad on every train_ref.DECODER_CASES
entry (Gram tails: HW = 529 / 1369 / 4624 = 2 / 3 / 10 chunks of 512, the 16-pixel tail workgroup of dba_bwd_a_kernel at 4624; the clamped-norm
branch; the teacher half c0 = 128 of a 256-row projection), with the gate term, the orthogonality term and both as separate upstream
gradients, and three gradient-buffer layouts: separate tensors, the flat arena g_dec_bias | g_head_w | g_head_b, and caller-zeroed buffers
under ops.prezeroed().  Discriminator: two calls (pseudo label, then student) accumulated into one gradient set, and two forward calls
reusing one zero-allocated `saved` buffer under ops.prezeroed().  Losses: disc_bce at the clamps, apm_bce at the headline size, step_loss
bit for bit.
"""
import pytest
import torch

from conftest import within
import train_ref as TR

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
SENTINEL = 7.0          # what the outputs the entry points must zero themselves hold before the call


class Checker:
    """Compares families slice by slice, records each family's worst slice through conftest.within, and collects failures so that one
    test reports every family it measured before it fails."""

    def __init__(self):
        self.failures = []

    def __call__(self, tag, kernel, r64, r32, slices):
        ek, e32 = TR.compare(kernel, r64, r32, slices)
        if not bool((e32 <= TR.CAP).all()):
            self.failures.append((tag, "cap", float(e32.max())))
        i, k, b = TR.worst(ek, e32)
        print(f"{tag}: worst slice {i} e_k {k:.3e} bound {b:.3e} (e_32 {float(e32[i]):.3e})")
        ok = TR.passes(ek, e32)
        try:
            within(tag, k, b)
        except AssertionError:
            ok = False
        if not ok:
            self.failures.append((tag, i, k, b))

    def done(self):
        assert not self.failures, self.failures


# ----------------------------------------------------------------------------------------------------------- decoder
def _bwd(layout, d, c0, emb, norm, hw, gram, gfg, gbg, gextra):
    if layout == "separate":
        gw, gb, gdb = (torch.full(s, SENTINEL, device=DEV) for s in ((2, 64), (2,), (128,)))
        return ops.dba_bwd(d, c0, emb, norm, hw, gram, gfg, gbg, gextra, g_head_w=gw, g_head_b=gb, g_dec_bias=gdb)
    arena = torch.full((258,), SENTINEL, device=DEV) if layout == "arena" else torch.zeros(258, device=DEV)
    views = dict(g_dec_bias=arena[:128], g_head_w=arena[128:256].view(2, 64), g_head_b=arena[256:258])
    if layout == "arena":
        return ops.dba_bwd(d, c0, emb, norm, hw, gram, gfg, gbg, gextra, **views)
    with ops.prezeroed():
        return ops.dba_bwd(d, c0, emb, norm, hw, gram, gfg, gbg, gextra, **views)


@pytest.mark.parametrize("case", TR.DECODER_CASES, ids=[c["id"] for c in TR.DECODER_CASES])
def test_decoder_chain_against_f64_autograd(case):
    inp = TR.decoder_inputs(case)
    c0, B = case["c0"], case["B"]
    HW = case["H"] ** 2
    r64 = TR.decoder_ref(inp, c0, F64)
    r32 = TR.decoder_ref(inp, c0, F32)
    chk = Checker()
    xg, W, b = inp["x"].to(DEV), inp["W"].to(DEV), inp["b"].to(DEV)
    emb, hw, hb = inp["emb"].to(DEV), inp["head_w"].to(DEV), inp["head_b"].to(DEV)
    zero = torch.zeros(B, HW, device=DEV)
    for exact in case["exact"]:
        path = {None: "default", True: "exact", False: "split"}[exact]
        d = ops.dba_project(xg, W, b, exact=exact)
        norm = ops.dba_colnorm(d, c0, emb)
        fg, bg, sdiag = ops.dba_heads(d, c0, emb, norm, hw, hb, want_sdiag=True, sdiag=torch.full((B,), SENTINEL, device=DEV))
        loss, gram = ops.orth_gram(d, c0, emb, norm, sdiag)
        got = dict(fg=fg, bg=bg, norm=norm, gram=gram, sdiag=sdiag, loss=loss)
        for k, s in TR.DECODER_FWD_SLICES.items():
            chk(f"r08/decoder/{case['id']}/{path}/{k}", got[k].cpu(), r64[k], r32[k], s)
        with ops.prezeroed():                                         # the caller-zeroed sdiag of the step (r.* buffers under one zero launch)
            fg0, bg0, sdiag0 = ops.dba_heads(d, c0, emb, norm, hw, hb, want_sdiag=True, sdiag=torch.zeros(B, device=DEV))
        for k, t in (("fg", fg0), ("bg", bg0), ("sdiag", sdiag0)):
            chk(f"r08/decoder/{case['id']}/{path}/prezeroed/{k}", t.cpu(), r64[k], r32[k], TR.DECODER_FWD_SLICES[k])
        layouts = ("separate", "arena", "prezeroed") if exact is case["exact"][0] else ("separate",)
        for mode, (gfg, gbg, gextra) in inp["modes"].items():
            gfg_d = zero if gfg is None else gfg.to(DEV)
            gbg_d = zero if gbg is None else gbg.to(DEV)
            for layout in layouts:
                gd, ghw, ghb, gdb = _bwd(layout, d, c0, emb, norm, hw, gram, gfg_d, gbg_d, gextra)
                gW = ops.dba_wgrad(gd, xg, gW=torch.full((128, case["C"]), SENTINEL, device=DEV), exact=exact)
                got = dict(gd=gd, gW=gW, g_head_w=ghw, g_head_b=ghb, g_dec_bias=gdb)
                for k, s in TR.DECODER_BWD_SLICES.items():
                    chk(f"r08/decoder/{case['id']}/{path}/{mode}/{layout}/{k}", got[k].cpu(), r64[mode][k], r32[mode][k], s)
        del d
    chk.done()


# ----------------------------------------------------------------------------------------------------------- discriminator
def _disc_tensors(sd):
    t = {k: sd[v].clone().float().contiguous().to(DEV) for k, v in TR.DISC_NAMES.items()}
    t["nbt"] = torch.tensor([int(sd[k]) for k in TR.NBT_KEYS], dtype=torch.int64, device=DEV)
    return t


def _grad_buffers(t, fill):
    return [torch.full(t["lin_w"].shape if shp is None else shp, fill, device=DEV) for _, shp in ops.DISC_GRAD_SHAPES]


@pytest.mark.parametrize("fs,B", TR.DISC_CASES)
def test_discriminator_two_calls_against_f64_autograd(fs, B):
    sd, masks, gprobs = TR.disc_inputs(fs, B)
    r64 = TR.disc_ref(sd, masks, gprobs, F64)
    r32 = TR.disc_ref(sd, masks, gprobs, F32)
    chk = Checker()
    tag = f"r08/disc/fs{fs}_b{B}"
    m_d = [m.to(DEV) for m in masks]
    gp_d = [g.to(DEV) for g in gprobs]
    nbt0 = [int(sd[k]) for k in TR.NBT_KEYS]

    # (a) pseudo label, then student: forward + backward each, the second backward accumulating (accumulate=False must overwrite)
    t = _disc_tensors(sd)
    grads = _grad_buffers(t, SENTINEL)
    for c in range(2):
        prob, saved = ops.disc_fwd(m_d[c], t)
        chk(f"{tag}/call{c}/prob", prob.cpu(), r64["prob"][c], r32["prob"][c], 0)
        for k in TR.DISC_RUNNING:
            chk(f"{tag}/call{c}/{k}", t[k].cpu(), r64["running"][c][k], r32["running"][c][k], 0)
        ops.disc_bwd(m_d[c], t, saved, gp_d[c], grads, accumulate=c == 1)
    assert t["nbt"].cpu().tolist() == r64["nbt"] == [n + 2 for n in nbt0]
    for (name, _), g in zip(ops.DISC_GRAD_SHAPES, grads):
        chk(f"{tag}/grad/{name}", TR.disc_grad_view(name, g.cpu(), fs), TR.disc_grad_view(name, r64["grads"][name], fs),
            TR.disc_grad_view(name, r32["grads"][name], fs), TR.DISC_GRAD_SLICES.get(name, 0))

    # (b) both forward calls on ONE zero-allocated saved buffer under ops.prezeroed() (r.disc_saved of the step): bn_finalize_kernel must
    # leave its f64 sums zeroed for the next call
    t = _disc_tensors(sd)
    saved = torch.zeros(N.load().ucod_disc_saved_bytes(B, fs), dtype=torch.uint8, device=DEV)
    for c in range(2):
        with ops.prezeroed():
            prob, _ = ops.disc_fwd(m_d[c], t, saved=saved)
        chk(f"{tag}/reuse/call{c}/prob", prob.cpu(), r64["prob"][c], r32["prob"][c], 0)
        for k in TR.DISC_RUNNING:
            chk(f"{tag}/reuse/call{c}/{k}", t[k].cpu(), r64["running"][c][k], r32["running"][c][k], 0)
    assert t["nbt"].cpu().tolist() == [n + 2 for n in nbt0]
    chk.done()


# ----------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("B", TR.BCE_BATCHES)
def test_disc_bce_against_f64_bce(B):
    """B > 256 runs the thread-stride loop; p = 1 / 0 hit the 1e-12 divisor and the -100 log clamp.  Gradients per element."""
    ps, pp = TR.bce_inputs(B)
    r64, r32 = TR.bce_ref(ps, pp, F64), TR.bce_ref(ps, pp, F32)
    gs, gp, loss = ops.disc_bce(ps.to(DEV), pp.to(DEV), 1.0 / (2 * B))
    chk = Checker()
    for k, v, s in (("g_student", gs, 1), ("g_pseudo", gp, 1), ("loss", loss.reshape(1), 0)):
        chk(f"r08/disc_bce/b{B}/{k}", v.cpu(), r64[k], r32[k], s)
    chk.done()


@pytest.mark.parametrize("frac", TR.APM_FRACS)
def test_apm_bce_at_the_headline_size(frac):
    """B = 32, HW = 4624: the three losses are sums over 148k terms reaching `losses` through f32 atomics.  With one workgroup per 256 pixels
    (608 atomics per loss) the order of the atomics spread the losses up to 1.2e-6 of the f64 value, past the bound (9.5e-7: the f32
    reference's pairwise sum rounds below an ulp) in 22 of 300 launches at fraction 1 (profiles/r08_apm_bce_loss_spread_ab.jsonl); one
    workgroup per image (32 atomics) stays at 2.7e-7."""
    inp = TR.apm_inputs()
    r64 = TR.apm_ref(inp, frac, TR.APM_GSCALE, F64)
    r32 = TR.apm_ref(inp, frac, TR.APM_GSCALE, F32)
    d = {k: v.to(DEV) for k, v in inp.items()}
    w, merged, gfg, gbg, losses = ops.apm_bce(d["pl"], d["teacher"], d["fg"], d["bg"], d["p_s"], d["p_p"], frac, gscale=TR.APM_GSCALE,
                                              losses=torch.full((4,), SENTINEL, device=DEV))
    ls = losses.cpu()
    got = dict(w=w.cpu(), merged=merged.cpu(), gfg=gfg.cpu(), gbg=gbg.cpu(), l1=ls[0:1], l2=ls[1:2], l3=ls[2:3])
    chk = Checker()
    for k, s in TR.APM_SLICES.items():
        chk(f"r08/apm_bce/frac{frac}/{k}", got[k], r64[k], r32[k], s)
    chk.done()


@pytest.mark.parametrize("finetune", [0, 1])
def test_step_loss_bit_for_bit(finetune):
    """out = ((l0 + l1) + extra) - l2 (without the last term when finetune is set), in f32, in that order"""
    g = torch.Generator().manual_seed(11 + finetune)
    for _ in range(32):
        losses = torch.rand(4, generator=g) * torch.exp2(torch.randint(-12, 4, (4,), generator=g).float())
        extra = torch.rand(1, generator=g) * torch.exp2(torch.randint(-20, 2, (1,), generator=g).float())
        out = ops.step_loss(losses.to(DEV), extra.to(DEV), finetune).cpu().reshape(1)
        ref = (losses[0:1] + losses[1:2]) + extra
        if not finetune:
            ref = ref - losses[2:3]
        assert torch.equal(out, ref), (losses, extra, out, ref)
