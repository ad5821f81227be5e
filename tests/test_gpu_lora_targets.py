"""GPU: LoRA ``target_modules`` -- subsets of query / key / value and the MLP input projection (``fc1``; ``weights_in`` on a SwiGLU checkpoint), every call
through the C ABI or the engine (models/modules/full_model.py:47-72 hands the list to peft).

1-4  the MLP module's row kernels against f64 on the same 16-bit-rounded operands, with canary rows behind every output, and their refusals;
5-6  whole passes against f64 autograd through the restatement of tests/lora_targets_ref.py (pinned on the CPU by tests/test_lora_targets_host.py), without and
     with dropout (masks restated by oracle.vit.lora_dropout_mask: q / k / v keys as ever, the MLP module's key L + l, projection 0);
7-9  the default engine is the engine it was, untargeted projections stay at zero through an optimiser step, and the public surface.

Measured on MI355X (the `lora_targets_passes` rows test 5 records), worst over the target sets and stream counts, none within 2x of its bar:
  GELU D = 128:    key max-abs 4.1e-3 (bar 3.0e-2),  worst gradient rel-L2 1.1e-2 (bar 4e-2),  worst MLP-module gradient 6.1e-3
  GELU D = 256:    key max-abs 5.6e-3 (bar 4.2e-2),  worst gradient rel-L2 1.4e-2 (bar 5e-2),  worst MLP-module gradient 5.9e-3
  SwiGLU D = 128:  key max-abs 3.1e-3 (bar 3.0e-2),  worst gradient rel-L2 1.1e-2 (bar 4e-2),  worst MLP-module gradient 7.8e-3
The gradient kernel alone (test 2): t within 2.9e-3, dA within 2.2e-7, dB within 1.7e-7 of f64, relative to max(1, |ref|max).
"""
import functools
import math

import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, swiglu  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTLoRAEngine  # noqa: E402
from oracle import vit as OV  # noqa: E402
import lora_targets_ref as R  # noqa: E402
from swiglu_ref import random_swiglu_state_dict  # noqa: E402

DEV = "cuda"
AUG = N.LORA_AUG
EINVAL = -1
GUARD_ROWS = 16


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def record(name, values):
    from test_gpu_parity_c2 import record as rec
    rec(name, values)


class Guarded:
    """[rows, cols] of ``dtype`` between GUARD_ROWS canary rows on either side; the payload starts as NaN, so an element no store reached shows."""

    def __init__(self, rows, cols, dtype):
        self.rows = rows
        self.canary = 1234.0
        self.buf = torch.full((rows + 2 * GUARD_ROWS, cols), self.canary, dtype=dtype, device=DEV)
        self.payload = self.buf[GUARD_ROWS:GUARD_ROWS + rows]
        self.payload.fill_(float("nan"))

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD_ROWS] == self.canary).all()) and bool((self.buf[GUARD_ROWS + self.rows:] == self.canary).all())


class FlatGuarded:
    """n f32 elements between two canary runs (the partials workspace: too large for whole guard rows)."""
    PAD = 4096

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * self.PAD,), 1234.0, dtype=torch.float32, device=DEV)

    def ptr(self):
        return self.buf[self.PAD:].data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.PAD] == 1234.0).all()) and bool((self.buf[self.PAD + self.n:] == 1234.0).all())


def drop_arg(p, seed, layer):
    import ctypes as C
    return C.byref(N.LoraDropout(p, seed, layer)) if p > 0 else None


# ------------------------------------------------------------------------------------------------ 1. LayerNorm + down-projection, one module
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("M,D,r", [(37, 128, 2), (300, 768, 2), (50, 384, 1), (53, 1536, 2)])
def test_layernorm_lora_mlp(M, D, r, x16, p_drop):
    """Bounds of tests/test_gpu_vit_train.py::test_layernorm_lora; with dropout the mask is the documented hash with key L + l (here 12 + 7), projection 0."""
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    if x16:
        x = x.half()
    gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)
    A = torch.randn(r, D, generator=g) / math.sqrt(D)
    seed, layer = 0x1234ABCD5678, 19
    out = Guarded(M, D + AUG, torch.bfloat16)
    xs, gs, bs, As = x.to(DEV), gam.to(DEV), bet.to(DEV), A.to(DEV)
    rc = N.load().ucod_layernorm_lora_mlp(N.ptr(xs), int(x16), N.ptr(gs), N.ptr(bs), N.ptr(As), r, out.ptr(), M, D, 1e-6, drop_arg(p_drop, seed, layer), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside its output"
    got = out.payload.float().cpu()
    assert bool(torch.isfinite(got).all()), "left elements unwritten"
    h = OV.layer_norm(x.double(), gam.double(), bet.double(), 1e-6)
    assert maxdiff(got[:, :D], h) < 2e-2 * max(1.0, h.abs().max().item())
    mask = OV.lora_dropout_mask(seed, layer, 0, M, D, p_drop).double() if p_drop > 0 else 1.0
    u = (h * mask) @ A.double().t()
    assert maxdiff(got[:, D:D + r], u) < 1e-2 * max(1.0, u.abs().max().item())
    assert float(got[:, D + r:].abs().max()) == 0.0
    if p_drop > 0:                                               # the mask matters: the undropped projection is far away
        assert maxdiff(got[:, D:D + r], h @ A.double().t()) > 0.05


# ------------------------------------------------------------------------------------------------ 2. the gradient kernel
GRAD_SHAPES = [(52, 512, 128, 2), (700, 1536, 384, 1), (3000, 3072, 768, 2), (300, 8192, 1536, 3)]


@functools.lru_cache(maxsize=None)
def grad_operands(M, N1, D, r, p_drop):
    """bf16-rounded operands of one case and the f64 references that do not depend on the kernel's output (computed once, never modified)."""
    g = torch.Generator().manual_seed(M + N1 + r)
    scaling, seed, layer = 2.0, 0xFEEDC0DE1234, 14
    A = torch.randn(r, D, generator=g) / math.sqrt(D)
    Bm = torch.randn(N1, r, generator=g) * 0.05
    dpre = torch.randn(M, N1, generator=g).bfloat16()
    h = torch.randn(M, D, generator=g).bfloat16()
    mask = OV.lora_dropout_mask(seed, layer, 0, M, D, p_drop).double() if p_drop > 0 else torch.ones(M, D, dtype=torch.float64)
    hd = h.double() * mask
    u = (hd @ A.double().t()).bfloat16()
    h_aug = torch.zeros(M, D + AUG, dtype=torch.bfloat16)
    h_aug[:, :D], h_aug[:, D:D + r] = h, u
    t_ref = scaling * dpre.double().to(DEV) @ Bm.double().to(DEV)
    dB_ref = scaling * dpre.double().to(DEV).t() @ u.double().to(DEV)
    return dict(scaling=scaling, seed=seed, layer=layer, flat=torch.cat((A.reshape(-1), Bm.reshape(-1))).to(DEV), dpre=dpre.to(DEV), h_aug=h_aug.to(DEV),
                hd=hd.to(DEV), t_ref=t_ref.cpu(), dB_ref=dB_ref.cpu())


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("M,N1,D,r", GRAD_SHAPES)
def test_lora_mlp_grad(M, N1, D, r, p_drop):
    """Bounds of tests/test_gpu_vit_train.py::test_lora_grad (t 1e-2, dA and dB 2e-4, relative to max(1, |ref|max)); dA from the bf16-rounded t the kernel wrote."""
    o = grad_operands(M, N1, D, r, p_drop)
    lib = N.load()
    wsb = lib.ucod_lora_mlp_grad_workspace_bytes(N1, D)
    assert wsb > 0
    runs = []
    for _ in range(2):
        ws = FlatGuarded(wsb // 4)
        t, grad = Guarded(M, AUG, torch.bfloat16), Guarded(1, r * (D + N1), torch.float32)
        rc = lib.ucod_lora_mlp_grad(N.ptr(o["dpre"]), N.ptr(o["h_aug"]), N.ptr(o["flat"]), r, o["scaling"], grad.ptr(), t.ptr(), ws.ptr(), wsb, M, N1, D,
                                    drop_arg(p_drop, o["seed"], o["layer"]), N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert t.guards_intact() and grad.guards_intact() and ws.guards_intact(), "wrote outside its outputs"
        runs.append((t.payload.clone(), grad.payload.clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    t_out, grad = runs[0][0].float().cpu(), runs[0][1].cpu().reshape(-1)
    assert bool(torch.isfinite(t_out).all()) and bool(torch.isfinite(grad).all()), "left elements unwritten"
    assert float(t_out[:, r:].abs().max()) == 0.0               # the unused aug columns
    e_t = maxdiff(t_out[:, :r], o["t_ref"]) / max(1.0, o["t_ref"].abs().max().item())
    dA_ref = (t_out[:, :r].double().to(DEV).t() @ o["hd"]).cpu()
    gA, gB = grad[:r * D].reshape(r, D), grad[r * D:].reshape(N1, r)
    e_a = maxdiff(gA, dA_ref) / max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, o["dB_ref"]) / max(1.0, o["dB_ref"].abs().max().item())
    print(f"lora_mlp_grad {(M, N1, D, r)} p={p_drop}: t {e_t:.2e} dA {e_a:.2e} dB {e_b:.2e}")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4, (e_t, e_a, e_b)
    assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. LayerNorm-2 backward with the LoRA term
@pytest.mark.parametrize("flags", [0, 1, 3])
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("M,D", [(37, 128), (300, 768), (20, 1536)])
def test_layernorm_bwd_lora_mlp(M, D, p_drop, flags):
    """== the plain backward applied to dy + mask (t A_m) formed in f64; bounds of tests/test_gpu_vit_train.py::test_layernorm_bwd.  flags: 0 = f32 dy and x,
    UCOD_LNB_DY_BF16 = bf16 dy on the f32 stream (resid="f32"), | UCOD_LNB_X_F16 = and the fp16 stream; the reference takes the 16-bit-rounded values."""
    r, seed, layer = 2, 0xABCDEF0123, 13
    g = torch.Generator().manual_seed(M * 3 + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    gam, dy, dres = torch.randn(D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    if flags & 1:
        dy = dy.bfloat16()
    if flags & 2:
        x = x.half()
    x_dev, dy_dev = x, dy                                        # what the kernel reads
    x, dy = x.float().requires_grad_(True), dy.float()
    sc = torch.rand(D, generator=g) + 0.5
    A = torch.randn(r, D, generator=g) / math.sqrt(D)
    t = torch.zeros(M, AUG, dtype=torch.bfloat16)
    t[:, :r] = torch.randn(M, r, generator=g).bfloat16()
    t[:, r:] = 55.0                                              # columns beyond the rank are never read
    mask = OV.lora_dropout_mask(seed, layer, 0, M, D, p_drop).double() if p_drop > 0 else 1.0
    dy2 = dy.double() + mask * (t[:, :r].double() @ A.double())
    y = OV.layer_norm(x.double(), gam.double(), torch.zeros(D).double(), 1e-6)
    (gx,) = torch.autograd.grad((y * dy2).sum(), x)
    ref = gx + dres.double()
    dx, s = Guarded(M, D, torch.float32), Guarded(M, D, torch.bfloat16)
    dys, xs, gs, scs, drs, ts, As = (v.to(DEV) for v in (dy_dev, x_dev, gam, sc, dres, t, A))
    rc = N.load().ucod_layernorm_bwd_lora_mlp(N.ptr(dys), N.ptr(xs), flags, N.ptr(gs), N.ptr(drs), N.ptr(scs), dx.ptr(), s.ptr(), M, D, 1e-6, N.ptr(ts), AUG, N.ptr(As), r,
                                              drop_arg(p_drop, seed, layer), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert dx.guards_intact() and s.guards_intact()
    assert maxdiff(dx.payload.cpu(), ref) < 2e-5 * max(1.0, ref.abs().max().item())
    assert maxdiff(s.payload.float().cpu(), ref * sc.double()) < 1e-2 * max(1.0, (ref * sc.double()).abs().max().item())
    (gx_plain,) = torch.autograd.grad((OV.layer_norm(x.double(), gam.double(), torch.zeros(D).double(), 1e-6) * dy.double()).sum(), x)
    assert maxdiff(gx_plain + dres.double(), ref) > 1e-2         # the term is there


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_outputs_untouched():
    M, N1, D, r = 52, 512, 128, 2
    o = grad_operands(M, N1, D, r, 0.0)
    lib, f16 = N.load(), N.load("f16")
    wsb = lib.ucod_lora_mlp_grad_workspace_bytes(N1, D)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    x, gam = torch.randn(M, D, device=DEV), torch.randn(D, device=DEV)
    outs = [torch.full((M, D + AUG), 3.0, dtype=torch.bfloat16, device=DEV), torch.full((M, AUG), 3.0, dtype=torch.bfloat16, device=DEV),
            torch.full((r * (D + N1),), 3.0, device=DEV), torch.full((N1, D + AUG), 3.0, dtype=torch.bfloat16, device=DEV), torch.full((M, D), 3.0, device=DEV)]
    y, t, grad, w_aug, dx = outs
    before = [v.clone() for v in outs]
    A9 = torch.zeros(9 * (D + N1), device=DEV)
    st = N.stream()
    P = N.ptr

    def ln(l, xp=P(x), a=P(o["flat"]), yp=P(y), rr=r):
        return l.ucod_layernorm_lora_mlp(xp, 0, P(gam), P(gam), a, rr, yp, M, D, 1e-6, None, st)

    def pack(l, a=P(o["flat"]), w=P(w_aug), rr=r):
        return l.ucod_lora_mlp_pack(a, rr, 2.0, w, N1, D, st)

    def grd(l, dp=P(o["dpre"]), a=P(o["flat"]), gp=P(grad), tp=P(t), rr=r, n1=N1, wb=wsb):
        return l.ucod_lora_mlp_grad(dp, P(o["h_aug"]), a, rr, 2.0, gp, tp, P(ws), wb, M, n1, D, None, st)

    def lnb(l, dyp=P(x), tp=P(t), a=P(o["flat"]), rr=r):
        return l.ucod_layernorm_bwd_lora_mlp(dyp, P(x), 0, P(gam), None, None, P(dx), None, M, D, 1e-6, tp, AUG, a, rr, None, st)

    calls = {
        "ln null x": lambda: ln(lib, xp=None), "ln null A": lambda: ln(lib, a=None), "ln null out": lambda: ln(lib, yp=None),
        "ln rank 9": lambda: ln(lib, a=P(A9), rr=9), "ln rank 0": lambda: ln(lib, rr=0), "ln fp16 build": lambda: ln(f16),
        "pack null": lambda: pack(lib, a=None), "pack null w": lambda: pack(lib, w=None), "pack rank 9": lambda: pack(lib, a=P(A9), rr=9), "pack fp16 build": lambda: pack(f16),
        "grad null dpre": lambda: grd(lib, dp=None), "grad null grad": lambda: grd(lib, gp=None), "grad null t": lambda: grd(lib, tp=None),
        "grad rank 9": lambda: grd(lib, a=P(A9), rr=9), "grad N1 % 128": lambda: grd(lib, n1=N1 - 64), "grad N1 > 8192": lambda: grd(lib, n1=16384),
        "grad small workspace": lambda: grd(lib, wb=wsb - 4), "grad fp16 build": lambda: grd(f16),
        "lnb null dy": lambda: lnb(lib, dyp=None), "lnb null t": lambda: lnb(lib, tp=None), "lnb null A": lambda: lnb(lib, a=None), "lnb rank 9": lambda: lnb(lib, a=P(A9), rr=9),
        "lnb fp16 build": lambda: lnb(f16),
    }
    for name, call in calls.items():
        rc = call()
        assert rc != 0, name
        if "workspace" not in name:
            assert rc == EINVAL, (name, rc)
    assert lib.ucod_lora_mlp_grad_workspace_bytes(N1 - 64, D) == 0 and lib.ucod_lora_mlp_grad_workspace_bytes(N1, 1664) == 0
    # the whole-pass entry points: a rank beyond the MLP module's limit is refused with the table given, taken without it (3 r <= 64 as ever)
    import ctypes as C
    td = N.VitTrainDesc()
    v = td.vit
    v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps = 2, 3, 70, 70, 14, 128, 2, 512, 3, 640, 1e-6
    td.lora_r, td.lora_scaling = 9, 0.5
    # (the tables point at real memory: a refusal must come before any dereference, but the test does not stake the machine on it)
    dummy = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    TM = (C.c_void_p * 9)(*([dummy.data_ptr()] * 9))
    assert lib.ucod_vit_train_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, TM) == 0
    assert lib.ucod_vit_lora_infer_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, TM) == 0
    assert lib.ucod_vit_train_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, None) == lib.ucod_vit_train_workspace_bytes_mlp(C.byref(td), N.UCOD_MLP_GELU) > 0
    key = torch.full((2, 128, 5, 5), 3.0, device=DEV)
    T = (C.c_void_p * 52)(*([dummy.data_ptr()] * 52))
    TT = (C.c_void_p * 21)(*([dummy.data_ptr()] * 21))
    assert lib.ucod_vit_forward_train_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, T, TT, TM, P(x), P(key), P(ws), wsb, st) == EINVAL
    assert lib.ucod_vit_backward_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, T, TT, TM, P(key), P(ws), wsb, st) == EINVAL
    assert lib.ucod_vit_forward_lora_infer_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, T, TT, TM, P(x), P(key), P(ws), wsb, st) == EINVAL
    td.lora_r = 2
    assert lib.ucod_vit_train_workspace_bytes_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, TM) > lib.ucod_vit_train_workspace_bytes_mlp(C.byref(td), N.UCOD_MLP_GELU)
    assert f16.ucod_vit_forward_train_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, T, TT, TM, P(x), P(key), P(ws), wsb, st) == EINVAL
    assert lib.ucod_vit_forward_train_lora_mlp(C.byref(td), N.UCOD_MLP_GELU, T, TT, TM, None, P(key), P(ws), wsb, st) == EINVAL
    torch.cuda.synchronize()
    for a, b in zip(outs + [key], before + [torch.full_like(key, 3.0)]):
        assert torch.equal(a, b), "a refused call wrote to its outputs"
    with pytest.raises(ValueError, match="rank"):
        ViTLoRAEngine(sub(load_golden("g8_dinov2_native"), "sd."), heads=2, r=9, device=DEV, target_modules=["query", "fc1"])


# ------------------------------------------------------------------------------------------------ 5. whole passes vs f64 autograd
@functools.lru_cache(maxsize=None)
def checkpoint(kind, D):
    """(HF-named state dict, heads, L, image size, batch)."""
    if kind == "swiglu":
        return random_swiglu_state_dict(128, 2, 3, image_size=70, seed=128), 2, 3, 70, 2
    if D == 128:
        sd = sub(load_golden("g8_dinov2_native"), "sd.")
        return sd, 2, 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer.")), 70, 2
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(21)
    m = Dinov2Model(Dinov2Config(hidden_size=256, num_hidden_layers=4, num_attention_heads=4, image_size=126, patch_size=14, mlp_ratio=4, layerscale_value=1.0)).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            if "position_embeddings" in n or "cls_token" in n:
                p.mul_(0.05)
    return {k: v.detach() for k, v in m.state_dict().items()}, 4, 4, 126, 3


def targeted_engine(sd, heads, targets, gen_seed=3, **kw):
    """An engine with B = 0.05 randn on its targeted modules (peft's B = 0 would make the LoRA branch vanish)."""
    gen = torch.Generator().manual_seed(gen_seed)
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=gen, allow_swiglu=True, target_modules=targets, **kw)
    lsd = eng.lora_state_dict()
    for k in sorted(lsd):
        if "lora_B" in k:
            lsd[k] = 0.05 * torch.randn(lsd[k].shape, generator=gen)
    eng.load_lora_state_dict(lsd)
    return eng


@functools.lru_cache(maxsize=None)
def pass_case(kind, D, targets):
    """The inputs of one (checkpoint, target set) and its f64 reference, computed once and shared by the stream counts."""
    sd, heads, L, image, B = checkpoint(kind, D)
    eng = targeted_engine(sd, heads, list(targets))
    gen = torch.Generator().manual_seed(7)
    gh = image // 14
    img, dkey = torch.randn(B, 3, image, image, generator=gen), torch.randn(B, D, gh, gh, generator=gen)
    lsd = {k: v.cpu() for k, v in eng.lora_state_dict().items()}
    key_ref, gref = R.lora_grads(img, {**sd, **lsd}, heads, dkey, eng.scaling, device=DEV)
    return sd, heads, L, img, dkey, lsd, key_ref.cpu(), {k: v.cpu() for k, v in gref.items()}


PASS_CASES = [("gelu", 128, s, t) for s in (1, 2) for t in (("query", "value"), ("key",), ("query", "key", "value", "fc1"))] + \
             [("gelu", 256, s, t) for s in (1, 2) for t in (("query", "value"), ("key",), ("query", "key", "value", "fc1"))] + \
             [("swiglu", 128, 2, t) for t in (("query", "value"), ("key",), ("value", "weights_in"))]


@pytest.mark.parametrize("kind,D,streams,targets", PASS_CASES)
def test_passes_vs_f64_autograd(kind, D, streams, targets):
    """Bars: the project's own for bf16 operands at this depth (tests/test_gpu_vit_train.py, tests/test_gpu_swiglu_train.py): key max-abs 3e-2 max(1, |key|max), every
    non-zero gradient rel-L2 5e-2 (4e-2 at D = 128).  Structurally zero gradients -- the last layer's query / value / MLP modules, every untargeted projection --
    are exactly zero."""
    sd, heads, L, img, dkey, lsd, key_ref, gref = pass_case(kind, D, targets)
    eng = targeted_engine(sd, heads, list(targets))
    eng.train_streams = streams
    assert {k: v.cpu() for k, v in eng.lora_state_dict().items()}.keys() == lsd.keys()
    key = eng.forward_train(img.to(DEV))
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    got = eng.lora_state_dict(grads=True)
    assert sorted(got) == sorted(gref)
    key_err, key_bar = maxdiff(key.cpu(), key_ref), 3e-2 * max(1.0, key_ref.abs().max().item())
    bar = 4e-2 if D == 128 else 5e-2
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    zero = [k for k, ref in gref.items() if float(ref.abs().max()) == 0.0]
    worst = max(errs, key=errs.get)
    mlp_errs = [e for k, e in errs.items() if ".mlp." in k]
    record("lora_targets_passes", dict(kind=kind, D=D, streams=streams, targets=",".join(targets), key_max_abs=key_err, key_bar=key_bar, worst_grad_rel_l2=errs[worst],
                                       worst_grad=worst, worst_mlp_grad_rel_l2=max(mlp_errs) if mlp_errs else None))
    print(f"{kind} D={D} streams={streams} {targets}: key {key_err:.2e} (bar {key_bar:.2e}), worst gradient {errs[worst]:.2e} ({worst}), MLP {max(mlp_errs) if mlp_errs else None}")
    assert key_err < key_bar, key_err
    # the last layer: only its key projection reaches the key map
    n_mod = len(targets)
    n_last_live = 2 if "key" in targets else 0
    assert len(zero) == 2 * n_mod - n_last_live and all(f"layer.{L - 1}." in k for k in zero), zero
    for k in zero:
        assert float(got[k].abs().max()) == 0.0, k
    assert len(errs) == 2 * n_mod * L - len(zero)
    for k, e in errs.items():
        assert e < bar, (k, e)
    # untargeted projections: parameters and gradients exactly zero
    for p, name in enumerate(("query", "key", "value")):
        if name not in targets:
            sa, sb = eng._slices(p)
            for sl in (sa, sb):
                assert float(eng.lora[:, sl].abs().max()) == 0.0 and float(eng.lora_grad[:, sl].abs().max()) == 0.0, name
    if eng.mlp_target is not None:
        assert eng.lora.shape == (L, 6 * 2 * D + 2 * (D + eng.N1)) and eng.lora_grad.shape == eng.lora.shape
        if kind == "swiglu":                                     # padded rows of B_m: parameters and gradients stay zero
            _, sb = eng._mlp_slices()
            pad = eng.lora_grad[:, sb].reshape(L, eng.N1 // 8, 2, 4, 2)[:, eng._F0 // 4:]
            assert eng.N1 == 768 and eng._F0 == 344 and float(pad.abs().max()) == 0.0
            assert float(eng.lora[:, sb].reshape(L, eng.N1 // 8, 2, 4, 2)[:, eng._F0 // 4:].abs().max()) == 0.0
    else:
        assert eng.lora.shape == (L, 6 * 2 * D)


# ------------------------------------------------------------------------------------------------ 6. dropout end to end
def test_dropout_end_to_end_with_the_mlp_module():
    sd, heads, L, image, B = checkpoint("gelu", 128)
    targets = ["query", "key", "value", "fc1"]
    p_drop, D, rows = 0.3, 128, 2 * 26
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(B, 3, image, image, generator=gen), torch.randn(B, D, 5, 5, generator=gen)
    eng = targeted_engine(sd, heads, targets, lora_dropout=p_drop, seed=1234)
    eng.train_streams = 1
    key = eng.forward_train(img.to(DEV))
    seed = eng._step_seed
    masks = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(("query", "key", "value"))}
    masks.update({(i, "fc1"): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
    km, kq = ((masks[(0, n)] > 0).float().flatten() for n in ("fc1", "query"))
    assert abs(float(torch.corrcoef(torch.stack((km, kq)))[0, 1])) < 0.05       # the MLP module's mask is its own
    lsd = {k: v.cpu() for k, v in eng.lora_state_dict().items()}
    key_ref, gref = R.lora_grads(img, {**sd, **lsd}, heads, dkey, eng.scaling, masks=masks, device=DEV)
    assert maxdiff(key.cpu(), key_ref.cpu()) < 3e-2 * max(1.0, key_ref.abs().max().item())
    eng.backward(dkey.to(DEV))
    got = eng.lora_state_dict(grads=True)
    for k, ref in gref.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
        else:
            assert rel_l2(got[k], ref) < 5e-2, (k, rel_l2(got[k], ref))
    _, g_nomask = R.lora_grads(img, {**sd, **lsd}, heads, dkey, eng.scaling, device=DEV)
    k0 = "encoder.layer.0.mlp.fc1.lora_A.weight"
    assert rel_l2(got[k0], g_nomask[k0]) > 0.1                   # the dropped branch really changes the answer
    # forward_nograd == forward_train under equal seeds
    mk = lambda: targeted_engine(sd, heads, targets, lora_dropout=p_drop, seed=11)  # noqa: E731
    x = img.to(DEV)
    k_train, k_f32, k_f16 = mk().forward_train(x), mk().forward_nograd(x, resid16=False), mk().forward_nograd(x, resid16=True)
    assert rel_l2(k_f32, k_train) < 2e-3, rel_l2(k_f32, k_train)
    assert rel_l2(k_f16, k_train) < 4e-3, rel_l2(k_f16, k_train)
    # eval() reproduces the no-dropout engine bit for bit
    eng.eval()
    ref_eng = targeted_engine(sd, heads, targets)
    ref_eng.train_streams = 1
    assert torch.equal(eng.lora, ref_eng.lora)
    assert torch.equal(eng.forward_train(x), ref_eng.forward_train(x))
    eng.backward(dkey.to(DEV))
    ref_eng.backward(dkey.to(DEV))
    assert torch.equal(eng.lora_grad, ref_eng.lora_grad)
    assert torch.equal(eng.forward_nograd(x), ref_eng.forward_nograd(x))


# ------------------------------------------------------------------------------------------------ 7. the default is untouched
def test_default_engine_equals_qkv_named_in_any_order():
    sd, heads, L, image, B = checkpoint("gelu", 128)
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(B, 3, image, image, generator=gen).to(DEV), torch.randn(B, 128, 5, 5, generator=gen).to(DEV)
    out = []
    for targets in (None, ["value", "query", "key"]):
        kw = {} if targets is None else dict(target_modules=targets)
        g = torch.Generator().manual_seed(3)
        eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=g, **kw)
        lsd = eng.lora_state_dict()
        for k in sorted(lsd):
            if "lora_B" in k:
                lsd[k] = 0.05 * torch.randn(lsd[k].shape, generator=g)
        eng.load_lora_state_dict(lsd)
        key = eng.forward_train(img)
        eng.backward(dkey)
        out.append((eng.lora.clone(), key.clone(), eng.lora_grad.clone()))
        assert eng.lora.shape == (L, 6 * 2 * 128) and eng.mlp_target is None and eng.mlp_layers == []
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[0][2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 8. untargeted projections stay at zero
def test_untargeted_projection_stays_zero_through_an_optimiser_step():
    from ucod_dpl_amd.engine.runner.loop_UCOD_DPL import FusedAdamW
    sd, heads, L, image, B = checkpoint("gelu", 128)
    eng = targeted_engine(sd, heads, ["query", "value"])
    ema = eng.clone_for_ema()
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(B, 3, image, image, generator=gen).to(DEV), torch.randn(B, 128, 5, 5, generator=gen).to(DEV)
    before = eng.lora.clone()
    eng.forward_train(img)
    eng.backward(dkey)
    n = eng.lora.numel()
    opt = FusedAdamW(eng.lora.view(-1), eng.lora_grad.view(-1), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), 1e-2)    # (weight decay 0.01: ops.adamw_ema)
    opt.step(ema=ema.lora.view(-1), alpha=0.5)
    eng.repack()
    ema.repack()
    torch.cuda.synchronize()
    sa, sb = eng._slices(1)
    for name, t in (("lora", eng.lora), ("lora_grad", eng.lora_grad), ("ema", ema.lora)):
        assert float(t[:, sa].abs().max()) == 0.0 and float(t[:, sb].abs().max()) == 0.0, name
    assert not torch.equal(eng.lora, before)                    # the targeted ones moved
    assert "encoder.layer.0.attention.attention.key.lora_A.weight" not in eng.lora_state_dict()
    with pytest.raises(KeyError, match="key"):
        eng.load_lora_state_dict({**eng.lora_state_dict(), "encoder.layer.0.attention.attention.key.lora_A.weight": torch.zeros(2, 128)})


# ------------------------------------------------------------------------------------------------ 9. public surface
def test_load_lora_and_full_model_with_the_mlp_target():
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.models.modules.full_model import LoRABackbone, full_model, load_lora
    from ucod_dpl_amd.models.uscod import baseline
    sd, heads, L, image, B = checkpoint("gelu", 128)
    torch.manual_seed(0)
    cfg = CfgNode(dict(model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, enable_ocm=False, freeze_lora=False),
                       lora_cfg=dict(r=2, lora_alpha=4, lora_dropout=0.0, target_modules=["query", "value", "fc1"])))
    bb = load_lora(cfg.lora_cfg, sd, heads=heads, device=DEV, generator=torch.Generator().manual_seed(1))
    assert isinstance(bb, LoRABackbone) and bb.engine.targets == (True, False, True) and bb.engine.mlp_target == "fc1"
    eng = bb.engine
    lsd = eng.lora_state_dict()
    assert lsd["encoder.layer.0.mlp.fc1.lora_A.weight"].shape == (2, 128) and lsd["encoder.layer.0.mlp.fc1.lora_B.weight"].shape == (512, 2)
    assert float(lsd["encoder.layer.0.mlp.fc1.lora_B.weight"].abs().max()) == 0.0 and float(lsd["encoder.layer.0.mlp.fc1.lora_A.weight"].abs().max()) > 0.0
    gen = torch.Generator().manual_seed(2)
    eng.load_lora_state_dict({k: (0.05 * torch.randn(v.shape, generator=gen) if "lora_B" in k else v) for k, v in sorted(lsd.items())})
    fm = full_model(cfg, bb, baseline(cfg.model_cfg).to(DEV))
    fm.hook_size = 8                                            # (a 5 x 5 grid: 5 -> 68 is outside the resize adjoint's tap budget)
    img = torch.randn(B, 3, image, image, generator=gen).to(DEV)
    fg, bg, extra = fm(img)
    (fg.square().mean() + bg.square().mean() + extra).backward()
    g = fm.backbone.lora.grad
    assert g is not None and g.shape == eng.lora.shape and bool(torch.isfinite(g).all())
    assert float(g[:L - 1, eng.qkv_numel:].abs().max()) > 0.0    # the MLP slice (layers below the last)
    assert float(g[L - 1, eng.qkv_numel:].abs().max()) == 0.0
    assert fm.backbone_ema.lora.grad is None
    assert fm.backbone_ema.engine.mlp_layers[0][0].data_ptr() != eng.mlp_layers[0][0].data_ptr()
    # state-dict export -> load round trip reproduces the key map bit for bit
    eng.eval()
    k0 = eng.forward_train(img).clone()
    other = load_lora(cfg.lora_cfg, sd, heads=heads, device=DEV).engine
    other.load_lora_state_dict({k: v.cpu() for k, v in eng.lora_state_dict().items()})
    other.eval()
    assert torch.equal(other.lora, eng.lora) and torch.equal(other.forward_train(img), k0)
    with pytest.raises(NotImplementedError, match="dense"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, target_modules=["dense"])), sd, heads=heads, device=DEV)


def test_swiglu_state_dict_round_trip_on_the_device():
    sd, heads, L, image, B = checkpoint("swiglu", 128)
    eng = targeted_engine(sd, heads, ["value", "weights_in"])
    lsd = eng.lora_state_dict()
    b = lsd["encoder.layer.1.mlp.weights_in.lora_B.weight"]
    assert b.shape == (2 * 344, 2) and float(b.abs().min()) > 0.0            # HF row order, unpadded
    other = ViTLoRAEngine(sd, heads=heads, device=DEV, allow_swiglu=True, target_modules=["value", "weights_in"])
    other.load_lora_state_dict(lsd)
    assert torch.equal(other.lora, eng.lora)
    _, sb = eng._mlp_slices()
    assert torch.equal(eng.lora[1, sb].reshape(768, 2).cpu(), swiglu.lora_b_to_engine(b.cpu()))
    img = torch.randn(B, 3, image, image, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(eng.forward_train(img), other.forward_train(img))
