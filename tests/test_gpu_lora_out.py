"""GPU: LoRA on the output projections -- ``attention.output.dense`` / ``mlp.fc2`` (``o_proj`` / ``down_proj`` on a DINOv3 checkpoint), the opt-in ``allow_out`` of
ViTLoRAEngine (models/modules/full_model.py:47-72 hands ``target_modules`` to peft), every call through the C ABI or the engine.

1-2  the three row kernels alone against f64 on the same 16-bit-rounded operands, with canary rows around every output, run twice;
3-6  whole passes against f64 autograd through tests/lora_out_ref.py (pinned on the CPU by tests/test_lora_out_host.py, which also shows that these cases have teeth):
     the G8 DINOv2 model and the D = 256 GELU model on one and two streams, with registers (G21 ``native``), DINOv3 (G23 ``g46``), the EMA teacher's pass;
7-8  merging and the adapter folder; one training step of the runner;
9    the four older tiers of the pass entry points, called directly, against the engine's own passes (which run the _lora_out_ex tier), bit for bit.

The bars are the ones tests/test_gpu_lora_targets.py holds the same quantities to (its tests 1-3 for the kernels, 5-6 for the passes), tests/test_gpu_dinov3_lora.py's
for the DINOv3 model and tests/test_gpu_lora_merge.py's for the merge; none is taken from a run of this code.  Two bars have no counterpart there and are derived:
the f32 stream row after the update is an f32 output of a row kernel (2e-5 max(1, |ref|max), what test 3 there asks of dx), the fp16 one adds the one rounding of
its storage format (2^-11 |ref|max).

Measured on MI355X (profiles/lora_out_tests.txt), worst over the cases: kernels alone -- u 1.1e-7, f32 stream 1.0e-7, fp16 stream 3.6e-4, t 9.4e-8, dA 5.3e-7, dB 1.1e-7,
cotangent 3.4e-3; passes -- D = 128 key 4.0e-3 (bar 3.0e-2), gradients 1.5e-2 (4e-2); D = 256 key 6.3e-3 (4.2e-2), gradients 1.4e-2 (5e-2); registers 2.9e-3 / 7.1e-3;
DINOv3 key 3.3e-3 rel-L2 (1.13e-2), gradients 1.6e-2 (5e-2); merged split3 4.9e-7 (3e-6); no-grad pass 1.9e-3 (2e-3) on the f32 stream, 1.2e-4 (4e-3) on the fp16 one."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, ViTLoRAEngine  # noqa: E402
from oracle import vit as OV  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402
import registers_ref as RR  # noqa: E402
import lora_out_ref as RO  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402

DEV = "cuda"
GUARD_ROWS = 16
W = N.LORA_OUT_W


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Guarded:
    """[rows, cols] of ``dtype`` between GUARD_ROWS canary rows on either side; the payload starts as ``fill`` (NaN: an element no store reached shows)."""

    def __init__(self, rows, cols, dtype, fill=None):
        self.rows, self.canary = rows, 1234.0
        self.buf = torch.full((rows + 2 * GUARD_ROWS, cols), self.canary, dtype=dtype, device=DEV)
        self.payload = self.buf[GUARD_ROWS:GUARD_ROWS + rows]
        if fill is None:
            self.payload.fill_(float("nan"))
        else:
            self.payload.copy_(fill)

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD_ROWS] == self.canary).all()) and bool((self.buf[GUARD_ROWS + self.rows:] == self.canary).all())


class FlatGuarded:
    """n f32 elements between two canary runs (the partials workspace)."""
    PAD = 4096

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * self.PAD,), 1234.0, dtype=torch.float32, device=DEV)

    def ptr(self):
        return self.buf[self.PAD:].data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.PAD] == 1234.0).all()) and bool((self.buf[self.PAD + self.n:] == 1234.0).all())


def drop_arg(p, seed, layer):
    return C.byref(N.LoraDropout(p, seed, layer)) if p > 0 else None


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


# (M, K, D, r): M = 111 is no multiple of any rows-per-block grouping (1, 4); 2 * 1370 rows is more rows than the forward has blocks (2048).  K = 128 ... 1024 with
# D = 128 / 256 are the issue's; K = 3072 takes the forward's two-vectors-per-thread form and three column slabs of grad_x, D = 768 / 1536 the two- and
# three-pair forms of grad_s; r = 1, 2 run the two-rank instantiations, r = 8 the eight-rank ones.
SHAPES = [(111, 128, 128, 1), (111, 512, 128, 2), (111, 1024, 256, 8), (111, 512, 256, 8), (111, 1024, 128, 2), (111, 128, 256, 2),
          (2 * 1370, 512, 128, 2), (111, 3072, 768, 2), (111, 1536, 1536, 8)]
SEED, KEY = 0x1234ABCD5678, 29


@functools.lru_cache(maxsize=None)
def operands(M, K, D, r, p_drop):
    """bf16-rounded operands of one shape and what does not depend on a kernel's output (computed once, never modified)."""
    g = torch.Generator().manual_seed(M + K + D + r)
    A = torch.randn(r, K, generator=g) / math.sqrt(K)
    Bo = torch.randn(D, r, generator=g) * 0.3
    lam = torch.rand(D, generator=g) + 0.5
    x_in = torch.randn(M, K, generator=g).bfloat16()
    x0 = torch.randn(M, D, generator=g) * 2
    s = torch.randn(M, D, generator=g).bfloat16()
    cot = torch.randn(M, K, generator=g).bfloat16()
    mask = OV.lora_dropout_mask(SEED, KEY, 0, M, K, p_drop).double() if p_drop > 0 else torch.ones(M, K, dtype=torch.float64)
    return dict(scaling=2.0, flat=torch.cat((A.reshape(-1), Bo.reshape(-1))).to(DEV), A=A.double(), B=Bo.double(), lam=lam, x_in=x_in, x0=x0, s=s, cot=cot, mask=mask)


# ------------------------------------------------------------------------------------------------ 1. the forward kernel
@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("M,K,D,r", SHAPES)
def test_lora_out_fwd(M, K, D, r, p_drop, h16):
    o = operands(M, K, D, r, p_drop)
    lib = N.load()
    x0 = o["x0"].half() if h16 else o["x0"]
    u_ref = (o["x_in"].double() * o["mask"]) @ o["A"].t()
    x_ref = x0.double() + o["lam"].double() * (o["scaling"] * u_ref @ o["B"].t())
    xin, lam = o["x_in"].to(DEV), o["lam"].to(DEV)
    runs = []
    for _ in range(2):
        xs, u = Guarded(M, D, x0.dtype, fill=x0.to(DEV)), Guarded(M, W, torch.float32)
        rc = lib.ucod_lora_out_fwd(N.ptr(xin), N.ptr(o["flat"]), r, o["scaling"], N.ptr(lam), xs.ptr(), int(h16), u.ptr(), M, K, D, drop_arg(p_drop, SEED, KEY), N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert xs.guards_intact() and u.guards_intact(), "wrote outside its outputs"
        runs.append((xs.payload.clone(), u.payload.clone()))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    xg, ug = runs[0][0].double().cpu(), runs[0][1].cpu()
    assert bool(torch.isfinite(ug).all()), "left elements of u unwritten"
    assert float(ug[:, r:].abs().max()) == 0.0 if r < W else True                     # the columns beyond the rank
    e_u = maxdiff(ug[:, :r], u_ref) / max(1.0, u_ref.abs().max().item())
    scale = max(1.0, x_ref.abs().max().item())
    e_x = maxdiff(xg, x_ref) / scale
    bar_x = 2e-5 + (2.0 ** -11 if h16 else 0.0)
    print(f"lora_out_fwd {(M, K, D, r)} p={p_drop} h16={h16}: u {e_u:.2e} (bar 1e-2), stream {e_x:.2e} (bar {bar_x:.2e})")
    assert e_u < 1e-2 and e_x < bar_x, (e_u, e_x)
    assert maxdiff(xg, x0.double()) > 0.1                                            # the update is there
    if p_drop > 0:                                                                   # ... and the mask matters
        assert maxdiff(ug[:, :r], o["x_in"].double() @ o["A"].t()) > 0.05
    # the no-grad form (u not stored) gives the same stream, bit for bit
    xs = Guarded(M, D, x0.dtype, fill=x0.to(DEV))
    assert lib.ucod_lora_out_fwd(N.ptr(xin), N.ptr(o["flat"]), r, o["scaling"], N.ptr(lam), xs.ptr(), int(h16), None, M, K, D, drop_arg(p_drop, SEED, KEY), N.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(xs.payload), bits(runs[0][0])) and xs.guards_intact()


# ------------------------------------------------------------------------------------------------ 2. the two backward kernels
@pytest.mark.parametrize("act", ["identity", "gelu"])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("M,K,D,r", SHAPES)
def test_lora_out_grad(M, K, D, r, p_drop, act):
    """t 1e-2, dA and dB 2e-4 relative to max(1, |ref|max) (tests/test_gpu_lora_targets.py::test_lora_mlp_grad; dA from the t the kernel wrote); the cotangent is a
    bf16 output: 1e-2 (what its test 3 asks of ``s``)."""
    o = operands(M, K, D, r, p_drop)
    lib = N.load()
    g = torch.Generator().manual_seed(K + r)
    u = torch.full((M, W), 55.0)                                 # columns beyond the rank are never read
    u[:, :r] = torch.randn(M, r, generator=g)
    wsb = lib.ucod_lora_out_grad_workspace_bytes(r, K, D)
    assert wsb > 0
    sdev, udev, xdev = o["s"].to(DEV), u.to(DEV), o["x_in"].to(DEV)
    t_ref = o["scaling"] * o["s"].double() @ o["B"]
    dB_ref = o["scaling"] * o["s"].double().t() @ u[:, :r].double()
    x = o["x_in"].double()
    if act == "gelu":
        xa = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
        da = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    else:
        xa, da = x, torch.ones_like(x)
    runs = []
    for _ in range(2):
        ws = FlatGuarded(wsb // 4)
        t, grad, cot = Guarded(M, W, torch.float32), Guarded(1, r * (K + D), torch.float32), Guarded(M, K, torch.bfloat16, fill=o["cot"].to(DEV))
        rc = lib.ucod_lora_out_grad_s(N.ptr(sdev), N.ptr(udev), N.ptr(o["flat"]), r, o["scaling"], grad.ptr(), t.ptr(), ws.ptr(), wsb, M, K, D, N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool(torch.isnan(grad.payload.reshape(-1)[:r * K]).all()), "grad_s wrote into the A part"
        rc = lib.ucod_lora_out_grad_x(N.ptr(xdev), N.LORA_OUT_ACT_GELU if act == "gelu" else N.LORA_OUT_ACT_IDENTITY, cot.ptr(), t.ptr(), N.ptr(o["flat"]), r, grad.ptr(),
                                      ws.ptr(), wsb, M, K, D, drop_arg(p_drop, SEED, KEY), N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert t.guards_intact() and grad.guards_intact() and cot.guards_intact() and ws.guards_intact(), "wrote outside its outputs"
        runs.append((t.payload.clone(), grad.payload.clone(), cot.payload.clone()))
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b)), "two runs differ"
    t_out, grad, cot_out = runs[0][0].cpu(), runs[0][1].cpu().reshape(-1), runs[0][2].double().cpu()
    assert bool(torch.isfinite(t_out).all()) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(cot_out).all()), "left elements unwritten"
    if r < W:
        assert float(t_out[:, r:].abs().max()) == 0.0
    tk = t_out[:, :r].double()
    dA_ref = tk.t() @ (xa * o["mask"])
    cot_ref = o["cot"].double() + da * o["mask"] * (tk @ o["A"])
    gA, gB = grad[:r * K].reshape(r, K), grad[r * K:].reshape(D, r)
    e_t = maxdiff(tk, t_ref) / max(1.0, t_ref.abs().max().item())
    e_a = maxdiff(gA, dA_ref) / max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, dB_ref) / max(1.0, dB_ref.abs().max().item())
    e_c = maxdiff(cot_out, cot_ref) / max(1.0, cot_ref.abs().max().item())
    print(f"lora_out_grad {(M, K, D, r)} p={p_drop} {act}: t {e_t:.2e} dA {e_a:.2e} dB {e_b:.2e} cotangent {e_c:.2e}")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4 and e_c < 1e-2, (e_t, e_a, e_b, e_c)
    assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0 and maxdiff(cot_out, o["cot"].double()) > 0.05
    if act == "gelu":                                           # the activation matters: the identity's dA is far away
        assert maxdiff(gA, tk.t() @ (x * o["mask"])) / max(1.0, dA_ref.abs().max().item()) > 1e-2


def test_refusals_leave_outputs_untouched():
    M, K, D, r = 111, 512, 128, 2
    o = operands(M, K, D, r, 0.0)
    lib, f16 = N.load(), N.load("f16")
    wsb = lib.ucod_lora_out_grad_workspace_bytes(r, K, D)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    outs = [torch.full((M, D), 3.0, device=DEV), torch.full((M, W), 3.0, device=DEV), torch.full((r * (K + D),), 3.0, device=DEV),
            torch.full((M, K), 3.0, dtype=torch.bfloat16, device=DEV)]
    xs, u, grad, cot = outs
    xin, s = o["x_in"].to(DEV), o["s"].to(DEV)
    st, P = N.stream(), N.ptr

    def fwd(l, xp=P(xin), a=P(o["flat"]), sp=P(xs), rr=r, k=K, d=D, h=0):
        return l.ucod_lora_out_fwd(xp, a, rr, 2.0, None, sp, h, P(u), M, k, d, None, st)

    def gs(l, sp=P(s), up=P(u), gp=P(grad), rr=r, k=K, wb=wsb):
        return l.ucod_lora_out_grad_s(sp, up, P(o["flat"]), rr, 2.0, gp, P(u), P(ws), wb, M, k, D, st)

    def gx(l, xp=P(xin), cp=P(cot), act=0, rr=r, k=K, wb=wsb):
        return l.ucod_lora_out_grad_x(xp, act, cp, P(u), P(o["flat"]), rr, P(grad), P(ws), wb, M, k, D, None, st)

    calls = {"fwd null x": lambda: fwd(lib, xp=None), "fwd null lora": lambda: fwd(lib, a=None), "fwd null stream": lambda: fwd(lib, sp=None), "fwd rank 9": lambda: fwd(lib, rr=9),
             "fwd rank 0": lambda: fwd(lib, rr=0), "fwd K % 128": lambda: fwd(lib, k=K - 64), "fwd K > 4096": lambda: fwd(lib, k=8192), "fwd D % 128": lambda: fwd(lib, d=192),
             "fwd stream type": lambda: fwd(lib, h=2), "fwd fp16 build": lambda: fwd(f16),
             "grad_s null s": lambda: gs(lib, sp=None), "grad_s null u": lambda: gs(lib, up=None), "grad_s null grad": lambda: gs(lib, gp=None), "grad_s rank 9": lambda: gs(lib, rr=9),
             "grad_s small workspace": lambda: gs(lib, wb=wsb - 4), "grad_s fp16 build": lambda: gs(f16),
             "grad_x null x": lambda: gx(lib, xp=None), "grad_x null cot": lambda: gx(lib, cp=None), "grad_x act": lambda: gx(lib, act=2), "grad_x rank 9": lambda: gx(lib, rr=9),
             "grad_x K > 4096": lambda: gx(lib, k=8192), "grad_x small workspace": lambda: gx(lib, wb=wsb - 4), "grad_x fp16 build": lambda: gx(f16)}
    for name, call in calls.items():
        rc = call()
        assert rc != 0, name
        if "workspace" not in name:
            assert rc == -1, (name, rc)
    torch.cuda.synchronize()
    for a in outs:
        assert bool((a.float() == 3.0).all()), "a refused call wrote to its outputs"
    sd = sub(load_golden("g8_dinov2_native"), "sd.")
    with pytest.raises(ValueError, match="rank"):
        ViTLoRAEngine(sd, heads=2, r=9, device=DEV, target_modules=["query", "dense"], allow_out=True)
    with pytest.raises(NotImplementedError, match="leading-dimension"):
        ViTLoRAEngine(sd, heads=2, device=DEV, target_modules=["query", "dense"])


# ------------------------------------------------------------------------------------------------ 3. whole passes vs f64 autograd
@functools.lru_cache(maxsize=None)
def checkpoint(D):
    if D == 128:
        sd = sub(load_golden("g8_dinov2_native"), "sd.")
        return sd, 2, 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer.")), 70, 2
    return RO.d256_state_dict()


def out_engine(sd, heads, targets, lora, **kw):
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=list(targets), allow_out=True, **kw)
    assert sorted(eng.lora_state_dict()) == sorted(lora)
    eng.load_lora_state_dict(lora)
    return eng


def chunked_reference(ref_fn, masks_of, img, dkey, bounds, seeds):
    """(key, gradients) of an f64 restatement chunk by chunk: each chunk of a pass has its own masks (``masks_of(seed, images)``); gradients add."""
    key_ref, gref = [], None
    for (b0, b1), seed in zip(bounds, seeds):
        k, g = ref_fn(img[b0:b1], dkey[b0:b1], masks_of(seed, b1 - b0))
        key_ref.append(k.cpu())
        gref = {n: v.cpu() for n, v in g.items()} if gref is None else {n: gref[n] + v.cpu() for n, v in g.items()}
    return torch.cat(key_ref, 0), gref


def dinov2_masks(targets, L, tok, D, F, p_drop):
    def masks_of(seed, images):
        if p_drop == 0:
            return None
        rows = images * tok
        m = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(("query", "key", "value")) if nm in targets}
        if "fc1" in targets:
            m.update({(i, "fc1"): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
        m.update({k: v for k, v in RO.out_masks(seed, L, rows, D, F, p_drop).items() if k[1] in targets})
        return m
    return masks_of


def check_pass(name, make, reference, img, dkey, key_bar_of, grad_bar_of, L, out_paths, key_measure="max_abs"):
    eng = make()
    key = eng.forward_train(img.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    key_ref, gref = reference(list(eng._bounds), list(eng._chunk_seed))
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    assert sorted(got) == sorted(gref)
    key_err = maxdiff(key.cpu(), key_ref) if key_measure == "max_abs" else rel_l2(key, key_ref)
    key_bar = key_bar_of(key_ref)
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=lambda k: errs[k] / grad_bar_of(k))
    new = [e for k, e in errs.items() if any(p in k for p in out_paths)]
    print(f"{name}: key {key_err:.3e} (bar {key_bar:.2e}); worst gradient {errs[worst]:.3e} of bar {grad_bar_of(worst):.2e} ({worst}); worst of the new modules {max(new):.3e}")
    assert key_err < key_bar, (key_err, key_bar)
    for k, ref in gref.items():                                   # zero by structure: exact zeros
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    for p in out_paths:                                           # the last layer's new modules are among them, the layers below are not
        for ab in "AB":
            assert any(k.endswith(f"{L - 1}.{p}.lora_{ab}.weight") and float(gref[k].abs().max()) == 0.0 for k in gref), p
            assert any(k.endswith(f"0.{p}.lora_{ab}.weight") and k in errs for k in gref), p
    for k, e in errs.items():
        assert e < grad_bar_of(k), (k, e, grad_bar_of(k))
    for p, on in enumerate(eng.targets):                          # untargeted projections: parameters and gradients exactly zero
        if not on:
            for sl in eng._slices(p):
                assert float(eng.lora[:, sl].abs().max()) == 0.0 and float(eng.lora_grad[:, sl].abs().max()) == 0.0, p
    eng2 = make()                                                 # two backward runs are bit-identical
    eng2.forward_train(img.to(DEV))
    assert torch.equal(eng2.backward(dkey.to(DEV)), eng.lora_grad)
    return eng


@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("targets", RO.TARGET_SETS)
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("D", [128, 256])
def test_passes_vs_f64_autograd(D, streams, targets, p_drop):
    """Bars of tests/test_gpu_lora_targets.py for the same checkpoints: key max-abs 3e-2 max(1, |key|max) (3.0e-2 / 4.2e-2), every non-zero gradient 4e-2 (D = 128) /
    5e-2 (D = 256, and with dropout) relative L2; gradients that are zero by structure -- untargeted modules, the last layer's new modules -- are exact zeros."""
    sd, heads, L, image, B = checkpoint(D)
    F = sd["encoder.layer.0.mlp.fc1.weight"].shape[0]
    img, dkey = RO.case_inputs(B, D, image)
    lora = RO.lora_for(sd, targets)
    tok = 1 + (image // 14) ** 2

    def make():
        e = out_engine(sd, heads, targets, lora, lora_dropout=p_drop, seed=1234)
        e.train_streams = streams
        return e

    masks_of = dinov2_masks(targets, L, tok, D, F, p_drop)
    ref_fn = lambda x, dk, masks: RO.lora_grads(x, {**sd, **lora}, heads, dk, 2.0, masks=masks, device=DEV)  # noqa: E731
    bar = 4e-2 if (D == 128 and p_drop == 0) else 5e-2
    eng = check_pass(f"lora_out D={D} streams={streams} {targets} p={p_drop}", make, lambda b, s: chunked_reference(ref_fn, masks_of, img, dkey, b, s), img, dkey,
                     lambda kr: 3e-2 * max(1.0, kr.abs().max().item()), lambda k: bar, L, [RO.PATHS[t] for t in targets if t in RO.OUT_NAMES])
    n_out = sum(t in RO.OUT_NAMES for t in targets)
    assert eng.out_targets == ("dense" in targets, "fc2" in targets)
    assert eng.lora.shape == (L, 6 * 2 * D + (2 * (D + F) if "fc1" in targets else 0) + (2 * 2 * D if "dense" in targets else 0) + (2 * (F + D) if "fc2" in targets else 0))
    assert n_out > 0


def test_flag_on_without_the_new_names_is_the_engine_it_was():
    """allow_out with none of the four names targeted: arena, key map and gradients of the engine without the flag, bit for bit (the same entry points run, with a NULL table)."""
    sd, heads, L, image, B = checkpoint(128)
    img, dkey = (t.to(DEV) for t in RO.case_inputs(B, 128, image))
    lora = RO.lora_for(sd, ("query", "value", "fc1"))
    out = []
    for kw in ({}, {"allow_out": True}):
        eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=["query", "value", "fc1"],
                            lora_dropout=0.05, seed=5, **kw)
        eng.load_lora_state_dict(lora)
        assert eng.out_targets == (False, False) and eng._out_table(eng.lora_grad) is None
        key = eng.forward_train(img).clone()
        out.append((eng.lora.clone(), key, eng.backward(dkey).clone(), eng.forward_nograd(img).clone(), sum(w.numel() for w in eng._tside_ws if w is not None)))
    for a, b in zip(*out):
        assert a == b if isinstance(a, int) else torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. registers
@pytest.mark.parametrize("p_drop,streams", [(0.0, 1), (0.05, 2)])
def test_passes_with_registers(p_drop, streams):
    """R = 4 (the G21 ``native`` checkpoint of tests/test_gpu_registers.py) with [dense, fc2], under the D = 128 bars."""
    sd = RR.g21_state_dict("native")
    L, D, F, tok, targets = 3, 128, sd["encoder.layer.0.mlp.fc1.weight"].shape[0], 1 + 4 + 25, ("dense", "fc2")
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen)
    lora = RO.lora_for(sd, targets)

    def make():
        e = out_engine(sd, 2, targets, lora, lora_dropout=p_drop, seed=1234)
        e.train_streams = streams
        assert e.R == 4
        return e

    ref_fn = lambda x, dk, masks: RO.lora_grads(x, {**sd, **lora}, 2, dk, 2.0, masks=masks, device=DEV)  # noqa: E731
    bar = 4e-2 if p_drop == 0 else 5e-2
    check_pass(f"lora_out registers p={p_drop} streams={streams}", make, lambda b, s: chunked_reference(ref_fn, dinov2_masks(targets, L, tok, D, F, p_drop), img, dkey, b, s),
               img, dkey, lambda kr: 3e-2 * max(1.0, kr.abs().max().item()), lambda k: bar, L, [RO.PATHS[t] for t in targets])


# ------------------------------------------------------------------------------------------------ 5. DINOv3
@pytest.mark.parametrize("p_drop,streams", [(0.0, 1), (0.0, 2), (0.05, 2)])
def test_passes_on_dinov3(p_drop, streams):
    """G23's ``g46`` model (non-gated) with allow_rope and [q_proj, k_proj, v_proj, o_proj, down_proj], against lora_out_ref.forward_dinov3 -- which is transformers' own
    G23 values when the new modules' B is zero (tests/test_lora_out_host.py).  Bars: tests/test_gpu_dinov3_lora.py's own -- the key map's relative L2 under
    dinov3_ref.engine_bound, q / k / v gradients under dinov3_lora_ref.grad_bar; the new modules' gradients under the project's 4e-2 (5e-2 with dropout)."""
    tag = "g46"
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"g23_dinov3_lora_{tag}.npz"))
    m = R3.G22[tag]
    sd = R3.g22_state_dict(tag)
    lora = {**{k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/")}, **RO.lora_for(sd, ("o_proj", "down_proj"), seed=5)}
    x, dkey = torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])
    L, D, heads = R3.G22_LAYERS, m["D"], m["heads"]
    F = sd["model.layer.0.mlp.up_proj.weight"].shape[0]
    tok = 1 + m["R"] + m["grid"][0] * m["grid"][1]
    targets = ["q_proj", "k_proj", "v_proj", "o_proj", "down_proj"]

    def make():
        e = ViTLoRAEngine(sd, heads=heads, r=RL.G23_R, lora_alpha=RL.G23_ALPHA, eps=1e-5, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=targets,
                          allow_rope=True, allow_out=True, lora_dropout=p_drop, seed=1234)
        assert sorted(e.lora_state_dict()) == sorted(lora) and e.out_targets == (True, True) and e.rope
        e.load_lora_state_dict(lora)
        e.train_streams = streams
        return e

    def masks_of(seed, images):
        if p_drop == 0:
            return None
        rows = images * tok
        mk = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(RL.QKV)}
        mk.update(RO.out_masks(seed, L, rows, D, F, p_drop, RO.OUT_LEAVES["dinov3"]))
        return mk

    ref_fn = lambda xx, dk, masks: RO.lora_grads(xx, {**sd, **lora}, heads, dk, RL.G23_SCALE, masks=masks, device=DEV, dinov3=True)  # noqa: E731
    plain = 4e-2 if p_drop == 0 else 5e-2
    bar_of = lambda k: RL.grad_bar(z, k, p_drop) if ("ebf/" + k) in z.files else plain  # noqa: E731
    check_pass(f"lora_out dinov3 {tag} p={p_drop} streams={streams}", make, lambda b, s: chunked_reference(ref_fn, masks_of, x, dkey, b, s), x, dkey,
               lambda kr: R3.engine_bound("bf16", z), bar_of, L, ["attention.o_proj", "mlp.down_proj"], key_measure="rel_l2")
    with pytest.raises(NotImplementedError, match="pre-activation"):
        ViTLoRAEngine(R3.g22_state_dict("gated"), heads=R3.G22["gated"]["heads"], eps=1e-5, device=DEV, target_modules=["q_proj", "down_proj"], allow_rope=True,
                      allow_swiglu=True, allow_out=True)


# ------------------------------------------------------------------------------------------------ 6. the EMA teacher's pass
def test_nograd_pass_equals_the_training_forward():
    """forward_nograd (ucod_vit_forward_lora_infer_lora_out_ex) against forward_train at dropout 0, on the checkpoint of the existing infer-vs-train test and under its
    bars (tests/test_gpu_lora_targets.py test 6, the G8 model: relative L2 2e-3 on the f32 stream, 4e-3 on the fp16 one -- the bars belong to that model; a deeper one
    has no bar there); the clone for the EMA teacher runs the same pass with its own arena."""
    D = 128
    sd, heads, L, image, B = checkpoint(D)
    targets = ("query", "key", "value", "fc1", "dense", "fc2")
    lora = RO.lora_for(sd, targets)
    x = RO.case_inputs(B, D, image)[0].to(DEV)
    eng = out_engine(sd, heads, targets, lora)
    k_train = eng.forward_train(x).clone()
    k_f32, k_f16 = eng.forward_nograd(x, resid16=False).clone(), eng.forward_nograd(x, resid16=True).clone()
    eng.check_overflow(wait=True)
    base = out_engine(sd, heads, ("query", "key", "value", "fc1"), RO.without_out_modules(lora))
    moved = rel_l2(base.forward_nograd(x, resid16=False), k_train)
    print(f"nograd D={D}: f32 stream {rel_l2(k_f32, k_train):.2e} (bar 2e-3), fp16 stream {rel_l2(k_f16, k_train):.2e} (bar 4e-3); without the new modules {moved:.2e}")
    assert rel_l2(k_f32, k_train) < 2e-3 and rel_l2(k_f16, k_train) < 4e-3
    assert moved > 10 * 4e-3                                     # the modules are in that pass
    ema = eng.clone_for_ema()
    assert ema.out_targets == (True, True) and ema.lora.data_ptr() != eng.lora.data_ptr() and torch.equal(ema.forward_nograd(x, resid16=False), k_f32)


# ------------------------------------------------------------------------------------------------ 7. merging, adapters
SPLIT3_G8_BAR = 3e-6            # tests/test_gpu_lora_merge.py (tests/test_gpu_split.py::test_split_engine_against_reference_golden, terms=3 on this golden)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def test_merge_all_six_modules(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.models.modules.full_model import load_lora_adapter, save_lora_adapter
    import lora_merge_ref as M
    sd, heads, L, image, B = checkpoint(128)
    targets = ("query", "key", "value", "fc1", "dense", "fc2")
    lora = RO.lora_for(sd, targets)
    eng = out_engine(sd, heads, targets, lora)
    img = load_golden("g8_dinov2_native")["x"]
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora}.items() if v.is_floating_point()}
    ref = RO.forward(img.to(DEV, torch.float64), full, heads, eng.scaling).cpu()
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    for p in ("attention.output.dense", "mlp.fc2"):
        k = f"encoder.layer.1.{p}.weight"
        want = M.merge(sd[k], lora[f"encoder.layer.1.{p}.lora_A.weight"], lora[f"encoder.layer.1.{p}.lora_B.weight"], eng.scaling)
        assert torch.equal(merged[k], want) and not torch.equal(merged[k], sd[k]), k
    x = img.to(DEV)
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(x), ref)
    qkv_only = out_engine(sd, heads, ("query", "key", "value", "fc1"), RO.without_out_modules(lora)).merged_state_dict()
    e_without = rel_l2(SplitViTEngine(qkv_only, heads=heads, device=DEV, terms=3)(x), ref)
    print(f"merged, all six modules: split3 {e_merged:.2e} (bar {SPLIT3_G8_BAR:.0e}); with dense / fc2 left unmerged {e_without:.2e}")
    assert e_merged < SPLIT3_G8_BAR and e_without > 100 * SPLIT3_G8_BAR
    # merge_into a live engine == an engine rebuilt from merged_state_dict(), bit for bit, on every tensor of the plain tables (D = 128: no fold) -- proj and fc2 among them
    for kw in ({}, {"half": "bf16"}):
        vit = ViTEngine(sd, heads=heads, device=DEV, **kw)
        before = [[None if t is None else t.clone() for t in row] for row in vit.layers]
        ptrs = [None if t is None else t.data_ptr() for row in vit.layers for t in row]
        assert eng.merge_into(vit) is vit
        torch.cuda.synchronize()
        fresh = ViTEngine(merged, heads=heads, device=DEV, **kw)
        assert ptrs == [None if t is None else t.data_ptr() for row in vit.layers for t in row]
        for i, (ra, rb, r0) in enumerate(zip(vit.layers, fresh.layers, before)):
            for s, (a, b, c) in enumerate(zip(ra, rb, r0)):
                assert (a is None and b is None) or same_bits(a, b), (i, N.VIT_LAYER_SLOTS[s])
            for s in (N.PROJ_W, N.FC2_W):
                assert not same_bits(ra[s], r0[s]), (i, N.VIT_LAYER_SLOTS[s])
    # adapter folder -> a second engine: the new modules' tensors under peft's names, identical arenas
    folder = save_lora_adapter(eng, str(tmp_path / "lora"))
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    pre = "base_model.model.ViT.encoder.layer."
    assert sorted(tensors) == sorted(pre + k[len("encoder.layer."):] for k in lora)
    assert tensors[pre + "0.mlp.fc2.lora_A.weight"].shape == (2, 512) and tensors[pre + "0.attention.output.dense.lora_B.weight"].shape == (128, 2)
    cfg = json.load(open(os.path.join(folder, "adapter_config.json")))
    assert cfg["target_modules"] == ["query", "key", "value", "fc1", "dense", "fc2"]
    other = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(99), target_modules=list(targets), allow_out=True)
    assert not torch.equal(other.lora, eng.lora)
    load_lora_adapter(other, folder)
    assert torch.equal(other.lora, eng.lora)
    with pytest.raises(ValueError, match="target_modules"):
        load_lora_adapter(ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, target_modules=["query", "key", "value", "fc1"]), folder)
    with pytest.raises(KeyError, match="dense"):
        other2 = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, target_modules=["query", "key", "value", "fc1", "fc2"], allow_out=True)
        other2.load_lora_state_dict({k: v for k, v in eng.lora_state_dict().items()})


# ------------------------------------------------------------------------------------------------ 8. one training step of the runner
def test_runner_trains_the_output_modules(tmp_path):
    """lora_cfg.allow_out through load_lora into the runner's backbone-backward step (the small geometry of tests/test_gpu_lora_merge.py's runner test): the loss is
    finite, the new modules' arena rows move (B away from peft's zeros), the checkpoint's lora/ folder holds their tensors."""
    from safetensors.torch import load_file, save_file
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.models.modules.full_model import load_lora
    sd, heads, L, image, B = checkpoint(128)
    weights = tmp_path / "weights"
    weights.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(weights / "model.safetensors"))
    (weights / "config.json").write_text(json.dumps({"model_type": "dinov2", "num_attention_heads": 2, "layer_norm_eps": 1e-6}))
    cfg = CfgNode(dict(
        model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, dis_use_features=False),
        lora_cfg=dict(r=2, lora_alpha=4, lora_dropout=0.05, target_modules=["query", "key", "value", "dense", "fc2"], allow_out=True),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=6e-4, dis_lr0=1e-3, step_lr_size=2, dis_step_lr_size=2,
                       step_lr_gamma=0.95, dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1,
                       dis_intertrain=2, save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50),
        dataset_cfg=dict(feature_extractor_cfg=dict(type="dinov2", backbone_type="huggingface", backbone="facebook/dinov2-base", backbone_weights=str(weights))),
        log_cfg=dict(log_interval=50, log_path=str(tmp_path / "log"), multi_rank=[0])))
    torch.manual_seed(3)
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    eng = load_lora(cfg.lora_cfg, sd, heads=heads, device=DEV, generator=torch.Generator().manual_seed(1)).engine
    assert eng.allow_out and eng.out_targets == (True, True) and eng.mlp_target is None and eng.lora_dropout == 0.05
    loop.attach_lora_backbone(eng)
    assert loop.lora_engine_ema.out_targets == (True, True)
    before = eng.lora.clone()
    img = load_golden("g8_dinov2_native")["x"].to(DEV)
    pl = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(11)) > 0.5).float()
    loss = loop._process_batch_full(img, pl)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    for m in (0, 1):
        sa, sb = eng._out_slices(m)
        assert float(before[:, sb].abs().max()) == 0.0 and float(before[:, sa].abs().min(dim=1).values.max()) >= 0.0
        assert bool((eng.lora[:L - 1, sb].abs().amax(dim=1) > 0).all()), m                                           # B of every layer below the last moved
        assert float(eng.lora[L - 1, sb].abs().max()) == 0.0                                                         # the last layer's modules never reach the key map
    runner.save_checkpoint(2)
    path = os.path.join(cfg.log_cfg.log_path, "ckp", "epoch2.pth")
    assert sorted(os.listdir(path)) == ["lora", "lora_ema", "model.safetensors"]
    saved = load_file(os.path.join(path, "lora", "adapter_model.safetensors"))
    pre = "base_model.model.ViT.encoder.layer."
    for i in range(L):
        for p in ("attention.output.dense", "mlp.fc2"):
            for ab in "AB":
                assert f"{pre}{i}.{p}.lora_{ab}.weight" in saved, (i, p, ab)
    assert torch.equal(saved[pre + "0.mlp.fc2.lora_B.weight"], eng.lora_state_dict()["encoder.layer.0.mlp.fc2.lora_B.weight"].cpu())
    assert json.load(open(os.path.join(path, "lora", "adapter_config.json")))["target_modules"] == ["query", "key", "value", "dense", "fc2"]


# ------------------------------------------------------------------------------------------------ 9. the older tiers of the pass entry points
def older_tiers(lib, mlp, TM, TO):
    """{tier: (train size, forward_train, backward, no-grad size, forward_lora_infer)} of every tier below _lora_out_ex that can express the configuration, each with
    the arguments between the descriptor and the image / dkey bound: f(t, T, TT, ...) for the passes, f(t) for the sizes."""
    five = ("ucod_vit_train_workspace_bytes{}", "ucod_vit_forward_train{}", "ucod_vit_backward{}", "ucod_vit_lora_infer_workspace_bytes{}", "ucod_vit_forward_lora_infer{}")

    def bind(suffix, lead, tabs):
        fns = [getattr(lib, n.format(suffix)) for n in five]
        size = lambda f: lambda t: f(t, *lead, *tabs)  # noqa: E731
        run = lambda f: lambda t, T, TT, *rest: f(t, *lead, T, TT, *tabs, *rest)  # noqa: E731
        return size(fns[0]), run(fns[1]), run(fns[2]), size(fns[3]), run(fns[4])

    tiers = {"_lora_out": bind("_lora_out", (mlp,), (TM, TO))}
    if TO is None:
        tiers["_lora_mlp"] = bind("_lora_mlp", (mlp,), (TM,))
    if TO is None and TM is None:
        tiers["_mlp"] = bind("_mlp", (mlp,), ())
    if TO is None and TM is None and mlp == N.UCOD_MLP_GELU:
        tiers["plain"] = bind("", (), ())
    return tiers


@pytest.mark.parametrize("kind,targets,expect", [("gelu", ("query", "key", "value"), {"plain", "_mlp", "_lora_mlp", "_lora_out"}),
                                                 ("gelu", ("query", "key", "value", "fc1"), {"_lora_mlp", "_lora_out"}),
                                                 ("gelu", ("query", "key", "value", "dense", "fc2"), {"_lora_out"}),
                                                 ("swiglu", ("query", "key", "value"), {"_mlp", "_lora_mlp", "_lora_out"})])
def test_older_tiers_run_the_engines_passes(kind, targets, expect):
    """The engine makes one call per pass, to the _lora_out_ex tier.  Every older tier that can express the engine's configuration -- the same descriptor, tables and
    chunk seed, its own zeroed workspace and gradient buffer -- gives the engine's key map, gradients and no-grad key map bit for bit (the passes reproduce from run
    to run, dropout on: test_flag_on_without_the_new_names_is_the_engine_it_was relies on the same), and its size functions the engine's workspace sizes."""
    sd, heads, L, image, B = checkpoint(128) if kind == "gelu" else (RS.g24_state_dict("dinov2"), 2, 3, 70, 2)
    ref = RO if kind == "gelu" else RS
    lora = ref.lora_for(sd, targets)
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=list(targets), allow_out=True,
                        allow_swiglu=(kind == "swiglu"), lora_dropout=0.05, seed=1234)
    eng.load_lora_state_dict(lora)
    eng.train_streams = 1
    D = eng.D
    assert D == 128 and L == 3 and eng.mlp == (N.UCOD_MLP_SWIGLU if kind == "swiglu" else N.UCOD_MLP_GELU) and eng._out_flags == 0
    x, dkey = (t.to(DEV) for t in RO.case_inputs(B, D, image))
    key = eng.forward_train(x).clone()
    seed_train = eng._chunk_seed[0]
    grad = eng.backward(dkey).clone()
    key_ng = eng.forward_nograd(x).clone()                        # (the fp16 residual stream, the teacher's default)
    seed_ng = eng._seed_of_chunk(0, 0)
    eng.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert float(grad.abs().max()) > 0 and not torch.equal(key, key_ng)
    n_train, n_ng = eng._tside_ws[0].numel(), eng._iside_ws[0].numel()
    lib, gh, P, st = eng.lib, image // 14, N.ptr, N.stream()
    g = torch.zeros_like(eng.lora_grad)
    T, TT, TM, keep = eng._tables(gh, gh, g)
    TO = eng._out_table(g)
    assert (TM is not None) == ("fc1" in targets) and (TO is not None) == ("dense" in targets)
    tiers = older_tiers(lib, eng.mlp, TM, TO)
    assert set(tiers) == expect
    t = eng._train_desc(B, image, image, seed_train)
    tn = eng._train_desc(B, image, image, seed_ng)
    tn.vit.resid16 = 1
    for name, (train_bytes, fwd, bwd, ng_bytes, fwd_ng) in tiers.items():
        assert train_bytes(C.byref(t)) == n_train and ng_bytes(C.byref(tn)) == n_ng, name
        ws, ws_ng = torch.zeros(n_train, dtype=torch.uint8, device=DEV), torch.zeros(n_ng, dtype=torch.uint8, device=DEV)
        k, k_ng = torch.full_like(key, 3.0), torch.full_like(key, 3.0)
        g.zero_()
        assert fwd(C.byref(t), T, TT, P(x), P(k), P(ws), n_train, st) == 0, name
        assert bwd(C.byref(t), T, TT, P(dkey), P(ws), n_train, st) == 0, name
        assert fwd_ng(C.byref(tn), T, TT, P(x), P(k_ng), P(ws_ng), n_ng, st) == 0, name
        torch.cuda.synchronize()
        assert torch.equal(k, key), name
        assert torch.equal(g, grad), name
        assert torch.equal(k_ng, key_ng), name
