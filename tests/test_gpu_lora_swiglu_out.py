"""GPU: LoRA on the SwiGLU MLP's output projection -- ``mlp.weights_out`` of a DINOv2 SwiGLU checkpoint, ``mlp.down_proj`` of a gated DINOv3 one -- the opt-in
``allow_swiglu_out`` of ViTLoRAEngine (models/modules/full_model.py:47-72 hands ``target_modules`` to peft), every call through the C ABI or the engine.

1-2  ucod_lora_out_grad_x_ex with UCOD_LORA_OUT_ACT_SWIGLU (behind ucod_lora_out_grad_s) and ucod_lora_out_fwd at K = 4096, alone, against f64 torch on the formulas
     of tests/lora_swiglu_out_ref.py, with canary rows around every output;
3-4  whole passes against f64 autograd through that restatement (pinned on transformers' own values by tests/test_lora_swiglu_out_host.py) and against the G24
     goldens themselves;
5-8  the no-grad pass, both merges, the adapter folder, and the engine with the flag off or the module not targeted.

No bar is taken from a run of this code.  Kernels: tests/test_gpu_lora_out.py's for the same quantities -- t 1e-2, dA and dB 2e-4, the bf16 cotangent 1e-2, the f32 /
fp16 stream 2e-5 / 2e-5 + 2^-11, all relative to max(1, |ref|max).  Passes: tests/test_gpu_lora_targets.py's SwiGLU D = 128 bars, key max-abs 3e-2 max(1, |key|max),
gradients 4e-2 relative L2; on the goldens dinov3_lora_ref.grad_bar (max(4e-2, 3 x the error of CPU bf16 autocast)) and dinov3_ref.engine_bound("bf16") for the key
map; no-grad pass 2e-3 / 4e-3 and merged split3 3e-6 as tests/test_gpu_lora_out.py holds fc2 to.

Measured on MI355X (profiles/lora_swiglu_out_tests.txt), worst over the cases: kernels alone -- t 1.1e-7, dA 2.1e-7, dB 2.1e-7, dpre 3.3e-3, u 1.1e-7, f32 stream 1.2e-7, fp16
stream 2.5e-4; passes -- key 3.1e-3 (bar 3.0e-2), gradients 1.3e-2 (4e-2); G24 DINOv2 key 2.8e-3 rel-L2 (1.08e-2), gradients 9.5e-3 (4e-2); G24 gated DINOv3 key 3.4e-3
(1.24e-2), gradients 1.5e-2 (4.2e-2); no-grad pass 1.7e-3 (2e-3) on the f32 stream, bit-identical on the fp16 one; merged split3 5.1e-7 (3e-6)."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, ViTLoRAEngine  # noqa: E402
from oracle import vit as OV  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402

DEV = "cuda"
GUARD_ROWS = 16
W = N.LORA_OUT_W
ALL = dict(allow_out=True, allow_swiglu_out=True)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


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


def interleave(x1, x2):
    """x1, x2 [rows, K] -> the engine's pre-activation order [rows, 2K]: columns 8k + e hold x1 of unit 4k + e, columns 8k + 4 + e its x2 (ucod_dpl_amd/swiglu.py)."""
    rows, K = x1.shape
    return torch.stack((x1.reshape(rows, K // 4, 4), x2.reshape(rows, K // 4, 4)), 2).reshape(rows, 2 * K)


def deinterleave(y):
    rows, K2 = y.shape
    z = y.reshape(rows, K2 // 8, 2, 4)
    return z[:, :, 0].reshape(rows, K2 // 2), z[:, :, 1].reshape(rows, K2 // 2)


# ------------------------------------------------------------------------------------------------ 1. the SwiGLU form of grad_x
# (rows, K, D, live units): 111 rows are no multiple of the four rows in flight and K = 384 has 40 padded units (pre-activation and A columns zero there); 2740 rows are
# more than the 256 x 4 a grid covers in one sweep (K = 512: one column slab of 128 threads); K = 4096 with D = 1536 is the register ceiling of both kernels (8 slabs).
SHAPES = [(111, 384, 128, 344), (2740, 512, 256, 512), (111, 4096, 1536, 4096)]
SEED, KEY = 0x1234ABCD5678, 29


@functools.lru_cache(maxsize=None)
def operands(M, K, D, K0, r, p_drop):
    """bf16-rounded operands of one shape and its f64 reference (computed once, never modified): the hidden, dA and the two dpre terms by autograd over the LoRA
    branch of lora_swiglu_out_ref.swiglu_out_linear, with the kernel's t as the branch's cotangent."""
    g = torch.Generator().manual_seed(M + K + D + r)
    live = (torch.arange(K) < K0).float()
    A = torch.randn(r, K, generator=g) / math.sqrt(K) * live
    Bo = torch.randn(D, r, generator=g) * 0.3
    x1 = (torch.randn(M, K, generator=g) * 1.5 * live).bfloat16()
    x2 = (torch.randn(M, K, generator=g) * live).bfloat16()
    s = torch.randn(M, D, generator=g).bfloat16()
    cot = torch.randn(M, 2 * K, generator=g).bfloat16()
    u = torch.full((M, W), 55.0)                                 # columns beyond the rank are never read
    u[:, :r] = torch.randn(M, r, generator=g)
    mask = OV.lora_dropout_mask(SEED, KEY, 0, M, K, p_drop).double().reshape(M, K) if p_drop > 0 else torch.ones(M, K, dtype=torch.float64)
    return dict(scaling=2.0, flat=torch.cat((A.reshape(-1), Bo.reshape(-1))).to(DEV), A=A.double(), B=Bo.double(), x1=x1, x2=x2, s=s, cot=cot, u=u, mask=mask)


def branch_grads(o, t):
    """d/d(A, x1, x2) of <t, (mask * silu(x1) x2) A^T>: dA and the terms dpre takes, by autograd over the restatement's LoRA branch (scale 1, B = identity rows)."""
    r = t.shape[1]
    A = o["A"].clone().requires_grad_(True)
    x1, x2 = o["x1"].double().requires_grad_(True), o["x2"].double().requires_grad_(True)
    sd = {"w.weight": torch.zeros(r, A.shape[1], dtype=torch.float64), "w.bias": torch.zeros(r, dtype=torch.float64), "w.lora_A.weight": A,
          "w.lora_B.weight": torch.eye(r, dtype=torch.float64)}
    y = RS.swiglu_out_linear(x1, x2, sd, "w", 1.0, o["mask"])
    return torch.autograd.grad((y * t).sum(), [A, x1, x2])


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("r", [1, 2, 8])
@pytest.mark.parametrize("M,K,D,K0", SHAPES)
def test_lora_out_grad_swiglu(M, K, D, K0, r, p_drop):
    """ucod_lora_out_grad_s, then ucod_lora_out_grad_x_ex(UCOD_LORA_OUT_ACT_SWIGLU, UCOD_LORA_OUT_SWIGLU) on the interleaved pre-activation and dpre [M, 2K], twice: bit-identical, nothing
    outside the outputs written, dA on padded units exactly zero."""
    o = operands(M, K, D, K0, r, p_drop)
    lib = N.load()
    wsb = lib.ucod_lora_out_grad_workspace_bytes(r, K, D)
    assert wsb > 0
    pre = interleave(o["x1"], o["x2"]).to(DEV)
    sdev, udev = o["s"].to(DEV), o["u"].to(DEV)
    t_ref = o["scaling"] * o["s"].double() @ o["B"]
    dB_ref = o["scaling"] * o["s"].double().t() @ o["u"][:, :r].double()
    runs = []
    for _ in range(2):
        ws = FlatGuarded(wsb // 4)
        t, grad, cot = Guarded(M, W, torch.float32), Guarded(1, r * (K + D), torch.float32), Guarded(M, 2 * K, torch.bfloat16, fill=o["cot"].to(DEV))
        rc = lib.ucod_lora_out_grad_s(N.ptr(sdev), N.ptr(udev), N.ptr(o["flat"]), r, o["scaling"], grad.ptr(), t.ptr(), ws.ptr(), wsb, M, K, D, N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool(torch.isnan(grad.payload.reshape(-1)[:r * K]).all()), "grad_s wrote into the A part"
        rc = lib.ucod_lora_out_grad_x_ex(N.ptr(pre), N.LORA_OUT_ACT_SWIGLU, N.LORA_OUT_SWIGLU, cot.ptr(), t.ptr(), N.ptr(o["flat"]), r, grad.ptr(), ws.ptr(), wsb, M, K, D,
                                      drop_arg(p_drop, SEED, KEY), N.stream())
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
    dA_ref, d1, d2 = branch_grads(o, tk)                        # (dA from the t the kernel wrote, as tests/test_gpu_lora_out.py takes it)
    c1, c2 = deinterleave(o["cot"].double())
    cot_ref = interleave(c1 + d1, c2 + d2)
    gA, gB = grad[:r * K].reshape(r, K), grad[r * K:].reshape(D, r)
    e_t = maxdiff(tk, t_ref) / max(1.0, t_ref.abs().max().item())
    e_a = maxdiff(gA, dA_ref) / max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, dB_ref) / max(1.0, dB_ref.abs().max().item())
    e_c = maxdiff(cot_out, cot_ref) / max(1.0, cot_ref.abs().max().item())
    print(f"lora_out_grad swiglu {(M, K, D, r)} p={p_drop}: t {e_t:.2e} (bar 1e-2) dA {e_a:.2e} (2e-4) dB {e_b:.2e} (2e-4) dpre {e_c:.2e} (1e-2)")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4 and e_c < 1e-2, (e_t, e_a, e_b, e_c)
    assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0 and maxdiff(cot_out, o["cot"].double()) > 0.05
    if K0 < K:                                                   # padded units: dA exactly zero, dpre untouched bit for bit
        assert float(gA[:, K0:].abs().max()) == 0.0
        got1, got2 = deinterleave(runs[0][2].cpu())
        assert torch.equal(bits(got1[:, K0:]), bits(deinterleave(o["cot"])[0][:, K0:])) and torch.equal(bits(got2[:, K0:]), bits(deinterleave(o["cot"])[1][:, K0:]))
    # teeth: dA from silu(x1) alone, and a dpre without the x2 half of the term, are far from what the kernel gave
    x1, x2 = o["x1"].double(), o["x2"].double()
    assert maxdiff(gA, tk.t() @ (TF.silu(x1) * o["mask"])) / max(1.0, dA_ref.abs().max().item()) > 1e-2
    assert maxdiff(cot_out, interleave(c1 + d1, c2)) / max(1.0, cot_ref.abs().max().item()) > 3e-2
    if p_drop > 0:                                               # ... and so is the unmasked dA
        assert maxdiff(gA, tk.t() @ (TF.silu(x1) * x2)) / max(1.0, dA_ref.abs().max().item()) > 1e-2


def test_swiglu_refusals_leave_outputs_untouched():
    M, K, D, K0, r = 111, 384, 128, 344, 2
    o = operands(M, K, D, K0, r, 0.0)
    lib, f16 = N.load(), N.load("f16")
    wsb = lib.ucod_lora_out_grad_workspace_bytes(r, K, D)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    t, grad = torch.full((M, W), 3.0, device=DEV), torch.full((r * (K + D),), 3.0, device=DEV)
    cot = torch.full((M, 2 * K), 3.0, dtype=torch.bfloat16, device=DEV)
    pre = interleave(o["x1"], o["x2"]).to(DEV)
    P, st = N.ptr, N.stream()

    def gx(l, xp=P(pre), cp=P(cot), act=N.LORA_OUT_ACT_SWIGLU, rr=r, k=K, wb=wsb, fl=N.LORA_OUT_SWIGLU):
        return l.ucod_lora_out_grad_x_ex(xp, act, fl, cp, P(t), P(o["flat"]), rr, P(grad), P(ws), wb, M, k, D, None, st)

    calls = {"null pre": lambda: gx(lib, xp=None), "null dpre": lambda: gx(lib, cp=None), "act 3": lambda: gx(lib, act=3), "act -1": lambda: gx(lib, act=-1), "act 2 without its flag": lambda: gx(lib, fl=0),
             "unknown flag bit": lambda: gx(lib, fl=N.LORA_OUT_SWIGLU | 2), "unknown flag bit, gelu": lambda: gx(lib, act=N.LORA_OUT_ACT_GELU, fl=2),
             "act 2 through the plain entry point": lambda: lib.ucod_lora_out_grad_x(P(pre), 2, P(cot), P(t), P(o["flat"]), r, P(grad), P(ws), wsb, M, K, D, None, st),
             "rank 9": lambda: gx(lib, rr=9), "K = 5120": lambda: gx(lib, k=5120), "K = 344": lambda: gx(lib, k=344), "small workspace": lambda: gx(lib, wb=wsb - 4),
             "fp16 build": lambda: gx(f16)}
    for name, call in calls.items():
        rc = call()
        assert rc != 0, name
        if "workspace" not in name:
            assert rc == -1, (name, rc)
    torch.cuda.synchronize()
    for a in (grad, cot):
        assert bool((a.float() == 3.0).all()), "a refused call wrote to its outputs"


# ------------------------------------------------------------------------------------------------ 2. the forward kernel at K = 4096
@pytest.mark.parametrize("h16", [False, True])
def test_lora_out_fwd_at_the_widest_input(h16):
    """(111, 4096, 1536, r = 8): the two-vectors-per-thread form at its last vector, the widest stream row; on the hidden a SwiGLU pass hands it (any bf16 [M, F])."""
    M, K, D, r, p_drop = 111, 4096, 1536, 8, 0.5
    g = torch.Generator().manual_seed(M + K + D + r)
    A, Bo = torch.randn(r, K, generator=g) / math.sqrt(K), torch.randn(D, r, generator=g) * 0.3
    lam = torch.rand(D, generator=g) + 0.5
    x_in = (TF.silu(torch.randn(M, K, generator=g)) * torch.randn(M, K, generator=g)).bfloat16()
    x0 = torch.randn(M, D, generator=g) * 2
    x0 = x0.half() if h16 else x0
    mask = OV.lora_dropout_mask(SEED, KEY, 0, M, K, p_drop).double().reshape(M, K)
    flat = torch.cat((A.reshape(-1), Bo.reshape(-1))).to(DEV)
    u_ref = (x_in.double() * mask) @ A.double().t()
    x_ref = x0.double() + lam.double() * (2.0 * u_ref @ Bo.double().t())
    lib = N.load()
    xin, lamd = x_in.to(DEV), lam.to(DEV)
    runs = []
    for _ in range(2):
        xs, u = Guarded(M, D, x0.dtype, fill=x0.to(DEV)), Guarded(M, W, torch.float32)
        rc = lib.ucod_lora_out_fwd(N.ptr(xin), N.ptr(flat), r, 2.0, N.ptr(lamd), xs.ptr(), int(h16), u.ptr(), M, K, D, drop_arg(p_drop, SEED, KEY), N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert xs.guards_intact() and u.guards_intact(), "wrote outside its outputs"
        runs.append((xs.payload.clone(), u.payload.clone()))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    xg, ug = runs[0][0].double().cpu(), runs[0][1].cpu()
    assert bool(torch.isfinite(ug).all()) and bool(torch.isfinite(xg).all()), "left elements unwritten"
    e_u = maxdiff(ug[:, :r], u_ref) / max(1.0, u_ref.abs().max().item())
    e_x = maxdiff(xg, x_ref) / max(1.0, x_ref.abs().max().item())
    bar_x = 2e-5 + (2.0 ** -11 if h16 else 0.0)
    print(f"lora_out_fwd {(M, K, D, r)} p={p_drop} h16={h16}: u {e_u:.2e} (bar 1e-2), stream {e_x:.2e} (bar {bar_x:.2e})")
    assert e_u < 1e-2 and e_x < bar_x, (e_u, e_x)
    assert maxdiff(xg, x0.double()) > 0.1 and maxdiff(ug[:, :r], x_in.double() @ A.double().t()) > 0.05       # the update is there, and the mask matters
    assert K > 4095 and lib.ucod_lora_out_fwd(N.ptr(xin), N.ptr(flat), r, 2.0, N.ptr(lamd), runs[0][0].data_ptr(), int(h16), None, M, K + 128, D, None, N.stream()) == -1


# ------------------------------------------------------------------------------------------------ 3. whole passes vs f64 autograd
@functools.lru_cache(maxsize=None)
def checkpoint():
    """The tiny SwiGLU model of tests/test_gpu_lora_targets.py (G24's ``dinov2``): (state dict, heads, L, image size, batch)."""
    return RS.g24_state_dict("dinov2"), 2, 3, 70, 2


def case_inputs(B, D, image, patch=14, seed=7):
    gen = torch.Generator().manual_seed(seed)
    gh = image // patch
    return torch.randn(B, 3, image, image, generator=gen), torch.randn(B, D, gh, gh, generator=gen)


def swiglu_engine(sd, heads, targets, lora, **kw):
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=list(targets), allow_swiglu=True,
                        **ALL, **kw)
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


def dinov2_masks(targets, L, tok, D, F0, p_drop):
    def masks_of(seed, images):
        if p_drop == 0:
            return None
        rows = images * tok
        m = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(("query", "key", "value")) if nm in targets}
        if "weights_in" in targets:
            m.update({(i, "weights_in"): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
        m.update({k: v for k, v in RS.out_masks(seed, L, rows, D, F0, p_drop).items() if k[1] in targets})
        return m
    return masks_of


def check_pass(name, make, reference, img, dkey, key_bar_of, grad_bar_of, L, out_paths, key_measure="max_abs"):
    """tests/test_gpu_lora_out.py's check of one pass: key map and every non-zero gradient under their bars, structural zeros exact, two runs bit-identical."""
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
    print(f"{name}: key {key_err:.3e} (bar {key_bar:.2e}); worst gradient {errs[worst]:.3e} of bar {grad_bar_of(worst):.2e} ({worst}); worst of the output modules {max(new):.3e}")
    assert key_err < key_bar, (key_err, key_bar)
    for k, ref in gref.items():                                   # zero by structure: exact zeros
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    for p in out_paths:                                           # the last layer's output modules are among them, the layers below are not
        for ab in "AB":
            assert any(k.endswith(f"{L - 1}.{p}.lora_{ab}.weight") and float(gref[k].abs().max()) == 0.0 for k in gref), p
            assert any(k.endswith(f"0.{p}.lora_{ab}.weight") and k in errs for k in gref), p
    for k, e in errs.items():
        assert e < grad_bar_of(k), (k, e, grad_bar_of(k))
    for p, on in enumerate(eng.targets):                          # untargeted projections: parameters and gradients exactly zero
        if not on:
            for sl in eng._slices(p):
                assert float(eng.lora[:, sl].abs().max()) == 0.0 and float(eng.lora_grad[:, sl].abs().max()) == 0.0, p
    if eng.out_targets[1] and eng.F != eng._F0:                   # the padded hidden units' columns of A_2: parameters and gradients exactly zero
        sa, _ = eng._out_slices(1)
        for arena in (eng.lora, eng.lora_grad):
            assert float(arena[:, sa].reshape(L, eng.r, eng.F)[:, :, eng._F0:].abs().max()) == 0.0
    eng2 = make()                                                 # two backward runs are bit-identical
    eng2.forward_train(img.to(DEV))
    assert torch.equal(eng2.backward(dkey.to(DEV)), eng.lora_grad)
    return eng


TARGET_SETS = (("weights_out",), ("dense", "weights_out"), ("query", "key", "value", "weights_in", "dense", "weights_out"))


@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("targets", TARGET_SETS)
@pytest.mark.parametrize("streams", [1, 2])
def test_passes_vs_f64_autograd(streams, targets, p_drop):
    """The D = 128 SwiGLU model (hidden width 344, padded to 384) under tests/test_gpu_lora_targets.py's bars for it: key max-abs 3e-2 max(1, |key|max), every non-zero
    gradient 4e-2 relative L2; gradients that are zero by structure are exact zeros."""
    sd, heads, L, image, B = checkpoint()
    D, F0 = 128, 344
    img, dkey = case_inputs(B, D, image)
    lora = RS.lora_for(sd, targets)
    tok = 1 + (image // 14) ** 2

    def make():
        e = swiglu_engine(sd, heads, targets, lora, lora_dropout=p_drop, seed=1234)
        e.train_streams = streams
        return e

    masks_of = dinov2_masks(targets, L, tok, D, F0, p_drop)
    ref_fn = lambda x, dk, masks: RS.lora_grads(x, {**sd, **lora}, heads, dk, 2.0, masks=masks, device=DEV)  # noqa: E731
    eng = check_pass(f"lora_swiglu_out streams={streams} {targets} p={p_drop}", make, lambda b, s: chunked_reference(ref_fn, masks_of, img, dkey, b, s), img, dkey,
                     lambda kr: 3e-2 * max(1.0, kr.abs().max().item()), lambda k: 4e-2, L, [RS.PATHS[t] for t in targets if t in RS.OUT_NAMES])
    assert eng.out_targets == ("dense" in targets, True) and eng._out_flags == N.LORA_OUT_SWIGLU and (eng.F, eng._F0) == (384, F0)
    assert eng.lora.shape == (L, 6 * 2 * D + (2 * (D + 2 * 384) if "weights_in" in targets else 0) + (2 * 2 * D if "dense" in targets else 0) + 2 * (384 + D))


# ------------------------------------------------------------------------------------------------ 4. against transformers' own values (G24)
@pytest.mark.parametrize("tag,streams", [("dinov2", 1), ("dinov2", 2), ("gated", 1), ("gated", 2)])
def test_passes_on_the_goldens(tag, streams):
    """Both G24 models with every module the engine can target on them, against transformers' f64 key map and gradients: the key map's relative L2 under
    dinov3_ref.engine_bound("bf16") (3 x transformers under bf16 autocast), every gradient under dinov3_lora_ref.grad_bar (max(4e-2, 3 x autocast's error))."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"g24_lora_swiglu_out_{tag}.npz"))
    sd = RS.g24_state_dict(tag)
    lora = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/")}
    x, dkey = torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])
    targets = list(RS.G24_TARGETS[tag])
    gated = tag == "gated"

    def make():
        e = ViTLoRAEngine(sd, heads=RS.G24_HEADS, r=RS.G24_R, lora_alpha=RS.G24_ALPHA, eps=1e-5 if gated else 1e-6, device=DEV, generator=torch.Generator().manual_seed(3),
                          target_modules=targets, allow_swiglu=True, allow_rope=gated, **ALL)
        assert sorted(e.lora_state_dict()) == sorted(lora) and e.out_targets == (True, True) and bool(e.rope) == gated and e._out_flags == N.LORA_OUT_SWIGLU
        e.load_lora_state_dict(lora)
        e.train_streams = streams
        return e

    golden = (torch.from_numpy(z["key"]), {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad/")})
    leaves = RS.OUT_LEAVES[RS.G24_FAMILY[tag]]
    check_pass(f"lora_swiglu_out G24 {tag} streams={streams}", make, lambda b, s: golden, x, dkey, lambda kr: R3.engine_bound("bf16", z), lambda k: RS.grad_bar(z, k),
               3, [RS.PATHS[t] for t in leaves], key_measure="rel_l2")


# ------------------------------------------------------------------------------------------------ 5. the EMA teacher's pass
def test_nograd_pass_equals_the_training_forward():
    """forward_nograd (ucod_vit_forward_lora_infer_lora_out_ex) against forward_train at dropout 0, under the bars tests/test_gpu_lora_out.py holds the same pair to with
    fc2 on its D = 128 model (relative L2 2e-3 on the f32 stream, 4e-3 on the fp16 one); the clone for the EMA teacher runs the same pass with its own arena."""
    sd, heads, L, image, B = checkpoint()
    targets = TARGET_SETS[2]
    lora = RS.lora_for(sd, targets)
    x = case_inputs(B, 128, image)[0].to(DEV)
    eng = swiglu_engine(sd, heads, targets, lora)
    k_train = eng.forward_train(x).clone()
    k_f32, k_f16 = eng.forward_nograd(x, resid16=False).clone(), eng.forward_nograd(x, resid16=True).clone()
    eng.check_overflow(wait=True)
    base = swiglu_engine(sd, heads, targets[:-1], RS.without(lora, "weights_out"))
    moved = rel_l2(base.forward_nograd(x, resid16=False), k_train)
    print(f"nograd swiglu D=128: f32 stream {rel_l2(k_f32, k_train):.2e} (bar 2e-3), fp16 stream {rel_l2(k_f16, k_train):.2e} (bar 4e-3); without weights_out {moved:.2e}")
    assert rel_l2(k_f32, k_train) < 2e-3 and rel_l2(k_f16, k_train) < 4e-3
    assert moved > 10 * 4e-3                                     # the module is in that pass
    ema = eng.clone_for_ema()
    assert ema.out_targets == (True, True) and ema._out_flags == N.LORA_OUT_SWIGLU and ema.lora.data_ptr() != eng.lora.data_ptr()
    assert torch.equal(ema.forward_nograd(x, resid16=False), k_f32)


# ------------------------------------------------------------------------------------------------ 6. merging, adapters
SPLIT3_BAR = 3e-6               # tests/test_gpu_lora_merge.py / tests/test_gpu_lora_out.py: a merged model on SplitViTEngine(terms=3) against the f64 LoRA forward


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def test_merge_and_adapter_with_weights_out(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.models.modules.full_model import load_lora, load_lora_adapter, save_lora_adapter
    from ucod_dpl_amd.engine.config import CfgNode
    import lora_merge_ref as M
    sd, heads, L, image, B = checkpoint()
    targets = TARGET_SETS[2]
    lora = RS.lora_for(sd, targets)
    eng = swiglu_engine(sd, heads, targets, lora)
    img = case_inputs(B, 128, image)[0]
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora}.items() if v.is_floating_point()}
    ref = RS.forward(img.to(DEV, torch.float64), full, heads, eng.scaling).cpu()
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    k = "encoder.layer.1.mlp.weights_out.weight"
    want = M.merge(sd[k], lora["encoder.layer.1.mlp.weights_out.lora_A.weight"], lora["encoder.layer.1.mlp.weights_out.lora_B.weight"], eng.scaling)
    assert merged[k].shape == (128, 344) and torch.equal(merged[k], want) and not torch.equal(merged[k], sd[k])
    x = img.to(DEV)
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(x), ref)
    rest = swiglu_engine(sd, heads, targets[:-1], RS.without(lora, "weights_out")).merged_state_dict()
    e_without = rel_l2(SplitViTEngine(rest, heads=heads, device=DEV, terms=3)(x), ref)
    print(f"merged, all six modules of the SwiGLU block: split3 {e_merged:.2e} (bar {SPLIT3_BAR:.0e}); with weights_out left unmerged {e_without:.2e}")
    assert e_merged < SPLIT3_BAR and e_without > 100 * SPLIT3_BAR
    # merge_into a live engine == an engine rebuilt from merged_state_dict(), bit for bit, on every tensor of the plain tables -- the zero-padded [D, F] weights_out too
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
            assert ra[N.FC2_W].shape == (128, 384) and float(ra[N.FC2_W][:, 344:].float().abs().max()) == 0.0
            assert not same_bits(ra[N.FC2_W], r0[N.FC2_W]) and not same_bits(ra[N.PROJ_W], r0[N.PROJ_W]), i
    # adapter folder -> a second engine built through load_lora (lora_cfg.allow_swiglu_out): peft's names, HF shapes, identical arenas
    folder = save_lora_adapter(eng, str(tmp_path / "lora"))
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    pre = "base_model.model.ViT.encoder.layer."
    assert sorted(tensors) == sorted(pre + k[len("encoder.layer."):] for k in lora)
    assert tensors[pre + "0.mlp.weights_out.lora_A.weight"].shape == (2, 344) and tensors[pre + "0.mlp.weights_out.lora_B.weight"].shape == (128, 2)
    assert json.load(open(os.path.join(folder, "adapter_config.json")))["target_modules"] == list(targets)
    cfg = CfgNode(dict(r=2, lora_alpha=4, lora_dropout=0.0, target_modules=list(targets), allow_out=True, allow_swiglu_out=True))
    other = load_lora(cfg, sd, heads=heads, device=DEV, generator=torch.Generator().manual_seed(99)).engine
    assert other.allow_swiglu_out and other.out_targets == (True, True) and not torch.equal(other.lora, eng.lora)
    sa, sb = other._out_slices(1)                                  # the constructor's own init: A_2 uniform within 1 / sqrt(F0) on the live units, zeros on the padding, B_2 = 0
    a0 = other.lora[:, sa].reshape(L, 2, 384)
    assert float(a0[:, :, 344:].abs().max()) == 0.0 and 0 < float(a0.abs().max()) <= 344 ** -0.5 and float(other.lora[:, sb].abs().max()) == 0.0
    load_lora_adapter(other, folder)
    assert torch.equal(other.lora, eng.lora)
    with pytest.raises(NotImplementedError, match="pre-activation"):
        load_lora(CfgNode(dict(r=2, lora_alpha=4, target_modules=list(targets), allow_out=True)), sd, heads=heads, device=DEV)


# ------------------------------------------------------------------------------------------------ 7. flag off, or on with the module not targeted
def test_flag_without_the_module_is_the_engine_it_was():
    """allow_swiglu_out with weights_out not among the targets: arena, key map, gradients, the no-grad pass and the workspace size of the engine without the flag, bit
    for bit -- the flags word both engines pass is 0."""
    sd, heads, L, image, B = checkpoint()
    img, dkey = (t.to(DEV) for t in case_inputs(B, 128, image))
    targets = ["query", "value", "weights_in", "dense"]
    lora = RS.lora_for(sd, targets)
    out = []
    for kw in (dict(allow_out=True), ALL):
        eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=targets, allow_swiglu=True,
                            lora_dropout=0.05, seed=5, **kw)
        eng.load_lora_state_dict(lora)
        assert eng.out_targets == (True, False) and eng._out_flags == 0
        key = eng.forward_train(img).clone()
        out.append((eng.lora.clone(), key, eng.backward(dkey).clone(), eng.forward_nograd(img).clone(), sum(w.numel() for w in eng._tside_ws if w is not None)))
    for a, b in zip(*out):
        assert a == b if isinstance(a, int) else torch.equal(a, b)
    # everything off: the engine of old, whatever the new keyword's default
    plain = [ViTLoRAEngine(sd, heads=heads, device=DEV, generator=torch.Generator().manual_seed(3), allow_swiglu=True, **kw) for kw in ({}, {"allow_swiglu_out": False})]
    assert torch.equal(plain[0].lora, plain[1].lora) and torch.equal(plain[0].forward_train(img), plain[1].forward_train(img))
    assert torch.equal(plain[0].backward(dkey), plain[1].backward(dkey))


def test_the_driver_refuses_without_its_flag():
    """The _lora_out entry points (flags 0) keep refusing the fc2 slot on the SwiGLU MLP, and the _ex forms an unknown bit -- before any launch: the key map and
    the gradients' buffer stay as they were."""
    sd, heads, L, image, B = checkpoint()
    eng = swiglu_engine(sd, heads, ("weights_out",), RS.lora_for(sd, ("weights_out",)))
    eng.train_streams = 1
    x = case_inputs(B, 128, image)[0].to(DEV)
    good = eng.forward_train(x).clone()
    torch.cuda.synchronize()
    lib, gh = eng.lib, image // 14
    t = eng._train_desc(B, image, image, eng._chunk_seed[0])
    grad = torch.full_like(eng.lora_grad, 3.0)
    T, TT, TM, keep = eng._tables(gh, gh, grad)
    TO = eng._out_table(grad)
    ws = eng._tside_ws[0]
    key, dkey = torch.full_like(good, 3.0), torch.ones_like(good)
    P, st, FL = N.ptr, N.stream(), N.LORA_OUT_SWIGLU
    assert TM is None and lib.ucod_vit_train_workspace_bytes_lora_out_ex(C.byref(t), eng.mlp, FL, None, TO) == ws.numel()
    assert lib.ucod_vit_forward_train_lora_out(C.byref(t), eng.mlp, T, TT, None, TO, P(x), P(key), P(ws), ws.numel(), st) == -1
    assert lib.ucod_vit_backward_lora_out(C.byref(t), eng.mlp, T, TT, None, TO, P(dkey), P(ws), ws.numel(), st) == -1
    assert lib.ucod_vit_forward_lora_infer_lora_out(C.byref(t), eng.mlp, T, TT, None, TO, P(x), P(key), P(ws), ws.numel(), st) == -1
    for flags in (0, 2, FL | 4):
        assert lib.ucod_vit_forward_train_lora_out_ex(C.byref(t), eng.mlp, flags, T, TT, None, TO, P(x), P(key), P(ws), ws.numel(), st) == -1, flags
        assert lib.ucod_vit_backward_lora_out_ex(C.byref(t), eng.mlp, flags, T, TT, None, TO, P(dkey), P(ws), ws.numel(), st) == -1, flags
        assert lib.ucod_vit_forward_lora_infer_lora_out_ex(C.byref(t), eng.mlp, flags, T, TT, None, TO, P(x), P(key), P(ws), ws.numel(), st) == -1, flags
    torch.cuda.synchronize()
    assert bool((key == 3.0).all()) and bool((grad == 3.0).all()), "a refused call wrote to its outputs"
    assert lib.ucod_vit_forward_train_lora_out_ex(C.byref(t), eng.mlp, FL, T, TT, None, TO, P(x), P(key), P(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(key, good)
