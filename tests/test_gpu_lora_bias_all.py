"""GPU: what LoRA ``bias="all"`` (models/modules/full_model.py:53,66 hands ``bias`` to peft) needs from the library -- the gradients of the LayerNorm betas and of the
patch embedding's bias in the backbone backward -- every call through the C ABI.

1-2  ucod_colsum_det_lora alone: exact inputs against f64 bit for bit at dropout 0 and 0.5 (1 / (1 - p) = 2 exactly), with the mask of oracle.vit.lora_dropout_mask
     under the driver's keys, canaries around output and workspace, large values beyond the read columns of t and behind the A rows, run twice; the same cases on
     N(0, 1) data under the bar of tests/test_gpu_lora_bias.py::test_colsum_random, 2e-4 max(1, |ref|max);
3    without a branch it is ucod_colsum_det bit for bit; refusals leave the output untouched;
4    ucod_colsum_det_tok: exact, random, first = 0 against ucod_colsum_det bit for bit, refusals;
5    ucod_vit_backward_lora_bias_ex against f64 autograd (tests/lora_bias_all_ref.py): the norm table's gradients on five models of tests/test_gpu_lora_bias.py and
     the gated DINOv3 model of G26 (gate_proj / up_proj: the pair form), dropout 0 and 0.05, under the bars of that file (4e-2; 5e-2 with dropout or at D = 256) on
     each layer's vector of betas and on the patch bias; the last layer's beta2 exact zeros, its beta1 and the patch bias not; every gradient in front of the new slots
     bit for bit what the engine's own backward returns; a second pass bit-identical;
6    the new tier with a NULL norm table is the _lora_bias tier: the same bytes, the same gradients from the same saved workspace;
7    ViTLoRAEngine(..., bias="all", allow_bias_all=True): whole passes against f64 autograd with every trained bias as a leaf, seven model / target sets (the key
     alone: five modules' biases trained without an adapter), dropout 0 / 0.05, one / two streams, the same bars; key map and LoRA gradients bit for bit those of
     bias="none"; frozen slots exact zeros; the names are peft's rule on the checkpoint minus the final LayerNorm;
8    the opt-in with "none" / "lora_only": arena, key map, gradients, no-grad pass, workspace and names of today's engine, bit for bit;
9    merges of perturbed betas, patch bias and Linear biases: merged_state_dict() on the f32-equivalent engine against the f64 forward (3e-6) and the distance with
     either group left unmerged; merge_into on the folded D = 256 engine against a rebuilt one; the adapter folder; the EMA clone's buffer;
10   three runner steps: every live bias moves, frozen slots and the final LayerNorm keep their bits, two runs identical;
11   the engine against G27: transformers' own f64 gradients of its ``named_parameters()`` with "bias" in the name, the same bars and measure.

No bar is taken from a run of this code.  Measured on MI355X: profiles/lora_bias_all_tests.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTLoRAEngine  # noqa: E402
from oracle import vit as OV  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402
import dinov3_lora_mlp_in_ref as RM  # noqa: E402
import registers_ref as RR  # noqa: E402
import lora_out_ref as RO  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402
import lora_bias_ref as RB  # noqa: E402
import lora_bias_all_ref as RA  # noqa: E402

DEV = "cuda"
HALF, F32 = N.ROPE_ELEM_HALF, N.ROPE_ELEM_F32
LNB_DY_BF16 = 1                      # include/ucod_dpl.h: UCOD_LNB_DY_BF16
CANARY, PAD = 1234.0, 4096
LEAK = 30000.0                       # what the columns and rows hold that must not be read
SEED, LAYERS, LAYER = 0x1234_5678_9ABC, 3, 1      # the dropout descriptor of the kernel tests: layer 1 of 3


class Flat:
    """n f32 elements (NaN: an element no store reached shows) between two canary runs"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
        self.payload = self.buf[PAD:PAD + n]
        self.payload.fill_(float("nan"))

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())


def twice(n, wsb, launch):
    """run ``launch(out pointer, workspace pointer)`` twice on fresh guarded buffers: 0 returned, guards intact, everything written, identical bits"""
    outs = []
    for _ in range(2):
        out, ws = Flat(n), Flat(wsb // 4)
        assert launch(out.ptr(), ws.ptr()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact() and ws.guards_intact(), "wrote outside its output or workspace"
        assert bool(torch.isfinite(out.payload).all()) and bool(torch.isfinite(ws.payload).all()), "left elements unwritten"
        outs.append(out.payload.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    return outs[0].cpu()


# ------------------------------------------------------------------------------------------------ 1-2. ucod_colsum_det_lora
# (M, D, np, r, dy is f32): one row; rows that are no multiple of the 16 row threads or of a slab; 43 slabs and the generic rank loop; the widest rows with one
# module at the generic loop; f32 dy with the pair
LCASES = [(1, 128, 3, 2, False), (111, 384, 3, 2, False), (2740, 768, 3, 8, False), (111, 1536, 1, 8, False), (2740, 256, 2, 2, True)]


def lora_operands(M, D, np_, r, t, a):
    """The device buffers as the driver lays them out, LEAK wherever the kernel must not read: t [np][M, r] -> bf16 rows of pitch ldt (q / k / v: the aug columns of a
    [M, 3 D + 64] dqkv_aug; else a [M, 64] scratch); a [np][r, D] -> f32 (q / k / v: [A | B] per module, stride 2 r D; else the A blocks side by side)."""
    if np_ == 3:
        ldt, first = 3 * D + 64, 3 * D
    else:
        ldt, first = 64, 0
    tb = torch.full((M, ldt), LEAK, dtype=torch.bfloat16)
    for p in range(np_):
        tb[:, first + p * r:first + (p + 1) * r] = t[p].to(torch.bfloat16)
    astride = (2 if np_ == 3 else 1) * r * D
    ab = torch.full((np_ * astride + r * D,), LEAK, dtype=torch.float32)
    for p in range(np_):
        ab[p * astride:p * astride + r * D] = a[p].float().reshape(-1)
    return tb.to(DEV), first, ldt, ab.to(DEV)


def run_colsum_lora(dy, f32, M, D, np_, r, t, a, p_drop, key):
    lib = N.load()
    wsb = lib.ucod_colsum_det_lora_workspace_bytes(M, D)
    assert wsb == min(128, -(-M // 64)) * D * 4
    tb, first, ldt, ab = lora_operands(M, D, np_, r, t, a)
    drop = N.LoraDropout(p_drop, SEED, key)
    dyd = dy.to(DEV)
    tptr = tb.data_ptr() + 2 * first
    return twice(D, wsb, lambda o, w: lib.ucod_colsum_det_lora(N.ptr(dyd), 0 if f32 else LNB_DY_BF16, M, D, tptr, ldt, N.ptr(ab), np_, r, C.byref(drop), o, w, wsb,
                                                                N.stream()))


def driver_key(np_):
    """the driver's dropout key: the layer for q / k / v (kind 0), L + l for the MLP input modules (kind 1)"""
    return LAYER if np_ == 3 else LAYERS + LAYER


def masks_of(np_, M, D, p_drop):
    return [OV.lora_dropout_mask(SEED, driver_key(np_), p, M, D, p_drop) for p in range(np_)]


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("M,D,np_,r,f32", LCASES)
def test_colsum_lora_exact(M, D, np_, r, f32, p_drop):
    """dy: integers in [-8, 8], t and A: integers in [-4, 4], dy and A times one power of two per column, the mask scale 1 or 2: every product, every branch sum and
    every partial sum in any order is an integer below 2^24 times that power (asserted), so the result must be the f64 value bit for bit whatever the order of the
    additions and wherever the compiler contracts."""
    g = torch.Generator().manual_seed(M + D + np_ + r)
    assert M * (8 + np_ * r * 16 * 2) < 2 ** 24
    col = torch.exp2(torch.randint(-6, 7, (D,), generator=g).double())
    dy = torch.randint(-8, 9, (M, D), generator=g).double() * col
    t = [torch.randint(-4, 5, (M, r), generator=g).double() for _ in range(np_)]
    a = [torch.randint(-4, 5, (r, D), generator=g).double() * col for _ in range(np_)]
    dtype = torch.float32 if f32 else torch.bfloat16
    assert torch.equal(dy.to(dtype).double(), dy) and all(torch.equal(x.to(torch.bfloat16).double(), x) for x in t) and all(torch.equal(x.float().double(), x) for x in a)
    masks = masks_of(np_, M, D, p_drop)
    assert all(set(mk.unique().tolist()) <= ({0.0, 2.0} if p_drop else {1.0}) for mk in masks)
    if p_drop and M > 1:
        assert all(0.3 < float((mk == 0).double().mean()) < 0.7 for mk in masks) and (np_ == 1 or not torch.equal(masks[0], masks[-1]))
    ref = RA.colsum_lora(dy, t, a, masks)
    assert torch.equal(ref.float().double(), ref)
    got = run_colsum_lora(dy.to(dtype), f32, M, D, np_, r, t, a, p_drop, driver_key(np_))
    assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {D} columns differ, worst {float((got.double() - ref).abs().max()):.3e}"
    assert float(ref.abs().max()) > 0 and not torch.equal(ref, dy.sum(0))          # (the branch is in the sum)


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("M,D,np_,r,f32", LCASES)
def test_colsum_lora_random(M, D, np_, r, f32, p_drop):
    """N(0, 1) rounded to the element types: |got - ref| <= 2e-4 max(1, |ref|max), the bar of tests/test_gpu_lora_bias.py::test_colsum_random."""
    g = torch.Generator().manual_seed(M + D + np_ + r + 1)
    dtype = torch.float32 if f32 else torch.bfloat16
    dy = torch.randn(M, D, generator=g).to(dtype)
    t = [torch.randn(M, r, generator=g).to(torch.bfloat16) for _ in range(np_)]
    a = [torch.randn(r, D, generator=g) for _ in range(np_)]
    ref = RA.colsum_lora(dy, t, a, masks_of(np_, M, D, p_drop))
    got = run_colsum_lora(dy, f32, M, D, np_, r, t, a, p_drop, driver_key(np_))
    err = maxdiff(got, ref) / max(1.0, ref.abs().max().item())
    print(f"colsum_lora {(M, D, np_, r)} {'f32' if f32 else 'bf16'} p={p_drop}: {err:.2e} (bar 2e-4)")
    assert err <= 2e-4, err


# ------------------------------------------------------------------------------------------------ 3. no branch; refusals
@pytest.mark.parametrize("M,D,f32", [(1, 128, False), (2740, 768, False), (111, 1536, False), (2740, 256, True)])
def test_colsum_lora_without_a_branch_is_colsum_det(M, D, f32):
    lib = N.load()
    g = torch.Generator().manual_seed(M + D)
    dy = torch.randn(M, D, generator=g).to(torch.float32 if f32 else torch.bfloat16).to(DEV)
    wsb = lib.ucod_colsum_det_lora_workspace_bytes(M, D)
    assert wsb == lib.ucod_colsum_det_workspace_bytes(M, D)
    a = twice(D, wsb, lambda o, w: lib.ucod_colsum_det_lora(N.ptr(dy), 0 if f32 else LNB_DY_BF16, M, D, None, 0, None, 0, 0, None, o, w, wsb, N.stream()))
    b = twice(D, wsb, lambda o, w: lib.ucod_colsum_det(N.ptr(dy), F32 if f32 else HALF, M, D, D, None, o, w, wsb, N.stream()))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_colsum_lora_refusals_leave_outputs_untouched():
    M, D, np_, r = 111, 384, 3, 2
    lib = N.load()
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(M, D, generator=g).bfloat16()
    t = [torch.randn(M, r, generator=g).bfloat16() for _ in range(np_)]
    a = [torch.randn(r, D, generator=g) for _ in range(np_)]
    tb, first, ldt, ab = lora_operands(M, D, np_, r, t, a)
    dyd = dy.to(DEV)
    wsb = lib.ucod_colsum_det_lora_workspace_bytes(M, D)
    out, ws = torch.full((D,), 3.0, device=DEV), torch.full((wsb // 4,), 3.0, device=DEV)
    drop, bad_lo, bad_hi = N.LoraDropout(0.05, SEED, LAYER), N.LoraDropout(-0.1, SEED, LAYER), N.LoraDropout(1.0, SEED, LAYER)
    ok = dict(dy=N.ptr(dyd), flags=LNB_DY_BF16, M=M, D=D, t=tb.data_ptr() + 2 * first, ldt=ldt, a=N.ptr(ab), np=np_, r=r, drop=C.byref(drop), out=N.ptr(out), ws=N.ptr(ws),
              wb=wsb)
    call = lambda **kw: lib.ucod_colsum_det_lora(*[{**ok, **kw}[k] for k in ("dy", "flags", "M", "D", "t", "ldt", "a", "np", "r", "drop", "out", "ws", "wb")], N.stream())  # noqa: E731
    bad = {"null dy": dict(dy=None), "null out": dict(out=None), "null workspace": dict(ws=None), "null lora": dict(a=None), "M < 1": dict(M=0), "D % 128": dict(D=320),
           "np = 0": dict(np=0), "np = 4": dict(np=4), "r = 0": dict(r=0), "r = 22 for np = 3": dict(r=22), "r = 9 for np = 1": dict(np=1, r=9),
           "r = 9 for np = 2": dict(np=2, r=9), "ldt < np r": dict(ldt=5), "p < 0": dict(drop=C.byref(bad_lo)), "p = 1": dict(drop=C.byref(bad_hi)),
           "small workspace": dict(wb=wsb - 4), "unknown flag": dict(flags=4), "misaligned dy": dict(dy=N.ptr(dyd) + 2)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    for M0, D0 in ((0, D), (M, 320), (M, 0), (M, 64)):
        assert lib.ucod_colsum_det_lora_workspace_bytes(M0, D0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((ws == 3.0).all()), "a refused call wrote to its outputs"
    assert call() == 0                                              # ... and the same arguments without a fault run
    torch.cuda.synchronize()
    ref = RA.colsum_lora(dy, t, a, masks_of(np_, M, D, 0.05))
    assert maxdiff(out.cpu(), ref) <= 2e-4 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 4. ucod_colsum_det_tok
# (B, tok, first, N, ld, elem, scaled): one image of 25 patches; three images with four registers; ViT-B/14 at 518 (f32: the residual cotangent the driver sums);
# ViT-S/16 with registers (16-bit, a pitch beyond N)
TCASES = [(1, 26, 1, 128, 128, F32, False), (1, 26, 1, 128, 192, HALF, True), (3, 30, 5, 128, 128, F32, True), (3, 30, 5, 128, 128, HALF, False),
          (2, 1370, 1, 768, 768, F32, False), (2, 1029, 5, 384, 448, HALF, False)]


def run_colsum_tok(x, elem, B, tok, first, n, ld, scale):
    lib = N.load()
    wsb = lib.ucod_colsum_det_tok_workspace_bytes(B, tok, first, n)
    assert wsb == min(128, -(-B * (tok - first) // 64)) * n * 4
    return twice(n, wsb, lambda o, w: lib.ucod_colsum_det_tok(N.ptr(x), elem, B, tok, first, n, ld, None if scale is None else N.ptr(scale), o, w, wsb, N.stream()))


@pytest.mark.parametrize("B,tok,first,n,ld,elem,scaled", TCASES)
def test_colsum_tok_exact(B, tok, first, n, ld, elem, scaled):
    """Integers in [-8, 8] times a power of two per column, as tests/test_gpu_lora_bias.py::test_colsum_exact; the rows that must not be summed hold integers too
    (16 times larger), so that a sum which takes them is wrong by far more than a rounding."""
    g = torch.Generator().manual_seed(B + tok + n)
    M = B * tok
    assert 8 * M < 2 ** 24
    x = torch.randint(-8, 9, (B, tok, n), generator=g).double()
    x[:, :first] *= 16
    x = (x * torch.exp2(torch.randint(-6, 7, (n,), generator=g).double())).reshape(M, n)
    scale = torch.exp2(torch.randint(-3, 4, (n,), generator=g).double()) if scaled else None
    dtype = torch.float32 if elem == F32 else torch.bfloat16
    buf = torch.full((M, ld), LEAK, dtype=dtype)
    buf[:, :n] = x.to(dtype)
    assert torch.equal(buf[:, :n].double(), x)
    ref = RA.colsum_tok(x, B, tok, first, scale)
    assert torch.equal(ref.float().double(), ref) and not torch.equal(ref, RA.colsum_tok(x, B, tok, 0, scale))
    got = run_colsum_tok(buf.to(DEV), elem, B, tok, first, n, ld, None if scale is None else scale.float().to(DEV))
    assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {n} columns differ, worst {float((got.double() - ref).abs().max()):.3e}"


@pytest.mark.parametrize("B,tok,first,n,ld,elem,scaled", TCASES)
def test_colsum_tok_random_and_first_0(B, tok, first, n, ld, elem, scaled):
    """N(0, 1) rounded to the element type under 2e-4 max(1, |ref|max); with first = 0 the bits of ucod_colsum_det at M = B tok."""
    lib = N.load()
    g = torch.Generator().manual_seed(B + tok + n + 1)
    M = B * tok
    dtype = torch.float32 if elem == F32 else torch.bfloat16
    buf = torch.full((M, ld), LEAK, dtype=dtype)
    buf[:, :n] = torch.randn(M, n, generator=g).to(dtype)
    scale = (torch.rand(n, generator=g) + 0.5) if scaled else None
    ref = RA.colsum_tok(buf[:, :n], B, tok, first, scale)
    bufd, scaled_d = buf.to(DEV), None if scale is None else scale.to(DEV)
    got = run_colsum_tok(bufd, elem, B, tok, first, n, ld, scaled_d)
    err = maxdiff(got, ref) / max(1.0, ref.abs().max().item())
    print(f"colsum_tok {(B, tok, first, n, ld)} {'f32' if elem == F32 else 'bf16'} scaled={scaled}: {err:.2e} (bar 2e-4)")
    assert err <= 2e-4, err
    all_rows = run_colsum_tok(bufd, elem, B, tok, 0, n, ld, scaled_d)
    wsb = lib.ucod_colsum_det_workspace_bytes(M, n)
    plain = twice(n, wsb, lambda o, w: lib.ucod_colsum_det(N.ptr(bufd), elem, M, n, ld, None if scale is None else N.ptr(scaled_d), o, w, wsb, N.stream()))
    assert torch.equal(all_rows.view(torch.int32), plain.view(torch.int32))


def test_colsum_tok_refusals_leave_outputs_untouched():
    B, tok, first, n, ld = 3, 30, 5, 384, 448
    lib = N.load()
    x = torch.randn(B * tok, ld, device=DEV).bfloat16()
    wsb = lib.ucod_colsum_det_tok_workspace_bytes(B, tok, first, n)
    out, ws = torch.full((n,), 3.0, device=DEV), torch.full((wsb // 4,), 3.0, device=DEV)
    ok = dict(x=N.ptr(x), elem=HALF, B=B, tok=tok, first=first, n=n, ld=ld, scale=None, out=N.ptr(out), ws=N.ptr(ws), wb=wsb)
    call = lambda **kw: lib.ucod_colsum_det_tok(*[{**ok, **kw}[k] for k in ("x", "elem", "B", "tok", "first", "n", "ld", "scale", "out", "ws", "wb")], N.stream())  # noqa: E731
    bad = {"null x": dict(x=None), "null out": dict(out=None), "null workspace": dict(ws=None), "B < 1": dict(B=0), "N % 8": dict(n=380), "ld < N": dict(ld=376),
           "misaligned ld": dict(ld=452), "small workspace": dict(wb=wsb - 4), "unknown elem": dict(elem=2), "first < 0": dict(first=-1), "first = tok": dict(first=tok),
           "first > tok": dict(first=tok + 1)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    for args in ((0, tok, first, n), (B, tok, -1, n), (B, tok, tok, n), (B, tok, first, 380)):
        assert lib.ucod_colsum_det_tok_workspace_bytes(*args) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((ws == 3.0).all()), "a refused call wrote to its outputs"
    assert call() == 0
    torch.cuda.synchronize()
    ref = RA.colsum_tok(x[:, :n].cpu(), B, tok, first)
    assert maxdiff(out.cpu(), ref) <= 2e-4 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 5. the backward's new tier vs f64 autograd
@functools.lru_cache(maxsize=None)
def model(tag):
    """One model: state dict, geometry, inputs, engine arguments, the targeted modules (every module that is built for it, the MLP input included where there is
    one), as tests/test_gpu_lora_bias.py builds the first five and tests/test_gpu_dinov3_lora_mlp_in.py the gated one."""
    m = dict(tag=tag, eps=1e-6, scale=2.0, r=2, alpha=4, kw={}, family="dinov2", D=128, gated=False, bias="lora_only")
    if tag == "g8":
        sd = sub(load_golden("g8_dinov2_native"), "sd.")
        m.update(sd=sd, heads=2, L=3, inputs=RO.case_inputs(2, 128, 70), kw=dict(allow_out=True), targets=("query", "key", "value", "fc1", "dense", "fc2"))
    elif tag == "g8key":                                              # the key alone: no MLP table, LayerNorm 2's beta from the plain sum
        m.update(model("g8"), tag=tag, targets=("key",))
    elif tag == "d256":
        sd, heads, L, image, B = RO.d256_state_dict()
        m.update(sd=sd, heads=heads, L=L, D=256, inputs=RO.case_inputs(B, 256, image), kw=dict(allow_out=True), targets=("query", "key", "value", "fc1", "dense", "fc2"))
    elif tag == "swiglu":
        sd = RS.g24_state_dict("dinov2")
        m.update(sd=sd, heads=2, L=3, inputs=RO.case_inputs(2, 128, 70), kw=dict(allow_swiglu=True, allow_out=True, allow_swiglu_out=True),
                 targets=("query", "key", "value", "weights_in", "dense", "weights_out"))
    elif tag == "reg":
        sd = RR.g21_state_dict("native")
        gen = torch.Generator().manual_seed(7)
        m.update(sd=sd, heads=2, L=3, inputs=(torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen)), kw=dict(allow_out=True),
                 targets=("query", "key", "value", "fc1", "dense", "fc2"))
    elif tag == "g46":
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g23_dinov3_lora_g46.npz"))
        sd = R3.g22_state_dict("g46")
        m.update(sd=sd, heads=R3.G22["g46"]["heads"], L=R3.G22_LAYERS, eps=1e-5, scale=RL.G23_SCALE, r=RL.G23_R, alpha=RL.G23_ALPHA, family="dinov3", z=z,
                 inputs=(torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])), kw=dict(allow_rope=True, allow_out=True),
                 targets=("q_proj", "k_proj", "v_proj", "o_proj", "down_proj"))
    else:
        assert tag == "gated"
        g = R3.G22["gated"]
        m.update(sd=R3.g22_state_dict("gated"), heads=g["heads"], L=R3.G22_LAYERS, D=g["D"], eps=1e-5, scale=RM.G26_SCALE, r=RM.G26_R, alpha=RM.G26_ALPHA, family="dinov3",
                 inputs=RM.g26_inputs("gated"), kw=dict(allow_rope=True, allow_swiglu=True, allow_mlp_in=True), targets=tuple(RM.g26_targets("gated", "both")), gated=True,
                 bias="none")
    m["tok"], m["lead"] = RB.geometry(m["inputs"][0], m["sd"])
    return m


def lora_of(m):
    sd, targets = m["sd"], m["targets"]
    if m["gated"]:
        return RM.g26_lora("gated", targets)
    if m["tag"] == "swiglu":
        return RS.lora_for(sd, targets)
    if m["tag"] == "g46":
        z = m["z"]
        qkv = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/") and any(f".{t}." in k for t in targets)}
        return {**qkv, **RO.lora_for(sd, tuple(t for t in targets if t in RO.OUT_NAMES), seed=5)}
    return RO.lora_for(sd, targets)


def masks_for(m, seed, images, p_drop):
    """the masks of one chunk under the driver's keys (kind * L + l), or None with dropout off"""
    if p_drop == 0:
        return None
    L, tok, D, sd, targets = m["L"], m["tok"], m["D"], m["sd"], m["targets"]
    rows = images * tok
    if m["gated"]:
        return RM.g26_masks("gated", targets, rows, seed, p_drop)
    lay = RB.layer_path(sd)
    qkv = RL.QKV if m["family"] == "dinov3" else ("query", "key", "value")
    mk = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(qkv) if nm in targets}
    for nm in ("fc1", "weights_in"):
        if nm in targets:
            mk.update({(i, nm): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
    if m["tag"] == "swiglu":
        out = RS.out_masks(seed, L, rows, D, 344, p_drop)
    else:
        F = sd[lay + "0." + ("mlp.up_proj" if m["family"] == "dinov3" else "mlp.fc1") + ".weight"].shape[0]
        out = RO.out_masks(seed, L, rows, D, F, p_drop, RO.OUT_LEAVES[m["family"]])
    mk.update({k: v for k, v in out.items() if k[1] in targets})
    return mk


def engine_of(m, lora, p_drop):
    eng = ViTLoRAEngine(m["sd"], heads=m["heads"], r=m["r"], lora_alpha=m["alpha"], eps=m["eps"], device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=list(m["targets"]), bias=m["bias"], lora_dropout=p_drop, seed=1234, **m["kw"])
    eng.load_lora_state_dict({**{k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}, **lora})
    eng.train_streams = 1
    return eng


def norm_table(L, D, trained=None):
    """(the table, its [1 + 2 L, D] buffer filled with 7): slot s NULL unless ``trained`` is None or holds s"""
    buf = torch.full((1 + 2 * L, D), 7.0, device=DEV)
    ptrs = [buf[s].data_ptr() if trained is None or s in trained else None for s in range(1 + 2 * L)]
    return (C.c_void_p * len(ptrs))(*ptrs), buf


def run_tier(eng, m, x, dkey, seed, TN, with_bias_table=True):
    """One training forward and one backward of the _lora_bias_ex tier on a workspace of its own; (the gradient arena it filled, workspace bytes)"""
    lib, P, st, B = eng.lib, N.ptr, N.stream(), x.shape[0]
    H, W = x.shape[2:]
    t = eng._train_desc(B, H, W, seed)
    g = torch.full_like(eng.lora_grad, 7.0)
    T, TT, TM, keep = eng._tables(H // eng.P, W // eng.P, g)
    TO, TB = eng._out_table(g), (eng._bias_table(g) if with_bias_table else None)
    lead = (C.byref(t), eng.mlp, eng._out_flags)
    n = lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, TM, TO, TB, TN)
    ws, k = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.empty(B, eng.D, H // eng.P, W // eng.P, device=DEV)
    assert lib.ucod_vit_forward_train_lora_out_ex(*lead, T, TT, TM, TO, P(x), P(k), P(ws), n, st) == 0
    assert lib.ucod_vit_backward_lora_bias_ex(*lead, T, TT, TM, TO, TB, TN, P(dkey), P(ws), n, st) == 0
    torch.cuda.synchronize()
    return g, n


@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tag", ["g8", "g8key", "d256", "swiglu", "reg", "g46", "gated"])
def test_norm_table_vs_f64_autograd(tag, p_drop):
    m = model(tag)
    sd, L, D, lay = m["sd"], m["L"], m["D"], RB.layer_path(m["sd"])
    lora = lora_of(m)
    x, dkey = (t.to(DEV) for t in m["inputs"])
    eng = engine_of(m, lora, p_drop)
    eng.forward_train(x)
    seed = eng._chunk_seed[0]
    own = eng.backward(dkey).clone()                               # the engine's own backward: the _lora_bias (or _lora_out_ex) tier
    eng.check_overflow(wait=True)
    TN, buf = norm_table(L, D)
    g, n = run_tier(eng, m, x, dkey, seed, TN)
    assert torch.equal(g, own), "a gradient in front of the new slots differs from the pass without the norm table"
    if eng._bias_table(eng.lora_grad) is not None:                 # the partials share the bias table's entry: no byte is added
        assert n == eng._tside_ws[0].numel()
    else:
        assert n > eng._tside_ws[0].numel()
    ref = RA.norm_grads(m["inputs"][0], {**sd, **lora}, m["heads"], m["inputs"][1], m["scale"], masks=masks_for(m, seed, x.shape[0], p_drop), gated=m["gated"], device=DEV)
    names = RA.norm_names(sd)
    got = {k: buf[s].cpu() for s, k in enumerate(names)}
    ref = {k: v.cpu() for k, v in ref.items()}
    bar = RB.BAR_LOOSE if (p_drop > 0 or D == 256) else RB.BAR
    patch = names[0]
    errs = RB.errors(got, {k: v for k, v in ref.items() if k != patch}, sd)
    errs[patch] = float((got[patch].double() - ref[patch]).norm() / ref[patch].norm())
    layers = {k: e for k, e in errs.items() if k.startswith("layer")}
    print(f"lora_bias_all {tag} {m['targets']} p={p_drop}: patch bias {errs[patch]:.3e}; worst layer vector of betas {max(layers.values()):.3e} "
          f"({max(layers, key=layers.get)}); worst tensor {max(errs.values()):.3e} ({max(errs, key=errs.get)}) (bar {bar:.0e})")
    assert len(layers) == L
    for k, e in errs.items():
        assert e < bar, (k, e, bar)
    for k in names:                                               # no trained vector with a non-zero f64 gradient falls outside both measures
        assert float(ref[k].abs().max()) == 0.0 or k in errs or any(k.startswith(f"{lay}{i}.") for i in range(L)), k
    last2 = f"{lay}{L - 1}.norm2.bias"
    assert float(ref[last2].abs().max()) == 0.0 and float(got[last2].abs().max()) == 0.0
    assert float(got[f"{lay}{L - 1}.norm1.bias"].abs().max()) > 0 and float(got[patch].abs().max()) > 0
    if p_drop == 0:                                                # a second pass: bit-identical
        TN2, buf2 = norm_table(L, D)
        g2, _ = run_tier(eng, m, x, dkey, seed, TN2)
        assert torch.equal(g2, g) and torch.equal(buf2, buf)


# ------------------------------------------------------------------------------------------------ 6. a NULL norm table is the _lora_bias tier
def test_the_new_tier_with_a_null_table_is_lora_bias():
    m = model("g8")
    lora = lora_of(m)
    eng = engine_of(m, lora, 0.05)
    x, dkey = (t.to(DEV) for t in m["inputs"])
    eng.forward_train(x)
    seed = eng._chunk_seed[0]
    own = eng.backward(dkey).clone()
    torch.cuda.synchronize()
    lib, t = eng.lib, eng._train_desc(x.shape[0], 70, 70, seed)
    g0 = torch.full_like(eng.lora_grad, 7.0)
    T, TT, TM, keep = eng._tables(5, 5, g0)
    TO, TB = eng._out_table(g0), eng._bias_table(g0)
    lead = (C.byref(t), eng.mlp, eng._out_flags)
    n_tb = lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, TM, TO, TB)
    n_ex = lib.ucod_vit_train_workspace_bytes_lora_out_ex(*lead, TM, TO)
    assert lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, TM, TO, TB, None) == n_tb == eng._tside_ws[0].numel()
    assert lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, TM, TO, None, None) == n_ex < n_tb
    g_null, n = run_tier(eng, m, x, dkey, seed, None)
    assert n == n_tb and torch.equal(g_null, own)
    # with only some slots set the others are not written, and the set ones are what the full table gives
    TN_all, full = norm_table(m["L"], m["D"])
    run_tier(eng, m, x, dkey, seed, TN_all)
    TN_some, some = norm_table(m["L"], m["D"], trained={1, 4})
    g_some, _ = run_tier(eng, m, x, dkey, seed, TN_some)
    assert torch.equal(g_some, own)
    for s in range(1 + 2 * m["L"]):
        assert torch.equal(some[s], full[s]) if s in (1, 4) else bool((some[s] == 7.0).all()), s
    # without the bias table the norm table brings its own partials; a workspace without them is refused
    TN, buf = norm_table(m["L"], m["D"])
    g_nb, n_nb = run_tier(eng, m, x, dkey, seed, TN, with_bias_table=False)
    assert n_ex < n_nb <= n_tb and torch.equal(buf, full)
    base = eng.lora.shape[1] - eng.bias_numel
    assert torch.equal(g_nb[:, :base], own[:, :base]) and bool((g_nb[:, base:] == 7.0).all())
    assert lib.ucod_vit_backward_lora_bias_ex(*lead, T, TT, TM, TO, None, TN, N.ptr(dkey), N.ptr(eng._tside_ws[0]), n_ex, N.stream()) == -2


# ================================================================================================ the engine: ViTLoRAEngine(..., bias="all", allow_bias_all=True)
def all_engine(m, lora, p_drop, bias="all", biases=None, **kw):
    eng = ViTLoRAEngine(m["sd"], heads=m["heads"], r=m["r"], lora_alpha=m["alpha"], eps=m["eps"], device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=list(m["targets"]), bias=bias, allow_bias_all=True, lora_dropout=p_drop, seed=1234, **m["kw"], **kw)
    have = {k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}
    if bias == "all":                                              # the names are peft's rule on the checkpoint, minus the final LayerNorm; the values the checkpoint's
        assert sorted(have) == RA.trained_names(m["sd"])
        for k, v in have.items():
            assert torch.equal(v.cpu(), m["sd"][k].float()), k
    eng.load_lora_state_dict({**have, **lora, **(biases or {})})
    return eng


# ------------------------------------------------------------------------------------------------ 7. whole passes through the engine
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tag", ["g8", "g8key", "d256", "swiglu", "reg", "g46", "gated"])
def test_engine_passes_vs_f64_autograd(tag, p_drop, streams):
    """Every trained bias against f64 autograd under the bars of tests/test_gpu_lora_bias.py (4e-2; 5e-2 with dropout or at D = 256): each layer's vector of Linear
    biases and betas, every tensor with at least 1e-3 of it, and the patch bias.  The key map and the LoRA gradients are those of the engine with bias="none" bit
    for bit (the same launches on the same data: their own files hold them to their bars).  g8key: the key alone is targeted, five modules' biases are trained
    without an adapter."""
    m = model(tag)
    sd, L, D, lay = m["sd"], m["L"], m["D"], RB.layer_path(m["sd"])
    lora = lora_of(m)
    x, dkey = (t.to(DEV) for t in m["inputs"])
    eng = all_engine(m, lora, p_drop)
    eng.train_streams = streams
    key = eng.forward_train(x).clone()
    eng.backward(dkey)
    eng.check_overflow(wait=True)
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    plain = all_engine(m, lora, p_drop, bias="none")
    plain.train_streams = streams
    assert torch.equal(plain.forward_train(x), key)
    plain.backward(dkey)
    for k, v in plain.lora_state_dict(grads=True).items():
        assert torch.equal(v.cpu(), got[k]), k
    ref = None
    for (b0, b1), seed in zip(eng._bounds, eng._chunk_seed):        # (each chunk has its own masks; gradients add)
        _, g = RA.all_grads(m["inputs"][0][b0:b1], {**sd, **lora}, m["heads"], m["inputs"][1][b0:b1], m["scale"], masks=masks_for(m, seed, b1 - b0, p_drop),
                            gated=m["gated"], device=DEV)
        ref = {k: v.cpu() for k, v in g.items()} if ref is None else {k: ref[k] + v.cpu() for k, v in g.items()}
    names = RA.trained_names(sd)
    assert sorted(got) == sorted(list(lora) + names)
    patch = RA.patch_bias_name(sd)
    bar = RB.BAR_LOOSE if (p_drop > 0 or D == 256) else RB.BAR
    errs = RB.errors(got, {k: ref[k] for k in names if k != patch}, sd)
    errs[patch] = float((got[patch].double() - ref[patch]).norm() / ref[patch].norm())
    layers = {k: e for k, e in errs.items() if k.startswith("layer")}
    print(f"lora_bias_all engine {tag} p={p_drop} streams={streams}: patch bias {errs[patch]:.3e}; worst layer vector {max(layers.values()):.3e} "
          f"({max(layers, key=layers.get)}); worst tensor {max(errs.values()):.3e} ({max(errs, key=errs.get)}) (bar {bar:.0e})")
    assert len(layers) == L
    for k, e in errs.items():
        assert e < bar, (k, e, bar)
    last = f"{lay}{L - 1}."
    for k in names:                                               # frozen slots: exact zeros, in f64 and here; the last layer's key bias and beta1 are live
        if k.startswith(last) and RB.leaf_of(k) not in RB.KEY_LEAVES + ("norm1",):
            assert float(ref[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k
    assert float(got[last + "norm1.bias"].abs().max()) > 0 and float(got[patch].abs().max()) > 0
    b1, b2, bp = eng.norm_off
    assert float(eng.lora_grad[1:, bp:bp + D].abs().max()) == 0.0 and float(eng.lora[1:, bp:bp + D].abs().max()) == 0.0     # the patch block is live in row 0 only
    if p_drop == 0:
        first = eng.lora_grad.clone()
        eng.forward_train(x)
        assert torch.equal(eng.backward(dkey), first)


# ------------------------------------------------------------------------------------------------ 8. the opt-in changes nothing
@pytest.mark.parametrize("tag,bias", [("g8", "none"), ("g8", "lora_only"), ("swiglu", "lora_only"), ("gated", "none")])
def test_the_opt_in_alone_changes_nothing(tag, bias):
    m = model(tag)
    lora = lora_of(m)
    x, dkey = (t.to(DEV) for t in m["inputs"])
    out = []
    for kw in ({}, {"allow_bias_all": True}):
        eng = ViTLoRAEngine(m["sd"], heads=m["heads"], r=m["r"], lora_alpha=m["alpha"], eps=m["eps"], device=DEV, generator=torch.Generator().manual_seed(3),
                            target_modules=list(m["targets"]), bias=bias, lora_dropout=0.05, seed=5, **m["kw"], **kw)
        eng.load_lora_state_dict({**{k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}, **lora})
        assert eng._norm_table(eng.lora_grad) is None and eng.norm_off is None
        key = eng.forward_train(x).clone()
        out.append((eng.lora.numel(), eng.lora.clone(), key, eng.backward(dkey).clone(), eng.forward_nograd(x).clone(), sum(w.numel() for w in eng._tside_ws if w is not None),
                    sorted(eng.lora_state_dict())))
    for a, b in zip(*out):
        assert a == b if not torch.is_tensor(a) else torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 9. merging, the adapter, the EMA clone
SPLIT3_G8_BAR = 3e-6            # tests/test_gpu_lora_bias.py / tests/test_gpu_lora_merge.py (terms=3 on this golden)
FOLDED_BAR = 3e-3               # tests/test_gpu_lora_merge.py: the folded fp16 default at D = 256


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_merged_state_dict_and_the_adapter_carry_every_bias(tmp_path):
    import json
    from safetensors.torch import load_file
    from ucod_dpl_amd.vit_engine import SplitViTEngine
    from ucod_dpl_amd.models.modules.full_model import load_lora_adapter, save_lora_adapter
    m = model("g8key")                                             # the key alone carries an adapter: five modules' biases, the betas and the patch bias are merged without one
    sd, heads = m["sd"], m["heads"]
    lora, moved = lora_of(m), RA.perturbed(sd)
    eng = all_engine(m, lora, 0.0, biases=moved)
    img = load_golden("g8_dinov2_native")["x"]
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora, **moved}.items() if v.is_floating_point()}
    ref = RO.forward(img.to(DEV, torch.float64), full, heads, eng.scaling).cpu()
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    for k, v in moved.items():
        assert torch.equal(merged[k], v) and not torch.equal(v, sd[k]), k
    assert merged["layernorm.bias"] is sd["layernorm.bias"]
    x = img.to(DEV)
    norms = [k for k in RA.norm_names(sd)]
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(x), ref)
    e_no_beta = rel_l2(SplitViTEngine({**merged, **{k: sd[k] for k in norms}}, heads=heads, device=DEV, terms=3)(x), ref)
    e_no_lin = rel_l2(SplitViTEngine({**merged, **{k: sd[k] for k in moved if k not in norms}}, heads=heads, device=DEV, terms=3)(x), ref)
    print(f"lora_bias_all merged: split3 {e_merged:.2e} (bar {SPLIT3_G8_BAR:.0e}); with the betas and the patch bias left unmerged {e_no_beta:.2e}; with the Linear biases "
          f"left unmerged {e_no_lin:.2e}")
    assert e_merged < SPLIT3_G8_BAR and e_no_beta > 100 * SPLIT3_G8_BAR and e_no_lin > 100 * SPLIT3_G8_BAR
    k_train = eng.forward_train(x)                                 # the training engine runs the perturbed vectors: repack carried them into its own buffer
    assert maxdiff(k_train.cpu(), ref) < 3e-2 * max(1.0, ref.abs().max().item())
    # the EMA clone: its own buffer, which follows ITS arena
    ema = eng.clone_for_ema()
    assert ema._bias_flat.data_ptr() != eng._bias_flat.data_ptr() and ema.patch_b.data_ptr() != eng.patch_b.data_ptr()
    assert ema.layers[0][N.LN1_B].data_ptr() != eng.layers[0][N.LN1_B].data_ptr() and torch.equal(ema.patch_b, eng.patch_b)
    b1, b2, bp = eng.norm_off
    ema.lora[0, bp:bp + 128] += 1.0
    ema.lora[1, b1:b1 + 128] += 1.0
    ema.repack()
    assert torch.equal(ema.patch_b, ema.lora[0, bp:bp + 128]) and torch.equal(ema.layers[1][N.LN1_B], ema.lora[1, b1:b1 + 128])
    assert not torch.equal(ema.patch_b, eng.patch_b) and torch.equal(eng.patch_b, moved[RA.patch_bias_name(sd)].to(DEV))
    # adapter folder -> a fresh engine: the same arena, the same buffer; the config says all; every ...bias tensor of the checkpoint is stored
    folder = save_lora_adapter(eng, str(tmp_path / "lora"))
    assert json.load(open(os.path.join(folder, "adapter_config.json")))["bias"] == "all"
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    pre = "base_model.model.ViT."
    assert sorted(tensors) == sorted(pre + k for k in list(lora) + [k for k in sd if "bias" in k])
    assert torch.equal(tensors[pre + "layernorm.bias"], sd["layernorm.bias"])
    for k, v in moved.items():
        assert torch.equal(tensors[pre + k], v), k
    other = all_engine(m, RO.lora_for(sd, m["targets"], seed=99), 0.0)
    assert not torch.equal(other.lora, eng.lora)
    load_lora_adapter(other, folder)
    assert torch.equal(other.lora, eng.lora) and torch.equal(other._bias_flat, eng._bias_flat)
    with pytest.raises(ValueError, match="bias is 'all'"):
        load_lora_adapter(all_engine(m, lora, 0.0, bias="lora_only"), folder)


def test_merge_into_refreshes_betas_and_every_fold():
    """D = 256 (the LayerNorm fold exists), the key alone targeted: merge_into on the default folded engine against an engine rebuilt from merged_state_dict() under
    the rules of tests/test_gpu_lora_bias.py -- the plain tables bit for bit, the folded weights and column sums bit for bit, the folded biases (which depend on the
    trained betas in EVERY folded QKV / fc1, targeted or not) within one f32 ulp plus 1e-12 |q| sum |w beta|."""
    from ucod_dpl_amd.vit_engine import ViTEngine, normalize_state_dict, _prepare_mlp
    m = dict(model("d256"), targets=("key",))
    sd, heads = m["sd"], m["heads"]
    lora, moved = RO.lora_for(sd, m["targets"]), RA.perturbed(sd)
    eng = all_engine(m, lora, 0.0, biases=moved)
    vit = ViTEngine(sd, heads=heads, device=DEV)
    assert vit.ln_fold
    x = m["inputs"][0].to(DEV)
    key_base = vit(x).clone()
    ptrs = [None if t is None else t.data_ptr() for rows in (vit.layers, vit.fold_layers) for row in rows for t in row]
    assert eng.merge_into(vit) is vit
    torch.cuda.synchronize()
    assert ptrs == [None if t is None else t.data_ptr() for rows in (vit.layers, vit.fold_layers) for row in rows for t in row], "merge_into reallocated a tensor"
    merged = eng.merged_state_dict()
    fresh = ViTEngine(merged, heads=heads, device=DEV)
    same = lambda a, b: a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b)  # noqa: E731
    _, mc = _prepare_mlp(normalize_state_dict(merged))
    assert torch.equal(vit.patch_b, fresh.patch_b)
    worst = 0.0
    for i in range(m["L"]):
        for s, (a, b) in enumerate(zip(vit.layers[i], fresh.layers[i])):
            assert (a is None and b is None) or same(a, b), (i, N.VIT_LAYER_SLOTS[s])
        for s, (a, b) in enumerate(zip(vit.fold_layers[i], fresh.fold_layers[i])):
            if a is not None and s not in (N.QKV_B, N.FC1_B):
                assert same(a, b), (i, N.VIT_LAYER_SLOTS[s])
        for slot_b, wname, bname in ((N.QKV_B, "qkv_w", "ln1_b"), (N.FC1_B, "fc1_w", "ln2_b")):
            got, want = vit.fold_layers[i][slot_b].cpu(), fresh.fold_layers[i][slot_b].cpu()
            q = vit.q_row_scale.cpu().double() if slot_b == N.QKV_B else torch.ones(got.numel(), dtype=torch.float64)
            ulp = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double()
            tol = ulp + 1e-12 * q * (mc["layers"][i][wname].double().abs() @ mc["layers"][i][bname].double().abs())
            err = (got.double() - want.double()).abs()
            worst = max(worst, float((err / ulp).max()))
            assert bool((err <= tol).all()), (i, N.VIT_LAYER_SLOTS[slot_b], float((err / tol).max()))
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora, **moved}.items() if v.is_floating_point()}
    ref = RO.forward(x.double(), full, heads, eng.scaling).cpu()
    k_live, k_fresh = vit(x), fresh(x)
    vit.check_overflow(wait=True)
    e_live, e_fresh = rel_l2(k_live, ref), rel_l2(k_fresh, ref)
    print(f"lora_bias_all merge_into, D = 256: live {e_live:.2e}, fresh {e_fresh:.2e} (bar {FOLDED_BAR:.0e}), live vs fresh {rel_l2(k_live, k_fresh):.2e}, "
          f"folded bias worst {worst:.2f} ulp, unrefreshed {rel_l2(key_base, ref):.2e}")
    assert e_live < FOLDED_BAR and e_fresh < FOLDED_BAR and rel_l2(key_base, ref) > 5 * e_live


# ------------------------------------------------------------------------------------------------ 10. the runner
def train_three_steps(tmp_path, tag):
    import json
    import math
    from safetensors.torch import save_file
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.models.modules.full_model import load_lora
    sd = model("g8")["sd"]
    weights = tmp_path / f"weights_{tag}"
    weights.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(weights / "model.safetensors"))
    (weights / "config.json").write_text(json.dumps({"model_type": "dinov2", "num_attention_heads": 2, "layer_norm_eps": 1e-6}))
    cfg = CfgNode(dict(
        model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, dis_use_features=False),
        lora_cfg=dict(r=2, lora_alpha=4, lora_dropout=0.05, target_modules=["query", "value", "dense"], allow_out=True, bias="all", allow_bias_all=True),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=6e-4, dis_lr0=1e-3, step_lr_size=2, dis_step_lr_size=2, deterministic=True,
                       step_lr_gamma=0.95, dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1,
                       dis_intertrain=2, save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50),
        dataset_cfg=dict(feature_extractor_cfg=dict(type="dinov2", backbone_type="huggingface", backbone="facebook/dinov2-base", backbone_weights=str(weights))),
        log_cfg=dict(log_interval=50, log_path=str(tmp_path / f"log_{tag}"), multi_rank=[0])))
    torch.manual_seed(3)
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    eng = load_lora(cfg.lora_cfg, sd, heads=2, device=DEV, generator=torch.Generator().manual_seed(1)).engine
    loop.attach_lora_backbone(eng)
    start = (eng.lora.clone(), loop.lora_engine_ema.lora.clone())
    img = load_golden("g8_dinov2_native")["x"].to(DEV)
    pl = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(11)) > 0.5).float()
    for _ in range(3):
        loss = loop._process_batch_full(img, pl)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    return eng, loop.lora_engine_ema, start


def test_training_moves_every_live_bias(tmp_path):
    sd = model("g8")["sd"]
    eng, ema, (lora0, ema0) = train_three_steps(tmp_path, "a")
    D, L = 128, 3
    assert eng.bias == ema.bias == "all" and all(o is not None for o in eng.bias_off) and eng.norm_off is not None
    assert ema._bias_flat.data_ptr() != eng._bias_flat.data_ptr()
    b1, b2, bp = eng.norm_off
    for e, first in ((eng, lora0), (ema, ema0)):
        for j, m in enumerate(e.modules):                          # every Linear bias, targeted or not: moved below the last layer (the key's there too), else an exact zero
            o, live = slice(m.bias_off, m.bias_off + m.nb), (L if j == 1 else L - 1)
            assert bool((e.lora[:live, o] != first[:live, o]).any(dim=1).all()), m.path
            assert live == L or float(e.lora[L - 1, o].abs().max()) == 0.0, m.path
        assert bool((e.lora[:, b1:b1 + D] != first[:, b1:b1 + D]).any(dim=1).all())                    # beta1 of every layer, the last included
        assert bool((e.lora[:L - 1, b2:b2 + D] != first[:L - 1, b2:b2 + D]).any(dim=1).all()) and float(e.lora[L - 1, b2:b2 + D].abs().max()) == 0.0
        assert not torch.equal(e.lora[0, bp:bp + D], first[0, bp:bp + D]) and float(e.lora[1:, bp:bp + D].abs().max()) == 0.0
        # the buffer the passes read follows the arena; frozen slots keep the checkpoint's bits
        assert torch.equal(e.patch_b, e.lora[0, bp:bp + D]) and torch.equal(e.layers[1][N.LN1_B], e.lora[1, b1:b1 + D]) and torch.equal(e.layers[0][N.LN2_B], e.lora[0, b2:b2 + D])
        assert torch.equal(e.layers[L - 1][N.LN2_B].cpu(), sd[f"encoder.layer.{L - 1}.norm2.bias"]) and torch.equal(e.layers[L - 1][N.FC2_B].cpu(), sd[f"encoder.layer.{L - 1}.mlp.fc2.bias"])
    assert not torch.equal(eng.lora, ema.lora)
    lsd, merged = eng.lora_state_dict(), eng.merged_state_dict()
    assert "layernorm.bias" not in lsd and merged["layernorm.bias"] is sd["layernorm.bias"]          # the final LayerNorm keeps its bits
    for k in (f"encoder.layer.{L - 1}.norm2.bias", f"encoder.layer.{L - 1}.mlp.fc1.bias"):
        assert torch.equal(lsd[k].cpu(), sd[k]) and torch.equal(merged[k].cpu(), sd[k]), k
    for k in ("encoder.layer.0.norm1.bias", "encoder.layer.0.mlp.fc1.bias", RA.patch_bias_name(sd), f"encoder.layer.{L - 1}.norm1.bias"):
        assert not torch.equal(lsd[k].cpu(), sd[k]) and torch.equal(merged[k].cpu(), lsd[k].cpu()), k
    eng2, ema2, _ = train_three_steps(tmp_path, "b")               # two runs from the same seed: identical arenas, student and teacher
    assert torch.equal(eng2.lora, eng.lora) and torch.equal(ema2.lora, ema.lora)


# ------------------------------------------------------------------------------------------------ 11. G27: transformers' own gradients
@pytest.mark.parametrize("tag", RA.G27_TAGS)
def test_engine_vs_g27(tag):
    """The engine with bias="all" against the f64 gradients transformers' own Dinov2Model / DINOv3ViTModel give their ``named_parameters()`` with "bias" in the name
    (tests/golden/make_golden_lora_bias_all.py), under the same bars and in the same measure; the names the engine trains are the golden's, the final LayerNorm
    aside; what torch leaves at grad = None is an exact zero here."""
    z, sd, heads, lora, scale, x, dkey, v3 = RA.g27(tag)
    kw = dict(allow_rope=True, allow_swiglu=True, allow_mlp_in=True) if v3 else dict(allow_swiglu=True, allow_out=True, allow_swiglu_out=True)
    targets = sorted({k.rsplit(".", 3)[-3] for k in lora})
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=2 * scale, eps=1e-5 if v3 else 1e-6, device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=targets, bias="all", allow_bias_all=True, lora_dropout=0.0, **kw)
    eng.load_lora_state_dict({**{k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}, **lora})
    eng.train_streams = 1
    key = eng.forward_train(x.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items() if ".lora_" not in k}
    want = RA.g27_grads(z)
    assert sorted(got) == sorted(want) == sorted(str(n) for n in z["names"] if str(n) not in RA.FINAL_NORMS)
    errs = RA.errors(got, want, sd)
    key_err = rel_l2(key, torch.from_numpy(z["key"]))
    print(f"lora_bias_all G27 {tag}: key rel-L2 {key_err:.3e}; worst of layer vectors, tensors and the patch bias {max(errs.values()):.3e} ({max(errs, key=errs.get)}) "
          f"(bar {RB.BAR:.0e})")
    for k, e in errs.items():
        assert e < RB.BAR, (k, e)
    for n in want:
        if int(z["none/" + n]):
            assert float(got[n].abs().max()) == 0.0, n
