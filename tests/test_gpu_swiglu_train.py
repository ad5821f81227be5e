"""GPU: backbone-backward (LoRA) mode on the SwiGLU MLP of DINOv2 ViT-g/14 (transformers modeling_dinov2.py:300-315), every call through the C ABI or the engine.

1. the two GEMM epilogues (UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 / UCOD_EPI_SWIGLU_BWD_BF16) against f64 on the same bf16-rounded operands, with canary rows around both
   outputs, every payload element written, the hidden bit for bit that of the inference epilogue, and the refusals;
2. whole passes (ucod_vit_forward_train_mlp / ucod_vit_backward_mlp) against f64 autograd through the SwiGLU restatement (tests/swiglu_ref.py) with the LoRA
   matrices merged into the query / key / value weights -- without dropout that is LoRA exactly;
3. the engine's passes against each other and against the frozen-backbone engine;
4. the public surface (load_lora / full_model) on a SwiGLU checkpoint.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, swiglu  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, ViTLoRAEngine  # noqa: E402
from swiglu_ref import dinov2_swiglu_forward, random_swiglu_state_dict  # noqa: E402

DEV = "cuda"
EINVAL = -1
GUARD_ROWS = 64
CANARY = 0x5A3C                                                 # (as bf16: a finite value no kernel here produces in whole rows)
SAVE, BWD, SWIGLU = N.EPI_BIAS_SWIGLU_SAVE_BF16, N.EPI_SWIGLU_BWD_BF16, N.EPI_BIAS_SWIGLU_BF16


def rel_l2(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def record(name, values):
    from test_gpu_parity_c2 import record as rec
    rec(name, values)


class Guarded:
    """bf16 [M, cols] between GUARD_ROWS canary rows on either side; the payload starts as NaN, so an element no store reached shows."""

    def __init__(self, M, cols):
        self.M, self.cols = M, cols
        self.buf = torch.full(((M + 2 * GUARD_ROWS), cols), CANARY, dtype=torch.int16, device=DEV)
        self.payload = self.buf[GUARD_ROWS:GUARD_ROWS + M].view(torch.bfloat16)
        self.payload.fill_(float("nan"))

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD_ROWS] == CANARY).all()) and bool((self.buf[GUARD_ROWS + self.M:] == CANARY).all())

    def all_written(self):
        return bool(torch.isfinite(self.payload.float()).all())


# ------------------------------------------------------------------------------------------------ 1. epilogues
SHAPES = [(300, 512, 128), (2740, 3072, 768), (1370, 8192, 1536)]           # (M, 2F, K)
VARIANTS = [0, 9, 10]


@functools.lru_cache(maxsize=None)
def operands(M, N2, K):
    """bf16-rounded operands of one shape and their f64 references, computed once and shared by the variants (never modified)."""
    F = N2 // 2
    g = torch.Generator(device=DEV).manual_seed(M + N2)
    A = (torch.randn(M, K, device=DEV, generator=g) * 0.5).bfloat16()
    W_in = (torch.randn(N2, K, device=DEV, generator=g) * K ** -0.5).bfloat16()       # interleaved weights_in [2F, K]
    b_in = torch.randn(N2, device=DEV, generator=g)
    W_out_t = (torch.randn(F, K, device=DEV, generator=g) * K ** -0.5).bfloat16()     # weights_out^T [F, K]
    aux = (torch.randn(M, N2, device=DEV, generator=g) * 1.5).bfloat16()
    pre_ref = A.double() @ W_in.double().t() + b_in.double()
    hid_ref = swiglu.swiglu_interleaved(pre_ref)
    bwd_ref = swiglu.swiglu_interleaved_grad(aux.double(), A.double() @ W_out_t.double().t())
    return dict(A=A, W_in=W_in, b_in=b_in, W_out_t=W_out_t, aux=aux, pre_ref=pre_ref, hid_ref=hid_ref, bwd_ref=bwd_ref)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_swiglu_save_epilogue(shape, variant):
    M, N2, K = shape
    F = N2 // 2
    o = operands(*shape)
    lib = N.load()
    hid, pre = Guarded(M, F), Guarded(M, N2)
    rc = lib.ucod_gemm_bf16_train(SAVE, N.ptr(o["A"]), N.ptr(o["W_in"]), hid.ptr(), M, N2, K, N.ptr(o["b_in"]), None, pre.ptr(), variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert hid.guards_intact() and pre.guards_intact(), "wrote outside its outputs"
    assert hid.all_written() and pre.all_written(), "left payload elements unwritten"
    e_pre, e_hid = rel_l2(pre.payload, o["pre_ref"]), rel_l2(hid.payload, o["hid_ref"])
    print(f"SAVE {shape} variant {variant}: pre {e_pre:.2e} hidden {e_hid:.2e}")
    assert e_pre < 4e-3, e_pre                                  # one bf16 rounding of an f32 value (test_gemm_train_epilogues' bound)
    assert e_hid < 3e-3, e_hid                                  # test_gpu_swiglu.py::test_swiglu_epilogue_vs_f64's bound for the bf16 library
    inf = torch.empty(M, F, dtype=torch.bfloat16, device=DEV)
    assert lib.ucod_gemm_bf16(SWIGLU, N.ptr(o["A"]), N.ptr(o["W_in"]), N.ptr(inf), M, N2, K, N.ptr(o["b_in"]), None, None, None, 0, variant, N.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(hid.payload.view(torch.int16), inf.view(torch.int16)), "training-mode hidden differs from the inference epilogue's"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_swiglu_bwd_epilogue(shape, variant):
    M, N2, K = shape
    F = N2 // 2
    o = operands(*shape)
    lib = N.load()
    out = Guarded(M, N2)
    rc = lib.ucod_gemm_bf16_train(BWD, N.ptr(o["A"]), N.ptr(o["W_out_t"]), out.ptr(), M, F, K, None, N.ptr(o["aux"]), None, variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside its output"
    assert out.all_written(), "left payload elements unwritten"
    err = rel_l2(out.payload, o["bwd_ref"])
    print(f"BWD {shape} variant {variant}: {err:.2e}")
    assert err < 5e-3, err                                      # one bf16 rounding of an f32 value (test_gemm_train_epilogues' bound for the GELU dgrad)


def test_swiglu_bwd_padded_hidden_units_give_exact_zeros():
    M, F, K = 300, 256, 128
    o = operands(300, 512, 128)
    aux = o["aux"].clone()
    aux.view(M, -1, 2, 4)[:, -8:] = 0                           # the last 32 hidden units are padding: x1 = x2 = 0
    out = torch.empty(M, 2 * F, dtype=torch.bfloat16, device=DEV)
    assert N.load().ucod_gemm_bf16_train(BWD, N.ptr(o["A"]), N.ptr(o["W_out_t"]), N.ptr(out), M, F, K, None, N.ptr(aux), None, 0, N.stream()) == 0
    torch.cuda.synchronize()
    assert float(out[:, -64:].float().abs().max()) == 0.0 and float(out[:, :-64].float().abs().max()) > 0.0


def test_swiglu_train_epilogue_refusals():
    M, N2, K = 300, 512, 128
    F = N2 // 2
    o = operands(M, N2, K)
    lib, f16 = N.load(), N.load("f16")
    A, W, b, Wt, aux = (N.ptr(o[k]) for k in ("A", "W_in", "b_in", "W_out_t", "aux"))
    out, out2 = Guarded(M, N2), Guarded(M, N2)
    before = (out.buf.clone(), out2.buf.clone())
    st = N.stream()
    calls = {
        "save N % 8": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2 - 4, K, b, None, out2.ptr(), 0, st),
        "bwd N % 8": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F - 4, K, None, aux, None, 0, st),
        "save K = 64": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2, 64, b, None, out2.ptr(), 0, st),
        "bwd K = 64": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F, 64, None, aux, None, 0, st),
        "save null out2": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2, K, b, None, None, 0, st),
        "save null bias": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2, K, None, None, out2.ptr(), 0, st),
        "bwd null aux": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F, K, None, None, None, 0, st),
        "save through ucod_gemm_bf16": lambda: lib.ucod_gemm_bf16(SAVE, A, W, out.ptr(), M, N2, K, b, None, None, None, 0, 0, st),
        "bwd through ucod_gemm_bf16": lambda: lib.ucod_gemm_bf16(BWD, A, Wt, out.ptr(), M, F, K, None, None, None, None, 0, 0, st),
        "save in the fp16 library": lambda: f16.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2, K, b, None, out2.ptr(), 0, st),
        "bwd in the fp16 library": lambda: f16.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F, K, None, aux, None, 0, st),
        # the widest row set [M, 2F] bf16 must fit 31-bit byte offsets: sizes only, the check precedes any launch
        "save 2^31": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), 1 << 17, 8192, K, b, None, out2.ptr(), 0, st),
        "bwd 2^31": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), 1 << 17, 4096, K, None, aux, None, 0, st),
        # no 64 x 64 kernel and no laboratory variant drains these epilogues
        "save variant 12": lambda: lib.ucod_gemm_bf16_train(SAVE, A, W, out.ptr(), M, N2, K, b, None, out2.ptr(), 12, st),
        "bwd variant 12": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F, K, None, aux, None, 12, st),
        "bwd variant 5": lambda: lib.ucod_gemm_bf16_train(BWD, A, Wt, out.ptr(), M, F, K, None, aux, None, 5, st),
    }
    for name, call in calls.items():
        assert call() != 0, name
    torch.cuda.synchronize()
    assert torch.equal(out.buf, before[0]) and torch.equal(out2.buf, before[1]), "a refused call wrote to its outputs"


# ------------------------------------------------------------------------------------------------ the LoRA gradient kernel at ViT-g's width
@pytest.mark.parametrize("M,D,r", [(53, 1536, 2), (700, 1280, 3)])
def test_lora_grad_beyond_d1024(M, D, r):
    """ucod_lora_grad at the widths the two-stream form covers (D / 128 = 10, 12; block reduction buffer past 64 KiB at 1536): the checks and bounds of
    tests/test_gpu_vit_train.py::test_lora_grad."""
    import math
    AUG = N.LORA_AUG
    g = torch.Generator().manual_seed(M + r)
    scaling = 2.0
    parts, mats = [], []
    for _ in range(3):
        A, Bm = torch.randn(r, D, generator=g) / math.sqrt(D), torch.randn(D, r, generator=g) * 0.05
        parts += [A.reshape(-1), Bm.reshape(-1)]
        mats.append((A, Bm))
    flat = torch.cat(parts)
    dqkv, h = torch.randn(M, 3 * D, generator=g).bfloat16(), torch.randn(M, D, generator=g).bfloat16()
    u = torch.cat([h.float() @ A.t() for A, _ in mats], 1).bfloat16()
    d_aug, h_aug = torch.zeros(M, 3 * D + AUG, dtype=torch.bfloat16), torch.zeros(M, D + AUG, dtype=torch.bfloat16)
    d_aug[:, :3 * D], h_aug[:, :D], h_aug[:, D:D + 3 * r] = dqkv, h, u
    lib = N.load()
    wsb = lib.ucod_lora_grad_workspace_bytes(D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    grad = torch.full((6 * r * D,), 9.0, device=DEV)
    ds, hs, fs = d_aug.to(DEV), h_aug.to(DEV), flat.to(DEV)
    N.check(lib.ucod_lora_grad(N.ptr(ds), N.ptr(hs), N.ptr(fs), r, scaling, N.ptr(grad), 0, N.ptr(ws), wsb, M, D, None, N.stream()), "lora_grad")
    grad, t_out = grad.cpu(), ds.float().cpu()[:, 3 * D:]
    maxdiff = lambda a, b: (a.double() - b.double()).abs().max().item()  # noqa: E731
    off = 0
    for p, (A, Bm) in enumerate(mats):
        dq = dqkv[:, p * D:(p + 1) * D].double()
        t = scaling * dq @ Bm.double()
        assert maxdiff(t_out[:, p * r:(p + 1) * r], t) < 1e-2 * max(1.0, t.abs().max().item())
        tb = t_out[:, p * r:(p + 1) * r].double()                            # the kernel uses the bf16-rounded t for dA
        dA, dB = tb.t() @ h.double(), scaling * dq.t() @ u[:, p * r:(p + 1) * r].double()
        gA, gB = grad[off:off + r * D].reshape(r, D), grad[off + r * D:off + 2 * r * D].reshape(D, r)
        off += 2 * r * D
        assert maxdiff(gA, dA) < 2e-4 * max(1.0, dA.abs().max().item()), p
        assert maxdiff(gB, dB) < 2e-4 * max(1.0, dB.abs().max().item()), p
    assert float(t_out[:, 3 * r:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 2. whole passes vs f64 autograd
_QKV = ("query", "key", "value")


def f64_lora_reference(sd, lora_sd, img, dkey, heads, scaling):
    """(key, {peft name: gradient}) in f64: the SwiGLU restatement on q / k / v weights W + scaling B A, A and B the leaves."""
    from oracle import vit as OV
    sdd = {k: v.to(DEV, torch.float64) for k, v in sd.items()}
    gh, gw = img.shape[-2] // 14, img.shape[-1] // 14
    sdd["embeddings.position_embeddings"] = OV.dinov2_pos_embed(sd["embeddings.position_embeddings"].double(), gh, gw).to(DEV)
    leaves = {k: v.to(DEV, torch.float64).requires_grad_(True) for k, v in lora_sd.items()}
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    for i in range(L):
        for nm in _QKV:
            base = f"encoder.layer.{i}.attention.attention.{nm}."
            sdd[base + "weight"] = sdd[base + "weight"] + scaling * leaves[base + "lora_B.weight"] @ leaves[base + "lora_A.weight"]
    _, key, _ = dinov2_swiglu_forward(img.to(DEV, torch.float64), sdd, heads, full_last_layer=False)
    names = sorted(leaves)
    grads = torch.autograd.grad((key * dkey.to(DEV, torch.float64)).sum(), [leaves[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, grads)}


def lora_engine(sd, heads, gen_seed=3, **kw):
    """A LoRA engine on a SwiGLU checkpoint with B = 0.05 randn (peft initialises B to zero: the LoRA branch would vanish)."""
    gen = torch.Generator().manual_seed(gen_seed)
    eng = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=gen, allow_swiglu=True, **kw)
    lsd = eng.lora_state_dict()
    for k in lsd:
        if "lora_B" in k:
            lsd[k] = 0.05 * torch.randn(lsd[k].shape, generator=gen)
    eng.load_lora_state_dict(lsd)
    return eng


# (D, heads, L, image, batch, gradient bar): F 344 padded to 384 | 2 x 2 chunks of 81 patches | the real width, F = 4096 unpadded, 26 tokens
PASSES = [(128, 2, 3, 70, 2, 4e-2), (256, 4, 4, 126, 3, 5e-2), (1536, 24, 2, 70, 2, 5e-2)]


@pytest.mark.parametrize("D,heads,L,image,B,bar", PASSES)
def test_lora_passes_vs_f64_autograd(D, heads, L, image, B, bar):
    """Measured on MI355X (the `swiglu_lora_passes` rows this test records): key max-abs 3.1e-3 / 4.3e-3 / 1.2e-2 against bars 3.0e-2 / 4.1e-2 / 8.5e-2, worst LoRA
    gradient rel-L2 9.3e-3 / 1.0e-2 / 9.1e-3 against 4e-2 / 5e-2 / 5e-2 -- the bars of the GELU tests for this operand type and depth (tests/test_gpu_vit_train.py)."""
    sd = random_swiglu_state_dict(D, heads, L, image_size=image, seed=D)
    eng = lora_engine(sd, heads)
    assert eng.mlp == N.UCOD_MLP_SWIGLU and eng.F == swiglu.padded_hidden(eng.F) and eng.train_layers[0][N.T_FC1_WT].shape == (D, 2 * eng.F)
    gen = torch.Generator().manual_seed(7)
    gh = image // 14
    img, dkey = torch.randn(B, 3, image, image, generator=gen), torch.randn(B, D, gh, gh, generator=gen)
    key_ref, gref = f64_lora_reference(sd, {k: v.cpu() for k, v in eng.lora_state_dict().items()}, img, dkey, heads, eng.scaling)
    key = eng.forward_train(img.to(DEV))
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    got = eng.lora_state_dict(grads=True)
    key_err = (key.double() - key_ref).abs().max().item()
    key_bar = 3e-2 * max(1.0, key_ref.abs().max().item())
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=errs.get)
    record("swiglu_lora_passes", dict(D=D, L=L, image=image, B=B, key_max_abs=key_err, key_bar=key_bar, worst_grad_rel_l2=errs[worst], worst_grad=worst))
    print(f"D={D} L={L}: key max-abs {key_err:.2e} (bar {key_bar:.2e}), worst gradient rel L2 {errs[worst]:.2e} ({worst})")
    assert key_err < key_bar, key_err
    zero = [k for k, ref in gref.items() if float(ref.abs().max()) == 0.0]
    assert len(zero) == 4 and all(f"layer.{L - 1}." in k for k in zero)      # the last layer's query / value LoRA: only its key projection reaches the loss
    for k in zero:
        assert float(got[k].abs().max()) == 0.0, k
    assert len(errs) == 6 * L - 4
    for k, e in errs.items():
        assert e < bar, (k, e)


# ------------------------------------------------------------------------------------------------ 3. engine consistency
@pytest.fixture(scope="module")
def small_sd():
    return random_swiglu_state_dict(128, 2, 3, seed=128)


@pytest.fixture(scope="module")
def small_img():
    return torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(5)).to(DEV)


def test_forward_train_is_deterministic(small_sd, small_img):
    eng = lora_engine(small_sd, 2)
    assert torch.equal(eng.forward_train(small_img), eng.forward_train(small_img))


def test_forward_nograd_matches_forward_train_under_dropout(small_sd, small_img):
    engine = lambda: lora_engine(small_sd, 2, lora_dropout=0.3, seed=11)  # noqa: E731      (equal seeds: the same parameters and the same masks)
    k_train = engine().forward_train(small_img)
    k_f32 = engine().forward_nograd(small_img, resid16=False)
    k_f16 = engine().forward_nograd(small_img, resid16=True)
    assert bool(torch.isfinite(k_f16).all())
    assert rel_l2(k_f32, k_train) < 2e-3, rel_l2(k_f32, k_train)
    assert rel_l2(k_f16, k_train) < 4e-3, rel_l2(k_f16, k_train)


def test_forward_train_with_zero_b_matches_the_frozen_engine(small_sd, small_img):
    eng = ViTLoRAEngine(small_sd, heads=2, device=DEV, allow_swiglu=True)    # lora_B = 0: the LoRA branch vanishes
    inf = ViTEngine(small_sd, heads=2, device=DEV, attn_variant=2, half="bf16")
    k0, k1 = inf(small_img), eng.forward_train(small_img)
    assert (k0 - k1).abs().max().item() < 1e-2 * max(1.0, k0.abs().max().item())


# ------------------------------------------------------------------------------------------------ 4. public surface
def test_load_lora_and_full_model_train_a_swiglu_checkpoint(small_sd, small_img):
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.models.modules.full_model import LoRABackbone, full_model, load_lora
    from ucod_dpl_amd.models.uscod import baseline
    torch.manual_seed(0)
    cfg = CfgNode(dict(model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, enable_ocm=False, freeze_lora=False), lora_cfg=dict(r=2, lora_alpha=4, lora_dropout=0.0)))
    bb = load_lora(cfg.lora_cfg, small_sd, heads=2, device=DEV)
    assert isinstance(bb, LoRABackbone) and bb.engine.mlp == N.UCOD_MLP_SWIGLU
    fm = full_model(cfg, bb, baseline(cfg.model_cfg).to(DEV))
    fm.hook_size = 8                                            # (a 5 x 5 grid: 5 -> 68 is outside the resize adjoint's tap budget)
    fg, bg, extra = fm(small_img)
    loss = fg.square().mean() + bg.square().mean() + extra
    loss.backward()
    g = fm.backbone.lora.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
    assert fm.backbone_ema.lora.grad is None
    t = fm(small_img, ema=True)
    assert not t.requires_grad and bool(torch.isfinite(t).all())


def test_lora_engine_without_the_keyword_still_refuses(small_sd):
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        ViTLoRAEngine(small_sd, heads=2, device=DEV)
