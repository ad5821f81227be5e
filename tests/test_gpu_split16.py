"""GPU: the split-operand backbone pass on fp16 terms ("split2h": two fp16 terms per operand, three partial products on the fp16 MFMA; include/ucod_dpl.h
"the split-operand pass on fp16 TERMS", csrc/split16.hip, SplitViTEngine(terms=2, term="f16")).

Mirrors the rows of tests/test_gpu_split.py.  Layouts are compared bit for bit with the torch restatement tests/split16_ref.py (itself checked against f64 in
tests/test_split16_host.py), pieces against f64 arithmetic on the same inputs, and the ENGINE against the three-term bf16 engine (split3, the f32-equivalent
pass of today) measured in the same test on the same inputs:  err(split2h) <= 4 err(split3) + 1e-7  -- 2^2 for 22 instead of 24 significand bits.
"""
import math

import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops  # noqa: E402
from ucod_dpl_amd.vit_engine import SplitViTEngine  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import backbone, ARCHS, trained_like_state_dict  # noqa: E402
from oracle import decoder as OD, vit as OV  # noqa: E402
from oracle.resize import torch_bilinear  # noqa: E402
import split16_ref as R  # noqa: E402
from split16_ref import rel_l2  # noqa: E402

DEV = "cuda"
S_LN, S_HID = 64.0, 16.0                                        # class scales of the pass (ucod_split16_class_scale; checked below)


def record(name, values):
    from test_gpu_parity_c2 import record as rec
    rec(name, values)


def relation(e16, e3):
    """The engine rows' bound: four times the three-term engine's error on the same inputs (22 against 24 bits) plus 1e-7."""
    return e16 <= 4.0 * e3 + 1e-7


def test_mfma_keeps_or_flushes_subnormal_fp16_inputs():
    """v_mfma_f32_32x32x16_f16 on 2^-24 (the smallest fp16 subnormal) x 2^14: 2^-10 if subnormal inputs are kept, 0 if they are flushed; the control 2^-14 x 2^14 = 1
    (smallest normal) must be exact either way.  The answer decides the floor of the operand split (2^-25 / s kept, 2^-14 / s flushed) and is recorded in DESIGN.md 5.2."""
    out = torch.full((2,), -1.0, dtype=torch.float32, device=DEV)
    N.check(N.load("f16").ucod_split16_mfma_subnormal_probe(N.ptr(out), N.stream()), "probe")
    sub_v, ctl = (float(v) for v in out.cpu())
    print(f"fp16 MFMA subnormal probe: 2^-24 * 2^14 -> {sub_v!r} (2^-10 = {2.0 ** -10!r}), control -> {ctl!r}")
    record("split16_mfma_subnormal_probe", dict(subnormal_product=sub_v, control=ctl, kept=sub_v == 2.0 ** -10))
    assert ctl == 1.0
    assert sub_v in (0.0, 2.0 ** -10)
    assert sub_v == 2.0 ** -10, "the fp16 MFMA flushes subnormal inputs: the floor of the split is 2^-14 / s, not 2^-25 / s (csrc/split16.hip, DESIGN.md 5.2)"


def test_class_scales_are_what_the_tests_assume():
    assert [ops.split16_class_scale(c) for c in (N.SPLIT16_LN, N.SPLIT16_QKV, N.SPLIT16_PROB, N.SPLIT16_ATT, N.SPLIT16_HIDDEN, N.SPLIT16_PATCH)] == [64.0, 32.0, 16384.0, 32.0, 16.0, 512.0]


@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 64.0, 2.0 ** 11])
def test_split_rows_layout_and_reconstruction(role, scale):
    g = torch.Generator().manual_seed(int(scale) + role)
    x = torch.randn(37, 72, generator=g) * torch.logspace(-9, 0, 72)[None, :] * (8.0 / scale * 64)       # nine decades, the largest values near 2^11 after scaling
    assert R.saturated(x, scale) == 0
    xs = ops.split_rows(x.to(DEV), 2, role, term="f16", scale=scale).cpu()
    assert xs.shape == (37, 3 * 72) and xs.dtype == torch.float16
    assert torch.equal(xs, R.layout(x, scale, role))               # bit-identical to the restatement, subnormal lo terms included
    hi, lo = xs[:, :72], xs[:, 144:] if role == 0 else xs[:, 72:144]
    err = (R.reconstruct(hi, lo, scale) - x.double()).abs()
    assert bool((err <= R.recon_bound(x, scale)).all()), float((err / R.recon_bound(x, scale)).max())
    rec = ops.unsplit(xs.to(DEV), 2, role, 72, term="f16", scale=scale).cpu()
    assert bool(((rec.double() - x.double()).abs() <= R.recon_bound(x, scale) + 2.0 ** -24 * x.double().abs()).all())
    # a strided view (columns 8 .. 71 of a wider matrix), GELU and scaling fused in front of the split
    wide = torch.randn(19, 80, generator=g).to(DEV)
    v = wide[:, 8:]
    assert torch.equal(ops.split_rows(v, 2, role, term="f16", scale=64.0).cpu(), R.layout(v.cpu(), 64.0, role))
    ge = ops.unsplit(ops.split_rows(v, 2, role, op=1, alpha=0.5, term="f16", scale=16.0), 2, role, 72, term="f16", scale=16.0).cpu().double()
    assert maxdiff(ge, torch.nn.functional.gelu(v.cpu().double() * 0.5)) < 3e-7 + 2.0 ** -22 * 6
    sc = ops.unsplit(ops.split_rows(v, 2, role, op=2, alpha=0.18033688, term="f16", scale=32.0), 2, role, 72, term="f16", scale=32.0).cpu()
    assert maxdiff(sc, v.cpu() * 0.18033688) < 1e-6


@pytest.mark.parametrize("M,Nn,K", [(200, 256, 256), (1370, 2304, 768), (4111, 768, 3072), (8220, 3072, 768)])
def test_linear_split_against_f64(M, Nn, K):
    """x w^T + b on fp16-term operands vs the f64 product of the SAME f32 inputs.  Bound 1e-6: the emulation with exact accumulation gives 7.4e-8, the MFMA's f32
    accumulation adds what it adds to a plain f32 GEMM (3.5e-7 for torch's on the host); still 4x under the two-term bf16 form's 4.4e-6."""
    g = torch.Generator().manual_seed(M + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05, torch.randn(Nn, generator=g)
    ref = x.double() @ w.double().t() + b.double()
    out = ops.linear_split(x.to(DEV), w.to(DEV), b.to(DEV), 2, term="f16").cpu()
    err, f32_err = rel_l2(out, ref), rel_l2(x @ w.t() + b, ref)
    emu = rel_l2(R.linear3(x, w, b, R.pow2_scale(x), R.pow2_scale(w)), ref) if M <= 1370 else float("nan")
    print(f"linear split2h M={M} N={Nn} K={K}: rel-L2 {err:.3e} (torch f32 {f32_err:.3e}, emulation with exact accumulation {emu:.3e})")
    record("split16_linear", dict(M=M, N=Nn, K=K, rel_l2=err, torch_f32_rel_l2=f32_err, emulation_rel_l2=emu))
    assert err < 1e-6, err
    assert err < 10 * f32_err + 2e-7, (err, f32_err)
    assert maxdiff(out.double(), ref) < 40 * 1e-6 * float(ref.abs().max())


LN_SHAPES = [(5, 128), (777, 384), (1371, 768), (333, 1024), (64, 1536), (7, 256), (9, 512), (11, 640), (6, 1280)]      # every D / 128 the pass admits


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_split(rows, D):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, D, generator=g) * 3 + 0.5
    x[:, 5] = 200.0                                             # a massive channel
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-6)
    for role in (0, 1):
        xs = ops.layernorm_split(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, 2, role, term="f16")
        assert xs.shape == (rows, 3 * D) and xs.dtype == torch.float16
        seg = xs.view(rows, 3, D)
        assert torch.equal(seg[:, 0], seg[:, 1 if role == 0 else 2])          # hi | hi | lo  /  hi | lo | hi
        hi = seg[:, 0].float()
        got = ops.unsplit(xs, 2, role, D, term="f16", scale=S_LN).cpu().double()
        # (the three-term bf16 row's bound: the f32 LayerNorm arithmetic itself; the 2^-22 split is below it)
        assert maxdiff(got, ref) < 2e-6 * max(1.0, float(ref.abs().max())), (maxdiff(got, ref), role)
        # lo is the split of what hi leaves: |lo| <= half an ulp of hi
        assert bool((seg[:, 2 if role == 0 else 1].float().abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -24).all())


FC1_SHAPES = [(200, 256, 256, 0), (200, 256, 256, 12), (1370, 3072, 768, 0), (4111, 1024, 256, 9), (8220, 3072, 768, 13), (43840, 3072, 768, 0),
              (4111, 1024, 256, 10), (8220, 1024, 768, 14), (1370, 3072, 768, 1), (1370, 3072, 768, 2), (4111, 1000, 256, 10), (4111, 4096, 256, 10)]     # 10 / 14 with N % 192 != 0 too


@pytest.mark.parametrize("M,Nn,K,variant", FC1_SHAPES)
def test_fc1_f32_epilogue_then_gelu_row_split(M, Nn, K, variant):
    """fc1 + GELU + split AS THE PASS RUNS IT -- two launches, NOT a fused epilogue (DESIGN.md 5.2 states the deviation and its measured cost): the fp16-build GEMM
    with the existing f32 epilogue on K-concatenated operands (accumulator = s_a s_b times the product, bias scaled to match), then ucod_split16_rows op 1 with
    alpha = 1 / (s_a s_b).  Every tile path the plan can select: 64 x 64 (12), 128 x 128 (1 / 2), one-shot large tiles 256 / 192 wide (9 / 10), mixed-height
    (13 / 14), N a multiple of 192 or not.  Both launches write rows of exactly N (3 N) elements, so the bytes behind a row's valid columns are the next row's first
    columns: a store past column N lands in checked data (the max-abs bound below) or, behind the last row, in the guard rows.
    Bound 2e-6 = the linear row's 1e-6 x GELU's largest slope 1.13 / the norm GELU keeps of a centred input (~0.6)."""
    g = torch.Generator().manual_seed(M + Nn)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05, torch.randn(Nn, generator=g) * 0.2
    ref = torch.nn.functional.gelu(x.double() @ w.double().t() + b.double())
    sw = ops.pow2_scale(w)
    S = S_LN * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=S_LN), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    f1 = torch.full((M + 3, Nn), -7.0, dtype=torch.float32, device=DEV)            # three guard rows behind the matrix
    ops._gemm_f16(N.EPI_BIAS_F32, xs, ws, f1, M, Nn, 3 * K, bias=(b * S).to(DEV), variant=variant)
    assert bool((f1[M:] == -7.0).all())
    out = torch.full((M + 3, 3 * Nn), -7.0, dtype=torch.float16, device=DEV)
    N.check(N.load("f16").ucod_split16_rows(N.ptr(f1), Nn, N.ptr(out), M, Nn, 0, 1, 1.0 / S, S_HID, N.stream()), "ucod_split16_rows")
    assert bool((out[M:] == -7.0).all())
    seg = out[:M].view(M, 3, Nn)
    assert torch.equal(seg[:, 0], seg[:, 1])                        # hi | hi
    got = ops.unsplit(out[:M].contiguous(), 2, 0, Nn, term="f16", scale=S_HID).cpu().double()
    err = rel_l2(got, ref)
    print(f"fc1+GELU split2h M={M} N={Nn} K={K} variant={variant}: rel-L2 {err:.3e}")
    assert err < 2e-6, err
    assert maxdiff(got, ref) < 40 * 2e-6 * max(1.0, float(ref.abs().max()))


def test_swiglu_row_op():
    """ucod_split16_rows op 3 (SwiGLU of interleaved rows 2 K wide, pitch wider than 2 K) against f64; 3e-7 = the three-term bf16 row's 2e-7 (f32 SiLU) + the
    2^-23 rms-ish rounding of lo."""
    from test_gpu_swiglu import swiglu_f64
    lib = N.load("f16")
    M, K = 300, 1024
    x = torch.randn(M, 2 * K + 64, device=DEV) * 3.0
    out = torch.full((M + 2, 3 * K), -7.0, dtype=torch.float16, device=DEV)
    assert lib.ucod_split16_rows(N.ptr(x), 2 * K + 64, N.ptr(out), M, K, 0, 3, 1.0, S_HID, N.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[M:] == -7.0).all())
    ref = swiglu_f64(x[:, :2 * K])
    seg = out[:M].view(M, 3, K)
    assert torch.equal(seg[:, 0], seg[:, 1])
    got = (seg[:, 0].double() + seg[:, 2].double()) / S_HID
    assert rel_l2(got, ref) < 3e-7, rel_l2(got, ref)
    # alpha multiplies both halves before the activation (the operand scales of fc1 leaving)
    x8 = (x * 8.0).contiguous()
    out2 = torch.empty(M, 3 * K, dtype=torch.float16, device=DEV)
    assert lib.ucod_split16_rows(N.ptr(x8), 2 * K + 64, N.ptr(out2), M, K, 0, 3, 0.125, S_HID, N.stream()) == 0
    assert torch.equal(out2, out[:M])
    assert lib.ucod_split16_rows(N.ptr(x), K, N.ptr(out), M, K, 0, 3, 1.0, S_HID, N.stream()) == -1            # op 3 reads rows 2 K wide


def attention_f64(qkv, B, tok, heads):
    D = heads * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().view(B, tok, heads, 64).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(2, 3) * 0.125, -1)
    return (p @ v).transpose(1, 2).reshape(B * tok, D)


@pytest.mark.parametrize("B,tok,heads,gain", [(2, 1370, 12, 1.0), (3, 197, 2, 4.0), (1, 33, 2, 4.0), (2, 257, 6, 8.0), (1, 64, 1, 1.0), (2, 20, 2, 4.0)])
def test_attention_split_against_f64(B, tok, heads, gain):
    """softmax(Q K^T / 8) V on fp16-term operands vs f64, incl. peaked rows (gain 4 / 8), token counts that are / are not multiples of 32, the padded last key
    block and a single key block (20 tokens).  Yardstick as in the bf16 rows: torch's f32 attention on the host (a score of magnitude s carries s 2^-24, which
    is the relative error of its exponential).  Two bounds: 4 x the three-term row's (1e-6 + 4 f32_err), and -- the engine rows' relation -- 4 x what the
    three-term bf16 KERNEL shows on the same inputs in this same test, + 1e-7: 22 against 24 bits in Q, K and the probabilities."""
    g = torch.Generator().manual_seed(tok + heads)
    qkv = torch.randn(B * tok, 3 * heads * 64, generator=g)
    qkv[:, :2 * heads * 64] *= math.sqrt(gain)
    ref = attention_f64(qkv, B, tok, heads)
    s_att = ops.split16_class_scale(N.SPLIT16_ATT)
    xs = ops.attention_split(qkv.to(DEV), B, tok, heads, 2, term="f16")
    seg = xs.view(B * tok, 3, heads * 64)
    assert torch.equal(seg[:, 0], seg[:, 1])
    got = ops.unsplit(xs, 2, 0, heads * 64, term="f16", scale=s_att).cpu()
    assert bool(torch.isfinite(got).all())
    D = heads * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].view(B, tok, heads, 64).transpose(1, 2) for i in range(3))
    f32_err = rel_l2((torch.softmax(q @ k.transpose(2, 3) * 0.125, -1) @ v).transpose(1, 2).reshape(B * tok, D), ref)
    err = rel_l2(got, ref)
    err3 = rel_l2(ops.unsplit(ops.attention_split(qkv.to(DEV), B, tok, heads, 3), 3, 0, heads * 64).cpu(), ref)
    print(f"attention split2h B={B} tok={tok} heads={heads} gain={gain}: rel-L2 {err:.3e} (three-term bf16 kernel {err3:.3e}, torch f32 {f32_err:.3e})")
    record("split16_attention", dict(B=B, tok=tok, heads=heads, gain=gain, rel_l2=err, split3_rel_l2=err3, torch_f32_rel_l2=f32_err))
    tol = 4 * (1e-6 + 4 * f32_err)
    assert err < tol, (err, gain, f32_err)
    assert relation(err, err3), (err, err3)
    assert maxdiff(got.double(), ref) < 30 * tol * float(ref.abs().max())
    # the same operands scaled on the way in (the QKV GEMM's operand scales leaving): same bits
    xs2 = ops.attention_split((qkv * 2.0 ** 20).to(DEV), B, tok, heads, 2, term="f16", in_mul=2.0 ** -20)
    assert torch.equal(xs2, xs)


def engines(sd, heads):
    return SplitViTEngine(sd, heads=heads, eps=1e-6, device=DEV, terms=2, term="f16"), SplitViTEngine(sd, heads=heads, eps=1e-6, device=DEV, terms=3)


@pytest.mark.parametrize("name,heads", [("g8_dinov2_native", 2), ("g8_dinov2_interp", 2), ("g8_dinov1_native", 2), ("g8_dinov1_interp", 2)])
def test_split_engine_against_reference_golden(name, heads):
    gd = load_golden(name)
    e16, e3 = engines(sub(gd, "sd."), heads)
    assert e16.half == "f16x2" and e16.term == "f16" and e3.term == "bf16"
    x = gd["x"].to(DEV)
    key = e16(x).cpu()
    e16.check_overflow(wait=True)
    assert key.shape == gd["key"].shape
    err16, err3 = rel_l2(key, gd["key"]), rel_l2(e3(x).cpu(), gd["key"])
    print(f"{name}: key rel-L2 split2h {err16:.3e}, split3 {err3:.3e}")
    record("split16_golden", dict(name=name, split2h=err16, split3=err3))
    assert relation(err16, err3), (err16, err3)
    assert err16 < 3e-6                                             # (the three-term row's own bound)
    k1 = e16.forward(x, n_layers=1).cpu()                           # truncated passes return that layer's key map
    assert k1.shape == key.shape and not torch.equal(k1, key)
    k2, events = e16.forward_async(x)                               # asynchronous form on the side stream: same bits
    for e in events:
        torch.cuda.current_stream().wait_event(e)
    assert torch.equal(k2.cpu(), key)
    e16.check_overflow(wait=True)


@pytest.mark.parametrize("D,heads,L", [(128, 2, 3), (256, 4, 4)])
def test_swiglu_engine_vs_restatement(D, heads, L):
    """The ViT-g form (SwiGLU MLP, tests/swiglu_ref.py) at small width against its f64 restatement."""
    from swiglu_ref import random_swiglu_state_dict
    from test_gpu_swiglu import f64_key
    sd = random_swiglu_state_dict(D, heads, L, seed=D)
    img = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(5))
    _, ref, _ = f64_key(sd, img, heads, full_last_layer=False)
    e16, e3 = engines(sd, heads)
    assert e16.mlp == N.UCOD_MLP_SWIGLU and e16.F == 384 * D // 128
    key = e16(img.to(DEV))
    e16.check_overflow(wait=True)
    err16, err3 = rel_l2(key, ref), rel_l2(e3(img.to(DEV)), ref)
    print(f"SwiGLU D={D}: key rel-L2 split2h {err16:.3e}, split3 {err3:.3e}")
    record("split16_swiglu", dict(D=D, split2h=err16, split3=err3))
    assert relation(err16, err3), (err16, err3)


@pytest.fixture(scope="module")
def peaked():
    """BASELINE configs[1] geometry, two images, the TRAINED-LIKE synthetic checkpoint: the inputs of tests/test_gpu_split.py's `peaked` fixture."""
    arch, n = "dinov2_vitb14", 2
    D, heads, L, P, _, _ = ARCHS[arch]
    sd = trained_like_state_dict(arch, 0, 518)
    img = torch.randn(n, 3, 518, 518, generator=torch.Generator().manual_seed(2024))
    with torch.no_grad():
        _, key = OV.dinov2_forward(img, sd, heads=heads, patch=P, eps=1e-6, full_last_layer=False)
        dec = OD.init_params(D, torch.Generator().manual_seed(42))
        fg, _, _ = OD.rev_decoder_forward(torch_bilinear(key, 68, 68), dec, orth="gram")
    return dict(sd=sd, img=img, key=key, fg=fg, dec=dec, heads=heads, D=D, n=n)


def test_c2_full_size_on_trained_like_weights_against_split3(peaked):
    """ViT-B/14 at 518 x 518, full depth, trained-like weights: key map and mask logits of the fp16-term engine against the f32 oracle, bounded by four times what the
    three-term bf16 engine shows on the same inputs in this same test (+1e-7), and in any case by the 2e-4 "far inside the bar" line of the two-term bf16 row."""
    from test_gpu_parity_c2 import device_logits
    c = peaked
    e16, e3 = engines(c["sd"], c["heads"])
    img = c["img"].to(DEV)
    res = {}
    for name, eng in (("split2h", e16), ("split3", e3)):
        key_dev = eng(img)
        eng.check_overflow(wait=True)
        assert bool(torch.isfinite(key_dev).all())
        fd = device_logits(key_dev, c["dec"], c["n"], c["D"])
        res[name] = dict(key_rel_l2=rel_l2(key_dev.cpu(), c["key"]), logit_max_abs=float((fd - c["fg"]).abs().max()), logit_rel_l2=rel_l2(fd, c["fg"]),
                         mask_flipped_fraction=float(((fd > 0) != (c["fg"] > 0)).float().mean()))
    print(f"c2 peaked: {res}")
    record("split16_c2_peaked", res)
    a, b = res["split2h"], res["split3"]
    assert a["logit_max_abs"] <= 2e-4, a
    assert a["mask_flipped_fraction"] == 0.0
    assert relation(a["key_rel_l2"], b["key_rel_l2"]), (a, b)
    assert relation(a["logit_max_abs"], b["logit_max_abs"]), (a, b)
    assert relation(a["logit_rel_l2"], b["logit_rel_l2"]), (a, b)


def test_key_map_does_not_depend_on_the_batch(peaked):
    c = peaked
    eng = SplitViTEngine(c["sd"], heads=c["heads"], eps=1e-6, device=DEV, terms=2, term="f16")
    img = torch.cat((c["img"], torch.randn(4, 3, 518, 518, generator=torch.Generator().manual_seed(5))), 0).to(DEV)
    k6 = eng(img).clone()
    k1 = eng(img[:1].contiguous())
    eng.check_overflow(wait=True)
    assert rel_l2(k1, k6[:1]) < 5e-6                             # other tile shapes = another f32 summation order, nothing else (the three-term row's bound)


def test_cls_attention_row_against_the_reference_and_split3():
    """forward_with_cls_attention: the CLS query's softmax row of the last layer against the HF model's own (G14), bounded by the three-term engine's in the same test."""
    g = load_golden("g14_pseudo_label")
    sd = sub(g, "sd.")
    e16, e3 = engines(sd, 2)
    x = g["x"].to(DEV)
    ref_att, kref = g["attn_cls"][:, :, 1:], g["key"][:, 1:, :]
    out = {}
    for name, eng in (("split2h", e16), ("split3", e3)):
        key, att = eng.forward_with_cls_attention(x)
        eng.check_overflow(wait=True)
        out[name] = (rel_l2(att, ref_att), rel_l2(key.cpu().flatten(2).transpose(1, 2), kref), att)
    print(f"CLS attention row rel-L2: split2h {out['split2h'][0]:.3e}, split3 {out['split3'][0]:.3e}; key {out['split2h'][1]:.3e} / {out['split3'][1]:.3e}")
    assert relation(out["split2h"][0], out["split3"][0]) and relation(out["split2h"][1], out["split3"][1]), out
    assert out["split2h"][0] < 2e-5 and out["split2h"][1] < 5e-6      # (the three-term row's own bounds)
    assert maxdiff(out["split2h"][2].sum(-1).cpu() + g["attn_cls"][:, :, 0], torch.ones(3, 2)) < 1e-5


def test_precision_name_on_the_public_surface(tmp_path):
    """backbone(precision="split2h") / with_precision, and precision="split2h" through build_feature_cache, PseudoLabelGenerator and CORAL's WindowFeatures; the
    defaults are unchanged ("f32eq" is still the three-term bf16 engine)."""
    from ucod_dpl_amd.data.datasets import MultiCacheManager, build_feature_cache
    from ucod_dpl_amd.generate_pseudo_label import PseudoLabelGenerator
    gd = load_golden("g8_dinov2_native")
    bb = backbone.from_state_dict(sub(gd, "sd."), heads=2, device=DEV)
    h = bb.with_precision("split2h")
    assert isinstance(h.engine, SplitViTEngine) and h.engine.term == "f16" and h.engine.terms == 2 and h.precision == "split2h"
    assert bb.with_precision("split2h") is h and h.with_precision("split2h") is h
    eq = bb.with_precision("f32eq")
    assert eq.engine.terms == 3 and eq.engine.term == "bf16" and eq is not h
    assert backbone.from_state_dict(sub(gd, "sd."), heads=2, device=DEV, precision="split2h").engine.term == "f16"
    x = gd["x"]
    fc = MultiCacheManager(str(tmp_path), "dinov2", "val", "T").get_features_cache()
    assert build_feature_cache([x[i] for i in range(x.shape[0])], bb, fc, batch_size=2, device=DEV, precision="split2h") == x.shape[0]
    for i in range(x.shape[0]):
        assert rel_l2(fc.read_file(i), gd["key"][i]) < 3e-6
    gen = PseudoLabelGenerator(bb, th_bkg=0.6, precision="split2h")
    assert gen.engine is h.engine
    assert PseudoLabelGenerator(bb, th_bkg=0.6).engine.terms == 3                   # default unchanged
    from ucod_dpl_amd.engine.runner.loop_CORAL import WindowFeatures
    import inspect
    assert inspect.signature(WindowFeatures.__init__).parameters["precision"].default == "f32eq"


def test_saturation_is_counted_and_raises():
    """Finite inputs beyond an operand class's bound (pixels of 1000 against the patch class's 127.9) are clamped, counted on the device, and check_overflow(wait=True)
    raises instead of letting the wrong key map pass; the next clean pass does not raise again.  A counted condition, not a fault."""
    gd = load_golden("g8_dinov2_native")
    eng = SplitViTEngine(sub(gd, "sd."), heads=2, eps=1e-6, device=DEV, terms=2, term="f16")
    x = gd["x"].to(DEV)
    good = eng(x).clone()
    eng.check_overflow(wait=True)
    bad = x.clone()
    bad[0, 0, :4, :4] = 1000.0
    key = eng(bad)
    assert bool(torch.isfinite(key).all())                          # clamped, never inf / NaN
    with pytest.raises(FloatingPointError, match="split2h"):
        eng.check_overflow(wait=True)
    assert torch.equal(eng(x), good)
    eng.check_overflow(wait=True)
    # another engine on the same device saw nothing
    other = SplitViTEngine(sub(gd, "sd."), heads=2, eps=1e-6, device=DEV, terms=2, term="f16")
    other(x)
    other.check_overflow(wait=True)


def test_refusals_of_both_libraries():
    x = torch.zeros(8, 64, dtype=torch.float32, device=DEV)
    out = torch.zeros(8, 64 * 6, dtype=torch.bfloat16, device=DEV)
    f, b = N.load("f16"), N.load("bf16")
    assert b.ucod_split16_rows(N.ptr(x), 64, N.ptr(out), 8, 64, 0, 0, 1.0, 1.0, N.stream()) == -1          # the bf16 library refuses the new entry points
    assert b.ucod_split16_layernorm(N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(out), 8, 128, 1e-6, 0, 64.0, N.stream()) == -1
    assert b.ucod_split16_scale_f32(N.ptr(x), 8 * 64, 0.5, N.stream()) == -1
    assert f.ucod_split16_rows(N.ptr(x), 64, N.ptr(out), 8, 64, 0, 0, 1.0, 1.0, N.stream()) == 0
    assert f.ucod_split16_rows(N.ptr(x), 64, N.ptr(out), 8, 64, 0, 0, 1.0, 3.0, N.stream()) == -1          # scale not a power of two
    assert f.ucod_split16_rows(N.ptr(x), 64, N.ptr(out), 8, 60, 0, 0, 1.0, 1.0, N.stream()) == -1          # K % 8
    assert f.ucod_split_rows(N.ptr(x), 64, N.ptr(out), 8, 64, 2, 0, 0, 1.0, N.stream()) == -1              # ... and the fp16 library still refuses the old ones
    assert f.ucod_layernorm_split(N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(out), 8, 128, 1e-6, 2, 0, N.stream()) == -1
    torch.cuda.synchronize()
