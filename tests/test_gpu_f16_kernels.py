"""GPU: the kernels of the fp16-operand library (libucod_dpl_f16.so: the default engine and the headline since round 6) against f64 references, every
call through the C ABI of the library under test (native.load(half)).  The kernel-level tests of tests/test_gpu_kernels.py run on the bf16 build only.

Attention (ucod_attention_fwd: attn_fwd_v5_kernel, attn_fwd_v6_kernel, the generic-scale attn_fwd_kernel), both builds.  Reference: f64 softmax(Q K^T) V on
the rounded operands; bound: F times the error of the CPU rounding model of tests/f16_ref.py (P rounded to the operand type, denominator from the unrounded
P, one output rounding), in relative L2 (there the tighter F_L2) and in the worst row.  The model puts bf16 at 1.85e-3 and fp16 at 2.3e-4; the bars of the product tests (4e-3
relative L2) would take an fp16 kernel with eight times its error.  Input families (f16_ref.py): R as the product tests draw it; S, where every score is
<= -22 so that a padded key counted as real carries the row; P, where every probability but one is an fp16 subnormal; D, the deferred-max constructions.
tests/test_f16_ref_host.py shows on the CPU that the rule refuses each of those faults.

GEMM epilogues of the fp16 library against the f64 product of the same fp16 operands, on every tile path; LayerNorm, im2col, CLS rows and the CLS
query / key projection against f64 / bit-exact references.  Every bound check goes through conftest.within (profiles/f16_kernels_tolerance_audit.jsonl).

Measured on an MI355X (ratio to the model's error; profiles/f16_kernels_tolerance_audit.jsonl holds every figure):
    generic kernel, both builds, every family      relative L2 0.85 - 1.05, worst row 0.77 - 1.03: the model IS this kernel's arithmetic
    v5 / v6, fp16                                  relative L2 1.00 - 1.25, worst row up to 2.79 (R, 200 tokens; S 2.10, D 1.28, P <= 1.00)
    v5 / v6, bf16                                  relative L2 1.00 - 1.26, worst row up to 2.23 (R, 200 tokens; S 2.03, D 1.43)
v5 and v6 agree to the last digit printed.  Their excess over the model is the deferred maximum (f16_ref.py, at F): rows whose first 32 keys hold the row
maximum sit at 1.00, rows whose running maximum trails carry the rounding of the heaviest key's P, which the model has exactly 1.  Not v_exp_f32, not the
summation order.  F = 3.5 (1.25 x the worst ratio), F_L2 = 1.9 (1.5 x the worst relative-L2 ratio).  No kernel fault was found: subnormal fp16 probabilities
are kept by the conversion and by the matrix pipe, no padded key is counted, guard rows stay, launches repeat bit for bit.
"""
import functools
import math

import pytest
import torch

import f16_ref as R
from conftest import within
from gemm_exact_ref import plan

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}               # half an ulp of the 16-bit output type, relative
SENT = -5.0                                                     # guard value (exact in every type used here)


def _guarded(rows, cols, dtype, guard=64):
    return torch.full((rows + guard, cols), SENT, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t == SENT).all())


# ================================================================================================ attention
FORMS = {"v5": (0.0, 0, True), "v6": (0.0, 66, True), "generic": (0.125, 0, False)}          # form -> (scale, variant, Q stored pre-scaled)
ATTN_SHAPES = [(1, 26, 2), (2, 64, 1), (1, 65, 3), (3, 129, 2), (1, 200, 3), (2, 255, 2), (1, 256, 1), (2, 257, 2), (1, 513, 1), (2, 300, 12), (9, 257, 1),
               (1, 1370, 2)]


@functools.lru_cache(maxsize=None)
def _attn_case(fam, arg, half, prescaled):
    """(qkv16, B, tok, heads, ref, model), computed once per (family, size, operand type, storage of Q) and shared by the entry forms."""
    dt = DT[half]
    if fam in ("r", "s"):
        B, tok, heads = arg
        x = (R.family_r if fam == "r" else R.family_s)(B, tok, heads, dt, prescaled)
    elif fam == "p":
        B, tok, heads = 1, R.P_TOK, 1
        x = R.family_p(arg, dt, prescaled)
    else:
        B, heads = 1, 1
        x, tok = R.family_d(arg, dt, prescaled)
    ls = 1.0 if prescaled else R.C_PRE
    return x, B, tok, heads, R.attention_ref(x, B, tok, heads, ls), R.attention_model(x, B, tok, heads, ls)


def _check_attention(half, form, fam, arg):
    scale, variant, prescaled = FORMS[form]
    x, B, tok, heads, ref, model = _attn_case(fam, arg, half, prescaled)
    lib = N.load(half)
    D = heads * 64
    assert x.shape == (B * tok, 3 * D)
    qd = x.to(DEV)
    bufs = [_guarded(B * tok, D, DT[half]) for _ in range(2)]
    for buf in bufs:
        assert lib.ucod_attention_fwd(N.ptr(qd), N.ptr(buf), B, tok, heads, scale, variant, N.stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(bufs[0][B * tok:]), "rows behind the output were written"
    assert torch.equal(bufs[0], bufs[1]), "a second launch differs"
    out = bufs[0][:B * tok].cpu()
    assert bool(torch.isfinite(out.float()).all())
    name = f"f16_kernels attention {half} {form} {fam} {arg}"
    e2, m2, er, mr = R.rel_l2(out, ref), R.rel_l2(model, ref), R.row_err(out, ref), R.row_err(model, ref)
    print(f"{name}: rel L2 {e2:.3e} (model {m2:.3e}, ratio {e2 / m2:.3f}) worst row {er:.3e} (model {mr:.3e}, ratio {er / mr:.3f})")
    within(name + " rel_l2", e2, R.F_L2 * m2)
    within(name + " worst row", er, R.F * mr)


@pytest.mark.parametrize("B,tok,heads", ATTN_SHAPES)
@pytest.mark.parametrize("fam", ["r", "s"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("half", ["f16", "bf16"])
def test_attention_against_the_rounding_model(half, form, fam, B, tok, heads):
    """Token counts: below one tile (26), one key tile exactly and one past it (64 / 65), three tiles and one key (129), rows past N in the only work item
    (200), around the 256-row work item of v6 (255 / 256 / 257), 513, several items per workgroup (12 heads x 2 images; 9 images of one head), 1370."""
    _check_attention(half, form, fam, (B, tok, heads))


@pytest.mark.parametrize("dominant", [0, 333])
@pytest.mark.parametrize("form", list(FORMS))
def test_attention_keeps_fp16_subnormal_probabilities(form, dominant):
    """Family P: all but one probability of every row is an fp16 subnormal and together they carry ~0.8 of the output.  Flushed to zero (by the conversion
    or by the matrix pipe) the relative error is 0.67; kept, the model's 2.6e-4.  bf16 has no such regime."""
    _check_attention("f16", form, "p", dominant)


@pytest.mark.parametrize("case", R.D_CASES)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("half", ["f16", "bf16"])
def test_attention_deferred_max_branches(half, form, case):
    _check_attention(half, form, "d", case)


# ================================================================================================ GEMM epilogues of the fp16 library
H = HALF_ULP["f16"]
# (M, N, K, variant) -> the kernel it launches on 256 CUs (gemm_exact_ref.plan, the mirror of launch(); asserted per case below): 64 x 64 and 128 x 128 tiles,
# auto at one image (198 128-tiles < 256 CUs: the 64 x 64 kernel again), the one-shot 256-wide large tile (51 tiles: no whole round, so NO leftover patches), the 192-wide one, 13 on a shape whose
# mixed-height plan is infeasible (33 tall tiles of 28: falls back to 9, a plain extra round), a long K on the small tile; then the shapes that DO reach the
# leftover patches and the mixed-height kernel (the fp16 residual epilogue takes the mixed-height kernel from 2048 rows up, whatever the variant), and an
# auto shape with 264 128-tiles, which does take the 128 x 128 kernel
GEMM_SHAPES = [(200, 256, 256, 12), (200, 256, 256, 2), (1370, 2304, 768, 0), (4111, 768, 768, 9), (5000, 768, 768, 10), (8220, 2304, 768, 13), (333, 128, 3072, 0),
               (21916, 768, 768, 9), (21916, 768, 768, 13), (1370, 3072, 768, 0)]
GEMM_PATHS = {(200, 256, 256, 12): "t64", (200, 256, 256, 2): "t128", (1370, 2304, 768, 0): "t64", (4111, 768, 768, 9): "big256", (5000, 768, 768, 10): "big192",
              (8220, 2304, 768, 13): "big256", (333, 128, 3072, 0): "t64", (21916, 768, 768, 9): "big256+patches", (21916, 768, 768, 13): "mixed256",
              (1370, 3072, 768, 0): "t128"}


def _kmul(K):
    """f32 accumulation error grows as a random walk in K: the 4e-5 term, set at K <= 1536, times sqrt(K / 1024) at K = 3072."""
    return math.sqrt(3.0) if K >= 3072 else 1.0


@functools.lru_cache(maxsize=None)
def _gemm_case(M, Nn, K):
    g = torch.Generator().manual_seed(M + Nn + K)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(Nn, K, generator=g) * 0.05).half()
    b, sc = torch.randn(Nn, generator=g) * 0.1, 0.5 + torch.rand(Nn, generator=g)
    resid = torch.randn(M, Nn, generator=g) * 2
    acc = A.double() @ W.double().t() + b.double()
    return A, W, b, sc, resid, acc


def _bound16(name, out, ref, kmul=1.0):
    ref = ref.double()
    err = (out.double() - ref).abs()
    within(name, float((err / (H * ref.abs() + 4e-5 * kmul * (1 + ref.abs()))).max()), 1.0)


def _bound32(name, out, ref, kmul=1.0):
    ref = ref.double()
    err = (out.double() - ref).abs()
    within(name + " elementwise", float((err / (4e-5 * kmul * (1 + ref.abs()))).max()), 1.0)
    within(name + " rel_l2", R.rel_l2(out, ref), 1e-5)


EPIS = {"bias16": N.EPI_BIAS_BF16, "gelu16": N.EPI_BIAS_GELU_BF16, "bias32": N.EPI_BIAS_F32, "resid32": N.EPI_BIAS_SCALE_RESID_F32, "resid16": N.EPI_BIAS_SCALE_RESID_H16}


@pytest.mark.parametrize("M,Nn,K,variant", GEMM_SHAPES)
@pytest.mark.parametrize("epi", list(EPIS))
def test_gemm_epilogues_against_the_f64_product(epi, M, Nn, K, variant):
    """out = epilogue(A W^T) on fp16 operands with f32 accumulation: the f64 product of the SAME operands, to one fp16 rounding of the output plus the f32
    accumulation (16-bit outputs) / the f32 accumulation alone (f32 outputs).  The two residual epilogues run IN PLACE (out aliases resid, as the driver
    calls them); rows past M keep their guard value; none of these (shape, variant) pairs may be refused, and each launches the kernel GEMM_PATHS names."""
    lib = N.load("f16")
    path = plan(epi, M, Nn, K, variant, torch.cuda.get_device_properties(0).multi_processor_count).path
    assert path == ("mixed256" if epi == "resid16" and M >= 2048 else GEMM_PATHS[(M, Nn, K, variant)]), (epi, M, Nn, K, variant, path)
    A, W, b, sc, resid, acc = _gemm_case(M, Nn, K)
    Ad, Wd, bd, scd = A.to(DEV), W.to(DEV), b.to(DEV), sc.to(DEV)
    f32_out = epi in ("bias32", "resid32")
    buf = _guarded(M, Nn, torch.float32 if f32_out else torch.float16)
    r = None
    if epi.startswith("resid"):
        r = resid if f32_out else resid.half()
        buf[:M] = r.to(DEV)
    rc = lib.ucod_gemm_bf16(EPIS[epi], N.ptr(Ad), N.ptr(Wd), N.ptr(buf), M, Nn, K, N.ptr(bd), N.ptr(scd) if r is not None else None,
                            N.ptr(buf) if r is not None else None, None, 0, variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _untouched(buf[M:])
    out = buf[:M].cpu()
    ref = acc
    if epi == "gelu16":
        ref = torch.nn.functional.gelu(acc)
    elif r is not None:
        ref = r.double() + sc.double() * acc
    name = f"f16_kernels gemm {epi} {M}x{Nn}x{K} v{variant}"
    (_bound32 if f32_out else _bound16)(name, out, ref, _kmul(K))


def test_gemm_refuses_what_its_tiles_cannot_take():
    """ucod_gemm_bf16 of the fp16 library returns UCOD_EINVAL (-1) and launches nothing: large-tile variants need N % 4 == 0 (N % 8 == 0 for 16-bit output),
    K % 64 == 0, laboratory variants and the epilogues of the other entry points are refused."""
    lib = N.load("f16")
    M, K = 256, 128
    A, W = torch.zeros(M, K, dtype=torch.float16, device=DEV), torch.zeros(104, K, dtype=torch.float16, device=DEV)
    b = torch.zeros(104, device=DEV)
    buf = _guarded(M, 104, torch.float32)                                                          # (large enough for every output type below)

    def call(epi, Nn, Kk, variant):
        return lib.ucod_gemm_bf16(epi, N.ptr(A), N.ptr(W), N.ptr(buf), M, Nn, Kk, N.ptr(b), None, None, None, 0, variant, N.stream())
    assert call(N.EPI_BIAS_BF16, 100, K, 9) == -1 and call(N.EPI_BIAS_GELU_BF16, 100, K, 10) == -1       # 16-bit rows: N % 8
    assert call(N.EPI_BIAS_F32, 102, K, 9) == -1 and call(N.EPI_BIAS_F32, 102, K, 10) == -1              # f32 rows: N % 4
    assert call(N.EPI_BIAS_F32, 104, K, 9) == 0 and call(N.EPI_BIAS_BF16, 104, K, 10) == 0                # (the same calls at a width the tiles take)
    assert call(N.EPI_BIAS_BF16, 104, 96, 0) == -1                                                        # K % 64
    for lab in (3, 5, 8, 11, 15):
        assert call(N.EPI_BIAS_BF16, 104, K, lab) == -1, lab
    for epi in (N.EPI_LNFOLD_BIAS_BF16, N.EPI_BIAS_SCALE_RESID_H16_STATS, N.EPI_GELU_BWD_BF16, N.EPI_BIAS_SWIGLU_SPLIT2):
        assert call(epi, 104, K, 0) == -1, epi
    torch.cuda.synchronize()
    assert _untouched(buf[M:])


@functools.lru_cache(maxsize=None)
def _patch_case():
    g = torch.Generator().manual_seed(42)
    Bimg, npatch, D, K = 40, 64, 256, 640
    A = (torch.randn(Bimg * npatch, K, generator=g) * 0.5).half()
    W = (torch.randn(D, K, generator=g) * 0.05).half()
    b, pos = torch.randn(D, generator=g), torch.randn(npatch + 1, D, generator=g)
    ref = (A.double() @ W.double().t() + b.double()).view(Bimg, npatch, D) + pos[1:].double()
    return Bimg, npatch, D, K, A, W, b, pos, ref


@pytest.mark.parametrize("variant", [0, 9, 10, 2])
@pytest.mark.parametrize("h16", [False, True])
def test_patch_token_epilogues_against_the_f64_product(variant, h16):
    """UCOD_EPI_PATCH_TOKENS_F32 / _H16: 40 images of 64 patches (row tiles straddle images), rows remapped past the CLS rows, + bias + position embedding;
    the CLS rows and the rows behind the last image stay untouched."""
    lib = N.load("f16")
    Bimg, npatch, D, K, A, W, b, pos, ref = _patch_case()
    tok = npatch + 1
    Ad, Wd, bd, pd = A.to(DEV), W.to(DEV), b.to(DEV), pos.to(DEV)
    buf = _guarded(Bimg * tok, D, torch.float16 if h16 else torch.float32)
    rc = lib.ucod_gemm_bf16(N.EPI_PATCH_TOKENS_H16 if h16 else N.EPI_PATCH_TOKENS_F32, N.ptr(Ad), N.ptr(Wd), N.ptr(buf), Bimg * npatch, D, K, N.ptr(bd), None, None,
                            N.ptr(pd), tok, variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = buf[:Bimg * tok].view(Bimg, tok, D).cpu()
    assert _untouched(got[:, 0]) and _untouched(buf[Bimg * tok:])
    (_bound16 if h16 else _bound32)(f"f16_kernels patch tokens {'h16' if h16 else 'f32'} v{variant}", got[:, 1:], ref)


@functools.lru_cache(maxsize=None)
def _key_case(C, K, Bimg, tok):
    g = torch.Generator().manual_seed(41 + C)
    Wk = (torch.randn(C, K, generator=g) * 0.1).half()
    x = torch.randn(Bimg * tok, K, generator=g).half()
    bias = torch.randn(C, generator=g)
    ref = (x.double() @ Wk.double().t() + bias.double()).view(Bimg, tok, C)[:, 1:].transpose(1, 2)
    return Wk, x, bias, ref


@pytest.mark.parametrize("variant", [0, 9, 10, 2])
@pytest.mark.parametrize("C,K,Bimg,tok", [(256, 128, 60, 50), (512, 128, 700, 50)])
def test_key_hook_epilogue_against_the_f64_product(C, K, Bimg, tok, variant):
    """UCOD_EPI_KEY_NCHW_F32: rows = channels, columns = tokens, a CLS column every 50 (most 64-column waves straddle an image), written as [B, C, tok - 1]
    with the per-channel bias; 3000 columns (128 x 128 tiles by auto) and the 35000 of tests/test_gpu_kernels.py (large tile)."""
    lib = N.load("f16")
    Wk, x, bias, ref = _key_case(C, K, Bimg, tok)
    Wd, xd, bd = Wk.to(DEV), x.to(DEV), bias.to(DEV)
    out = torch.full((Bimg + 1, C, tok - 1), SENT, device=DEV)
    rc = lib.ucod_gemm_bf16(N.EPI_KEY_NCHW_F32, N.ptr(Wd), N.ptr(xd), N.ptr(out), C, Bimg * tok, K, N.ptr(bd), None, None, None, tok, variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _untouched(out[Bimg])
    _bound32(f"f16_kernels key hook {C}x{K}x{Bimg * tok} v{variant}", out[:Bimg].cpu(), ref)


# ================================================================================================ row kernels
def _ln_ref(x, w, b, eps=1e-6):
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    return (xd - mean) * (var + eps).rsqrt() * w.double() + b.double()


@pytest.mark.parametrize("rows", [37, 777])
@pytest.mark.parametrize("D", [128, 384, 768, 1024, 1536])
@pytest.mark.parametrize("half", ["f16", "bf16"])
def test_layernorm_against_f64(half, D, rows):
    """ucod_layernorm (f32 rows -> f32 / 16-bit) and ucod_layernorm_h16 (fp16 rows -> 16-bit) with one channel at 200 (a massive activation: the row's
    variance is its square over D): 16-bit outputs to one rounding of the output type plus 2e-5 of the output scale, f32 outputs to 2e-5."""
    lib = N.load(half)
    g = torch.Generator().manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) * 3 + 0.5
    x[:, 5] = 200.0
    w, b = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref = _ln_ref(x, w, b)
    name = f"f16_kernels layernorm {half} {rows}x{D}"
    y32 = _guarded(rows, D, torch.float32, guard=8)
    assert lib.ucod_layernorm(N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(y32), rows, D, 1e-6, 1, N.stream()) == 0
    y16 = _guarded(rows, D, DT[half], guard=8)
    assert lib.ucod_layernorm(N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(y16), rows, D, 1e-6, 0, N.stream()) == 0
    x16 = x.half()
    x16d = x16.to(DEV)
    yh = _guarded(rows, D, DT[half], guard=8)
    assert lib.ucod_layernorm_h16(N.ptr(x16d), N.ptr(wd), N.ptr(bd), N.ptr(yh), rows, D, 1e-6, N.stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(y32[rows:]) and _untouched(y16[rows:]) and _untouched(yh[rows:])
    within(name + " f32 out", float((y32[:rows].cpu().double() - ref).abs().max()), 2e-5)
    for tag, y, r in (("16-bit out", y16, ref), ("h16", yh, _ln_ref(x16, w, b))):
        err = (y[:rows].cpu().double() - r).abs()
        bound = HALF_ULP[half] * r.abs() + 2e-5 * max(1.0, float(r.abs().max()))
        within(f"{name} {tag}", float((err / bound).max()), 1.0)


@pytest.mark.parametrize("half", ["f16", "bf16"])
def test_layernorm_refuses_widths_it_has_no_kernel_for(half):
    lib = N.load(half)
    x = torch.zeros(8, 2048, device=DEV)
    x16 = torch.zeros(8, 2048, dtype=torch.float16, device=DEV)
    w = torch.ones(2048, device=DEV)
    y = _guarded(8, 2048, torch.float32, guard=8)
    for D in (64, 896, 200):                                     # not a multiple of 128; 7 x 128 has no instance
        assert lib.ucod_layernorm(N.ptr(x), N.ptr(w), N.ptr(w), N.ptr(y), 8, D, 1e-6, 1, N.stream()) == -1, D
        assert lib.ucod_layernorm(N.ptr(x), N.ptr(w), N.ptr(w), N.ptr(y), 8, D, 1e-6, 0, N.stream()) == -1, D
    for D in (64, 200, 1664, 2048):                              # fp16 rows: D <= 1536
        assert lib.ucod_layernorm_h16(N.ptr(x16), N.ptr(w), N.ptr(w), N.ptr(y), 8, D, 1e-6, N.stream()) == -1, D
    torch.cuda.synchronize()
    assert _untouched(y)


# (B, C, H, P, Kpad): the row-staged kernel (P^2 % 4 == 0) with and without pad columns, and the elementwise one (P = 7)
@pytest.mark.parametrize("B,C,H,P,Kpad", [(2, 3, 70, 14, 640), (2, 3, 224, 8, 192), (2, 3, 64, 16, 832), (2, 3, 28, 7, 192)])
@pytest.mark.parametrize("half", ["f16", "bf16"])
def test_patch_im2col_is_unfold_rounded_to_the_operand_type(half, B, C, H, P, Kpad):
    lib = N.load(half)
    img = torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(H + P))
    n, K = (H // P) ** 2, C * P * P
    imgd = img.to(DEV)
    buf = _guarded(B * n, Kpad, DT[half], guard=4)
    assert lib.ucod_patch_im2col(N.ptr(imgd), N.ptr(buf), B, C, H, H, P, Kpad, N.stream()) == 0
    torch.cuda.synchronize()
    ref = torch.nn.functional.unfold(img, P, stride=P).transpose(1, 2).reshape(B * n, K).to(DT[half])
    got = buf[:B * n].cpu()
    assert torch.equal(got[:, :K].view(torch.int16), ref.view(torch.int16))
    assert bool((got[:, K:].view(torch.int16) == 0).all()) and _untouched(buf[B * n:])


@pytest.mark.parametrize("B,tok,D", [(3, 26, 384), (2, 5, 1024), (5, 1370, 768)])
def test_cls_rows_are_cls_plus_pos0_and_nothing_else(B, tok, D):
    lib = N.load("f16")
    g = torch.Generator().manual_seed(B + D)
    cls, pos = torch.randn(D, generator=g), torch.randn(tok, D, generator=g) * 0.5
    cd, pd = cls.to(DEV), pos.to(DEV)
    want = cls + pos[0]                                          # one f32 add; the fp16 stream takes its round-to-nearest-even
    x32, x16 = _guarded(B * tok, D, torch.float32, guard=2), _guarded(B * tok, D, torch.float16, guard=2)
    assert lib.ucod_cls_rows(N.ptr(x32), N.ptr(cd), N.ptr(pd), B, tok, D, N.stream()) == 0
    assert lib.ucod_cls_rows_h16(N.ptr(x16), N.ptr(cd), N.ptr(pd), B, tok, D, N.stream()) == 0
    torch.cuda.synchronize()
    for x, w in ((x32.cpu(), want), (x16.cpu(), want.half())):
        rows = x[:B * tok].view(B, tok, D)
        assert torch.equal(rows[:, 0], w.expand(B, D))
        assert _untouched(rows[:, 1:]) and _untouched(x[B * tok:])


@pytest.mark.parametrize("B,tok,D", [(3, 26, 128), (2, 50, 768)])
def test_cls_qk_against_f64(B, tok, D):
    """q_cls, k_cls = the query / key projection of token 0 of every image (fp16 rows and weights, f32 sums): f64 on the same operands."""
    lib = N.load("f16")
    g = torch.Generator().manual_seed(tok + D)
    h = torch.randn(B * tok, D, generator=g).half()
    w = (torch.randn(3 * D, D, generator=g) * 0.05).half()
    b = torch.randn(3 * D, generator=g) * 0.1
    hd, wd, bd = h.to(DEV), w.to(DEV), b.to(DEV)
    q, k = _guarded(B, D, torch.float32, guard=1), _guarded(B, D, torch.float32, guard=1)
    assert lib.ucod_cls_qk(N.ptr(hd), N.ptr(wd), N.ptr(bd), N.ptr(q), N.ptr(k), B, tok, D, N.stream()) == 0
    torch.cuda.synchronize()
    ref = h.view(B, tok, D)[:, 0].double() @ w[:2 * D].double().t() + b[:2 * D].double()
    for tag, got, r in (("q", q, ref[:, :D]), ("k", k, ref[:, D:])):
        assert _untouched(got[B:])
        err = (got[:B].cpu().double() - r).abs()
        within(f"f16_kernels cls_qk {tag} {B}x{tok}x{D}", float((err / (4e-5 * (1 + r.abs()))).max()), 1.0)
