"""GPU: DINOv2 with registers (HF Dinov2WithRegistersModel) on every backbone engine -- an image's tokens are [CLS | R registers | n patches].

1  the two row-mapped GEMM drains (patch embedding, key hook) at R in {1, 4} on every tile path of both libraries: values against the f64 product of the same
   rounded operands under the tolerances of the existing R = 0 cases (tests/test_gpu_kernels.py, tests/test_gpu_f16_kernels.py), and as CONDITIONS: the patch GEMM
   leaves the CLS and register rows' bytes alone, the key drain writes every element of [B, C, n] and nothing else, guard bands in front and behind stay;
2  the leading-row kernels (CLS + register rows) bit for bit, their row partials under tests/test_gpu_lnfold.py's bounds;
3  every engine precision against the G21 goldens (transformers' own outputs; tests/golden/make_golden_registers.py) under the bound the G8 DINOv2 test of the same
   engine uses, a D = 256 model for the LayerNorm fold, batch / stream independence;
4  the CLS attention row (softmax over all 1 + R + n keys, patch columns returned);
5  backbone-backward (LoRA) mode against f64 autograd through tests/registers_ref.py, merge paths;
6  the public surface: backbone.random_init("dinov2_vits14_reg"), with_precision, PseudoLabelGenerator.

Measured on an MI355X (conftest.within leaves every bounded figure in its tolerance audit file): G21 key relative L2 -- split2 5.4 - 5.7e-6 (bound 3e-5), split3 6.0 - 6.4e-7
(3e-6), split2h = split2hf 5.1 - 5.5e-7 (3e-6); the folded D = 256 engine 5.0e-4 (unfolded 5.0e-4; bound 1.5e-3); CLS row 2.0 - 2.2e-5 (16-bit engine, bound 2e-2) and
6.5 - 9.9e-8 (three terms, 2e-5), row sums within 2.3e-6 / 1.8e-7 of the golden's; LoRA key max-abs 2.7 - 3.5e-3 (bar 3e-2 |key|max), worst gradient 1.0 - 1.7e-2
(bar 4e-2, 5e-2 with dropout); merged three-term engine 4.8e-7 from the f64 LoRA forward (unmerged 3.0e-2); dinov2_vits14_reg default vs f32eq 5.4 - 5.5e-4 (1.5e-3).
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import within, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, ViTLoRAEngine  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import backbone  # noqa: E402
import registers_ref as RR  # noqa: E402

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
H = 2.0 ** -11                                                  # half an ulp of fp16, relative
SENT = -5.0                                                     # guard / prefill value (exact in every type used here)
GUARD = 4096                                                    # elements in front of and behind every output
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Banded:
    """``numel`` elements of ``dtype`` prefilled with ``fill`` between two guard bands of SENT."""

    def __init__(self, numel, dtype, fill=SENT):
        self.numel = numel
        self.buf = torch.full((numel + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.payload = self.buf[GUARD:GUARD + numel]
        self.payload.fill_(fill)

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.numel:] == SENT).all())


# ================================================================================================ 1. row-mapped drains
GRIDS = [(5, 5), (4, 6)]                                        # n = 25 (odd) and 24 (even)
B_DRAIN, K_DRAIN = 9, 128                                       # 9 images: 225 / 216 patch rows, 270 / 261 (R = 4) token columns -- past a 256-wide tile


@functools.lru_cache(maxsize=None)
def patch_case(half, n, D):
    """operands rounded to the library's type and the f64 reference [B, n, D] = (A W^T + b) + pos[1 + p]  (never modified)"""
    g = torch.Generator().manual_seed(100 * n + D)
    A = (torch.randn(B_DRAIN * n, K_DRAIN, generator=g) * 0.5).to(DT[half])
    W = (torch.randn(D, K_DRAIN, generator=g) * 0.05).to(DT[half])
    b, pos = torch.randn(D, generator=g), torch.randn(n + 1, D, generator=g)
    ref = (A.double() @ W.double().t() + b.double()).view(B_DRAIN, n, D) + pos[1:].double()
    return A.to(DEV), W.to(DEV), b.to(DEV), pos.to(DEV), ref


def check_values(name, half, h16, got, ref):
    """bf16 library: tests/test_gpu_kernels.py::test_patch_token_epilogues_on_the_large_tile_kernel / test_key_hook_epilogue_on_the_large_tile_kernel;
    fp16 library: _bound16 / _bound32 of tests/test_gpu_f16_kernels.py (K <= 1536)."""
    ref = ref.double()
    err = (got.double() - ref).abs()
    if half == "bf16":
        within(name, float(err.max()), (2e-2 if h16 else 2e-3) * max(1.0, float(ref.abs().max())))
    elif h16:
        within(name, float((err / (H * ref.abs() + 4e-5 * (1 + ref.abs()))).max()), 1.0)
    else:
        within(name + " elementwise", float((err / (4e-5 * (1 + ref.abs()))).max()), 1.0)
        within(name + " rel_l2", rel_l2(got, ref), 1e-5)


@pytest.mark.parametrize("variant", [0, 9, 10, 2])
@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("gh,gw", GRIDS)
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_patch_drain_with_registers(half, R, gh, gw, D, h16, variant):
    lib = N.load(half)
    n = gh * gw
    tok = 1 + R + n
    A, W, b, pos, ref = patch_case(half, n, D)
    out = Banded(B_DRAIN * tok * D, torch.float16 if h16 else torch.float32)
    rc = lib.ucod_gemm_bf16_reg(N.EPI_PATCH_TOKENS_H16 if h16 else N.EPI_PATCH_TOKENS_F32, N.ptr(A), N.ptr(W), out.ptr(), B_DRAIN * n, D, K_DRAIN, N.ptr(b), None, None,
                                N.ptr(pos), tok, R, variant, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside the token rows"
    rows = out.payload.view(B_DRAIN, tok, D).cpu()
    assert bool((rows[:, :1 + R] == SENT).all()), "the patch GEMM wrote a CLS or register row"
    check_values(f"registers patch {half} R={R} {gh}x{gw} D={D} {'h16' if h16 else 'f32'} v{variant}", half, h16, rows[:, 1 + R:], ref)


@functools.lru_cache(maxsize=None)
def key_case(half, B, tok, C):
    g = torch.Generator().manual_seed(41 + tok + C + B)
    Wk = (torch.randn(C, K_DRAIN, generator=g) * 0.1).to(DT[half])
    x = torch.randn(B * tok, K_DRAIN, generator=g).to(DT[half])
    bias = torch.randn(C, generator=g)
    full = (x.double() @ Wk.double().t() + bias.double()).view(B, tok, C)          # every token; the caller drops 1 + R of them
    return Wk.to(DEV), x.to(DEV), bias.to(DEV), full


@pytest.mark.parametrize("variant", [0, 9, 10, 2])
@pytest.mark.parametrize("C", [128, 384])
@pytest.mark.parametrize("gh,gw", GRIDS)
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("B", [B_DRAIN, 12])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_key_drain_with_registers(half, B, R, gh, gw, C, variant):
    """B = 9: 243 / 234 / 270 / 261 token columns, none a multiple of 4 -- the forced large-tile variants (9 / 10) need N % 4 == 0 (include/ucod_dpl.h: 16-byte row
    stores) and must REFUSE these without writing a byte; auto and the 128 x 128 kernel take them.  B = 12 (324 / 312 / 360 / 348 columns, still past a 256-wide
    tile, images straddling 4-token groups and the tile edge) is what runs the large-tile drains, the 256-wide offset-scheme one included."""
    lib = N.load(half)
    n = gh * gw
    tok = 1 + R + n
    Wk, x, bias, full = key_case(half, B, tok, C)
    out = Banded(B * C * n, torch.float32, fill=float("nan"))
    rc = lib.ucod_gemm_bf16_reg(N.EPI_KEY_NCHW_F32, N.ptr(Wk), N.ptr(x), out.ptr(), C, B * tok, K_DRAIN, N.ptr(bias), None, None, None, tok, R, variant, N.stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside [B, C, n]"
    if variant in (9, 10) and (B * tok) % 4 != 0:
        assert rc == -1, rc
        assert bool(torch.isnan(out.payload).all()), "a refused launch wrote to its output"
        return
    assert rc == 0, rc
    got = out.payload.view(B, C, n).cpu()
    assert bool(torch.isfinite(got).all()), "left elements of [B, C, n] unwritten"
    check_values(f"registers key {half} B={B} R={R} {gh}x{gw} C={C} v{variant}", half, False, got, full[:, 1 + R:].transpose(1, 2))


def test_register_entry_points_are_the_plain_ones_at_zero_and_refuse_nonsense():
    lib = N.load("f16")
    n, D = 25, 128
    A, W, b, pos, _ = patch_case("f16", n, D)
    a0, a1 = Banded(B_DRAIN * 26 * D, torch.float32), Banded(B_DRAIN * 26 * D, torch.float32)
    assert lib.ucod_gemm_bf16(N.EPI_PATCH_TOKENS_F32, N.ptr(A), N.ptr(W), a0.ptr(), B_DRAIN * n, D, K_DRAIN, N.ptr(b), None, None, N.ptr(pos), 26, 0, N.stream()) == 0
    assert lib.ucod_gemm_bf16_reg(N.EPI_PATCH_TOKENS_F32, N.ptr(A), N.ptr(W), a1.ptr(), B_DRAIN * n, D, K_DRAIN, N.ptr(b), None, None, N.ptr(pos), 26, 0, 0, N.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a0.buf, a1.buf)
    before = a1.buf.clone()
    call = lambda epi, tok, R: lib.ucod_gemm_bf16_reg(epi, N.ptr(A), N.ptr(W), a1.ptr(), B_DRAIN * n, D, K_DRAIN, N.ptr(b), None, None, N.ptr(pos), tok, R, 0, N.stream())  # noqa: E731
    assert call(N.EPI_PATCH_TOKENS_F32, 26, -1) == -1 and call(N.EPI_PATCH_TOKENS_F32, 5, 4) == -1          # negative R; no patch token left
    assert call(N.EPI_BIAS_F32, 26, 4) == -1                                                                   # an epilogue without a row map takes R = 0 only
    x = torch.zeros(4, D, device=DEV)
    assert lib.ucod_cls_rows_reg(N.ptr(x), N.ptr(b), N.ptr(pos), 2, 2, D, 2, N.stream()) == -1                 # R rows do not fit tok
    assert lib.ucod_cls_attention_reg(N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x), 1, 2, 1, -1, 0.125, N.stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(a1.buf, before)


# ================================================================================================ 2. leading rows
@pytest.mark.parametrize("B,n,D,R", [(3, 25, 384, 4), (2, 4, 1024, 1), (5, 24, 128, 4), (2, 7, 256, 0)])
def test_leading_rows_are_cls_plus_pos0_then_the_registers(B, n, D, R):
    lib = N.load("f16")
    g = torch.Generator().manual_seed(B + D + R)
    tok = 1 + R + n
    lead, pos = torch.randn(1 + R, D, generator=g), torch.randn(n + 1, D, generator=g) * 0.5
    want = lead.clone()
    want[0] = lead[0] + pos[0]                                   # one f32 add; register rows as they are; the fp16 stream takes round-to-nearest-even
    ld, pd = lead.to(DEV), pos.to(DEV)
    x32, x16, xs = Banded(B * tok * D, torch.float32), Banded(B * tok * D, torch.float16), Banded(B * tok * D, torch.float16)
    part = Banded(B * tok * (D // 64) * 2, torch.float32)
    assert lib.ucod_cls_rows_reg(x32.ptr(), N.ptr(ld), N.ptr(pd), B, tok, D, R, N.stream()) == 0
    assert lib.ucod_cls_rows_h16_reg(x16.ptr(), N.ptr(ld), N.ptr(pd), B, tok, D, R, N.stream()) == 0
    assert lib.ucod_cls_rows_h16_stats_reg(xs.ptr(), N.ptr(ld), N.ptr(pd), part.ptr(), D // 64, B, tok, D, R, N.stream()) == 0
    torch.cuda.synchronize()
    for x, w in ((x32, want), (x16, want.half()), (xs, want.half())):
        assert x.guards_intact()
        rows = x.payload.view(B, tok, D).cpu()
        assert torch.equal(rows[:, :1 + R], w.expand(B, 1 + R, D))
        assert bool((rows[:, 1 + R:] == SENT).all()), "a patch row was written"
    assert part.guards_intact()
    p = part.payload.view(B, tok, D // 64, 2).cpu()
    assert bool((p[:, 1 + R:] == SENT).all())
    # Chan's merge of the (S, M2) slots of every leading row against the row's own statistics: the bounds of tests/test_gpu_lnfold.py
    S, M2 = p[:, :1 + R, :, 0].double().reshape(-1, D // 64), p[:, :1 + R, :, 1].double().reshape(-1, D // 64)
    mean = S.sum(1) / D
    var = (M2.sum(1) + 64 * ((S / 64 - mean[:, None]) ** 2).sum(1)) / D
    xr = want.half().double().repeat(B, 1)
    assert bool(((mean - xr.mean(1)).abs() <= 1e-6 * xr.abs().mean(1) + 1e-6).all())
    assert bool(((var - xr.var(1, unbiased=False)).abs() <= 2e-6 * xr.var(1, unbiased=False) + 1e-7).all())


@pytest.mark.parametrize("R", [1, 4])
def test_patch_embedding_with_row_partials_and_registers(R):
    """UCOD_EPI_PATCH_TOKENS_H16_STATS at R in {1, 4} on the large-tile kernel (9 images of 256 patches = 2304 rows): the token rows against the plain epilogue's as
    tests/test_gpu_lnfold.py compares them at R = 0, the CLS / register rows and their partials untouched by the GEMM, every patch row's partials merging to its
    mean and variance."""
    lib = N.load("f16")
    B, n, D, K = 9, 256, 256, 128
    tok = 1 + R + n
    g = torch.Generator().manual_seed(77)
    a = (torch.randn(B * n, K, generator=g) * 0.5).half().to(DEV)
    w = (torch.randn(D, K, generator=g) * 0.05).half().to(DEV)
    b, pos = (torch.randn(D, generator=g) * 0.1).to(DEV), (torch.randn(n + 1, D, generator=g) * 0.5).to(DEV)
    plain, out = Banded(B * tok * D, torch.float16), Banded(B * tok * D, torch.float16)
    part = Banded(B * tok * (D // 64) * 2, torch.float32)
    assert lib.ucod_gemm_bf16_reg(N.EPI_PATCH_TOKENS_H16, N.ptr(a), N.ptr(w), plain.ptr(), B * n, D, K, N.ptr(b), None, None, N.ptr(pos), tok, R, 9, N.stream()) == 0
    rc = lib.ucod_gemm_bf16_stats_reg(N.EPI_PATCH_TOKENS_H16_STATS, N.ptr(a), N.ptr(w), out.ptr(), B * n, D, K, N.ptr(b), None, None, N.ptr(pos), tok, R, part.ptr(), D // 64,
                                      N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert plain.guards_intact() and out.guards_intact() and part.guards_intact()
    o, pl = out.payload.view(B, tok, D), plain.payload.view(B, tok, D)
    assert bool((o[:, :1 + R] == SENT).all()) and bool((pl[:, :1 + R] == SENT).all())
    differs = (o != pl)
    assert float(differs.float().mean()) < 2e-3 and maxdiff(o.float().cpu(), pl.float().cpu()) <= 2.0 ** -9 * max(1.0, float(pl[:, 1 + R:].float().abs().max()))
    p = part.payload.view(B, tok, D // 64, 2)
    assert bool((p[:, :1 + R] == SENT).all()), "the GEMM wrote a leading row's partials"
    pp = p[:, 1 + R:].reshape(-1, D // 64, 2).cpu().double()
    assert bool(torch.isfinite(pp).all())
    xs = o[:, 1 + R:].reshape(-1, D).double().cpu()
    mean = pp[:, :, 0].sum(1) / D
    var = (pp[:, :, 1].sum(1) + 64 * ((pp[:, :, 0] / 64 - mean[:, None]) ** 2).sum(1)) / D
    assert bool(((mean - xs.mean(1)).abs() <= 1e-6 * xs.abs().mean(1) + 1e-6).all())
    assert bool(((var - xs.var(1, unbiased=False)).abs() <= 2e-6 * xs.var(1, unbiased=False) + 1e-7).all())


# ================================================================================================ 3. engines against G21
@functools.lru_cache(maxsize=None)
def g21(tag):
    z = np.load(os.path.join(GOLDEN, f"g21_dinov2_registers_{tag}.npz"))
    sd = RR.g21_state_dict(tag)                                  # (its weights: tests/test_registers_host.py checks their hash, as for G20 -- the draw goes through the host's
                                                                 # vectorised erfinv, which may differ in the last bit on another CPU: far below every bound here)
    return sd, torch.from_numpy(z["x"]), torch.from_numpy(z["key"]), torch.from_numpy(z["cls_att"])


def make_engine(precision, sd, heads):
    kw = dict(heads=heads, eps=1e-6, device=DEV)
    if precision == "f16":
        return ViTEngine(sd, **kw)
    if precision == "bf16":
        return ViTEngine(sd, half="bf16", **kw)
    if precision == "f16_resid32":
        return ViTEngine(sd, resid="f32", **kw)
    if precision in ("split2", "split3"):
        return SplitViTEngine(sd, terms=int(precision[-1]), **kw)
    return SplitViTEngine(sd, terms=2, term="f16", fuse_mlp=precision == "split2hf", **kw)


# the bound of the G8 DINOv2 test of the same engine (same width, same depth): tests/test_gpu_kernels.py (fp16 operands 1e-3; bf16 6e-3 and 0.1 max-abs),
# tests/test_gpu_split.py (3e-5 / 3e-6), tests/test_gpu_split16.py and tests/test_gpu_split16_fused.py (3e-6, and the relations to the three-term engine)
G8_BOUND = {"f16": 1e-3, "bf16": 6e-3, "f16_resid32": 1e-3, "split2": 3e-5, "split3": 3e-6, "split2h": 3e-6, "split2hf": 3e-6}


@pytest.mark.parametrize("tag", sorted(RR.G21))
@pytest.mark.parametrize("precision", list(G8_BOUND))
def test_engines_against_the_g21_goldens(precision, tag):
    sd, x, key_ref, _ = g21(tag)
    eng = make_engine(precision, sd, RR.G21_HEADS)
    assert eng.R == RR.G21[tag][2]
    key = eng(x.to(DEV)).cpu()
    eng.check_overflow(wait=True)
    assert key.shape == key_ref.shape
    err = rel_l2(key, key_ref)
    print(f"g21 {tag} {precision}: key rel-L2 {err:.3e} (bound {G8_BOUND[precision]:.0e})")
    within(f"g21:{tag}:{precision}", err, G8_BOUND[precision])
    if precision == "bf16":
        assert maxdiff(key, key_ref) < 0.1 * key_ref.abs().max().item()
    if precision in ("split2h", "split2hf"):
        e3 = rel_l2(make_engine("split3", sd, RR.G21_HEADS)(x.to(DEV)), key_ref)
        assert err <= 4.0 * e3 + 1e-7, (err, e3)                 # tests/test_gpu_split16.py: relation()
        if precision == "split2hf":
            eu = rel_l2(make_engine("split2h", sd, RR.G21_HEADS)(x.to(DEV)), key_ref)
            assert err <= 1.25 * eu + 1e-7, (err, eu)            # tests/test_gpu_split16_fused.py: fused_bounds()


@functools.lru_cache(maxsize=None)
def fold_case():
    """D = 256, 4 heads, 2 layers, R = 4, a 5 x 5 grid on its own checkpoint grid; f64 key map and CLS row through registers_ref."""
    sd = RR.random_registers_state_dict(256, 4, 2, 4, image_size=70, seed=256)
    x = torch.randn(5, 3, 70, 70, generator=torch.Generator().manual_seed(9))
    key, att = RR.forward_f64(x, sd, 4, device=DEV)
    return sd, x, key, att


def test_folded_engine_with_registers():
    """tests/test_gpu_lnfold.py's bound for the folded fp16 engine at this width (1.5e-3, and no farther than 1.25 x the unfolded engine + 1e-4)."""
    sd, x, ref, _ = fold_case()
    fold = ViTEngine(sd, heads=4, device=DEV)
    plain = ViTEngine(sd, heads=4, device=DEV, half="f16", resid="f16", ln_fold=False)
    assert fold.ln_fold and fold.R == 4 and not plain.ln_fold and fold._desc(5, 70, 70).n_reg == 4
    kf, kp = fold(x.to(DEV)).cpu(), plain(x.to(DEV)).cpu()
    fold.check_overflow(wait=True)
    df, dp = rel_l2(kf, ref), rel_l2(kp, ref)
    print(f"folded registers engine: {df:.3e} (unfolded {dp:.3e})")
    assert df < 1.5e-3 and df <= 1.25 * dp + 1e-4, (df, dp)


@pytest.mark.parametrize("precision", ["f16", "bf16", "f16_resid32", "split2", "split3", "split2h", "split2hf", "fold256"])
def test_key_map_does_not_depend_on_the_batch_or_the_streams(precision):
    """B = 5: image 0 alone against image 0 inside the batch, and one stream against two.  The stream count never changes a bit (same kernels per image: torch.equal,
    as tests/test_gpu_kernels.py demands); the batch changes tile shapes, i.e. the f32 summation order: the existing bounds (16-bit engines: tests/test_gpu_lnfold.py
    1e-3; three-term and fp16-term split engines: 5e-6, tests/test_gpu_split.py / test_gpu_split16.py / test_gpu_split16_fused.py).  The two-term bf16 engine has no
    such test yet: an f32 value that moved by one ulp can round to the neighbouring 16-bit pair of terms, 2^-16 = 1.5e-5 of it away, so its bound is the level of its own
    operand rounding, 3e-5 (what tests/test_gpu_split.py allows the engine against G8) -- the reasoning behind the bf16 engine's 8e-3 above."""
    if precision == "fold256":
        sd, x, _, _ = fold_case()
        eng = ViTEngine(sd, heads=4, device=DEV)
    else:
        sd, x3, _, _ = g21("down")
        x = torch.cat((x3, torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(5))), 0)
        eng = make_engine(precision, sd, RR.G21_HEADS)
    x = x.to(DEV)
    k5 = eng(x).clone()
    k1 = eng(x[:1].contiguous()).clone()
    bound = 3e-5 if precision == "split2" else 5e-6 if precision.startswith("split") else (8e-3 if precision == "bf16" else 1e-3)
    assert rel_l2(k1, k5[:1]) < bound, rel_l2(k1, k5[:1])
    if isinstance(eng, ViTEngine):
        eng.streams = 2
        k2 = eng(x).clone()
        # the two-stream pass runs images 0-1 and 2-4 as sub-batches: each equals the single-stream pass over the same sub-batch, bit for bit
        eng.streams = 1
        assert torch.equal(k2[:2], eng(x[:2].contiguous())) and torch.equal(k2[2:], eng(x[2:].contiguous()))
    eng.check_overflow(wait=True)


# ================================================================================================ 4. CLS attention row
@pytest.mark.parametrize("tag", ["native", "down", "nonsquare", "r1"])
@pytest.mark.parametrize("engine", ["vit", "split3"])
def test_cls_attention_row_counts_the_register_keys(engine, tag):
    """G14's bounds (tests/test_gpu_pseudo_label.py): 2e-2 relative L2 for the 16-bit engine, 2e-5 for the three-term one; row sums against the golden's within the
    2e-3 / 1e-5 those tests allow the sum with the CLS column.  A softmax that left the register keys out of the denominator sums too high (checked below)."""
    sd, x, key_ref, att_ref = g21(tag)
    R = RR.G21[tag][2]
    eng = ViTEngine(sd, heads=2, device=DEV, attn_variant=2) if engine == "vit" else SplitViTEngine(sd, heads=2, device=DEV, terms=3)
    key, att = eng.forward_with_cls_attention(x.to(DEV))
    assert att.shape == att_ref.shape and key.shape == key_ref.shape
    e_att, e_sum = rel_l2(att, att_ref), maxdiff(att.sum(-1).cpu(), att_ref.sum(-1))
    print(f"cls row {engine} {tag}: rel-L2 {e_att:.3e}, row sums {e_sum:.3e}")
    assert e_att < (2e-2 if engine == "vit" else 2e-5), e_att
    assert e_sum < (2e-3 if engine == "vit" else 1e-5), e_sum
    assert rel_l2(key, key_ref) < (1e-3 if engine == "vit" else 5e-6)
    # teeth: the same row renormalised without the register keys misses the row-sum bound
    _, att_all = RR.forward_f64(x, sd, 2)
    reg_mass = 1.0 - att_all.sum(-1)                              # CLS + register columns
    assert float(reg_mass.min()) > 0.0
    if R == 4:
        assert float(reg_mass.max()) > 50 * (2e-3 if engine == "vit" else 1e-5)


# ================================================================================================ 5. LoRA
def lora_engine(sd, targets, gen_seed=3, **kw):
    """B = 0.05 randn on the targeted modules (tests/test_gpu_lora_targets.py: peft's B = 0 would make the LoRA branch vanish)."""
    gen = torch.Generator().manual_seed(gen_seed)
    eng = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, device=DEV, generator=gen, target_modules=targets, **kw)
    lsd = eng.lora_state_dict()
    for k in sorted(lsd):
        if "lora_B" in k:
            lsd[k] = 0.05 * torch.randn(lsd[k].shape, generator=gen)
    eng.load_lora_state_dict(lsd)
    return eng


TARGET_SETS = {"default": None, "qv_fc1": ["query", "value", "fc1"]}


@functools.lru_cache(maxsize=None)
def lora_case(tset, p_drop):
    sd = RR.g21_state_dict("native")
    eng = lora_engine(sd, TARGET_SETS[tset], lora_dropout=p_drop, seed=1234)
    gen = torch.Generator().manual_seed(7)
    img, dkey = torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen)
    return sd, img, dkey, {k: v.cpu() for k, v in eng.lora_state_dict().items()}


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tset", list(TARGET_SETS))
def test_lora_passes_with_registers_vs_f64_autograd(tset, p_drop, streams):
    """The bars tests/test_gpu_lora_targets.py applies at D = 128: key max-abs 3e-2 max(1, |key|max), every non-zero gradient 4e-2 relative L2 (5e-2 with dropout, its
    test 6), structurally zero gradients exactly zero.  Dropout masks are restated per chunk (oracle.vit.lora_dropout_mask over the chunk's B (1 + R + n) rows)."""
    from oracle import vit as OV
    sd, img, dkey, lsd = lora_case(tset, p_drop)
    L, D, tok = 3, 128, 1 + 4 + 25
    eng = lora_engine(sd, TARGET_SETS[tset], lora_dropout=p_drop, seed=1234)
    eng.train_streams = streams
    assert eng.R == 4 and {k: 0 for k in eng.lora_state_dict()}.keys() == lsd.keys()
    key = eng.forward_train(img.to(DEV))
    bounds, seeds = list(eng._bounds), list(eng._chunk_seed)
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    got = eng.lora_state_dict(grads=True)
    key_ref, gref = [], None
    for (b0, b1), seed in zip(bounds, seeds):                    # the reference chunk by chunk: each chunk has its own masks; gradients add
        masks = None
        if p_drop > 0:
            rows = (b1 - b0) * tok
            masks = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(("query", "key", "value"))}
            masks.update({(i, "fc1"): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
        k, g = RR.lora_grads(img[b0:b1], {**sd, **lsd}, 2, dkey[b0:b1], eng.scaling, masks=masks, device=DEV)
        key_ref.append(k.cpu())
        gref = {n: v.cpu() for n, v in g.items()} if gref is None else {n: gref[n] + v.cpu() for n, v in g.items()}
    key_ref = torch.cat(key_ref, 0)
    assert sorted(got) == sorted(gref)
    key_err = maxdiff(key.cpu(), key_ref)
    bar = 4e-2 if p_drop == 0 else 5e-2
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=errs.get)
    print(f"registers LoRA {tset} p={p_drop} streams={streams}: key {key_err:.2e}, worst gradient {errs[worst]:.2e} ({worst})")
    assert key_err < 3e-2 * max(1.0, key_ref.abs().max().item()), key_err
    for k, ref in gref.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    assert len(errs) > 0 and all(e < bar for e in errs.values()), (worst, errs[worst])
    # two backward runs are bit-identical
    eng2 = lora_engine(sd, TARGET_SETS[tset], lora_dropout=p_drop, seed=1234)
    eng2.train_streams = streams
    eng2.forward_train(img.to(DEV))
    g2 = eng2.backward(dkey.to(DEV))
    assert torch.equal(g2, eng.lora_grad)


def test_lora_nograd_ema_clone_and_merges_with_registers():
    sd, img, dkey, lsd = lora_case("qv_fc1", 0.0)
    eng = lora_engine(sd, TARGET_SETS["qv_fc1"])
    x = img.to(DEV)
    k_train = eng.forward_train(x).clone()
    k_f16, k_f32 = eng.forward_nograd(x, resid16=True).clone(), eng.forward_nograd(x, resid16=False).clone()
    eng.check_overflow(wait=True)
    assert rel_l2(k_f32, k_train) < 2e-3 and rel_l2(k_f16, k_train) < 4e-3        # tests/test_gpu_lora_targets.py test 6
    ema = eng.clone_for_ema()
    assert ema.R == 4 and torch.equal(ema.forward_nograd(x, resid16=False), k_f32)
    # merged_state_dict -> SplitViTEngine(terms=3): the f64 LoRA forward, within the merge test's bound, registers still there
    merged = eng.merged_state_dict()
    assert torch.equal(merged["embeddings.register_tokens"], sd["embeddings.register_tokens"]) and not any(".lora_" in k for k in merged)
    ref, _ = RR.lora_grads(img, {**sd, **lsd}, 2, dkey, eng.scaling, device=DEV)
    e3 = SplitViTEngine(merged, heads=2, device=DEV, terms=3)
    assert e3.R == 4
    e_merged, e_base = rel_l2(e3(x), ref), rel_l2(SplitViTEngine(sd, heads=2, device=DEV, terms=3)(x), ref)
    print(f"merged registers engine: {e_merged:.2e} (unmerged {e_base:.2e})")
    assert e_merged < 3e-6 and e_base > 100 * 3e-6                 # SPLIT3_G8_BAR of tests/test_gpu_lora_merge.py
    # merge_into a live default engine == rebuilding it (D = 128: no fold; the plain tables tensor for tensor)
    vit = ViTEngine(sd, heads=2, device=DEV)
    ptrs = [t.data_ptr() for row in vit.layers for t in row if t is not None]
    assert eng.merge_into(vit) is vit
    fresh = ViTEngine(merged, heads=2, device=DEV)
    for ra, rb in zip(vit.layers, fresh.layers):
        for a, b in zip(ra, rb):
            assert (a is None and b is None) or torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b)
    assert ptrs == [t.data_ptr() for row in vit.layers for t in row if t is not None]
    assert torch.equal(vit(x), fresh(x)) and torch.equal(vit.cls, fresh.cls)
    # an engine with another R is refused
    other = {k: v for k, v in sd.items() if "register_tokens" not in k}
    with pytest.raises(ValueError, match="register"):
        eng.merge_into(ViTEngine(other, heads=2, device=DEV))
    with pytest.raises(ValueError, match="register"):
        eng.merge_into(ViTEngine(RR.g21_state_dict("r1"), heads=2, device=DEV))


# ================================================================================================ 6. drop-in
def test_drop_in_backbone_and_pseudo_label_generator():
    from ucod_dpl_amd.generate_pseudo_label import PseudoLabelGenerator
    bb = backbone.random_init("dinov2_vits14_reg", image_size=224, device=DEV)
    assert isinstance(bb.engine, ViTEngine) and bb.engine.R == 4 and bb.engine._pos_antialias and not bb.engine.ln_fold and not bb.engine.resid16
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    _, key = bb(x)
    assert tuple(key.shape) == (2, 384, 16, 16) and bool(torch.isfinite(key).all())
    # the bound of the same configuration -- fp16 operands on the f32 stream, which is what "auto" gives ViT-S (D % 256 != 0: no fold) -- at this depth:
    # tests/test_gpu_parity_c2.py::test_c2_full_size_logits_against_the_oracle ("f16", "f32"): key 1.5e-3 relative L2 from the f32 reference
    eq = bb.with_precision("f32eq")
    assert isinstance(eq.engine, SplitViTEngine) and eq.engine.R == 4
    e = rel_l2(key, eq(x)[1])
    print(f"dinov2_vits14_reg @224 (own grid) default vs f32eq: {e:.3e}")
    assert e < 1.5e-3, e
    # the checkpoint as published -- a 37 x 37 position grid (518 px) -- run at 224 px: the antialiased downsampling to 16 x 16, the pseudo-label generator's geometry
    bb518 = backbone.random_init("dinov2_vits14_reg", device=DEV)
    assert tuple(bb518.engine._pos_src.shape) == (1, 1 + 37 * 37, 384)
    _, key518 = bb518(x)
    assert tuple(key518.shape) == (2, 384, 16, 16)
    e518 = rel_l2(key518, bb518.with_precision("f32eq")(x)[1])
    print(f"dinov2_vits14_reg @224 (37 x 37 grid downsampled) default vs f32eq: {e518:.3e}")
    assert e518 < 1.5e-3, e518
    pos = bb518.engine._pos(16, 16).cpu()
    assert torch.equal(pos, RR.pos_embed(bb518.engine._pos_src, 16, 16, True)[0]) and not torch.equal(pos, RR.pos_embed(bb518.engine._pos_src, 16, 16, False)[0])
    # the generator end to end at G14's tiny geometry (3 x 112 x 112 -> 8 x 8 patches)
    sd = RR.random_registers_state_dict(128, 2, 2, 4, image_size=112, seed=14)
    gen = PseudoLabelGenerator(backbone.from_state_dict(sd, heads=2, device=DEV), th_bkg=0.6)
    assert isinstance(gen.engine, SplitViTEngine) and gen.engine.R == 4
    imgs = torch.randn(3, 3, 112, 112, generator=torch.Generator().manual_seed(4))
    raw = gen.raw_masks(imgs).cpu()
    assert tuple(raw.shape) == (3, 8, 8) and bool(((raw == 0) | (raw == 1)).all())
    masks = gen.generate_masks(imgs)
    assert len(masks) == 3 and all(tuple(m.shape)[-2:] == (8, 8) for m in masks)
