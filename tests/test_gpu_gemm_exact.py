"""GPU: the 16-bit MFMA GEMM (ucod_gemm_bf16 of both libraries: 64 x 64, 128 x 128, large-tile, leftover-as-patches and mixed-height kernels) and its linear
epilogues against an EXACT reference, bit for bit.  Operands are small integers (times a power of two) for which every partial sum in every order is an f32
number (tests/gemm_exact_ref.py asserts it per case; tests/test_gemm_exact_host.py shows it on the CPU), so every output bit is determined -- the rounding to
bf16 / fp16 included -- and a drain or tile-schedule change is judged by equality.  GELU outputs are held to the documented error of the kernel's fit plus
half an ulp of the output type.

Every case states the kernel it is meant to reach and asserts that gemm_exact_ref.plan() -- the mirror of launch() -- agrees on this device; every output
buffer has guard rows in front of and behind the written region; every launch is repeated into a second buffer and must give equal bits.
References are f64 products on the device, one per (family, shape), shared by every epilogue, variant and library: the file's ~730 cases take about 16 s on an MI355X.
"""
import functools
import os

import pytest
import torch

import gemm_exact_ref as X

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
F32, F16 = torch.float32, torch.float16
N_CU = torch.cuda.get_device_properties(0).multi_processor_count
SENT = -5.0                                                       # guard value (exact in every type used here)
GUARD = 8                                                         # guard rows on either side of the written region
_NEEDS_LAB = pytest.mark.skipif(not N.have_lab(), reason="laboratory library not built (make -C ucod_dpl_amd/csrc variants)")


def lab(*values):
    return pytest.param(*values, marks=[pytest.mark.variants, _NEEDS_LAB])


@pytest.fixture(autouse=True)
def _a_gpu_fault_ends_the_run():
    """A launch that faults leaves the device in an error state: nothing more is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, run ended: {e}", returncode=3)


# ================================================================================================ shapes, each with the path it must reach
T128 = [(128, 128, 64), (129, 132, 128), (1, 8, 64), (257, 260, 192), (200, 130, 192)]          # (200, 130): N % 4 != 0, the element-wise drain
T64 = [(64, 64, 64), (65, 72, 128), (130, 66, 192)]
BIG = [(256, 256, 64), (300, 264, 128), (513, 392, 192), (333, 128, 3072)]                       # one K tile (prologue only) | ragged both ways | 3 K tiles, 8-column last 192-wide tile | long K
P = X.Plan
# (M, N, K, variant, plan)
SMALL_CASES = ([(*s, v, P("t128", 0, 0)) for s in T128 for v in (1, 2)] + [(*s, v, P("t64", 0, 0)) for s in T64 for v in (12, 0)] +
               [(*s, 9, P("big256", 0, 0)) for s in BIG] + [(*s, 10, P("big192", 0, 0)) for s in BIG])
PATCH_CASES = ([(21916, 768, K, 9, P("big256+patches", 1, 0)) for K in (64, 192, 768, 2304, 5632)] +      # patch k-steps per wave: 0-or-1, 0-or-1, 3, 6+3, 12+6+3+1
               [(16401, 776, 128, 9, P("big256+patches", 2, 0)),                                          # last row tile 17 rows, last column tile 8 columns: dead patches
                (43840, 768, 128, 9, P("big256+patches", 1, 0)),                                          # two rounds
                (16401, 768, 128, 10, P("big192+patches", 2, 0)), (16401, 768, 768, 10, P("big192+patches", 2, 0))])
MIXED_CASES = [(21916, 768, 128, 13, P("mixed256", 0, 5)), (21916, 768, 192, 13, P("mixed256", 0, 5)), (16500, 776, 128, 13, P("mixed256", 0, 4)),
               (16500, 768, 192, 14, P("mixed192", 0, 4)), (43840, 2304, 128, 0, P("mixed256", 0, 10))]  # (6 rounds: auto picks 13 for the column-fused epilogues)
CASES = SMALL_CASES + PATCH_CASES + MIXED_CASES
# the fp16 residual stream: small passes on the 128 x 128 / 64 x 64 kernels, large ones always on the 256-wide mixed-height kernel (with or without tall tiles)
RESID16_CASES = ([c for c in SMALL_CASES if c[4].path in ("t128", "t64")] +
                 [(21916, 768, 128, 0, P("mixed256", 0, 5)), (21916, 768, 192, 0, P("mixed256", 0, 5)), (16500, 776, 128, 0, P("mixed256", 0, 4)),
                  (16401, 776, 128, 0, P("mixed256", 0, 1)), (43840, 768, 128, 0, P("mixed256", 0, 10)), (4111, 768, 128, 0, P("mixed256", 0, 0))])
WSCALE_CASES = [c for c in CASES if c[:4] in ((129, 132, 128, 2), (65, 72, 128, 12), (300, 264, 128, 9), (513, 392, 192, 10), (16401, 776, 128, 9),
                                              (16401, 768, 128, 10), (16500, 776, 128, 13), (16500, 768, 192, 14))]
FAM_SEED = {"f32": 1, "h16": 2, "resid16": 3, "gelu": 4, "wscale": 5}


def _id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-v{c[3]}-{c[4].path}"


@functools.lru_cache(maxsize=None)
def _case(fam, out_dtype, M, Nn, K):
    """One case per (family, output type, shape): generated once, reference on the device in f64, shared by every epilogue and variant, never modified."""
    return X.exact_case(M, Nn, K, seed=M + Nn + K + 1000 * FAM_SEED[fam], device=DEV, **X.family(fam, K, out_dtype))


@functools.lru_cache(maxsize=None)
def _dev(fam, out_dtype, M, Nn, K, half, what):
    c = _case(fam, out_dtype, M, Nn, K)
    if what == "AW":
        return c.operands(DT[half], DEV)
    t = getattr(c, what)
    t32 = t.float()
    assert bool((t32.double() == t).all())                        # (an f32 number: the kernel reads it as given)
    return t32.to(DEV)


# kind -> (epilogue, plan kind, family, reference, output type (None: the operand type), scale, residual, in place, bias)
KINDS = {
    "bias32": (N.EPI_BIAS_F32, "bias32", "f32", "bias", F32, False, False, False, True),
    "nobias32": (N.EPI_BIAS_F32, "bias32", "f32", "plain", F32, False, False, False, False),
    "bias16": (N.EPI_BIAS_BF16, "bias16", "h16", "bias", None, False, False, False, True),
    "scale16": (N.EPI_BIAS_BF16, "bias16", "h16", "scale", None, True, False, False, True),
    "resid32": (N.EPI_BIAS_SCALE_RESID_F32, "resid32", "f32", "resid", F32, True, True, False, True),
    "resid32_inplace": (N.EPI_BIAS_SCALE_RESID_F32, "resid32", "f32", "resid", F32, True, True, True, True),
    "resid16": (N.EPI_BIAS_SCALE_RESID_H16, "resid16", "resid16", "resid", F16, True, True, True, True),
    "wscale32": (N.EPI_BIAS_SCALE_RESID_F32, "resid32", "wscale", "resid", F32, True, True, False, True),
    "wscale16": (N.EPI_BIAS_BF16, "bias16", "wscale", "scale", None, True, False, False, True),
    "gelu16": (N.EPI_BIAS_GELU_BF16, "gelu16", "gelu", "bias", None, False, False, False, True),
}


def _guarded(rows, cols, dtype):
    buf = torch.full((GUARD + rows + GUARD, cols), SENT, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + rows:] == SENT).all())


def _run(half, kind, M, Nn, K, variant, want_plan, fn=None, plan_kw=None):
    epi, pkind, fam, refname, odt, use_scale, use_resid, in_place, has_bias = KINDS[kind]
    odt = odt or DT[half]
    plan = X.plan(pkind, M, Nn, K, variant, N_CU, has_bias=has_bias, **(plan_kw or {}))
    assert plan == want_plan, f"{kind} {M}x{Nn}x{K} v{variant} on {N_CU} CUs launches {plan}, the case is meant for {want_plan}"
    key = (fam, odt if fam in ("h16", "wscale") else None, M, Nn, K)       # (the other families do not depend on the output type)
    c = _case(*key)
    A, W = _dev(*key, half, "AW")
    bias = _dev(*key, half, "bias") if has_bias else None
    scale = _dev(*key, half, "scale") if use_scale else None
    resid = None
    if use_resid:
        resid = _dev(*key, half, "resid")
        if odt == F16:
            r16 = resid.to(F16)
            assert bool((r16.float() == resid).all())
            resid = r16
    fn = fn or N.load(half).ucod_gemm_bf16
    bufs = []
    for _ in range(2):                                             # the second launch must give equal bits
        buf, out = _guarded(M, Nn, odt)
        if in_place:
            out.copy_(resid)
        rc = fn(epi, N.ptr(A), N.ptr(W), out.data_ptr(), M, Nn, K, N.ptr(bias), N.ptr(scale), out.data_ptr() if in_place else N.ptr(resid), None, 0, variant,
                N.stream())
        assert rc == 0, rc
        bufs.append(buf)
    torch.cuda.synchronize()
    what = f"{half} {kind} {M}x{Nn}x{K} v{variant} ({want_plan.path})"
    assert _guards_intact(bufs[0], M) and _guards_intact(bufs[1], M), what + ": guard rows were written"
    assert torch.equal(bufs[0], bufs[1]), what + ": a second launch differs"
    out = bufs[0][GUARD:GUARD + M]
    if kind == "gelu16":
        X.check_gelu(out, c.ref(refname), odt, what)
    else:
        X.check_exact(out, c.ref(refname), odt, what)


# ================================================================================================ linear epilogues, bit for bit
def _takes_null_bias(c):
    """NULL bias (the plain product of the dgrad GEMMs): large-tile kernels only -- variant >= 9, or auto where it picks one -- and K >= 128."""
    return c[2] >= 128 and c[3] != 12 and (c[3] >= 9 or c[4].path.startswith("mixed"))


LINEAR = [(k, c) for c in CASES for k in ("bias32", "nobias32", "bias16", "scale16", "resid32", "resid32_inplace", "gelu16") if k != "nobias32" or _takes_null_bias(c)]


@pytest.mark.parametrize("kind,case", LINEAR, ids=[f"{k}-{_id(c)}" for k, c in LINEAR])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_gemm_epilogue_is_exact_on_every_tile_path(half, kind, case):
    """UCOD_EPI_BIAS_F32 (with and without a bias), UCOD_EPI_BIAS_BF16 (with and without the column scale), UCOD_EPI_BIAS_SCALE_RESID_F32 (out of place and with
    out == resid): bitwise the exactly rounded reference.  UCOD_EPI_BIAS_GELU_BF16 on pre-activations k / 64: within the fit's error plus half an ulp.
    The 16-bit cases need a real rounding in at least half of their elements (asserted by the helper): that is what pins the rounding mode."""
    M, Nn, K, variant, plan = case
    _run(half, kind, M, Nn, K, variant, plan)


@pytest.mark.parametrize("case", RESID16_CASES, ids=_id)
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_gemm_fp16_residual_stream_epilogue_is_exact(half, case):
    """UCOD_EPI_BIAS_SCALE_RESID_H16, in place as the driver calls it: amp 1 and a residual within +-64, so that every value of the reference is an fp16 number
    (asserted by the helper) and the 16-bit read-modify-write is exact."""
    M, Nn, K, variant, plan = case
    _run(half, "resid16", M, Nn, K, variant, plan)


@pytest.mark.parametrize("case", WSCALE_CASES, ids=_id)
@pytest.mark.parametrize("kind", ["wscale32", "wscale16"])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_gemm_column_scale_keeps_its_f32_bits(half, kind, case):
    """Column scales with 9 fraction bits (no bf16 value; (sum + bias) * scale still fits 24 bits): a scale that passes through 16 bits shows."""
    M, Nn, K, variant, plan = case
    _run(half, kind, M, Nn, K, variant, plan)


@pytest.mark.parametrize("kind", ["bias16", "resid32", "bias32"])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_gemm_without_patches_gives_the_same_bits(half, kind):
    """UCOD_GEMM_NO_PATCH=1 (leftover tiles as a partly filled round): the tiles-only plan of a patches shape equals the same exact reference bit for bit."""
    M, Nn, K = 16401, 776, 128
    lib = N.load(half)
    old = os.environ.get("UCOD_GEMM_NO_PATCH")
    os.environ["UCOD_GEMM_NO_PATCH"] = "1"
    try:
        lib.ucod_gemm_reload_tuning()                              # (the tuning variables are read once per process, not per launch)
        _run(half, kind, M, Nn, K, 9, P("big256", 0, 0), plan_kw={"no_patch": True})
    finally:
        if old is None:
            del os.environ["UCOD_GEMM_NO_PATCH"]
        else:
            os.environ["UCOD_GEMM_NO_PATCH"] = old
        lib.ucod_gemm_reload_tuning()
    _run(half, kind, M, Nn, K, 9, P("big256+patches", 2, 0))


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_entry_refuses_what_would_read_a_null_bias_or_split_a_row_store(half):
    """A NULL bias is the plain product of the large-tile kernels; the 128 x 128 and 64 x 64 kernels (variants 1, 2, 12) read the bias in their drain, so the
    entry refuses them (UCOD_EINVAL, nothing launched) -- as it does K < 128 and N % 4 != 0."""
    lib = N.load(half)
    M, Nn, K = 64, 64, 128
    A, W = torch.zeros(M, K, dtype=DT[half], device=DEV), torch.zeros(Nn, K, dtype=DT[half], device=DEV)
    buf, out = _guarded(M, Nn, F32)
    for epi in (N.EPI_BIAS_F32, N.EPI_BIAS_BF16):
        for variant in (1, 2, 12):
            assert X.plan("bias32", M, Nn, K, variant, N_CU, has_bias=False).path == "refused"
            assert lib.ucod_gemm_bf16(epi, N.ptr(A), N.ptr(W), out.data_ptr(), M, Nn, K, None, None, None, None, 0, variant, N.stream()) == -1, (epi, variant)
        assert lib.ucod_gemm_bf16(epi, N.ptr(A), N.ptr(W), out.data_ptr(), M, Nn, 64, None, None, None, None, 0, 9, N.stream()) == -1
    # 13 / 14 fall back to 9 / 10 where no mixed-height plan applies: the same widths are refused (16-byte row stores)
    b = torch.zeros(104, device=DEV)
    for variant in (9, 10, 13, 14):
        assert X.plan("bias32", M, 102, K, variant, N_CU).path == "refused" and X.plan("bias16", M, 100, K, variant, N_CU).path == "refused"
        assert lib.ucod_gemm_bf16(N.EPI_BIAS_F32, N.ptr(A), N.ptr(W), out.data_ptr(), M, 62, K, N.ptr(b), None, None, None, 0, variant, N.stream()) == -1, variant
        assert lib.ucod_gemm_bf16(N.EPI_BIAS_BF16, N.ptr(A), N.ptr(W), out.data_ptr(), M, 60, K, N.ptr(b), None, None, None, 0, variant, N.stream()) == -1, variant
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


LAB_CASES = ([(300, 264, 128, v, P("big256" if v in (3, 5) else "big192", 0, 0)) for v in (3, 4, 5, 6)] + [(300, 264, 128, 7, P("pers256", 0, 0)), (513, 392, 192, 8, P("pers192", 0, 0))] +
             [(513, 392, 192, v, P("big256" if v in (3, 5) else "big192", 0, 0)) for v in (3, 4, 5, 6)] +
             [(21916, 768, 192, 3, P("big256+patches", 1, 0)), (21916, 768, 192, 5, P("big256+patches", 1, 0)), (21916, 768, 192, 4, P("big192", 0, 0)),
              (21916, 768, 192, 6, P("big192", 0, 0)), (21916, 768, 192, 7, P("pers256", 0, 0)), (21916, 768, 192, 8, P("pers192", 0, 0)),
              (16401, 768, 128, 4, P("big192+patches", 2, 0)), (16401, 768, 128, 6, P("big192+patches", 2, 0))])


@pytest.mark.parametrize("case", [lab(c) for c in LAB_CASES], ids=[_id(c) for c in LAB_CASES])
@pytest.mark.parametrize("kind", ["bias32", "bias16", "scale16", "resid32", "gelu16"])
def test_laboratory_variants_are_exact(kind, case):
    """Variants 3-8 of the laboratory library (bf16 operands): the same template instantiated with four barrier intervals / no stagger / persistent."""
    M, Nn, K, variant, plan = case
    _run("bf16", kind, M, Nn, K, variant, plan, fn=N.load_lab().ucod_gemm_bf16_lab)


# ================================================================================================ row-mapped epilogues
B_IMG, NP, D_EMB, C_KEY, K_RM = 21, 25, 264, 300, 128             # 525 patch rows: three 256-row tiles, every one straddling images; 264 / 300: ragged last tiles
RM_PLANS = {9: "big256", 10: "big192", 2: "t128", 12: "t64", 0: "t64"}   # 9: the 256-wide offset-scheme drain; 10: the chunk-by-chunk drain


@functools.lru_cache(maxsize=None)
def _patch_case(h16):
    kw = X.family("h16", K_RM, F16) if h16 else X.family("f32", K_RM)
    kw["rounding_refs"] = ("pos",) if h16 else ()
    return X.exact_case(B_IMG * NP, D_EMB, K_RM, seed=4242 + h16, pos_rows=NP + 1, device=DEV, **kw)


@pytest.mark.parametrize("variant", [9, 10, 2, 12, 0])
@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("n_reg", [0, 4])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_patch_token_epilogues_are_exact(half, n_reg, h16, variant):
    """UCOD_EPI_PATCH_TOKENS_F32 / _H16 through ucod_gemm_bf16_reg: (sum + bias) + position row, rows remapped past the CLS and register rows, which stay
    untouched like the guard rows around the token matrix."""
    lib = N.load(half)
    c = _patch_case(h16)
    M, tok, odt = B_IMG * NP, 1 + n_reg + NP, F16 if h16 else F32
    kind = "patch16" if h16 else "patch32"
    plan = X.plan(kind, M, D_EMB, K_RM, variant, N_CU, tok=tok, n_reg=n_reg)
    assert plan.path == RM_PLANS[variant], (plan, variant)
    A, W = c.operands(DT[half], DEV)
    bias, pos = c.bias.float().to(DEV), c.pos.float().to(DEV)
    assert bool((bias.double().cpu() == c.bias).all()) and bool((pos.double().cpu() == c.pos).all())
    bufs = []
    for _ in range(2):
        buf, out = _guarded(B_IMG * tok, D_EMB, odt)
        rc = lib.ucod_gemm_bf16_reg(N.EPI_PATCH_TOKENS_H16 if h16 else N.EPI_PATCH_TOKENS_F32, N.ptr(A), N.ptr(W), out.data_ptr(), M, D_EMB, K_RM, N.ptr(bias), None, None,
                                    N.ptr(pos), tok, n_reg, variant, N.stream())
        assert rc == 0, rc
        bufs.append(buf)
    torch.cuda.synchronize()
    what = f"{half} {kind} R={n_reg} v{variant} ({plan.path})"
    assert _guards_intact(bufs[0], B_IMG * tok), what + ": guard rows were written"
    assert torch.equal(bufs[0], bufs[1]), what + ": a second launch differs"
    rows = bufs[0][GUARD:GUARD + B_IMG * tok].view(B_IMG, tok, D_EMB)
    assert bool((rows[:, :1 + n_reg] == SENT).all()), what + ": a CLS or register row was written"
    X.check_exact(rows[:, 1 + n_reg:].reshape(M, D_EMB), c.ref("pos"), odt, what)


@functools.lru_cache(maxsize=None)
def _key_case(tok):
    return X.exact_case(C_KEY, 12 * tok, K_RM, seed=777 + tok, device=DEV, **X.family("f32", K_RM))


@pytest.mark.parametrize("variant", [9, 10, 2, 12, 0])
@pytest.mark.parametrize("n_reg", [0, 4])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_key_hook_epilogue_is_exact(half, n_reg, variant):
    """UCOD_EPI_KEY_NCHW_F32 through ucod_gemm_bf16_reg: rows = 300 channels, columns = 12 images of 26 / 30 tokens (images straddle 4-token groups, 64-column
    waves and the tile edge), CLS and register columns dropped, written as [B, C, n_patch] with the per-channel bias."""
    lib = N.load(half)
    tok, Bk = 1 + n_reg + NP, 12
    c = _key_case(tok)
    plan = X.plan("key32", C_KEY, Bk * tok, K_RM, variant, N_CU, tok=tok, n_reg=n_reg)
    assert plan.path == RM_PLANS[variant], (plan, variant)
    Wk, x = c.operands(DT[half], DEV)
    bias = c.rowbias.float().to(DEV)
    assert bool((bias.double().cpu() == c.rowbias).all())
    bufs = []
    for _ in range(2):
        buf, out = _guarded(Bk * C_KEY, NP, F32)
        rc = lib.ucod_gemm_bf16_reg(N.EPI_KEY_NCHW_F32, N.ptr(Wk), N.ptr(x), out.data_ptr(), C_KEY, Bk * tok, K_RM, N.ptr(bias), None, None, None, tok, n_reg, variant, N.stream())
        assert rc == 0, rc
        bufs.append(buf)
    torch.cuda.synchronize()
    what = f"{half} key32 R={n_reg} v{variant} ({plan.path})"
    assert _guards_intact(bufs[0], Bk * C_KEY), what + ": guard rows were written"
    assert torch.equal(bufs[0], bufs[1]), what + ": a second launch differs"
    want = c.ref("rowbias").view(C_KEY, Bk, tok)[:, :, 1 + n_reg:].permute(1, 0, 2).reshape(Bk * C_KEY, NP)
    X.check_exact(bufs[0][GUARD:GUARD + Bk * C_KEY], want, F32, what)
