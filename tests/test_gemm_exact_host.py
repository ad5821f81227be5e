"""CPU: what makes the bit-for-bit GEMM tests of tests/test_gpu_gemm_exact.py legitimate, and what they can see.

1. Preconditions: for every case family of gemm_exact_ref.family() the f32 sum over K gives identical bits in every order a kernel uses -- forward,
   reversed, the 8 interleaved partials of patch_phase (gemm_bf16_tiles.h), 64-wide K tiles -- and those bits are the f64 reference.
2. Checker sensitivity: each fault that the global bounds of tests/test_gpu_kernels.py let through (replayed there on the CPU: truncated output, an accumulator
   rounded to 16 bits in front of the bias, one K term lost in one row per 128-row tile, a 16-bit bias or residual in an f32 epilogue), plus a neighbour's bias, a
   row written one row too far and a 16-bit scale, applied to a correct product: check_exact / check_gelu reject every one.  The old pair of bounds
   (rel_l2 < 4e-3, maxdiff < 2e-2 max|ref|) accepts truncation and double rounding: asserted, as a record of the gap.
3. The gelu_erf2 polynomial of gemm_bf16_epilogue.h, transcribed in f32, against f64 GELU over [-30, 30] within E = 1e-6 + 2^-22 |x|.
4. The launch-plan mirror on the shapes of the GPU file at 256 CUs.
"""
import pytest
import torch

import gemm_exact_ref as X

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


# ================================================================================================ 1. preconditions
def _sum_orders(A, W):
    """f32 sums of A W^T over K in four orders, [M, N] each."""
    M, K = A.shape
    term = lambda k: A[:, k, None] * W[None, :, k]               # noqa: E731   (one k at a time: no hidden order inside a matmul)
    fwd = torch.zeros(M, W.shape[0])
    for k in range(K):
        fwd = fwd + term(k)
    rev = torch.zeros_like(fwd)
    for k in reversed(range(K)):
        rev = rev + term(k)
    parts = []                                                    # patch_phase: wave w takes the 32-wide k-steps w, w + 8, ...; the partials meet in wave order
    for w in range(8):
        p = torch.zeros_like(fwd)
        for st in range(w, K // 32, 8):
            for k in range(32 * st, 32 * st + 32):
                p = p + term(k)
        parts.append(p)
    inter = parts[0]
    for p in parts[1:]:
        inter = inter + p
    tiles = torch.zeros_like(fwd)                                 # 64-wide K tiles, each summed on its own (4 x 16-deep MFMA chains) and then added
    for t in range(K // 64):
        sub = torch.zeros_like(fwd)
        for q in range(4):
            s4 = torch.zeros_like(fwd)
            for k in range(64 * t + 16 * q, 64 * t + 16 * q + 16):
                s4 = s4 + term(k)
            sub = sub + s4
        tiles = tiles + sub
    return {"forward": fwd, "reversed": rev, "8 interleaved partials": inter, "64-wide K tiles": tiles}


@pytest.mark.parametrize("fam,K", [("f32", 128), ("f32", 768), ("f32", 5632), ("h16", 128), ("h16", 192), ("h16", 5632), ("h16f", 128), ("h16f", 768), ("h16f", 5632), ("resid16", 192), ("gelu", 128), ("gelu", 5632),
                                   ("wscale", 128)])
def test_every_summation_order_gives_the_same_f32_bits(fam, K):
    c = X.exact_case(24, 16, K, seed=K + len(fam), **(X.family("h16", K, HF) if fam == "h16f" else X.family(fam, K, BF)))
    A, W = c.operands(F32, "cpu")
    want = c.ref("plain").float()
    assert bool((want.double() == c.ref("plain")).all())
    for name, got in _sum_orders(A, W).items():
        assert got.dtype == F32 and torch.equal(got, want), (fam, K, name)
    # the epilogue arithmetic in f32, bias in front of the sum (large tiles) or behind it (128 x 128 tiles, patches): the same bits again
    b, s, r = c.bias.float(), c.scale.float(), c.resid.float()
    assert bool((b.double() == c.bias).all() and (s.double() == c.scale).all() and (r.double() == c.resid).all())
    assert torch.equal(want + b, c.ref("bias").float()) and bool((c.ref("bias").float().double() == c.ref("bias")).all())
    assert torch.equal((want + b) * s, c.ref("scale").float())
    assert torch.equal(r + s * (want + b), c.ref("resid").float()) and bool((c.ref("resid").float().double() == c.ref("resid")).all())
    front = b.expand(24, 16).clone()
    for k in range(K):
        front = front + A[:, k, None] * W[None, :, k]
    assert torch.equal(front, c.ref("bias").float())


def test_the_helper_refuses_cases_that_are_not_exact():
    with pytest.raises(AssertionError, match="not exact"):
        X.exact_case(8, 8, 4096, seed=1, amp=64, fine_bits=7)                         # 4096 * 64 * 64 * 2^7 >= 2^24
    with pytest.raises(AssertionError, match="not exact"):
        X.exact_case(8, 8, 128, seed=1, amp=4, fine_bits=7, resid_amp=1 << 17).ref("resid")
    with pytest.raises(AssertionError, match="declared representable"):
        X.exact_case(64, 64, 768, seed=1, amp=4, out_dtype=BF, representable_refs=("bias",))
    with pytest.raises(AssertionError, match="rounding mode"):
        X.exact_case(64, 64, 64, seed=1, amp=1, out_dtype=HF, rounding_refs=("bias",))


# ================================================================================================ 2. checker sensitivity
def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def _trunc16(v, dtype):
    """f32 -> 16 bits by dropping the low bits (toward zero) instead of rounding."""
    drop = 16 if dtype == BF else 13
    return ((v.float().contiguous().view(torch.int32) >> drop) << drop).view(F32).to(dtype)


def _lose_a_term(c, k0=5):
    """A W^T with the term k0 missing in the last row of every 128-row tile."""
    A, W = c.operands(torch.float64, "cpu")
    acc = c.acc.clone()
    rows = [r for r in range(c.M) if r % 128 == 127]
    acc[rows] -= A[rows, k0, None] * W[None, :, k0]
    return acc


@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("M,N,K", [(200, 256, 128), (300, 128, 768), (333, 128, 3072)])
def test_check_exact_rejects_every_fault_in_a_16_bit_output(dtype, M, N, K):
    c = X.exact_case(M, N, K, seed=M + N + K, **X.family("h16", K, dtype))
    v, vs = c.ref("bias"), c.ref("scale")
    X.check_exact(v.to(dtype), v, dtype)                                                       # the correct product passes
    X.check_exact(vs.to(dtype), vs, dtype)
    _rejects(X.check_exact, _trunc16(v, dtype), v, dtype)                                      # truncated instead of rounded
    _rejects(X.check_exact, (c.acc.to(dtype).double() + c.bias).to(dtype), v, dtype)           # accumulator rounded to 16 bits in front of the bias
    _rejects(X.check_exact, (_lose_a_term(c) + c.bias).to(dtype), v, dtype)                    # one K term lost in the last row of every 128-row tile
    nb = c.bias.clone()
    nb[5::16] = c.bias[6::16]
    assert not torch.equal(nb, c.bias)
    _rejects(X.check_exact, (c.acc + nb).to(dtype), v, dtype)                                  # a neighbouring column's bias in one column of 16
    shifted = v.to(dtype).clone()
    shifted[131] = shifted[130]
    shifted[130] = -5.0
    _rejects(X.check_exact, shifted, v, dtype)                                                 # one output row written one row too far


@pytest.mark.parametrize("M,N,K", [(200, 256, 128), (300, 128, 768), (333, 128, 3072)])
def test_check_exact_rejects_every_fault_in_an_f32_output(M, N, K):
    c = X.exact_case(M, N, K, seed=M + N + K + 1, **X.family("f32", K))
    v, vr = c.ref("bias"), c.ref("resid")
    X.check_exact(v.float(), v, F32)
    X.check_exact(vr.float(), vr, F32)
    _rejects(X.check_exact, (c.acc + c.bias.to(BF).double()).float(), v, F32)                  # bias rounded to bf16
    _rejects(X.check_exact, (c.resid.to(HF).double() + c.scale * (c.acc + c.bias)).float(), vr, F32)   # residual rounded to fp16
    _rejects(X.check_exact, (_lose_a_term(c) + c.bias).float(), v, F32)
    _rejects(X.check_exact, (c.acc.to(BF).double() + c.bias).float(), v, F32)
    w = X.exact_case(M, N, 128, seed=M + N + 2, **X.family("wscale", 128))
    vw = w.ref("resid")
    X.check_exact(vw.float(), vw, F32)
    assert not torch.equal(w.scale.to(BF).double(), w.scale)
    _rejects(X.check_exact, (w.resid + w.scale.to(BF).double() * (w.acc + w.bias)).float(), vw, F32)   # a scale rounded to bf16
    w16 = X.exact_case(M, N, 128, seed=M + N + 3, **X.family("wscale", 128, BF))
    _rejects(X.check_exact, ((w16.acc + w16.bias) * w16.scale.to(BF).double()).to(BF), w16.ref("scale"), BF)


@pytest.mark.parametrize("dtype", [BF, HF])
def test_check_gelu_rejects_faults_and_accepts_the_fit(dtype):
    c = X.exact_case(200, 256, 768, seed=9, **X.family("gelu", 768, dtype))
    x = c.ref("bias")
    assert float(x.abs().max()) > 6.0 and float(x.abs().max()) < 30.0
    X.check_gelu(X.gelu_f64(x).to(dtype), x, dtype)                                             # exact GELU, one rounding
    X.check_gelu(X.gelu_erf2_f32(x.float()).to(dtype), x, dtype)                                # the kernel's fit in f32, one rounding
    _rejects(X.check_gelu, _trunc16(X.gelu_f64(x), dtype), x, dtype)
    _rejects(X.check_gelu, torch.nn.functional.gelu(x, approximate="tanh").to(dtype), x, dtype)   # the tanh form
    if dtype == BF:                                                                             # (k / 64 below 32 is an fp16 number: nothing to see there)
        _rejects(X.check_gelu, X.gelu_f64(x.to(dtype).double()).to(dtype), x, dtype)            # pre-activation rounded to 16 bits first
    nb = c.bias.clone()
    nb[5::16] = c.bias[6::16]
    _rejects(X.check_gelu, X.gelu_f64(c.acc + nb).to(dtype), x, dtype)


def _old_bounds_accept(out, ref):
    rel = ((out.double() - ref.double()).norm() / ref.double().norm()).item()
    return rel < 4e-3 and (out.double() - ref.double()).abs().max().item() < 2e-2 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("M,N,K", [(200, 256, 128), (2740, 384, 768), (333, 128, 3072)])
def test_the_old_global_bounds_accept_truncation_and_double_rounding(M, N, K):
    """The record of the gap: the assertions of test_gemm_bf16_bias (tests/test_gpu_kernels.py), on its own operands and seeds."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(BF)
    W = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    b = torch.randn(N, generator=g)
    acc = A.double() @ W.double().t()
    ref = (acc + b.double()).float()
    assert _old_bounds_accept(ref.to(BF), ref)
    assert _old_bounds_accept(_trunc16(ref, BF), ref)                                            # truncated, accepted
    assert _old_bounds_accept((acc.float().to(BF).float() + b).to(BF), ref)                      # double rounding, accepted
    _rejects(X.check_exact, _trunc16(ref, BF), ref.double(), BF)                                 # (what equality with the rounded reference says of the same output)


# ================================================================================================ 3. the GELU fit
def test_gelu_erf2_fit_meets_its_documented_error():
    """gemm_bf16_epilogue.h documents max |gelu err| = 7.1e-7 over [-30, 30] in fp32 for gelu_erf2; E = 1e-6 + 2^-22 |x| is that figure with room for the f32
    operations around the fit.  Dense grid, and the dyadic points k / 64 the GPU cases land on."""
    dense = torch.linspace(-30.0, 30.0, 3_000_001, dtype=torch.float64).float()
    dyadic = torch.arange(-30 * 64, 30 * 64 + 1, dtype=torch.float64).float() / 64.0
    for x in (dense, dyadic):
        err = (X.gelu_erf2_f32(x).double() - X.gelu_f64(x)).abs()
        ratio = err / X.gelu_tolerance(x)
        i = int(ratio.argmax())
        print(f"gelu_erf2 fit: worst error / E = {float(ratio[i]):.3f} at x = {float(x[i])!r} (|err| {float(err[i]):.3e}); max |err| {float(err.max()):.3e}")
        assert float(ratio.max()) <= 1.0, (float(x[i]), float(err[i]))


# ================================================================================================ 4. the plan mirror
PLAN_TABLE = [
    # kind, (M, N, K), variant -> path, patches per workgroup, tall tiles
    ("bias16", (128, 128, 64), 1, "t128", 0, 0), ("bias16", (129, 132, 128), 2, "t128", 0, 0), ("bias32", (1, 8, 64), 1, "t128", 0, 0),
    ("resid32", (257, 260, 192), 2, "t128", 0, 0), ("bias16", (200, 130, 192), 1, "t128", 0, 0),
    ("bias16", (64, 64, 64), 12, "t64", 0, 0), ("bias16", (65, 72, 128), 0, "t64", 0, 0), ("gelu16", (130, 66, 192), 0, "t64", 0, 0), ("gelu16", (130, 66, 192), 12, "t64", 0, 0),
    ("bias16", (256, 256, 64), 9, "big256", 0, 0), ("bias16", (256, 256, 64), 10, "big192", 0, 0), ("resid32", (300, 264, 128), 9, "big256", 0, 0),
    ("gelu16", (513, 392, 192), 10, "big192", 0, 0), ("bias32", (333, 128, 3072), 9, "big256", 0, 0), ("bias32", (333, 128, 3072), 0, "t64", 0, 0),
    ("bias16", (21916, 768, 64), 9, "big256+patches", 1, 0), ("bias16", (21916, 768, 192), 9, "big256+patches", 1, 0), ("bias16", (21916, 768, 768), 9, "big256+patches", 1, 0),
    ("resid32", (21916, 768, 2304), 9, "big256+patches", 1, 0), ("gelu16", (21916, 768, 5632), 9, "big256+patches", 1, 0),
    ("bias16", (16401, 776, 128), 9, "big256+patches", 2, 0), ("bias16", (43840, 768, 128), 9, "big256+patches", 1, 0),
    ("bias16", (16401, 768, 128), 10, "big192+patches", 2, 0), ("bias32", (16401, 768, 768), 10, "big192+patches", 2, 0),
    ("bias16", (21916, 768, 128), 13, "mixed256", 0, 5), ("gelu16", (21916, 768, 192), 13, "mixed256", 0, 5), ("resid32", (16500, 776, 128), 13, "mixed256", 0, 4),
    ("bias16", (16500, 768, 192), 14, "mixed192", 0, 4), ("bias16", (43840, 2304, 128), 0, "mixed256", 0, 10), ("gelu16", (43840, 2304, 128), 0, "mixed256", 0, 10),
    ("resid16", (21916, 768, 128), 0, "mixed256", 0, 5), ("resid16", (4111, 768, 128), 9, "mixed256", 0, 0), ("resid16", (257, 260, 192), 2, "t128", 0, 0),
    # the two shapes tests/test_gpu_f16_kernels.py named for patches and for mixed-height tiles: neither reached them
    ("bias16", (4111, 768, 768), 9, "big256", 0, 0), ("bias16", (8220, 2304, 768), 13, "big256", 0, 0),
    # ... and the two that do
    ("bias16", (21916, 768, 768), 13, "mixed256", 0, 5), ("resid32", (21916, 768, 768), 9, "big256+patches", 1, 0),
    # NULL bias: large tiles only
    ("bias32", (300, 264, 128), 0, "big192", 0, 0),
]


@pytest.mark.parametrize("kind,shape,variant,path,ppw,n_tall", PLAN_TABLE)
def test_plan_mirror_on_256_cus(kind, shape, variant, path, ppw, n_tall):
    has_bias = not (kind == "bias32" and shape == (300, 264, 128) and variant == 0)
    assert X.plan(kind, *shape, variant, 256, has_bias=has_bias) == X.Plan(path, ppw, n_tall)


def test_plan_mirror_switches_and_refusals():
    assert X.plan("bias16", 16401, 776, 128, 9, 256, no_patch=True) == X.Plan("big256", 0, 0)              # UCOD_GEMM_NO_PATCH=1
    assert X.plan("bias16", 43840, 2304, 128, 0, 256, no_mixed=True).path in ("big256", "big192")          # UCOD_GEMM_NO_MIXED=1
    assert X.plan("bias16", 256, 100, 128, 9, 256).path == "refused" and X.plan("bias32", 256, 102, 128, 10, 256).path == "refused"
    assert X.plan("bias32", 256, 104, 128, 9, 256).path == "big256" and X.plan("bias16", 256, 104, 96, 0, 256).path == "refused"
    assert X.plan("bias32", 256, 104, 128, 2, 256, has_bias=False).path == "refused" and X.plan("bias16", 256, 104, 128, 11, 256).path == "refused"
    for v in (13, 14):                                                                                      # (they become 9 / 10 where no mixed plan applies)
        assert X.plan("bias32", 256, 102, 128, v, 256).path == "refused" and X.plan("bias16", 256, 100, 128, v, 256).path == "refused"
        assert X.plan("bias32", 256, 104, 128, v, 256).path == ("big256" if v == 13 else "big192")
    # row-mapped drains: the 256-wide offset scheme needs whole images (and N % 8 for fp16 rows), else the 192-wide chunk drain
    assert X.plan("patch32", 525, 264, 128, 9, 256, tok=26).path == "big256" and X.plan("patch32", 520, 264, 128, 9, 256, tok=26).path == "big192"
    assert X.plan("patch16", 525, 260, 128, 9, 256, tok=30, n_reg=4).path == "big192" and X.plan("key32", 300, 360, 128, 9, 256, tok=30, n_reg=4).path == "big256"
    assert X.plan("key32", 300, 360, 128, 13, 256, tok=30, n_reg=4).path == "big256"                       # (not column-fused: 13 is 9)
    # laboratory variants: 3 / 5 as 9, 4 / 6 as 10 (patches included), 7 / 8 persistent
    assert X.plan("bias16", 21916, 768, 192, 5, 256) == X.Plan("big256+patches", 1, 0) and X.plan("bias16", 21916, 768, 192, 6, 256).path == "big192"
    assert X.plan("bias16", 21916, 768, 192, 7, 256).path == "pers256" and X.plan("resid16", 300, 264, 128, 3, 256).path == "refused"
