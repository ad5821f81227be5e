"""GPU: the MLP hidden in MFMA-fragment order (BLK16: include/ucod_dpl.h, ucod_dpl_amd/blk16.py).

fc1's blocked drain (UCOD_EPI_LNFOLD_GELU_BLK16, UCOD_EPI_BIAS_GELU_BLK16) applies the row-major epilogue's f32 operations to the same accumulator values, so its
buffer, unpacked on the host, must equal the row-major launch BIT FOR BIT -- on every large-tile path, with M % 16 != 0, into a buffer pre-filled with NaN patterns.
fc2 with a BLK16 A operand and the column-permuted weight (ucod_gemm_bf16_blk16a) sums K in another order: bit-identical to the row-major launch (and to the exactly
rounded reference) on the integer operands of tests/gemm_exact_ref.py, row partials included; within the f64-reference bound of tests/test_gpu_f16_kernels.py on
random operands; and with NaN in the padding rows of A nothing stored is touched by them and the saturation counter stays at zero.
"""
import functools
import math

import pytest
import torch

import gemm_exact_ref as X
from conftest import within

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import blk16, native as N, ops  # noqa: E402

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
NAN_BITS = {"f16": 0x7E00, "bf16": 0x7FC0}
N_CU = torch.cuda.get_device_properties(0).multi_processor_count
EPS = 1e-6
H = 2.0 ** -11
GUARD = 4096                                                      # elements behind the BLK16 buffer that must keep their NaN pattern
P = X.Plan


@pytest.fixture(autouse=True)
def _a_gpu_fault_ends_the_run():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, run ended: {e}", returncode=3)


def _overflow_count(half):
    lib = N.load(half)
    host = torch.zeros(1, dtype=torch.int32).pin_memory()
    N.check(lib.ucod_resid16_overflow_fetch(host.data_ptr(), N.stream()), "fetch")
    torch.cuda.synchronize()
    n = int(host[0])
    N.check(lib.ucod_resid16_overflow_reset(N.stream()), "reset")
    torch.cuda.synchronize()
    return n


def _nan_buffer(n, half):
    return torch.full((n,), NAN_BITS[half], dtype=torch.int16, device=DEV).view(DT[half])


def _bits(t):
    return t.contiguous().view(torch.int16)


# ================================================================================================ fc1: the blocked drain against the row-major epilogue
# (M, N, K, variant, the path the ROW-MAJOR unfolded launch takes (mirror), the path both folded launches and the blocked unfolded one take)
FC1 = [(256, 256, 256, 9, P("big256", 0, 0), "big256"),
       (300, 320, 256, 9, P("big256", 0, 0), "big256"),             # ragged rows (M % 16 = 12) and a column tile whose last three waves are dead
       (513, 384, 256, 9, P("big256", 0, 0), "big256"),             # M % 16 = 1
       (1370, 3072, 768, 9, P("big256", 0, 0), "big256"),           # one image at the backbone's fc1 shape, M % 16 = 10
       (21916, 3072, 256, 0, P("mixed256", 0, 5), "mixed256"),      # auto: four whole rounds of mixed-height tiles, M % 16 = 12
       (21916, 768, 128, 13, P("mixed256", 0, 5), "mixed256"),      # tall tiles among one round
       (21916, 768, 192, 9, P("big256+patches", 1, 0), "big256")]   # where the row-major launch computes leftover tiles as patches, the blocked one runs tiles only


def _fc1_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-v{c[3]}-{c[5]}"


def _mixed_expected(M, Nn):
    feasible, _, n_tall, rounds = X.mixed_plan(M, Nn, 256, N_CU)
    return feasible, n_tall, rounds


@functools.lru_cache(maxsize=None)
def _fc1_operands(M, Nn, K):
    g = torch.Generator().manual_seed(M + Nn + K)
    x = (torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g) * 2) + torch.randn(M, 1, generator=g) * 0.3)
    w, b = torch.randn(Nn, K, generator=g) * 0.04, torch.randn(Nn, generator=g) * 0.1
    gamma, beta = 1 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    return x, w, b, gamma, beta


def _check_blocked(half, buf, M, Nn, want, what):
    Mp = blk16.padded_rows(M)
    got = blk16.unpack(buf[:Mp * Nn], M, Nn)
    assert not bool(want.isnan().any()), what
    assert torch.equal(_bits(got), _bits(want)), f"{what}: {int((_bits(got) != _bits(want)).sum())} of {M * Nn} values differ from the row-major epilogue"
    assert bool((_bits(buf[Mp * Nn:]) == _bits(_nan_buffer(1, half))[0]).all()), what + ": wrote behind the buffer"


@pytest.mark.parametrize("case", FC1, ids=_fc1_id)
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_fc1_blocked_drain_equals_the_row_major_epilogue(half, case):
    """UCOD_EPI_BIAS_GELU_BLK16 against UCOD_EPI_BIAS_GELU_BF16, same operands, same variant."""
    M, Nn, K, variant, rm_plan, path = case
    assert X.plan("gelu16", M, Nn, K, variant, N_CU) == rm_plan, (case, X.plan("gelu16", M, Nn, K, variant, N_CU))
    if path == "mixed256":
        feasible, n_tall, rounds = _mixed_expected(M, Nn)
        assert feasible and n_tall == rm_plan.n_tall and (variant != 0 or rounds >= 3), (feasible, n_tall, rounds)
    if "patches" in rm_plan.path:
        # the row-major launch sums the leftover tiles' K in another order (8 interleaved partials): equal bits are owed only where every order gives the same
        # f32 sum -- the integer operands of the exact-arithmetic suite (pre-activations on a grid of 2^-6)
        c = X.exact_case(M, Nn, K, seed=M + Nn + K + 4000, device=DEV, **X.family("gelu", K, DT[half]))
        A, W = c.operands(DT[half], DEV)
        bias = c.bias.float().to(DEV)
    else:
        x, w, b, _, _ = _fc1_operands(M, Nn, K)
        A, W, bias = x.to(DT[half]).to(DEV), w.to(DT[half]).to(DEV), b.to(DEV)
    lib = N.load(half)
    want = torch.empty(M, Nn, dtype=DT[half], device=DEV)
    N.check(lib.ucod_gemm_bf16(N.EPI_BIAS_GELU_BF16, N.ptr(A), N.ptr(W), N.ptr(want), M, Nn, K, N.ptr(bias), None, None, None, 0, variant, N.stream()), "row-major")
    buf = _nan_buffer(blk16.padded_rows(M) * Nn + GUARD, half)
    N.check(lib.ucod_gemm_bf16(N.EPI_BIAS_GELU_BLK16, N.ptr(A), N.ptr(W), N.ptr(buf), M, Nn, K, N.ptr(bias), None, None, None, 0, variant, N.stream()), "blocked")
    torch.cuda.synchronize()
    _check_blocked(half, buf, M, Nn, want, f"{half} gelu {_fc1_id(case)}")


# row partials exist for large passes only (ucod_gemm_bf16_stats refuses smaller ones), and the consumer merges them in pairs of 64-column slots
FC1_FOLDED = [(c, False) for c in FC1] + [(c, True) for c in FC1 if c[0] >= 2048 and (c[2] // 64) % 2 == 0]


@pytest.mark.parametrize("case,partials", FC1_FOLDED, ids=[f"{_fc1_id(c)}-{'partials' if p else 'stats'}" for c, p in FC1_FOLDED])
def test_fc1_folded_blocked_drain_equals_the_row_major_epilogue(case, partials):
    """UCOD_EPI_LNFOLD_GELU_BLK16 against UCOD_EPI_LNFOLD_GELU_BF16 (fp16-operand build): row statistics from ucod_row_stats_h16, and -- large passes, as the
    engine runs them -- from the row partials a residual producer left."""
    M, Nn, K, variant, _, path = case
    x, w, b, gamma, beta = _fc1_operands(M, Nn, K)
    wf, bf_, cs = ops.fold_layernorm_linear(gamma.to(DEV), beta.to(DEV), w.to(DEV), b.to(DEV))
    xd = x.half().to(DEV)
    part = None
    if partials:                                                    # x = x + 1 * (0 W^T + 0): the rows themselves, with their partials
        z = torch.zeros(M, 128, dtype=torch.float16, device=DEV)
        xd, part = ops.linear_scale_resid_h16_stats(z, torch.zeros(K, 128, dtype=torch.float16, device=DEV), torch.zeros(K, device=DEV), torch.ones(K, device=DEV), xd)
    st = None
    if not partials:                                                # (rstd, -mean rstd) per row; both launches read the same table (ucod_row_stats_h16 has no kernel for every K here)
        mean, var = xd.float().mean(1), xd.float().var(1, unbiased=False)
        rstd = (var + EPS).rsqrt()
        st = torch.stack([rstd, -mean * rstd], 1).contiguous()
    nslot = K // 64 if partials else 0
    lib = N.load("f16")

    def run(epi, out):
        N.check(lib.ucod_gemm_lnfold(epi, N.ptr(xd), N.ptr(wf), N.ptr(out), M, Nn, K, N.ptr(bf_), N.ptr(cs), N.ptr(st), N.ptr(part), nslot, EPS, None, variant,
                                     N.stream()), "ucod_gemm_lnfold")
    want = torch.empty(M, Nn, dtype=torch.float16, device=DEV)
    run(N.EPI_LNFOLD_GELU_BF16, want)
    buf = _nan_buffer(blk16.padded_rows(M) * Nn + GUARD, "f16")
    run(N.EPI_LNFOLD_GELU_BLK16, buf)
    torch.cuda.synchronize()
    _check_blocked("f16", buf, M, Nn, want, f"folded gelu {_fc1_id(case)} {'partials' if partials else 'stats'}")
    assert _overflow_count("f16") == 0


def test_blocked_epilogues_refuse_what_the_large_tiles_cannot_take():
    lib = N.load("f16")
    A = torch.zeros(4096, 256, dtype=torch.float16, device=DEV)
    W = torch.zeros(256, 256, dtype=torch.float16, device=DEV)
    out = torch.zeros(4096 * 256, dtype=torch.float16, device=DEV)
    b = torch.zeros(256, device=DEV)

    def call(M, Nn, K, variant):
        return lib.ucod_gemm_bf16(N.EPI_BIAS_GELU_BLK16, N.ptr(A), N.ptr(W), N.ptr(out), M, Nn, K, N.ptr(b), None, None, None, 0, variant, N.stream())
    assert call(4096, 256, 256, 0) == 0
    assert call(4096, 224, 256, 0) == -1                            # N % 64
    assert call(4096, 256, 64, 0) == -1                             # K < 128
    assert call(200, 256, 256, 0) == -1                             # auto on a small pass: no large tile
    for v in (1, 2, 10, 12, 14):
        assert call(4096, 256, 256, v) == -1
    assert lib.ucod_gemm_bf16(N.EPI_LNFOLD_GELU_BLK16, N.ptr(A), N.ptr(W), N.ptr(out), 4096, 256, 256, N.ptr(b), None, None, None, 0, 0, N.stream()) == -1
    assert N.load("bf16").ucod_gemm_lnfold(N.EPI_LNFOLD_GELU_BLK16, N.ptr(A), N.ptr(W), N.ptr(out), 4096, 256, 256, N.ptr(b), N.ptr(b), N.ptr(b), None, 0, EPS, None, 0,
                                           N.stream()) == -1
    args = (N.ptr(A), N.ptr(W), N.ptr(out), 200, 256, 256, N.ptr(b), N.ptr(b), N.ptr(out), None, 0, N.stream())
    assert lib.ucod_gemm_bf16_blk16a(N.EPI_BIAS_SCALE_RESID_H16, *args) == -1                      # a small pass
    assert lib.ucod_gemm_bf16_blk16a(N.EPI_BIAS_BF16, *args) == -1
    torch.cuda.synchronize()


# ================================================================================================ fc2: BLK16 A operand, permuted weight
# the large fp16-residual cases of tests/test_gpu_gemm_exact.py (all on the mixed-height kernel, with and without tall tiles); M % 16 = 12, 4, 1, 0, 15
FC2_EXACT = [(21916, 768, 128, 5), (21916, 768, 192, 5), (16500, 776, 128, 4), (16401, 776, 128, 1), (43840, 768, 128, 10), (4111, 768, 128, 0)]


@functools.lru_cache(maxsize=None)
def _exact(M, Nn, K):
    return X.exact_case(M, Nn, K, seed=M + Nn + K + 3000, device=DEV, **X.family("resid16", K))


FC2_EXACT_RUNS = [(*c, False) for c in FC2_EXACT] + [(*c, True) for c in FC2_EXACT if c[1] % 64 == 0]     # (row partials need whole 64-column slots)


@pytest.mark.parametrize("M,Nn,K,n_tall,stats", FC2_EXACT_RUNS, ids=[f"{c[0]}x{c[1]}x{c[2]}-{'stats' if c[4] else 'plain'}" for c in FC2_EXACT_RUNS])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_fc2_blk16_operand_is_exact_and_ignores_poisoned_padding_rows(half, M, Nn, K, n_tall, stats):
    """Integer operands: every order of the K sum gives the same f32 bits, so the BLK16 launch must equal the row-major launch and the exactly rounded reference bit
    for bit -- outputs and (STATS) row partials.  The padding rows of A hold NaN: no stored output or partial may show it, and the saturation counter stays zero."""
    assert X.plan("resid16", M, Nn, K, 0, N_CU) == P("mixed256", 0, n_tall)
    c = _exact(M, Nn, K)
    A, W = c.operands(DT[half], DEV)
    bias, scale = c.bias.float().to(DEV), c.scale.float().to(DEV)
    resid = c.resid.to(torch.float16).to(DEV)
    Ab = blk16.pack(A, fill=float("nan"))
    assert M % 16 == 0 or bool(Ab.isnan().any())
    Wp = blk16.permute_weight(W)
    lib = N.load(half)
    nslot = Nn // 64 if stats else 0
    epi = N.EPI_BIAS_SCALE_RESID_H16_STATS if stats else N.EPI_BIAS_SCALE_RESID_H16
    _overflow_count(half)
    want, got = resid.clone(), resid.clone()
    pw = torch.full((M, max(nslot, 1), 2), float("nan"), device=DEV)
    pg = pw.clone()
    if stats:
        N.check(lib.ucod_gemm_bf16_stats(epi, N.ptr(A), N.ptr(W), N.ptr(want), M, Nn, K, N.ptr(bias), N.ptr(scale), N.ptr(want), None, 0, N.ptr(pw), nslot, N.stream()), "row-major")
    else:
        N.check(lib.ucod_gemm_bf16(epi, N.ptr(A), N.ptr(W), N.ptr(want), M, Nn, K, N.ptr(bias), N.ptr(scale), N.ptr(want), None, 0, 0, N.stream()), "row-major")
    N.check(lib.ucod_gemm_bf16_blk16a(epi, N.ptr(Ab), N.ptr(Wp), N.ptr(got), M, Nn, K, N.ptr(bias), N.ptr(scale), N.ptr(got), N.ptr(pg) if stats else None, nslot,
                                      N.stream()), "blk16a")
    torch.cuda.synchronize()
    what = f"{half} fc2 blk16 {M}x{Nn}x{K}"
    assert bool(got.isfinite().all()), what
    assert torch.equal(got, want), what
    X.check_exact(got, c.ref("resid"), torch.float16, what)
    if stats:
        assert bool(pg.isfinite().all()) and torch.equal(pg, pw), what + ": row partials"
    assert _overflow_count(half) == 0, what + ": the padding rows reached the saturation test"


@pytest.mark.parametrize("M,Nn,K", [(4111, 768, 3072), (21916, 768, 768)])
def test_fc2_blk16_operand_against_the_f64_product(M, Nn, K):
    """Random fp16 operands: the bound test_gpu_f16_kernels.py holds the row-major resid16 epilogue to (one fp16 rounding of the output plus the f32 accumulation,
    4e-5 (1 + |ref|), times sqrt(3) at K = 3072) -- only the order of the f32 additions differs."""
    g = torch.Generator().manual_seed(M + Nn + K)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(Nn, K, generator=g) * 0.05).half()
    b, sc = torch.randn(Nn, generator=g) * 0.1, 0.5 + torch.rand(Nn, generator=g)
    resid = (torch.randn(M, Nn, generator=g) * 2).half()
    Ad, Wd = A.to(DEV), W.to(DEV)
    ref = resid.to(DEV).double() + sc.to(DEV).double() * (Ad.double() @ Wd.double().t() + b.to(DEV).double())
    out = resid.to(DEV).clone()
    bd, scd = b.to(DEV), sc.to(DEV)
    N.check(N.load("f16").ucod_gemm_bf16_blk16a(N.EPI_BIAS_SCALE_RESID_H16, N.ptr(blk16.pack(Ad, fill=float("nan"))), N.ptr(blk16.permute_weight(Wd)), N.ptr(out), M, Nn, K,
                                                N.ptr(bd), N.ptr(scd), N.ptr(out), None, 0, N.stream()), "blk16a")
    torch.cuda.synchronize()
    kmul = math.sqrt(3.0) if K >= 3072 else 1.0
    err = (out.double() - ref).abs()
    within(f"blk16 fc2 resid16 {M}x{Nn}x{K}", float((err / (H * ref.abs() + 4e-5 * kmul * (1 + ref.abs()))).max()), 1.0)
