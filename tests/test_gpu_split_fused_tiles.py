"""GPU: UCOD_EPI_BIAS_GELU_SPLIT2 (fc1 + GELU + the two-term bf16 split in one launch, csrc/split.hip's terms = 2 pass) on the 192-wide tile paths -- variants 10
(one-shot large tile) and 14 (mixed-height) -- with N % 192 != 0.

The staged drain of those tiles marks a dropped 16-byte chunk (columns past N, rows 16..31 of a short last pass) with an out-of-range offset and used to ADD the
segment offsets 2 N and 4 N to it: 0xFFFFFFF0 + 2 N wraps back into the first rows of the wave's tile, where the stray hi / lo store raced with the rightful owner of
those bytes.  The segments now keep the sentinel (`o >= 0x80000000u ? o : o + ...`, as the SwiGLU branch always did).  A race: the old code did not fail every time,
and this test need not have failed on it deterministically; it pins the paths' results -- every value against f64, hi | hi equal, guard rows intact -- which
tests/test_gpu_split.py covers for variants 0, 12, 9 and 13 only."""
import pytest
import torch

from conftest import maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops  # noqa: E402

from split16_ref import rel_l2  # noqa: E402

DEV = "cuda"


@pytest.mark.parametrize("variant", [10, 14])
@pytest.mark.parametrize("M,Nn,K", [(4111, 4096, 256), (4111, 1000, 256)])
def test_gelu_split2_on_192_wide_tiles_with_ragged_columns(M, Nn, K, variant):
    """Bounds of tests/test_gpu_split.py::test_fc1_gelu_split2_epilogue (2e-5 rel-L2: two bf16 terms keep 16 bits; 6e-4 max).  A stray store of another chunk's hi or
    lo words into a live row is an error of the size of the values themselves, far above either bound; rows are exactly 3 N wide, so one behind the last row lands in
    the guard rows."""
    g = torch.Generator().manual_seed(M + Nn)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05, torch.randn(Nn, generator=g) * 0.2
    ref = torch.nn.functional.gelu(x.double() @ w.double().t() + b.double())
    xs, ws = ops.split_rows(x.to(DEV), 2, 0), ops.split_rows(w.to(DEV), 2, 1)
    bias = b.to(DEV)
    for rep in range(3):                                            # (a race shows up in some launches only)
        out = torch.full((M + 3, 3 * Nn), -7.0, dtype=torch.bfloat16, device=DEV)
        ops.gemm_bf16(N.EPI_BIAS_GELU_SPLIT2, xs, ws, out, M, Nn, 3 * K, bias=bias, variant=variant)
        assert bool((out[M:] == -7.0).all()), (variant, rep)
        seg = out[:M].view(M, 3, Nn)
        assert torch.equal(seg[:, 0], seg[:, 1]), (variant, rep)   # hi | hi
        got = ops.unsplit(out[:M].contiguous(), 2, 0, Nn).cpu().double()
        err = rel_l2(got, ref)
        print(f"GELU_SPLIT2 M={M} N={Nn} variant={variant} launch {rep}: rel-L2 {err:.3e}, max {maxdiff(got, ref):.3e}")
        assert err < 2e-5, (err, variant, rep)
        assert maxdiff(got, ref) < 6e-4 * max(1.0, float(ref.abs().max())), (variant, rep)
