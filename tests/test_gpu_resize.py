"""GPU: ucod_bilinear_resize, ucod_bilinear_resize_adjoint and ucod_binarize (csrc/elementwise.hip) at every dispatch case, through the C ABI only.

resize_ref.py holds the f64 weight model, the derived bounds, the restatement of the two launch functions and the case lists; test_resize_ref_host.py
shows on the CPU that the model is ATen's, that the lists reach every class and that the checker rejects the faults the cases are there for.  Here:

   1  test_forward / test_adjoint          every case against the model within its bound; sentinels in front and behind; a second launch bit for bit
   2  test_dyadic_cases_are_exact          power-of-two ratios on integers and masks: equal to the model, in both dispatch classes of both directions
   3  test_adjoint_is_the_transpose        <Ux, y> == <x, U^T y> in f64 from the two GPU results, within the sum of the two bounds
   4  test_thresholds_of_resized_masks     (gpu > 0.5) == (model > 0.5) away from the ties, at the evaluation path's geometries; binarize agrees
   5  test_binarize_*                      the threshold itself: special values, both modes, n = 0, the second trip of the grid stride
   6  test_resize_then_binarize_logits     loop_look_twice.py:214 as it runs
   7  test_refusals                        NULL pointers, non-positive sizes, more than 16 taps: UCOD_EINVAL and nothing written

Every output is a view inside a larger buffer of one NaN bit pattern, the payload included, so an element no store reached shows.
Measured ratios: profiles/resize_tests.txt (a record; no bound is taken from it).
"""
import numpy as np
import pytest
import torch

import resize_ref as R
from conftest import within

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402

DEV = "cuda"
EINVAL = -1
PAD = 1024                                                                     # floats on either side of an output (a multiple of 4: the payload stays 16-byte aligned)
SENTINEL = 0x7FC5A5A5                                                          # a quiet NaN no kernel here produces


class Guarded:
    """n floats between two sentinel runs, all SENTINEL to begin with"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)

    def ptr(self):
        return N.ptr(self.buf[PAD:PAD + self.n])

    def guards_intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def bits(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy()

    def values(self, shape):
        return self.bits().view(np.float32).reshape(shape)


def device_input(a, off=0):
    """the array on the GPU, starting `off` floats past a 16-byte boundary: a view into a larger buffer, as a slice of a batch is"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    buf = torch.zeros(off + a.size, dtype=torch.float32, device=DEV)
    view = buf[off:]
    view.copy_(torch.from_numpy(a.copy()))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * off) % 16
    return view


def run_fwd(c, x):
    out = Guarded(c.planes * c.oh * c.ow)
    xd = device_input(x, c.off)
    rc = N.load().ucod_bilinear_resize(N.ptr(xd), out.ptr(), c.planes, c.ih, c.iw, c.oh, c.ow, N.stream())
    torch.cuda.synchronize()
    return rc, out


def run_adj(c, g):
    out = Guarded(c.planes * c.ih * c.iw)
    gd = device_input(g, c.off)
    rc = N.load().ucod_bilinear_resize_adjoint(N.ptr(gd), out.ptr(), c.planes, c.ih, c.iw, c.oh, c.ow, N.stream())
    torch.cuda.synchronize()
    return rc, out


def run_binarize(x, logits, n=None):
    x = np.asarray(x, dtype=np.float32)
    n = x.size if n is None else n
    out = Guarded(max(n, 1))
    xd = device_input(x)
    rc = N.load().ucod_binarize(N.ptr(xd), out.ptr(), n, int(logits), N.stream())
    torch.cuda.synchronize()
    return rc, out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ================================================================================================ 1. every case against the model
@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
def test_forward(c):
    assert R.fwd_class(*c)["kernel"] == ("lds" if c in R.FWD_LDS_CASES else "elem")
    x = R.fwd_input(c)
    ref, bound = R.fwd_expected(c)
    rc, out = run_fwd(c, x)
    assert rc == 0, rc
    assert out.guards_intact(), "a word in front of or behind the output was written"
    got = out.values(ref.shape)
    r = R.ratio(got, ref, bound)
    print(f"\nRATIO fwd:{R.case_id(c)}  {r:.3f}")
    within(f"resize:fwd:{R.case_id(c)}", r, 1.0)
    if c in R.IDENTITY_CASES:
        assert np.array_equal(_bits(got), _bits(x)), "same size in, same size out: a copy, bit for bit"
    rc, again = run_fwd(c, x)
    assert rc == 0 and np.array_equal(again.bits(), out.bits()), "two launches differ"


@pytest.mark.parametrize("c", R.ADJ_CASES, ids=R.case_id)
def test_adjoint(c):
    assert R.adj_class(*c)["kernel"] == ("sep" if c in R.ADJ_SEP_CASES else "elem")
    g = R.adj_input(c)
    ref, bound = R.adj_expected(c)
    rc, out = run_adj(c, g)
    assert rc == 0, rc
    assert out.guards_intact(), "a word in front of or behind the output was written"
    got = out.values(ref.shape)
    r = R.ratio(got, ref, bound)
    print(f"\nRATIO adj:{R.case_id(c)}  {r:.3f}")
    within(f"resize:adj:{R.case_id(c)}", r, 1.0)
    if c in R.IDENTITY_CASES:
        assert np.array_equal(_bits(got), _bits(g))
    rc, again = run_adj(c, g)
    assert rc == 0 and np.array_equal(again.bits(), out.bits()), "two launches differ"


# ================================================================================================ 2. exact cases
@pytest.mark.parametrize("kind", R.DYADIC_KINDS)
@pytest.mark.parametrize("c", R.DYADIC_CASES, ids=R.case_id)
def test_dyadic_cases_are_exact(c, kind):
    """every weight, product and sum is exact in f32: no rounding to allow for, in either direction, ties at 0.5 included"""
    ref, _ = R.fwd_expected(c, kind)
    rc, out = run_fwd(c, R.fwd_input(c, kind))
    assert rc == 0 and out.guards_intact()
    got = out.values(ref.shape)
    assert np.array_equal(got.astype(np.float64), ref), ("forward", int((got != ref).sum()))
    if kind == "mask":
        assert np.array_equal(got > 0.5, ref > 0.5)
    ref, _ = R.adj_expected(c, kind)
    rc, out = run_adj(c, R.adj_input(c, kind))
    assert rc == 0 and out.guards_intact()
    got = out.values(ref.shape)
    assert np.array_equal(got.astype(np.float64), ref), ("adjoint", int((got != ref).sum()))


# ================================================================================================ 3. the adjoint is the transpose
@pytest.mark.parametrize("c", R.ADJ_CASES, ids=R.case_id)
def test_adjoint_is_the_transpose(c):
    x, y = R.fwd_input(c).astype(np.float64), R.adj_input(c).astype(np.float64)
    _, bf = R.fwd_expected(c)
    _, ba = R.adj_expected(c)
    rc, ux = run_fwd(c, R.fwd_input(c))
    assert rc == 0
    rc, uty = run_adj(c, R.adj_input(c))
    assert rc == 0
    lhs = float((ux.values(y.shape).astype(np.float64) * y).sum())
    rhs = float((x * uty.values(x.shape).astype(np.float64)).sum())
    tol = float((bf * np.abs(y)).sum() + (ba * np.abs(x)).sum())
    print(f"\nRATIO transpose:{R.case_id(c)}  {abs(lhs - rhs) / tol:.4f}")
    within(f"resize:transpose:{R.case_id(c)}", abs(lhs - rhs) / tol, 1.0)


# ================================================================================================ 4. thresholds
@pytest.mark.parametrize("c", R.THRESHOLD_CASES, ids=R.case_id)
def test_thresholds_of_resized_masks(c):
    """loop_look_twice.py:399 / loop_CORAL.py:128: a 0/1 prediction resized to a label's own size and cut at > 0.5.  Where the model is further than 2^-20
    from 0.5 the cut is the model's; exact ties (the rest) are decided by the blend's rounding, which the dyadic and the ATen bit-for-bit tests pin."""
    x = R.fwd_input(c, "mask")
    ref, bound = R.fwd_expected(c, "mask")
    rc, out = run_fwd(c, x)
    assert rc == 0 and out.guards_intact()
    got = out.values(ref.shape)
    within(f"resize:mask:{R.case_id(c)}", R.ratio(got, ref, bound), 1.0)
    wrong, share = R.threshold_compare(got, ref, 0.5)
    print(f"\nSHARE threshold:{R.case_id(c)}  compared {share:.4f}  wrong {wrong}")
    assert share >= R.THRESHOLD_SHARE, share
    assert wrong == 0, wrong
    rc, cut = run_binarize(got, logits=False)
    assert rc == 0 and cut.guards_intact()
    assert np.array_equal(cut.values(ref.shape), (got > 0.5).astype(np.float32)), "ucod_binarize is not > 0.5"


# ================================================================================================ 5. binarize
def test_binarize_special_values():
    x = R.binarize_specials()
    for logits in (False, True):
        want, decided = R.binarize_ref(x, logits)
        rc, out = run_binarize(x, logits)
        assert rc == 0 and out.guards_intact()
        got = out.values(x.shape)
        assert set(np.unique(got)) <= {0.0, 1.0}
        assert np.array_equal(got[decided], want[decided]), (logits, x[decided][got[decided] != want[decided]])
        assert np.array_equal(_bits(got[decided]), _bits(want[decided])), "a -0.0 or a NaN where 0.0 belongs"


def test_binarize_sweeps():
    """logits = 0: exactly x > 0.5 around the threshold, ulp by ulp.  logits = 1: 1 for every x >= 2^-20 and 0 for every x <= 0; nothing is asserted
    between, where the rounding of 1 / (1 + expf(-x)) decides."""
    half = np.float32(0.5)
    near = [half]
    for _ in range(64):
        near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(1))]
    g = np.random.default_rng(11)
    x = np.concatenate([np.array(near, dtype=np.float32), g.standard_normal(5000, dtype=np.float32) * 0.5 + 0.5, g.random(5000, dtype=np.float32)])
    want, _ = R.binarize_ref(x, False)
    rc, out = run_binarize(x, False)
    assert rc == 0 and out.guards_intact() and np.array_equal(out.values(x.shape), want)
    pos = np.geomspace(R.THRESHOLD_MARGIN, 3e38, 4000).astype(np.float32)
    pos[0] = np.float32(R.THRESHOLD_MARGIN)
    neg = -np.concatenate([np.geomspace(1e-45, 3e38, 4000), [0.0]]).astype(np.float32)
    x = np.concatenate([pos, neg, g.standard_normal(5000, dtype=np.float32) * 4])
    want, decided = R.binarize_ref(x, True)
    rc, out = run_binarize(x, True)
    assert rc == 0 and out.guards_intact()
    got = out.values(x.shape)
    assert set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got[decided], want[decided]), x[decided][got[decided] != want[decided]][:8]


def test_binarize_lengths():
    """n = 0 is no launch; 4096 x 256 + 77 elements take 77 threads into a second trip of the grid stride; 1 and 257: a ragged workgroup"""
    rc, out = run_binarize(np.ones(8, dtype=np.float32), False, n=0)
    assert rc == 0 and out.untouched()
    g = np.random.default_rng(12)
    for n in (1, 257, R.BINARIZE_LONG):
        x = g.standard_normal(n, dtype=np.float32)
        for logits in (False, True):
            want, decided = R.binarize_ref(x, logits)
            rc, out = run_binarize(x, logits)
            assert rc == 0 and out.guards_intact(), (n, logits)
            got = out.values(x.shape)
            assert np.array_equal(got[decided], want[decided]), (n, logits)
            assert decided.mean() > 0.999


# ================================================================================================ 6. resize, then binarize the logits
def test_resize_then_binarize_logits():
    """loop_look_twice.py:214,227: binarize(resize(logits), logits=True) is (model > 0) wherever the model is further than 2^-20 from 0"""
    c = R.COMPOSITION_CASE
    ref, _ = R.fwd_expected(c)
    rc, up = run_fwd(c, R.fwd_input(c))
    assert rc == 0
    rc, cut = run_binarize(up.values(-1), True)
    assert rc == 0 and cut.guards_intact()
    got = cut.values(ref.shape)
    assert set(np.unique(got)) <= {0.0, 1.0}
    far = np.abs(ref) > R.THRESHOLD_MARGIN
    print(f"\nSHARE composition:{R.case_id(c)}  compared {far.mean():.6f}")
    assert far.mean() >= R.THRESHOLD_SHARE
    assert np.array_equal(got[far] > 0.5, ref[far] > 0)
    assert 0.2 < got.mean() < 0.9                                                # both outcomes occur: the comparison is about something


# ================================================================================================ 7. refusals
def test_refusals():
    lib = N.load()
    c = R.Case(3, 5, 7, 12, 9)
    x, g = device_input(R.fwd_input(c)), device_input(R.adj_input(c))
    up, down = Guarded(c.planes * c.oh * c.ow), Guarded(c.planes * c.ih * c.iw)
    good_f = [N.ptr(x), up.ptr(), c.planes, c.ih, c.iw, c.oh, c.ow]
    good_a = [N.ptr(g), down.ptr(), c.planes, c.ih, c.iw, c.oh, c.ow]
    for fn, good in ((lib.ucod_bilinear_resize, good_f), (lib.ucod_bilinear_resize_adjoint, good_a)):
        for k in range(len(good)):
            for bad in ((None,) if k < 2 else (0, -1, -2 ** 31)):
                args = list(good)
                args[k] = bad
                assert fn(*args, N.stream()) == EINVAL, (fn.__name__, k, bad)
    for r in R.ADJ_REFUSED:                                                       # more than 16 taps on an axis
        assert R.adj_class(*r)["kernel"] == "refused"
        gr = device_input(R.adj_input(r))
        out = Guarded(r.planes * r.ih * r.iw)
        assert lib.ucod_bilinear_resize_adjoint(N.ptr(gr), out.ptr(), r.planes, r.ih, r.iw, r.oh, r.ow, N.stream()) == EINVAL, r
        torch.cuda.synchronize()
        assert out.untouched(), r
    cut = Guarded(64)
    assert lib.ucod_binarize(None, cut.ptr(), 64, 0, N.stream()) == EINVAL
    assert lib.ucod_binarize(N.ptr(x), None, 64, 1, N.stream()) == EINVAL
    assert lib.ucod_binarize(None, None, 0, 0, N.stream()) == EINVAL
    torch.cuda.synchronize()
    assert up.untouched() and down.untouched() and cut.untouched()
    # the stream carries nothing over from the refusals: the same calls, valid, are right
    assert lib.ucod_bilinear_resize(*good_f, N.stream()) == 0 and lib.ucod_bilinear_resize_adjoint(*good_a, N.stream()) == 0
    torch.cuda.synchronize()
    assert R.ratio(up.values((c.planes, c.oh, c.ow)), *R.fwd_expected(c)) < 1 and R.ratio(down.values((c.planes, c.ih, c.iw)), *R.adj_expected(c)) < 1
    assert up.guards_intact() and down.guards_intact()
