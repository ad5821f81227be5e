"""Exact-arithmetic cases for the 16-bit MFMA GEMM (ucod_dpl_amd/csrc/gemm_bf16.hip, gemm_bf16_tiles.h, gemm_bf16_epilogue.h), shared by
tests/test_gemm_exact_host.py (CPU) and tests/test_gpu_gemm_exact.py.

A GEMM is the one kernel whose reference can be exact.  With A integers in [-amp, amp] and W integers in [-amp, amp] times 2^-grid_bits, every product is a
multiple of u = 2^-grid_bits; the bias, the residual and the position rows are multiples of u * 2^-fine_bits.  While every partial sum -- in ANY order of the
additions over K, the bias in front of the sum or behind it -- stays below 2^24 of the finest unit, each of them is representable in the f32 accumulator and
f32 arithmetic makes no rounding at all: tile path, patch path (8 interleaved partials) and every drain must give the SAME bits, and the one rounding that
remains -- the f32 value to a bf16 / fp16 output -- is round-to-nearest-even of the exact value.  No tolerance is needed, and a drain or schedule change is
judged by equality.  (The scale 2^-grid_bits sits on one operand only: on both, products would lie on 2^-(2 grid_bits) and the 2^24 condition would have to
be stated for that unit.)

exact_case() refuses a case that breaks these conditions, so that no test passes on a case that was never exact:
    (|A| |W|^T + |bias|).max() / unit < 2^24        for the sum itself, and the same with the column scale (|s| < 4, scale_bits more unit bits) and the
                                                    residual / position row for each reference it hands out (Case.ref);
    representable_refs:  ref.to(out_dtype) == ref   (epilogues that combine 16-bit values);
    rounding_refs:       at least half of the reference elements are NOT representable in out_dtype -- what pins the rounding mode.

plan() mirrors the variant selection of launch() / gemm_entry() in gemm_bf16.hip and big_plan() / mixed_plan() of gemm_bf16_plan.h (and launch_lab() of
variants/gemm_bf16_lab.hip for the laboratory variants): it says which kernel a (kind, shape, variant) launches, so that every GPU case can state the path
it is meant to reach and fail loudly when the shape has drifted off it.  IT MUST MOVE WITH THOSE FILES.
"""
import collections
import math

import torch

TWO24 = float(1 << 24)
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}                 # significand bits, the implicit one included
EMIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}           # exponent of the smallest normal number
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ cases
class Case:
    """Operands as small CPU integer tensors (A_int, W_int: int8) and the grid they sit on; bias [N], rowbias [M] (the key hook's per-channel bias), scale [N],
    resid [M, N], pos [pos_rows, N] as f64 CPU tensors; acc = A W^T in f64 on `device`.  Nothing here is ever modified by a test."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._refs = {}

    @property
    def resid(self):
        if "_resid" not in self.__dict__:
            self._resid = self._make_resid()
        return self._resid

    def operands(self, dtype, device):
        """(A, W) in the operand type: exact (asserted)."""
        A = self.A_int.to(device).to(dtype)
        W = (self.W_int.to(device).double() * 2.0 ** -self.grid_bits).to(dtype)
        assert bool((A.double() == self.A_int.to(device).double()).all()) and bool((W.double() * 2.0 ** self.grid_bits == self.W_int.to(device).double()).all())
        return A, W

    def _legit(self, what, mag, unit_bits):
        assert mag * 2.0 ** unit_bits < TWO24, f"{what}: |partial sums| up to {mag} in units of 2^-{unit_bits} exceed 2^24: the case is not exact in f32"

    def ref(self, epi):
        """f64 reference [M, N] on self.device of: 'plain' A W^T | 'bias' + bias | 'scale' (A W^T + bias) * scale | 'resid' resid + scale * (A W^T + bias) |
        'pos' (A W^T + bias) + pos[1 + m % (pos_rows - 1)] | 'rowbias' A W^T + rowbias[m].  Each one asserts the bound that makes its f32 evaluation exact."""
        if epi in self._refs:
            return self._refs[epi]
        dev, ub = self.device, self.grid_bits + self.fine_bits
        acc = self.acc
        if epi == "plain":
            self._legit(epi, self.mag_plain, self.grid_bits)
            r = acc
        elif epi == "bias":
            self._legit(epi, self.mag, ub)
            r = acc + self.bias.to(dev)
        elif epi == "rowbias":
            self._legit(epi, self.mag_plain + float(self.rowbias.abs().max()), ub)
            r = acc + self.rowbias.to(dev)[:, None]
        elif epi == "pos":
            self._legit(epi, self.mag + float(self.pos.abs().max()), ub)
            npatch = self.pos.shape[0] - 1
            assert self.M % npatch == 0
            r = ((acc + self.bias.to(dev)).view(-1, npatch, self.N) + self.pos[1:].to(dev)).view(self.M, self.N)
        elif epi in ("scale", "resid"):
            smax = float(self.scale.abs().max())
            self._legit(epi, smax * self.mag + (float(self.resid.abs().max()) if epi == "resid" else 0.0), ub + 1 + self.scale_bits)
            r = (acc + self.bias.to(dev)) * self.scale.to(dev)
            if epi == "resid":
                r = self.resid.to(dev) + r
        else:
            raise KeyError(epi)
        self._refs[epi] = r
        return r


def representable(ref, dtype):
    """Boolean mask: ref (f64) survives a round trip through dtype."""
    return ref.to(dtype).double() == ref


def exact_case(M, N, K, seed, grid_bits=0, amp=4, out_dtype=torch.float32, fine_bits=0, scale_bits=0, resid_amp=64, pos_rows=0, representable_refs=(),
               rounding_refs=(), device="cpu"):
    """A, W integers in [-amp, amp], W times 2^-grid_bits; bias / rowbias = (integer in [-amp, amp] + j / 2^fine_bits) * 2^-grid_bits; resid and pos the same with
    integers in [-resid_amp, resid_amp] / [-amp, amp]; column scales from {+-0.5, +-1, +-2}, times (1 + j / 2^scale_bits) when scale_bits > 0 (then no bf16 value:
    a scale rounded to 16 bits shows).  Everything is drawn from one seeded CPU generator; A W^T is an f64 matmul (exact: asserted below through the 2^24
    bound, which is far inside f64's 2^53) on `device`.
    representable_refs: names of Case.ref() that must be representable in out_dtype; rounding_refs: names of which at least half must NOT be."""
    assert K % 64 == 0 and amp <= 64
    g = torch.Generator().manual_seed(seed)
    u = 2.0 ** -grid_bits

    def ints(shape, a):
        return torch.randint(-a, a + 1, shape, generator=g)

    def fine(shape, a):
        f = torch.randint(0, 1 << fine_bits, shape, generator=g).double() * 2.0 ** -fine_bits if fine_bits else 0.0
        return (ints(shape, a).double() + f) * u
    A_int, W_int = ints((M, K), amp).to(torch.int8), ints((N, K), amp).to(torch.int8)
    bias, rowbias = fine((N,), amp), fine((M,), amp)
    scale = torch.tensor(SCALES, dtype=torch.float64)[torch.randint(0, len(SCALES), (N,), generator=g)]
    if scale_bits:
        scale = scale * (1.0 + torch.randint(0, 1 << scale_bits, (N,), generator=g).double() * 2.0 ** -scale_bits)
    pos = fine((pos_rows, N), amp) if pos_rows else None

    def make_resid():                                                # (on first use, from a generator of its own: the largest cases never ask for it)
        nonlocal g
        g = torch.Generator().manual_seed(seed + 0x5EED)
        return fine((M, N), resid_amp)
    Ad, Wd = A_int.to(device).double(), W_int.to(device).double() * u
    acc = Ad @ Wd.t()
    # max of |A| |W|^T: the matmul itself where that is cheap, else the smaller of the two rigorous bounds  max_m sum_k |a_mk| * max |w|  and its mirror
    if M * N * K <= 4e9:
        mag_plain = float((Ad.abs() @ Wd.abs().t()).max())
    else:
        mag_plain = min(float(Ad.abs().sum(1).max()) * float(Wd.abs().max()), float(Wd.abs().sum(1).max()) * float(Ad.abs().max()))
    assert float(acc.abs().max()) <= mag_plain
    c = Case(M=M, N=N, K=K, seed=seed, grid_bits=grid_bits, fine_bits=fine_bits, scale_bits=scale_bits, amp=amp, A_int=A_int, W_int=W_int, bias=bias,
             rowbias=rowbias, scale=scale, _make_resid=make_resid, pos=pos, acc=acc, device=device, mag_plain=mag_plain, mag=mag_plain + float(bias.abs().max()))
    c._legit("sum", c.mag, grid_bits + fine_bits)                  # bounds every partial sum in every order
    for name in representable_refs:
        r = c.ref(name)
        assert bool(representable(r, out_dtype).all()), f"{name}: declared representable in {out_dtype}, is not"
    for name in rounding_refs:
        r = c.ref(name)
        frac = float((~representable(r, out_dtype)).double().mean())
        assert frac >= 0.5, f"{name}: only {frac:.2f} of the reference needs a rounding to {out_dtype}: the case does not pin the rounding mode"
    return c


# ================================================================================================ checkers
def check_exact(out, ref, dtype, what=""):
    """out == RNE(ref) to dtype, bit for bit (f32 outputs: ref.float()).  On failure: how many elements are wrong and the first few (row, col, got, want), with
    the row inside a 256- and a 288-row tile and the column inside a 32-column patch / wave quarter -- the tile-local position usually names the culprit."""
    assert out.dtype == dtype, (out.dtype, dtype)
    want = ref.to(dtype)
    assert want.shape == out.shape, (want.shape, out.shape)
    if torch.equal(out, want.to(out.device)):
        return
    o, w = out.detach().cpu(), want.cpu()
    bad = (o != w) | (o.isnan() != w.isnan())
    idx = bad.reshape(o.shape[0], -1).nonzero()
    ncol = bad.reshape(o.shape[0], -1).shape[1]
    lines = []
    for r, cidx in idx[:8].tolist():
        lines.append(f"  (row {r}, col {cidx}) got {o.reshape(o.shape[0], -1)[r, cidx].item()!r} want {w.reshape(o.shape[0], -1)[r, cidx].item()!r}"
                     f"  [row % 256 = {r % 256}, row % 288 = {r % 288}, col % 32 = {cidx % 32}]")
    rows, cols = idx[:, 0], idx[:, 1]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exactly rounded reference ({ncol} columns); rows {int(rows.min())}.."
                         f"{int(rows.max())}, cols {int(cols.min())}..{int(cols.max())}; distinct row % 256: {sorted(set((rows % 256).tolist()))[:16]}, "
                         f"distinct col % 32: {sorted(set((cols % 32).tolist()))[:16]}\n" + "\n".join(lines))


def half_ulp(v, dtype):
    """Half an ulp of dtype at magnitude v (f64 tensor, >= 0): 2^(floor(log2 v) - significand bits), with the exponent held at the smallest normal one."""
    _, e = torch.frexp(v)                                            # v = m 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    e = torch.clamp(e.to(torch.float64) - 1.0, min=float(EMIN[dtype]))
    return torch.exp2(e - MANT[dtype])


def gelu_f64(x):
    """erf-GELU x Phi(x) in f64 (transformers ACT2FN["gelu"]); erfc keeps the relative accuracy of the negative tail."""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x * (1.0 / math.sqrt(2.0)))


def gelu_tolerance(x):
    """E = 1e-6 + 2^-22 |x|: the documented 7.1e-7 of gelu_erf2 (gemm_bf16_epilogue.h) rounded up for the f32 operations around the fit -- the last
    subtraction max(x, 0) - |x| t alone rounds at 2^-24 |x|.  Not a number tuned on the GPU."""
    return 1e-6 + 2.0 ** -22 * x.double().abs()


def check_gelu(out, x_exact, dtype, what=""):
    """|out - gelu(x)| <= E + half_ulp_dtype(|gelu(x)| + E) per element, x the EXACT pre-activation (f64)."""
    assert out.dtype == dtype, (out.dtype, dtype)
    x = x_exact.double()
    g, E = gelu_f64(x), gelu_tolerance(x)
    err = (out.to(x.device).double() - g).abs()
    bound = E + half_ulp(g.abs() + E, dtype)
    bad = ~(err <= bound)                                            # (a NaN fails)
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    lines = [f"  (row {r}, col {c}) x {x[r, c].item()!r} got {out[r, c].item()!r} want {g[r, c].item()!r} bound {bound[r, c].item():.3e}"
             f"  [row % 256 = {r % 256}, row % 288 = {r % 288}, col % 32 = {c % 32}]" for r, c in idx[:8].tolist()]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements miss the GELU bound; worst error / bound {float((err / bound).max()):.3f}\n" + "\n".join(lines))


def gelu_erf2_f32(x):
    """gelu_erf2 of gemm_bf16_epilogue.h transcribed operation by operation in torch f32 (separate multiply and add where the kernel's packed FMA rounds once:
    the transcription rounds MORE often than the kernel)."""
    x = x.float()
    pos = torch.clamp(x, min=0.0)
    a = pos * 2.0 - x
    p = a * 4.881021588e-04 + (-7.198718842e-03)
    for c in (5.214663086e-02, 4.595958292e-01, 1.151000509e+00, 1.0):
        p = p * a + c
    return pos - a * torch.exp2(-p)


# ================================================================================================ launch-plan mirror
KINDS = {  # kind -> (column-fused drain, 16-bit output rows (N % 8), row-mapped, bias-like or GELU)
    "bias16": (True, True, False, True), "gelu16": (True, True, False, True), "bias32": (True, False, False, False), "resid32": (True, False, False, False),
    "resid16": (True, False, False, False), "patch32": (False, False, True, False), "patch16": (False, False, True, False), "key32": (False, False, True, False)}
Plan = collections.namedtuple("Plan", "path patches_per_wg n_tall")
REFUSED = Plan("refused", 0, 0)


def big_plan(M, N, K, bn, n_cu, patch_epi=True, no_patch=False, patch_rounds=2):
    """gemm_bf16_plan.h: big_plan -> (patches, cost, rounds, left, patches per leftover tile)."""
    total = cdiv(M, 256) * cdiv(N, bn)
    rounds = total // n_cu
    left = total - rounds * n_cu
    ppt = 16 * (bn // 32)
    patches = patch_epi and not no_patch and 1 <= rounds <= patch_rounds and left > 0 and left * ppt <= 2 * rounds * n_cu and (K & 31) == 0
    tile = 0.45 * 256 + 0.55 * bn
    fill = left / n_cu
    plain = (rounds + ((0.4 + 0.6 * fill) if left else 0.0)) * tile
    patched = rounds * tile * 1.08
    if patches and patched >= plain:
        patches = False
    return patches, (patched if patches else plain), rounds, left, ppt


def mixed_plan(M, N, bn, n_cu):
    """gemm_bf16_plan.h: mixed_plan -> (feasible, row-tiles, tall ones, whole rounds)."""
    tiles_n = cdiv(N, bn)
    t0 = cdiv(M, 256) * tiles_n
    rounds = t0 // n_cu
    if rounds < 1 or t0 == rounds * n_cu:
        return False, 0, 0, 0
    tm = (rounds * n_cu) // tiles_n
    short_rows = M - 256 * tm
    if tm < 1 or short_rows <= 0:
        return False, 0, 0, 0
    n_tall = cdiv(short_rows, 32)
    if n_tall > tm:
        return False, 0, 0, 0
    return True, tm, n_tall, rounds


def plan(kind, M, N, K, variant, n_cu, tok=0, n_reg=0, has_bias=True, no_patch=False, no_mixed=False, patch_rounds=2):
    """Which kernel ucod_gemm_bf16 / ucod_gemm_bf16_reg (variants 0, 1, 2, 9, 10, 12, 13, 14) or ucod_gemm_bf16_lab (3..8) launches:
    Plan(path, patches_per_wg, n_tall) with path one of t64, t128, big256, big192, big256+patches, big192+patches, mixed256, mixed192 (laboratory 7 / 8:
    pers256 / pers192), or 'refused' (UCOD_EINVAL).  kind: a key of KINDS.  Mirrors gemm_bf16_plan.h and launch() / gemm_entry() of gemm_bf16.hip."""
    col_fused, out16, row_mapped, biaslike = KINDS[kind]

    def cheaper():
        return 10 if big_plan(M, N, K, 192, n_cu, True, no_patch, patch_rounds)[1] < big_plan(M, N, K, 256, n_cu, True, no_patch, patch_rounds)[1] else 9

    def big(v):
        bn = 256 if v == 9 else 192
        patches, _, rounds, left, ppt = big_plan(M, N, K, bn, n_cu, True, no_patch, patch_rounds)
        return Plan(f"big{bn}+patches", cdiv(left * ppt, rounds * n_cu), 0) if patches else Plan(f"big{bn}", 0, 0)
    if M <= 0 or N <= 0 or K <= 0 or K % 64 != 0 or n_reg < 0:
        return REFUSED
    if 3 <= variant <= 8:                                           # launch_lab (epilogues 0..5)
        if kind in ("resid16", "patch16") or (N & 3) != 0 or (kind in ("bias16", "gelu16") and (N & 7) != 0):
            return REFUSED
        if variant >= 7:
            return Plan("pers256" if variant == 7 else "pers192", 0, 0)
        return big(9 if variant in (3, 5) else 10)
    if kind in ("bias16", "bias32") and not has_bias and (variant in (1, 2, 12) or K < 128 or (N & 3) != 0):
        return REFUSED
    if row_mapped and tok < 2 + n_reg:
        return REFUSED
    if kind == "resid16":
        if M >= 2048 and K >= 128 and (N & 7) == 0 and M * K * 2 < (1 << 32) and N * K * 2 < (1 << 32):   # launch_resid_h16: always the mixed-height kernel
            feasible, _, n_tall, _ = mixed_plan(M, N, 256, n_cu)
            return Plan("mixed256", 0, n_tall if feasible else 0)
        variant = variant if variant in (0, 1, 2, 12) else 0
    auto_small = variant == 0
    if variant == 0:
        variant = 2
        if (M >= 2048 or (M >= 512 and M * N >= (1 << 24))) and K >= 128 and (N & 3) == 0 and (not biaslike or (N & 7) == 0):
            variant = cheaper()
            feasible, _, _, rounds = mixed_plan(M, N, 256, n_cu)
            if col_fused and feasible and rounds >= 3 and not no_mixed:
                variant = 13
    if kind in ("bias16", "bias32") and not has_bias and variant < 3:
        variant = cheaper()
    if variant == 11 or variant > 14 or variant < 0:
        return REFUSED
    if variant in (9, 10, 13, 14) and ((N & 3) != 0 or (out16 and (N & 7) != 0)):
        return REFUSED
    if variant in (13, 14):
        bn = 256 if variant == 13 else 192
        feasible, _, n_tall, _ = mixed_plan(M, N, bn, n_cu)
        fits32 = M * K * 2 < (1 << 32) and N * K * 2 < (1 << 32)
        if col_fused and feasible and fits32 and (N & 3) == 0 and not (out16 and (N & 7) != 0) and K >= 128:
            return Plan(f"mixed{bn}", 0, n_tall)
        variant -= 4
    if row_mapped and variant == 9:
        np_ = tok - 1 - n_reg
        if kind == "key32":
            out_bytes, whole = (N // tok) * M * np_ * 4, N % tok == 0
        else:
            out_bytes, whole = (M // np_) * tok * N * (2 if kind == "patch16" else 4), M % np_ == 0
        if not (whole and out_bytes < 0x7FFFFFF0 and tok * N * 4 < 0x7FFFFFF0 and (kind != "patch16" or (N & 7) == 0)):
            variant = 10
    if variant in (9, 10):
        return big(variant)
    t128 = cdiv(M, 128) * cdiv(N, 128)
    return Plan("t64" if variant == 12 or (variant == 2 and auto_small and t128 < n_cu) else "t128", 0, 0)


# ================================================================================================ the case families of the two test files
def family(name, K, out_dtype=torch.float32):
    """Keyword arguments of exact_case() for a family of epilogues at depth K (both test files draw their cases from here):
    f32      f32 outputs: bias / residual with 7 (K <= 768) or 6 fine bits -- neither a bf16 nor (the residual, +-4096) an fp16 value, so a 16-bit detour shows;
    h16      16-bit outputs: bf16 amp 8 up to K = 192 and amp 4 from K = 768, fp16 amp 32 / 16 / 8 with 5 / 4 / 3 fine bits (sums beyond the type's exact-integer
             range, 256 / 2048): at least half of the reference needs a real rounding (asserted);
    resid16  the fp16 residual stream: amp 1 and a residual within +-64, every reference value an fp16 number (asserted);
    gelu     grid 2^-6, amp 4: pre-activations spread over a few units either side of zero;
    wscale   column scales with 9 fraction bits (not bf16 values), amp 2: the product (sum + bias) * scale still fits 24 bits."""
    fb = 7 if K <= 768 else 5
    if name == "f32":
        return dict(amp=4, fine_bits=max(fb, 6), resid_amp=4096, out_dtype=torch.float32)
    if name == "h16":
        if out_dtype == torch.float16:                             # (11 bits: the sums themselves must pass 2048 for a 16-bit accumulator to show)
            amp, fb16 = (32, 5) if K <= 192 else (16, 4) if K <= 768 else (8, 3)
            return dict(amp=amp, fine_bits=fb16, out_dtype=out_dtype, rounding_refs=("bias", "scale"))
        return dict(amp=8 if K <= 192 else 4, fine_bits=fb, out_dtype=out_dtype, rounding_refs=("bias", "scale"))
    if name == "resid16":
        return dict(amp=1, resid_amp=64, out_dtype=torch.float16, representable_refs=("resid",))
    if name == "gelu":
        return dict(grid_bits=6, amp=4, out_dtype=out_dtype)
    if name == "wscale":
        return dict(amp=2, scale_bits=9, resid_amp=4096, out_dtype=out_dtype, rounding_refs=("scale",) if out_dtype != torch.float32 else ())
    raise KeyError(name)
