"""CPU reference, rounding model, dispatch restatement, case lists, inputs and checker for the LoRA row kernels of csrc/vit_train.hip: ln_lora_kernel /
ln_lora4_kernel (ucod_layernorm_lora, _lora_h16, _lora_mlp), ln_bwd_kernel (ucod_layernorm_bwd, _bwd_ex, _bwd_lora, _bwd_lora_ex, _bwd_lora_mlp),
key_grad_tokens_kernel, lora_pack_kernel and lora_grad_kernel with its reduce.

Test infrastructure only: nothing here is the code under test, and nothing here reads GPU output to set a bound.

Formulas (the kernel headers), every sum in f64, on the values the kernel reads (dy and t already rounded to bf16, x to fp16 where the entry takes fp16):

    y    = LN(x) = (x - mean x) * rstd * gamma + beta,   rstd = 1 / sqrt(var x + eps)                       x^ = (x - mean x) * rstd
    u_p  = (y * mask_p) A_p^T                            p = 0..NP-1 (q, k, v; or the one MLP module), mask_p in {0, 1 / (1 - T / 1024)}
    dy' = dy + sum_p mask_p * (t_p A_p);   g = dy' * gamma;   dx = rstd * (g - mean g - x^ * mean(g x^)) + dres;   s = next_scale * dx
    t_p  = scaling * dqkv_p B_p;   dA_p = t_p^T (h * mask_p);   dB_p = scaling * dqkv_p^T u_p

Rounding model: the same with a rounding only where the kernel rounds -- y, u, s, t to bf16; dx and the gradients of lora_grad to f32.
"""
import collections
import functools
import math

import torch

from conftest import within
from oracle import vit as OV

AUG = 64                # UCOD_LORA_AUG
MLP_MAX_R = 8           # UCOD_LORA_MLP_MAX_R
EPS = 1e-6
F = 2.0                 # kernel error / model error on a bf16 output, both against the f64 reference (attn_bwd_ref.F: same constant, same argument)
DX_TOL, GRAD_TOL = 2e-5, 2e-4       # test_gpu_vit_train.py: test_layernorm_bwd / test_lora_grad, relative to max(1, |ref|max) -- here per row
LDS_ASK = 64 * 1024     # a launch gets more dynamic LDS than this only after asking (hipFuncAttributeMaxDynamicSharedMemorySize)
LDS_GFX950 = 160 * 1024  # one workgroup's LDS on gfx950 (the library queries its device; the table below is for that chip)
T_FILL = 55.0           # what the t columns past the rank hold: never to be read
ROWS = (1, 5, 37)
SEED = 0x1234567887654321


# ================================================================================================ arithmetic
def bf16_round(x):
    return x.to(torch.bfloat16).double()


def f32_round(x):
    return x.float().double()


def _exact(x):
    return x


def layer_norm_stats(x, eps=EPS):
    """x f64 [rows, D] -> (x^, rstd [rows, 1])"""
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    return (x - mean) * rstd, rstd


def drop_threshold(p):
    """T = floor(1024 p) of the f32 p the struct carries, clamped at 1023 (make_drop)"""
    return min(int(float(torch.tensor(p, dtype=torch.float32)) * 1024.0), 1023)


def masks(drop, rows, D, n_proj):
    """one [rows, D] f64 mask per projection from oracle.vit.lora_dropout_mask; ``drop`` = (p, seed, layer) or None (all ones)"""
    if drop is None or drop_threshold(drop[0]) == 0:
        return [torch.ones(rows, D, dtype=torch.float64) for _ in range(n_proj)]
    p, seed, layer = drop
    return [OV.lora_dropout_mask(seed, layer, proj, rows, D, p).double() for proj in range(n_proj)]


def ln_lora(x, gamma, beta, A, drop, rnd=_exact):
    """x [rows, D], A = list of NP [r, D] matrices -> {"y": [rows, D], "u": [rows, NP r]}.  The kernel projects its unrounded f32 y."""
    xh, _ = layer_norm_stats(x.double())
    y = xh * gamma.double() + beta.double()
    m = masks(drop, x.shape[0], x.shape[1], len(A))
    u = torch.cat([(y * m[p]) @ A[p].double().t() for p in range(len(A))], 1)
    return {"y": rnd(y), "u": rnd(u)}


def ln_bwd_closed_form(dy, x, gamma, dres=None):
    """g = dy gamma; dx = rstd (g - mean g - x^ mean(g x^)) + dres, all f64"""
    xh, rstd = layer_norm_stats(x.double())
    g = dy.double() * gamma.double()
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx if dres is None else dx + dres.double()


def ln_bwd(dy, x, gamma, dres, scale, t, A, drop, rnd_dx=_exact, rnd_s=_exact):
    """t [rows, NP r] (or None: the plain form), A = list of NP [r, D] -> {"dx": [rows, D], "s": [rows, D]}; s is formed from the unrounded dx times scale
    (the kernel multiplies its f32 dx, whose rounding is 2^-15 of a bf16 one)."""
    dyl = dy.double()
    if t is not None:
        r = A[0].shape[0]
        m = masks(drop, x.shape[0], x.shape[1], len(A))
        for p in range(len(A)):
            dyl = dyl + m[p] * (t[:, p * r:(p + 1) * r].double() @ A[p].double())
    dx = ln_bwd_closed_form(dyl, x, gamma, dres)
    s = dx if scale is None else dx * scale.double()
    return {"dx": rnd_dx(dx), "s": rnd_s(s)}


def lora_t(dqkv, B, scaling, rnd=_exact):
    """t [rows, 3 r] = scaling * dqkv_p B_p"""
    D = B[0].shape[0]
    return rnd(torch.cat([scaling * dqkv[:, p * D:(p + 1) * D].double() @ B[p].double() for p in range(3)], 1))


def lora_grads(dqkv, h, u, t, scaling, drop, rnd=_exact):
    """(dA [3][r, D], dB [3][D, r]) from the t handed in (the kernel uses the bf16 t it wrote: the callers pass that one, as test_lora_grad does)"""
    rows, D = h.shape
    r = t.shape[1] // 3
    m = masks(drop, rows, D, 3)
    dA = [rnd(t[:, p * r:(p + 1) * r].double().t() @ (h.double() * m[p])) for p in range(3)]
    dB = [rnd(scaling * dqkv[:, p * D:(p + 1) * D].double().t() @ u[:, p * r:(p + 1) * r].double()) for p in range(3)]
    return dA, dB


def key_grad_tokens(dkey, tok, n_reg):
    """dkey f32 [B, D, tok - 1 - n_reg] -> [B, tok, 3 D + 64] bf16: K third = dkey^T behind the CLS and register rows, everything else zero"""
    B, D, hw = dkey.shape
    out = torch.zeros(B, tok, 3 * D + AUG, dtype=torch.bfloat16)
    out[:, 1 + n_reg:, D:2 * D] = dkey.transpose(1, 2).to(torch.bfloat16)
    return out


def lora_pack(mats, r, D, scaling, zero_a):
    """aug columns of Wqkv_aug [3 D, 64] and WqkvT_aug [D, 64] (bf16)"""
    w = torch.zeros(3 * D, AUG, dtype=torch.bfloat16)
    wt = torch.zeros(D, AUG, dtype=torch.bfloat16)
    for p, (A, B) in enumerate(mats):
        w[p * D:(p + 1) * D, p * r:(p + 1) * r] = (torch.tensor(scaling, dtype=torch.float32) * B).to(torch.bfloat16)
        if not zero_a:
            wt[:, p * r:(p + 1) * r] = A.t().to(torch.bfloat16)
    return w, wt


# ================================================================================================ dispatch, restated from the launch functions
LN_BWD_WIDTHS = {256 * n: (n, 4) for n in range(1, 7)}                     # launch_ln_bwd: D % 256 == 0 -> C(D / 256, 4), 1..6
LN_BWD_WIDTHS.update({128 * n: (n, 2) for n in (1, 3, 5, 7, 9, 11)})      # else C(D / 128, 2)
LN_BWD_ENTRIES = {                                                          # entry -> (LORA, the flags it takes; None = it has no flags argument)
    "bwd": (0, (None,)), "bwd_ex": (0, (0, 1, 3)), "bwd_lora": (3, (None,)), "bwd_lora_ex": (3, (0, 1, 3)), "bwd_lora_mlp": (1, (0, 1, 3)),
}
LN_LORA_ENTRIES = {"lora": (3, False), "lora_h16": (3, True), "lora_mlp": (1, False), "lora_mlp_h16": (1, True)}   # entry -> (NP, x is fp16)
LN_LORA_REFUSED_D = (896, 1152, 1408, 1664, 1792)


def ln_bwd_instance(entry, D, flags, r=2):
    """(NCH, VW, LORA, DYB, XH) of the ln_bwd_kernel instantiation the call reaches, or None where the entry or launch_ln_bwd refuses it"""
    lora, allowed = LN_BWD_ENTRIES[entry]
    if flags not in allowed or D <= 0 or D % 128 or D not in LN_BWD_WIDTHS:
        return None
    if lora == 3 and not 1 <= r <= AUG // 3 or lora == 1 and not 1 <= r <= MLP_MAX_R:
        return None
    f = flags or 0
    dyb, xh = bool(f & 1), bool(f & 2)
    if xh and not dyb:
        return None
    return LN_BWD_WIDTHS[D] + (lora, dyb, xh)


def ln_lora_instance(entry, D, r, lds_limit=LDS_GFX950):
    """(kernel, chunks, XH16, NP) of the instantiation launch_ln_lora reaches, or None where it refuses (the product build: no measurement knobs)"""
    np_, xh = LN_LORA_ENTRIES[entry]
    if D <= 0 or D % 128 or r < 1 or np_ * r > AUG or (np_ == 1 and r > MLP_MAX_R) or np_ * r * D * 4 > lds_limit:
        return None
    if D % 256 == 0 and D <= 1536:
        return ("ln_lora4", D // 256, xh, np_)
    if D // 128 in (1, 3, 5):                # (the switch also lists 2, 4, 6, 8, 10, 12: all multiples of 256 up to 1536, which took the branch above)
        return ("ln_lora", D // 128, xh, np_)
    return None                              # 896, 1152, 1408 (7, 9, 11) and everything past 1536


ALL_LN_BWD = frozenset((n, vw, lora, dyb, xh) for n, vw in LN_BWD_WIDTHS.values() for lora in (0, 1, 3) for dyb, xh in ((False, False), (True, False), (True, True)))
ALL_LN_LORA = frozenset((k, n, xh, np_) for k, ns in (("ln_lora4", range(1, 7)), ("ln_lora", (1, 3, 5))) for n in ns for xh in (False, True) for np_ in (3, 1))

# ================================================================================================ cases
FwdCase = collections.namedtuple("FwdCase", "entry D rows r p kind")
BwdCase = collections.namedtuple("BwdCase", "entry flags D rows r dres scale p kind")
GradCase = collections.namedtuple("GradCase", "rows D r p accumulate")

FWD_WIDTHS = (128, 384, 640, 256, 512, 768, 1024, 1280, 1536)
BWD_FORMS = (("bwd", None), ("bwd_ex", 1), ("bwd_ex", 3), ("bwd_lora", None), ("bwd_lora_ex", 0), ("bwd_lora_ex", 1), ("bwd_lora_ex", 3),
             ("bwd_lora_mlp", 0), ("bwd_lora_mlp", 1), ("bwd_lora_mlp", 3))


def _fwd_cases():
    """1. every instantiation: 9 widths x 4 entries x dropout off / 0.3; rows, rank and input kind rotate so that each appears with each width and entry"""
    out, k = [], 0
    for wi, D in enumerate(FWD_WIDTHS):
        for ei, entry in enumerate(LN_LORA_ENTRIES):
            for p in (0.0, 0.3):
                out.append(FwdCase(entry, D, ROWS[k % 3], (2, 1, 3)[(wi + ei) % 3], p, "massive" if (k + wi) % 4 == 1 else "randn"))
                k += 1
    return tuple(out)


def _bwd_cases():
    """3. every instantiation: 12 widths x 10 (entry, flags) forms; rows / dres / next_scale / p / kind rotate"""
    out = []
    for wi, D in enumerate(sorted(LN_BWD_WIDTHS)):
        for fi, (entry, flags) in enumerate(BWD_FORMS):
            k = wi * len(BWD_FORMS) + fi
            p = 0.3 if (wi + fi) % 3 else 0.0
            out.append(BwdCase(entry, flags, D, ROWS[k % 3], 2, bool((k // 3) % 2), bool((wi + fi // 2) % 2), p, "massive" if (k + wi) % 4 == 1 else "randn"))
    return tuple(out)


FWD_CASES = _fwd_cases()
BWD_CASES = _bwd_cases()
# 4. rank: the unrolled branches (1, 2, 4) and the generic loop (everything else), up to the header's limits
RANK_BWD_CASES = tuple(BwdCase("bwd_lora_ex", 1, D, 5, r, True, True, 0.3, "randn") for D in (128, 768) for r in (1, 2, 3, 4, 5, 8, 21)) + \
    tuple(BwdCase("bwd_lora_mlp", 3, D, 5, r, True, False, 0.3, "randn") for D in (128, 768) for r in (1, 2, 3, 4, 8))
RANK_FWD_CASES = tuple(FwdCase("lora", 128, 5, r, 0.3, "randn") for r in (1, 2, 3, 4, 5, 8, 21)) + \
    tuple(FwdCase("lora_mlp", 128, 5, r, 0.3, "randn") for r in (1, 2, 3, 4, 8))
LDS_CASES = ((768, 7), (768, 8), (768, 17), (768, 18), (1024, 6), (1536, 4), (1536, 8), (1536, 9))      # 3 r D 4 bytes around 64 KiB and 160 KiB
# 2. the row walk: 2048 blocks x 4 waves x 2 rows = 16 384 rows per trip
WALK_CASES = tuple(FwdCase("lora", 128, rows, 2, 0.0, "randn") for rows in (1, 2, 7, 8, 9, 16384, 16385, 16393, 32769)) + \
    (FwdCase("lora", 256, 16385, 2, 0.3, "randn"),)
GRAD_CASES = tuple(GradCase(52, 128, r, 0.0, False) for r in (4, 5, 8, 21)) + (GradCase(300, 768, 8, 0.0, False),) + \
    tuple(GradCase(rows, 128, 2, 0.0, False) for rows in (1, 2, 3)) + (GradCase(52, 128, 3, 0.0, True), GradCase(52, 128, 2, 0.3, False), GradCase(37, 256, 5, 0.3, True))


def edge_rows(rows):
    """rows where a wrong row walk would land: first, last, 8 k +- 1 (a block's rows), and the turn of the second trip, 16 383 .. 16 392"""
    cand = [0, 1, rows - 2, rows - 1] + [8 * k + d for k in (1, 2, 1024, 2047, 2048, 2049, 4096) for d in (-1, 0, 1)] + list(range(16383, 16393))
    return sorted({i for i in cand if 0 <= i < rows})


def drop_of(p, layer=3):
    return None if p is None else (p, SEED, layer)


def make_x(rows, D, kind, g):
    """randn * 2 + 0.3 (the existing tests); "massive" sets one channel to 200 (test_layernorm_against_f64's massive-activation row): in the lane's last chunk
    on even rows, its first on odd ones, so a chunk a wrong NCH drops or a wrong mean moves the whole row"""
    x = torch.randn(rows, D, generator=g) * 2 + 0.3
    if kind == "massive":
        x[0::2, D - 3] = 200.0
        x[1::2, 1] = 200.0
    elif kind != "randn":
        raise ValueError(kind)
    return x


def arena(r, D, g, n_proj=3, b_scale=0.05):
    """n_proj = 3: one layer [A_q | B_q | A_k | B_k | A_v | B_v] (test_gpu_vit_train.lora_arena); 1: A_m alone.  -> (flat f32, [(A, B)])"""
    parts, mats = [], []
    for _ in range(n_proj):
        A = torch.randn(r, D, generator=g) / math.sqrt(D)
        B = torch.randn(D, r, generator=g) * b_scale
        parts += [A.reshape(-1)] + ([B.reshape(-1)] if n_proj == 3 else [])
        mats.append((A, B))
    return torch.cat(parts), mats


@functools.lru_cache(maxsize=None)
def fwd_inputs(case):
    """x (fp16-representable where the entry takes fp16), gamma, beta, the flat arena and its matrices; seeded per case"""
    n_proj, xh = LN_LORA_ENTRIES[case.entry]
    g = torch.Generator().manual_seed(case.D * 131 + case.rows * 7 + case.r)
    x = make_x(case.rows, case.D, case.kind, g)
    if xh:
        x = x.to(torch.float16).float()
    gam, bet = torch.randn(case.D, generator=g), torch.randn(case.D, generator=g)
    flat, mats = arena(case.r, case.D, g, n_proj)
    return {"x": x, "gamma": gam, "beta": bet, "flat": flat, "mats": mats}


@functools.lru_cache(maxsize=None)
def fwd_expected(case):
    """(reference, rounding model): computed once, shared, never modified"""
    i = fwd_inputs(case)
    A = [a for a, _ in i["mats"]]
    args = (i["x"], i["gamma"], i["beta"], A, drop_of(case.p))
    return ln_lora(*args), ln_lora(*args, rnd=bf16_round)


@functools.lru_cache(maxsize=None)
def bwd_inputs(case):
    """dy and t bf16-representable, x fp16-representable under UCOD_LNB_X_F16, all held as f32"""
    lora, _ = LN_BWD_ENTRIES[case.entry]
    g = torch.Generator().manual_seed(case.D * 257 + case.rows * 11 + case.r * 3 + (case.flags or 0))
    x = make_x(case.rows, case.D, case.kind, g)
    if (case.flags or 0) & 2:
        x = x.to(torch.float16).float()
    bf = lambda v: v.to(torch.bfloat16).float()                                 # noqa: E731
    out = {"x": x, "gamma": torch.randn(case.D, generator=g), "dy": bf(torch.randn(case.rows, case.D, generator=g)),
           "dres": torch.randn(case.rows, case.D, generator=g) if case.dres else None,
           "scale": torch.rand(case.D, generator=g) + 0.5 if case.scale else None, "t": None, "flat": None, "mats": None}
    if lora:
        out["flat"], out["mats"] = arena(case.r, case.D, g, lora)
        out["t"] = bf(torch.randn(case.rows, lora * case.r, generator=g) * 2)
    return out


@functools.lru_cache(maxsize=None)
def bwd_expected(case):
    i = bwd_inputs(case)
    A = [a for a, _ in i["mats"]] if i["mats"] else None
    args = (i["dy"], i["x"], i["gamma"], i["dres"], i["scale"], i["t"], A, drop_of(case.p))
    return ln_bwd(*args), ln_bwd(*args, rnd_dx=f32_round, rnd_s=bf16_round)


@functools.lru_cache(maxsize=None)
def grad_inputs(case):
    g = torch.Generator().manual_seed(case.rows * 13 + case.D + case.r)
    bf = lambda v: v.to(torch.bfloat16)                                         # noqa: E731
    flat, mats = arena(case.r, case.D, g)
    dqkv, h = bf(torch.randn(case.rows, 3 * case.D, generator=g)), bf(torch.randn(case.rows, case.D, generator=g))
    u = bf(ln_lora_u(h, mats, drop_of(case.p)))
    return {"flat": flat, "mats": mats, "dqkv": dqkv, "h": h, "u": u, "grad0": torch.randn(6 * case.r * case.D, generator=g), "scaling": 2.0}


def ln_lora_u(h, mats, drop):
    m = masks(drop, h.shape[0], h.shape[1], 3)
    return torch.cat([(h.double() * m[p]) @ mats[p][0].double().t() for p in range(3)], 1)


# ================================================================================================ the checker
def bf16_ulp(mag):
    """one bf16 ulp (8 significant bits) at magnitude ``mag`` (f64 tensor); 0 at 0"""
    safe = mag.clamp_min(2.0 ** -126)
    return torch.where(mag > 0, torch.exp2(torch.floor(torch.log2(safe)) - 7), torch.zeros_like(mag))


def row_err(x, ref):
    """largest absolute error per row"""
    return (x.double() - ref).abs().amax(1)


def bf16_row_bound(ref, model, floor=True):
    """per row: F x the model's error, not below one bf16 ulp of the row's largest reference magnitude"""
    b = F * row_err(model, ref)
    return torch.maximum(b, bf16_ulp(ref.abs().amax(1))) if floor else b


def check_bf16(name, got, ref, model, audit=True):
    """every row of a bf16 output: error against f64 <= bf16_row_bound.  The kernel and the model round the same value once, the kernel from an f32
    intermediate: equal in all but the elements whose f32 error straddles a rounding boundary, where the error is the model's plus at most an ulp.
    Returns (largest kernel row error / model row error, largest kernel row error / row bound); the second is what is asserted (<= 1)."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got.double()).all()), (name, "not finite: an element no store reached, or a wrong read")
    e, em, b = row_err(got, ref), row_err(model, ref), bf16_row_bound(ref, model)
    ratio = float(torch.where(em > 0, e / em.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, math.inf), torch.zeros_like(e))).max())
    worst = float(torch.where(b > 0, e / b.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, math.inf), torch.zeros_like(e))).max())
    if audit:
        within(f"lora_rows:{name}:row_error_over_bound", worst, 1.0 + 1e-12)
    else:
        assert worst <= 1.0, (name, worst)
    return ratio, worst


def check_f32(name, got, ref, tol, audit=True):
    """every row of an f32 output: |got - ref| < tol * max(1, |ref row|max).  Returns the largest row error over its bound."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got.double()).all()), (name, "not finite")
    worst = float((row_err(got, ref) / (tol * ref.abs().amax(1).clamp_min(1.0))).max())
    if audit:
        within(f"lora_rows:{name}:row_error_over_bound", worst, 1.0)
    else:
        assert worst < 1.0, (name, worst)
    return worst
