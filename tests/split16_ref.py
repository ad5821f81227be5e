"""Torch restatement of the fp16-term operand split ("split2h", ucod_dpl_amd/csrc/split16.hip): the checker the host and GPU tests of that pass compare against.

    hi = fp16(s v),  lo = fp16(s v - hi)            s a power of two; the subtraction is exact in f32
    |v - (hi + lo) / s| <= max(2^-22 |v|, 2^-25 / s)
    x w^T ~ (x_hi w_hi^T + x_hi w_lo^T + x_lo w_hi^T) / (s_x s_w)

Plain torch on the CPU (f32 for the split, f64 for the sums): nothing here calls the library.
"""
import math

import torch

F16_MAX = 65504.0


def is_pow2(s):
    return s > 0 and math.isfinite(s) and math.frexp(s)[0] == 0.5


def pow2_scale(t, top=14):
    """The power of two that puts max |t| into [2^(top-1), 2^top): the per-tensor rule of the engine's weights and of ops.linear_split(term="f16")."""
    m = float(t.abs().max())
    return 2.0 ** (top - math.frexp(m)[1]) if m > 0 and math.isfinite(m) else 1.0


def split16(v, s):
    """(hi, lo) fp16 tensors of s * v, values beyond fp16's range clamped (the kernels count those)."""
    assert is_pow2(s), s
    t = (v.float() * s).clamp(-F16_MAX, F16_MAX)
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi, lo


def layout(v, s, role):
    """The K-concatenated operand [M, 3 K]: role 0 (A side) hi | hi | lo, role 1 (B side) hi | lo | hi."""
    hi, lo = split16(v, s)
    return torch.cat((hi, hi, lo) if role == 0 else (hi, lo, hi), 1)


def reconstruct(hi, lo, s):
    return (hi.double() + lo.double()) / s


def recon_bound(v, s):
    return torch.maximum(2.0 ** -22 * v.double().abs(), torch.full_like(v, 2.0 ** -25 / s, dtype=torch.float64))


def saturated(v, s):
    """How many elements the kernels would clamp (and count)."""
    return int(((v.float() * s).abs() > F16_MAX).sum())


def linear3(x, w, b, sx, sw):
    """The three-product sum with exact (f64) accumulation and one f32 rounding of the result."""
    xh, xl = (t.double() for t in split16(x, sx))
    wh, wl = (t.double() for t in split16(w, sw))
    acc = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    out = acc / (sx * sw)
    if b is not None:
        out = out + b.double()
    return out.float()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
