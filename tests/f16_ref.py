"""CPU references of the attention kernels (ucod_dpl_amd/csrc/attention.hip) on 16-bit operands, for either operand type of the two builds
(torch.float16: libucod_dpl_f16.so, torch.bfloat16: libucod_dpl.so): the checker tests/test_f16_ref_host.py and tests/test_gpu_f16_kernels.py share.

    attention_ref     softmax(Q K^T) V in f64 on the ALREADY ROUNDED operands: what an exact kernel would return before its one output rounding
    attention_model   the same with the roundings every product kernel makes: exp2(s - rowmax) in f64, the numerator on P rounded to the operand type
                      (through f32, so an fp16 subnormal P keeps the bits the hardware's conversion keeps), the denominator the sum of the UNROUNDED P
                      (attention.hip: sum_pair / psum), the quotient rounded once to the operand type
    accepts           the acceptance rule: a kernel output is taken when its relative L2 error and its largest row error (inf-norm of a row's error, worst
                      row) against attention_ref are at most F times the model's (the relative L2 error also at most F_L2 times).  The model's error is
                      fixed by the number formats, not by any kernel.

Scores are in log2 units.  The pre-scaled-Q forms (ucod_attention_fwd with scale == 0) take Q already multiplied by head_dim^-0.5 log2(e) = C_PRE
(log2_scale = 1); the generic form takes Q as the reference holds it and scale = 0.125 (log2_scale = C_PRE).  The generators below return the 16-bit
operand for either storage of the SAME logical Q.

Plain torch on the CPU: nothing here calls the library.
"""
import math

import torch

C_PRE = 0.125 * math.log2(math.e)
# Acceptance factors.  F is the factor of the rule (both bounds); F_L2 <= F is a tighter one the relative-L2 bound also has to meet.
# The model forms P against the TRUE row maximum, so the heaviest key's P is exactly 1 and carries no rounding error at all.  attn_fwd_v5_kernel and
# attn_fwd_v6_kernel defer the maximum: the running maximum trails the true one by up to 2^8 until a block runs away, P = 2^delta exp2(s - rowmax) with a
# non-integer delta, and the heaviest key is rounded like every other.  That is the whole difference (tests/test_f16_ref_host.py reproduces the measured
# ratios with a trailing maximum on the CPU; rows whose first 32 keys hold the maximum, and the generic kernel, sit at 1.00): measured on an MI355X over
# every case of tests/test_gpu_f16_kernels.py, relative L2 at most 1.26 x the model's (both builds), worst row at most 2.79 x (fp16, 200 tokens) / 2.23 x
# (bf16).  F = 1.25 x 2.79, F_L2 = 1.5 x 1.26.  Probabilities carrying bf16-sized error on fp16 operands sit at 3.6 - 4.0 x in relative L2 (8 x with a bf16
# output rounding): F_L2 refuses them with room, F alone would not, and F must never pass 4.
F = 3.5
F_L2 = 1.9


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def row_err(a, b):
    """Largest inf-norm of a row's error."""
    return (a.double() - b.double()).abs().amax(-1).max().item()


def heads_of(qkv16, B, tok, heads):
    """q, k, v as f64 [B, heads, tok, 64] of the 16-bit rows [B tok, 3 heads 64] = [q | k | v]."""
    D = heads * 64
    x = qkv16.double()
    return tuple(x[:, i * D:(i + 1) * D].reshape(B, tok, heads, 64).transpose(1, 2) for i in range(3))


def scores(qkv16, B, tok, heads, log2_scale):
    q, k, _ = heads_of(qkv16, B, tok, heads)
    return torch.matmul(q, k.transpose(2, 3)) * log2_scale


def _rows(o, B, tok, heads):
    return o.transpose(1, 2).reshape(B * tok, heads * 64)


def softmax_v(s, v):
    """f64 softmax (base 2) of scores s [..., q, keys] times v [..., keys, d]."""
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.matmul(p, v) / p.sum(-1, keepdim=True)


def softmax_v_model(s, v, p_dtype, out_dtype, flush_subnormal_p=False, lag=0.0):
    """The rounding model on scores / values.  ``lag``: P is formed against rowmax - lag (the deferred max of attn_fwd_v5_kernel lets the running maximum trail
    the true one by up to 2^8: P <= 2^lag); ``flush_subnormal_p``: a faulty conversion that turns fp16 subnormal P into zero (negative control)."""
    p = torch.exp2(s - s.amax(-1, keepdim=True) + lag)
    p16 = p.float().to(p_dtype)
    if flush_subnormal_p:
        p16 = torch.where(p16.float().abs() < torch.finfo(p_dtype).tiny, torch.zeros_like(p16), p16)
    o = torch.matmul(p16.double(), v) / p.sum(-1, keepdim=True)
    return o.float().to(out_dtype).double()


def attention_ref(qkv16, B, tok, heads, log2_scale):
    _, _, v = heads_of(qkv16, B, tok, heads)
    return _rows(softmax_v(scores(qkv16, B, tok, heads, log2_scale), v), B, tok, heads)


def attention_model(qkv16, B, tok, heads, log2_scale, p_dtype=None, out_dtype=None, **kw):
    dt = qkv16.dtype
    _, _, v = heads_of(qkv16, B, tok, heads)
    return _rows(softmax_v_model(scores(qkv16, B, tok, heads, log2_scale), v, p_dtype or dt, out_dtype or dt, **kw), B, tok, heads)


def accepts(out, ref, model):
    """(taken, relative-L2 ratio, row-error ratio) of a kernel output under the acceptance rule."""
    r2, rm = rel_l2(out, ref) / rel_l2(model, ref), row_err(out, ref) / row_err(model, ref)
    return (bool(torch.isfinite(out.double()).all()) and r2 <= F_L2 and rm <= F), r2, rm


# ------------------------------------------------------------------------------------------------ input families (seeded; f32 before the 16-bit rounding)
def _store(x, D, dt, prescaled):
    """x f32 [rows, 3 D] with Q in log2 units (the pre-scaled storage) -> the 16-bit operand; the generic form stores Q / C_PRE."""
    x = x.clone()
    if not prescaled:
        x[:, :D] /= C_PRE
    return x.to(dt)


def family_r(B, tok, heads, dt, prescaled=True, seed=None):
    """randn * 1.5, as the product attention tests of tests/test_gpu_kernels.py draw it."""
    D = heads * 64
    g = torch.Generator().manual_seed(tok * 5 + heads if seed is None else seed)
    x = torch.randn(B * tok, 3 * D, generator=g) * 1.5
    x[:, :D] *= C_PRE
    return _store(x, D, dt, prescaled)


def family_s(B, tok, heads, dt, prescaled=True):
    """Family R shifted: column 0 of every head's Q = -4.0 in the pre-scaled storage and of every head's K = +10.0.  The term both columns contributed is
    replaced by -40 for every (query, key): the softmax sees a constant shift, every score is <= -22 (63 remaining terms of sigma 3.2, 5.5 sigma of them),
    and a key that reads as zero (a padded row counted as real) has score 0 -- it would carry the whole row."""
    D = heads * 64
    g = torch.Generator().manual_seed(tok * 5 + heads)
    x = torch.randn(B * tok, 3 * D, generator=g) * 1.5
    x[:, :D] *= C_PRE
    x[:, 0:D:64] = -4.0
    x[:, D:2 * D:64] = 10.0
    return _store(x, D, dt, prescaled)


P_TOK = 400


def family_p(dominant, dt=torch.float16, prescaled=True):
    """fp16 subnormal probabilities: 400 tokens, one head.  Every query scores the ``dominant`` key ~0 and the other 399 keys ~-18 (sigma 0.2), whose V is
    512 + 64 randn while the dominant key's V row is randn: each of the 399 probabilities is an fp16 SUBNORMAL (2^-18: six significant bits left) and together
    they carry ~0.78 of an output of magnitude ~1.  Kept, the rounding model's error is 2.6e-4; flushed to zero it is 0.67.  dominant = 0: its block sets the
    running maximum; 333: a late rescale by 2^-18."""
    tok, D = P_TOK, 64
    g = torch.Generator().manual_seed(31 + dominant)
    x = torch.empty(tok, 3 * D)
    x[:, :D] = torch.randn(tok, D, generator=g) * 0.05
    x[:, 0] = 4.0
    x[:, D:2 * D] = torch.randn(tok, D, generator=g) * 0.5
    x[:, D] = -4.5
    x[dominant, D] = 0.0
    x[:, 2 * D:] = torch.randn(tok, D, generator=g) * 64 + 512
    x[dominant, 2 * D:] = torch.randn(D, generator=g)
    return _store(x, D, dt, prescaled)


D_CASES = ("jump", "creep", "first_tile", "spike")


def family_d(case, dt, prescaled=True):
    """(qkv16, tok): the deferred-max constructions (a) (b) (c) of test_attention_prescaled_deferred_max_branches and the spiked row of
    test_attention_spiked_row_forces_rescale (tests/test_gpu_kernels.py), one head, unchanged."""
    D = 64
    if case == "spike":
        tok = 300
        x = torch.randn(tok, 3 * D, generator=torch.Generator().manual_seed(9)) * 0.5
        x[17, :D] = 3.0
        x[250, D:2 * D] = 4.0
    else:
        tok = 400
        x = torch.randn(tok, 3 * D, generator=torch.Generator().manual_seed(21)) * 0.3
        if case == "jump":                                   # (a) a late key beats the running max by far more than the threshold
            x[5, :D] = 2.0
            x[333, D:2 * D] = 6.0
        elif case == "creep":                                # (b) scores creep up by less than the threshold per tile: no rescale, P > 1
            x[:, D:2 * D] += torch.linspace(0, 1.2, tok).view(-1, 1) * 0.5
            x[:, :D] = 0.5
        elif case == "first_tile":                           # (c) everything far below the first tile
            x[:64, D:2 * D] += 3.0
            x[:, :D] = 1.0
        else:
            raise ValueError(case)
    x[:, :D] *= C_PRE
    return _store(x, D, dt, prescaled), tok
