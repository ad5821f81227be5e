"""Functional wrappers over the C ABI: allocate outputs with torch, launch on the current stream.

Every function requires CUDA (ROCm) tensors and raises otherwise -- there is no CPU path here.
"""
import ctypes as C
import os

import torch

from . import native as N
from .native import ptr, stream, check


def _f32(t):
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t


def _bf16(t):
    if t.dtype != torch.bfloat16:
        raise TypeError(f"expected bfloat16, got {t.dtype}")
    return t


# ----------------------------------------------------------------------------- backbone pieces
def gemm_bf16(epilogue, A, Bm, out, M, Nn, K, bias=None, scale=None, resid=None, pos=None, tok=0, variant=0):
    """``variant`` outside the product set (native.GEMM_PRODUCT_VARIANTS) goes to the laboratory library (`make variants`)."""
    if variant in N.GEMM_PRODUCT_VARIANTS:
        fn, what = N.load().ucod_gemm_bf16, "ucod_gemm_bf16"
    else:
        fn, what = N.load_lab().ucod_gemm_bf16_lab, "ucod_gemm_bf16_lab"
    check(fn(epilogue, ptr(_bf16(A)), ptr(_bf16(Bm)), ptr(out), M, Nn, K, ptr(bias), ptr(scale), ptr(resid), ptr(pos), tok, variant, stream()), what)
    return out


def linear_bf16(x, w, b, gelu=False, variant=0):
    """x bf16 [M,K], w bf16 [N,K], b f32 [N] -> bf16 [M,N]."""
    M, K = x.shape
    out = torch.empty(M, w.shape[0], dtype=torch.bfloat16, device=x.device)
    return gemm_bf16(N.EPI_BIAS_GELU_BF16 if gelu else N.EPI_BIAS_BF16, x, w, out, M, w.shape[0], K, bias=_f32(b), variant=variant)


def linear_bf16_asm(x, w, b, out=None, dbg=None, form=0):
    """LABORATORY: the hand-placed persistent GEMM (variants/gemm_asm_lab.hip; K = 768, N % 256 == 0): x bf16 [M,K], w bf16 [N,K], b f32 [N] -> bf16 [M,N]."""
    M, K = x.shape
    out = torch.empty(M, w.shape[0], dtype=torch.bfloat16, device=x.device) if out is None else out
    check(N.load_lab().ucod_gemm_bf16_asm_lab(ptr(_bf16(x)), ptr(_bf16(w)), ptr(_f32(b)), ptr(out), M, w.shape[0], K, form, ptr(dbg), stream()), "ucod_gemm_bf16_asm_lab")
    return out


def linear_scale_resid(x, w, b, scale, resid, variant=0):
    """resid f32 [M,N] + scale[n]*(x w^T + b) -> new f32 [M,N]."""
    M, K = x.shape
    out = torch.empty_like(resid)
    return gemm_bf16(N.EPI_BIAS_SCALE_RESID_F32, x, w, out, M, w.shape[0], K, bias=b, scale=scale, resid=resid, variant=variant)


# ---- split-operand (f32-equivalent) pieces: include/ucod_dpl.h, "split-operand backbone pass"; csrc/split.hip
def split_products(terms):
    n = N.load().ucod_split_products(int(terms))
    if n == 0:
        raise ValueError(f"terms must be 2 or 3, got {terms}")
    return n


def _term16(term, terms):
    """True for the fp16-term form ("split2h", csrc/split16.hip: two terms, three products, libucod_dpl_f16.so), False for the bf16-term form of csrc/split.hip."""
    if term not in ("bf16", "f16"):
        raise ValueError(f"term must be 'bf16' or 'f16', got {term!r}")
    if term == "f16" and int(terms) != 2:
        raise ValueError(f"term='f16' is the two-term form (terms=2), got terms={terms!r}")
    return term == "f16"


def pow2_scale(t, top=14):
    """The power of two s with max |s t| in [2^(top-1), 2^top): the per-tensor scale of an fp16-term operand (1.0 for an all-zero tensor)."""
    import math
    m = float(t.detach().abs().max())
    if not (m > 0.0 and math.isfinite(m)):
        return 1.0
    return 2.0 ** (top - math.frexp(m)[1])


def split16_class_scale(cls):
    s = float(N.load("f16").ucod_split16_class_scale(int(cls)))
    if s == 0.0:
        raise ValueError(f"unknown operand class {cls}")
    return s


def _gemm_f16(epilogue, A, Bm, out, M, Nn, K, bias=None, scale=None, resid=None, pos=None, tok=0, variant=0):
    """ucod_gemm_bf16 of the fp16-operand library (the GEMMs of the fp16-term split pass)."""
    if A.dtype != torch.float16 or Bm.dtype != torch.float16:
        raise TypeError(f"expected float16 operands, got {A.dtype} / {Bm.dtype}")
    if variant not in N.GEMM_PRODUCT_VARIANTS:
        raise ValueError(f"variant must be one of {N.GEMM_PRODUCT_VARIANTS}")
    check(N.load("f16").ucod_gemm_bf16(epilogue, ptr(A), ptr(Bm), ptr(out), M, Nn, K, ptr(bias), ptr(scale), ptr(resid), ptr(pos), tok, variant, stream()), "ucod_gemm_bf16 (f16)")
    return out


def gemm_act_split16(xs, ws, bias, op, alpha, scale, variant=0, out=None):
    """fc1 + activation + fp16-term split in ONE launch (ucod_split16_gemm_act): ``xs`` fp16 [M, 3 K] (A side), ``ws`` fp16 [N, 3 K] (B side), ``bias`` f32 [N] already
    times the operands' scales S, ``alpha`` = 1 / S, ``scale`` the scale of the result (powers of two).  op 1: exact-erf GELU -> fp16 [M, 3 N]; op 3: SwiGLU of the
    interleaved x1 / x2 columns -> fp16 [M, 3 N / 2].  The same bits as _gemm_f16(EPI_BIAS_F32) + split_rows(term="f16", op=op) wherever both sum K in one order."""
    if xs.dtype != torch.float16 or ws.dtype != torch.float16:
        raise TypeError(f"expected float16 split operands, got {xs.dtype} / {ws.dtype}")
    if op not in (1, 3):
        raise ValueError(f"op must be 1 (GELU) or 3 (SwiGLU), got {op!r}")
    if variant not in N.GEMM_PRODUCT_VARIANTS:
        raise ValueError(f"variant must be one of {N.GEMM_PRODUCT_VARIANTS}")
    M, K3 = xs.shape
    Nn = ws.shape[0]
    if ws.shape[1] != K3:
        raise ValueError(f"operand widths differ: {K3} / {ws.shape[1]}")
    width = 3 * Nn if op == 1 else 3 * Nn // 2
    if out is None:
        out = torch.empty(M, width, dtype=torch.float16, device=xs.device)
    elif out.dtype != torch.float16 or out.numel() < M * width:
        raise ValueError(f"out must hold {M} x {width} float16 values")
    check(N.load("f16").ucod_split16_gemm_act(int(op), ptr(xs), ptr(ws), ptr(out), M, Nn, K3, ptr(_f32(bias)), float(alpha), float(scale), int(variant), stream()),
          "ucod_split16_gemm_act")
    return out


def split_rows(x, terms, role, op=0, alpha=1.0, term="bf16", scale=1.0):
    """x f32 [M,K] (rows may be strided) -> bf16 [M, P K]: segment p holds term {0,0,1,1,0,2}[p] (role 0, the A side) / {0,1,0,1,2,0}[p] (role 1, the B side)
    of x = x0 + x1 (+ x2).  op 1: exact-erf GELU of x first; op 2: x * alpha first.
    ``term="f16"`` (terms = 2): fp16 [M, 3 K] = hi | hi | lo (role 0) / hi | lo | hi (role 1) of ``scale`` * f(x), ``scale`` a power of two (csrc/split16.hip; op 1 and
    op 3 apply ``alpha`` to their argument too); values with |scale * f| > 65504 are clamped and counted (ucod_resid16_overflow_*)."""
    f16 = _term16(term, terms)
    _f32(x)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_rows takes a 2-d tensor with contiguous rows")
    if not x.is_cuda:
        raise RuntimeError("ucod_dpl_amd: tensor is not on a GPU; the HIP path has no CPU fallback")
    M, K = x.shape
    if f16:
        if op == 3:
            K //= 2
        out = torch.empty(M, 3 * K, dtype=torch.float16, device=x.device)
        check(N.load("f16").ucod_split16_rows(x.data_ptr(), x.stride(0), ptr(out), M, K, int(role), int(op), float(alpha), float(scale), stream()), "ucod_split16_rows")
        return out
    if scale != 1.0:
        raise ValueError("scale belongs to term='f16'")
    out = torch.empty(M, split_products(terms) * K, dtype=torch.bfloat16, device=x.device)
    check(N.load().ucod_split_rows(x.data_ptr(), x.stride(0), ptr(out), M, K, int(terms), int(role), int(op), float(alpha), stream()), "ucod_split_rows")
    return out


def linear_split(x, w, b, terms, variant=0, term="bf16", x_scale=None, w_scale=None):
    """f32-equivalent x w^T + b on the bf16 matrix pipe: x f32 [M,K], w f32 [N,K], b f32 [N] -> f32 [M,N] (ucod_gemm_bf16 over the K-concatenated split operands).
    ``term="f16"``: the same on two fp16 terms per operand; ``x_scale`` / ``w_scale`` default to the per-tensor power of two that puts the largest magnitude in
    [2^13, 2^14).  The accumulator holds x_scale w_scale times the product: the bias goes in times that factor and one exact in-place pass takes it out."""
    M, K = x.shape
    if _term16(term, terms):
        sx = pow2_scale(x) if x_scale is None else float(x_scale)
        sw = pow2_scale(w) if w_scale is None else float(w_scale)
        out = torch.empty(M, w.shape[0], dtype=torch.float32, device=x.device)
        _gemm_f16(N.EPI_BIAS_F32, split_rows(x, 2, 0, term="f16", scale=sx), split_rows(w, 2, 1, term="f16", scale=sw), out, M, w.shape[0], 3 * K,
                  bias=(_f32(b) * (sx * sw)).contiguous(), variant=variant)
        check(N.load("f16").ucod_split16_scale_f32(ptr(out), out.numel(), 1.0 / (sx * sw), stream()), "ucod_split16_scale_f32")
        return out
    P = split_products(terms)
    out = torch.empty(M, w.shape[0], dtype=torch.float32, device=x.device)
    return gemm_bf16(N.EPI_BIAS_F32, split_rows(x, terms, 0), split_rows(w, terms, 1), out, M, w.shape[0], P * K, bias=_f32(b), variant=variant)


def layernorm_split(x, gamma, beta, eps, terms, role=0, term="bf16", scale=None):
    """``term="f16"``: fp16 [rows, 3 D] of ``scale`` (default: the pass's LayerNorm class scale) times the LayerNorm output."""
    rows, D = x.shape
    if _term16(term, terms):
        scale = split16_class_scale(N.SPLIT16_LN) if scale is None else float(scale)
        out = torch.empty(rows, 3 * D, dtype=torch.float16, device=x.device)
        check(N.load("f16").ucod_split16_layernorm(ptr(_f32(x)), ptr(_f32(gamma)), ptr(_f32(beta)), ptr(out), rows, D, float(eps), int(role), scale, stream()),
              "ucod_split16_layernorm")
        return out
    out = torch.empty(rows, split_products(terms) * D, dtype=torch.bfloat16, device=x.device)
    check(N.load().ucod_layernorm_split(ptr(_f32(x)), ptr(_f32(gamma)), ptr(_f32(beta)), ptr(out), rows, D, float(eps), int(terms), int(role), stream()), "ucod_layernorm_split")
    return out


def attention_split(qkv, B, tok, heads, terms, qscale=0.125 * 1.4426950408889634, term="bf16", in_mul=1.0):
    """qkv f32 [B*tok, 3*heads*64] -> the attention output as the A-side split operand bf16 [B*tok, P*heads*64] (softmax(Q K^T / 8) V, f32-equivalent).
    ``term="f16"``: fp16 [B*tok, 3*heads*64] carrying the pass's attention-output class scale; ``in_mul`` (a power of two) multiplies qkv as it is read."""
    if _term16(term, terms):
        lib = N.load("f16")
        need = lib.ucod_split16_attention_operand_bytes(B, tok, heads)
        if need == 0:
            raise ValueError("unsupported attention geometry")
        opnd = torch.empty(need, dtype=torch.uint8, device=qkv.device)
        out = torch.empty(B * tok, 3 * heads * 64, dtype=torch.float16, device=qkv.device)
        s_qkv, s_att = split16_class_scale(N.SPLIT16_QKV), split16_class_scale(N.SPLIT16_ATT)
        check(lib.ucod_split16_qkv(ptr(_f32(qkv)), ptr(opnd), B, tok, heads, float(in_mul), float(qscale), s_qkv, stream()), "ucod_split16_qkv")
        check(lib.ucod_split16_attention_fwd(ptr(opnd), ptr(out), B, tok, heads, s_qkv, s_att, stream()), "ucod_split16_attention_fwd")
        return out
    lib = N.load()
    need = lib.ucod_attention_split_operand_bytes(B, tok, heads, int(terms))
    if need == 0:
        raise ValueError("unsupported attention geometry")
    opnd = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    out = torch.empty(B * tok, split_products(terms) * heads * 64, dtype=torch.bfloat16, device=qkv.device)
    check(lib.ucod_qkv_split(ptr(_f32(qkv)), ptr(opnd), B, tok, heads, int(terms), float(qscale), stream()), "ucod_qkv_split")
    check(lib.ucod_attention_split_fwd(ptr(opnd), ptr(out), B, tok, heads, int(terms), stream()), "ucod_attention_split_fwd")
    return out


def unsplit(xs, terms, role, K, term="bf16", scale=1.0):
    """The f32 value a split operand [M, P K] stands for (sum of its distinct terms): test helper, torch arithmetic on the device.
    ``term="f16"``: (hi + lo) / scale of an fp16-term operand (the sum rounded to f32; the division by a power of two is exact)."""
    if _term16(term, terms):
        seg = xs.view(xs.shape[0], 3, K).float()
        return (seg[:, 0] + seg[:, 2 if role == 0 else 1]) / float(scale)
    P = split_products(terms)
    seg = xs.view(xs.shape[0], P, K).float()
    order = ([0, 0, 1, 1, 0, 2] if role == 0 else [0, 1, 0, 1, 2, 0])[:P]
    first = [order.index(t) for t in range(int(terms))]
    return sum(seg[:, i] for i in first)


def row_stats_h16(x, eps):
    """x fp16 [rows, D] (the fp16 residual stream) -> f32 [rows, 2] = (rstd, -mean * rstd): what the LayerNorm-folded epilogues read."""
    if x.dtype != torch.float16:
        raise TypeError(f"expected float16, got {x.dtype}")
    rows, D = x.shape
    st = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    check(N.load("f16").ucod_row_stats_h16(ptr(x), ptr(st), rows, D, float(eps), stream()), "ucod_row_stats_h16")
    return st


def fold_layernorm_linear(gamma, beta, w, b):
    """(w_folded fp16 [N,K], bias_folded f32 [N], colsum f32 [N]) of LayerNorm(gamma, beta) -> Linear(w, b): include/ucod_dpl.h, ucod_gemm_lnfold."""
    from .fold import fold_layernorm_linear as _fold
    return _fold(_f32(gamma), _f32(beta), _f32(w), _f32(b))


def linear_lnfold(x, stats, wf, bias_f, colsum, gelu=False, scale=None, variant=0, partials=None, eps=1e-6):
    """LayerNorm + Linear (+ GELU | * scale) as ONE GEMM on the un-normalised fp16 rows (fp16-operand build): x fp16 [M,K] -> fp16 [M,N].
    ``stats`` f32 [M,2] (row_stats_h16) or ``partials`` f32 [M,nslot,2] (left by linear_scale_resid_h16_stats / the patch embedding)."""
    if x.dtype != torch.float16 or wf.dtype != torch.float16:
        raise TypeError("linear_lnfold takes fp16 rows and fp16 folded weights")
    M, K = x.shape
    out = torch.empty(M, wf.shape[0], dtype=torch.float16, device=x.device)
    nslot = 0 if partials is None else partials.shape[1]
    check(N.load("f16").ucod_gemm_lnfold(N.EPI_LNFOLD_GELU_BF16 if gelu else N.EPI_LNFOLD_BIAS_BF16, ptr(x), ptr(wf), ptr(out), M, wf.shape[0], K,
                                         ptr(_f32(bias_f)), ptr(_f32(colsum)), ptr(stats), ptr(partials), nslot, float(eps), ptr(scale), variant, stream()),
          "ucod_gemm_lnfold")
    return out


def linear_scale_resid_h16_stats(a, w, b, scale, resid, half="f16"):
    """resid f16 [M,N] + scale[n] * (a w^T + b) -> (new f16 [M,N], partials f32 [M, N/64, 2]) -- the out-projection / fc2 epilogue on the fp16 stream
    that also leaves each row's (sum, sum of squares) per 64-column slot.  Raises for shapes the large-tile kernels do not take."""
    M, K = a.shape
    Nn = w.shape[0]
    out = torch.empty(M, Nn, dtype=torch.float16, device=a.device)
    part = torch.empty(M, Nn // 64, 2, dtype=torch.float32, device=a.device)
    check(N.load(half).ucod_gemm_bf16_stats(N.EPI_BIAS_SCALE_RESID_H16_STATS, ptr(a), ptr(w), ptr(out), M, Nn, K, ptr(_f32(b)), ptr(_f32(scale)), ptr(resid), None, 0,
                                            ptr(part), Nn // 64, stream()), "ucod_gemm_bf16_stats")
    return out, part


def layernorm(x, gamma, beta, eps, out_f32=False):
    rows, D = x.shape
    y = torch.empty(rows, D, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    check(N.load().ucod_layernorm(ptr(_f32(x)), ptr(_f32(gamma)), ptr(_f32(beta)), ptr(y), rows, D, float(eps), int(out_f32), stream()),
          "ucod_layernorm")
    return y


def attention(qkv, B, tok, heads, scale=0.125, variant=0):
    """``scale`` != 0: generic kernel; ``scale`` == 0: Q pre-scaled by hd^-1/2 log2 e (the product kernel).  ``variant`` outside
    native.ATTN_PRODUCT_VARIANTS selects a laboratory kernel of libucod_dpl_variants.so (`make variants`)."""
    out = torch.empty(B * tok, heads * 64, dtype=torch.bfloat16, device=qkv.device)
    if variant in N.ATTN_PRODUCT_VARIANTS:
        check(N.load().ucod_attention_fwd(ptr(_bf16(qkv)), ptr(out), B, tok, heads, float(scale), variant, stream()), "ucod_attention_fwd")
    else:
        check(N.load_lab().ucod_attention_fwd_lab(ptr(_bf16(qkv)), ptr(out), B, tok, heads, float(scale), variant, stream()), "ucod_attention_fwd_lab")
    return out


def attention_asm(qkv, B, tok, heads, form=0, want_lse=False):
    """LABORATORY (libucod_dpl_variants.so): the hand-placed gfx950 assembly kernels of round 4 -- form 0 = ucod_attn_fwd_pw64 (4 waves x 64 query rows),
    1 = ucod_attn_fwd_pw32 (8 waves x 32 rows).  Q pre-scaled; raises for fewer than three key tiles.  -> out [, lse [B, heads, tok]]"""
    out = torch.empty(B * tok, heads * 64, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, heads, tok, dtype=torch.float32, device=qkv.device) if want_lse else None
    check(N.load_lab().ucod_attention_fwd_asm_lab(ptr(_bf16(qkv)), ptr(out), ptr(lse), B, tok, heads, form, stream()), "ucod_attention_fwd_asm_lab")
    return (out, lse) if want_lse else out


def attention_fp8(qkv, B, tok, heads, q_exp=5, k_exp=3, v_exp=3):
    """The fp8 (e4m3, block-scaled MFMA) attention path of BASELINE configs[4]; ``qkv`` bf16 with Q pre-scaled by hd^-1/2 * log2 e."""
    lib = N.load()
    out = torch.empty(B * tok, heads * 64, dtype=torch.bfloat16, device=qkv.device)
    ws = torch.empty(lib.ucod_attention_fp8_workspace_bytes(B, tok, heads), dtype=torch.uint8, device=qkv.device)
    check(lib.ucod_attention_fwd_fp8(ptr(_bf16(qkv)), ptr(out), ptr(ws), ws.numel(), B, tok, heads, q_exp, k_exp, v_exp, stream()),
          "ucod_attention_fwd_fp8")
    return out


def qkv_fp8_attention(h, w_qkv, b_qkv, B, tok, heads, q_exp=5, k_exp=3, v_exp=3):
    """Fused fp8 path: QKV projection with the e4m3 epilogue (UCOD_EPI_QKV_FP8) straight into Q8 | K8 | V8, then the fp8 attention
    kernel that transposes V on the fly.  ``h`` bf16 [B*tok, D] (LayerNorm output), ``w_qkv`` bf16 [3D, D], ``b_qkv`` f32 [3D]."""
    import math
    lib = N.load()
    D = heads * 64
    M = B * tok
    ws = torch.empty(lib.ucod_attention_fp8_workspace_bytes(B, tok, heads), dtype=torch.uint8, device=h.device)
    scale = torch.empty(3 * D, dtype=torch.float32, device=h.device)
    check(lib.ucod_fill_qscale3(ptr(scale), D, 0.125 * math.log2(math.e) * 2.0 ** q_exp, 2.0 ** k_exp, 2.0 ** v_exp, stream()), "ucod_fill_qscale3")
    check(lib.ucod_attention_fp8_zero_pad(ptr(ws), B, tok, heads, stream()), "ucod_attention_fp8_zero_pad")
    check(lib.ucod_gemm_bf16(N.EPI_QKV_FP8, ptr(_bf16(h)), ptr(_bf16(w_qkv)), ptr(ws), M, 3 * D, D, ptr(_f32(b_qkv)), ptr(scale), None, None, tok, 0,
                             stream()), "ucod_gemm_bf16(QKV_FP8)")
    out = torch.empty(M, D, dtype=torch.bfloat16, device=h.device)
    check(lib.ucod_attention_fwd_fp8_fused(ptr(ws), ptr(out), B, tok, heads, q_exp, k_exp, v_exp, stream()), "ucod_attention_fwd_fp8_fused")
    return out, ws


def patch_im2col(img, P, Kpad):
    B, Cc, H, W = img.shape
    out = torch.empty(B * (H // P) * (W // P), Kpad, dtype=torch.bfloat16, device=img.device)
    check(N.load().ucod_patch_im2col(ptr(_f32(img)), ptr(out), B, Cc, H, W, P, Kpad, stream()), "ucod_patch_im2col")
    return out


def cast_bf16(t, lib=None):
    """f32 -> the 16-bit operand type of ``lib`` (bf16 for the default library, fp16 for the f16 build; round-to-nearest-even)."""
    lib = lib or N.load()
    t = _f32(t).contiguous()
    out = torch.empty(t.shape, dtype=torch.float16 if lib.ucod_half_name() == b"f16" else torch.bfloat16, device=t.device)
    check(lib.ucod_cast_f32_bf16(ptr(t), ptr(out), t.numel(), stream()), "ucod_cast_f32_bf16")
    return out


# ----------------------------------------------------------------------------- decoder pieces
def bilinear_resize(x, oh, ow):
    x = _f32(x).contiguous()
    *lead, ih, iw = x.shape
    planes = 1
    for v in lead:
        planes *= v
    out = torch.empty(*lead, oh, ow, dtype=torch.float32, device=x.device)
    check(N.load().ucod_bilinear_resize(ptr(x), ptr(out), planes, ih, iw, oh, ow, stream()), "ucod_bilinear_resize")
    return out


def bilinear_resize_adjoint(gout, ih, iw):
    gout = _f32(gout).contiguous()
    *lead, oh, ow = gout.shape
    planes = 1
    for v in lead:
        planes *= v
    gin = torch.empty(*lead, ih, iw, dtype=torch.float32, device=gout.device)
    check(N.load().ucod_bilinear_resize_adjoint(ptr(gout), ptr(gin), planes, ih, iw, oh, ow, stream()), "ucod_bilinear_resize_adjoint")
    return gin


class _BilinearResizeFn(torch.autograd.Function):
    """F.interpolate(mode='bilinear', align_corners=False) with its exact transpose as the backward (both HIP kernels)."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.in_hw = tuple(x.shape[-2:])
        return bilinear_resize(x, oh, ow)

    @staticmethod
    def backward(ctx, g):
        return bilinear_resize_adjoint(g.contiguous(), *ctx.in_hw), None, None


def bilinear_resize_autograd(x, oh, ow):
    return _BilinearResizeFn.apply(x, oh, ow)


_EXACT_F32 = bool(os.environ.get("UCOD_DBA_EXACT_F32"))          # the v_mfma_f32_32x32x2_f32 forms of the two decoder GEMMs


def dba_project(x, W, bias, exact=None):
    """x [B,C,H,W] f32, W [Nout,C], bias [Nout] -> d [B,Nout,HW].  Default: the f32-equivalent three-way bf16 split on the bf16 matrix
    pipe (csrc/gemm_split.hip); exact=True (or UCOD_DBA_EXACT_F32=1, or a shape the split kernel does not take): the f32 MFMA kernel."""
    B, Cc, H, Wd = x.shape
    Nout = W.shape[0]
    d = torch.empty(B, Nout, H * Wd, dtype=torch.float32, device=x.device)
    lib = N.load()
    if exact is None and _EXACT_F32:
        exact = True
    if exact is False and not (Cc % 16 == 0 and Nout in (128, 256)):
        raise ValueError("dba_project(exact=False): the split kernel needs C % 16 == 0 and Nout in (128, 256)")
    # (the split kernel runs one 192-pixel tile per workgroup, one workgroup per CU: below ~100 workgroups the f32 kernel's finer grid is faster)
    if exact is False or (not exact and Cc % 16 == 0 and Nout in (128, 256) and B * ((H * Wd + 191) // 192) >= 100):
        nb = lib.ucod_dba_project_split_workspace_bytes(Cc, Nout)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        check(lib.ucod_dba_project_split(ptr(_f32(x)), ptr(_f32(W)), ptr(_f32(bias)), ptr(d), ptr(ws), nb, B, Cc, H * Wd, Nout, stream()),
              "ucod_dba_project_split")
        return d
    check(lib.ucod_dba_project(ptr(_f32(x)), ptr(_f32(W)), ptr(_f32(bias)), ptr(d), B, Cc, H * Wd, Nout, stream()), "ucod_dba_project")
    return d


def dba_colnorm(d, c0, emb):
    B, ld_c, HW = d.shape
    norm = torch.empty(B, 128, dtype=torch.float32, device=d.device)
    check(N.load().ucod_dba_colnorm(ptr(d), ld_c, c0, ptr(_f32(emb)), ptr(norm), B, HW, stream()), "ucod_dba_colnorm")
    return norm


class DetWorkspaces:
    """Per-(entry point, size, device) cache of the workspaces of the deterministic forms (``deterministic=True`` below): a caller that runs the step
    again and again owns one (StandardRunner.det_ws, as it owns disc_saved) instead of a fresh ``torch.empty`` per call.  A workspace is consumed inside the
    call that fills it (stream order), so calls on one stream may share it."""

    def __init__(self):
        self._bufs = {}

    def get(self, name, nbytes, device):
        key = (name, int(nbytes), str(device))
        if key not in self._bufs:
            self._bufs[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._bufs[key]

    def nbytes(self):
        return sum(t.numel() for t in self._bufs.values())


def _det_ws(ws, name, nbytes, device):
    """``ws`` of a deterministic call: None (a fresh buffer), a uint8 tensor of at least ``nbytes`` (the caller reads the partials back), or a DetWorkspaces."""
    if nbytes == 0:
        raise ValueError(f"{name}: unsupported shape")
    if ws is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    if isinstance(ws, DetWorkspaces):
        return ws.get(name, nbytes, device)
    if ws.dtype != torch.uint8:
        raise TypeError(f"{name}: the workspace is a uint8 tensor, got {ws.dtype}")
    return ws                                               # (its size is checked by the entry point)


def dba_heads(d, c0, emb, norm, head_w, head_b, want_bg=True, want_sdiag=False, sdiag=None, deterministic=False, ws=None):
    """``deterministic``: ucod_dba_heads_fwd_det (sdiag as an ordered sum of per-workgroup shares; fg / bg are the same bits either way)."""
    B, ld_c, HW = d.shape
    fg = torch.empty(B, HW, dtype=torch.float32, device=d.device)
    bg = torch.empty(B, HW, dtype=torch.float32, device=d.device) if want_bg else None
    if sdiag is None:
        sdiag = torch.empty(B, dtype=torch.float32, device=d.device) if want_sdiag else None
    if deterministic:
        lib = N.load()
        nb = lib.ucod_dba_heads_fwd_det_workspace_bytes(B, HW)
        ws = _det_ws(ws, "ucod_dba_heads_fwd_det", nb, d.device) if sdiag is not None else None
        check(lib.ucod_dba_heads_fwd_det(ptr(d), ld_c, c0, ptr(emb), ptr(norm), ptr(_f32(head_w)), ptr(_f32(head_b)), ptr(fg), ptr(bg), ptr(sdiag),
                                         ptr(ws), 0 if ws is None else ws.numel(), B, HW, stream()), "ucod_dba_heads_fwd_det")
        return fg, bg, sdiag
    check(N.load().ucod_dba_heads_fwd(ptr(d), ld_c, c0, ptr(emb), ptr(norm), ptr(_f32(head_w)), ptr(_f32(head_b)), ptr(fg), ptr(bg),
                                      ptr(sdiag), B, HW, stream()), "ucod_dba_heads_fwd")
    return fg, bg, sdiag


def orth_gram(d, c0, emb, norm, sdiag):
    B, ld_c, HW = d.shape
    lib = N.load()
    ws = torch.empty(lib.ucod_orth_workspace_bytes(B, HW), dtype=torch.uint8, device=d.device)
    gram = torch.empty(B, 2, 64, 64, dtype=torch.float32, device=d.device)
    loss = torch.empty(1, dtype=torch.float32, device=d.device)
    check(lib.ucod_orth_gram_fwd(ptr(d), ld_c, c0, ptr(emb), ptr(norm), ptr(sdiag), ptr(gram), ptr(loss), ptr(ws), B, HW, stream()),
          "ucod_orth_gram_fwd")
    return loss, gram


def dba_bwd(d, c0, emb, norm, head_w, gram, gfg, gbg, gextra, g_head_w=None, g_head_b=None, g_dec_bias=None, deterministic=False, ws=None):
    """``deterministic``: ucod_dba_bwd_det (the three small gradients as ordered sums over the images; gd is the same bits either way)."""
    B, ld_c, HW = d.shape
    lib = N.load()
    dev = d.device
    gd = torch.empty(B, 128, HW, dtype=torch.float32, device=dev)
    g_head_w = torch.empty(2, 64, dtype=torch.float32, device=dev) if g_head_w is None else g_head_w
    g_head_b = torch.empty(2, dtype=torch.float32, device=dev) if g_head_b is None else g_head_b
    g_dec_bias = torch.empty(128, dtype=torch.float32, device=dev) if g_dec_bias is None else g_dec_bias
    if deterministic:
        ws = _det_ws(ws, "ucod_dba_bwd_det", lib.ucod_dba_bwd_det_workspace_bytes(B, HW), dev)
        check(lib.ucod_dba_bwd_det(ptr(d), ld_c, c0, ptr(emb), ptr(norm), ptr(head_w), ptr(gram), ptr(_f32(gfg)), ptr(_f32(gbg)), float(gextra),
                                   ptr(gd), ptr(g_head_w), ptr(g_head_b), ptr(g_dec_bias), ptr(ws), ws.numel(), B, HW, stream()), "ucod_dba_bwd_det")
        return gd, g_head_w, g_head_b, g_dec_bias
    ws = torch.empty(lib.ucod_dba_bwd_workspace_bytes(B, HW), dtype=torch.uint8, device=dev)
    check(lib.ucod_dba_bwd(ptr(d), ld_c, c0, ptr(emb), ptr(norm), ptr(head_w), ptr(gram), ptr(_f32(gfg)), ptr(_f32(gbg)), float(gextra),
                           ptr(gd), ptr(g_head_w), ptr(g_head_b), ptr(g_dec_bias), ptr(ws), B, HW, stream()), "ucod_dba_bwd")
    return gd, g_head_w, g_head_b, g_dec_bias


def dba_wgrad(gd, x, gW=None, exact=None, deterministic=False, ws=None):
    """gW [128,C] = sum_{b,p} gd[b,n,p] x[b,c,p].  Default on large batches: the three-way bf16 split on the bf16 matrix pipe
    (csrc/gemm_split.hip, f32-equivalent); exact=True / UCOD_DBA_EXACT_F32=1 / small batches: the f32 MFMA kernel.
    ``deterministic``: ucod_dba_wgrad_det -- the same kernel choice, per-workgroup partials in ``ws`` and an ordered sum instead of f32 atomics."""
    B, Cc = x.shape[0], x.shape[1]
    HW = gd.shape[2]
    gW = torch.empty(128, Cc, dtype=torch.float32, device=x.device) if gW is None else gW
    if exact is None and _EXACT_F32:
        exact = True
    split = exact is False or (not exact and B * ((Cc + 383) // 384) >= 32)
    if deterministic:
        lib = N.load()
        ws = _det_ws(ws, "ucod_dba_wgrad_det", lib.ucod_dba_wgrad_det_workspace_bytes(B, Cc, HW, int(not split)), x.device)
        check(lib.ucod_dba_wgrad_det(ptr(gd), ptr(_f32(x)), ptr(gW), B, Cc, HW, int(not split), ptr(ws), ws.numel(), stream()), "ucod_dba_wgrad_det")
        return gW
    if split:
        check(N.load().ucod_dba_wgrad_split(ptr(gd), ptr(_f32(x)), ptr(gW), B, Cc, HW, stream()), "ucod_dba_wgrad_split")
    else:
        check(N.load().ucod_dba_wgrad(ptr(gd), ptr(_f32(x)), ptr(gW), B, Cc, HW, stream()), "ucod_dba_wgrad")
    return gW


# ----------------------------------------------------------------------------- discriminator / APM / optimiser
def disc_params_struct(tensors):
    """tensors: dict with the 17 DiscParams field names -> CUDA f32 tensors."""
    s = N.DiscParams()
    for name, _ in N.DiscParams._fields_:
        if name == "nbt":                                   # int64[3] view of the three num_batches_tracked counters, or absent
            t = tensors.get("nbt")
            s.nbt = None if t is None else t.data_ptr()
            continue
        setattr(s, name, ptr(_f32(tensors[name])))
    return s


def step_loss(losses, extra, finetune):
    out = torch.empty(1, dtype=torch.float32, device=losses.device)
    check(N.load().ucod_step_loss(ptr(losses), ptr(extra), int(bool(finetune)), ptr(out), stream()), "ucod_step_loss")
    return out[0]


def disc_fwd(mask, tensors, update_running=True, saved=None, deterministic=False, ws=None):
    """``deterministic``: ucod_disc_fwd_det (the BatchNorm sums as ordered f64 sums of per-workgroup partials)."""
    B, _, fs, _ = mask.shape
    lib = N.load()
    if saved is None:
        saved = torch.empty(lib.ucod_disc_saved_bytes(B, fs), dtype=torch.uint8, device=mask.device)
    prob = torch.empty(B, dtype=torch.float32, device=mask.device)
    ps = disc_params_struct(tensors)
    if deterministic:
        ws = _det_ws(ws, "ucod_disc_fwd_det", lib.ucod_disc_fwd_det_workspace_bytes(B, fs), mask.device)
        check(lib.ucod_disc_fwd_det(ptr(_f32(mask)), C.byref(ps), ptr(prob), ptr(saved), B, fs, int(update_running), ptr(ws), ws.numel(), stream()),
              "ucod_disc_fwd_det")
        return prob, saved
    check(lib.ucod_disc_fwd(ptr(_f32(mask)), C.byref(ps), ptr(prob), ptr(saved), B, fs, int(update_running), stream()), "ucod_disc_fwd")
    return prob, saved


def disc_bce(probs_student, probs_pseudo, inv):
    """nn.BCELoss(cat(student, pseudo), [0..0, 1..1]) (mean over 2B) and inv * d(sum)/dprob, one launch -> (g_student, g_pseudo, loss 0-d)"""
    B = probs_student.numel()
    gs, gp = torch.empty_like(probs_student), torch.empty_like(probs_pseudo)
    loss = torch.empty(1, dtype=torch.float32, device=probs_student.device)
    check(N.load().ucod_disc_bce(ptr(_f32(probs_student)), ptr(_f32(probs_pseudo)), ptr(gs), ptr(gp), ptr(loss), B, float(inv), stream()), "ucod_disc_bce")
    return gs, gp, loss[0]


def copy_segments(pairs):
    """[(dst, src), ...] (at most four contiguous f32 tensors each way, same numel pairwise): one launch instead of one copy kernel per pair"""
    k = len(pairs)
    for d, s_ in pairs:
        if d.dtype != torch.float32 or s_.dtype != torch.float32 or not d.is_contiguous() or not s_.is_contiguous() or d.numel() != s_.numel():
            raise ValueError("copy_segments: contiguous f32 tensors of equal size")
    dst = (C.c_void_p * k)(*[d.data_ptr() for d, _ in pairs])
    src = (C.c_void_p * k)(*[s_.data_ptr() for _, s_ in pairs])
    n = (C.c_size_t * k)(*[d.numel() for d, _ in pairs])
    check(N.load().ucod_copy_segments(dst, src, n, k, stream()), "ucod_copy_segments")


def zero_segments(tensors):
    """Zero up to eight contiguous device tensors with ONE launch (ucod_zero_segments)."""
    k = len(tensors)
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous() or (t.numel() * t.element_size()) % 4:
            raise ValueError("zero_segments: contiguous device tensors of a multiple of 4 bytes")
    dst = (C.c_void_p * k)(*[t.data_ptr() for t in tensors])
    n = (C.c_size_t * k)(*[t.numel() * t.element_size() for t in tensors])
    check(N.load().ucod_zero_segments(dst, n, k, stream()), "ucod_zero_segments")


class prezeroed:
    """Context: the accumulating outputs of the calls inside were zeroed by the caller (``zero_segments``); the entry points skip their own memsets
    (include/ucod_dpl.h: ucod_accumulators_prezeroed)."""

    def __enter__(self):
        N.load().ucod_accumulators_prezeroed(1)

    def __exit__(self, *exc):
        N.load().ucod_accumulators_prezeroed(0)
        return False


def binarize(x, logits):
    x = _f32(x).contiguous()
    out = torch.empty_like(x)
    check(N.load().ucod_binarize(ptr(x), ptr(out), x.numel(), int(logits), stream()), "ucod_binarize")
    return out


def apm_bce(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale=1.0, losses=None, deterministic=False, ws=None):
    """``deterministic``: ucod_apm_bce_det (the three loss cells as ordered sums over the images; w, merged, gfg, gbg are the same bits either way)."""
    B = pl.shape[0]
    HW = pl.numel() // B
    dev = pl.device
    w = torch.empty(B, dtype=torch.float32, device=dev)
    merged = torch.empty(B, HW, dtype=torch.float32, device=dev)
    gfg = torch.empty(B, HW, dtype=torch.float32, device=dev)
    gbg = torch.empty(B, HW, dtype=torch.float32, device=dev)
    losses = torch.empty(4, dtype=torch.float32, device=dev) if losses is None else losses
    if deterministic:
        lib = N.load()
        ws = _det_ws(ws, "ucod_apm_bce_det", lib.ucod_apm_bce_det_workspace_bytes(B), dev)
        check(lib.ucod_apm_bce_det(ptr(pl), ptr(teacher), ptr(fg), ptr(bg), ptr(p_s), ptr(p_p), float(epoch_frac), float(gscale), ptr(w), ptr(merged),
                                   ptr(gfg), ptr(gbg), ptr(losses), ptr(ws), ws.numel(), B, HW, stream()), "ucod_apm_bce_det")
        return w, merged, gfg, gbg, losses
    check(N.load().ucod_apm_bce(ptr(pl), ptr(teacher), ptr(fg), ptr(bg), ptr(p_s), ptr(p_p), float(epoch_frac), float(gscale), ptr(w),
                                ptr(merged), ptr(gfg), ptr(gbg), ptr(losses), B, HW, stream()), "ucod_apm_bce")
    return w, merged, gfg, gbg, losses


def apm_bce_gprob(pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale=1.0, finetune=False):
    """-> (gp_s [B], gp_p [B]): the step loss's gradient with respect to the two discriminator probabilities (the targets of both BCEWithLogits terms
    depend on w(p_s, p_p); ``loss -= dis_loss`` on p_s unless ``finetune``) -- what ``apm_bce`` holds constant.  Deterministic."""
    B = pl.shape[0]
    HW = pl.numel() // B
    gp_s = torch.empty(B, dtype=torch.float32, device=pl.device)
    gp_p = torch.empty(B, dtype=torch.float32, device=pl.device)
    check(N.load().ucod_apm_bce_gprob(ptr(pl), ptr(teacher), ptr(fg), ptr(bg), ptr(p_s), ptr(p_p), float(epoch_frac), float(gscale), int(bool(finetune)),
                                      ptr(gp_s), ptr(gp_p), B, HW, stream()), "ucod_apm_bce_gprob")
    return gp_s, gp_p


def conv3x3(x, wmat, nout=None):
    """3x3 / stride 1 / pad 1 convolution without the unfold buffer: x [B,C,H,W] f32, wmat [Nout,Kpad] (column c*9 + ky*3 + kx, Kpad % 16 == 0,
    Kpad >= 9C) -> [B,Nout,H,W]; bit-identical to ucod_unfold3x3 + ucod_dba_project with a zero bias"""
    B, Cin, H, W = x.shape
    nout = wmat.shape[0] if nout is None else nout
    y = torch.empty(B, nout, H, W, dtype=torch.float32, device=x.device)
    check(N.load().ucod_conv3x3_f32(ptr(x), ptr(wmat), ptr(y), B, Cin, H, W, nout, wmat.shape[1], stream()), "ucod_conv3x3_f32")
    return y


def conv3x3_dgrad_weights(weight):
    """conv weight [Cout,Cin,3,3] -> Wd [Cin, 16 * ceil(9 Cout / 16)] with conv3x3(gy, Wd) = the data gradient of the pad-1 convolution (exact copy)"""
    Cout, Cin = weight.shape[:2]
    kpad = (9 * Cout + 15) // 16 * 16
    wd = torch.empty(Cin, kpad, dtype=torch.float32, device=weight.device)
    check(N.load().ucod_conv3x3_dgrad_weights(ptr(_f32(weight).contiguous()), ptr(wd), Cout, Cin, kpad, stream()), "ucod_conv3x3_dgrad_weights")
    return wd


def adamw_ema(p, g, m, v, ema, lr, step, ema_alpha=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01):
    check(N.load().ucod_adamw_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), float(lr), beta1, beta2, eps, weight_decay, int(step),
                                  float(ema_alpha), stream()), "ucod_adamw_ema")


DISC_GRAD_SHAPES = (("w1", (32, 1, 3, 3)), ("g1", (32,)), ("b1", (32,)), ("w2", (16, 32, 3, 3)), ("g2", (16,)), ("b2", (16,)),
                    ("w3", (8, 16, 3, 3)), ("g3", (8,)), ("b3", (8,)), ("lin_w", None), ("lin_b", (1,)))


def disc_bwd(mask, tensors, saved, gprob, grads=None, accumulate=False, deterministic=False, ws=None):
    """Gradients of sum_b gprob[b]*prob[b] w.r.t. the 11 discriminator parameters (reference order).
    ``deterministic``: ucod_disc_bwd_det (the Linear layer's gradients as ordered sums over the images)."""
    B, _, fs, _ = mask.shape
    lib = N.load()
    dev = mask.device
    if grads is None:
        grads = [torch.zeros(tensors["lin_w"].shape if shp is None else shp, dtype=torch.float32, device=dev) for _, shp in DISC_GRAD_SHAPES]
        accumulate = True                                   # freshly zeroed
    gs = N.DiscGrads()
    for (name, _), t in zip(DISC_GRAD_SHAPES, grads):
        setattr(gs, name, ptr(_f32(t)))
    ps = disc_params_struct(tensors)
    if deterministic:
        ws = _det_ws(ws, "ucod_disc_bwd_det", lib.ucod_disc_bwd_det_workspace_bytes(B, fs), dev)
        check(lib.ucod_disc_bwd_det(ptr(_f32(mask)), C.byref(ps), ptr(saved), ptr(_f32(gprob)), C.byref(gs), int(accumulate), ptr(ws), ws.numel(), B, fs,
                                    stream()), "ucod_disc_bwd_det")
        return grads
    ws = torch.empty(lib.ucod_disc_bwd_workspace_bytes(B, fs), dtype=torch.uint8, device=dev)
    check(lib.ucod_disc_bwd(ptr(_f32(mask)), C.byref(ps), ptr(saved), ptr(_f32(gprob)), C.byref(gs), int(accumulate), ptr(ws), B, fs,
                            stream()), "ucod_disc_bwd")
    return grads


# ----------------------------------------------------------------------------- COD measures (row N4)
def cod_metrics(pred, gt):
    """pred, gt f32 [B,H,W] -> f64 [B, COD_RECORD] per-image measures (layout in include/ucod_dpl.h)."""
    pred, gt = _f32(pred).contiguous(), _f32(gt).contiguous()
    B, H, W = pred.shape
    if gt.shape != pred.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ")
    lib = N.load()
    nbytes = lib.ucod_cod_metrics_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    out = torch.empty(B, N.COD_RECORD, dtype=torch.float64, device=pred.device)
    check(lib.ucod_cod_metrics(ptr(pred), ptr(gt), B, H, W, ptr(out), ptr(ws), nbytes, stream()), "ucod_cod_metrics")
    return out


# ----------------------------------------------------------------------------- refiner training (the window branch of models/UDLR.py)
def pad_rows64(M):
    """Mp of ucod_transpose_pad_bf16: the K of a weight-gradient GEMM over M token rows."""
    return max(128, 64 * ((M + 63) // 64))


def transpose_pad_bf16(src, cols=None):
    """src [M, ld] f32 or bf16 -> bf16 [cols, Mp] = src[:, :cols]^T (round to nearest even), zeros in the pad columns M .. Mp-1."""
    M, ld = src.shape
    cols = ld if cols is None else cols
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"expected float32 or bfloat16, got {src.dtype}")
    out = torch.empty(cols, pad_rows64(M), dtype=torch.bfloat16, device=src.device)
    check(N.load().ucod_transpose_pad_bf16(ptr(src), int(src.dtype == torch.bfloat16), M, cols, ld, ptr(out), stream()), "ucod_transpose_pad_bf16")
    return out


def weight_grad(dy, x, out=None):
    """dW f32 [N, K] = dy^T x for dy [M, N], x [M, K] (f32 or bf16 rows; 16-bit operands, f32 accumulation): two transposes and the project's GEMM."""
    a, b = transpose_pad_bf16(dy), transpose_pad_bf16(x)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=dy.device) if out is None else out
    return gemm_bf16(N.EPI_BIAS_F32, a, b, out, a.shape[0], b.shape[0], a.shape[1])


def _rows2d(t, what):
    """(data pointer, row stride) of a 2-D device tensor whose rows are dense; a column slice of a wider buffer (``kv[:, C:]``) is taken where it lies."""
    if not t.is_cuda:
        raise RuntimeError("ucod_dpl_amd: tensor is not on a GPU; the HIP path has no CPU fallback")
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise RuntimeError(f"ucod_dpl_amd: {what} must be 2-D with dense rows, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    return t.data_ptr(), int(t.stride(0))


def weight_grad_direct(dy, x, out=None, accumulate=False, ws=None):
    """dW f32 [N, K] (+)= dy^T x for bf16 dy [M, N], x [M, K] read token-major where they lie (row-strided views allowed; no transposed copy): ucod_wgrad_bf16_det,
    the token axis split into ``ucod_wgrad_bf16_det_nsplit(M, N, K)`` chunks whose f32 partials are added in ascending order -- bit-identical from run to run.
    ``out``: f32 [N, K] rows of any stride >= K (e.g. rows of the in_proj gradient); ``accumulate`` adds into it.  ``ws``: a uint8 workspace of at least
    ``ucod_wgrad_bf16_det_workspace_bytes(M, N, K)`` bytes to reuse; allocated when None."""
    lib = N.load()
    _bf16(dy), _bf16(x)
    (pdy, ld_dy), (px, ld_x) = _rows2d(dy, "dy"), _rows2d(x, "x")
    M, Nn = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError(f"weight_grad_direct: dy has {M} rows, x has {x.shape[0]}")
    if out is None:
        if accumulate:
            raise ValueError("weight_grad_direct: accumulate needs out")
        out = torch.empty(Nn, K, dtype=torch.float32, device=dy.device)
    if tuple(out.shape) != (Nn, K):
        raise ValueError(f"weight_grad_direct: out shape {tuple(out.shape)} != {(Nn, K)}")
    pout, ld_dw = _rows2d(_f32(out), "out")
    nbytes = lib.ucod_wgrad_bf16_det_workspace_bytes(M, Nn, K)
    if ws is None and nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    check(lib.ucod_wgrad_bf16_det(pdy, ld_dy, px, ld_x, pout, ld_dw, M, Nn, K, int(bool(accumulate)), ptr(ws) if nbytes else None,
                                  ws.numel() * ws.element_size() if nbytes else 0, stream()), "ucod_wgrad_bf16_det")
    return out


def dgrad_bf16(dy, wt, gelu_pre=None):
    """dx bf16 [M, K] = dy [M, N] wt[K, N]^T (wt = the transposed weight), times gelu'(gelu_pre) when the saved fc1 pre-activation is given."""
    M, Nn = dy.shape
    out = torch.empty(M, wt.shape[0], dtype=torch.bfloat16, device=dy.device)
    epi = N.EPI_BIAS_BF16 if gelu_pre is None else N.EPI_GELU_BWD_BF16
    check(N.load().ucod_gemm_bf16_train(epi, ptr(_bf16(dy)), ptr(_bf16(wt)), ptr(out), M, wt.shape[0], Nn, None, ptr(gelu_pre), None, 0, stream()),
          "ucod_gemm_bf16_train")
    return out


def colsum_det(x, out=None):
    """out f32 [N] = column sums of x [M, N] (f32 or bf16), fixed summation order."""
    lib = N.load()
    M, Nn = x.shape
    out = torch.empty(Nn, dtype=torch.float32, device=x.device) if out is None else out
    nbytes = lib.ucod_colsum_det_workspace_bytes(M, Nn)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    elem = N.ROPE_ELEM_F32 if x.dtype == torch.float32 else N.ROPE_ELEM_HALF
    check(lib.ucod_colsum_det(ptr(x), elem, M, Nn, Nn, None, ptr(out), ptr(ws), nbytes, stream()), "ucod_colsum_det")
    return out


def layernorm_param_grad(dy, x, eps, out=None):
    """(dgamma, dbeta) f32 [D] of a LayerNorm over rows: dy [rows, D] f32 or bf16, x f32 [rows, D].  ``out``: the two f32 [D] destinations, or None."""
    rows, D = x.shape
    slabs = min(128, (rows + 63) // 64)
    ws = torch.empty(slabs * 2 * D, dtype=torch.float32, device=x.device)
    dg, db = (torch.empty(D, dtype=torch.float32, device=x.device), torch.empty(D, dtype=torch.float32, device=x.device)) if out is None else (_f32(out[0]), _f32(out[1]))
    check(N.load().ucod_layernorm_param_grad(ptr(dy), N.LNB_DY_BF16 if dy.dtype == torch.bfloat16 else 0, ptr(_f32(x)), ptr(dg), ptr(db), ptr(ws),
                                             ws.numel() * 4, rows, D, float(eps), stream()), "ucod_layernorm_param_grad")
    return dg, db


def gated_ensemble_bwd(l1_up, l2, ge_w, f0w, f0b, f2w, g_out):
    """Backward of ucod_gated_ensemble for the cotangent ``g_out`` of its output -> (dl2 [B,1,h,w], d fuser.0.weight [64], d fuser.0.bias [64],
    d fuser.2.weight [64], d fuser.2.bias [1]), all f32; deterministic (per-workgroup partials, one ordered f64 sum)."""
    lib = N.load()
    B, _, h, w = l2.shape
    dev = l2.device
    dl2 = torch.empty_like(l2)
    d_a, d_c, d_d = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    d_b = torch.empty(1, dtype=torch.float32, device=dev)
    nbytes = lib.ucod_gated_ensemble_bwd_workspace_bytes(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib.ucod_gated_ensemble_bwd(ptr(_f32(l1_up)), ptr(_f32(l2)), ptr(_f32(ge_w)), ptr(f0w), ptr(f0b), ptr(f2w), ptr(_f32(g_out)), ptr(dl2), ptr(d_a), ptr(d_c),
                                      ptr(d_d), ptr(d_b), ptr(ws), nbytes, B, h, w, stream()), "ucod_gated_ensemble_bwd")
    return dl2, d_a, d_c, d_d, d_b


def window_gather(dl2, coords, win_img, g, accumulate, H, W, ws):
    """g [n,1,H,W] (+)= the windows' cells of dl2 [B,1,ws*H,ws*W] / (1 + 1e-6): the adjoint of ucod_window_scatter."""
    n, B = int(g.shape[0]), int(dl2.shape[0])
    check(N.load().ucod_window_gather(ptr(dl2), ptr(coords) if n else None, ptr(win_img) if n else None, ptr(g) if n else None, int(bool(accumulate)), n, B, H, W,
                                      ws, stream()), "ucod_window_gather")
    return g
