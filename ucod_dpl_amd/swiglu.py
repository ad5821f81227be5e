"""Host side of the SwiGLU MLP of DINOv2 ViT-g/14 (transformers modeling_dinov2.py:300-315, ``Dinov2SwiGLUFFN``): pure torch, runs on any device.

    hidden = silu(x1) * x2,   (x1, x2) = weights_in(x).chunk(2)        out = weights_out(hidden)

The device computes the product inside the fc1 GEMM's epilogue (include/ucod_dpl.h: UCOD_EPI_BIAS_SWIGLU_BF16), where a lane holds 8 consecutive columns of one
row.  ``x1[j]`` and ``x2[j]`` are F columns apart in HF's layout, so the rows of ``weights_in`` (and its bias) are permuted once here, in blocks of 4:

    GEMM column 8k + e     (e < 4)  <-  x1 unit 4k + e   (row 4k + e of weights_in)
    GEMM column 8k + 4 + e          <-  x2 unit 4k + e   (row F + 4k + e)

Before that, F is padded up to a multiple of 128 (what the kernels' tiles need) with zero rows of ``weights_in`` and zero bias in both halves and zero columns of
``weights_out``: exact, because the padded units compute silu(0) * 0 = 0 and are multiplied by zero weights.  HF's F is ((int(4 D 2 / 3) + 7) // 8) 8: 4096 at
D = 1536 (no padding), 344 at D = 128 (padded to 384).
"""
import torch

PAD = 128


def padded_hidden(F):
    """F rounded up to the kernels' multiple of 128."""
    return (F + PAD - 1) // PAD * PAD


def interleave_perm(F):
    """Row order of the interleaved ``weights_in`` [2F, D] in terms of HF's rows: out row 8k + e <- x1 row 4k + e, 8k + 4 + e <- x2 row F + 4k + e.  F % 4 == 0."""
    if F % 4:
        raise ValueError(f"the SwiGLU interleave needs F % 4 == 0, got {F}")
    j = torch.arange(F).reshape(-1, 4)
    return torch.stack((j, j + F), 1).reshape(-1)


def prepare(w_in, b_in, w_out):
    """HF (weights_in [2F0, D], bias [2F0], weights_out [D, F0]) -> (w_in [2F, D], b_in [2F], w_out [D, F]) padded to F = padded_hidden(F0) and interleaved
    (same dtypes and device as the inputs)."""
    F0 = w_in.shape[0] // 2
    if w_in.shape[0] != 2 * F0 or b_in.shape[0] != 2 * F0 or w_out.shape[1] != F0:
        raise ValueError(f"SwiGLU shapes disagree: weights_in {tuple(w_in.shape)}, bias {tuple(b_in.shape)}, weights_out {tuple(w_out.shape)}")
    F = padded_hidden(F0)
    D = w_in.shape[1]
    wp = w_in.new_zeros(2 * F, D)
    bp = b_in.new_zeros(2 * F)
    wp[:F0], wp[F:F + F0] = w_in[:F0], w_in[F0:]
    bp[:F0], bp[F:F + F0] = b_in[:F0], b_in[F0:]
    wo = w_out.new_zeros(w_out.shape[0], F)
    wo[:, :F0] = w_out
    perm = interleave_perm(F).to(w_in.device)
    return wp[perm].contiguous(), bp[perm].contiguous(), wo.contiguous()


def lora_b_to_engine(b_hf):
    """LoRA B of ``weights_in`` in HF row order, [2 F0, r], -> the engine's rows [2 F, r]: padded like ``prepare`` pads the weight (zero rows) and interleaved."""
    F0 = b_hf.shape[0] // 2
    if b_hf.shape[0] != 2 * F0:
        raise ValueError(f"lora_B of weights_in must have an even number of rows, got {tuple(b_hf.shape)}")
    F = padded_hidden(F0)
    bp = b_hf.new_zeros(2 * F, *b_hf.shape[1:])
    bp[:F0], bp[F:F + F0] = b_hf[:F0], b_hf[F0:]
    return bp[interleave_perm(F).to(b_hf.device)].contiguous()


def lora_b_from_engine(b_eng, F0):
    """The inverse of ``lora_b_to_engine``: rows [2 F, r] of the engine -> HF order, unpadded [2 F0, r] (padded rows are dropped)."""
    F = b_eng.shape[0] // 2
    if F != padded_hidden(F0):
        raise ValueError(f"{tuple(b_eng.shape)} is not the padded form of a hidden width of {F0}")
    bp = torch.empty_like(b_eng)
    bp[interleave_perm(F).to(b_eng.device)] = b_eng
    return torch.cat((bp[:F0], bp[F:F + F0]), 0).contiguous()


def swiglu_interleaved(y):
    """The epilogue's arithmetic on the interleaved GEMM output y [..., 2F] -> [..., F] (checker form; any dtype)."""
    z = y.reshape(*y.shape[:-1], -1, 2, 4)
    return (torch.nn.functional.silu(z[..., 0, :]) * z[..., 1, :]).reshape(*y.shape[:-1], -1)


def swiglu_interleaved_grad(pre, dhid):
    """The backward of ``swiglu_interleaved``: interleaved pre-activation ``pre`` [..., 2F] and the hidden's cotangent ``dhid`` [..., F] -> the cotangent of ``pre``
    [..., 2F] in the same interleaved order (checker form of UCOD_EPI_SWIGLU_BWD_BF16; the dtype of the inputs).  With g the cotangent of hidden unit 4k + e,
    x1 = pre[8k + e], x2 = pre[8k + 4 + e] and sig = 1 / (1 + exp(-x1)):

        d pre[8k + e] = g x2 sig (1 + x1 (1 - sig)),        d pre[8k + 4 + e] = g x1 sig
    """
    z = pre.reshape(*pre.shape[:-1], -1, 2, 4)
    g = dhid.reshape(*dhid.shape[:-1], -1, 4)
    x1, x2 = z[..., 0, :], z[..., 1, :]
    sig = torch.sigmoid(x1)
    return torch.stack((g * x2 * sig * (1 + x1 * (1 - sig)), g * x1 * sig), -2).reshape(pre.shape)
