"""BLK16: the MLP hidden in MFMA-fragment order (include/ucod_dpl.h, "BLK16").

An activation [M, F] (F % 64 == 0, rows padded to Mp = 16 ceil(M / 16)) is stored as the A operands of v_mfma_f32_16x16x32:
    chunk (m, s, g) -- token row m, k-step s = 0 .. F/32 - 1, g = 0 .. 3 -- is 8 values at element offset (((m // 16) (F / 32) + s) 64 + g 16 + m % 16) 8,
    and element e of the chunk is hidden unit pi(32 s + 8 g + e) = 32 s + 16 (e >> 2) + 4 g + (e & 3).
The consumer's weight carries pi on its K axis: W'[n, k] = W[n, pi(k)].  Host-side helpers: the permutation is applied once, when an engine is built; pack / unpack
are what the tests read the kernels' buffers with."""
import torch


def padded_rows(M):
    return 16 * ((M + 15) // 16)


def pi(F):
    """Index vector p [F] with p[k] = pi(k): position k of the consumer's K axis holds hidden unit p[k]."""
    if F % 32 != 0:
        raise ValueError("BLK16 needs F % 32 == 0")
    k = torch.arange(F)
    s, g, e = k // 32, (k % 32) // 8, k % 8
    return 32 * s + 16 * (e // 4) + 4 * g + (e % 4)


def permute_weight(w):
    """fc2's weight [N, F] -> W' = W[:, pi]: the B operand of ucod_gemm_bf16_blk16a."""
    return w[:, pi(w.shape[1]).to(w.device)].contiguous()


def pack(x, fill=0):
    """Row-major [M, F] -> the BLK16 buffer, flat [Mp F]; rows M .. Mp - 1 hold `fill`."""
    M, F = x.shape
    if F % 64 != 0:
        raise ValueError("BLK16 needs F % 64 == 0")
    Mp = padded_rows(M)
    xp = torch.full((Mp, F), fill, dtype=x.dtype, device=x.device)
    xp[:M] = x
    # [mb, ml, s, h = e >> 2, g, r = e & 3] -> [mb, s, g, ml, h, r]
    return xp.view(Mp // 16, 16, F // 32, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous().view(-1)


def unpack(buf, M, F):
    """The BLK16 buffer (flat, Mp F values) -> row-major [M, F] (the padding rows are dropped)."""
    Mp = padded_rows(M)
    return buf.view(-1)[:Mp * F].view(Mp // 16, F // 32, 4, 16, 2, 4).permute(0, 3, 1, 4, 2, 5).contiguous().view(Mp, F)[:M]
