"""CPU reference, rounding model, tile-walk restatement, inputs and checker for the attention backward pair of csrc/attention_bwd.hip
(attn_bwd_dq_kernel / attn_bwd_dkv_kernel behind ucod_attention_bwd) and the LSE forward it consumes (ucod_attention_fwd_lse).

Test infrastructure only: nothing here is the code under test, and nothing here reads GPU output to set a bound.

Tensors.  Operands are [B, N, D] bf16 with D = heads * 64: ``qs`` is Q as the QKV epilogue stores it (already multiplied by 0.125 * log2(e) and rounded
to bf16), ``k``, ``v``, ``do`` as they are.  Results are dicts of f64 tensors per (image, head) slab: "out", "dq", "dk", "dv" [B, heads, N, 64] and
"lse", "delta" [B, heads, N].  With S = qs K^T, L = log2 sum_j 2^S (base 2), P = 2^(S - L), dP = dO V^T, delta = rowsum(dO * O), dS = P * (dP - delta):

    O = P V        dQ = 0.125 * dS K        dK = ln 2 * dS^T qs        dV = P^T dO

(the closed formulas of the kernel header; dQ is with respect to the unscaled q = qs / (0.125 * log2 e), as in test_gpu_vit_train.py).
"""
import collections
import functools
import math

import torch

from conftest import within

HD = 64                 # head_dim
WT = 128                # rows (queries or keys) owned by one workgroup: 4 waves x 32          (attention_bwd.hip: WT)
ST = 64                 # rows per streamed tile                                                (attention_bwd.hip: ST)
WAVE_ROWS = 32          # rows owned by one wave
DEFER_THR = 8.0         # the forward moves its running maximum only when a score exceeds it by more than this  (attention.hip: DEFER_THR)
GROUP = 8               # (image, head) pairs per grid group: one per XCD                       (attention_bwd.hip: decode())
C_Q = 0.125 * 1.4426950408889634
LN2 = math.log(2.0)
F = 2.0                 # kernel error / model error, both against the f64 reference (see check())
GRADS = ("dq", "dk", "dv")


# ================================================================================================ arithmetic
def heads_of(t, heads):
    """[B, N, heads * 64] -> [B, heads, N, 64] f64"""
    B, N, D = t.shape
    return t.double().view(B, N, heads, HD).transpose(1, 2)


def bf16_round(x):
    return x.to(torch.bfloat16).double()


def _exact(x):
    return x


def _no_hook(stage, x):
    return x


def forward_running_max(S):
    """m_run of attn_fwd_v5_kernel at the moment each probability is rounded, restated from attention.hip:346-368: the maximum of the row's first 32 keys,
    then, per 32-key block, raised to the block's maximum (never lowered) for all 32 queries of a wave when ANY of them has a score more than DEFER_THR above
    its own m_run.  [B, heads, N, N] -> [B, heads, N, n_blocks]: the value in force for each block."""
    B, H, N, _ = S.shape
    pad = -N % WAVE_ROWS
    m, per_block = None, []
    for k0 in range(0, N, WAVE_ROWS):
        top = S[..., k0:k0 + WAVE_ROWS].amax(-1)
        if m is None:
            m = top
        else:
            over = torch.nn.functional.pad(top - m > DEFER_THR, (0, pad))
            fire = over.view(B, H, -1, WAVE_ROWS).any(-1, keepdim=True).expand(-1, -1, -1, WAVE_ROWS).reshape(B, H, N + pad)[..., :N]
            m = torch.where(fire, torch.maximum(m, top), m)
        per_block.append(m)
    return torch.stack(per_block, -1)


def forward_out(S, P, L, V, rnd):
    """`out` as the forward forms it.  It rounds its UNNORMALISED probabilities 2^(S - m_run) to bf16 in front of the P V product, rescales what it has by
    2^-(the move) when m_run moves, and divides by the f32 sum of the unrounded ones (attention.hip:357-377 and :402-404); with rnd = identity this is P V.
    m_run is in general not the row maximum, so the row's largest probability is no power of two and carries a full relative rounding: on a peaked row all
    of `out`, and with it delta, is off by up to 2^-9 coherently, which reaches dQ and dK row by row."""
    m = forward_running_max(S).repeat_interleave(WAVE_ROWS, -1)[..., :S.shape[-1]]        # per key: the m_run its probability was rounded under
    scale = torch.exp2(L.unsqueeze(-1) - m)                                                 # P * scale = 2^(S - m_run)
    return (rnd(P * scale) / scale) @ V


def backward(qs, k, v, do, heads, rnd, hook=_no_hook, rnd_forward=None):
    """The closed formulas, every sum in f64, ``rnd`` applied at the points the kernel sources document (``rnd_forward``, default ``rnd``: the one inside the
    forward).  ``hook(stage, tensor)`` may replace an intermediate: test_attn_bwd_host.py injects its faults through it; reference() and rounding_model()
    pass none."""
    Q, K, V, dO = (heads_of(t, heads) for t in (qs, k, v, do))
    S = Q @ K.transpose(2, 3)
    m = S.amax(-1, keepdim=True)
    L = hook("lse", (m + torch.log2(torch.exp2(S - m).sum(-1, keepdim=True))).squeeze(-1))
    P = hook("p", torch.exp2(S - L.unsqueeze(-1)))
    O = forward_out(S, P, L, V, rnd if rnd_forward is None else rnd_forward)
    delta = hook("delta", (dO * rnd(O)).sum(-1))                        # the dQ kernel reads the forward's bf16 `out` (attention_bwd.hip:144-146)
    dS = P * (dO @ V.transpose(2, 3) - delta.unsqueeze(-1))             # from the f32 P; P and dS are rounded separately (pack_b, :228 / :381)
    dS_q, dS_k, P_v = hook("ds_for_dq", rnd(dS)), hook("ds_for_dk", rnd(dS)), hook("p_for_dv", rnd(P))
    dq = rnd(hook("dq_scale", 0.125) * (dS_q @ K))                      # scale, then one rounding (store_rows64)
    dk = rnd(hook("dk_scale", LN2) * (dS_k.transpose(2, 3) @ Q))
    dv = rnd(P_v.transpose(2, 3) @ dO)
    return {"out": O, "lse": L, "delta": delta, "dq": dq, "dk": dk, "dv": dv}


def reference(qs, k, v, do, heads):
    """All f64, from the bf16-rounded operands, no rounding anywhere."""
    return backward(qs, k, v, do, heads, _exact)


def rounding_model(qs, k, v, do, heads, hook=_no_hook, forward=True):
    """The same formulas with the rounding points the kernel sources document and nothing else, every sum in f64.  The header of attention_bwd.hip gives:
    O to bf16 before delta, P and dS to bf16 before the gradient products, dQ / dK / dV to bf16.  ``forward`` adds the one attention.hip documents inside the
    forward that wrote `out` (forward_out); without it the GPU's dQ and dK rows measured up to 4.8 x the model's error on peaked rows, with it 1.0 x.
    The yardstick for tolerances -- not the code under test."""
    return backward(qs, k, v, do, heads, bf16_round, hook, None if forward else _exact)


# ================================================================================================ the tile walk
Walk = collections.namedtuple("Walk", "dq dkv dead_waves last_wave_partial nb grid")


def _parity(n):
    return "zero" if n == 0 else ("odd" if n & 1 else "even")


def walk(N, B, heads):
    """Every decision the launch and the two kernels take for this shape, restated from the kernel source.

    dq   (nfull parity, tail): attn_bwd_dq_kernel walks nt = ceil(N / 64) key tiles two per iteration; nfull = tiles with all 64 keys in range.  An odd
         nfull leaves one full tile for the remainder arm, which then runs the TAIL tile on buffer 1; an even one runs TAIL on buffer 0; nfull == 0 has
         only the TAIL tile.  tail = "none" (N % 64 == 0), "skipped" (N % 64 in 1..32: the second 32-key block is left by the break) or "masked"
         (33..63: the second block runs under the key >= N mask).
    dkv  (nmain parity, second): attn_bwd_dkv_kernel walks nmain = nt - 1 query tiles, then the LAST tile on buffer nmain & 1, whose second 32-query block
         is "skipped" when (nt - 1) * 64 + 32 >= N and "processed" otherwise.
    rows dead_waves = waves of the last workgroup whose 32 rows all lie past N (they only stage and keep the barriers); last_wave_partial = the last live
         wave has rows past N (clamped loads, ROW_DROPPED stores); nb = "one" or "many" 128-row blocks.
    grid npairs = B * heads against the group of 8: "lt8" (one partial group: workgroups with !mp.ok), "eq8", "gt8_full", "gt8_partial"."""
    nt = -(-N // ST)
    rem = N % ST
    nfull = nt - 1 if rem else nt
    tail = "none" if rem == 0 else ("skipped" if rem <= 32 else "masked")
    nmain = nt - 1
    second = "skipped" if nmain * ST + 32 >= N else "processed"
    nb = -(-N // WT)
    live_rows = N - (nb - 1) * WT
    live_waves = -(-live_rows // WAVE_ROWS)
    npairs = B * heads
    if npairs < GROUP:
        grid = "lt8"
    elif npairs == GROUP:
        grid = "eq8"
    else:
        grid = "gt8_full" if npairs % GROUP == 0 else "gt8_partial"
    return Walk((_parity(nfull), tail), (_parity(nmain), second), WT // WAVE_ROWS - live_waves, live_rows % WAVE_ROWS != 0,
                "one" if nb == 1 else "many", grid)


# ================================================================================================ cases and inputs
# (B, tokens, heads)
CASES = (
    (1, 26, 2), (2, 200, 3), (1, 1370, 2), (2, 129, 1),                                        # test_gpu_vit_train.py::test_attention_backward
    (1, 7, 1), (1, 33, 2), (1, 64, 1), (1, 100, 1), (2, 128, 1), (1, 165, 1), (1, 192, 3), (1, 256, 1),   # every (dq, dkv) pair of walk()
    (3, 40, 3), (1, 140, 8), (2, 70, 12), (2, 300, 12),                                        # grid: partial / exact / full groups, one and many row blocks
    (1, 485, 2), (1, 1029, 1), (1, 1374, 2),                                                   # 22x22 patches + CLS; DINOv3 at 512; DINOv2 + registers at 518
    # added by the coverage test of test_attn_bwd_host.py (smallest token counts already in the list that reach the class):
    (1, 40, 8), (3, 140, 3),                                                                   # exactly 8 pairs with one row block; a partial last group with many
    (1, 32, 1), (1, 96, 1),                                                                    # dead waves behind a FULL last live wave (3 and 1)
)
KINDS = ("randn", "edges")


def edge_rows(N):
    """Rows where a tile-walk error would land: the edges of the first 32-, 64- and 128-row blocks, of the last 64-row tile, the first rows of the last
    32- and 128-row blocks and the last two rows -- each where it exists."""
    t0 = (N - 1) // ST * ST
    cand = (0, 31, 32, 63, 64, 127, 128, t0, t0 + 31, t0 + 32, (N - 1) // WAVE_ROWS * WAVE_ROWS, (N - 1) // WT * WT, N - 2, N - 1)
    return sorted({i for i in cand if 0 <= i < N})


@functools.lru_cache(maxsize=None)
def inputs(case, kind):
    """(qs, k, v, do), [B, N, D] bf16, seeded per case.  "randn" is what test_attention_backward builds.  "edges" adds 3u to every query (u a unit vector
    per head), 4u to the keys at edge_rows(N) and multiplies dO by 8 there: probability and gradient mass sit on the rows a tile-boundary error would
    lose, so such an error is large at any N."""
    B, N, heads = case
    D = heads * HD
    g = torch.Generator().manual_seed(B * 1000 + N)
    q = torch.randn(B, N, D, generator=g) * 1.5
    k = torch.randn(B, N, D, generator=g) * 1.5
    v = torch.randn(B, N, D, generator=g)
    do = torch.randn(B, N, D, generator=g)
    if kind == "edges":
        u = torch.randn(heads, HD, generator=g)
        u = (u / u.norm(dim=1, keepdim=True)).reshape(D)
        rows = edge_rows(N)
        q = q + 3.0 * u
        k[:, rows] += 4.0 * u
        do[:, rows] *= 8.0
    elif kind != "randn":
        raise ValueError(kind)
    bf = lambda t: t.to(torch.bfloat16)                                     # noqa: E731
    return bf(bf(q).float() * C_Q), bf(k), bf(v), bf(do)


@functools.lru_cache(maxsize=None)
def expected(case, kind):
    """(reference, rounding model) of inputs(case, kind): computed once per session, shared by the tests, never modified."""
    ops = inputs(case, kind)
    return reference(*ops, case[2]), rounding_model(*ops, case[2])


# ================================================================================================ the checker
def slab_error(x, ref):
    """relative L2 error per (image, head) slab: [B, heads]"""
    return (x - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2).clamp_min(1e-300)


def row_error(x, ref):
    """largest per-row error over the slab's RMS row norm: [B, heads]"""
    rms = ref.norm(dim=3).pow(2).mean(dim=2).sqrt().clamp_min(1e-300)
    return (x - ref).norm(dim=3).amax(dim=2) / rms


def ratios(got, ref, model):
    """{(gradient, bound): largest over the slabs of (got's error / model's error)}, both errors against ``ref``."""
    out = {}
    for name in GRADS:
        for bound, fn in (("slab", slab_error), ("row", row_error)):
            e_got, e_model = fn(got[name].double(), ref[name]), fn(model[name], ref[name])
            r = torch.where(e_model > 0, e_got / e_model, torch.where(e_got > 0, torch.full_like(e_got, math.inf), torch.zeros_like(e_got)))
            out[name, bound] = float(r.max())
    return out


def check(name, got, ref, model, audit=True):
    """For dq, dk, dv and each (image, head) slab: (a) the slab's relative L2 error against ``ref`` is below F x the model's, (b) the largest per-row
    error over the slab's RMS row norm is below F x the model's largest.

    F = 2: the kernel's roundings are the model's plus f32 accumulation and the hardware exp2, both three orders of magnitude below a bf16 rounding;
    independent noise of equal size would give sqrt(2), and 2 leaves headroom without hiding a lost term (test_attn_bwd_host.py demonstrates that).  The
    bounds come from the model's distance to the f64 reference, never from GPU output.  Returns the measured ratios.  ``audit=False`` makes the same
    comparisons without recording them (the CPU fault-injection test, whose values are wrong on purpose)."""
    r = ratios(got, ref, model)
    for (grad, bound), value in r.items():
        label = f"attn_bwd:{name}:{grad}:{bound}_error_over_model"
        if audit:
            within(label, value, F)
        else:
            assert value < F, (label, value, F)
    return r
