"""CPU references for the direct weight-gradient kernel (ucod_dpl_amd/csrc/wgrad.hip: ucod_wgrad_bf16_det) and the refiner's optimizer step, shared by
tests/test_refiner_step_host.py (CPU) and tests/test_gpu_refiner_wgrad.py / tests/test_gpu_refiner_step.py.

Test infrastructure only: nothing here is the code under test, and nothing here reads GPU output to set a bound.

* ``nsplit_rule`` / ``chunking``: the split of the token axis restated from include/ucod_dpl.h.  IT MUST MOVE WITH csrc/wgrad.hip.
* ``make_case``: operands inside wider, longer buffers (leading dimensions above the widths, live rows behind row M), either random or EXACT: dy integers in
  [-7, 7] times 2^-3, x integers in [-7, 7], the accumulate base integers times 2^-3.  Every product is a multiple of u = 2^-3 and every partial sum, in any
  order, stays below 2^24 u (asserted), so f32 arithmetic rounds nowhere and the expected dW holds bit for bit whatever the order of the additions --
  the idiom of tests/gemm_exact_ref.py.
* ``emulate``: the kernel's arithmetic chunk by chunk in f64 with named faults, for the host test that proves the checker.
* ``bound``: |err| <= c * 2^-24 * (sum_m |dy||x| + |base|) with c from the kernel's longest chain of f32 additions.
"""
import functools

import torch

TILE = 128              # wgrad.hip: WG_TILE
SLAB = 64               # wgrad.hip: WG_SLAB
MFMA_DEPTH = 16         # rows one v_mfma_f32_32x32x16_bf16 adds to the accumulator
CUS = 256               # wgrad.hip: WG_CUS
TWO24 = float(1 << 24)
FAULTS = ("drop_last_row", "chunk_twice", "tail_past_M", "no_accumulate")


def cdiv(a, b):
    return -(-a // b)


def nsplit_rule(M, N, K):
    """(nsplit, chunk) of include/ucod_dpl.h"""
    tiles = cdiv(N, TILE) * cdiv(K, TILE)
    n = max(1, min((CUS + tiles // 2) // tiles, cdiv(M, SLAB)))
    chunk = SLAB * cdiv(cdiv(M, n), SLAB)
    return cdiv(M, chunk), chunk


def chunking(M, nsplit):
    """(chunk, [(first row, end row) of chunk s]) from nsplit alone, as the issue states it"""
    chunk = SLAB * cdiv(cdiv(M, nsplit), SLAB)
    return chunk, [(s * chunk, min(M, (s + 1) * chunk)) for s in range(nsplit)]


def chain_length(M, nsplit):
    """the longest chain of f32 additions behind one element of dW: one per MFMA of a chunk (an MFMA adds its 16 products to the accumulator in one
    step), one per partial, one into dW"""
    chunk, _ = chunking(M, nsplit)
    return chunk // MFMA_DEPTH + nsplit + 1


def bound(case, nsplit):
    """[N, K] f64: c u / (1 - c u) * (sum_m |dy||x| + |base|), u = 2^-24 -- the standard bound of a sum of c roundings, each relative to a partial
    sum that the absolute sum dominates.  Derived from the chain, never from a measurement."""
    c, u = chain_length(case["M"], nsplit), 2.0 ** -24
    mag = case["dy"].double().abs().t() @ case["x"].double().abs()
    if case["accumulate"]:
        mag = mag + case["base"].double().abs()
    return c * u / (1 - c * u) * mag


@functools.lru_cache(maxsize=None)
def make_case(M, N, K, kind="exact", accumulate=False, wide=False, seed=0):
    """dict: dy_buf bf16 [M + 3, ld_dy], x_buf bf16 [M + 3, ld_x] (rows M .. M+2 hold LIVE values: a kernel that reads past M gets a wrong answer, not a
    fault), col (first column of dy inside its buffer: ``wide`` puts dy in the second half of a [., 2N] buffer, as V lies in kv), dy / x the [M, N] / [M, K]
    views, base f32 [N, K] (what dW holds before the call), ref f64 [N, K] = (accumulate ? base : 0) + dy^T x.  Never modified by a test."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * M + N + 3 * K)
    ld_dy, col, ld_x = (2 * N, N, K + 8) if wide else (N, 0, K)
    if kind == "exact":
        dyb = torch.randint(-7, 8, (M + 3, ld_dy), generator=g).double() / 8
        xb = torch.randint(-7, 8, (M + 3, ld_x), generator=g).double()
        base = torch.randint(-1000, 1001, (N, K), generator=g).double() / 8
        assert (49 * (M + 3) + 1000) < TWO24, "the case is not exact in f32"
    else:
        dyb = torch.randn(M + 3, ld_dy, generator=g).double()
        xb = torch.randn(M + 3, ld_x, generator=g).double()
        base = torch.randn(N, K, generator=g).double() * 3
    dyb, xb, base = dyb.to(torch.bfloat16), xb.to(torch.bfloat16), base.float()
    dy, x = dyb[:M, col:col + N], xb[:M, :K]
    ref = dy.double().t() @ x.double() + (base.double() if accumulate else 0)
    if kind == "exact":
        assert bool((ref.float().double() == ref).all())
    return dict(M=M, N=N, K=K, kind=kind, accumulate=accumulate, dy_buf=dyb, x_buf=xb, col=col, dy=dy, x=x, base=base, ref=ref)


def emulate(case, nsplit, fault=None):
    """f64 [N, K]: the kernel's sums chunk by chunk.  Faults: "drop_last_row" (the last row of chunk 0 is not added), "chunk_twice" (the last partial is
    added twice), "tail_past_M" (the last slab is read whole: live rows behind M come in), "no_accumulate" (dW is overwritten where it should be added to)."""
    assert fault is None or fault in FAULTS
    M, N, col = case["M"], case["N"], case["col"]
    dyb, xb = case["dy_buf"].double()[:, col:col + N], case["x_buf"].double()[:, :case["K"]]
    _, ranges = chunking(M, nsplit)
    parts = []
    for s, (a, b) in enumerate(ranges):
        if fault == "drop_last_row" and s == 0:
            b -= 1
        if fault == "tail_past_M" and s == nsplit - 1:
            b = min(dyb.shape[0], a + SLAB * cdiv(b - a, SLAB))
        parts.append(dyb[a:b].t() @ xb[a:b])
    if fault == "chunk_twice":
        parts.append(parts[-1])
    total = sum(parts[1:], parts[0])
    if case["accumulate"] and fault != "no_accumulate":
        total = case["base"].double() + total
    return total


def check(case, got, nsplit):
    """None when ``got`` [N, K] passes, else a string saying what failed: bit equality for an exact case, the derived bound for a random one"""
    got = got.detach().cpu()
    if case["kind"] == "exact":
        return None if torch.equal(got.double(), case["ref"]) else f"exact case differs in {int((got.double() != case['ref']).sum())} elements"
    err, lim = (got.double() - case["ref"]).abs(), bound(case, nsplit)
    worst = float((err / lim.clamp_min(1e-300)).max())
    return None if bool((err <= lim).all()) else f"error / bound = {worst:.3g}"


# ================================================================================================ the optimizer step
ADAMW_LR = 1e-4                       # configs/uscod/CORAL_dinov2.py: train_cfg.lr0 (AdamW's other hyper-parameters are torch's defaults, runner.py:444-460)


def adamw_cpu(p, g, m, v, ema, lr, step, ema_alpha=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01):
    """ops.adamw_ema's contract with no EMA target, in torch on the CPU (torch.optim.AdamW's single-tensor algorithm): lets the host test drive the loop's own
    segment rule without a GPU"""
    import math
    assert ema is None
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    p.addcdiv_(m, (v.sqrt() / math.sqrt(1 - beta2 ** step)).add_(eps), value=-lr / (1 - beta1 ** step))


@functools.lru_cache(maxsize=None)
def adamw_losses(mode="f64", steps=5, lr=ADAMW_LR, tag="full", kind="prob"):
    """ex_loss at the start of each of ``steps`` torch.optim.AdamW(lr) steps on the HRE.CSF parameters through the CPU oracle, the batch, the selected windows
    and the loss constants held fixed (the first stage is frozen): mode "f64" (the reference) or "autocast" (f32 parameters under bf16 autocast, the yardstick)."""
    import contextlib
    from unittest import mock
    import refiner_train_ref as R
    fx = R.fixture(tag, kind)
    dt = torch.float64 if mode == "f64" else torch.float32
    sd = {k: v.to(dt).clone().requires_grad_(k.startswith(R.CSF)) for k, v in fx["sd"].items()}
    params = [sd[k] for k in fx["names"]]
    opt = torch.optim.AdamW(params, lr=lr)
    out = []
    for _ in range(steps):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=(mode == "autocast")), \
                (mock.patch.object(R.OR, "F", R._UnfoldF64()) if mode == "f64" else contextlib.nullcontext()):
            wp = R.OR.csf(fx["l_sel"].to(dt), fx["h_sel"].to(dt), sd)
            loss, _, _ = R.OR.cal_ex_loss(fx["preds"].to(dt), wp.to(dt), fx["mask"], fx["ht"].to(dt), 3)
        out.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return tuple(out)


def loss_deviation(losses, ref):
    """the largest relative distance of a loss sequence from the f64 one"""
    return max(abs(a - b) / abs(b) for a, b in zip(losses, ref))


ARENA_ORDER_TAIL =("GE.fuser.0.weight", "GE.fuser.0.bias", "GE.fuser.2.weight", "GE.fuser.2.bias", "GE.alpha")


def arena_layout(module):
    """[(state-dict name, offset, numel)] of the flat refiner arena: the 18 HRE.CSF parameters in named_parameters order, the four fuser parameters, GE.alpha"""
    names = ["HRE.CSF." + n for n, _ in module.HRE.CSF.named_parameters()] + list(ARENA_ORDER_TAIL)
    sd = dict(module.named_parameters())
    out, off = [], 0
    for n in names:
        out.append((n, off, sd[n].numel()))
        off += sd[n].numel()
    return out
