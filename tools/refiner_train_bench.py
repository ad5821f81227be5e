#!/usr/bin/env python3
"""Training of the CORAL refiner's window branch at the config's full size (configs/uscod/CORAL_*.py: window length 56 -> 3136 tokens per window, C = 768,
B = 2, all 18 windows selected, random init), one process:
  1. SparseRefiner eval forward beside the training-mode forward + ex_loss.backward(), interleaved, median of ROUNDS x REPS (device events);
  2. ucod_cross_attention96_fwd / _fwd_lse and ucod_cross_attention96_bwd alone, in TF/s against the 2.5 PF/s bf16 peak, the two backward kernels apart
     where the profiler names them;
  3. the six weight gradients (two ucod_transpose_pad_bf16 + one ucod_gemm_bf16 each) alone, and their share of the step;
  4. peak memory of the step above the resident state.
    refiner_train_bench.py [rounds [reps]]     -> profiles/refiner_train_bench.txt (and stdout)"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ucod_dpl_amd import native as N, ops
from ucod_dpl_amd.engine.config import CfgNode
from ucod_dpl_amd.models.UDLR import SparseRefiner, HEADS

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
PEAK_TF = 2500.0
B, WS, WL, C, HD = 2, 3, 56, 768, 96
DEV = "cuda"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(forms):
    """{name: fn} -> {name: median over ROUNDS of the mean of REPS calls}, the forms taking turns inside every round"""
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timed(fn, REPS))
    return {k: statistics.median(v) for k, v in times.items()}, times


def main():
    torch.manual_seed(0)
    m = SparseRefiner.from_config(CfgNode(dict(window_size=WS, threshold=0.0015))).to(DEV)
    g = torch.Generator().manual_seed(1)
    l = torch.randn(B, C, WL, WL, generator=g).to(DEV)
    h = torch.randn(B, WS * WS, C, WL, WL, generator=g).to(DEV)
    preds = (torch.randn(B, 1, WL, WL, generator=g) * 2).to(DEV)
    ht = torch.rand(B * WS * WS, 1, WL, WL, generator=g).to(DEV)
    n, HW = B * WS * WS, WL * WL
    M = n * HW

    def eval_fwd():
        with torch.no_grad():
            return m.eval()(l, h, preds)

    def train_step():
        m.train()
        for p in m.parameters():
            p.grad = None
        _, ex, opt = m(l, h, preds, ht)
        ex.backward()
        return opt

    assert int(train_step()["mask"].sum()) == n, "not every window was selected"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    eval_fwd()
    torch.cuda.synchronize()
    peak_eval = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    train_step()
    torch.cuda.synchronize()
    peak_train = torch.cuda.max_memory_allocated() - base
    med, rounds = interleaved({"eval forward": eval_fwd, "train forward + backward": train_step})
    say(f"# 1. SparseRefiner at {n} windows x {HW} tokens, C = {C} (median of {ROUNDS} x {REPS}, interleaved)")
    for k in med:
        say(f"{k:26s} {med[k]:9.3f} ms   (rounds {', '.join(f'{t:.3f}' for t in rounds[k])})")
    say(f"training step / eval forward = {med['train forward + backward'] / med['eval forward']:.2f}")
    step_ms = med["train forward + backward"]

    # ---- 2. the attention kernels alone
    lib, st = N.load(), N.stream
    bf = lambda *s: (torch.randn(*s, device=DEV) * 0.5).to(torch.bfloat16)          # noqa: E731
    q, kv, do = bf(M, C) * 0.15, bf(M, 2 * C), bf(M, C)
    att, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
    lse, delta = (torch.empty(n, HEADS, HW, device=DEV) for _ in range(2))
    kp, vp = kv.data_ptr(), kv.data_ptr() + 2 * C
    fwd = lambda: N.check(lib.ucod_cross_attention96_fwd(N.ptr(q), C, kp, vp, 2 * C, N.ptr(att), n, HW, HW, HEADS, st()), "fwd")          # noqa: E731
    fwd_lse = lambda: N.check(lib.ucod_cross_attention96_fwd_lse(N.ptr(q), C, kp, vp, 2 * C, N.ptr(att), N.ptr(lse), n, HW, HW, HEADS, st()), "fwd_lse")   # noqa: E731
    bwd = lambda: N.check(lib.ucod_cross_attention96_bwd(N.ptr(q), C, kp, vp, 2 * C, N.ptr(att), N.ptr(do), N.ptr(lse), N.ptr(delta), N.ptr(dq), C, N.ptr(dkv),  # noqa: E731
                                                         dkv.data_ptr() + 2 * C, 2 * C, n, HW, HW, HEADS, st()), "bwd")
    med, _ = interleaved({"fwd": fwd, "fwd_lse": fwd_lse, "bwd": bwd})
    prod = 2.0 * n * HEADS * HW * HW * HD                           # FLOP of one [HW, 96] x [96, HW]-sized product over all (window, head) pairs
    say(f"# 2. head_dim-96 attention alone, {n} x {HEADS} (window, head) pairs of {HW} x {HW} (TF/s against the {PEAK_TF / 1000:.1f} PF/s bf16 peak)")
    say(f"ucod_cross_attention96_fwd      {med['fwd']:8.3f} ms  {2 * prod / med['fwd'] / 1e9:7.1f} TF/s = {2 * prod / med['fwd'] / 1e9 / PEAK_TF * 100:4.1f} %  (2 products)")
    say(f"ucod_cross_attention96_fwd_lse  {med['fwd_lse']:8.3f} ms  {2 * prod / med['fwd_lse'] / 1e9:7.1f} TF/s = {2 * prod / med['fwd_lse'] / 1e9 / PEAK_TF * 100:4.1f} %")
    say(f"ucod_cross_attention96_bwd      {med['bwd']:8.3f} ms  {7 * prod / med['bwd'] / 1e9:7.1f} TF/s = {7 * prod / med['bwd'] / 1e9 / PEAK_TF * 100:4.1f} %  (7 products: S and dP in both "
        f"kernels, dQ, dK, dV; a one-pass backward would need 5 = 2.5 x the forward)")
    say(f"backward pair / forward = {med['bwd'] / med['fwd_lse']:.2f} in time (3.5 in MFMA work as built, 2.5 for a one-pass backward)")
    # ---- 3. the weight gradients alone
    say("# 3. weight gradients: two ucod_transpose_pad_bf16 + ucod_gemm_bf16(A = dY^T, B = X^T, K = Mp) each")
    total = 0.0
    for name, Nn, K in (("q", C, C), ("kv", 2 * C, C), ("out_proj", C, C), ("fc1", 4 * C, C), ("fc2", C, 4 * C)):
        dy, x = bf(M, Nn), bf(M, K)
        out = torch.empty(Nn, K, device=DEV)
        both = lambda: ops.weight_grad(dy, x, out=out)                              # noqa: E731
        tr = lambda: (ops.transpose_pad_bf16(dy), ops.transpose_pad_bf16(x))        # noqa: E731
        med, _ = interleaved({"both": both, "tr": tr})
        total += med["both"]
        say(f"{name:9s} dW [{Nn:4d},{K:4d}] over M = {M}: {med['both']:7.3f} ms, of which transposes {med['tr']:7.3f} ms; GEMM {2.0 * M * Nn * K / (med['both'] - med['tr']) / 1e9:6.1f} TF/s")
        del dy, x, out
    say(f"sum {total:.3f} ms = {total / step_ms * 100:.1f} % of the training step ({step_ms:.3f} ms)")
    say(f"# 4. peak memory above the resident state: eval forward +{peak_eval / 2**20:.0f} MiB, training step +{peak_train / 2**20:.0f} MiB "
        f"(saved activations, cotangents, transposed operands and reduction workspaces)")
    write()
    say("# 5. the two backward kernels apart (profiler kernel records)")
    kernel_split(bwd, prod)


def kernel_split(bwd, prod):
    """the two backward kernels apart, by the profiler's kernel records (a convenience behind everything else: the pair's time above stands without it)"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(REPS):
                bwd()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if "attn96_bwd" in ev.key:
                name = "attn96_bwd_dq_kernel " if "dq_kernel" in ev.key else "attn96_bwd_dkv_kernel"
                nprod = 3 if "dq_kernel" in ev.key else 4
                t = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                say(f"  {name} {t / 1e3:8.3f} ms  {nprod * prod / (t / 1e3) / 1e9:7.1f} TF/s  ({nprod} products)")
    except Exception as e:
        say(f"  (per-kernel split not available: {type(e).__name__})")


def write():
    out = os.path.join(ROOT, "profiles", "refiner_train_bench.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("refiner_train_bench.py measures on the GPU: none found")
    say(f"refiner_train_bench.py {' '.join(sys.argv[1:])}  ({torch.cuda.get_device_name(0)})")
    main()
    write()
