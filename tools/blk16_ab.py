#!/usr/bin/env python3
"""Isolated A/B of the MLP pair in BLK16 (MFMA-fragment) order against the row-major pair, on the backbone's shapes (fp16-operand library, ONE process,
interleaved rounds): fc1 = ucod_gemm_lnfold (LayerNorm folded, GELU; statistics from row partials as in the engine's large passes), N = 3072, K = 768;
fc2 = the fp16-residual producer with row partials, N = 768, K = 3072; M = 32 x 1370 and 16 x 1370.
  python tools/blk16_ab.py            (BLK16_ROUNDS, BLK16_ITERS, BLK16_WARM: default 9 timed rounds of 200 launches behind 3 discarded ones -- shorter
                                       rounds measure the clock: at 50 launches the row-major spread was 4.4 us, at 200 it is 1.4-1.8 us; the arm order
                                       alternates from round to round so that a clock drift does not favour one arm)
Per shape and arm: median / min / spread (max - min of the per-round means) in us, and the gate of the BLK16 change: fc1 faster by more than the row-major
arm's spread, fc2 not slower by more than it."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ucod_dpl_amd import blk16, native as N, ops  # noqa: E402

ROUNDS, ITERS, WARM = int(os.environ.get("BLK16_ROUNDS", "9")), int(os.environ.get("BLK16_ITERS", "200")), int(os.environ.get("BLK16_WARM", "3"))
D, F, EPS = 768, 3072, 1e-6
lib = N.load("f16")
st = N.stream()
g = torch.Generator(device="cuda").manual_seed(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3


def ab(name, arms, flops):
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(WARM + ROUNDS):
        order = list(arms.items())
        for k, fn in (order if r % 2 == 0 else order[::-1]):
            t = timed(fn)
            if r >= WARM:
                times[k].append(t)
    res = {}
    for k, t in times.items():
        res[k] = (statistics.median(t), min(t), max(t) - min(t))
        print(f"{name:22s} {k:10s}: median {res[k][0]:7.1f} us  min {res[k][1]:7.1f} us  spread {res[k][2]:5.1f} us  {flops / (res[k][0] * 1e-6) / 1e12:7.1f} TF/s   rounds "
              + " ".join(f"{x:.1f}" for x in t))
    return res


print(f"# BLK16 A/B: {ROUNDS} interleaved rounds x {ITERS} launches ({WARM} rounds discarded first), us per launch")
ok = True
for M in (32 * 1370, 16 * 1370):
    Mp = blk16.padded_rows(M)
    # the residual stream and its row partials, as a producer leaves them
    x0 = (torch.randn(M, D, device="cuda", generator=g) * 1.5).half()
    z = torch.zeros(M, 128, dtype=torch.float16, device="cuda")
    x, part = ops.linear_scale_resid_h16_stats(z, torch.zeros(D, 128, dtype=torch.float16, device="cuda"), torch.zeros(D, device="cuda"), torch.ones(D, device="cuda"), x0)
    w1, b1 = torch.randn(F, D, device="cuda", generator=g) * 0.04, torch.randn(F, device="cuda", generator=g) * 0.1
    gamma, beta = 1 + 0.3 * torch.randn(D, device="cuda", generator=g), 0.2 * torch.randn(D, device="cuda", generator=g)
    wf, bf_, cs = ops.fold_layernorm_linear(gamma, beta, w1, b1)
    h_rm = torch.empty(M, F, dtype=torch.float16, device="cuda")
    h_blk = torch.empty(Mp * F, dtype=torch.float16, device="cuda")

    def fc1(epi, out):
        N.check(lib.ucod_gemm_lnfold(epi, N.ptr(x), N.ptr(wf), N.ptr(out), M, F, D, N.ptr(bf_), N.ptr(cs), None, N.ptr(part), D // 64, EPS, None, 0, st), "fc1")
    r1 = ab(f"fc1 M={M}", {"row-major": lambda: fc1(N.EPI_LNFOLD_GELU_BF16, h_rm), "blk16": lambda: fc1(N.EPI_LNFOLD_GELU_BLK16, h_blk)}, 2.0 * M * F * D)
    same = torch.equal(blk16.unpack(h_blk, M, F), h_rm)
    print(f"    hidden bit-identical: {same}")
    w2 = (torch.randn(D, F, device="cuda", generator=g) * 0.02).half()
    w2p = blk16.permute_weight(w2)
    b2, ls = torch.randn(D, device="cuda", generator=g) * 0.1, torch.rand(D, device="cuda", generator=g) * 1e-3      # (in place: the stream stays in range over every timed launch)
    o_rm, o_blk = x.clone(), x.clone()
    p_rm, p_blk = torch.empty_like(part), torch.empty_like(part)
    rm = lambda: N.check(lib.ucod_gemm_bf16_stats(N.EPI_BIAS_SCALE_RESID_H16_STATS, N.ptr(h_rm), N.ptr(w2), N.ptr(o_rm), M, D, F, N.ptr(b2), N.ptr(ls), N.ptr(o_rm), None, 0,
                                                  N.ptr(p_rm), D // 64, st), "fc2")
    bl = lambda: N.check(lib.ucod_gemm_bf16_blk16a(N.EPI_BIAS_SCALE_RESID_H16_STATS, N.ptr(h_blk), N.ptr(w2p), N.ptr(o_blk), M, D, F, N.ptr(b2), N.ptr(ls), N.ptr(o_blk),
                                                   N.ptr(p_blk), D // 64, st), "fc2 blk16")
    r2 = ab(f"fc2 M={M}", {"row-major": rm, "blk16": bl}, 2.0 * M * F * D)
    o_rm.copy_(x)                                                    # (one launch each from the same rows: the timed launches accumulate in place)
    o_blk.copy_(x)
    rm()
    bl()
    torch.cuda.synchronize()
    print(f"    fc2, one launch from the same rows: max |diff| {float((o_rm.float() - o_blk.float()).abs().max()):.3e}  partials max |diff| {float((p_rm - p_blk).abs().max()):.3e}")
    g1 = r1["row-major"][0] - r1["blk16"][0]
    g2 = r2["row-major"][0] - r2["blk16"][0]
    pass1, pass2 = g1 > r1["row-major"][2], g2 > -r2["row-major"][2]
    print(f"    gate M={M}: fc1 gain {g1:+.1f} us vs row-major spread {r1['row-major'][2]:.1f} -> {'PASS' if pass1 else 'FAIL'};  "
          f"fc2 gain {g2:+.1f} us vs spread {r2['row-major'][2]:.1f} -> {'PASS' if pass2 else 'FAIL'};  pair {g1 + g2:+.1f} us")
    ok = ok and same and pass1 and pass2
print("GATE (a):", "PASS" if ok else "FAIL")
