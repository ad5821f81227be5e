#!/usr/bin/env python3
"""Micro-benchmark of ucod_gemm_bf16 variants on the backbone's shapes (random data, interleaved rounds in one process).

    python tools/gemm_bench.py [variants]          ViT-B shapes, the given variants (default 2,3,4,5,6)
    python tools/gemm_bench.py --swiglu [half]     DINOv2 ViT-g/14's fc1 (weights_in 1536 -> 8192) at 32 x 1370 rows, interleaved A/B of the fused SwiGLU epilogue
                                                   against the GELU epilogue on the same GEMM and against UCOD_EPI_BIAS_F32 + an unfused rows pass (half: bf16 / f16)
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N, ops

def run(M, Nn, K, epi, variants, rounds=5, iters=10):
    dev = "cuda"
    A = torch.randn(M, K, device=dev).to(torch.bfloat16)
    W = (torch.randn(Nn, K, device=dev) * 0.05).to(torch.bfloat16)
    b = torch.randn(Nn, device=dev); sc = torch.ones(Nn, device=dev); resid = torch.randn(M, Nn, device=dev)
    out = torch.empty(M, Nn, device=dev, dtype=torch.float32 if epi == N.EPI_BIAS_SCALE_RESID_F32 else torch.bfloat16)
    res = {v: [] for v in variants}
    for r in range(rounds):
        for v in variants:
            kw = dict(bias=b, variant=v)
            if epi == N.EPI_BIAS_SCALE_RESID_F32: kw.update(scale=sc, resid=resid)
            ops.gemm_bf16(epi, A, W, out, M, Nn, K, **kw)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters): ops.gemm_bf16(epi, A, W, out, M, Nn, K, **kw)
            e1.record(); torch.cuda.synchronize()
            res[v].append(e0.elapsed_time(e1) / iters * 1e3)
    fl = 2.0 * M * Nn * K
    return {v: (min(t), fl / (min(t) * 1e-6) / 1e12) for v, t in res.items()}


def swiglu_ab(half="bf16", M=32 * 1370, Nn=8192, K=1536, rounds=7, iters=10):
    """Interleaved A/B at one shape, every form timed in every round (auto variant, the product path): min and median over the rounds, in us.
      swiglu   UCOD_EPI_BIAS_SWIGLU_BF16 -> 16-bit [M, N/2]                (the fused form)
      gelu     UCOD_EPI_BIAS_GELU_BF16   -> 16-bit [M, N]                  (the same GEMM with the GELU epilogue: the gate's yardstick)
      f32      UCOD_EPI_BIAS_F32         -> f32 [M, N]                     (the GEMM of any unfused form: a lower bound on f32 + rows)
      f32+rows UCOD_EPI_BIAS_F32 + ucod_split_rows op 3 (two terms)        (the unfused pair the split pass runs; bf16 library only)"""
    dev = "cuda"
    lib = N.load(half)
    dt = torch.float16 if half == "f16" else torch.bfloat16
    A = torch.randn(M, K, device=dev).to(dt)
    W = (torch.randn(Nn, K, device=dev) * K ** -0.5).to(dt)
    b = torch.randn(Nn, device=dev)
    o16 = torch.empty(M, Nn, device=dev, dtype=dt)
    o32 = torch.empty(M, Nn, device=dev, dtype=torch.float32)
    osp = torch.empty(M, 3 * (Nn // 2), device=dev, dtype=torch.bfloat16) if half == "bf16" else None
    g = lambda epi, out: N.check(lib.ucod_gemm_bf16(epi, N.ptr(A), N.ptr(W), N.ptr(out), M, Nn, K, N.ptr(b), None, None, None, 0, 0, N.stream()), "gemm")  # noqa: E731
    forms = {"swiglu": lambda: g(N.EPI_BIAS_SWIGLU_BF16, o16), "gelu": lambda: g(N.EPI_BIAS_GELU_BF16, o16), "f32": lambda: g(N.EPI_BIAS_F32, o32)}
    if osp is not None:
        def f32_rows():
            g(N.EPI_BIAS_F32, o32)
            N.check(lib.ucod_split_rows(N.ptr(o32), Nn, N.ptr(osp), M, Nn // 2, 2, 0, 3, 1.0, N.stream()), "split_rows")
        forms["f32+rows"] = f32_rows
    res = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters): fn()
            e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / iters * 1e3)
    fl = 2.0 * M * Nn * K
    print(f"{half} library, M={M} N={Nn} K={K} ({fl / 1e9:.1f} GFLOP), {rounds} interleaved rounds x {iters} launches, auto variant:")
    for k, t in res.items():
        t = sorted(t)
        print(f"  {k:9s} min {t[0]:8.1f} us  median {t[len(t) // 2]:8.1f} us  {fl / (t[0] * 1e-6) / 1e12:6.1f} TF/s")
    sw, ge, f32 = min(res["swiglu"]), min(res["gelu"]), min(res["f32"])
    print(f"  swiglu / gelu = {sw / ge:.3f} (gate <= 1.05)   swiglu / f32 GEMM alone = {sw / f32:.3f} (< 1: beats f32 + any rows pass)"
          + (f"   swiglu / (f32 + rows) = {sw / min(res['f32+rows']):.3f}" if "f32+rows" in res else ""), flush=True)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--swiglu":
        for half in (sys.argv[2:] or ["bf16", "f16"]):
            swiglu_ab(half)
        sys.exit(0)
    variants = [int(x) for x in (sys.argv[1].split(",") if len(sys.argv) > 1 else "2,3,4,5,6".split(","))]
    M = 32 * 1370
    shapes = [("qkv", M, 2304, 768, N.EPI_BIAS_BF16), ("fc1", M, 3072, 768, N.EPI_BIAS_GELU_BF16), ("proj", M, 768, 768, N.EPI_BIAS_SCALE_RESID_F32),
              ("fc2", M, 768, 3072, N.EPI_BIAS_SCALE_RESID_F32), ("sq4k", 4096, 4096, 4096, N.EPI_BIAS_BF16), ("sq8k", 8192, 8192, 8192, N.EPI_BIAS_BF16),
              ("fc1_nogelu", M, 3072, 768, N.EPI_BIAS_BF16), ("fc2_bf16out", M, 768, 3072, N.EPI_BIAS_BF16)]
    for name, m, n, k, epi in shapes:
        r = run(m, n, k, epi, variants)
        print(f"{name:12s} M={m} N={n} K={k}: " + "  ".join(f"v{v}: {t:7.1f}us {tf:6.1f}TF" for v, (t, tf) in r.items()), flush=True)
