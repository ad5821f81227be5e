#!/usr/bin/env python3
"""Micro-benchmark of ucod_gemm_bf16 variants on the backbone's shapes (random data, interleaved rounds in one process).

    python tools/gemm_bench.py [variants]          ViT-B shapes, the given variants (default 2,3,4,5,6)
    python tools/gemm_bench.py --swiglu [half]     DINOv2 ViT-g/14's fc1 (weights_in 1536 -> 8192) at 32 x 1370 rows, interleaved A/B of the fused SwiGLU epilogue
                                                   against the GELU epilogue on the same GEMM and against UCOD_EPI_BIAS_F32 + an unfused rows pass (half: bf16 / f16)
    python tools/gemm_bench.py --split16-fused     fp16-term split pass: interleaved A/B of ucod_split16_gemm_act (fc1 + activation + split in one launch) against the
                                                   pair it replaces, UCOD_EPI_BIAS_F32 + ucod_split16_rows, at ViT-B's fc1 (GELU) and ViT-g's (SwiGLU), 32 x 1370 rows
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


def split16_fused_ab(op, M, Nn, D, rounds=7, iters=10, variant=0):
    """Interleaved A/B on the fp16 library, K-concatenated fp16 split operands (K3 = 3 D), every form timed in every round: min and median over the rounds, in us.
      fused     ucod_split16_gemm_act                       -> fp16 [M, 3 N] (op 1, GELU) / [M, 3 N / 2] (op 3, SwiGLU)
      f32       UCOD_EPI_BIAS_F32                           -> f32 [M, N]      (the GEMM of the unfused pair alone)
      rows      ucod_split16_rows on that f32 buffer                           (the row pass alone)
      f32+rows  the two back to back                                           (what the unfused pass runs per layer)"""
    dev = "cuda"
    lib = N.load("f16")
    g = torch.Generator().manual_seed(Nn)
    x, w = torch.randn(M, D, generator=g).to(dev), (torch.randn(Nn, D, generator=g) * D ** -0.5).to(dev)
    s_ln, s_hid, sw = ops.split16_class_scale(N.SPLIT16_LN), ops.split16_class_scale(N.SPLIT16_HIDDEN), ops.pow2_scale(w)
    S = s_ln * sw
    xs, ws = ops.split_rows(x, 2, 0, term="f16", scale=s_ln), ops.split_rows(w, 2, 1, term="f16", scale=sw)
    del x, w
    b = torch.randn(Nn, generator=g).to(dev) * S
    Ko = Nn if op == 1 else Nn // 2
    o32 = torch.empty(M, Nn, device=dev, dtype=torch.float32)
    osp = torch.empty(M, 3 * Ko, device=dev, dtype=torch.float16)
    ofu = torch.empty(M, 3 * Ko, device=dev, dtype=torch.float16)
    fused = lambda: N.check(lib.ucod_split16_gemm_act(op, N.ptr(xs), N.ptr(ws), N.ptr(ofu), M, Nn, 3 * D, N.ptr(b), 1.0 / S, s_hid, variant, N.stream()), "gemm_act")  # noqa: E731
    f32 = lambda: N.check(lib.ucod_gemm_bf16(N.EPI_BIAS_F32, N.ptr(xs), N.ptr(ws), N.ptr(o32), M, Nn, 3 * D, N.ptr(b), None, None, None, 0, variant, N.stream()), "gemm")  # noqa: E731
    rows = lambda: N.check(lib.ucod_split16_rows(N.ptr(o32), Nn, N.ptr(osp), M, Ko, 0, op, 1.0 / S, s_hid, N.stream()), "rows")  # noqa: E731

    def pair():
        f32()
        rows()
    forms = {"fused": fused, "f32": f32, "rows": rows, "f32+rows": pair}
    res = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(ofu, osp))
    for _ in range(rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters): fn()
            e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / iters * 1e3)
    fl = 2.0 * M * Nn * D
    print(f"fp16 terms, op {op} ({'GELU' if op == 1 else 'SwiGLU'}), M={M} N={Nn} K={D} x 3 products ({fl / 1e9:.1f} GFLOP algorithmic), {rounds} interleaved rounds x {iters} "
          f"launches, variant {variant}; fused output bit-identical to the pair's: {same}")
    for k, t in res.items():
        t = sorted(t)
        print(f"  {k:9s} min {t[0]:8.1f} us  median {t[len(t) // 2]:8.1f} us  {fl / (t[0] * 1e-6) / 1e12:6.1f} TF/s algorithmic")
    med = lambda k: sorted(res[k])[len(res[k]) // 2]  # noqa: E731
    print(f"  fused / (f32 + rows) = {med('fused') / med('f32+rows'):.3f} (medians)   fused - f32 GEMM alone = {med('fused') - med('f32'):+.1f} us   rows alone = {med('rows'):.1f} us",
          flush=True)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--split16-fused":
        split16_fused_ab(1, 32 * 1370, 3072, 768)                # ViT-B/14 fc1 at C2
        split16_fused_ab(3, 32 * 1370, 8192, 1536)               # ViT-g/14 weights_in
        sys.exit(0)
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
