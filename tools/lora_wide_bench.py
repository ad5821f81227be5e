#!/usr/bin/env python3
"""The wide LoRA row kernels (UCOD_LORA_WIDE: dinov3_vith16plus, hidden 5120) beside the narrow ones they extend, per launch, interleaved in ONE process.

    lora_wide_bench.py [images [windows]]          (defaults 8, 7: M = images x 1029 rows, the tokens of a 512 x 512 DINOv3 image)

1  ucod_lora_mlp_pair_grad_wide at (M, N1 = 10240, D = 1280) -- five vectors per thread, one rank per pass -- beside ucod_lora_mlp_pair_grad at (M, 8192, 1280) --
   four vectors, two ranks per pass -- r = 2 and 8, dropout 0.05.  A launch is all its passes (gradient kernel + reduce each).  Bytes: what the algorithm needs,
   ONE read of dpre [M, N1] and of h2_aug [M, D + 64] per launch, and beside it the bytes the passes actually read (r passes wide, ceil(r / 2) narrow).
2  ucod_lora_out_fwd_wide at K = 5120 -- blocks of 512 threads -- beside ucod_lora_out_fwd at K = 4096, D = 1280, r = 2 and 8, f32 and fp16 stream, dropout 0.05.
   Bytes: x_in [M, K] bf16 read, the stream row [M, D] read and written, u [M, 8] written.
Windows of 20 launches, the two kernels of a pair in alternating windows; median and min .. max over the windows.
"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N

images = int(sys.argv[1]) if len(sys.argv) > 1 else 8
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
lib = N.load()
DEV = "cuda"
M, D, PER = images * 1029, 1280, 20


def timed(fn, n):
    """ms per call of ``fn`` over one window of ``n`` calls (device time between two events)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(calls):
    for fn in calls.values():
        timed(fn, 5)
    ts = {k: [] for k in calls}
    for _ in range(windows):
        for k, fn in calls.items():
            ts[k].append(timed(fn, PER))
    return ts


def report(name, ts, byts, extra=""):
    med = statistics.median(ts)
    print(f"  {name:34s} median {med * 1e3:9.1f} us   min .. max {min(ts) * 1e3:9.1f} .. {max(ts) * 1e3:9.1f} us   {byts / 1e6:7.1f} MB   {byts / (med * 1e-3) / 1e12:.2f} TB/s{extra}")
    return byts / (med * 1e-3)


print(f"1. the MLP input's pair gradient, M = {M} rows, D = {D}, dropout 0.05 ({windows} alternating windows of {PER} launches)")
g = torch.Generator().manual_seed(1)
h = torch.randn(M, D + N.LORA_AUG, generator=g).bfloat16().to(DEV)
t = torch.zeros(M, N.LORA_AUG, dtype=torch.bfloat16, device=DEV)
drop = C.byref(N.LoraDropout(0.05, 1234, 14))
dpres = {n1: torch.randn(M, n1, generator=g).bfloat16().to(DEV) for n1 in (8192, 10240)}
for r in (2, 8):
    calls, need, read = {}, {}, {}
    for name, fn, wsf, N1, passes in (("ucod_lora_mlp_pair_grad       8192", lib.ucod_lora_mlp_pair_grad, lib.ucod_lora_mlp_pair_grad_workspace_bytes, 8192, (r + 1) // 2),
                                      ("ucod_lora_mlp_pair_grad_wide 10240", lib.ucod_lora_mlp_pair_grad_wide, lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide, 10240, r)):
        lora = (0.05 * torch.randn(r * (2 * D + N1), generator=g)).to(DEV)
        grad, wsb = torch.zeros_like(lora), wsf(N1, D)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        calls[name] = (lambda fn=fn, lora=lora, grad=grad, ws=ws, wsb=wsb, N1=N1, name=name:
                       N.check(fn(N.ptr(dpres[N1]), N.ptr(h), N.ptr(lora), r, 2.0, N.ptr(grad), N.ptr(t), N.ptr(ws), wsb, M, N1, D, drop, N.stream()), name))
        need[name] = M * (N1 + D + N.LORA_AUG) * 2
        read[name] = passes * need[name]
    ts = alternate(calls)
    print(f" r = {r}")
    rates = {k: report(k, v, need[k], f"   (all passes read {read[k] / 1e6:.1f} MB: {read[k] / (statistics.median(v) * 1e-3) / 1e12:.2f} TB/s)") for k, v in ts.items()}
    a, b = rates.values()
    print(f"  wide / narrow, bytes the algorithm needs per second: {b / a:.2f}")
del dpres, h, calls

print(f"2. the output projection's forward, M = {M} rows, D = {D}, dropout 0.05")
drop = C.byref(N.LoraDropout(0.05, 1234, 29))
xins = {k: torch.randn(M, k, generator=g).bfloat16().to(DEV) for k in (4096, 5120)}
lam = (torch.rand(D, generator=g) + 0.5).to(DEV)
u = torch.zeros(M, N.LORA_OUT_W, device=DEV)
for h16 in (0, 1):
    xs = torch.zeros(M, D, dtype=torch.float16 if h16 else torch.float32, device=DEV)
    for r in (2, 8):
        calls, byts = {}, {}
        for name, fn, K in (("ucod_lora_out_fwd      4096", lib.ucod_lora_out_fwd, 4096), ("ucod_lora_out_fwd_wide 5120", lib.ucod_lora_out_fwd_wide, 5120)):
            lora = (0.001 * torch.randn(r * (K + D), generator=g)).to(DEV)          # (small: the stream is updated in place in every launch)
            calls[name] = (lambda fn=fn, lora=lora, K=K, name=name:
                           N.check(fn(N.ptr(xins[K]), N.ptr(lora), r, 2.0, N.ptr(lam), N.ptr(xs), h16, N.ptr(u), M, K, D, drop, N.stream()), name))
            byts[name] = M * (K * 2 + 2 * D * xs.element_size() + N.LORA_OUT_W * 4)
        ts = alternate(calls)
        print(f" r = {r}, {'fp16' if h16 else 'f32'} stream")
        rates = {k: report(k, v, byts[k]) for k, v in ts.items()}
        a, b = rates.values()
        print(f"  wide / narrow, bytes per second: {b / a:.2f}")
