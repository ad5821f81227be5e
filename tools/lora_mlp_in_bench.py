#!/usr/bin/env python3
"""LoRA on DINOv3's MLP input (ViTLoRAEngine(allow_mlp_in=True)): what the gate_proj / up_proj pair costs, measured interleaved in ONE process.

    lora_mlp_in_bench.py [B [windows [steps per window]]]          (defaults 32, 7, 6)

1  The pair gradient kernel alone, ucod_lora_mlp_pair_grad, beside the yardstick ucod_lora_mlp_grad on the same build at the same sizes -- (N1 = 3072, D = 384), the
   dinov3_vits16plus shape, and (8192, 1536), the widest the kernels take -- r = 2, M = 16 images x 1029 tokens, dropout 0 and 0.05.  Both read the same bytes of dpre
   and h2_aug.  Windows of 40 launch pairs (grad + reduce: 1 - 14 ms per window at these sizes), the two kernels in alternating windows, median and min .. max over the windows.
2  forward_train + backward of dinov3_vits16plus at 512 x 512 with q / k / v targeted, and with q / k / v + gate_proj + up_proj, in alternating windows of
   ``steps per window`` steps, lora_dropout 0.05, two streams: median and min .. max over the windows.
"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTLoRAEngine
from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
lib = N.load()
DEV = "cuda"


def timed(fn, n):
    """ms per call of ``fn`` over one window of ``n`` calls (device time between two events)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def report(name, ts, extra=""):
    print(f"  {name:44s} median {statistics.median(ts) * 1e3:9.1f} us   min .. max {min(ts) * 1e3:9.1f} .. {max(ts) * 1e3:9.1f} us{extra}")
    return statistics.median(ts)


print(f"1. the gradient kernels alone (r = 2, M = 16 x 1029 rows; {windows} alternating windows of 40 launch pairs)")
M, r = 16 * 1029, 2
for N1, D in ((3072, 384), (8192, 1536)):
    for p in (0.0, 0.05):
        g = torch.Generator().manual_seed(1)
        dpre = torch.randn(M, N1, generator=g).bfloat16().to(DEV)
        h = torch.randn(M, D + N.LORA_AUG, generator=g).bfloat16().to(DEV)
        t = torch.zeros(M, N.LORA_AUG, dtype=torch.bfloat16, device=DEV)
        drop = C.byref(N.LoraDropout(p, 1234, 14)) if p > 0 else None
        calls = {}
        for name, fn, wsf, na in (("ucod_lora_mlp_grad", lib.ucod_lora_mlp_grad, lib.ucod_lora_mlp_grad_workspace_bytes, 1),
                                  ("ucod_lora_mlp_pair_grad", lib.ucod_lora_mlp_pair_grad, lib.ucod_lora_mlp_pair_grad_workspace_bytes, 2)):
            lora = (0.05 * torch.randn(r * (na * D + N1), generator=g)).to(DEV)
            grad, wsb = torch.zeros_like(lora), wsf(N1, D)
            ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
            calls[name] = (lambda fn=fn, lora=lora, grad=grad, ws=ws, wsb=wsb, name=name:
                           N.check(fn(N.ptr(dpre), N.ptr(h), N.ptr(lora), r, 2.0, N.ptr(grad), N.ptr(t), N.ptr(ws), wsb, M, N1, D, drop, N.stream()), name))
        for fn in calls.values():
            timed(fn, 20)
        ts = {k: [] for k in calls}
        for _ in range(windows):
            for k, fn in calls.items():
                ts[k].append(timed(fn, 40))
        byts = M * (N1 + D + N.LORA_AUG) * 2
        print(f" N1 = {N1}, D = {D}, dropout {p}: {byts / 1e6:.1f} MB read per launch pair")
        meds = {k: report(k, v, f"   {byts / (statistics.median(v) * 1e-3) / 1e12:.2f} TB/s") for k, v in ts.items()}
        print(f"  pair / single = {meds['ucod_lora_mlp_pair_grad'] / meds['ucod_lora_mlp_grad']:.3f}")
        del dpre, h, calls

arch = "dinov3_vits16plus"
heads = ARCHS[arch][1]
print(f"2. {arch} at 512 x 512, B = {B}, lora_dropout 0.05, 2 streams ({windows} alternating windows of {steps} steps)")
sd = random_state_dict(arch, seed=0)
kw = dict(heads=heads, device=DEV, lora_dropout=0.05, allow_swiglu=True, allow_rope=True, eps=1e-5)
engines = {"q,k,v": ViTLoRAEngine(sd, **kw),
           "q,k,v,gate_proj,up_proj": ViTLoRAEngine(sd, target_modules=["q_proj", "k_proj", "v_proj", "gate_proj", "up_proj"], allow_mlp_in=True, **kw)}
x = torch.randn(B, 3, 512, 512, device=DEV)
dkey = torch.randn(B, 64 * heads, 32, 32, device=DEV)


def step(e):
    e.forward_train(x)
    e.backward(dkey)


for e in engines.values():
    e.train_streams = 2
    for _ in range(2):
        step(e)
torch.cuda.synchronize()
ts = {k: [] for k in engines}
for _ in range(windows):
    for k, e in engines.items():
        ts[k].append(timed(lambda e=e: step(e), steps))
meds = {}
for k, v in ts.items():
    meds[k] = statistics.median(v)
    print(f"  {k:28s} forward + backward  median {meds[k]:7.2f} ms   min .. max {min(v):7.2f} .. {max(v):7.2f} ms   ({B / meds[k] * 1e3:.0f} img/s)")
print(f"  the pair adds {meds['q,k,v,gate_proj,up_proj'] - meds['q,k,v']:.2f} ms per step ({(meds['q,k,v,gate_proj,up_proj'] / meds['q,k,v'] - 1) * 100:.1f} %)")
