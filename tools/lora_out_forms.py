#!/usr/bin/env python
"""ucod_lora_out_grad_x in its SwiGLU and GELU forms at equal (rows, K, D), interleaved in one process: time per call (the gradient kernel + its reduce launch, device
events around ``calls`` calls, ``rounds`` rounds of each form in turn) and the bytes each form has to move per second.  Per hidden unit the SwiGLU form reads and
writes twice the GELU form's bytes (pre and dpre are [rows, 2K]); the expectation is the same bytes per second, so twice the time.
    lora_out_forms.py [rows [K [D [r [dropout [rounds [calls]]]]]]]      (default: ViT-g/14 at B = 8, 518 px: 10960 4096 1536 2 0.0 9 20)"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
rows, K, D, r, drop, rounds, calls = arg(1, 10960), arg(2, 4096), arg(3, 1536), arg(4, 2), arg(5, 0.0, float), arg(6, 9), arg(7, 20)
lib = N.load()
wsb = lib.ucod_lora_out_grad_workspace_bytes(r, K, D)
if wsb == 0:
    sys.exit(f"(r, K, D) = {(r, K, D)} is outside the kernels' limits")
g = torch.Generator().manual_seed(0)
dev = "cuda"
flat = torch.cat(((torch.randn(r, K, generator=g) / K ** 0.5).reshape(-1), torch.randn(D * r, generator=g))).to(dev)
t = torch.zeros(rows, N.LORA_OUT_W)
t[:, :r] = torch.randn(rows, r, generator=g)
t = t.to(dev)
grad, ws = torch.empty(r * (K + D), device=dev), torch.empty(wsb, dtype=torch.uint8, device=dev)
dp = C.byref(N.LoraDropout(drop, 1234, 7)) if drop > 0 else None
forms = {}
for name, act, width in (("swiglu", N.LORA_OUT_ACT_SWIGLU, 2 * K), ("gelu", N.LORA_OUT_ACT_GELU, K)):
    x = torch.randn(rows, width, generator=g).bfloat16().to(dev)
    cot0 = torch.randn(rows, width, generator=g).bfloat16().to(dev)
    forms[name] = dict(act=act, x=x, cot0=cot0, cot=cot0.clone(), bytes=3 * rows * width * 2 + rows * 32, ms=[])


def run(f):
    N.check(lib.ucod_lora_out_grad_x_ex(N.ptr(f["x"]), f["act"], N.LORA_OUT_SWIGLU if f["act"] == N.LORA_OUT_ACT_SWIGLU else 0, N.ptr(f["cot"]), N.ptr(t), N.ptr(flat), r, N.ptr(grad), N.ptr(ws), wsb, rows, K, D, dp, N.stream()),
            "ucod_lora_out_grad_x_ex")


for f in forms.values():                                            # warm-up: code objects loaded, clocks up
    for _ in range(5):
        run(f)
torch.cuda.synchronize()
for _ in range(rounds):
    for f in forms.values():
        f["cot"].copy_(f["cot0"])                                   # (the cotangent is updated in place: every round starts from the same values)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            run(f)
        b.record()
        torch.cuda.synchronize()
        f["ms"].append(a.elapsed_time(b) / calls)
print(f"ucod_lora_out_grad_x (+ reduce) at rows {rows}, K {K}, D {D}, r {r}, dropout {drop}: {rounds} rounds of {calls} calls, forms alternating")
for name, f in forms.items():
    med = statistics.median(f["ms"])
    print(f"  {name:6s} {f['bytes'] / 1e6:7.1f} MB per call   median {med * 1e3:7.1f} us  (min {min(f['ms']) * 1e3:.1f}, max {max(f['ms']) * 1e3:.1f})"
          f"  -> {f['bytes'] / (med * 1e-3) / 1e12:.2f} TB/s")
ratio = statistics.median(forms["swiglu"]["ms"]) / statistics.median(forms["gelu"]["ms"])
print(f"  swiglu / gelu: time x{ratio:.2f} for x{forms['swiglu']['bytes'] / forms['gelu']['bytes']:.2f} the bytes")
