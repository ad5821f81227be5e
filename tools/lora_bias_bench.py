#!/usr/bin/env python3
"""What LoRA bias="lora_only" costs: (1) forward_train + backward of the LoRA engine with bias "none", "lora_only" and "all", three engines in one process, timed in alternating
rounds with device events; (2) ucod_colsum_det alone at the buffer shapes of that backward, as bytes read over time against the HBM rate.
    lora_bias_bench.py [B [rounds [streams [dropout [arch [targets]]]]]]
The engines share their side streams (see below: a second pair of streams would not get hardware queues of its own).
Defaults: 32 images, 7 rounds of 3 steps, 2 streams, dropout 0.05, dinov2_vitb14 @518, query,key,value,fc1,dense,fc2."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTLoRAEngine
from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
streams = int(sys.argv[3]) if len(sys.argv) > 3 else 2
drop = float(sys.argv[4]) if len(sys.argv) > 4 else 0.05
arch = sys.argv[5] if len(sys.argv) > 5 else "dinov2_vitb14"
targets = (sys.argv[6] if len(sys.argv) > 6 else "query,key,value,fc1,dense,fc2").split(",")
STEPS = 3
heads, patch = ARCHS[arch][1], ARCHS[arch][3]
side = 518
grid = side // patch
sd = random_state_dict(arch, seed=0)
engines = {}
for bias in ("none", "lora_only", "all"):
    e = ViTLoRAEngine(sd, heads=heads, device="cuda", lora_dropout=drop, target_modules=targets, allow_out=True, allow_swiglu=arch.startswith("dinov2_vitg14"), bias=bias,
                      allow_bias_all=True)
    e.train_streams = streams
    engines[bias] = e
x = torch.randn(B, 3, side, side, device="cuda")
dkey = torch.randn(B, 64 * heads, grid, grid, device="cuda")
for e in engines.values():                                # warm up every shape the timed window uses
    for _ in range(2):
        e.forward_train(x); e.backward(dkey)
torch.cuda.synchronize()
# Both engines on the SAME side streams.  HIP gives a process a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default): with two side streams per engine the engine
# built second shares queues with the first one's, its two image-parallel chunks run one after the other, and it measures 5 ms per step slower whichever mode it
# is -- the first form of this tool reported +6.6 ms for lora_only that way (profiles/lora_bias_bench.txt).  The rounds below are serial, so sharing is safe.
engines["lora_only"]._tside = engines["all"]._tside = engines["none"]._tside
times = {k: [] for k in engines}
for r in range(rounds):
    for k in (("none", "lora_only", "all") if r % 2 == 0 else ("all", "lora_only", "none")):      # alternate the order as well
        e = engines[k]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            e.forward_train(x); e.backward(dkey)
        e1.record(); e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / STEPS)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
eng = engines["lora_only"]
print(f"{arch} B={B} streams={streams} dropout={drop} targets={targets}: arena row {engines['none'].lora.shape[1]} -> {eng.lora.shape[1]} (+{eng.bias_numel} bias values)")
for k, v in times.items():
    print(f"  bias={k:9s} forward_train + backward, ms per step over {rounds} rounds of {STEPS}: median {med[k]:.2f}, min {min(v):.2f}, max {max(v):.2f}")
print(f"  lora_only - none = {med['lora_only'] - med['none']:+.3f} ms ({(med['lora_only'] / med['none'] - 1) * 100:+.2f} %); spread of one mode {max(times['none']) - min(times['none']):.3f} ms")
d_lo, d_all = med["lora_only"] - med["none"], med["all"] - med["none"]
print(f"  all - none = {d_all:+.3f} ms ({(med['all'] / med['none'] - 1) * 100:+.2f} %) = {d_all / max(d_lo, 1e-9):.2f} x what lora_only adds; arena row of all {engines['all'].lora.shape[1]}")
# the kernel alone at the backward's buffer shapes (one chunk of `streams`): a third of dqkv [M, 3D+64], dpre [M, N1], s [M, D], and all of dqkv in one call
lib, D, N1 = N.load(), eng.D, eng.N1
M = (B // streams) * (1 + grid * grid)
shapes = [("a third of dqkv", M, D, 3 * D + 64), ("dpre", M, N1, N1), ("s", M, D, D), ("all three thirds at once", M, 3 * D, 3 * D + 64)]
out = {"arch": arch, "B": B, "streams": streams, "step_ms": med, "step_ms_all": times, "kernel": []}
for name, m, n, ld in shapes:
    buf = torch.randn(m, ld, device="cuda").bfloat16()
    wsb = lib.ucod_colsum_det_workspace_bytes(m, n)
    ws, o = torch.empty(wsb, dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda")
    run = lambda: N.check(lib.ucod_colsum_det(N.ptr(buf), N.ROPE_ELEM_HALF, m, n, ld, None, N.ptr(o), N.ptr(ws), wsb, N.stream()), "ucod_colsum_det")  # noqa: E731
    for _ in range(3):
        run()
    us = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record(); e1.synchronize()
        us.append(e0.elapsed_time(e1) / 20 * 1e3)
    t = sorted(us)[len(us) // 2]
    byts = m * n * 2 + 2 * wsb                             # the columns read once, the partials written and read once
    print(f"  ucod_colsum_det {name:26s} [{m}, {n}] ld {ld}: {t:7.1f} us per call (two launches), {byts / 1e6:6.1f} MB -> {byts / t * 1e-6:5.2f} TB/s "
          f"({byts / t * 1e-6 / 6.3 * 100:4.1f} % of the 6.3 TB/s a streaming copy reaches)")
    out["kernel"].append(dict(name=name, M=m, N=n, ld=ld, us=t, bytes=byts, TBps=byts / t * 1e-6))
print(json.dumps(out))
