#!/usr/bin/env python3
"""What the norm table of LoRA bias="all" costs in the backbone backward: (1) one training forward + backward of one image-parallel chunk through the C ABI, in three
forms timed in alternating rounds in one process on one workspace -- _lora_out_ex (bias "none"), _lora_bias (the six Linear biases: "lora_only") and _lora_bias_ex
with the norm table on top (the LayerNorm betas and the patch bias: what "all" adds); (2) ucod_colsum_det_lora and ucod_colsum_det_tok alone at that pass's shapes,
as bytes read over time against the HBM rate.
    lora_bias_all_bench.py [B [rounds [dropout [arch [targets]]]]]
Defaults: 16 images (one of the two chunks of a batch of 32), 7 rounds of 3 passes, dropout 0.05, dinov2_vitb14 @518, query,key,value,fc1,dense,fc2."""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import ViTLoRAEngine
from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
drop = float(sys.argv[3]) if len(sys.argv) > 3 else 0.05
arch = sys.argv[4] if len(sys.argv) > 4 else "dinov2_vitb14"
targets = (sys.argv[5] if len(sys.argv) > 5 else "query,key,value,fc1,dense,fc2").split(",")
STEPS = 3
heads, patch = ARCHS[arch][1], ARCHS[arch][3]
side = 518
grid = side // patch
sd = random_state_dict(arch, seed=0)
eng = ViTLoRAEngine(sd, heads=heads, device="cuda", lora_dropout=drop, target_modules=targets, allow_out=True, allow_swiglu=arch.startswith("dinov2_vitg14"), bias="lora_only")
lib, P, D, L = eng.lib, N.ptr, eng.D, eng.L
x = torch.randn(B, 3, side, side, device="cuda")
dkey = torch.randn(B, D, grid, grid, device="cuda")
key = torch.empty(B, D, grid, grid, device="cuda")
t = eng._train_desc(B, side, side, 12345)
g = torch.zeros_like(eng.lora_grad)
T, TT, TM, keep = eng._tables(grid, grid, g)
TO, TB = eng._out_table(g), eng._bias_table(g)
norm = torch.zeros(1 + 2 * L, D, device="cuda")
TN = (C.c_void_p * (1 + 2 * L))(*[norm[s].data_ptr() for s in range(1 + 2 * L)])
lead = (C.byref(t), eng.mlp, eng._out_flags)
nbytes = lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, TM, TO, TB, TN)
assert nbytes == lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, TM, TO, TB)
ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
st = N.stream()


def step(mode):
    N.check(lib.ucod_vit_forward_train_lora_out_ex(*lead, T, TT, TM, TO, P(x), P(key), P(ws), nbytes, st), "forward")
    if mode == "none":
        N.check(lib.ucod_vit_backward_lora_out_ex(*lead, T, TT, TM, TO, P(dkey), P(ws), nbytes, st), "backward")
    else:
        N.check(lib.ucod_vit_backward_lora_bias_ex(*lead, T, TT, TM, TO, TB, TN if mode == "all" else None, P(dkey), P(ws), nbytes, st), "backward")


MODES = ("none", "lora_only", "all")
for m in MODES:
    for _ in range(2):
        step(m)
torch.cuda.synchronize()
times = {m: [] for m in MODES}
for r in range(rounds):
    for m in (MODES if r % 2 == 0 else MODES[::-1]):                 # alternate the order as well
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            step(m)
        e1.record(); e1.synchronize()
        times[m].append(e0.elapsed_time(e1) / STEPS)
med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
print(f"{arch} B={B} (one chunk, one stream) dropout={drop} targets={targets}: training forward + backward through the C ABI, ms per pass over {rounds} rounds of {STEPS}")
for m, v in times.items():
    print(f"  {m:9s} median {med[m]:.2f}, min {min(v):.2f}, max {max(v):.2f}")
d_lo, d_all = med["lora_only"] - med["none"], med["all"] - med["lora_only"]
print(f"  lora_only - none = {d_lo:+.3f} ms; all - lora_only = {d_all:+.3f} ms ({d_all / max(d_lo, 1e-9):.2f} x what lora_only adds); spread of one mode "
      f"{max(times['none']) - min(times['none']):.3f} ms")
out = {"arch": arch, "B": B, "dropout": drop, "step_ms": med, "step_ms_all": times, "kernel": []}

# the kernels alone at this pass's shapes
M, tok, r = B * (1 + grid * grid), 1 + grid * grid, eng.r
dh = torch.randn(M, D, device="cuda").bfloat16()
dqkv = torch.randn(M, 3 * D + 64, device="cuda").bfloat16()
tm = torch.randn(M, 64, device="cuda").bfloat16()
dx = torch.randn(M, D, device="cuda")
arena = torch.randn(6 * r * D, device="cuda")
o = torch.empty(D, device="cuda")
wsb = lib.ucod_colsum_det_lora_workspace_bytes(M, D)
wk = torch.empty(wsb, dtype=torch.uint8, device="cuda")
dd = N.LoraDropout(drop, 12345, 3)
cases = [
    ("ucod_colsum_det of dh (beta1, dropout off)", M * D * 2, lambda: lib.ucod_colsum_det(P(dh), N.ROPE_ELEM_HALF, M, D, D, None, P(o), P(wk), wsb, st)),
    ("ucod_colsum_det_lora np=3 (beta1, dropout on)", M * D * 2 + M * 3 * r * 2, lambda: lib.ucod_colsum_det_lora(P(dh), 1, M, D, dqkv.data_ptr() + 6 * D, 3 * D + 64, P(arena), 3, r, C.byref(dd), P(o), P(wk), wsb, st)),
    ("ucod_colsum_det_lora np=1 (beta2, MLP adapter)", M * D * 2 + M * r * 2, lambda: lib.ucod_colsum_det_lora(P(dh), 1, M, D, P(tm), 64, P(arena), 1, r, C.byref(dd), P(o), P(wk), wsb, st)),
    ("ucod_colsum_det_tok of dx f32 (patch bias)", (M - B) * D * 4, lambda: lib.ucod_colsum_det_tok(P(dx), N.ROPE_ELEM_F32, B, tok, 1, D, D, None, P(o), P(wk), wsb, st)),
]
for name, byts, run in cases:
    for _ in range(3):
        N.check(run(), name)
    us = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record(); e1.synchronize()
        us.append(e0.elapsed_time(e1) / 20 * 1e3)
    tt = sorted(us)[len(us) // 2]
    byts += 2 * wsb                                           # the partials written and read once
    print(f"  {name:48s} [{M}, {D}]: {tt:7.1f} us per call (two launches), {byts / 1e6:6.1f} MB -> {byts / tt * 1e-6:5.2f} TB/s "
          f"({byts / tt * 1e-6 / 6.3 * 100:4.1f} % of the 6.3 TB/s a streaming copy reaches)")
    out["kernel"].append(dict(name=name, M=M, D=D, us=tt, bytes=byts, TBps=byts / tt * 1e-6))
print(json.dumps(out))
