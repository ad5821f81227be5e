#!/usr/bin/env python3
"""Backbone-backward (LoRA) mode at the headline size: forward_train + backward of DINOv2 ViT-B/14 @518 (or, sixth argument dinov2_vitg14, of ViT-g/14 with its
SwiGLU MLP; or a DINOv3 name such as dinov3_vitb16, rotary embedding in both passes, @512), per-class kernel times.
    lora_bench.py [B [steps [streams [dropout [resid [arch [targets [side] [bias]]]]]]]]
``targets``: comma list of LoRA target modules (default: the engine's query,key,value / q_proj,k_proj,v_proj), e.g. query,key,value,fc1 or query,key,value,weights_in
on ViT-g, or q_proj,k_proj,v_proj,gate_proj,up_proj on dinov3_vits16plus (a DINOv3 MLP input module switches ``allow_mlp_in`` on, an MLP module of dinov3_vith16plus ``allow_wide_mlp``); naming an output projection (dense, fc2; o_proj, down_proj) switches the engine's ``allow_out`` on, e.g. query,key,value,dense,fc2.  ``side``: the image side in pixels, a multiple of the patch size (default 518; 512 on a DINOv3 arch, patch 16).
``bias``: a trailing none / lora_only / all (peft's LoraConfig.bias; with or without ``side`` in front of it): lora_only also trains the targeted modules' biases -- one
deterministic column sum per bias and layer in the backward (tools/lora_bias_bench.py times the three modes against each other in one process)."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucod_dpl_amd import native as N
from ucod_dpl_amd.vit_engine import LORA_BIAS_MODES, ViTLoRAEngine
from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS, DINOV3_ARCHS, SWIGLU_ARCHS

bias = sys.argv.pop() if sys.argv[-1] in LORA_BIAS_MODES else "none"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
streams = int(sys.argv[3]) if len(sys.argv) > 3 else 2
lib = N.load()
drop = float(sys.argv[4]) if len(sys.argv) > 4 else 0.0   # the reference trains with lora_dropout 0.05 (configs/model/UCOD_DPL.py)
resid = sys.argv[5] if len(sys.argv) > 5 else "auto"      # residual stream of the training pass: auto (fp16 with bf16 operands) / f32
arch = sys.argv[6] if len(sys.argv) > 6 else "dinov2_vitb14"
v3 = arch in DINOV3_ARCHS                                 # DINOv3: rotary embedding in both passes (allow_rope), patch 16, eps 1e-5
if arch not in ("dinov2_vitb14", "dinov2_vitg14", "dinov2_vitb14_reg", "dinov2_vitg14_reg") and not v3:        # (_reg: DINOv2 with registers, 4 register tokens per image)
    sys.exit(f"arch must be dinov2_vitb14 or dinov2_vitg14 (or their _reg forms) or one of {sorted(DINOV3_ARCHS)}, got {arch}")
giant = arch.startswith("dinov2_vitg14")
heads, patch = ARCHS[arch][1], ARCHS[arch][3]
targets = sys.argv[7].split(",") if len(sys.argv) > 7 and sys.argv[7] else None
side = int(sys.argv[8]) if len(sys.argv) > 8 else (512 if v3 else 518)
if side % patch:
    sys.exit(f"the image side must be a multiple of the patch size {patch}, got {side}")
grid, n_lead = side // patch, 1 + (DINOV3_ARCHS[arch] if v3 else 4 if arch.endswith("_reg") else 0)
kw = {} if targets is None else dict(target_modules=targets)
kw.update(bias=bias, allow_bias_all=bias == "all")    # (a trailing all: every bias of the backbone -- sets the opt-in)
if v3:
    kw.update(allow_rope=True, eps=1e-5)
leaves = [t.rsplit(".", 1)[-1] for t in targets or ()]
if any(t in ("dense", "fc2", "o_proj", "down_proj", "weights_out") for t in leaves):
    kw.update(allow_out=True)                             # the output projections are opt-in (ViTLoRAEngine)
if "weights_out" in leaves or ("down_proj" in leaves and arch in SWIGLU_ARCHS):
    kw.update(allow_swiglu_out=True)                      # ... and the SwiGLU MLP's has an opt-in of its own (the hidden is recomputed in the backward)
if v3 and any(t in ("up_proj", "gate_proj") for t in leaves):
    kw.update(allow_mlp_in=True)                          # DINOv3's MLP input modules are opt-in too (on the gated MLP: the gate_proj / up_proj pair kernels)
if arch == "dinov3_vith16plus" and any(t in ("up_proj", "gate_proj", "down_proj") for t in leaves):
    kw.update(allow_wide_mlp=True)                        # hidden 5120: N1 = 10240 rows and K = 5120 columns are the wide row kernels' (UCOD_LORA_WIDE)
eng = ViTLoRAEngine(random_state_dict(arch, seed=0), heads=heads, device="cuda", lora_dropout=drop, resid=resid, allow_swiglu=giant or arch in SWIGLU_ARCHS, **kw)
if targets is not None:
    print(f"targets {targets}, bias {bias}: arena [{eng.L}, {eng.lora.shape[1]}]")
eng.train_streams = streams
x = torch.randn(B, 3, side, side, device="cuda")
dkey = torch.randn(B, 64 * heads, grid, grid, device="cuda")
for _ in range(2):
    eng.forward_train(x); eng.backward(dkey)
torch.cuda.synchronize()
t0 = time.time()
for _ in range(steps):
    eng.forward_train(x)
torch.cuda.synchronize(); t1 = time.time()
for _ in range(steps):
    eng.forward_train(x); eng.backward(dkey)
torch.cuda.synchronize(); t2 = time.time()
fwd = (t1 - t0) / steps * 1e3; both = (t2 - t1) / steps * 1e3
print(f"B={B}: forward_train {fwd:.2f} ms, forward+backward {both:.2f} ms  ({B / both * 1e3:.1f} img/s), workspace {sum(w.numel() for w in eng._tside_ws if w is not None) / 2**30:.2f} GiB in {len(eng._tside)} stream(s)")
eng.train_streams = 1          # exclusive per-kernel durations
eng.forward_train(x); eng.backward(dkey)
torch.cuda.synchronize()
lib.ucod_prof_enable(1)
eng.forward_train(x); eng.backward(dkey)
torch.cuda.synchronize()
lib.ucod_prof_enable(0)
n = lib.ucod_prof_num_classes()
tot = (C.c_double * n)(); cnt = (C.c_longlong * n)()
lib.ucod_prof_collect(tot, cnt)
rows = [(lib.ucod_prof_class_name(i).decode(), cnt[i], tot[i]) for i in range(n) if cnt[i]]
for name, c, t in sorted(rows, key=lambda r: -r[2]):
    print(f"  {name:34s} {c:4d} launches  {t:8.3f} ms total  {t / c * 1e3:8.1f} us avg")
print(f"  sum {sum(r[2] for r in rows):.2f} ms")
if getattr(eng, "mlp_target", None) is not None:
    # the MLP module's gradient kernel against the bytes it has to move: one pass over dpre [M, N1] and one over h2_aug [M, D+64], both bf16 (per two ranks)
    M = B * (n_lead + grid * grid)
    byts = (M * eng.N1 * 2 + M * (eng.D + 64) * 2) * ((eng.r + 1) // 2)
    for name, c, t in rows:
        if name == "lora_mlp_grad":
            print(f"  lora_mlp_grad: {byts / 1e6:.1f} MB per launch pair (grad + reduce), {t / c * 1e3:.1f} us -> {byts / (t / c * 1e-3) / 1e12:.2f} TB/s")
if any(getattr(eng, "out_targets", ())):
    # the output modules' three kernels against the bytes each has to move (per launch; grad_s / grad_x include their reduce launch): the forward reads x_in [M, K]
    # bf16, reads and writes the stream row and writes u; grad_s reads s [M, D] and u, writes t; grad_x reads x_in and reads and writes its cotangent
    M, D, sb = B * (n_lead + grid * grid), eng.D, 2 if eng.resid16 else 4
    Ks = [K for K, on in zip((D, eng.F), eng.out_targets) if on]
    # (the SwiGLU MLP's module: its grad_x has a profiler class of its own and moves twice the bytes per hidden unit -- pre and dpre are [M, 2F])
    sw = bool(getattr(eng, "_out_flags", 0))
    Kx = ([D] if eng.out_targets[0] else []) + ([eng.F] if eng.out_targets[1] and not sw else [])
    per = {"lora_out_fwd": sum(M * K * 2 + 2 * M * D * sb + M * 32 for K in Ks) / len(Ks), "lora_out_grad_s": sum(M * D * 2 + 2 * M * 32 for K in Ks) / len(Ks)}
    if Kx:
        per["lora_out_grad_x"] = sum(3 * M * K * 2 + M * 32 for K in Kx) / len(Kx)
    if sw:
        per["lora_out_grad_x_swiglu"] = 3 * M * 2 * eng.F * 2 + M * 32
    over = {"lora_out_grad_x": Kx, "lora_out_grad_x_swiglu": [eng.F]}
    for name, c, t in rows:
        if name in per:
            byts = per[name]                                # the mean over the modules that class runs for, as the average time is
            print(f"  {name}: {byts / 1e6:.1f} MB per launch (mean of K = {over.get(name, Ks)}), {t / c * 1e3:.1f} us -> {byts / (t / c * 1e-3) / 1e12:.2f} TB/s")
if giant:
    # the two SwiGLU training launches alone at this pass's shapes, and beside them (orientation) the launches they extend: UCOD_EPI_BIAS_SWIGLU_BF16 at (M, 2F, D),
    # which the SAVE form extends by one [M, 2F] store, and UCOD_EPI_GELU_BWD_BF16 at (M, F, D), which reads and writes half the bytes of the SwiGLU dgrad drain
    M, D, F = B * (n_lead + grid * grid), eng.D, eng.F
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()  # noqa: E731
    A, w_in, w_out_t, b_in = rnd(M, D), rnd(2 * F, D) * D ** -0.5, rnd(F, D) * D ** -0.5, torch.randn(2 * F, device="cuda", generator=g)
    pre2, pre1 = rnd(M, 2 * F), rnd(M, F)
    hid, out2, out1 = torch.empty(M, F, dtype=torch.bfloat16, device="cuda"), torch.empty(M, 2 * F, dtype=torch.bfloat16, device="cuda"), torch.empty(M, F, dtype=torch.bfloat16, device="cuda")
    p, st = N.ptr, N.stream
    forms = [
        ("swiglu_save   (M, 2F, D)", lambda: lib.ucod_gemm_bf16_train(N.EPI_BIAS_SWIGLU_SAVE_BF16, p(A), p(w_in), p(hid), M, 2 * F, D, p(b_in), None, p(out2), 0, st()), 2.0 * M * 2 * F * D),
        ("swiglu (infer)(M, 2F, D)", lambda: lib.ucod_gemm_bf16(N.EPI_BIAS_SWIGLU_BF16, p(A), p(w_in), p(hid), M, 2 * F, D, p(b_in), None, None, None, 0, 0, st()), 2.0 * M * 2 * F * D),
        ("swiglu_bwd    (M, F, D) ", lambda: lib.ucod_gemm_bf16_train(N.EPI_SWIGLU_BWD_BF16, p(A), p(w_out_t), p(out2), M, F, D, None, p(pre2), None, 0, st()), 2.0 * M * F * D),
        ("gelu_bwd      (M, F, D) ", lambda: lib.ucod_gemm_bf16_train(N.EPI_GELU_BWD_BF16, p(A), p(w_out_t), p(out1), M, F, D, None, p(pre1), None, 0, st()), 2.0 * M * F * D),
    ]
    print(f"  isolated launches at M = {M}, D = {D}, F = {F} (median of 7 rounds x 10 launches, interleaved):")
    times = {name: [] for name, _, _ in forms}
    for rnd_i in range(8):
        for name, fn, _ in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                N.check(fn(), name)
            e1.record()
            e1.synchronize()
            if rnd_i:                                         # (round 0 warms up)
                times[name].append(e0.elapsed_time(e1) / 10 * 1e3)
    for name, _, flops in forms:
        us = sorted(times[name])[len(times[name]) // 2]
        print(f"    {name} {us:8.1f} us  {flops / us * 1e-6:7.1f} TF/s")
