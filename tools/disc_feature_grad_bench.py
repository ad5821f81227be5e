#!/usr/bin/env python3
"""The gradient into the features of the discriminator's feature branch at the real size (dim 768, fs 68), one process, interleaved runs:
  1. ucod_conv3x3_f32(gy, Wd) (the data gradient of featureConv without an unfold-sized buffer) beside the route it replaces for that block, the W^T GEMM into
     gcols [B, 9 dim, fs^2] followed by ucod_fold3x3, on the same inputs: time (device events), peak memory over the call, TF/s against the 157 TF/s f32-MFMA peak;
  2. the step: TrainLoop._process_batch_full on DINOv2 ViT-B/14 @518 with dis_use_features False and True (host clock around steps that end in a synchronise).
    disc_feature_grad_bench.py [B_step [rounds [steps_per_round]]]     -> profiles/disc_feature_grad_bench.txt (and stdout)
The register / scratch use of the three kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/conv3x3.hip) is appended by hand: it needs no GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ucod_dpl_amd import ops
from ucod_dpl_amd.engine.config import CfgNode
from ucod_dpl_amd.models.discriminator import Discriminator

B_STEP = int(sys.argv[1]) if len(sys.argv) > 1 else 32
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
PEAK_TF = 157.0
DIM, FS = 768, 68
DEV = "cuda"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """-> (ms per call by device events, peak bytes above the level at entry, last result)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, torch.cuda.max_memory_allocated() - base, out


def kernel_part():
    disc = Discriminator(CfgNode(dict(dim=DIM, feature_size=FS, ema_weight=0.99, dis_use_features=True))).to(DEV)
    weight = disc.featureConv.layers[0].weight.detach()
    K = 9 * DIM
    wmat = weight.reshape(DIM, K).contiguous()                      # 9 * 768 is a multiple of 16: no padding
    say(f"# 1. data gradient of featureConv ({DIM} -> {DIM}, 3x3, stride 1) at fs {FS}: ucod_conv3x3_f32(gy, Wd) vs W^T GEMM + ucod_fold3x3")
    for B in (8, 32):
        gy = torch.randn(B, DIM, FS, FS, device=DEV)
        rec = dict(wmat=wmat, geom=(B, DIM, FS, FS, DIM, FS, FS, 1, K, K))
        new = lambda: ops.conv3x3(gy, ops.conv3x3_dgrad_weights(weight))                     # noqa: E731  (the weight re-layout is part of the new route)
        old = lambda: disc._conv_dgrad_fold(rec, gy.view(B, DIM, FS * FS))                   # noqa: E731
        a, b = new(), old()
        err = float((a - b).abs().max()) / float(b.abs().max())
        del a, b
        flop = 2.0 * B * FS * FS * DIM * K
        tn, to, mn, mo = [], [], 0, 0
        for _ in range(ROUNDS):                                      # interleaved: new, old, new, old ...
            t, m, _ = timed(new, 5)
            tn.append(t)
            mn = max(mn, m)
            t, m, _ = timed(old, 5)
            to.append(t)
            mo = max(mo, m)
        say(f"B={B:2d}: conv3x3 {min(tn):8.3f} ms (rounds {', '.join(f'{t:.3f}' for t in tn)}), {flop / min(tn) / 1e9:6.1f} TF/s = {flop / min(tn) / 1e9 / PEAK_TF * 100:4.1f} % of "
            f"{PEAK_TF:.0f}, peak +{mn / 2**20:8.1f} MiB | GEMM+fold {min(to):8.3f} ms (rounds {', '.join(f'{t:.3f}' for t in to)}), {flop / min(to) / 1e9:6.1f} TF/s, "
            f"peak +{mo / 2**20:8.1f} MiB | max |new - old| / |old|max {err:.2e}")
        del gy
    del disc
    torch.cuda.empty_cache()


def build_loop(use_features):
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine
    from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS
    cfg = CfgNode(dict(
        model_cfg=dict(dim=DIM, feature_size=FS, ema_weight=0.99, dis_use_features=use_features),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=2e-4, dis_lr0=1e-3, step_lr_size=25, dis_step_lr_size=25, step_lr_gamma=0.95,
                       dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1, dis_intertrain=2,
                       save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50), log_cfg=dict(log_interval=50, log_path="/tmp/ucod_bench", multi_rank=[0])))
    torch.manual_seed(0)
    runner = StandardRunner(cfg)
    loop = TrainLoop(runner.config, runner)
    arch = "dinov2_vitb14"
    eng = ViTLoRAEngine(random_state_dict(arch, seed=0), heads=ARCHS[arch][1], r=2, lora_alpha=4, device=DEV, generator=torch.Generator().manual_seed(7),
                        lora_dropout=0.05, seed=1234)
    loop.attach_lora_backbone(eng)
    return loop


def step_part():
    say(f"# 2. TrainLoop._process_batch_full, DINOv2 ViT-B/14 @518, batch {B_STEP}, LoRA r=2 on q/k/v: dis_use_features False vs True ({ROUNDS} interleaved rounds of {STEPS} steps)")
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(B_STEP, 3, 518, 518, generator=gen).to(DEV)
    pl = (torch.rand(B_STEP, 1, 2 * FS, 2 * FS, generator=gen) > 0.7).float().to(DEV)
    loops = {False: build_loop(False), True: build_loop(True)}
    times, peaks = {False: [], True: []}, {False: 0, True: 0}
    for uf, loop in loops.items():
        for _ in range(2):                                           # warm-up: code objects, workspaces, the allocator's blocks
            loop._process_batch_full(images, pl)
            loop.global_step += 1
    for _ in range(ROUNDS):
        for uf, loop in loops.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                loss = loop._process_batch_full(images, pl)
                loop.global_step += 1
            torch.cuda.synchronize()
            times[uf].append((time.perf_counter() - t0) / STEPS * 1e3)
            peaks[uf] = max(peaks[uf], torch.cuda.max_memory_allocated() - base)
            assert bool(torch.isfinite(loss)), "the step's loss is not finite"
    for uf in (False, True):
        say(f"dis_use_features={str(uf):5s}: {min(times[uf]):8.2f} ms / step (rounds {', '.join(f'{t:.2f}' for t in times[uf])}), {B_STEP / min(times[uf]) * 1e3:6.1f} img/s, "
            f"peak above the resident state +{peaks[uf] / 2**30:.2f} GiB")
    say(f"the feature branch costs {min(times[True]) - min(times[False]):.2f} ms / step: two featureConv forwards through the unfold route (a [B, 9 dim, fs^2] buffer each, "
        f"{B_STEP * 9 * DIM * FS * FS * 4 / 2**30:.2f} GiB), the two stride-2 blocks both ways, one featureConv backward through ucod_conv3x3_f32")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("disc_feature_grad_bench.py measures on the GPU: none found")
    say(f"disc_feature_grad_bench.py {' '.join(sys.argv[1:])}  ({torch.cuda.get_device_name(0)})")
    kernel_part()
    step_part()
    out = os.path.join(ROOT, "profiles", "disc_feature_grad_bench.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
