#!/usr/bin/env python3
"""Headline benchmark of the UCOD-DPL hot path on MI355X: training images/sec at 3x518x518, DINOv2 ViT-B/14,
batch 32 per GPU (BASELINE.json configs[1]); weak-scaled data parallel for --gpus N (one process per GPU,
launched by torch.distributed.run; the only collective is one RCCL all-reduce of the flat decoder-gradient buffer).

A "step" = one pass of the hot path over one resident synthetic batch:
  frozen backbone forward (bf16 MFMA) -> last-layer key map -> bilinear 37->68 -> DBA student + EMA teacher ->
  Gram orthogonality loss -> APM (2 discriminator calls) -> both BCE losses -> closed-form backward ->
  [all-reduce] -> AdamW + EMA.
Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times --steps steps and prints the
headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...) of that timed region.  `--full` adds everything else
to the line: `roofline` (dominant kernel class, timed live with HIP events on the launch stream in a serial pass), the sustained run, the
discriminator phase, the backbone-backward mode, `cpu_baseline` (the CPU oracle on a bounded sample, with the full-size parity table) and
the other backbone configurations.  `--dump-outputs DIR` writes what the last timed step computed (DIR/<name>.npy).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# HIP runtime knob, set before the runtime initialises: kernel arguments are written straight to device memory instead of being
# fetched from host memory at dispatch.  The step is ~130 launches; measured +1.2 % (2890 -> 2925 images/s, same box, alternating runs).
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0      # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md chip table
DUMP_SAMPLE = 1 << 20               # --dump-outputs: elements kept of a larger output (a fixed, seeded sample)
DUMP_MAX_BYTES = 64 << 20
MFMA_F32_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--arch", default="dinov2_vitb14")
    ap.add_argument("--image", type=int, default=518)
    ap.add_argument("--full-last-layer", action="store_true", help="also run the reference's dead tail of the last layer")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-images", type=int, default=4)
    ap.add_argument("--gemm-variant", type=int, default=0)
    ap.add_argument("--attn-variant", type=int, default=2, choices=[0, 1, 2, 5, 8, 66], help="0 / 2 product kernel, 1 generic-scale kernel, 8 fp8 path (BASELINE configs[4]), 5 / 66 attn_fwd_v5_kernel / attn_fwd_v6_kernel by name")
    ap.add_argument("--resid", default=os.environ.get("UCOD_RESID", "default"), choices=["default", "auto", "f32", "f16"],
                    help="residual-stream type of the backbone (default: fp16 -- with fp16 operands that also folds LayerNorm into QKV / fc1; auto: the "
                         "engine's own choice, fp16 for bf16 operands and f32 for fp16 operands)")
    ap.add_argument("--streams", type=int, default=2, help="image-parallel sub-batches of the backbone pass on independent HIP streams")
    ap.add_argument("--no-pipeline", action="store_true", help="serial order: backbone pass, then decoder step, on one stream")
    ap.add_argument("--half", default="f16", choices=["bf16", "f16", "split2", "split3"],
                    help="arithmetic of the backbone.  f16 (default; the drop-in's default engine since round 6): IEEE fp16 operands on the fp16 residual stream with LayerNorm "
                         "folded into QKV / fc1 -- meets the 1e-3 logit bar on the flat init AND is the fastest; bf16: the operand type BASELINE configs[1] names; split2 / "
                         "split3: the split-operand pass (SplitViTEngine: two / three bf16 terms per f32 operand, f32 residual stream) -- split2 is the fastest configuration "
                         "that meets the bar on trained-like weights, split3 is f32-equivalent (what the feature-cache pass runs); all reported beside the headline")
    ap.add_argument("--sustain-s", type=float, default=40.0,
                    help="--full: after the timed region, keep running the same step for this many seconds in 10-s windows (images/s and held shader clock per window); 0 = skip. "
                         "The reference's hot loop is 126 steps x 25 epochs (engine/runner/loop_UCOD_DPL.py:94-146), the timed region 0.2-0.4 s")
    ap.add_argument("--pmc-traffic", action="store_true",
                    help="measure roofline.traffic in THIS run: two child `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE) of the serial step before the timed run "
                         "(+ ~3 min); default: the committed profiles/r0N_pmc_traffic.json, labelled as such")
    ap.add_argument("--ln-fold", default="auto", choices=["auto", "on", "off"], help="LayerNorm folded into the QKV / fc1 GEMMs (auto: on with fp16 operands on the fp16 stream)")
    ap.add_argument("--look-twice", action="store_true", help="the validation leg of BASELINE configs[3]: first-stage decode + batched Look-Twice second pass "
                    "(fallback centre box on every image); use with --arch dinov2_vitl14 --batch 16")
    ap.add_argument("--lora-resid", default="auto", choices=["auto", "f32", "f16"], help="residual stream of the backbone-backward engine (auto: fp16 with bf16 operands)")
    ap.add_argument("--lora-steps", type=int, default=6, help="steps of the separate backbone-backward (LoRA) measurement; 0 = skip")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the serial pass with per-kernel HIP events (kernels, roofline), the sustained run, the discriminator phase, "
                         "the backbone-backward (LoRA) mode, the CPU baseline with the full-size parity table and the other backbone configurations in their own "
                         "processes (Look-Twice leg: the exclusive per-kernel pass, the first backbone pass alone and its CPU baseline).  Without it a run sets up, "
                         "warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its LAST step as DIR/<name>.npy (float32; an output of more than "
                         f"{DUMP_SAMPLE} elements as a fixed, seeded sample of them): the same arguments give the same inputs in every run")
    a = ap.parse_args()
    if a.pmc_traffic and not a.full:
        ap.error("--pmc-traffic feeds the roofline of a --full run: add --full")
    return a


def make_cfg(fs=68, dim=768):
    from ucod_dpl_amd.engine.config import CfgNode
    cfg = CfgNode(CfgNode.load_with_base(os.path.join(ROOT, "configs", "uscod", "UCOD-DPL_dinov2.py")))
    cfg.model_cfg.dim = dim
    cfg.model_cfg.feature_size = fs
    cfg.log_cfg.log_path = "/tmp/ucod_bench"
    return cfg


def which_config(arch, image, batch, attn_variant=2):
    """Label of the BASELINE.json configuration a command line corresponds to (configs[1] is the one the metric is quoted on)."""
    table = {("dinov2_vitb14", 518, 32): "BASELINE configs[1]", ("dino_vits8", 224, 2): "BASELINE configs[0] geometry (full step instead of decoder only)",
             ("dinov2_vitl14", 518, 16): "BASELINE configs[3] per-GPU geometry (first stage)",
             ("dinov2_vitb14", 518, 64): "BASELINE configs[4] geometry on the bf16 attention path (--attn-variant 8 selects the fp8 path)"}
    label = table.get((arch, image, batch), "non-BASELINE geometry")
    if attn_variant == 8:
        label = ("BASELINE configs[4] (fp8 e4m3 attention path on v_mfma_scale_f32_32x32x64_f8f6f4)" if (arch, image, batch) == ("dinov2_vitb14", 518, 64)
                 else label + " with the fp8 attention path")
    return label


def algorithmic_work(name, B, tok, D, F, heads, Kpad, C_dec, HW):
    """FLOPs (or bytes) per LAUNCH of each op class (DESIGN.md section 'algorithmic work')."""
    M = B * tok
    f = {
        "gemm_bf16_qkv_bias": 2.0 * M * 3 * D * D,
        "gemm_bf16_fc1_gelu": 2.0 * M * F * D,
        "gemm_bf16_proj_fc2_scale_resid": None,            # mixed K (D and F): priced from the per-step total below
        "gemm_bf16_patch_embed": 2.0 * B * (tok - 1) * D * Kpad,
        "gemm_bf16_key_nchw": 2.0 * M * D * D,
        "attention_fwd": 4.0 * B * heads * tok * tok * 64,
        "dba_project_f32": 2.0 * B * (tok - 1) * C_dec * 256,   # on the backbone's native grid (conv and resize commute)
        "dba_wgrad_f32": 2.0 * B * (tok - 1) * C_dec * 128,
    }
    return f.get(name)


def launch_ranks(a):
    """`python bench.py --gpus N` without a torchrun environment: start N ranks (one process per GPU, RCCL over xGMI) as a CHILD
    `python -m torch.distributed.run`, relay its output and exit with its code -- the way the reference's
    scripts/launch_train_first_stage.sh:20-40 starts `accelerate launch --num_processes G`.  Runs before this process touches the
    GPU (device_count() does not initialise HIP), and never replaces a process image."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < a.gpus and os.environ.get("UCOD_SINGLE_DEVICE") != "1":
        raise SystemExit(f"bench.py: --gpus {a.gpus} requested but this node exposes {have} GPU(s)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def pmc_traffic_pass(a):
    """`--pmc-traffic`: HBM-side bytes per launch of every kernel class, measured by THIS run -- two child `rocprofv3 --pmc` passes (FETCH_SIZE, then WRITE_SIZE:
    separate passes, counters only, as MI355X_MICROARCH.md's HBM section prescribes) over the serial form of the same step, each under `timeout`, started before
    this process touches the GPU; tools/pmc_traffic.py applies the guide's corrections (FETCH_SIZE x 2 on gfx950, KiB units).  Returns {class: {...traffic_bytes}}
    or None when a pass fails (the line then says so)."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        print("bench.py: --pmc-traffic needs rocprofv3 on PATH; traffic left to the committed file", file=sys.stderr)
        return None
    tmp = tempfile.mkdtemp(prefix="ucod_pmc_", dir="/tmp")
    args = ["--half", a.half, "--resid", a.resid, "--ln-fold", a.ln_fold, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--lora-steps", "-1", "--no-pipeline",
            "--streams", "1", "--sustain-s", "0", "--batch", str(a.batch), "--arch", a.arch, "--image", str(a.image), "--attn-variant", str(a.attn_variant), "--full"]
    env = dict(os.environ, TMPDIR="/tmp", UCOD_BENCH_CHILD="1")
    for counter, sub in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
        cmd = ["timeout", "900", "rocprofv3", "--pmc", counter, "--output-format", "csv", "-d", os.path.join(tmp, sub), "--", sys.executable, os.path.abspath(__file__)] + args
        r = subprocess.run(cmd, env=env, cwd="/tmp", capture_output=True, text=True)
        if r.returncode != 0:
            print(f"bench.py: the {counter} pass failed or timed out (rc {r.returncode}); traffic left to the committed file\n" + r.stderr[-800:], file=sys.stderr)
            shutil.rmtree(tmp, ignore_errors=True)
            return None
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_traffic.py"), os.path.join(tmp, "fetch"), os.path.join(tmp, "write"), "this run"], capture_output=True, text=True)
    shutil.rmtree(tmp, ignore_errors=True)
    if r.returncode != 0:
        print("bench.py: tools/pmc_traffic.py failed:\n" + r.stderr[-800:], file=sys.stderr)
        return None
    return json.loads(r.stdout).get("kernels") or None


def main():
    a = parse()
    if a.resid == "default":
        a.resid = "auto"                                          # the engine's own choice (round 6: fp16 stream + fold for fp16 operands where the fold exists)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(a)
    measured_traffic = pmc_traffic_pass(a) if (a.full and a.pmc_traffic and a.gpus == 1 and not os.environ.get("UCOD_BENCH_CHILD")) else None   # (before this process touches the GPU)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {a.gpus}: launch with --nproc-per-node equal to --gpus")
    from ucod_dpl_amd import parallel as _par
    pinned_cores = _par.pin_rank_cores(local_rank, world)     # before the first GPU call: each rank on its own slice of the host's cores
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the hot path is HIP-only)")
    from ucod_dpl_amd import parallel
    host_threads = parallel.cap_host_threads(world)           # cores // world intra-op threads per rank (the ranks share one host)
    local_rank = parallel.device_index()                      # = LOCAL_RANK (UCOD_SINGLE_DEVICE=1: test rigs with one GPU)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from ucod_dpl_amd import native
    from ucod_dpl_amd.data.utils.feature_extractor import backbone, ARCHS
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.engine.utils.seed import set_random_seed

    lib = native.load()
    if a.look_twice:
        return look_twice_leg(a, dev, lib, world, rank, host_threads, pinned_cores)
    set_random_seed(42)                                       # engine/utils/seed.py, decoder / discriminator init
    D, heads, L, P, _, _ = ARCHS[a.arch]
    cfg = make_cfg(68, D)
    runner = StandardRunner(cfg)                              # initialises the RCCL process group when WORLD_SIZE > 1
    ranks_seen = parallel.ranks_seen(dev)                     # (a collective: every rank calls it) who took part, on which device
    if world > 1 and len({(r[2], r[3]) for r in ranks_seen}) != world and os.environ.get("UCOD_SINGLE_DEVICE") != "1":
        raise SystemExit(f"bench.py: {world} ranks but the devices seen are {ranks_seen}: ranks share a GPU")
    loop = TrainLoop(cfg, runner)
    split = a.half in ("split2", "split3")
    if split:
        bb = backbone.random_init(a.arch, seed=0, image_size=a.image, device=dev, gemm_variant=a.gemm_variant, precision=a.half)
    else:
        bb = backbone.random_init(a.arch, seed=0, image_size=a.image, device=dev, full_last_layer=a.full_last_layer,
                                  gemm_variant=a.gemm_variant, attn_variant=a.attn_variant, half=a.half, resid=a.resid,
                                  ln_fold={"auto": "auto", "on": True, "off": False}[a.ln_fold])
    ln_fold = bool(bb.engine.ln_fold)
    bb.engine.streams = a.streams
    B = a.batch
    resid16 = bool(bb.engine.resid16)                         # fp16 residual stream (ViTEngine resid="auto": a property of the engine)
    g = torch.Generator().manual_seed(1234 + rank)
    images = torch.randn(B, 3, a.image, a.image, generator=g).to(dev)
    pl = (torch.rand(B, 1, 16, 16, generator=g) > 0.7).float().to(dev)
    gh = a.image // P
    kpad = bb.engine.Kpad
    key = torch.empty(B, D, gh, gh, dtype=torch.float32, device=dev)
    last = {}                                                 # the key map the latest step's decoder step consumed (--dump-outputs)

    def serial_step():
        bb.engine.forward(images, out=key)
        last["key"] = key
        return loop._process_batch((pl, key))

    # Default schedule: the frozen backbone pass of step k+1 runs on side HIP streams (two image-parallel halves) while the
    # main stream runs the decoder step of step k (ucod_dpl_amd/engine/runner/pipeline.py).  Every timed step still enqueues
    # exactly one backbone pass and one decoder step; results are identical to the serial order (final_loss is the same).
    from ucod_dpl_amd.engine.runner import FeaturePipeline
    pipe = FeaturePipeline(bb.engine)

    def pipelined_step():
        k = pipe.next_features()
        pipe.submit(images)
        last["key"] = k
        return loop._process_batch((pl, k))

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    step = serial_step if a.no_pipeline else pipelined_step
    _STEP.update(step=step, loop=loop)                        # (the sustained run below drives the same closure)
    if not a.no_pipeline:
        pipe.submit(images)
    for _ in range(a.warmup):
        step()
        loop.global_step += 1
    barrier()
    t0 = time.perf_counter()
    host_enqueue = 0.0                                        # host time inside the step calls = first to last launch of a step (nothing in them syncs)
    for _ in range(a.steps):
        h0 = time.perf_counter()
        loss = step()
        host_enqueue += time.perf_counter() - h0
        loop.global_step += 1
    barrier()
    dt = time.perf_counter() - t0
    final_loss = float(loss.item())
    bb.engine.check_overflow(wait=True)                       # a saturated fp16 residual stream is an error of the run, never a green line
    if world > 1:
        tdt = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
        dt = tdt.item()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, train_step_outputs(loop, last["key"]))
    if not a.full:
        if rank == 0:
            _flush_c_stdio()
            print(json.dumps(plain_line(a, dict(world=world, B=B, image=a.image, resid16=resid16, ln_fold=ln_fold, dt=dt, final_loss=final_loss,
                                                host_enqueue=host_enqueue, host_threads=host_threads, pinned_cores=pinned_cores, ranks_seen=ranks_seen,
                                                collectives=collectives_label(world, parallel)))), flush=True)
        return

    # Roofline pass: the SAME step in serial order on one stream, so that every launch has the chip to itself and the
    # HIP-event duration of a kernel class is its exclusive duration (with overlapping streams it is not).
    bb.engine.streams = 1
    for _ in range(2):
        serial_step()
        loop.global_step += 1
    barrier()
    t1 = time.perf_counter()                                  # (a) serial order without per-launch events: the plain serial step time
    for _ in range(a.steps):
        serial_step()
        loop.global_step += 1
    barrier()
    dt_serial_plain = time.perf_counter() - t1
    libs = [lib] + ([bb.engine.lib] if bb.engine.lib is not lib else [])     # (the fp16 build is a second library with its own event log)
    for l_ in libs:
        l_.ucod_prof_enable(1)
    t1 = time.perf_counter()
    for _ in range(a.steps):
        serial_step()
        loop.global_step += 1
    barrier()
    dt_serial = time.perf_counter() - t1
    bb.engine.streams = a.streams
    ncls = lib.ucod_prof_num_classes()
    tot = (C.c_double * ncls)()
    cnt = (C.c_longlong * ncls)()
    for l_ in libs:
        l_.ucod_prof_enable(0)
        t_, c_ = (C.c_double * ncls)(), (C.c_longlong * ncls)()
        l_.ucod_prof_collect(t_, c_)
        for i in range(ncls):
            tot[i] += t_[i]
            cnt[i] += c_[i]
    # Sustained run: the same step, back to back, for --sustain-s seconds in ~10-s windows; with several ranks they agree every 16 steps on the
    # slowest rank's clock, so that all leave a window after the same number of steps (the all-reduces stay matched); the host keeps at most 16 steps in flight.
    sustained = None
    if a.sustain_s > 0:
        sustained = sustain(a, lib, dev, world, B, dt / a.steps, barrier)
        bb.engine.check_overflow(wait=True)
    # Discriminator phase (row A8, loop_UCOD_DPL.py:230-255), timed separately as SURVEY.md 8d asks: it runs one epoch in every
    # `dis_intertrain` epochs on the cached features (no backbone pass), so its unit is feature batches, not images through the ViT.
    for _ in range(3):
        loop._discriminator_batch((pl, key))
    barrier()
    t2 = time.perf_counter()
    for _ in range(a.steps):
        dl = loop._discriminator_batch((pl, key))
    barrier()
    dt_dis = time.perf_counter() - t2
    if world > 1:
        tdt = torch.tensor([dt_dis], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
        dt_dis = tdt.item()
    dis_phase = {"value": round(world * B * a.steps / dt_dis, 1), "unit": "feature maps/s", "ms_per_step": round(dt_dis / a.steps * 1e3, 3),
                 "loss": round(float(dl.item()), 6),
                 "what": "discriminator step on resident key maps: student decoder fwd (no grad), 2 discriminator fwd + bwd, all-reduce, fused AdamW"}

    # The same step with IEEE fp16 GEMM / attention operands (ViTEngine(half="f16"): the reference's own autocast type, 8x finer rounding
    # than bf16 -- the build that meets the 1e-3 logit bar, see cpu_baseline.parity_full_size.f16_operands), same schedule, reported
    # SEPARATELY (never part of `value`).  Measured by a CHILD process running this script with --half f16 once this process has
    # finished its own GPU work (a second engine in the same process measures 10 % low: it inherits the allocator and clock state of
    # everything that ran before it); N = 1 only.
    del bb, pipe
    torch.cuda.empty_cache()
    run_children = a.lora_steps >= 0 and world == 1 and not os.environ.get("UCOD_BENCH_CHILD")
    # Optional mode of SURVEY.md 8a row B9, reported SEPARATELY (never part of `value`): images -> LoRA backbone (student,
    # activations saved) + EMA backbone (teacher) -> the same decoder/APM/discriminator step -> backbone backward -> all-reduce
    # of decoder and LoRA gradients -> both fused optimisers.
    lora_mode = None
    if a.lora_steps > 0:
        from ucod_dpl_amd.vit_engine import ViTLoRAEngine
        from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict
        eng = ViTLoRAEngine(random_state_dict(a.arch, 0, a.image), heads, r=2, lora_alpha=4, device=dev, gemm_variant=a.gemm_variant,
                            generator=torch.Generator().manual_seed(7), lora_dropout=0.05, seed=1234 + rank, resid=a.lora_resid)
        loop.attach_lora_backbone(eng)
        for _ in range(2):
            loop._process_batch_full(images, pl)
            loop.global_step += 1
        barrier()
        t0 = time.perf_counter()                              # (no per-launch events in the timed region: the exclusive durations come from the serial pass below)
        for _ in range(a.lora_steps):
            l2 = loop._process_batch_full(images, pl)
            loop.global_step += 1
        barrier()
        dt2 = time.perf_counter() - t0
        if world > 1:
            tdt = torch.tensor([dt2], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
            dt2 = tdt.item()
        # per-class EXCLUSIVE durations: the same step in serial order (one stream for student, teacher and both chunks), so that no two
        # launches overlap and an event pair brackets one kernel alone; never part of `value`
        eng.train_streams, loop.lora_engine_ema.train_streams, loop.serial_schedule = 1, 1, True
        loop._process_batch_full(images, pl)
        loop.global_step += 1
        barrier()
        lib.ucod_prof_enable(1)
        t0 = time.perf_counter()
        for _ in range(2):
            loop._process_batch_full(images, pl)
            loop.global_step += 1
        barrier()
        dt2s = (time.perf_counter() - t0) / 2
        lib.ucod_prof_enable(0)
        tot3, cnt3 = (C.c_double * ncls)(), (C.c_longlong * ncls)()
        lib.ucod_prof_collect(tot3, cnt3)
        loop.serial_schedule = False
        top = sorted(((lib.ucod_prof_class_name(i).decode(), tot3[i] / 2) for i in range(ncls) if cnt3[i]), key=lambda r: -r[1])[:8]
        lora_mode = {"value": round(world * B * a.lora_steps / dt2, 2), "unit": "images/s", "ms_per_step": round(dt2 / a.lora_steps * 1e3, 3),
                     "steps": a.lora_steps, "final_loss": round(float(l2.item()), 6),
                     "what": "LoRA r=2, alpha=4, dropout 0.05 on q/k/v of all layers: student fwd (saved activations) + EMA-teacher fwd + decoder step + backbone "
                             "backward (dgrad only) + LoRA/decoder all-reduce + 2 fused AdamW/EMA",
                     "serial_ms_per_step": round(dt2s * 1e3, 3),
                     "top_kernels_exclusive_ms_per_step": {n: round(t, 3) for n, t in top},
                     "top_kernels_measured_in": "separate serial single-stream pass of the same step (exclusive launch durations, HIP events)"}
    if rank != 0:
        return
    classes = [(lib.ucod_prof_class_name(i).decode(), tot[i], cnt[i]) for i in range(ncls) if cnt[i]]

    cpu = None
    if not a.no_cpu_baseline and world == 1:                  # rank 0 at N = 1 only (the contract); the N > 1 lines carry null
        cpu = cpu_baseline(a, D, heads, L, P)

    # The backbone configurations, each measured in its OWN process (a second engine in this process measures ~10 % low: it inherits the allocator and
    # clock state of everything that ran before it): this process's is the headline, the others are reported beside it, never part of `value`.
    others = {}
    if run_children:
        import subprocess
        torch.cuda.synchronize()
        for name, (half, resid) in CONFIGS.items():
            if name == config_name(a.half, resid16):
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--half", half, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--batch", str(B), "--arch", a.arch, "--image", str(a.image), "--streams", str(a.streams), "--attn-variant", str(a.attn_variant),
                   "--lora-steps", "-1", "--no-cpu-baseline", "--ln-fold", a.ln_fold, "--sustain-s", "0", "--full"] + (["--resid", resid] if resid else []) + \
                  (["--no-pipeline"] if a.no_pipeline else []) + (["--full-last-layer"] if a.full_last_layer and resid else [])
            if half in ("split2", "split3"):                     # 3x / 6x the matrix work: a quarter of the steps keeps the whole run inside minutes
                cmd[cmd.index("--steps") + 1], cmd[cmd.index("--warmup") + 1] = str(max(3, a.steps // 4)), str(max(1, a.warmup // 4))
            r = subprocess.run(cmd, env=dict(os.environ, UCOD_BENCH_CHILD="1"), capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench.py: the child run of configuration {name} failed:\n" + r.stderr[-2000:])
            c = json.loads(line[-1])
            others[name] = {"value": c["value"], "unit": "images/s", "ms_per_step": c["ms_per_step"], "steps": c["steps"], "dtype": half, "residual_stream": c["config"]["residual_stream"],
                            "ln_fold": c["config"].get("ln_fold"), "serial_ms_per_step": c["roofline"]["serial_ms_per_step_without_events"],
                            "kernels_avg_us": {k: v["avg_us"] for k, v in c["kernels"].items()}, "roofline": {k: c["roofline"].get(k) for k in ("kernel", "achieved", "frac", "mfma_issued_tflops", "mfma_issued_frac")},
                            "how": f"python bench.py --half {half}" + (f" --resid {resid}" if resid else "") + " (own process, same schedule, same box)"}

    traffic, traffic_source = None, None
    if measured_traffic is not None:
        traffic, traffic_source = measured_traffic, "measured by this run: two child rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) of the serial step, corrected as MI355X_MICROARCH.md prescribes (tools/pmc_traffic.py)"
    else:
        tpath = next((t for t in (os.path.join(ROOT, "profiles", f"r0{r}_pmc_traffic.json") for r in (6, 5, 4, 3)) if os.path.exists(t)), "")
        if tpath and a.arch == "dinov2_vitb14" and B == 32 and a.image == 518 and not split:
            traffic, traffic_source = json.load(open(tpath)).get("kernels", {}), f"committed file {os.path.relpath(tpath, ROOT)} (a --pmc pass of an earlier run of this configuration; `--pmc-traffic` measures it in the run)"
    meas = dict(world=world, B=B, D=D, heads=heads, L=L, P=P, kpad=kpad, image=a.image, resid16=resid16, ln_fold=ln_fold, dt=dt, dt_serial=dt_serial, dt_serial_plain=dt_serial_plain,
                classes=classes, final_loss=final_loss, dis_phase=dis_phase, lora_mode=lora_mode, host_enqueue=host_enqueue, host_threads=host_threads,
                pinned_cores=pinned_cores, ranks_seen=ranks_seen, cpu=cpu, others=others, traffic=traffic, traffic_source=traffic_source, sustained=sustained,
                collectives=collectives_label(world, parallel))
    _flush_c_stdio()
    print(json.dumps(build_line(a, meas)), flush=True)


def collectives_label(world, parallel):
    if world == 1 and parallel.collectives_on():
        return "RCCL world-size-1 process group FORCED (UCOD_FORCE_DIST=1): broadcast at construction and every all-reduce of the step are issued on the group's stream"
    return "one asynchronous RCCL all-reduce of the flat gradient arena per step" if world > 1 else "none (world size 1: short-circuit)"


def train_step_outputs(loop, key):
    """What a caller of the timed training step holds after its last step: the loss it returned, the step's other results (TrainLoop.last: mask logits of
    student and teacher, APM weights and merged pseudo label, discriminator probabilities and loss, orthogonality term), the key map the step consumed
    and the decoder / EMA-teacher parameters the optimiser left behind."""
    out = {name: t for name, t in loop.last.items()}
    out["key"] = key
    out["decoder_params"] = loop.runner.arena.p
    out["decoder_ema_params"] = loop.runner.arena.ema
    return out


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float32 (float64 stays float64).  An output of more than DUMP_SAMPLE elements is written as
    <name>_sample.npy: its flattened elements at DUMP_SAMPLE sorted positions drawn by a generator of fixed seed (the same positions in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        if t is None:
            continue
        t = torch.as_tensor(t).detach()
        t = t.cpu().to(torch.float64 if t.dtype == torch.float64 else torch.float32)
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            t, name = t.reshape(-1)[idx], name + "_sample"
        arr = t.numpy()
        total += arr.nbytes
        if total > DUMP_MAX_BYTES:
            raise SystemExit(f"bench.py --dump-outputs: more than {DUMP_MAX_BYTES >> 20} MB of outputs")
        np.save(os.path.join(path, name + ".npy"), arr)


def _flush_c_stdio():
    """RCCL prints its version banner through C stdio when the communicator comes up; with stdout redirected that text sits in libc's buffer until exit and would
    land BEHIND the JSON line.  Push it out first: the line is the last thing this process writes to stdout."""
    sys.stdout.flush()
    try:
        C.CDLL(None).fflush(None)
    except Exception:                                           # noqa: BLE001
        pass


MAX_CLOCK_MHZ = 2400.0                                        # MI355X_MICROARCH.md chip table: the clock the 2.5 PFLOP/s dense bf16 / fp16 peak is quoted at
# name -> (--half, --resid or None): the configurations reported in `configurations`
CONFIGS = {"f16_f16_stream": ("f16", "f16"), "f16_f32_stream": ("f16", "f32"), "bf16": ("bf16", "auto"), "split2": ("split2", None), "split3": ("split3", None)}


def config_name(half, resid16):
    return half if half in ("bf16", "split2", "split3") else ("f16_f16_stream" if resid16 else "f16_f32_stream")


def sustain(a, lib, dev, world, B, sec_per_step, barrier):
    """Run the module-level step (set by main) for ~a.sustain_s seconds in windows of ~10 s (time-bounded: a window ends at the first multiple of 16 steps past its length).  Per window: images/s over the wall clock between two
    barrier + synchronize points, and the shader clock the chip HELD = delta s_memtime / delta s_memrealtime x 100 MHz between two single-wave probe launches
    on the step's stream (MI355X_MICROARCH.md, in-kernel clock recipe; ucod_clock_probe)."""
    step, loop = _STEP["step"], _STEP["loop"]
    n_win = max(1, int(round(a.sustain_s / 10.0)))
    win_s = a.sustain_s / n_win
    probes = torch.zeros(n_win, 2, 2, dtype=torch.int64, device=dev)
    windows, ring = [], []
    CHUNK = 16                                                    # steps between two looks at the clock (and, with several ranks, two agreements on it)
    for w in range(n_win):
        barrier()
        lib.ucod_clock_probe(probes[w, 0].data_ptr(), torch.cuda.current_stream().cuda_stream)
        t0 = time.perf_counter()
        n = 0
        while True:
            for i in range(CHUNK):
                step()
                loop.global_step += 1
                if i % 8 == 7:                                    # bound the host's lead: at most 16 steps enqueued ahead of the device
                    ev = torch.cuda.Event()
                    ev.record()
                    ring.append(ev)
                    if len(ring) > 2:
                        ring.pop(0).synchronize()
            n += CHUNK
            elapsed = time.perf_counter() - t0
            if world > 1:                                         # every rank must leave the window after the SAME number of steps (the all-reduces stay matched):
                te = torch.tensor([elapsed], dtype=torch.float64, device=dev)   # they agree on the slowest rank's clock
                torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
                elapsed = te.item()
            if elapsed >= win_s:
                break
        lib.ucod_clock_probe(probes[w, 1].data_ptr(), torch.cuda.current_stream().cuda_stream)
        barrier()
        t1 = time.perf_counter()
        ring.clear()
        windows.append([n, t1 - t0])
    pr = probes.cpu()
    if world > 1:                                                 # max over ranks of every window's wall time
        tw = torch.tensor([w_[1] for w_ in windows], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tw, op=torch.distributed.ReduceOp.MAX)
        for w_, t_ in zip(windows, tw.tolist()):
            w_[1] = t_
    out = []
    for w, (n, t) in enumerate(windows):
        dcyc, dref = int(pr[w, 1, 0] - pr[w, 0, 0]), int(pr[w, 1, 1] - pr[w, 0, 1])
        out.append({"steps": n, "seconds": round(t, 3), "images_per_s": round(world * B * n / t, 2), "held_clock_mhz": round(dcyc / max(dref, 1) * 100.0, 1)})
    return {"seconds": round(sum(w_["seconds"] for w_ in out), 2), "windows": out, "value_sustained": out[-1]["images_per_s"],
            "held_clock_mhz": round(sum(w_["held_clock_mhz"] for w_ in out) / len(out), 1),
            "what": "the timed region's step, back to back; per ~10-s window: images/s between two barrier + synchronize points and the mean shader clock between two "
                    "s_memtime / s_memrealtime probes on the step's stream; value_sustained = the LAST window"}


_STEP = {}


METRIC = "training images/sec at 3x518x518, DINOv2-B (frozen backbone fwd + DBA/APM/discriminator train step)"


def _dtype(a):
    return {"split2": "bf16x2", "split3": "bf16x3"}.get(a.half, a.half)


def _config(a, m):
    """The line's `config` block (both forms of the line)."""
    world, B, resid16, split = m["world"], m["B"], m["resid16"], a.half in ("split2", "split3")
    arith = {"bf16": "bf16 MFMA", "f16": "fp16 MFMA", "split2": "two-term split bf16 MFMA (16 significand bits per operand), f32 residual stream",
             "split3": "three-term split bf16 MFMA (f32-equivalent), f32 residual stream"}[a.half]
    return {"workload": f"{which_config(a.arch, m['image'], B, a.attn_variant)}: {a.arch} @{m['image']}x{m['image']}, batch {B}/GPU, full APM+DBA+discriminator step, "
                        f"decoder path f32 (1x1 conv as a three-way bf16 split on the matrix pipe: f32-equivalent), backbone {arith}", "global_batch": B * world, "parallelism": f"dp{world}",
            "backbone_last_layer": "full (as reference)" if a.full_last_layer else "key-minimal (identical key output; 279.6 of 303.1 GFLOP/img)",
            "random_init_weights": True, "residual_stream": "fp16" if resid16 else "f32", "ln_fold": m["ln_fold"],
            "schedule": "serial, one stream" if a.no_pipeline else
                        f"backbone pass of step k+1 on {1 if split else a.streams} side stream(s) overlapped with the decoder step of step k"}


def plain_line(a, m):
    """The line of a run without --full: the headline of the timed region alone.  `metric`, `value`, `unit`, `higher_is_better`, `dtype` and `ms_per_step`
    are what build_line reports for the same timed region (value = the timed region: a plain run has no sustained run)."""
    world, B, dt = m["world"], m["B"], m["dt"]
    ips = world * B * a.steps / dt
    return {"metric": METRIC, "value": round(ips, 2), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": _dtype(a), "data": "synthetic",
            "value_is": "the timed region", "value_timed_region": round(ips, 2), "full": False, "final_loss": round(m["final_loss"], 6),
            "host_enqueue_ms_per_step": round(m["host_enqueue"] / a.steps * 1e3, 3), "host_threads": m["host_threads"], "host_cores_pinned": m["pinned_cores"],
            "ranks_seen": m["ranks_seen"], "collectives": m.get("collectives"), "config": _config(a, m)}


def build_line(a, m):
    """The ONE JSON line of the contract from the run's measurements `m` (a plain dict: wall times, per-class HIP-event totals, the child runs' lines, the CPU leg).
    Pure host arithmetic -- tests/test_bench_line.py calls it on canned measurements on CPU."""
    world, B, D, heads, L, P, kpad = m["world"], m["B"], m["D"], m["heads"], m["L"], m["P"], m["kpad"]
    resid16, ln_fold, dt, dt_serial, dt_serial_plain = m["resid16"], m["ln_fold"], m["dt"], m["dt_serial"], m["dt_serial_plain"]
    cpu, others, sustained = m["cpu"], m["others"], m["sustained"]
    split = a.half in ("split2", "split3")
    nprod = {"split2": 3, "split3": 6}.get(a.half, 1)
    gh = m["image"] // P
    tok = gh * gh + 1
    F = 4 * D
    HW = 68 * 68
    n_layers = L if a.full_last_layer else L - 1
    kernels = {}
    for name, total_ms, count in m["classes"]:
        avg_us = total_ms / count * 1e3
        k = {"launches_per_step": count / a.steps, "avg_us": round(avg_us, 2), "ms_per_step": round(total_ms / a.steps, 4)}
        fl = algorithmic_work(name, B, tok, D, F, heads, kpad, D, HW)
        per_step = None
        if name == "gemm_bf16_proj_fc2_scale_resid":
            per_step = n_layers * (2.0 * B * tok * D * D + 2.0 * B * tok * D * F)
        elif name == "gemm_bf16_bias_f32" and split:          # the split pass runs QKV and fc1 through UCOD_EPI_BIAS_F32: priced from the per-step total
            per_step = n_layers * (2.0 * B * tok * 3 * D * D + 2.0 * B * tok * F * D)
        elif name == "attention_split_fwd":
            fl = 4.0 * B * heads * tok * tok * 64
        if per_step is not None:
            k["tflops"] = round(per_step / (total_ms / a.steps * 1e-3) / 1e12, 1)
        elif fl:
            k["tflops"] = round(fl / (avg_us * 1e-6) / 1e12, 1)
        if split and "tflops" in k and name.startswith(("gemm_bf16", "attention_split")):
            k["mfma_issued_tflops"] = round(k["tflops"] * nprod, 1)   # the partial products the matrix pipe actually multiplies (3 / 6 per algorithmic product)
        kernels[name] = k
    # HBM-bound representative: LayerNorm.  ALGORITHMIC bytes per SURVEY.md 8(d) / BASELINE.md section 3 = rows*D*(2 B read + 2 B write);
    # with the fp16 residual stream (default on large passes) that is also what the launch moves; with the f32 stream it moves
    # rows*D*(4 + 2) B (PMC: 202 MB) -- reported beside it as `moved_gbs`
    ln_moved = 4 if resid16 else 6
    if "layernorm" in kernels:
        kernels["layernorm"]["gbs"] = round(B * tok * D * 4 / (kernels["layernorm"]["avg_us"] * 1e-6) / 1e9, 1)
        kernels["layernorm"]["moved_gbs"] = round(B * tok * D * ln_moved / (kernels["layernorm"]["avg_us"] * 1e-6) / 1e9, 1)
    if "row_stats" in kernels:                              # LayerNorm-folded passes: the statistics launch reads the fp16 rows once (2 B / element) and writes 8 B per row
        kernels["row_stats"]["gbs"] = round(B * tok * (D * 2 + 8) / (kernels["row_stats"]["avg_us"] * 1e-6) / 1e9, 1)
    if "layernorm_split" in kernels:                        # f32 row in (4 B), nprod bf16 segments out
        kernels["layernorm_split"]["gbs"] = round(B * tok * D * (4 + 2 * nprod) / (kernels["layernorm_split"]["avg_us"] * 1e-6) / 1e9, 1)
    dom = max((n for n in kernels if "tflops" in kernels[n] and n.startswith(("gemm_bf16", "attention"))),
              key=lambda n: kernels[n]["ms_per_step"])
    traffic = m["traffic"]
    if isinstance(traffic, dict):
        traffic = (traffic.get(dom) or {}).get("traffic_bytes")
    serial_ms = dt_serial / a.steps * 1e3
    roofline = {"kernel": dom, "bound": "mfma", "achieved": kernels[dom]["tflops"], "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(kernels[dom]["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": m["traffic_source"] if traffic is not None else None,
                "avg_launch_us": kernels[dom]["avg_us"], "share_of_step": round(kernels[dom]["ms_per_step"] / serial_ms, 3),
                "measured_in": "separate serial single-stream pass of the same step (exclusive launch durations)",
                "serial_ms_per_step": round(serial_ms, 3),
                "serial_ms_per_step_without_events": round(dt_serial_plain / a.steps * 1e3, 3)}
    if split:
        roofline["flops"] = f"algorithmic (one product per f32 multiply); the matrix pipe issues {nprod} bf16 partial products per algorithmic one"
        roofline["mfma_issued_tflops"] = kernels[dom]["mfma_issued_tflops"]
        roofline["mfma_issued_frac"] = round(kernels[dom]["mfma_issued_tflops"] / MFMA_BF16_PEAK_TFLOPS, 4)
    if sustained:                                           # the roofline against what the chip can do at the clock it HOLDS under this load
        held = sustained["held_clock_mhz"]
        roofline["held_clock_mhz"] = held
        roofline["peak_at_held_clock"] = round(MFMA_BF16_PEAK_TFLOPS * held / MAX_CLOCK_MHZ, 1)
        roofline["frac_at_held_clock"] = round(kernels[dom]["tflops"] / (MFMA_BF16_PEAK_TFLOPS * held / MAX_CLOCK_MHZ), 4) if held > 0 else None
        roofline["held_clock_measured_in"] = "the sustained pipelined run (s_memtime / s_memrealtime probes around each ~10-s window); the kernel durations come from the serial pass"
    # the attention kernel's own row: on the fp8 path (BASELINE configs[4]) it is priced against the fp8 matrix peak (block-scaled
    # v_mfma_scale_f32_32x32x64_f8f6f4: 5 PFLOP/s dense), not the bf16 one
    att = next((n for n in kernels if n.startswith("attention") and "tflops" in kernels[n]), None)
    if att is not None:
        peak_att = 5000.0 if a.attn_variant == 8 else MFMA_BF16_PEAK_TFLOPS
        roofline["attention_row"] = {"kernel": att, "achieved": kernels[att]["tflops"], "peak": peak_att, "unit": "TFLOP/s",
                                     "frac": round(kernels[att]["tflops"] / peak_att, 4), "avg_launch_us": kernels[att]["avg_us"],
                                     "peak_is": "fp8 dense (block-scaled MFMA)" if a.attn_variant == 8 else "bf16 / fp16 dense",
                                     "flops": "algorithmic: 4 * B * heads * N^2 * 64 (Q K^T + P V)"}
    hb = "layernorm" if "layernorm" in kernels else ("layernorm_split" if "layernorm_split" in kernels else None)
    if hb == "layernorm":
        roofline["layernorm_launches_per_step"] = kernels["layernorm"]["launches_per_step"]     # 23 unfolded; 1 with LayerNorm folded into QKV / fc1 (the last layer's LayerNorm 1)
        roofline["hbm_row"] = {"kernel": "layernorm", "achieved": kernels["layernorm"]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(kernels["layernorm"]["gbs"] / HBM_PEAK_GBS, 4),
                               "bytes": "algorithmic (SURVEY 8d): bf16 read + bf16 write = 4 B/element",
                               "moved": {"achieved": kernels["layernorm"]["moved_gbs"], "frac": round(kernels["layernorm"]["moved_gbs"] / HBM_PEAK_GBS, 4),
                                         "bytes": "fp16 residual read + 16-bit write = 4 B/element: the launch moves exactly the algorithmic bytes (PMC 135 MB)" if resid16
                                         else "f32 residual read + bf16 write = 6 B/element (what the launch moves; PMC 202 MB)"}}
    elif hb == "layernorm_split":
        roofline["hbm_row"] = {"kernel": "layernorm_split", "achieved": kernels[hb]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(kernels[hb]["gbs"] / HBM_PEAK_GBS, 4),
                               "bytes": f"what the launch moves: f32 row in (4 B/element) + {nprod} bf16 segments out ({2 * nprod} B/element)"}

    PARITY_KEY = {"f16_f16_stream": "f16_operands_f16_stream" if (ln_fold or a.half != "f16") else "f16_operands_f16_stream_unfolded", "f16_f32_stream": "f16_operands", "bf16": "bf16",
                  "split2": "split2", "split3": "split3"}
    mine = config_name(a.half, resid16)

    # North-star parity bar (mask logits within 1e-3 of the f32 reference), at the top level of the line for THIS line's configuration, and for every
    # configuration in `configurations` with its own throughput.
    BAR = 1e-3
    par = (cpu or {}).get("parity_full_size") or {}
    tl = par.get("trained_like_weights") or {}
    own = par.get(PARITY_KEY[mine]) or {}
    logit_max_abs = own.get("logit_max_abs")
    own_tl = tl.get(PARITY_KEY[mine]) or {}
    ips = world * B * a.steps / dt
    ENGINE = {"f16_f16_stream": "ViTEngine() [the default: half='f16', resid='auto' -> fp16 stream]", "f16_f32_stream": "ViTEngine(half='f16', resid='f32')",
              "bf16": "ViTEngine(half='bf16')", "split2": "SplitViTEngine(terms=2)", "split3": "SplitViTEngine(terms=3) [backbone.with_precision('f32eq'): the feature-cache pass]"}

    def describe(name, value, ms, extra):
        pf, tlw = par.get(PARITY_KEY[name]) or {}, tl.get(PARITY_KEY[name]) or {}
        d_ = {"value": value, "unit": "images/s", "ms_per_step": ms, "dtype": CONFIGS[name][0],
              "engine": ENGINE[name] + (" with LayerNorm folded into the QKV / fc1 GEMMs" if extra.get("ln_fold") else ""), **extra}
        if pf:
            d_.update({"logit_max_abs": pf["logit_max_abs"], "key_rel_l2": pf["key_rel_l2"], "mask_flipped_fraction": pf["mask_flipped_fraction"], "bar": BAR,
                       "bar_met": bool(pf["logit_max_abs"] <= BAR), "margin": round(BAR / max(pf["logit_max_abs"], 1e-12), 2),
                       # the same engine on trained-like synthetic weights (peaked attention, massive channels): the honest figure for a real checkpoint
                       "trained_like_weights": {k: tlw.get(k) for k in ("logit_max_abs", "logit_rel_l2", "key_rel_l2", "mask_flipped_fraction")},
                       "bar_met_on_trained_like_weights": (None if not tlw else bool(tlw["logit_max_abs"] <= BAR))})
        return d_

    configurations = {mine: describe(mine, round(ips, 2), round(dt / a.steps * 1e3, 3), {"residual_stream": "fp16" if resid16 else "f32", "ln_fold": ln_fold, "this_line": True})}
    for name, o in others.items():
        configurations[name] = describe(name, o["value"], o["ms_per_step"], {k: o[k] for k in ("residual_stream", "ln_fold", "serial_ms_per_step", "steps", "roofline", "how") if k in o})
    met = [c_ for c_ in configurations.values() if c_.get("bar_met")]
    bar_meeting = dict(max(met, key=lambda c_: c_["value"])) if met else None       # the fastest configuration under the bar on the flat init
    met_tl = [c_ for c_ in configurations.values() if c_.get("bar_met") and c_.get("bar_met_on_trained_like_weights")]
    bar_meeting_tl = dict(max(met_tl, key=lambda c_: c_["value"])) if met_tl else None  # ... and the fastest one that ALSO meets it on the trained-like weights
    # why fp16 operands cost clock: per kernel class, same serial pass, own processes on this box (bf16 against fp16 operands on the same stream type)
    f16_vs_bf16 = None
    pair = ("bf16", "f16_f16_stream")
    if all(n_ == mine or n_ in others for n_ in pair):
        ka = {n_: ({k: v["avg_us"] for k, v in kernels.items()} if n_ == mine else others[n_]["kernels_avg_us"]) for n_ in pair}
        f16_vs_bf16 = {"avg_us_bf16_vs_f16": {k: [ka["bf16"][k], ka["f16_f16_stream"].get(k)] for k in ka["bf16"] if k in ka["f16_f16_stream"] and ka["bf16"][k] > 20},
                       "what": "same step on the fp16 residual stream, serial pass with HIP events: the fp16 MFMA kernels run longer at equal cycles (the chip holds a lower "
                               "clock on fp16 operands: profiles/r03_f16_vs_bf16_*); the fp16 build has no LayerNorm launches (folded into QKV / fc1, whose "
                               "epilogues carry the two per-row scalars instead)"}
    value, value_is = round(ips, 2), "the timed region"
    if sustained and sustained["value_sustained"] < 0.97 * ips:      # a burst figure the chip does not hold is not the headline
        value, value_is = sustained["value_sustained"], "the LAST ~10-s window of the sustained run (below 0.97 of the timed region's figure, reported as value_timed_region)"
    out = {
        "metric": METRIC,
        "value": value, "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": _dtype(a), "data": "synthetic", "full": True,
        "value_is": value_is, "value_timed_region": round(ips, 2), "value_sustained": (sustained or {}).get("value_sustained"), "sustained": sustained,
        "logit_max_abs": logit_max_abs, "bar": BAR, "bar_met": (None if logit_max_abs is None else bool(logit_max_abs <= BAR)),
        "logit_max_abs_trained_like_weights": own_tl.get("logit_max_abs"),
        "bar_met_trained_like_weights": (None if not own_tl else bool(own_tl["logit_max_abs"] <= BAR)),
        # the reference's OWN fp16-autocast forward against its f32 forward (emulated on the CPU oracle): [random-init weights, trained-like weights]
        "logit_max_abs_of_reference_fp16_autocast": [((par or {}).get("reference_fp16_autocast_emulation") or {}).get("logit_max_abs"),
                                                     (((par or {}).get("trained_like_weights") or {}).get("reference_fp16_autocast_emulation") or {}).get("logit_max_abs")],
        # throughput of the fastest configuration that MEETS the bar on the flat-init weights (None: no configuration measured / none meets it), and of the fastest one
        # that also meets it on the trained-like weights (the split-operand pass: the precision the reference caches its features at)
        "value_at_bar": (bar_meeting or {}).get("value"), "value_at_bar_config": (bar_meeting or {}).get("engine"),
        "value_at_bar_met_on_trained_like_weights": (bar_meeting or {}).get("bar_met_on_trained_like_weights"),
        "value_at_bar_on_trained_like_weights": (bar_meeting_tl or {}).get("value"), "value_at_bar_on_trained_like_weights_config": (bar_meeting_tl or {}).get("engine"),
        "drop_in_default_engine": ENGINE["f16_f16_stream"] + " = the configuration of this line" if mine == "f16_f16_stream" else ENGINE["f16_f16_stream"],
        "configurations": configurations, "bar_meeting_config": bar_meeting, "bar_meeting_config_on_trained_like_weights": bar_meeting_tl, "f16_vs_bf16_per_kernel": f16_vs_bf16,
        "host_enqueue_ms_per_step": round(m["host_enqueue"] / a.steps * 1e3, 3), "host_threads": m["host_threads"], "host_cores_pinned": m["pinned_cores"],
        "ranks_seen": m["ranks_seen"], "collectives": m.get("collectives"),
        "config": _config(a, m),
        "roofline": roofline, "cpu_baseline": cpu, "kernels": kernels, "final_loss": round(m["final_loss"], 6),
        "backbone_backward_mode": m["lora_mode"], "discriminator_phase": m["dis_phase"],
    }
    return out


def look_twice_leg(a, dev, lib, world, rank, host_threads, pinned_cores):
    """BASELINE configs[3] as SURVEY 8(d) defines C4's validation side: ViT-L/14, B = 16 per GPU, Look-Twice pass with the fallback centre box
    [129,129,259,259] (2x zoom) on every image.  A step = one validation batch, end to end on resident inputs: backbone over the B images (what the
    feature-cache pass does for the validation set) -> key maps -> ValLoop_Look_Twice.validate_batch (decode at 68 x 68, upsample + threshold, device CCL
    + box tables, ONE crop launch pair over all B crops, ONE backbone pass over the crops, decode at 37 x 37, Pillow-exact resize + paste) -> resize to
    the label size -> the nine COD measures (engine/runner/loop_UCOD_DPL.py:297-352).  The decoder's fg-head bias is set to -10 so that every first-stage
    mask is empty and every image takes the fallback box, as C4 prescribes; the work does not depend on the mask content."""
    import types
    from ucod_dpl_amd import ops
    from ucod_dpl_amd.data.utils.feature_extractor import backbone, ARCHS
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import loop_look_twice as LT
    from ucod_dpl_amd.engine.utils.metrics import statistics
    from ucod_dpl_amd.models.uscod import baseline
    D, heads, L, P, _, _ = ARCHS[a.arch]
    B, S = a.batch, a.image
    if a.half in ("split2", "split3"):
        bb = backbone.random_init(a.arch, seed=0, image_size=S, device=dev, gemm_variant=a.gemm_variant, precision=a.half)
    else:
        bb = backbone.random_init(a.arch, seed=0, image_size=S, device=dev, gemm_variant=a.gemm_variant, attn_variant=a.attn_variant, half=a.half, resid=a.resid,
                                  ln_fold={"auto": "auto", "on": True, "off": False}[a.ln_fold])
    bb.engine.streams = a.streams                             # both backbone passes as image-parallel halves on two HIP streams, like the training step's
    torch.manual_seed(5)
    model = baseline(CfgNode(dict(dim=D, feature_size=68, ema_weight=0.99, dis_use_features=False))).to(dev)
    with torch.no_grad():
        model.decoder.conv_out_fg.bias.fill_(-10.0)
    model.eval()
    runner = types.SimpleNamespace(device=dev, model=model, world_size=world, rank=rank, val_dataloader=[], logger=None)
    cfg = CfgNode(dict(train_cfg=dict(dist_train=False), model_cfg=dict(feature_size=68), val_cfg=dict(look_twice=True, look_twice_th=0.15, expand_type="dynamic"),
                       dataset_cfg=dict(valset_cfg=dict(image_size=(S, S)))))
    loop = LT.ValLoop_Look_Twice(cfg, runner, feature_extractor=bb)
    g = torch.Generator().manual_seed(1234 + rank)
    raw = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)            # the images as the loader's PIL path would hand them over
    mean, std = torch.tensor([0.485, 0.456, 0.406], device=dev), torch.tensor([0.229, 0.224, 0.225], device=dev)
    images = ((raw.float() / 255.0 - mean) / std).permute(0, 3, 1, 2).contiguous()              # first-stage input (Resize is the identity at 518 x 518)
    labels = (torch.rand(B, S, S, generator=g) > 0.7).float().to(dev)
    paths = [raw[i] for i in range(B)]
    stats = statistics()

    def step():
        _, key = bb(images)
        preds_up, boxes = loop.validate_batch(key, paths)
        stats.step(labels, ops.bilinear_resize(preds_up.reshape(B, 1, S, S).contiguous(), S, S).reshape(B, S, S) > 0.5)
        return preds_up, boxes, key

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(max(1, a.warmup)):
        preds_up, boxes, _ = step()
    if not all(b == [list(LT.DEFAULT_BOX)] for b in boxes):
        raise SystemExit("bench.py --look-twice: not every image took the fallback box")
    stats.reset()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        preds_up, boxes, key = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tdt = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
        dt = tdt.item()
    if a.dump_outputs and rank == 0:                          # the final masks, their boxes, the first-stage key maps of the last step
        dump_outputs(a.dump_outputs, {"preds_up": preds_up, "key": key,
                                      "boxes": torch.tensor([float(v) for b in boxes for bx in b for v in bx], dtype=torch.float64).reshape(-1, 4),
                                      "boxes_per_image": torch.tensor([float(len(b)) for b in boxes])})
    head = {"metric": "validation images/sec at 3x518x518 with the Look-Twice second pass (two backbone passes per image + decode + box logic + paste + COD measures)",
            "value": round(world * B * a.steps / dt, 2), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.half, "data": "synthetic",
            "full": a.full,
            "config": {"workload": f"BASELINE configs[3] (validation side, SURVEY 8d C4): {a.arch} @{S}x{S}, batch {B}/GPU, Look-Twice second pass with the fallback centre box "
                                   f"{LT.DEFAULT_BOX} (2x zoom) on every image", "global_batch": B * world, "parallelism": f"dp{world}", "random_init_weights": True,
                       "residual_stream": "fp16" if bb.engine.resid16 else "f32", "ln_fold": bool(bb.engine.ln_fold),
                       "batched": "all crops of all images in one crop launch pair, one backbone pass, one decoder pass, one paste call (loop_look_twice.py::look_twice_batch)",
                       "schedule": f"serial steps; each backbone pass as {a.streams} image-parallel sub-batches on independent HIP streams"}}
    if not a.full:
        if rank == 0:
            _flush_c_stdio()
            print(json.dumps(dict(head, host_threads=host_threads, host_cores_pinned=pinned_cores)), flush=True)
        return
    # exclusive per-class durations: the same step with each backbone pass on ONE stream (no two launches overlap)
    libs = [lib] + ([bb.engine.lib] if bb.engine.lib is not lib else [])
    bb.engine.streams = 1
    step()
    barrier()
    for l_ in libs:
        l_.ucod_prof_enable(1)
    stats.reset()
    for _ in range(a.steps):
        step()
    barrier()
    bb.engine.streams = a.streams
    ncls = lib.ucod_prof_num_classes()
    tot, cnt = (C.c_double * ncls)(), (C.c_longlong * ncls)()
    for l_ in libs:
        l_.ucod_prof_enable(0)
        t_, c_ = (C.c_double * ncls)(), (C.c_longlong * ncls)()
        l_.ucod_prof_collect(t_, c_)
        for i in range(ncls):
            tot[i] += t_[i]
            cnt[i] += c_[i]
    # the two halves alone: the first backbone pass, and everything behind it
    barrier()
    t1 = time.perf_counter()
    for _ in range(a.steps):
        _, key = bb(images)
    barrier()
    dt_first = time.perf_counter() - t1
    if rank != 0:
        return
    cpu = None
    if not a.no_cpu_baseline and world == 1:
        # CPU baseline of THIS leg on a bounded sample (one image: two f32 backbone passes of the oracle + its decoder + the oracle's Look-Twice box logic, crop,
        # resize and paste) and parity of the device path on the same image: box tables, the crop tensor bit for bit, the second pass's logits at 37 x 37
        from oracle import vit as OV, decoder as OD, look_twice as OLT
        from oracle.resize import torch_bilinear
        from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict
        sd = random_state_dict(a.arch, 0, S)
        dec = {k: v.detach().cpu().clone() for k, v in model.decoder.state_dict().items()}
        img_u8, x1 = raw[0].cpu().numpy(), images[:1].cpu()
        seen = {}

        def encode(crop):
            with torch.no_grad():
                _, k2 = OV.dinov2_forward(crop, sd, heads=heads, patch=P, eps=1e-6, full_last_layer=False)
                f2, _, _ = OD.rev_decoder_forward(k2, dec, orth="gram")
            seen["crop"], seen["logits"] = crop, f2
            return f2

        t0 = time.perf_counter()
        with torch.no_grad():
            _, key1 = OV.dinov2_forward(x1, sd, heads=heads, patch=P, eps=1e-6, full_last_layer=False)
            fg1, _, _ = OD.rev_decoder_forward(torch_bilinear(key1, 68, 68), dec, orth="gram")
        up1, boxes1 = OLT.process_preds(fg1, (S, S), 0.15, "dynamic")
        new1 = OLT.look_twice(img_u8, boxes1, up1.clone(), (S, S), encode)
        t_cpu = time.perf_counter() - t0
        bb.engine.streams = 1
        with torch.no_grad():
            _, key_d = bb(images[:1])
            mask_d, boxes_d = loop.validate_batch(key_d, [raw[0]])
            crop_d = loop.crop_batch(raw[0], [loop.resize_bbox(b, S, S, S, S) for b in boxes_d[0]])
            logits_d = model(bb(crop_d)[1])[0].cpu()
        bb.engine.streams = a.streams
        scale_ = float(seen["logits"].abs().max())
        cpu = {"value": round(1.0 / t_cpu, 4), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"1 image: oracle {a.arch} forward f32 twice (image, then its one crop) + oracle decoder at 68 x 68 and 37 x 37 + oracle Look-Twice box logic, "
                         f"Pillow-exact crop / resize / paste ({t_cpu:.1f} s)",
               "parity": {"what": "the device path on the same image against the oracle", "boxes_equal": bool(boxes_d[0] == boxes1),
                          "crop_tensor_bit_identical": bool(torch.equal(crop_d.cpu(), seen["crop"])),
                          "second_pass_logit_max_abs": round(float((logits_d - seen["logits"]).abs().max()), 6), "second_pass_logit_abs_max_of_reference": round(scale_, 4),
                          "first_pass_key_rel_l2": round(float((key_d.cpu() - key1).norm() / key1.norm()), 6),
                          "final_mask_equal": bool(torch.equal(mask_d[0].cpu(), new1.reshape(S, S)))}}
    gh = S // P
    tok, F = gh * gh + 1, 4 * D
    kernels = {}
    for i in range(ncls):
        if cnt[i] == 0:
            continue
        name = lib.ucod_prof_class_name(i).decode()
        avg_us = tot[i] / cnt[i] * 1e3
        k = {"launches_per_step": cnt[i] / a.steps, "avg_us": round(avg_us, 2), "ms_per_step": round(tot[i] / a.steps, 4)}
        fl = algorithmic_work(name, B, tok, D, F, heads, bb.engine.Kpad, D, 68 * 68)
        if name == "gemm_bf16_proj_fc2_scale_resid":
            per_step = 2 * (L - 1) * (2.0 * B * tok * D * D + 2.0 * B * tok * D * F)      # two backbone passes per step
            k["tflops"] = round(per_step / (tot[i] / a.steps * 1e-3) / 1e12, 1)
        elif fl:
            k["tflops"] = round(fl / (avg_us * 1e-6) / 1e12, 1)
        kernels[name] = k
    dom = max((n for n in kernels if "tflops" in kernels[n]), key=lambda n: kernels[n]["ms_per_step"])
    roofline = {"kernel": dom, "bound": "mfma", "achieved": kernels[dom]["tflops"], "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(kernels[dom]["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None, "avg_launch_us": kernels[dom]["avg_us"],
                "measured_in": "the same step with every backbone pass on ONE stream and HIP events around every launch (exclusive launch durations)"}
    out = {**head,
           "first_backbone_pass_ms": round(dt_first / a.steps * 1e3, 3),
           "second_pass_and_tail_ms": round((dt - dt_first) / a.steps * 1e3, 3),
           "roofline": roofline, "cpu_baseline": cpu, "kernels": kernels,
           "host_threads": host_threads, "host_cores_pinned": pinned_cores}
    _flush_c_stdio()
    print(json.dumps(out), flush=True)


def cpu_baseline(a, D, heads, L, P):
    """The CPU oracle (a parity-pinned restatement of the reference: HF Dinov2 forward + TrainLoop._process_batch with the
    reference's naive [B,HW,HW] orthogonality loss) timed on this box's host cores, on a bounded sample."""
    from oracle import vit as OV, train_step as OT, decoder as OD, discriminator as ODISC
    from oracle.resize import torch_bilinear
    from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict
    n = a.cpu_images
    torch.manual_seed(0)
    sd = random_state_dict(a.arch, 0, a.image)
    img = torch.randn(n, 3, a.image, a.image)
    pl = (torch.rand(n, 1, 16, 16) > 0.7).float()
    gen = torch.Generator().manual_seed(42)
    dec, ema, disc = OD.init_params(D, gen), OD.init_params(D, gen), ODISC.init_state(68, gen)
    st = OT.TrainState(dec, ema, disc, dict(feature_size=68, ema_weight=0.99, lr0=2e-4, dis_lr0=1e-3, step_lr_size=25, step_lr_gamma=0.95,
                                            dis_step_lr_size=25, dis_step_lr_gamma=0.95, max_epoch=25, start_finetune=-5))
    v1 = any(k.startswith("blocks.") for k in sd)               # DINO (v1) state dict: timm key names, no LayerScale (BASELINE configs[0])
    oracle_fwd = OV.dinov1_forward if v1 else OV.dinov2_forward
    if not v1 and "encoder.layer.0.layer_scale1.lambda1" not in sd:  # HF-format DINO (v1) weights carry no LayerScale: the engine multiplies by nothing,
        sd = dict(sd)                                                # the oracle by ones
        for i in range(L):
            sd[f"encoder.layer.{i}.layer_scale1.lambda1"] = sd[f"encoder.layer.{i}.layer_scale2.lambda1"] = torch.ones(D)
        v1 = True                                                    # (and the trained-like recipe below does not apply)
    t0 = time.perf_counter()
    with torch.no_grad():
        _, key = oracle_fwd(img, sd, heads=heads, patch=P, eps=1e-6, full_last_layer=True)
    t1 = time.perf_counter()
    with torch.no_grad():
        fg_ref, _, _ = OD.rev_decoder_forward(torch_bilinear(key, 68, 68), dec, orth="gram")
    OT.process_batch(st, key, pl, orth="naive")
    t2 = time.perf_counter()
    out = {"value": round(n / (t2 - t0), 4), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
           "sample": f"{n} images: oracle Dinov2 fwd f32 ({t1 - t0:.1f}s) + oracle _process_batch with the reference's naive orth loss ({t2 - t1:.1f}s)"}
    # Parity of the bf16 device path at FULL size against the f32 oracle on the same images and weights (report max-abs,
    # relative L2 and the fraction of mask pixels that land on the other side of the 0.5 threshold).  The oracle is the checker here.
    # (an error here is an error of the bench -- non-zero exit -- never a green line)
    from ucod_dpl_amd import ops
    from ucod_dpl_amd.vit_engine import ViTEngine
    from ucod_dpl_amd import parallel
    dev = torch.device("cuda", parallel.device_index())
    layer_ref = list(OV.dinov2_forward.layer_keys) if oracle_fwd is OV.dinov2_forward else None   # the key hook's map after every layer, f32 oracle
    emb = dec["learnable_embedding"].reshape(128).to(dev)
    hw = torch.cat((dec["conv_out_fg.weight"].reshape(64), dec["conv_out_bg.weight"].reshape(64))).to(dev)
    hb = torch.cat((dec["conv_out_fg.bias"], dec["conv_out_bg.bias"])).to(dev)

    def device_logits(key_dev):
        d = ops.bilinear_resize(ops.dba_project(key_dev, dec["decoupling.weight"].reshape(128, D).to(dev), dec["decoupling.bias"].to(dev)).view(n, 128, *key_dev.shape[-2:]), 68, 68).view(n, 128, 68 * 68)
        return ops.dba_heads(d, 0, emb, ops.dba_colnorm(d, 0, emb), hw, hb, want_bg=False)[0].view(n, 1, 68, 68).cpu()

    def parity(half, resid="auto", sd=sd, img=img, key=key, fg_ref=fg_ref, layer_ref=layer_ref, ln_fold="auto"):
        if half in ("split2", "split3"):
            from ucod_dpl_amd.vit_engine import SplitViTEngine
            eng = SplitViTEngine(sd, heads=heads, eps=1e-6, device=dev, terms=int(half[-1]))
            layer_ref = None                                        # (the per-layer table is the 16-bit engines' error budget)
        else:
            eng = ViTEngine(sd, heads=heads, eps=1e-6, device=dev, attn_variant=a.attn_variant, half=half, resid=resid, ln_fold=ln_fold)
        key_dev = eng(img.to(dev))
        kd, fd = key_dev.cpu(), device_logits(key_dev)
        per_layer = []
        for li in range(1, L + 1) if layer_ref is not None else ():       # error budget: key map after li layers vs the oracle's
            kl = eng.forward(img.to(dev), n_layers=li).cpu()
            per_layer.append(round(float((kl - layer_ref[li - 1]).norm() / layer_ref[li - 1].norm()), 6))
        eng.check_overflow(wait=True)
        res = {"residual_stream": "fp16" if eng.resid16 else "f32", "ln_fold": bool(eng.ln_fold),
               "key_rel_l2": round(float((kd - key).norm() / key.norm()), 8), "key_max_abs": round(float((kd - key).abs().max()), 7),
               "logit_max_abs": round(float((fd - fg_ref).abs().max()), 8), "logit_rel_l2": round(float((fd - fg_ref).norm() / fg_ref.norm()), 8),
               "mask_flipped_fraction": round(float(((fd > 0) != (fg_ref > 0)).float().mean()), 6)}
        if per_layer:
            res["key_rel_l2_after_layer"] = per_layer
        return res

    # The same comparison on TRAINED-LIKE synthetic weights (peaked attention rows, LayerScale 0.1 .. 1, two massive residual channels:
    # feature_extractor.trained_like_state_dict) -- the regime a real checkpoint puts the kernels in; the random init above is the flattest.
    from ucod_dpl_amd.data.utils.feature_extractor import trained_like_state_dict
    if v1:                                                      # (the trained-like recipe scales LayerScale and the HF key names: DINOv2 only)
        f16s = parity("f16", "f16")
        out["parity_full_size"] = {"what": f"{n} images at {a.image}x{a.image}, {a.arch}: device backbone + f32 device decoder vs the f32 oracle "
                                           f"(same random-init weights); north-star bar: logit max-abs <= 1e-3", "bf16": parity("bf16"), "f16_operands": parity("f16", "f32"),
                                   "f16_operands_f16_stream": f16s, "f16_operands_f16_stream_unfolded": f16s if not f16s["ln_fold"] else parity("f16", "f16", ln_fold=False)}
        return out
    sd_p = trained_like_state_dict(a.arch, 0, a.image)
    with torch.no_grad():
        _, key_p = OV.dinov2_forward(img, sd_p, heads=heads, patch=P, eps=1e-6, full_last_layer=False)
        fg_p, _, _ = OD.rev_decoder_forward(torch_bilinear(key_p, 68, 68), dec, orth="gram")
    peaked = dict(sd=sd_p, key=key_p, fg_ref=fg_p, layer_ref=None)

    # Second data point: the REFERENCE's own launcher numerics.  `accelerate launch --mixed_precision fp16`
    # (scripts/launch_train_first_stage.sh:20) autocasts the model forward; oracle/vit.py emulates those roundings (checked against torch's
    # autocast on the real HF module in tests/test_oracle_autocast.py).  How far that forward sits from ITS f32 self, same images and weights:
    def autocast_deviation(sd_x, key_x, fg_x):
        with torch.no_grad():
            _, key_ac = OV.dinov2_forward(img, sd_x, heads=heads, patch=P, eps=1e-6, full_last_layer=False, autocast=torch.float16)
            fg_ac, _, _ = OD.rev_decoder_forward(torch_bilinear(key_ac, 68, 68), dec, orth="gram")
        return {"what": "f32 oracle with torch-autocast(fp16) roundings (linear / matmul operands and results in fp16, LayerNorm / softmax f32) vs the plain f32 oracle; f32 decoder",
                "key_rel_l2": round(float((key_ac - key_x).norm() / key_x.norm()), 6), "logit_max_abs": round(float((fg_ac - fg_x).abs().max()), 6),
                "logit_rel_l2": round(float((fg_ac - fg_x).norm() / fg_x.norm()), 6), "mask_flipped_fraction": round(float(((fg_ac > 0) != (fg_x > 0)).float().mean()), 6)}

    out["parity_full_size"] = {
        "what": f"{n} images at {a.image}x{a.image}, {a.arch}: device backbone + f32 device decoder vs the f32 oracle (same random-init weights); "
                f"north-star bar: logit max-abs <= 1e-3",
        "bf16": parity("bf16"),
        "reference_fp16_autocast_emulation": autocast_deviation(sd, key, fg_ref),
        "f16_operands": parity("f16", "f32"),                      # fp16 operands on the f32 residual stream
        "f16_operands_f16_stream": parity("f16", "f16"),            # (LayerNorm folded into QKV / fc1: the engine's default for this pair)
        "f16_operands_f16_stream_unfolded": parity("f16", "f16", ln_fold=False),
        "split2": parity("split2"), "split3": parity("split3"),    # the split-operand pass (SplitViTEngine): two / three bf16 terms per f32 operand, f32 residual stream
        "trained_like_weights": {
            "what": "same images, trained_like_state_dict (pre-softmax score std ~4, row entropy ~3.7 of ln 1370 = 7.2, LayerScale 0.1 .. 1, "
                    "massive channels +-200); reference logits reach |%.2f| (flat init: |%.2f|)" % (float(fg_p.abs().max()), float(fg_ref.abs().max())),
            "bf16": parity("bf16", **peaked), "f16_operands": parity("f16", "f32", **peaked), "f16_operands_f16_stream": parity("f16", "f16", **peaked),
            "f16_operands_f16_stream_unfolded": parity("f16", "f16", ln_fold=False, **peaked),
            "split2": parity("split2", **peaked), "split3": parity("split3", **peaked),
            "reference_fp16_autocast_emulation": autocast_deviation(sd_p, key_p, fg_p)}}
    return out


if __name__ == "__main__":
    try:
        main()
    finally:
        sys.stdout.flush()
        # leave the process group in order (RCCL's communicator teardown at interpreter exit can take the process down before a block-buffered line is written:
        # the UCOD_FORCE_DIST=1 run of round 6 lost its line that way)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            try:
                torch.distributed.destroy_process_group()
            except Exception:                                   # noqa: BLE001
                pass
