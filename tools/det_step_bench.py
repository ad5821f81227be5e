"""Cost of the deterministic training step: bench.py's decoder step (ViT-B/14 key map, B = 32, 37 x 37 features, fs = 68) from CACHED features, the default
(atomic) and the deterministic form of TrainLoop._process_batch timed interleaved in one process.

    python tools/det_step_bench.py [--rounds 7] [--steps 200] [--batch 32] [--out profiles/det_step_bench.json]

Each round times `steps` back-to-back steps of one form between two stream synchronisations, then the same for the other form (the order alternates from round
to round); the figure per form is the median over the rounds of (window / steps).  A window is hundreds of milliseconds, so the host clock's resolution
and the synchronisation's latency are below 1e-4 of it (docs/lab/blk16.md: windows that measure the clock).  The weight gradient -- the one reduction with a
workspace of any size -- is also timed on its own (HIP events around `steps` calls of ops.dba_wgrad), and the workspace bytes of every deterministic entry point
are listed.  For the split of the deterministic weight gradient into its two kernels run the tool under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(deterministic, dim, fs):
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.engine.utils.seed import set_random_seed
    set_random_seed(42)
    cfg = CfgNode(CfgNode.load_with_base(os.path.join(ROOT, "configs", "uscod", "UCOD-DPL_dinov2.py")))
    cfg.model_cfg.dim, cfg.model_cfg.feature_size = dim, fs
    cfg.log_cfg.log_path = "/tmp/ucod_det_bench"
    cfg.train_cfg["deterministic"] = bool(deterministic)
    runner = StandardRunner(cfg)
    return runner, TrainLoop(cfg, runner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--arch", default="dinov2_vitb14")
    ap.add_argument("--image", type=int, default=518)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ucod_dpl_amd import native, ops
    from ucod_dpl_amd.data.utils.feature_extractor import backbone, ARCHS
    lib = native.load()
    dev = torch.device("cuda", 0)
    D, _, _, P, _, _ = ARCHS[a.arch]
    fs, B = 68, a.batch
    g = torch.Generator().manual_seed(1234)
    images = torch.randn(B, 3, a.image, a.image, generator=g).to(dev)
    pl = (torch.rand(B, 1, 16, 16, generator=g) > 0.7).float().to(dev)
    bb = backbone.random_init(a.arch, seed=0, image_size=a.image, device=dev)
    key = bb(images)[1].float().contiguous().clone()             # the cached feature map: [B, D, 37, 37]
    del bb
    loops = {}
    for name, det in (("default", False), ("deterministic", True)):
        runner, loop = build(det, D, fs)
        assert loop.deterministic is det
        loops[name] = loop
        for _ in range(10):                                      # warm-up: allocator pools, workspace cache, code objects
            loop._process_batch((pl, key))
    torch.cuda.synchronize()

    def window(loop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loop._process_batch((pl, key))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    ms = {"default": [], "deterministic": []}
    for r in range(a.rounds):
        order = ("default", "deterministic") if r % 2 == 0 else ("deterministic", "default")
        for name in order:
            ms[name].append(window(loops[name]))

    # the weight gradient alone, at the step's shape (the gradient map on the native 37 x 37 grid)
    HW = key.shape[2] * key.shape[3]
    gd = torch.randn(B, 128, HW, generator=g).to(dev)
    x = key.view(B, D, HW)
    ws = ops.DetWorkspaces()
    gW = torch.empty(128, D, device=dev)

    def events(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps               # us per call

    wg = {"default": [], "deterministic": []}
    for r in range(a.rounds):
        for name in (("default", "deterministic") if r % 2 == 0 else ("deterministic", "default")):
            det = name == "deterministic"
            wg[name].append(events(lambda: ops.dba_wgrad(gd, x, gW=gW, deterministic=det, ws=ws if det else None)))

    res = {
        "tool": "tools/det_step_bench.py", "arch": a.arch, "batch": B, "dim": D, "features": list(key.shape[2:]), "feature_size": fs,
        "rounds": a.rounds, "steps_per_window": a.steps,
        "step_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": [round(t, 5) for t in v]} for k, v in ms.items()},
        "step_ms_delta_of_medians": statistics.median(ms["deterministic"]) - statistics.median(ms["default"]),
        "wgrad_us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in wg.items()},
        "workspace_bytes": {
            "ucod_dba_wgrad_det": lib.ucod_dba_wgrad_det_workspace_bytes(B, D, HW, 0),
            "ucod_dba_wgrad_det(exact)": lib.ucod_dba_wgrad_det_workspace_bytes(B, D, HW, 1),
            "ucod_dba_heads_fwd_det": lib.ucod_dba_heads_fwd_det_workspace_bytes(B, fs * fs),
            "ucod_dba_bwd_det (behind the default form's)": lib.ucod_dba_bwd_det_workspace_bytes(B, fs * fs) - lib.ucod_dba_bwd_workspace_bytes(B, fs * fs),
            "ucod_apm_bce_det": lib.ucod_apm_bce_det_workspace_bytes(B),
            "ucod_disc_fwd_det": lib.ucod_disc_fwd_det_workspace_bytes(B, fs),
            "ucod_disc_bwd_det (behind the default form's)": lib.ucod_disc_bwd_det_workspace_bytes(B, fs) - lib.ucod_disc_bwd_workspace_bytes(B, fs),
            "step_cache_total": loops["deterministic"].runner.det_ws.nbytes(),
        },
        "wgrad_planes": lib.ucod_dba_wgrad_det_workspace_bytes(B, D, HW, 0) // (128 * D * 4),
        "final_loss": {k: float(loops[k].last["loss"].item()) for k in loops},
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
