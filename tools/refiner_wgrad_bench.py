#!/usr/bin/env python3
"""The refiner's weight gradients and optimizer step at the config's full size (18 windows x 3136 tokens, C = 768), one process, interleaved rounds as in
tools/refiner_train_bench.py:
  1. ops.weight_grad_direct (ucod_wgrad_bf16_det: token-major operands, split token axis) beside ops.weight_grad (two ucod_transpose_pad_bf16 + the plain
     GEMM) at the five shapes of profiles/refiner_train_bench.txt section 3, with nsplit, workspace bytes and TF/s;
  2. LocalRefineTrainLoop.step with direct_wgrad on and off beside the training forward + ex_loss.backward() under autograd, the two AdamW segment steps plus
     the re-preparation of the bf16 operands on their own line, and the peak memory of each.
    refiner_wgrad_bench.py [rounds [reps [kernel|step|all]]]     -> profiles/refiner_wgrad_bench.txt (and stdout)"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ucod_dpl_amd import native as N, ops
from ucod_dpl_amd.engine.config import CfgNode
from ucod_dpl_amd.models.UDLR import SparseRefiner

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WHAT = sys.argv[3] if len(sys.argv) > 3 else "all"
B, WS, WL, C = 2, 3, 56, 768
DEV = "cuda"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(forms):
    """{name: fn} -> ({name: median over ROUNDS of the mean of REPS calls}, {name: the rounds}), the forms taking turns inside every round"""
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timed(fn, REPS))
    return {k: statistics.median(v) for k, v in times.items()}, times


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def kernel_section():
    lib = N.load()
    n, HW = B * WS * WS, WL * WL
    M = n * HW
    bf = lambda *s: (torch.randn(*s, device=DEV) * 0.5).to(torch.bfloat16)          # noqa: E731
    say(f"# 1. weight gradients over M = {M} rows (median of {ROUNDS} x {REPS}, interleaved): direct = ucod_wgrad_bf16_det, parent = two ucod_transpose_pad_bf16 + ucod_gemm_bf16")
    tot = {"direct": [0.0] * ROUNDS, "parent": [0.0] * ROUNDS}
    for name, Nn, K in (("q", C, C), ("kv", 2 * C, C), ("out_proj", C, C), ("fc1", 4 * C, C), ("fc2", C, 4 * C)):
        dy, x = bf(M, Nn), bf(M, K)
        out = torch.empty(Nn, K, device=DEV)
        nbytes = lib.ucod_wgrad_bf16_det_workspace_bytes(M, Nn, K)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        med, rounds = interleaved({"direct": lambda: ops.weight_grad_direct(dy, x, out=out, ws=ws), "parent": lambda: ops.weight_grad(dy, x, out=out)})
        for k in tot:
            tot[k] = [a + b for a, b in zip(tot[k], rounds[k])]
        tf = lambda ms: 2.0 * M * Nn * K / ms / 1e9                                 # noqa: E731
        say(f"{name:9s} dW [{Nn:4d},{K:4d}]: direct {med['direct']:6.3f} ms {tf(med['direct']):6.1f} TF/s (nsplit {lib.ucod_wgrad_bf16_det_nsplit(M, Nn, K)}, workspace "
            f"{nbytes / 2**20:5.1f} MiB, spread {spread(rounds['direct']) * 100:.1f} %) | parent {med['parent']:6.3f} ms {tf(med['parent']):6.1f} TF/s (spread "
            f"{spread(rounds['parent']) * 100:.1f} %) | parent / direct = {med['parent'] / med['direct']:.2f}")
        del dy, x, out, ws
    d, p = statistics.median(tot["direct"]), statistics.median(tot["parent"])
    say(f"sum of the five: direct {d:.3f} ms (spread {spread(tot['direct']) * 100:.1f} %), parent {p:.3f} ms (spread {spread(tot['parent']) * 100:.1f} %), parent / direct = {p / d:.2f}")


def step_section():
    from types import SimpleNamespace
    from ucod_dpl_amd.engine.runner.loop_CORAL import LocalRefineTrainLoop
    g = torch.Generator().manual_seed(1)
    l = torch.randn(B, C, WL, WL, generator=g).to(DEV)
    h = torch.randn(B, WS * WS, C, WL, WL, generator=g).to(DEV)
    preds = (torch.randn(B, 1, WL, WL, generator=g) * 2).to(DEV)
    ht = torch.rand(B * WS * WS, 1, WL, WL, generator=g).to(DEV)
    n, HW = B * WS * WS, WL * WL
    batch = dict(features=l, h_inputs=h, h_targets=ht)

    def module():
        torch.manual_seed(0)
        return SparseRefiner.from_config(CfgNode(dict(window_size=WS, threshold=0.0015))).to(DEV).train()

    def loop(direct):
        cfg = CfgNode(dict(model_cfg=dict(window_length=WL),
                           train_cfg=dict(dist_train=False, lr0=1e-4, step_lr_size=10, step_lr_gamma=0.5, max_epoch=1, start_epoch=0, refiner_direct_wgrad=direct,
                                          save_cfg=dict(save_interval=1, start_save=0))))
        runner = SimpleNamespace(refiner=module(), model=lambda x: (preds,), device=torch.device(DEV, 0), train_dataloader=[batch])   # the frozen first stage: fixed logits
        return LocalRefineTrainLoop(cfg, runner)

    m_auto = module()
    loops = {True: loop(True), False: loop(False)}

    def autograd_step():
        for p in m_auto.parameters():
            p.grad = None
        _, ex, _ = m_auto(l, h, preds, ht)
        ex.backward()

    a, b, c = "LocalRefineTrainLoop.step (direct_wgrad)", "the same, refiner_direct_wgrad=False", "parent: forward + ex_loss.backward()"
    forms = {a: lambda: loops[True].step(batch), b: lambda: loops[False].step(batch), c: autograd_step}
    assert loops[True].step(batch)["windows"] == n, "not every window was selected"
    peaks = {}
    for k, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated() - base
    lp = loops[True]

    def update_only():
        lp.apply_updates(True, False)
        lp.refiner._prepare(l.device)

    forms["AdamW segment step (HRE.CSF) + re-preparation of the bf16 operands alone"] = update_only
    med, rounds = interleaved(forms)
    say(f"# 2. the whole step at {n} windows x {HW} tokens, C = {C} (median of {ROUNDS} x {REPS}, interleaved)")
    for k in med:
        peak = f"   peak +{peaks[k] / 2**20:.0f} MiB" if k in peaks else ""
        say(f"{k:76s} {med[k]:8.3f} ms   (spread {spread(rounds[k]) * 100:.1f} %){peak}")
    say(f"direct / non-direct = {med[a] / med[b]:.3f}; direct step - parent forward + backward = {med[a] - med[c]:+.3f} ms")


def write():
    out = os.path.join(ROOT, "profiles", "refiner_wgrad_bench.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("refiner_wgrad_bench.py measures on the GPU: none found")
    say(f"refiner_wgrad_bench.py {' '.join(sys.argv[1:])}  ({torch.cuda.get_device_name(0)})")
    if WHAT in ("kernel", "all"):
        kernel_section()
    if WHAT in ("step", "all"):
        step_section()
    write()
