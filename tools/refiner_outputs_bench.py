#!/usr/bin/env python3
"""The gradient through the CORAL refiner's `outputs` (SparseRefiner(train_outputs=True)) at the config's full size (window length 56 -> 3136 tokens per
window, C = 768, B = 2, all 18 windows selected, random init), three steps interleaved in ONE process, median of ROUNDS x REPS (device events):
  (a) forward + ex_loss.backward() with the feature off;
  (b) forward + (ex_loss + <G, outputs>).backward() with it on;
  (c) ucod_gated_ensemble_bwd + ucod_window_gather alone, on the step's own tensors.
The condition: (b) <= 1.05 x (a), both measured in this run (a second CSF backward would show as roughly 2 x).  The spread between the rounds of (a) is
printed beside it: above 5 % the windows are too short to carry the ratio -- raise REPS.
    refiner_outputs_bench.py [rounds [reps]]     -> profiles/refiner_outputs_bench.txt (and stdout)
    refiner_outputs_bench.py ge [rounds [reps]]  -> stdout: ucod_gated_ensemble (the forward) alone at B = 2, 168 x 168, the production map, of whichever
                                                    library ucod_dpl_amd.native loads (profiles/gated_ensemble_fwd.txt keeps two such runs)"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ucod_dpl_amd import ops
from ucod_dpl_amd.engine.config import CfgNode
from ucod_dpl_amd.models.UDLR import SparseRefiner

GE_ONLY = len(sys.argv) > 1 and sys.argv[1] == "ge"
ARGS = sys.argv[2:] if GE_ONLY else sys.argv[1:]
ROUNDS = int(ARGS[0]) if len(ARGS) > 0 else 7
REPS = int(ARGS[1]) if len(ARGS) > 1 else (200 if GE_ONLY else 10)
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
    """{name: fn} -> {name: median over ROUNDS of the mean of REPS calls}, the forms taking turns inside every round"""
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timed(fn, REPS))
    return {k: statistics.median(v) for k, v in times.items()}, times


def main():
    def module(**keys):
        torch.manual_seed(0)
        return SparseRefiner.from_config(CfgNode(dict(window_size=WS, threshold=0.0015, **keys))).to(DEV).train()

    off, on = module(), module(train_outputs=True)
    g = torch.Generator().manual_seed(1)
    l = torch.randn(B, C, WL, WL, generator=g).to(DEV)
    h = torch.randn(B, WS * WS, C, WL, WL, generator=g).to(DEV)
    preds = (torch.randn(B, 1, WL, WL, generator=g) * 2).to(DEV)
    ht = torch.rand(B * WS * WS, 1, WL, WL, generator=g).to(DEV)
    G = torch.randn(B, 1, WS * WL, WS * WL, generator=g).to(DEV)
    n = B * WS * WS

    def step_off():
        for p in off.parameters():
            p.grad = None
        _, ex, opt = off(l, h, preds, ht)
        ex.backward()
        return opt

    def step_on():
        for p in on.parameters():
            p.grad = None
        out, ex, opt = on(l, h, preds, ht)
        (ex + (out * G).sum()).backward()
        return opt

    assert int(step_off()["mask"].sum()) == n, "not every window was selected"
    calls = on.csf_backward_calls
    opt = step_on()
    assert on.csf_backward_calls == calls + 1, "the CSF backward must run exactly once per backward"
    P = on._prepare(torch.device(DEV, torch.cuda.current_device()))
    l1 = ops.bilinear_resize(preds, WS * WL, WS * WL)
    cd = opt["coords_list"].to(torch.int32).contiguous()
    img = torch.arange(B, device=DEV, dtype=torch.int32).repeat_interleave(WS * WS)
    gwin = torch.zeros(n, 1, WL, WL, device=DEV)

    def ge_alone():
        dl2 = ops.gated_ensemble_bwd(l1, opt["h_preds"], opt["GE_w"], P["f0w"], P["f0b"], P["f2w"], G)[0]
        ops.window_gather(dl2, cd, img, gwin, True, WL, WL, WS)

    med, rounds = interleaved({"a": step_off, "b": step_on, "c": ge_alone})
    names = {"a": "(a) train_outputs off: forward + ex_loss.backward()", "b": "(b) on: forward + (ex_loss + <G, outputs>).backward()",
             "c": "(c) ucod_gated_ensemble_bwd + ucod_window_gather alone"}
    say(f"# SparseRefiner at {n} windows x {WL * WL} tokens, C = {C}; `outputs` [{B},1,{WS * WL},{WS * WL}] (median of {ROUNDS} x {REPS}, interleaved)")
    for k in med:
        say(f"{names[k]:58s} {med[k]:9.4f} ms   (rounds {', '.join(f'{t:.4f}' for t in rounds[k])})")
    spread = (max(rounds["a"]) - min(rounds["a"])) / med["a"]
    ratio = med["b"] / med["a"]
    say(f"spread between the rounds of (a): {spread * 100:.2f} %  (above 5 %: raise REPS, the ratio below does not carry)")
    say(f"(b) / (a) = {ratio:.4f}   (condition: <= 1.05; a second CSF backward would show as ~2)   (c) / (a) = {med['c'] / med['a'] * 100:.2f} %")
    write()
    if spread > 0.05:
        sys.exit("the rounds of (a) spread by more than 5 %: lengthen the windows (more REPS)")
    if ratio > 1.05:
        sys.exit(f"(b) / (a) = {ratio:.4f} > 1.05")


def ge_forward():
    """ucod_gated_ensemble alone on the production map: random logits, the module's default fuser"""
    from ucod_dpl_amd import native as N
    lib, st = N.load(), N.stream()
    torch.manual_seed(0)
    m = SparseRefiner.from_config(CfgNode(dict(window_size=WS, threshold=0.0015))).to(DEV)
    P = m._prepare(torch.device(DEV, torch.cuda.current_device()))
    g = torch.Generator().manual_seed(1)
    h = w = WS * WL
    l1, l2 = ((torch.randn(B, 1, h, w, generator=g) * 2).to(DEV) for _ in range(2))
    out, wgt = torch.empty_like(l1), torch.empty_like(l1)
    nbytes = lib.ucod_gated_ensemble_workspace_bytes(B, h, w)
    wsb = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call():
        N.check(lib.ucod_gated_ensemble(N.ptr(l1), N.ptr(l2), N.ptr(P["f0w"]), N.ptr(P["f0b"]), N.ptr(P["f2w"]), P["f2b"], N.ptr(out), N.ptr(wgt), N.ptr(wsb),
                                        B, h, w, st), "ucod_gated_ensemble")

    med, rounds = interleaved({"ge": call})
    first = wgt.clone()
    call()
    torch.cuda.synchronize()
    say(f"# ucod_gated_ensemble at [{B},1,{h},{w}] ({-(-h * w // 256)} workgroups per image), workspace {nbytes} bytes, library {N.LIB_PATH}")
    say(f"median of {ROUNDS} x {REPS}: {med['ge'] * 1e3:9.2f} us   (rounds {', '.join(f'{t * 1e3:.2f}' for t in rounds['ge'])})")
    say(f"GE_w of two calls bit-identical: {bool(torch.equal(first.view(torch.int32), wgt.view(torch.int32)))}")


def write():
    out = os.path.join(ROOT, "profiles", "refiner_outputs_bench.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("refiner_outputs_bench.py measures on the GPU: none found")
    say(f"refiner_outputs_bench.py {' '.join(sys.argv[1:])}  ({torch.cuda.get_device_name(0)})")
    ge_forward() if GE_ONLY else main()
