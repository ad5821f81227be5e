"""Measure merging trained LoRA matrices into a live engine:  python tools/lora_merge_bench.py ARCH [ARCH ...] [--rounds N] [--out FILE]

For each architecture (dinov2_vitb14, dinov2_vitg14; random init, 224 px position rows) a LoRA engine with query / key / value and the MLP input projection
targeted (r = 2) and a default ``ViTEngine`` (fp16 operands, LayerNorm folded) over the same checkpoint.  Timed, interleaved, median of the rounds, host clock
around a device synchronise:

  merge_into   ``lora.merge_into(vit)``: stage the f32 base weights, merge, cast and fold into the live engine's tensors;
  rebuild      ``ViTEngine(lora.merged_state_dict(), ...)``: what it replaces (merge to the host, then the engine's own host-side fold and upload).

And the two kernels alone on the architecture's largest targeted matrix, device events around a run of launches, with the bytes the algorithm needs
(read w0 + write out + A + B;  read w + write fp16 + vectors) over that time.  One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import ARCHS, SWIGLU_ARCHS, random_state_dict  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, ViTLoRAEngine  # noqa: E402

DEV = "cuda"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_time(launch, iters=20):
    """seconds per launch: device events around ``iters`` launches, after a warm-up"""
    for _ in range(3):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def kernels(n, k, r):
    lib = N.load("f16")
    g = torch.Generator().manual_seed(0)
    w0, A, B = (torch.randn(*s, generator=g).to(DEV) for s in ((n, k), (r, k), (n, r)))
    gamma, beta, b = (torch.randn(s, generator=g).to(DEV) for s in (k, k, n))
    out, wf = torch.empty_like(w0), torch.empty(n, k, dtype=torch.float16, device=DEV)
    bias, cs = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    P, st = N.ptr, N.stream()
    t_merge = kernel_time(lambda: N.check(lib.ucod_lora_merge_f32(P(w0), P(A), P(B), r, 2.0, P(out), n, k, st), "ucod_lora_merge_f32"))
    t_fold = kernel_time(lambda: N.check(lib.ucod_fold_ln_linear(P(out), P(gamma), P(beta), P(b), None, P(wf), P(bias), P(cs), n, k, st), "ucod_fold_ln_linear"))
    merge_bytes = 2 * n * k * 4 + r * k * 4 + n * r * 4
    fold_bytes = n * k * 4 + n * k * 2 + 2 * k * 4 + 3 * n * 4
    return dict(shape=[n, k], r=r, merge_us=t_merge * 1e6, merge_bytes=merge_bytes, merge_TBps=merge_bytes / t_merge / 1e12,
                fold_us=t_fold * 1e6, fold_bytes=fold_bytes, fold_TBps=fold_bytes / t_fold / 1e12)


def bench(arch, rounds):
    D, heads, L = ARCHS[arch][:3]
    sd = random_state_dict(arch, seed=0, image_size=224)
    mlp_in = "weights_in" if arch in SWIGLU_ARCHS else "fc1"
    gen = torch.Generator().manual_seed(1)
    lora = ViTLoRAEngine(sd, heads=heads, r=2, lora_alpha=4, device=DEV, generator=gen, allow_swiglu=True, target_modules=["query", "key", "value", mlp_in])
    lsd = lora.lora_state_dict()
    lora.load_lora_state_dict({k: (0.05 * torch.randn(v.shape, generator=gen) if "lora_B" in k else v) for k, v in sorted(lsd.items())})
    vit = ViTEngine(sd, heads=heads, device=DEV)
    lora.merge_into(vit)                                         # warm-up: the staging buffer, the code objects
    t_merge, t_rebuild = [], []
    for _ in range(rounds):
        t_merge.append(timed(lambda: lora.merge_into(vit))[0])
        t, fresh = timed(lambda: ViTEngine(lora.merged_state_dict(), heads=heads, device=DEV))
        t_rebuild.append(t)
        print(f"{arch} round {len(t_merge)}: merge_into {t_merge[-1]:.3f} s, rebuild {t:.3f} s", file=sys.stderr, flush=True)
    same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for la, lb in zip(vit.layers, fresh.layers) for a, b in ((la[N.QKV_W], lb[N.QKV_W]), (la[N.FC1_W], lb[N.FC1_W])))
    staged = sum(sd[k].numel() * 4 for k in sd if k.endswith(".weight") and any(f".{m}." in k for m in ("query", "key", "value", mlp_in)))
    return dict(arch=arch, D=D, L=L, ln_fold=bool(vit.ln_fold), rounds=rounds, targets=["query", "key", "value", mlp_in], base_bytes_staged=staged,
                merge_into_s=dict(median=statistics.median(t_merge), all=t_merge), rebuild_s=dict(median=statistics.median(t_rebuild), all=t_rebuild),
                rebuild_over_merge_into=statistics.median(t_rebuild) / statistics.median(t_merge), refreshed_equals_rebuilt_weights=bool(same),
                kernels=kernels(lora.N1, D, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("arch", nargs="+", choices=sorted(ARCHS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_merge_bench needs a GPU: a CPU run measures nothing")
    doc = dict(tool="tools/lora_merge_bench.py", device=torch.cuda.get_device_name(0), results=[bench(arch, a.rounds) for arch in a.arch])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
