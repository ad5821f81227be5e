#!/usr/bin/env python3
"""The split-operand pass at BASELINE configs[1]'s shape (32 x 1370 tokens, D = 768).

    python tools/split_bench.py [--terms 2|3] [--precision split2|split3|split2h|split2hf] [--batch 32]      per-kernel times of one precision
    python tools/split_bench.py --engines split3,split2,split2h,split2hf --rounds 5 --json out.json         whole-pass images/s, the precisions INTERLEAVED round by round

HIP events around `iters` back-to-back launches of each piece (or whole passes), after a warm-up.  "split2h" is the fp16-term form (csrc/split16.hip), "split2hf" the
same with fc1 + GELU + split fused into one launch (ucod_split16_gemm_act)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucod_dpl_amd import native as N, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=2)
ap.add_argument("--precision", default="", choices=["", "split2", "split3", "split2h", "split2hf"], help="overrides --terms")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--engines", default="", help="comma-separated precisions: whole-pass images/s of SplitViTEngine on ViT-B/14 at 518 x 518, interleaved")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default="")
a = ap.parse_args()
if a.precision:
    a.terms = 3 if a.precision == "split3" else 2
H16 = a.precision in ("split2h", "split2hf")
FUSED = a.precision == "split2hf"
dev, T, B, tok, heads, D, F = "cuda", a.terms, a.batch, 1370, 12, 768, 3072
M, P = B * tok, ops.split_products(a.terms)
g = torch.Generator().manual_seed(0)
results = []


def timed(name, fn, flops=None, nbytes=None):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1e3
    extra = (f"  {flops / us / 1e6:8.1f} TF/s algorithmic ({flops * P / us / 1e6:7.1f} issued)" if flops else "") + (f"  {nbytes / us / 1e3:8.1f} GB/s" if nbytes else "")
    print(f"{name:34s} {us:9.1f} us{extra}", flush=True)
    results.append(dict(kernel=name, us=us))
    return us


def engines_mode():
    from ucod_dpl_amd.vit_engine import SplitViTEngine
    from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS
    kw = {"split2": dict(terms=2), "split3": dict(terms=3), "split2h": dict(terms=2, term="f16"), "split2hf": dict(terms=2, term="f16", fuse_mlp=True)}
    names = [n for n in a.engines.split(",") if n]
    sd = random_state_dict("dinov2_vitb14", 0, 518)
    img = torch.randn(B, 3, 518, 518, generator=g).to(dev)
    engs = {n: SplitViTEngine(sd, heads=ARCHS["dinov2_vitb14"][1], device=dev, **kw[n]) for n in names}
    out = {n: torch.empty(B, D, 37, 37, device=dev) for n in names}
    for n in names:                                              # warm-up: workspaces, first-launch costs
        for _ in range(2):
            engs[n](img, out=out[n])
        engs[n].check_overflow(wait=True)
    torch.cuda.synchronize()
    per = {n: [] for n in names}
    for r in range(a.rounds):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                engs[n](img, out=out[n])
            e1.record()
            torch.cuda.synchronize()
            per[n].append(B * a.iters / (e0.elapsed_time(e1) * 1e-3))
        print(f"round {r}: " + "  ".join(f"{n} {per[n][-1]:8.1f} img/s" for n in names), flush=True)
    for n in names:
        engs[n].check_overflow(wait=True)
    summary = {n: dict(images_per_s_median=statistics.median(per[n]), images_per_s_min=min(per[n]), images_per_s_max=max(per[n]),
                       spread_rel=(max(per[n]) - min(per[n])) / statistics.median(per[n]), rounds=per[n]) for n in names}
    doc = dict(tool="tools/split_bench.py", mode="engines", arch="dinov2_vitb14", size=518, batch=B, iters_per_round=a.iters, rounds=a.rounds,
               device=torch.cuda.get_device_name(0), interleaved=True, engines=summary)
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)


if a.engines:
    engines_mode()
    sys.exit(0)

x = torch.randn(M, D, generator=g).to(dev)
gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
qkv = torch.randn(M, 3 * D, generator=g).to(dev)
f1 = torch.randn(M, F, generator=g).to(dev)
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
bq, bp, b1 = torch.zeros(3 * D, device=dev), torch.zeros(D, device=dev), torch.zeros(F, device=dev)
ls = torch.ones(D, device=dev)
oq = torch.empty(M, 3 * D, device=dev)
if H16:
    lib = N.load("f16")
    need = lib.ucod_split16_attention_operand_bytes(B, tok, heads)
    opnd = torch.empty(need, dtype=torch.uint8, device=dev)
    aout, hs, gs = (torch.empty(M, 3 * n, dtype=torch.float16, device=dev) for n in (D, D, F))
    print(f"# split-operand pieces, fp16 terms ({a.precision}, P = 3), {B} x {tok} tokens, D = {D}")
    timed("layernorm_split16", lambda: N.check(lib.ucod_split16_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), hs.data_ptr(), M, D, 1e-6, 0, 64.0, st()), "ln"), nbytes=M * D * (4 + 6))
    timed("qkv_split16", lambda: N.check(lib.ucod_split16_qkv(qkv.data_ptr(), opnd.data_ptr(), B, tok, heads, 1.0, 0.18, 32.0, st()), "qs"), nbytes=M * 3 * D * 4 + need)
    timed("attention_split16_fwd", lambda: N.check(lib.ucod_split16_attention_fwd(opnd.data_ptr(), aout.data_ptr(), B, tok, heads, 32.0, 32.0, st()), "att"), flops=4.0 * B * heads * tok * tok * 64)
    if not FUSED:                                               # (split2hf has no row pass behind fc1: see the fused GEMM row below)
        timed("split16_rows(gelu) fc1 out", lambda: N.check(lib.ucod_split16_rows(f1.data_ptr(), F, gs.data_ptr(), M, F, 0, 1, 1.0, 16.0, st()), "sg"), nbytes=M * F * (4 + 6))
    timed("split16_scale_f32 (tokens)", lambda: N.check(lib.ucod_split16_scale_f32(x.data_ptr(), M * D, 1.0, st()), "sc"), nbytes=M * D * 8)
    sw = lambda t: ops.split_rows(t, 2, 1, term="f16", scale=ops.pow2_scale(t))  # noqa: E731
    gemm = ops._gemm_f16
else:
    lib = N.load()
    need = lib.ucod_attention_split_operand_bytes(B, tok, heads, T)
    opnd = torch.empty(need, dtype=torch.uint8, device=dev)
    aout, hs, gs = (torch.empty(M, P * n, dtype=torch.bfloat16, device=dev) for n in (D, D, F))
    print(f"# split-operand pieces, terms = {T} (P = {P}), {B} x {tok} tokens, D = {D}")
    timed("layernorm_split", lambda: N.check(lib.ucod_layernorm_split(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), hs.data_ptr(), M, D, 1e-6, T, 0, st()), "ln"), nbytes=M * D * (4 + 2 * P))
    timed("qkv_split", lambda: N.check(lib.ucod_qkv_split(qkv.data_ptr(), opnd.data_ptr(), B, tok, heads, T, 0.18, st()), "qs"), nbytes=M * 3 * D * 4 + need)
    timed("attention_split_fwd", lambda: N.check(lib.ucod_attention_split_fwd(opnd.data_ptr(), aout.data_ptr(), B, tok, heads, T, st()), "att"), flops=4.0 * B * heads * tok * tok * 64)
    timed("split_rows(gelu) fc1 out", lambda: N.check(lib.ucod_split_rows(f1.data_ptr(), F, gs.data_ptr(), M, F, T, 0, 1, 1.0, st()), "sg"), nbytes=M * F * (4 + 2 * P))
    sw = lambda t: ops.split_rows(t, T, 1)  # noqa: E731
    gemm = ops.gemm_bf16
wq = sw(torch.randn(3 * D, D, generator=g).to(dev) * 0.02)
wp = sw(torch.randn(D, D, generator=g).to(dev) * 0.02)
w1_raw = torch.randn(F, D, generator=g).to(dev) * 0.02
w1 = sw(w1_raw)
alpha1 = 1.0 / (64.0 * ops.pow2_scale(w1_raw)) if H16 else 1.0  # what leaves fc1's accumulator in the fp16-term pass: the LayerNorm class scale times the weight's
w2 = sw(torch.randn(D, F, generator=g).to(dev) * 0.02)
timed("GEMM qkv  (BIAS_F32)", lambda: gemm(N.EPI_BIAS_F32, hs, wq, oq, M, 3 * D, P * D, bias=bq), flops=2.0 * M * 3 * D * D)
if not FUSED:
    timed("GEMM fc1  (BIAS_F32)", lambda: gemm(N.EPI_BIAS_F32, hs, w1, f1, M, F, P * D, bias=b1), flops=2.0 * M * F * D)
if FUSED:                                                       # fc1 + exact-erf GELU + fp16-term split in one launch (ucod_split16_gemm_act)
    timed("GEMM fc1  (GELU_SPLIT16: fused)", lambda: ops.gemm_act_split16(hs, w1, b1, 1, alpha1, 16.0, out=gs), flops=2.0 * M * F * D)
if T == 2 and not H16:                                          # (the bf16-term pass's fused fc1 epilogue)
    timed("GEMM fc1  (GELU_SPLIT2: fused)", lambda: gemm(N.EPI_BIAS_GELU_SPLIT2, hs, w1, gs, M, F, P * D, bias=b1), flops=2.0 * M * F * D)
timed("GEMM proj (SCALE_RESID_F32)", lambda: gemm(N.EPI_BIAS_SCALE_RESID_F32, aout, wp, x, M, D, P * D, bias=bp, scale=ls, resid=x), flops=2.0 * M * D * D)
timed("GEMM fc2  (SCALE_RESID_F32)", lambda: gemm(N.EPI_BIAS_SCALE_RESID_F32, gs, w2, x, M, D, P * F, bias=bp, scale=ls, resid=x), flops=2.0 * M * D * F)
if a.json:
    with open(a.json, "w") as f:
        json.dump(dict(tool="tools/split_bench.py", mode="kernels", precision=a.precision or f"split{T}", batch=B, tokens=tok, D=D, iters=a.iters, kernels=results), f, indent=1)
