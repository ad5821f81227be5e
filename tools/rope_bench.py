#!/usr/bin/env python3
"""ucod_rope_qk alone at the backbone's shape (ViT-B/16 at 512 x 512, batch 32: B = 32, tok = 1 + 4 + 1024, D = 768), on the fp16 QKV buffer of the 16-bit engines and
on the f32 buffer of the split passes, and ucod_rope_qk_ld in the transposed direction on the 16-bit dqkv_aug buffer of backbone-backward mode (row pitch 3 D + 64:
the 64 LoRA columns are skipped), interleaved in one process with ucod_layernorm_h16 on the same M and D -- the project's reference point for a row kernel
(DESIGN section 5.1).  Medians of 7 windows of 10 launches, device events.  Bytes are what the algorithm needs from HBM: the Q and K thirds of the patch rows read
and written once (the 256 KB table is served by L2 and not counted); LayerNorm: the fp16 row read, the 16-bit row written.

    python tools/rope_bench.py [out.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import rope_table  # noqa: E402

B, GH, R, D = 32, 32, 4, 768
WINDOWS, LAUNCHES = 7, 10


def main():
    lib = N.load("f16")
    n, heads = GH * GH, D // 64
    tok = 1 + R + n
    M = B * tok
    table = rope_table(GH, GH).cuda()
    q16 = torch.randn(M, 3 * D, device="cuda").half()
    q32 = torch.randn(M, 3 * D, device="cuda")
    dq16 = torch.randn(M, 3 * D + 64, device="cuda").half()
    x16 = torch.randn(M, D, device="cuda").half()
    y16 = torch.empty_like(x16)
    g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    runs = {
        "rope_qk_f16": (lambda: lib.ucod_rope_qk(N.ptr(q16), N.ROPE_ELEM_HALF, N.ptr(table), B, tok, R, heads, N.stream()), 2 * B * n * 2 * D * 2),
        "rope_qk_f32": (lambda: lib.ucod_rope_qk(N.ptr(q32), N.ROPE_ELEM_F32, N.ptr(table), B, tok, R, heads, N.stream()), 2 * B * n * 2 * D * 4),
        "rope_qk_ld_inverse_f16": (lambda: lib.ucod_rope_qk_ld(N.ptr(dq16), N.ROPE_ELEM_HALF, N.ptr(table), B, tok, R, heads, 3 * D + 64, 1, N.stream()), 2 * B * n * 2 * D * 2),
        "layernorm_h16": (lambda: lib.ucod_layernorm_h16(N.ptr(x16), N.ptr(g), N.ptr(b), N.ptr(y16), M, D, 1e-5, N.stream()), 2 * M * D * 2),
    }
    for fn, _ in runs.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(WINDOWS):                                    # interleaved: every window times each kernel once
        for name, (fn, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    out = {"shape": dict(B=B, tok=tok, n_reg=R, D=D, rows=M), "windows": WINDOWS, "launches_per_window": LAUNCHES, "kernels": {}}
    for name, (_, nbytes) in runs.items():
        med = statistics.median(us[name])
        out["kernels"][name] = {"hbm_bytes": nbytes, "us_median": round(med, 2), "us_min": round(min(us[name]), 2), "us_max": round(max(us[name]), 2),
                                "TB_per_s": round(nbytes / med / 1e6, 3)}
    ln = out["kernels"]["layernorm_h16"]["TB_per_s"]
    for name in ("rope_qk_f16", "rope_qk_f32", "rope_qk_ld_inverse_f16"):
        out["kernels"][name]["of_layernorm_h16_rate"] = round(out["kernels"][name]["TB_per_s"] / ln, 3)
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
