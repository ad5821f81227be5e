#!/usr/bin/env python3
"""ucod_cls_attention_rope beside ucod_cls_attention_reg on the same buffers, at ViT-B/16's 512 x 512 shape (B = 32, 12 heads, hw = 1024, n_reg = 4): what rotating
the patch keys inside the row kernel costs.  One process, interleaved rounds (every window times each kernel once), device events; medians of 9 windows of 20
launches.  Both kernels read the key map once (B D hw f32 = 100.7 MB, the only traffic of size) and write B heads hw f32; the rotated one also reads the
[hw, 64] f32 table (256 KB) once per block, STRAIGHT FROM L2 -- each lane walks its own 256-byte row in 16-byte loads; no LDS staging (csrc/pseudo_label.hip).
There is no gate: the generator runs once per dataset, and one backbone pass at this shape costs tens of milliseconds.

    python tools/cls_row_bench.py [out.txt]          (profiles/dinov3_cls_row_kernel.txt holds an MI355X run)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import rope_table  # noqa: E402

B, HEADS, GH, R = 32, 12, 32, 4
WINDOWS, LAUNCHES = 9, 20


def main():
    lib = N.load("f16")
    hw, D = GH * GH, HEADS * 64
    g = torch.Generator().manual_seed(1)
    q = (2.0 * torch.randn(B, D, generator=g)).cuda()
    k_lead = torch.randn(B, 1 + R, D, generator=g).cuda()
    key = torch.randn(B, D, hw, generator=g).cuda()
    table = rope_table(GH, GH).cuda()
    att = torch.empty(B, HEADS, hw, device="cuda")
    runs = {
        "ucod_cls_attention_reg": lambda: lib.ucod_cls_attention_reg(N.ptr(q), N.ptr(k_lead), N.ptr(key), N.ptr(att), B, HEADS, hw, R, 0.125, N.stream()),
        "ucod_cls_attention_rope": lambda: lib.ucod_cls_attention_rope(N.ptr(q), N.ptr(k_lead), N.ptr(key), N.ptr(table), N.ptr(att), B, HEADS, hw, R, 0.125, N.stream()),
    }
    for fn in runs.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(WINDOWS):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    nbytes = (B * D * hw + B * HEADS * hw) * 4
    lines = [f"CLS attention row kernels at B = {B}, heads = {HEADS}, hw = {hw}, n_reg = {R} (ViT-B/16 at 512 x 512); device {torch.cuda.get_device_name(0)}",
             f"{WINDOWS} interleaved windows of {LAUNCHES} launches, device events; HBM bytes per launch (key map read + row written): {nbytes}",
             "table reads of the rotated kernel: straight from L2, a lane walking its 256-byte row in 16-byte loads (no LDS staging)", ""]
    med = {}
    for name in runs:
        med[name] = statistics.median(us[name])
        lines.append(f"{name:<26} median {med[name]:8.2f} us   min {min(us[name]):8.2f}   max {max(us[name]):8.2f}   {nbytes / med[name] / 1e6:6.3f} TB/s")
    lines.append("")
    lines.append(f"the rotation costs {med['ucod_cls_attention_rope'] - med['ucod_cls_attention_reg']:+.2f} us per launch "
                 f"({med['ucod_cls_attention_rope'] / med['ucod_cls_attention_reg']:.2f} x ucod_cls_attention_reg)")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
