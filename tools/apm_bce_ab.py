#!/usr/bin/env python3
"""A/B of builds of ucod_apm_bce at the step's size (B = 32, HW = 4624) in ONE process: per epoch fraction, the error of the three losses
against the f64 reference (tests/train_ref.apm_ref) over 300 launches -- the spread the order of the f32 atomics gives, with the count of
launches past the bound of tests/test_gpu_train_kernels.py -- and the time per launch.  Arms: `label=path-to-libucod_dpl.so` (default arm
`product` = the in-tree library).  One JSON line per (fraction, arm) on stdout.
  python tools/apm_bce_ab.py parent=/path/to/parent/libucod_dpl.so"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_ref as TR  # noqa: E402

vp, cf, ci = C.c_void_p, C.c_float, C.c_int
arms = [a.split("=", 1) for a in sys.argv[1:]] + [("product", os.path.join(ROOT, "ucod_dpl_amd", "_native", "libucod_dpl.so"))]
libs = {name: C.CDLL(path) for name, path in arms}
for lib in libs.values():
    lib.ucod_apm_bce.restype = ci
    lib.ucod_apm_bce.argtypes = [vp] * 6 + [cf, cf] + [vp] * 5 + [ci, ci, vp]

inp = TR.apm_inputs()
B, HW = TR.APM_SHAPE
d = {k: v.cuda() for k, v in inp.items()}
w = torch.empty(B, device="cuda")
merged, gfg, gbg = (torch.empty(B, HW, device="cuda") for _ in range(3))
losses = torch.empty(4, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
N = 300
for frac in TR.APM_FRACS:
    r64 = TR.apm_ref(inp, frac, TR.APM_GSCALE, torch.float64)
    r32 = TR.apm_ref(inp, frac, TR.APM_GSCALE, torch.float32)
    for name, lib in libs.items():
        def call():
            rc = lib.ucod_apm_bce(*[t.data_ptr() for t in (d["pl"], d["teacher"], d["fg"], d["bg"], d["p_s"], d["p_p"])], frac, TR.APM_GSCALE,
                                  *[t.data_ptr() for t in (w, merged, gfg, gbg, losses)], B, HW, stream)
            assert rc == 0, rc
        vals = []
        for _ in range(N):
            call()
            vals.append(losses[:3].clone())
        ls = torch.stack(vals).cpu().double()
        rec = {"frac": frac, "lib": name}
        for j, k in enumerate(("l1", "l2", "l3")):
            ref = float(r64[k])
            e = (ls[:, j] - ref).abs() / abs(ref)
            _, e32 = TR.compare(r32[k], r64[k], r32[k], 0)
            b = TR.bound(float(e32))
            rec[k] = {"max": float(e.max()), "median": float(e.median()), "over_bound": int((e > b).sum()), "bound": b,
                      "distinct_values": int(torch.unique(ls[:, j]).numel())}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(200):
            call()
        ev1.record()
        torch.cuda.synchronize()
        rec["us_per_launch"] = ev0.elapsed_time(ev1) * 1000 / 200
        print(json.dumps(rec), flush=True)
