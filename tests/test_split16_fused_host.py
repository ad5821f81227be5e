"""CPU: the fused fc1 -> activation -> fp16-term split launch ("split2hf": ucod_split16_gemm_act, UCOD_SPLIT16_FUSE_MLP; ucod_dpl_amd/csrc/split16.hip and the
kSplit16 drains of gemm_bf16_epilogue.h) -- presence of the new names, argument validation before any device work, the workspace the flag saves, the engine's and the
precision switch's argument checks, and the accuracy condition of the GPU test restated on the host: it must separate the exact-erf GELU the drain calls from the
minimax fit of the 16-bit drains (tests/test_gpu_split16_fused.py applies it to the kernels)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import split16_ref as R

NEW_NAMES = ["ucod_split16_gemm_act", "ucod_vit_split16_workspace_bytes_ex", "ucod_vit_split16_stream_offset_ex", "ucod_vit_forward_split16_ex"]
FUSE = 1                                                          # UCOD_SPLIT16_FUSE_MLP


def test_new_names_in_header_binding_and_both_libraries():
    from ucod_dpl_amd import native as N
    raw = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in NEW_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in N.SIGNATURES, n
        assert hasattr(N.load("bf16"), n) and hasattr(N.load("f16"), n), n
    assert re.search(r"enum\s*\{\s*UCOD_SPLIT16_FUSE_MLP\s*=\s*1\s*\}", text)          # the fifth new name: the flag
    assert N.SPLIT16_FUSE_MLP == FUSE
    assert N.load().ucod_abi_version() == 5 and N.load("f16").ucod_abi_version() == 5 and N.ABI_VERSION == 5
    assert "#define UCOD_ABI_VERSION 5" in raw


def desc(N, B=32, D=768, heads=12, F=3072, L=12):
    d = N.VitDesc()
    d.B, d.C, d.H, d.W, d.P, d.D, d.heads, d.F, d.L, d.Kpad = B, 3, 518, 518, 14, D, heads, F, L, 640
    d.eps = 1e-6
    return d


def test_gemm_act_validates_its_arguments_before_any_device_work():
    """UCOD_EINVAL (-1) for null pointers, op outside {1, 3}, N % 8 != 0, alpha / scale that are not powers of two; the bf16 library refuses everything.  (No GPU:
    nothing is launched -- every call below is refused before the GEMM entry is reached.)"""
    from ucod_dpl_amd import native as N
    f, b = N.load("f16"), N.load("bf16")
    one = ctypes.c_void_p(256)                                     # a non-null address that is never dereferenced
    ok = dict(op=1, a=one, b=one, out=one, M=64, N=64, K3=192, bias=one, alpha=2.0 ** -20, scale=16.0, variant=0)

    def call(lib, **kw):
        p = dict(ok, **kw)
        return lib.ucod_split16_gemm_act(p["op"], p["a"], p["b"], p["out"], p["M"], p["N"], p["K3"], p["bias"], p["alpha"], p["scale"], p["variant"], None)

    for k in ("a", "b", "out", "bias"):
        assert call(f, **{k: None}) == -1, k
    for op in (0, 2, 4, -1):
        assert call(f, op=op) == -1, op
    for Nn in (60, 68, 100, 0, -8):
        assert call(f, N=Nn) == -1, Nn
    assert call(f, op=3, N=60) == -1
    for bad in (3.0, 0.0, -2.0, float("inf"), float("nan"), 0.3):
        assert call(f, alpha=bad) == -1, bad
        assert call(f, scale=bad) == -1, bad
    assert call(f, M=0) == -1 and call(f, K3=0) == -1
    assert call(b) == -1 and call(b, op=3) == -1                  # the bf16 library exports the name and refuses it


def test_flags_and_the_workspace_the_fused_pass_saves():
    from ucod_dpl_amd import native as N
    f, b = N.load("f16"), N.load("bf16")
    one = ctypes.c_void_p(256)
    none = ctypes.c_size_t(-1).value
    # C2 (ViT-B/14, 518 x 518, batch 32; GELU) and the ViT-g shape (SwiGLU, F = 4096, D = 1536)
    for d, mlp, width in ((desc(N), 0, 1), (desc(N, D=1536, heads=24, F=4096, L=40), 1, 2)):
        M = d.B * 1370
        base = f.ucod_vit_split16_workspace_bytes(ctypes.byref(d), mlp)
        assert base > 0
        assert f.ucod_vit_split16_workspace_bytes_ex(ctypes.byref(d), mlp, 0) == base
        fused = f.ucod_vit_split16_workspace_bytes_ex(ctypes.byref(d), mlp, FUSE)
        assert 0 < fused <= base - M * d.F * 4 * width, (base, fused)
        assert fused >= M * d.D * 4 + 2 * M * 3 * d.D * 2 + M * 3 * d.D * 4 + M * 3 * d.F * 2          # stream, two split operands, f32 qkv, the split hidden
        assert f.ucod_vit_split16_stream_offset_ex(ctypes.byref(d), mlp, 0) == f.ucod_vit_split16_stream_offset(ctypes.byref(d), mlp) == 0
        assert f.ucod_vit_split16_stream_offset_ex(ctypes.byref(d), mlp, FUSE) == 0
        for flags in (2, 3, 4, -1, 1 << 16):                       # unknown flag bits
            assert f.ucod_vit_split16_workspace_bytes_ex(ctypes.byref(d), mlp, flags) == 0, flags
            assert f.ucod_vit_split16_stream_offset_ex(ctypes.byref(d), mlp, flags) == none, flags
    d = desc(N)
    need = f.ucod_vit_split16_workspace_bytes_ex(ctypes.byref(d), 0, FUSE)
    wsc = (ctypes.c_float * 49)(*([1.0] * 49))
    tab = (ctypes.c_void_p * (4 + 16 * 12))()
    fwd = f.ucod_vit_forward_split16_ex
    assert fwd(ctypes.byref(d), 0, FUSE, tab, wsc, 49, None, None, None, 0, None) == -1           # null pointers
    assert fwd(ctypes.byref(d), 0, 2, tab, wsc, 49, one, one, one, need, None) == -1              # unknown flag bit
    assert fwd(ctypes.byref(d), 0, FUSE | 4, tab, wsc, 49, one, one, one, need, None) == -1
    assert fwd(ctypes.byref(d), 0, FUSE, tab, wsc, 48, one, one, one, need, None) == -1           # one scale per weight matrix
    wsc[7] = 3.0
    assert fwd(ctypes.byref(d), 0, FUSE, tab, wsc, 49, one, one, one, need, None) == -1           # not a power of two
    wsc[7] = 1.0
    assert fwd(ctypes.byref(d), 0, FUSE, tab, wsc, 49, one, one, one, need - 1, None) == -2       # UCOD_ENOMEM: the fused pass's own, smaller size is what it asks for
    assert fwd(ctypes.byref(d), 0, 0, tab, wsc, 49, one, one, one, need, None) == -2              # ... and the unfused pass does not fit into it
    d.D, d.heads = 896, 14                                         # a width without a LayerNorm kernel: refused with or without the flag
    assert f.ucod_vit_split16_workspace_bytes_ex(ctypes.byref(d), 0, FUSE) == 0 and f.ucod_vit_split16_stream_offset_ex(ctypes.byref(d), 0, FUSE) == none
    d = desc(N)
    assert b.ucod_vit_forward_split16_ex(ctypes.byref(d), 0, FUSE, tab, wsc, 49, one, one, one, need, None) == -1      # the bf16 library refuses the pass


def test_engine_and_precision_switch_validate_their_arguments(monkeypatch):
    import inspect
    from ucod_dpl_amd import ops
    from ucod_dpl_amd.vit_engine import SplitViTEngine
    from ucod_dpl_amd.data.utils.feature_extractor import backbone, random_state_dict, ARCHS
    monkeypatch.setitem(ARCHS, "split16_fused_host_vit", (128, 2, 2, 14, 70, True))
    sd = random_state_dict("split16_fused_host_vit", seed=1)
    with pytest.raises(ValueError, match="fuse_mlp"):
        SplitViTEngine(sd, heads=2, device="cpu", terms=2, term="bf16", fuse_mlp=True)
    with pytest.raises(ValueError, match="fuse_mlp"):
        SplitViTEngine(sd, heads=2, device="cpu", terms=3, fuse_mlp=True)
    assert inspect.signature(SplitViTEngine.__init__).parameters["fuse_mlp"].default is False
    assert backbone.PRECISIONS["split2hf"] == 2 and backbone.TERM_TYPES["split2hf"] == "f16" and "split2hf" in backbone.FUSED_MLP
    assert backbone.PRECISIONS["split2h"] == 2 and "split2h" not in backbone.FUSED_MLP            # split2h keeps its launches
    assert backbone.PRECISIONS["f32eq"] == 3 and "f32eq" not in backbone.TERM_TYPES and "f32eq" not in backbone.FUSED_MLP
    with pytest.raises(ValueError, match="split2hf"):              # the error message lists the new name
        backbone.from_state_dict(sd, heads=2, device="cpu", precision="fp64")
    with pytest.raises(ValueError):                                # the split engines take no residual-stream / fold options
        backbone.from_state_dict(sd, heads=2, device="cpu", precision="split2hf", resid="f16")
    xs = torch.zeros(8, 192, dtype=torch.float16)
    with pytest.raises(ValueError, match="op"):
        ops.gemm_act_split16(xs, xs, torch.zeros(8), 2, 1.0, 16.0)
    with pytest.raises(TypeError):
        ops.gemm_act_split16(xs.float(), xs, torch.zeros(8), 1, 1.0, 16.0)
    with pytest.raises(ValueError, match="variant"):
        ops.gemm_act_split16(xs, xs, torch.zeros(8), 1, 1.0, 16.0, variant=5)
    with pytest.raises(RuntimeError, match="GPU"):                 # no CPU path
        ops.gemm_act_split16(xs, xs, torch.zeros(8), 1, 1.0, 16.0)


def gelu_minimax_f32(x):
    """gelu_erf2 of gemm_bf16_epilogue.h (the 16-bit drains' GELU) in f32 torch arithmetic: max(x, 0) - |x| 2^-p(|x|)."""
    a = x.abs()
    p = a * 4.881021588e-04 + (-7.198718842e-03)
    for c in (5.214663086e-02, 4.595958292e-01, 1.151000509e+00, 1.0):
        p = p * a + c
    return x.clamp_min(0.0) - a * torch.exp2(-p)


def test_accuracy_condition_separates_exact_erf_from_the_minimax_fit():
    """The GPU test's input and operation on the host.  z~ = what a scale-64 split keeps of 8 220 draws from 1.2 N(0, 1) (the accumulator of the one-hot GEMM is exactly
    S z~); GELU in f32, then the scale-16 split; reference f64 on z~.  exact erf: 6e-8 to 9e-8 depending on the erf routine (f32 GELU rounding 2^-25 rms-ish + the split's 2^-23); the minimax
    fit of the 16-bit drains: 4.6e-7 (|err| <= 7.1e-7 absolute against an output rms of ~0.8).  The GPU condition rel-L2(fused) <= 2 rel-L2(unfused) + 2e-8 with an
    exact-erf unfused pair is at most 1.4e-7: the erf restatement stays under it, the minimax form does not."""
    g = torch.Generator().manual_seed(8220)
    z = torch.randn(8220, generator=g) * 1.2
    hi, lo = R.split16(z, 64.0)
    zt = R.reconstruct(hi, lo, 64.0).float()                       # (22 bits: exact in f32)
    assert bool((zt.double() == R.reconstruct(hi, lo, 64.0)).all())
    ref = torch.nn.functional.gelu(zt.double())

    def after_split(v):
        h, l = R.split16(v, 16.0)
        return R.reconstruct(h, l, 16.0)

    e_erf = R.rel_l2(after_split(torch.nn.functional.gelu(zt)), ref)
    e_mm = R.rel_l2(after_split(gelu_minimax_f32(zt)), ref)
    print(f"restated fused drain: exact erf {e_erf:.3e}, minimax fit {e_mm:.3e}")
    assert e_erf < 1.4e-7, e_erf
    assert e_mm > 1.4e-7, e_mm
    assert 2 * e_erf + 2e-8 < e_mm                                 # the GPU bound, formed from the erf pair, excludes the minimax form
