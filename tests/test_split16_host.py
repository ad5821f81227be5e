"""CPU: the fp16-term split ("split2h": two fp16 terms per operand, three partial products; ucod_dpl_amd/csrc/split16.hip) restated in torch and checked against f64,
the reconstruction bound of the split, the scale rules, argument validation of the engine / precision switch / C entry points, and the presence of the new names.

The emulation (tests/split16_ref.py) accumulates exactly and rounds the result to f32 once; what the MFMA's f32 accumulation adds is measured on the GPU
(tests/test_gpu_split16.py)."""
import os
import re

import pytest
import torch

from conftest import ROOT
import split16_ref as R

KINDS = ["unit", "massive", "small"]


def operand(kind, M, K, g):
    x = torch.randn(M, K, generator=g)
    if kind == "massive":
        x[:, 5] *= 200.0                                          # N(0, 1) + two x200 channels
        x[:, K // 2] *= 200.0
    if kind == "small":
        x = x * 1e-3                                              # N(0, 1e-6)
    return x


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("kind", KINDS)
def test_three_products_against_f64_with_per_tensor_scales(kind, K):
    """[512, K] x [256, K]^T, weights N(0, 0.02^2), both operands scaled per tensor to max in [2^13, 2^14) -- the rule the engine applies to every weight and
    ops.linear_split(term="f16") to both sides.  Bound 2e-7 = the f32 rounding of the result (2^-25 rms-ish) + the dropped lo lo term (2^-22 per product, random signs);
    the emulation sits at 7.4e-8 on all three operand kinds."""
    g = torch.Generator().manual_seed(K + len(kind))
    x, w = operand(kind, 512, K, g), torch.randn(256, K, generator=g) * 0.02
    sx, sw = R.pow2_scale(x), R.pow2_scale(w)
    assert R.is_pow2(sx) and R.is_pow2(sw) and 2.0 ** 13 <= float((w * sw).abs().max()) < 2.0 ** 14 and 2.0 ** 13 <= float((x * sx).abs().max()) < 2.0 ** 14
    assert R.saturated(x, sx) == 0 and R.saturated(w, sw) == 0
    ref = x.double() @ w.double().t()
    err = R.rel_l2(R.linear3(x, w, None, sx, sw), ref)
    print(f"split2h emulation kind={kind} K={K}: rel-L2 {err:.3e} (torch f32 GEMM {R.rel_l2(x @ w.t(), ref):.3e})")
    assert err < 2e-7, err


@pytest.mark.parametrize("kind", KINDS)
def test_three_products_with_the_fixed_layernorm_class_scale(kind):
    """The pass cannot scale an ACTIVATION per tensor (its maximum is not known when the kernel that writes it runs): it uses one power of two per operand class, 64 for
    LayerNorm outputs (bound 1023).  On unit-scale rows, with or without x200 channels, that is as good as the per-tensor rule (< 2e-7).  Rows of magnitude 1e-3 --
    which a LayerNorm output is not -- meet fp16's subnormal floor: lo is rounded at 2^-25 absolute, i.e. 2^-25 / (64 sqrt 3) rms per element against 1e-3:
    2.7e-7, the price of a scale chosen for range (the third row of the issue's table shows the unscaled case: 1.7e-5)."""
    g = torch.Generator().manual_seed(len(kind))
    x, w = operand(kind, 512, 768, g), torch.randn(256, 768, generator=g) * 0.02
    sx, sw = 64.0, R.pow2_scale(w)
    assert R.saturated(x, sx) == 0
    err = R.rel_l2(R.linear3(x, w, None, sx, sw), x.double() @ w.double().t())
    print(f"split2h emulation, class scale 64, kind={kind}: rel-L2 {err:.3e}")
    if kind == "small":
        floor = 2.0 ** -25 / 64 / 3 ** 0.5 / 1e-3
        assert err < (floor ** 2 + 2e-7 ** 2) ** 0.5, (err, floor)
        assert err < 4.4e-6 / 5                                   # still far below the two-term bf16 form
    else:
        assert err < 2e-7, err


def test_without_scales_the_subnormal_floor_costs_what_the_issue_measured():
    """No scale at all: weights of magnitude 0.02 lose an order of magnitude to fp16's subnormal spacing, activations of 1e-3 two: the scales are not optional."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(256, 768, generator=g) * 0.02
    x1, x3 = operand("unit", 512, 768, g), operand("small", 512, 768, g)
    e1 = R.rel_l2(R.linear3(x1, w, None, 1.0, 1.0), x1.double() @ w.double().t())
    e3 = R.rel_l2(R.linear3(x3, w, None, 1.0, 1.0), x3.double() @ w.double().t())
    assert 3e-7 < e1 < 3e-6 and 5e-6 < e3 < 5e-5, (e1, e3)


@pytest.mark.parametrize("s", [1.0, 64.0, 2.0 ** 14, 2.0 ** -3])
def test_reconstruction_bound_and_layout(s):
    g = torch.Generator().manual_seed(int(s * 8))
    x = torch.randn(37, 72, generator=g) * torch.logspace(-9, 0, 72)[None, :] * (60000.0 / s / 6)     # nine decades below the range's edge
    x = x.clamp(-65000.0 / s, 65000.0 / s)
    hi, lo = R.split16(x, s)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and R.saturated(x, s) == 0
    err = (R.reconstruct(hi, lo, s) - x.double()).abs()
    assert bool((err <= R.recon_bound(x, s)).all()), float((err / R.recon_bound(x, s)).max())
    assert bool((err > 2.0 ** -22 * x.double().abs()).any())      # ... and the floor term is really met by the small columns
    a, b = R.layout(x, s, 0), R.layout(x, s, 1)
    assert a.shape == (37, 216) and torch.equal(a[:, :72], hi) and torch.equal(a[:, 72:144], hi) and torch.equal(a[:, 144:], lo)
    assert torch.equal(b[:, :72], hi) and torch.equal(b[:, 72:144], lo) and torch.equal(b[:, 144:], hi)
    # beyond the range: clamped, and counted
    big = torch.tensor([[70000.0 / s, -1e9, 1.0]])
    assert R.saturated(big, s) == 2 and bool(torch.isfinite(R.split16(big, s)[0].float()).all())


def test_scale_must_be_a_power_of_two():
    assert R.is_pow2(1.0) and R.is_pow2(2.0 ** -20) and R.is_pow2(16384.0)
    assert not R.is_pow2(3.0) and not R.is_pow2(0.0) and not R.is_pow2(-2.0) and not R.is_pow2(float("inf"))
    with pytest.raises(AssertionError):
        R.split16(torch.ones(2, 8), 3.0)
    from ucod_dpl_amd import ops
    for t in (torch.tensor([0.02, -0.07]), torch.tensor([3000.0]), torch.tensor([1.0]), torch.tensor([2.0 ** -30])):
        s = ops.pow2_scale(t)
        assert s == R.pow2_scale(t) and R.is_pow2(s) and 2.0 ** 13 <= float(t.abs().max()) * s < 2.0 ** 14
    assert ops.pow2_scale(torch.zeros(3)) == 1.0


def test_new_names_in_header_binding_and_both_libraries():
    from ucod_dpl_amd import native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucod_dpl.h")).read(), flags=re.S)
    names = ["ucod_split16_class_scale", "ucod_split16_rows", "ucod_split16_layernorm", "ucod_split16_patch_im2col", "ucod_split16_scale_f32",
             "ucod_split16_attention_operand_bytes", "ucod_split16_qkv", "ucod_split16_attention_fwd", "ucod_split16_mfma_subnormal_probe",
             "ucod_vit_split16_workspace_bytes", "ucod_vit_split16_stream_offset", "ucod_vit_forward_split16"]
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in N.SIGNATURES, n
        assert hasattr(N.load("bf16"), n) and hasattr(N.load("f16"), n), n
    assert N.load().ucod_abi_version() == 5 and N.ABI_VERSION == 5


def test_entry_points_validate_their_arguments_before_any_device_work():
    """Null pointers, K % 8, LayerNorm widths without a kernel, scales that are not powers of two: UCOD_EINVAL (-1) from the fp16 library; the bf16 library refuses
    everything.  (No GPU: nothing is launched.)"""
    import ctypes
    from ucod_dpl_amd import native as N
    f, b = N.load("f16"), N.load("bf16")
    one = ctypes.c_void_p(256)                                     # a non-null address that is never dereferenced: every call below is refused first
    assert f.ucod_split16_rows(None, 8, None, 1, 8, 0, 0, 1.0, 1.0, None) == -1
    assert f.ucod_split16_rows(one, 64, one, 8, 60, 0, 0, 1.0, 1.0, None) == -1          # K % 8
    assert f.ucod_split16_rows(one, 64, one, 8, 64, 0, 0, 1.0, 3.0, None) == -1          # scale not a power of two
    assert f.ucod_split16_rows(one, 64, one, 8, 64, 2, 0, 1.0, 1.0, None) == -1          # role
    assert f.ucod_split16_rows(one, 64, one, 8, 64, 0, 3, 1.0, 1.0, None) == -1          # op 3 needs rows 2 K wide
    assert f.ucod_split16_layernorm(None, None, None, None, 1, 128, 1e-6, 0, 64.0, None) == -1
    for D in (100, 896, 1152, 1408, 1664):                         # D / 128 = 7, 9, 11, 13: no kernel -> refused by the op AND by the pass
        assert f.ucod_split16_layernorm(one, one, one, one, 1, D, 1e-6, 0, 64.0, None) == -1, D
    assert f.ucod_split16_layernorm(one, one, one, one, 1, 128, 1e-6, 0, 48.0, None) == -1
    assert f.ucod_split16_patch_im2col(one, one, 1, 3, 28, 28, 14, 600, 512.0, None) == -1   # Kpad % 64
    assert f.ucod_split16_patch_im2col(one, one, 1, 3, 28, 28, 14, 640, 500.0, None) == -1
    assert f.ucod_split16_scale_f32(one, 4, 0.3, None) == -1 and f.ucod_split16_scale_f32(None, 4, 0.5, None) == -1
    assert f.ucod_split16_qkv(one, one, 1, 33, 2, 1.0, 0.18, 24.0, None) == -1 and f.ucod_split16_qkv(None, one, 1, 33, 2, 1.0, 0.18, 32.0, None) == -1
    assert f.ucod_split16_attention_fwd(one, one, 1, 33, 2, 32.0, 33.0, None) == -1 and f.ucod_split16_attention_fwd(None, None, 1, 33, 2, 32.0, 32.0, None) == -1
    assert f.ucod_split16_mfma_subnormal_probe(None, None) == -1
    assert f.ucod_split16_attention_operand_bytes(1, 33, 2) == 3 * 2 * 64 * 2 * 64 * 2 and f.ucod_split16_attention_operand_bytes(0, 33, 2) == 0
    assert [f.ucod_split16_class_scale(c) for c in range(7)] == [64.0, 32.0, 16384.0, 32.0, 16.0, 512.0, 0.0]
    d = N.VitDesc()
    d.B, d.C, d.H, d.W, d.P, d.D, d.heads, d.F, d.L, d.Kpad = 32, 3, 518, 518, 14, 768, 12, 3072, 12, 640
    d.eps = 1e-6
    M = 32 * 1370
    need = f.ucod_vit_split16_workspace_bytes(ctypes.byref(d), 0)
    assert need >= M * 768 * 4 + 2 * M * 3 * 768 * 2 + M * 2304 * 4 + M * 3072 * 4 + M * 3 * 3072 * 2
    assert need < b.ucod_vit_split_workspace_bytes(ctypes.byref(d), 3)                   # 4 instead of 6 operand bytes per element
    assert f.ucod_vit_split16_stream_offset(ctypes.byref(d), 0) == 0
    wsc = (ctypes.c_float * 49)(*([1.0] * 49))
    tab = (ctypes.c_void_p * (4 + 16 * 12))()
    assert f.ucod_vit_forward_split16(ctypes.byref(d), 0, tab, wsc, 49, None, None, None, 0, None) == -1       # null pointers
    assert f.ucod_vit_forward_split16(ctypes.byref(d), 0, tab, wsc, 48, one, one, one, need, None) == -1       # one scale per weight matrix
    wsc[7] = 3.0
    assert f.ucod_vit_forward_split16(ctypes.byref(d), 0, tab, wsc, 49, one, one, one, need, None) == -1       # not a power of two
    wsc[7] = 1.0
    assert f.ucod_vit_forward_split16(ctypes.byref(d), 0, tab, wsc, 49, one, one, one, need - 1, None) == -2   # UCOD_ENOMEM
    for D, heads in ((896, 14), (1152, 18), (1664, 26)):           # every width the pass admits has a LayerNorm kernel: these have none
        d.D, d.heads = D, heads
        assert f.ucod_vit_split16_workspace_bytes(ctypes.byref(d), 0) == 0 and f.ucod_vit_split16_stream_offset(ctypes.byref(d), 0) == ctypes.c_size_t(-1).value
    d.D, d.heads = 1536, 24
    assert f.ucod_vit_split16_workspace_bytes(ctypes.byref(d), 1) > 0
    d.full_last_layer = 1
    assert f.ucod_vit_split16_workspace_bytes(ctypes.byref(d), 0) == 0
    # the bf16 library exports the names and refuses them
    assert b.ucod_split16_rows(one, 64, one, 8, 64, 0, 0, 1.0, 1.0, None) == -1
    assert b.ucod_split16_layernorm(one, one, one, one, 1, 128, 1e-6, 0, 64.0, None) == -1
    assert b.ucod_split16_scale_f32(one, 4, 0.5, None) == -1 and b.ucod_split16_mfma_subnormal_probe(one, None) == -1
    d.full_last_layer, d.D, d.heads = 0, 768, 12
    assert b.ucod_vit_forward_split16(ctypes.byref(d), 0, tab, wsc, 49, one, one, one, need, None) == -1


def test_engine_and_precision_switch_validate_their_arguments(monkeypatch):
    from ucod_dpl_amd import ops
    from ucod_dpl_amd.vit_engine import SplitViTEngine
    from ucod_dpl_amd.data.utils.feature_extractor import backbone, random_state_dict, ARCHS
    monkeypatch.setitem(ARCHS, "split16_host_vit", (128, 2, 2, 14, 70, True))
    sd = random_state_dict("split16_host_vit", seed=1)
    with pytest.raises(ValueError, match="term"):
        SplitViTEngine(sd, heads=2, device="cpu", terms=2, term="fp8")
    with pytest.raises(ValueError, match="two-term"):
        SplitViTEngine(sd, heads=2, device="cpu", terms=3, term="f16")
    with pytest.raises(ValueError, match="terms"):
        SplitViTEngine(sd, heads=2, device="cpu", terms=4, term="f16")
    with pytest.raises(ValueError):
        ops.split_rows(torch.zeros(8, 64), 3, 0, term="f16")
    with pytest.raises(ValueError):
        ops.split_rows(torch.zeros(8, 64), 2, 0, term="half")
    with pytest.raises(RuntimeError, match="GPU"):                 # no CPU path
        ops.split_rows(torch.zeros(8, 64), 2, 0, term="f16", scale=64.0)
    assert backbone.PRECISIONS["split2h"] == 2 and backbone.TERM_TYPES["split2h"] == "f16"
    assert backbone.PRECISIONS["f32eq"] == 3 and "f32eq" not in backbone.TERM_TYPES            # the default meaning of "f32eq" is unchanged: split3
    with pytest.raises(ValueError, match="split2h"):               # the error message lists the new name
        backbone.from_state_dict(sd, heads=2, device="cpu", precision="fp64")
    with pytest.raises(ValueError):                                # the split engines take no residual-stream / fold options
        backbone.from_state_dict(sd, heads=2, device="cpu", precision="split2h", resid="f16")
