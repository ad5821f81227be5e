"""CPU: the host side of backbone-backward (LoRA) mode on the SwiGLU MLP of DINOv2 ViT-g/14 (transformers modeling_dinov2.py:300-315) -- the checker form of the
dgrad epilogue (swiglu.swiglu_interleaved_grad) against torch.autograd in f64, the size helpers of the _mlp training entry points through the loaded library (no GPU
call), and the opt-in keyword of the engine."""
import ctypes as C
import inspect
import os

import pytest
import torch

from ucod_dpl_amd import swiglu


def _pre_dhid(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(5, 2 * 24, generator=g, dtype=torch.float64), torch.randn(5, 24, generator=g, dtype=torch.float64)


def test_interleaved_grad_is_the_autograd_of_swiglu_interleaved_in_f64():
    pre, dhid = _pre_dhid()
    leaf = pre.clone().requires_grad_(True)
    ref, = torch.autograd.grad((swiglu.swiglu_interleaved(leaf) * dhid).sum(), leaf)
    got = swiglu.swiglu_interleaved_grad(pre, dhid)
    assert got.shape == pre.shape and got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0.0)


def test_interleaved_grad_zeros_and_large_gate_values():
    pre, dhid = _pre_dhid(1)
    z = swiglu.swiglu_interleaved_grad(torch.zeros_like(pre), dhid)          # padded hidden units: x1 = x2 = 0
    assert float(z.abs().max()) == 0.0
    assert float(swiglu.swiglu_interleaved_grad(pre, torch.zeros_like(dhid)).abs().max()) == 0.0
    big = pre.clone()
    v = big[2].view(-1, 2, 4)
    v[:, 0, :2], v[:, 0, 2:] = 40.0, -40.0                                   # x1 = +-40 across one row
    for dt in (torch.float64, torch.float32, torch.bfloat16):
        out = swiglu.swiglu_interleaved_grad(big.to(dt), dhid.to(dt))
        assert out.dtype == dt and bool(torch.isfinite(out).all()), dt
    leaf = big.clone().requires_grad_(True)
    ref, = torch.autograd.grad((swiglu.swiglu_interleaved(leaf) * dhid).sum(), leaf)
    torch.testing.assert_close(swiglu.swiglu_interleaved_grad(big, dhid), ref, rtol=1e-12, atol=1e-300)


@pytest.fixture(scope="module")
def lib():
    from ucod_dpl_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load()


def _train_desc(F=3072):
    from ucod_dpl_amd import native as N
    t = N.VitTrainDesc()
    d = t.vit
    d.B, d.C, d.H, d.W, d.P, d.D, d.heads, d.F, d.L, d.Kpad = 4, 3, 518, 518, 14, 768, 12, F, 12, 640
    d.eps = 1e-6
    t.lora_r, t.lora_scaling, t.lora_dropout, t.seed = 2, 2.0, 0.0, 0
    return t


def test_mlp_size_helpers(lib):
    from ucod_dpl_amd import native as N
    t = _train_desc()
    gelu = lib.ucod_vit_train_workspace_bytes(C.byref(t))
    assert gelu > 0 and lib.ucod_vit_train_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_GELU) == gelu
    igelu = lib.ucod_vit_lora_infer_workspace_bytes(C.byref(t))
    assert igelu > 0 and lib.ucod_vit_lora_infer_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_GELU) == igelu
    # SwiGLU at equal F: the saved pre-activation of each of the L - 1 saving layers and the hidden / dpre transient are [M, 2F] instead of [M, F]
    sw = lib.ucod_vit_train_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_SWIGLU)
    M, F, L = 4 * 1370, 3072, 12
    assert sw >= gelu + L * M * F * 2 and sw > gelu
    # the no-grad pass keeps only the hidden [M, F] (the weights_in output never reaches memory): non-zero, and no smaller than the GELU pass's
    isw = lib.ucod_vit_lora_infer_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_SWIGLU)
    assert isw > 0 and isw >= igelu
    assert lib.ucod_vit_train_workspace_bytes_mlp(C.byref(t), 7) == 0
    assert lib.ucod_vit_lora_infer_workspace_bytes_mlp(C.byref(t), 7) == 0
    t.vit.heads = 11                                                         # head_dim != 64: refused for either kind
    assert lib.ucod_vit_train_workspace_bytes_mlp(C.byref(t), N.UCOD_MLP_SWIGLU) == 0


def test_mlp_passes_refuse_an_unknown_kind_before_any_device_work(lib):
    t = _train_desc()
    assert lib.ucod_vit_forward_train_mlp(C.byref(t), 7, None, None, None, None, None, 0, None) == -1
    assert lib.ucod_vit_backward_mlp(C.byref(t), 7, None, None, None, None, 0, None) == -1
    assert lib.ucod_vit_forward_lora_infer_mlp(C.byref(t), 7, None, None, None, None, None, 0, None) == -1


def test_epilogue_constants_follow_the_header():
    from conftest import ROOT
    from ucod_dpl_amd import native as N
    text = open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()
    assert f"UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 = {N.EPI_BIAS_SWIGLU_SAVE_BF16}," in text and N.EPI_BIAS_SWIGLU_SAVE_BF16 == 21
    assert f"UCOD_EPI_SWIGLU_BWD_BF16 = {N.EPI_SWIGLU_BWD_BF16}," in text and N.EPI_SWIGLU_BWD_BF16 == 22


def test_lora_engine_swiglu_is_opt_in():
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine
    assert inspect.signature(ViTLoRAEngine.__init__).parameters["allow_swiglu"].default is False
