"""GPU: DINOv2 ViT-g/14's SwiGLU MLP (transformers modeling_dinov2.py:300-315) -- the fused epilogues UCOD_EPI_BIAS_SWIGLU_BF16 / UCOD_EPI_LNFOLD_SWIGLU_BF16 /
UCOD_EPI_BIAS_SWIGLU_SPLIT2 and ucod_split_rows op 3 against f64 on every tile path, with a poisoned guard region around the output; the engines (_mlp entry points)
against the SwiGLU restatement (tests/swiglu_ref.py); ViT-g itself at full width; the drop-in backbone on a SwiGLU checkpoint folder; the decoder step at C = 1536."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops, swiglu  # noqa: E402
from ucod_dpl_amd.fold import fold_layernorm_linear, row_stats  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import backbone, random_state_dict, trained_like_state_dict, ARCHS  # noqa: E402
from swiglu_ref import dinov2_swiglu_forward, random_swiglu_state_dict  # noqa: E402

DEV = "cuda"
EPI_SWIGLU, EPI_LNFOLD_SWIGLU, EPI_SWIGLU_SPLIT2 = N.EPI_BIAS_SWIGLU_BF16, N.EPI_LNFOLD_SWIGLU_BF16, N.EPI_BIAS_SWIGLU_SPLIT2
EINVAL = -1                                                     # UCOD_EINVAL
GUARD = 4096                                                    # bytes of poison on each side of an output


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def swiglu_f64(y):
    return swiglu.swiglu_interleaved(y.double())


def guarded(nbytes):
    """(whole buffer, byte offset of the payload): the payload between two GUARD-byte runs of 0xA5."""
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, GUARD


def guard_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


SHAPES = [(200, 768, 256), (1370, 8192, 1536), (4111, 8192, 256), (43840, 8192, 1536)]
VARIANTS = [0, 1, 2, 9, 10, 12, 13, 14]


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_swiglu_epilogue_vs_f64(half, shape):
    M, Nn, K = shape
    lib = N.load(half)
    dt = torch.float16 if half == "f16" else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(M + Nn)
    A = (torch.randn(M, K, device=DEV, generator=g) * 0.5).to(dt)
    B = (torch.randn(Nn, K, device=DEV, generator=g) * (1.0 / K ** 0.5)).to(dt)
    bias = torch.randn(Nn, device=DEV, generator=g)
    rows = torch.arange(M, device=DEV) if M <= 4111 else torch.cat((torch.arange(600, device=DEV), torch.arange(M - 600, M, device=DEV)))
    ref = swiglu_f64(A[rows].double() @ B.double().t() + bias.double())
    variants = VARIANTS if M <= 4111 else [0, 9, 10, 13, 14]
    for v in variants:
        nbytes = M * (Nn // 2) * 2
        buf, off = guarded(nbytes)
        rc = lib.ucod_gemm_bf16(EPI_SWIGLU, N.ptr(A), N.ptr(B), buf.data_ptr() + off, M, Nn, K, N.ptr(bias), None, None, None, 0, v, N.stream())
        assert rc == 0, (v, rc)
        torch.cuda.synchronize()
        assert guard_intact(buf, nbytes), f"variant {v} wrote outside its output"
        out = buf[off:off + nbytes].view(dt).view(M, Nn // 2)[rows]
        err = rel_l2(out, ref)
        # one 16-bit rounding of the output (bf16 2^-9, fp16 2^-12 relative, rms well below) + f32 accumulation + v_exp / v_rcp
        assert err < (3e-3 if half == "bf16" else 4e-4), (v, err)


def test_swiglu_epilogue_edge_values_and_refusals():
    lib = N.load("f16")
    M, Nn, K = 256, 768, 256
    A = torch.zeros(M, K, dtype=torch.float16, device=DEV)
    B = torch.zeros(Nn, K, dtype=torch.float16, device=DEV)
    bias = torch.ones(Nn, device=DEV)
    bias[0], bias[1], bias[2], bias[3] = float("-inf"), float("nan"), -1e4, float("inf")
    for v in VARIANTS:
        out = torch.empty(M, Nn // 2, dtype=torch.float16, device=DEV)
        assert lib.ucod_gemm_bf16(EPI_SWIGLU, N.ptr(A), N.ptr(B), N.ptr(out), M, Nn, K, N.ptr(bias), None, None, None, 0, v, N.stream()) == 0
        torch.cuda.synchronize()
        o = out.float().cpu()
        assert (o[:, 0] == 0).all() and torch.signbit(o[:, 0]).all(), v       # silu(-inf) * 1 = -0, not NaN
        assert o[:, 1].isnan().all(), v                                       # NaN propagates
        assert (o[:, 2] == 0).all() and (o[:, 3] == float("inf")).all(), v
    # the f32-accuracy SiLU (silu_f32) of the split epilogue, bf16 library: the same poisoned bias, segments hi | hi | lo
    lb = N.load("bf16")
    Ab, Bb = A.bfloat16(), B.bfloat16()
    for v in VARIANTS:
        o = torch.empty(M, 3, Nn // 2, dtype=torch.bfloat16, device=DEV)
        assert lb.ucod_gemm_bf16(EPI_SWIGLU_SPLIT2, N.ptr(Ab), N.ptr(Bb), N.ptr(o), M, Nn, K, N.ptr(bias), None, None, None, 0, v, N.stream()) == 0
        torch.cuda.synchronize()
        o = o.float().cpu()
        assert (o[:, 0:2, 0] == 0).all() and torch.signbit(o[:, 0:2, 0]).all() and (o[:, 2, 0] == 0).all(), v
        assert o[:, :, 1].isnan().all(), v
        assert (o[:, 0:2, 2] == 0).all() and (o[:, 0:2, 3] == float("inf")).all(), v
    # ucod_split_rows op 3 (silu_f32): x1 = -inf / NaN / -1e4 / +inf against x2 = 1
    for terms in (2, 3):
        x = torch.ones(64, 16, device=DEV)
        x[:, 0], x[:, 1], x[:, 2], x[:, 3] = float("-inf"), float("nan"), -1e4, float("inf")
        P = ops.split_products(terms)
        so = torch.empty(64, P * 8, dtype=torch.bfloat16, device=DEV)
        assert lb.ucod_split_rows(N.ptr(x), 16, N.ptr(so), 64, 8, terms, 0, 3, 1.0, N.stream()) == 0
        torch.cuda.synchronize()
        h = so.float().cpu().view(64, P, 8)[:, 0]
        assert (h[:, 0] == 0).all() and torch.signbit(h[:, 0]).all() and h[:, 1].isnan().all(), terms
        assert (h[:, 2] == 0).all() and (h[:, 3] == float("inf")).all(), terms
    out = torch.empty(M, Nn // 2, dtype=torch.float16, device=DEV)
    assert lib.ucod_gemm_bf16(EPI_SWIGLU, N.ptr(A), N.ptr(B), N.ptr(out), M, 764, K, N.ptr(bias), None, None, None, 0, 0, N.stream()) == EINVAL
    assert lib.ucod_gemm_bf16(EPI_SWIGLU_SPLIT2, N.ptr(A), N.ptr(B), N.ptr(out), M, Nn, K, N.ptr(bias), None, None, None, 0, 0, N.stream()) == EINVAL


@pytest.mark.parametrize("M", [200, 4111])
def test_lnfold_swiglu_vs_f64_layernorm_linear_swiglu(M):
    lib = N.load("f16")
    D, F0 = 256, 344
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, D, generator=g) * 2.0
    x[3] += 50.0                                                # a common-mode offset row (|mean| = 25 sigma)
    x = x.half().float()
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    w_in, b_in, w_out = torch.randn(2 * F0, D, generator=g) * D ** -0.5, 0.1 * torch.randn(2 * F0, generator=g), torch.randn(D, F0, generator=g)
    wp, bp, _ = swiglu.prepare(w_in, b_in, w_out)
    wf, bf, cs = fold_layernorm_linear(gamma, beta, wp, bp)
    st = row_stats(x, 1e-6).float()
    ln = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-6)
    ref = swiglu_f64(ln @ wp.double().t() + bp.double())
    xd, wfd, bfd, csd, std = (t.to(DEV).contiguous() for t in (x.half(), wf, bf, cs, st))
    Nn = wp.shape[0]
    for v in [0, 1, 2, 9, 12, 13]:
        out = torch.empty(M, Nn // 2, dtype=torch.float16, device=DEV)
        rc = lib.ucod_gemm_lnfold(EPI_LNFOLD_SWIGLU, N.ptr(xd), N.ptr(wfd), N.ptr(out), M, Nn, D, N.ptr(bfd), N.ptr(csd), N.ptr(std), None, 0, 1e-6, None, v, N.stream())
        assert rc == 0, (v, rc)
        torch.cuda.synchronize()
        err = rel_l2(out, ref)
        assert err < 2e-3, (v, err)                             # fp16 weights (2^-12) + fp16 output
        assert rel_l2(out[3], ref[3]) < 2e-3, v


@pytest.mark.parametrize("M,Nn,K", [(200, 768, 256), (1370, 8192, 512)])
def test_swiglu_split2_epilogue_reconstructs_f64(M, Nn, K):
    lib = N.load("bf16")
    g = torch.Generator(device=DEV).manual_seed(M)
    A = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    B = (torch.randn(Nn, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(Nn, device=DEV, generator=g)
    ref = swiglu_f64(A.double() @ B.double().t() + bias.double())
    F = Nn // 2
    for v in VARIANTS:
        nbytes = M * 3 * F * 2
        buf, off = guarded(nbytes)
        assert lib.ucod_gemm_bf16(EPI_SWIGLU_SPLIT2, N.ptr(A), N.ptr(B), buf.data_ptr() + off, M, Nn, K, N.ptr(bias), None, None, None, 0, v, N.stream()) == 0
        torch.cuda.synchronize()
        assert guard_intact(buf, nbytes), v
        o = buf[off:off + nbytes].view(torch.bfloat16).view(M, 3, F)
        assert torch.equal(o[:, 0], o[:, 1]), v                 # segments hi | hi | lo
        hi, lo = o[:, 0].double(), o[:, 2].double()
        assert (lo.abs() <= hi.abs() * 2.0 ** -8).all(), v       # lo is below half an ulp of hi
        assert rel_l2(hi + lo, ref) < 2.0 ** -16, (v, rel_l2(hi + lo, ref))


@pytest.mark.parametrize("terms", [2, 3])
def test_split_rows_op3_layout_and_reconstruction(terms):
    lib = N.load("bf16")
    M, K = 300, 1024
    x = torch.randn(M, 2 * K + 64, device=DEV) * 3.0            # pitch wider than 2 K
    P = ops.split_products(terms)
    out = torch.empty(M, P * K, dtype=torch.bfloat16, device=DEV)
    assert lib.ucod_split_rows(N.ptr(x), 2 * K + 64, N.ptr(out), M, K, terms, 0, 3, 1.0, N.stream()) == 0
    torch.cuda.synchronize()
    ref = swiglu_f64(x[:, :2 * K])
    seg = out.view(M, P, K)
    a_term = [0, 0, 1, 1, 0, 2][:P]
    t = [seg[:, a_term.index(s)].double() for s in range(terms)]
    for p in range(P):
        assert torch.equal(seg[:, p], seg[:, a_term.index(a_term[p])]), p
    assert rel_l2(sum(t), ref) < (2.0 ** -16 if terms == 2 else 2e-7)
    assert lib.ucod_split_rows(N.ptr(x), K, N.ptr(out), M, K, terms, 0, 3, 1.0, N.stream()) == EINVAL   # op 3 reads 2 K wide rows


def f64_key(sd, img, heads, **kw):
    from oracle import vit as OV
    sdd = {k: v.to(DEV, torch.float64) for k, v in sd.items()}
    gh, gw = img.shape[-2] // 14, img.shape[-1] // 14           # (the oracle's bicubic interpolation runs on the host: interpolate there, in f64)
    sdd["embeddings.position_embeddings"] = OV.dinov2_pos_embed(sd["embeddings.position_embeddings"].double(), gh, gw).to(DEV)
    return dinov2_swiglu_forward(img.to(DEV, torch.float64), sdd, heads, **kw)


# measured on MI355X (D = 128 / 256, 3 / 4 layers, 70 px, batch 2): f16 3.7e-4 / 6.4e-4 (folded), bf16 3.0e-3 / 3.1e-3, f16 on the f32 stream 3.7e-4 / 3.9e-4,
# split2 5.7e-6 / 5.7e-6, split3 4.8e-7 / 5.5e-7
ENGINES = [("f16", dict(), 3e-3), ("bf16", dict(half="bf16"), 6e-3), ("f16_f32_stream", dict(half="f16", resid="f32"), 3e-3),
           ("split2", dict(terms=2), 5e-5), ("split3", dict(terms=3), 5e-6)]


@pytest.mark.parametrize("D,heads,L", [(128, 2, 3), (256, 4, 4)])
@pytest.mark.parametrize("name,kw,bound", ENGINES, ids=[e[0] for e in ENGINES])
def test_engines_vs_restatement(D, heads, L, name, kw, bound):
    sd = random_swiglu_state_dict(D, heads, L, seed=D)
    img = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(5))
    _, ref, _ = f64_key(sd, img, heads, full_last_layer=False)
    eng = SplitViTEngine(sd, heads=heads, device=DEV, **kw) if "terms" in kw else ViTEngine(sd, heads=heads, device=DEV, **kw)
    assert eng.mlp == N.UCOD_MLP_SWIGLU and eng.F == 384 * D // 128
    if D == 256 and name == "f16":
        assert eng.ln_fold                                      # the fold path (D % 256 == 0)
    key = eng(img.to(DEV))
    eng.check_overflow(wait=True)
    err = rel_l2(key, ref)
    print(f"{name} D={D}: rel L2 {err:.2e}")
    assert err < bound, err


@pytest.fixture(scope="module")
def giant_sd():
    return random_state_dict("dinov2_vitg14", seed=0)


def test_vitg14_full_depth_224(giant_sd):
    img = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    _, ref, _ = f64_key(giant_sd, img, 24, full_last_layer=False)
    eng = ViTEngine(giant_sd, heads=24, device=DEV)
    assert eng.ln_fold and eng.F == 4096
    e16 = rel_l2(eng(img.to(DEV)), ref)
    eng.check_overflow(wait=True)
    del eng
    e3 = rel_l2(SplitViTEngine(giant_sd, heads=24, device=DEV, terms=3)(img.to(DEV)), ref)
    print(f"ViT-g/14 224 px 40 layers: f16 default {e16:.2e}, split3 {e3:.2e}")
    assert e16 < 6e-3 and e3 < 1e-5                             # measured 2.99e-3 / 5.5e-6 (40 layers of fp16 rounding / split-operand f32 rounding)


@pytest.mark.parametrize("weights", ["random", "trained_like"])
def test_vitg14_518_key_does_not_depend_on_the_batch(giant_sd, weights):
    sd = giant_sd if weights == "random" else trained_like_state_dict("dinov2_vitg14", seed=0)
    eng = ViTEngine(sd, heads=24, device=DEV)
    img = torch.randn(3, 3, 518, 518, generator=torch.Generator().manual_seed(2)).to(DEV)
    k3 = eng(img, n_layers=4)
    k1 = eng(img[:1].contiguous(), n_layers=4)
    eng.check_overflow(wait=True)
    _, ref, _ = f64_key(sd, img[:1].cpu(), 24, n_layers=4, full_last_layer=False)
    e = rel_l2(k1, k3[:1])
    print(f"{weights}: B=1 vs B=3 rel L2 {e:.2e}; vs f64 {rel_l2(k1, ref):.2e}")
    # not bitwise: B = 1 and B = 3 take different tile paths (and the fold's statistics vs partials), whose fp16 roundings differ; measured 4.5e-4 (random,
    # 9.5e-4 from f64) and 1.0e-3 (trained-like, 4.3e-3 from f64) -- the batch moves an image's key by less than the engine's own error
    assert e < rel_l2(k1, ref)


def test_dropin_backbone_on_a_swiglu_checkpoint_folder(tmp_path):
    from safetensors.torch import save_file
    from ucod_dpl_amd.engine.config import CfgNode
    import numpy as np
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g20_dinov2_swiglu_native.npz"))     # tests/golden/make_golden_swiglu.py (transformers)
    sd = random_swiglu_state_dict(128, 2, 3, image_size=int(z["image_size"]), seed=int(z["seed"]))     # (its weights: the host test checks their hash)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="dinov2", hidden_size=128, num_attention_heads=2, num_hidden_layers=3,
                                                          use_swiglu_ffn=True, layer_norm_eps=1e-6, patch_size=14)))
    cfg = CfgNode(dict(type="dinov2", backbone="facebook/dinov2-giant", backbone_type="huggingface", backbone_weights=str(tmp_path)))
    bb = backbone(cfg, device=DEV)
    img = torch.from_numpy(z["x"])
    gold_key, gold_att = torch.from_numpy(z["key"]), torch.from_numpy(z["cls_att"])
    _, ref, att_ref = f64_key(sd, img, 2, full_last_layer=False)
    _, key = bb(img.to(DEV))
    assert rel_l2(key, ref) < 3e-3 and rel_l2(key, gold_key) < 3e-3
    f32 = bb.with_precision("f32eq")
    _, k32 = f32(img.to(DEV))
    assert rel_l2(k32, ref) < 5e-6 and rel_l2(k32, gold_key) < 5e-6
    k2, att = f32.engine.forward_with_cls_attention(img.to(DEV))
    assert (att.double().cpu() - att_ref.cpu()).abs().max().item() < 2e-5
    assert (att.double().cpu() - gold_att.double()).abs().max().item() < 2e-5


def test_decoder_step_at_c1536(giant_sd):
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from oracle import train_step as OT
    torch.manual_seed(0)
    B, fs = 2, 12
    eng = ViTEngine(giant_sd, heads=24, device=DEV)
    key = eng(torch.randn(B, 3, 70, 70).to(DEV), n_layers=2)
    cfg = CfgNode(dict(
        model_cfg=dict(dim=1536, feature_size=fs, ema_weight=0.99, dis_use_features=False),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=2e-4, dis_lr0=1e-3, step_lr_size=25, dis_step_lr_size=25,
                       step_lr_gamma=0.95, dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1,
                       dis_intertrain=2, save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50), log_cfg=dict(log_interval=50, log_path="/tmp/ucod_swiglu_c1536", multi_rank=[0])))
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    dec0 = {k[len("decoder."):]: v.detach().cpu().clone() for k, v in runner.model.state_dict().items() if k.startswith("decoder.")}
    ema0 = {k[len("decoder_ema."):]: v.detach().cpu().clone() for k, v in runner.model.state_dict().items() if k.startswith("decoder_ema.")}
    disc0 = {k: v.detach().cpu().clone() for k, v in runner.discriminator.state_dict().items()}
    pl = (torch.rand(B, 1, 16, 16) > 0.7).float() * 0.9 + 0.05
    loss = loop._process_batch({"pseudo_label": pl, "label_tensor": torch.zeros(1), "features": key, "img_path": ["x"]})
    torch.cuda.synchronize()
    st = OT.TrainState(dec0, ema0, disc0, dict(feature_size=fs, ema_weight=0.99, lr0=2e-4, dis_lr0=1e-3, step_lr_size=25, step_lr_gamma=0.95,
                                               dis_step_lr_size=25, dis_step_lr_gamma=0.95, max_epoch=25, start_finetune=-5))
    ref = OT.process_batch(st, key.cpu(), pl, orth="gram")
    dw = (runner.model.decoder.decoupling.weight.detach().cpu() - st.dec["decoupling.weight"]).abs().max().item()
    de = (runner.model.decoder_ema.decoupling.weight.detach().cpu() - st.ema["decoupling.weight"]).abs().max().item()
    assert abs(loss.item() - ref["loss"].item()) < 1e-4 and dw < 5e-5 and de < 5e-5
