"""GPU: DINOv3 ViT checkpoints (HF DINOv3ViTModel: rotary position embedding on the patch tokens' q and k) on the frozen-backbone engines.

1  ucod_rope_qk (csrc/rope.hip) in both libraries, on the library's 16-bit type and on f32, against the f64 rotation of the same stored values:
   |got - ref| <= u |ref| + 4 * 2^-24 (|a cos| + |b sin|) (+ 2^-25 for fp16, whose smallest results are subnormal), u = 2^-11 (fp16) / 2^-8 (bf16) / 0 (f32) -- one
   output rounding plus the f32 evaluation; and as CONDITIONS: the V third, every CLS / register row and the guard bands in front of and behind the buffer are bit
   for bit the input.  One case whose work exceeds the launch's block cap (the grid-stride loop).
2  every engine against the G22 goldens (transformers' own f64 outputs; tests/golden/make_golden_dinov3.py) under the bounds of tests/dinov3_ref.engine_bound,
   each of which tests/test_dinov3_host.py shows to lie under half the smallest fault distance of its golden: a pass that rotates wrongly cannot stay inside.
3  invariants: batch independence, stream invariance, full_last_layer.
4  the surface: backbone.random_init / with_precision / backbone(fe_cfg) with config.json, the refusals, and a DINOv2 engine untouched by a DINOv3 one.

Measured on an MI355X (conftest.within leaves every bounded figure in its tolerance audit file): the kernel's worst element, in units of its bound, 0.9994 (fp16) /
0.9958 (bf16) -- u is the type's exact half-ulp, so a value just above a power of two sits at the bound -- and 0.47 / 0.49 (f32, either library); G22 key relative L2 --
split3 4.3 - 5.4e-7, split2h = split2hf 3.5 - 4.2e-7 (bound 2.2 - 2.4e-6), split2 5.1 - 5.5e-6 (2.2e-5), fp16 operands 3.7 - 3.9e-4 (f32 stream) / 5.6 - 6.1e-4 (fp16
stream) / 6.0e-4 (folded, D = 256) (1.4 - 1.5e-3), bf16 3.2e-3 (1.2e-2); dinov3_vits16 @96 default vs f32eq 5.3e-4 (1.5e-3); theta = 37 from config.json 4.4e-7 from
its own f64 key map and 1.6e-2 from theta = 100's.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import within

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, rope_table  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import backbone, random_state_dict  # noqa: E402
import dinov3_ref as R3  # noqa: E402

DEV = "cuda"
SENT = -5.0                                                     # guard value (exact in every type used here)
GUARD = 4096                                                    # elements in front of and behind the buffer (a multiple of 16 bytes in every type)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ELEM = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8), "f32": (torch.float32, 0.0)}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Banded:
    """``values`` (any shape) between two guard bands of SENT, in the values' dtype, on the device."""

    def __init__(self, values):
        self.numel = values.numel()
        self.buf = torch.full((self.numel + 2 * GUARD,), SENT, dtype=values.dtype, device=DEV)
        self.payload = self.buf[GUARD:GUARD + self.numel]
        self.payload.copy_(values.reshape(-1))

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.numel:] == SENT).all())


# ================================================================================================ 1. the kernel
def rope_case(name, lib_half, elem, B, gh, gw, R, D, device_ref=False):
    """Run ucod_rope_qk on a guarded [B tok, 3 D] buffer and check values and conditions.  Inputs: N(0, 1) with every seventh token row scaled by 2^-16, so that some
    fp16 results are subnormal (|v| < 2^-14)."""
    lib = N.load(lib_half)
    dtype, u = ELEM[elem]
    n, heads = gh * gw, D // 64
    tok = 1 + R + n
    g = torch.Generator().manual_seed(1000 * n + 10 * R + D)
    x = torch.randn(B, tok, 3 * D, generator=g)
    x[:, ::7] *= 2.0 ** -16
    x = x.to(dtype)
    table = rope_table(gh, gw)
    buf, tdev = Banded(x), table.to(DEV)
    rc = lib.ucod_rope_qk(buf.ptr(), N.ROPE_ELEM_F32 if elem == "f32" else N.ROPE_ELEM_HALF, N.ptr(tdev), B, tok, R, heads, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert buf.guards_intact(), "wrote outside the buffer"
    where = DEV if device_ref else "cpu"
    got = buf.payload.view(B, tok, 3 * D).to(where)
    x = x.to(where)
    assert torch.equal(got[:, :, 2 * D:], x[:, :, 2 * D:]), "the V third changed"
    assert torch.equal(got[:, :1 + R], x[:, :1 + R]), "a CLS or register row changed"
    # the f64 rotation of the stored values: q | k of the patch rows as [B, n, 2 heads, 64]
    v = x[:, 1 + R:, :2 * D].double().reshape(B, n, 2 * heads, 64)
    a, b = v[..., :32], v[..., 32:]
    c, s = table[:, None, :32].double().to(where), table[:, None, 32:].double().to(where)
    ref = torch.cat((a * c - b * s, b * c + a * s), -1)
    mag = torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), -1)
    bound = u * ref.abs() + 4 * 2.0 ** -24 * mag + (2.0 ** -25 if elem == "f16" else 0.0)
    err = (got[:, 1 + R:, :2 * D].double().reshape(B, n, 2 * heads, 64) - ref).abs()
    if elem == "f16":
        assert bool(((ref.abs() < 2.0 ** -14) & (ref != 0)).any()), "the case holds no subnormal fp16 result"
    # the worst element in units of its bound (<= 1: inside); the zero-bound elements (exact zeros) must be exact
    assert bool((err[bound == 0] == 0).all())
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert float(ref.abs().max()) > 1.0 and float((got[:, 1 + R:, :2 * D].double() - x[:, 1 + R:, :2 * D].double()).abs().max()) > 0.1, "nothing was rotated"
    within(name, worst, 1.0 + 1e-12)


@pytest.mark.parametrize("R", [0, 1, 4])
@pytest.mark.parametrize("gh,gw", [(5, 5), (4, 6)])
@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("lib_half,elem", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32")])
def test_rope_kernel(lib_half, elem, D, gh, gw, R):
    rope_case(f"rope {lib_half}:{elem} D={D} {gh}x{gw} R={R}", lib_half, elem, 3, gh, gw, R, D)


@pytest.mark.parametrize("lib_half,elem", [("f16", "f16"), ("bf16", "f32")])
def test_rope_kernel_beyond_the_block_cap(lib_half, elem):
    """B = 24, a 16 x 16 grid, D = 768: 24 * 256 * 12 * 8 = 589 824 lanes = 2304 blocks of 256, more than the launch's cap of 2048 -- the grid-stride loop runs."""
    rope_case(f"rope {lib_half}:{elem} beyond the block cap", lib_half, elem, 24, 16, 16, 4, 768, device_ref=True)


def test_rope_kernel_refuses_nonsense_without_writing():
    lib = N.load("f16")
    x = Banded(torch.randn(2 * 10 * 384).half())
    before = x.buf.clone()
    t = rope_table(1, 5).to(DEV)
    call = lambda elem, B, tok, R, heads, q=None, tab=None: lib.ucod_rope_qk(x.ptr() if q is None else q, elem, N.ptr(t) if tab is None else tab, B, tok, R, heads, N.stream())  # noqa: E731
    assert call(2, 2, 10, 4, 2) == -1 and call(0, 0, 10, 4, 2) == -1 and call(0, 2, 10, -1, 2) == -1 and call(0, 2, 10, 9, 2) == -1 and call(0, 2, 10, 4, 0) == -1
    assert call(0, 2, 10, 4, 2, q=x.ptr() + 2) == -1 and call(0, 2, 10, 4, 2, tab=t.data_ptr() + 4) == -1      # 16-byte loads and stores
    torch.cuda.synchronize()
    assert torch.equal(x.buf, before)


# ================================================================================================ 2. engines against G22
@functools.lru_cache(maxsize=None)
def g22(tag):
    z = np.load(os.path.join(GOLDEN, f"g22_dinov3_{tag}.npz"))
    # (the weights: tests/test_dinov3_host.py checks their hash)
    return z, R3.g22_state_dict(tag), torch.from_numpy(z["x"]), torch.from_numpy(z["key"])


def make_engine(precision, sd, heads, **kw):
    kw = dict(dict(heads=heads, eps=1e-5, device=DEV), **kw)
    if precision == "f16_fold":
        return ViTEngine(sd, **kw)
    if precision == "f16_resid32":
        return ViTEngine(sd, resid="f32", **kw)
    if precision == "f16_resid16":
        return ViTEngine(sd, resid="f16", ln_fold=False, **kw)
    if precision == "bf16":
        return ViTEngine(sd, half="bf16", **kw)
    if precision in ("split2", "split3"):
        return SplitViTEngine(sd, terms=int(precision[-1]), **kw)
    return SplitViTEngine(sd, terms=2, term="f16", fuse_mlp=precision == "split2hf", **kw)


@pytest.mark.parametrize("precision,tag", R3.ENGINE_ROWS)
def test_engines_against_the_g22_goldens(precision, tag):
    z, sd, x, key_ref = g22(tag)
    m = R3.G22[tag]
    eng = make_engine(precision, sd, m["heads"])
    assert eng.rope and eng.kind == "dinov3" and eng.R == m["R"] and eng.ln_fold == (precision == "f16_fold")
    assert (eng.mlp == N.UCOD_MLP_SWIGLU) == m["gated"]
    d = eng._desc(x.shape[0], x.shape[2], x.shape[3])
    assert d.rope == eng._rope(*m["grid"]).data_ptr() and d.n_reg == m["R"]
    assert not bool(eng._pos(*m["grid"]).any())                   # slot +3: zeros [1 + n, D]
    key = eng(x.to(DEV)).cpu()
    eng.check_overflow(wait=True)
    assert key.shape == key_ref.shape
    err, bound = rel_l2(key, key_ref), R3.engine_bound(precision, z)
    print(f"g22 {tag} {precision}: key rel-L2 {err:.3e} (bound {bound:.2e})")
    within(f"g22:{tag}:{precision}", err, bound)


# ================================================================================================ 3. invariants
@pytest.mark.parametrize("precision,tag", [("f16_resid32", "g46"), ("f16_resid16", "g46"), ("f16_fold", "d256"), ("bf16", "d256"), ("split2", "g46"), ("split3", "g46"),
                                           ("split2h", "g46"), ("split2hf", "gated")])
def test_key_map_does_not_depend_on_the_batch_or_the_streams(precision, tag):
    """Image 0 alone against image 0 inside a batch of 5 (the non-square 4 x 6 golden's input plus three images), and one stream against two.  The stream count never
    changes a bit; the batch changes tile shapes, i.e. the f32 summation order: the bounds of tests/test_gpu_registers.py's test of the same name."""
    _, sd, x2, _ = g22(tag)
    x = torch.cat((x2, torch.randn(3, *x2.shape[1:], generator=torch.Generator().manual_seed(5))), 0).to(DEV)
    eng = make_engine(precision, sd, R3.G22[tag]["heads"])
    k5 = eng(x).clone()
    k1 = eng(x[:1].contiguous()).clone()
    bound = 3e-5 if precision == "split2" else 5e-6 if precision.startswith("split") else (8e-3 if precision == "bf16" else 1e-3)
    assert rel_l2(k1, k5[:1]) < bound, rel_l2(k1, k5[:1])
    if isinstance(eng, ViTEngine):
        eng.streams = 2
        k2 = eng(x).clone()
        eng.streams = 1
        assert torch.equal(k2[:2], eng(x[:2].contiguous())) and torch.equal(k2[2:], eng(x[2:].contiguous()))
    eng.check_overflow(wait=True)


@pytest.mark.parametrize("precision,tag", [("f16_resid32", "g46"), ("f16_fold", "d256"), ("bf16", "d256")])
def test_full_last_layer_gives_the_same_key_map(precision, tag):
    """The key hook takes k before the rotation; with full_last_layer the last layer then runs QKV, the rotation and attention as well (output discarded)."""
    _, sd, x, _ = g22(tag)
    heads = R3.G22[tag]["heads"]
    a, b = make_engine(precision, sd, heads), make_engine(precision, sd, heads, full_last_layer=True)
    ka, kb = a(x.to(DEV)).clone(), b(x.to(DEV)).clone()
    b.check_overflow(wait=True)
    assert torch.equal(ka, kb)


# ================================================================================================ 4. the surface
def test_random_init_and_with_precision():
    bb = backbone.random_init("dinov3_vits16", image_size=96, device=DEV)
    assert isinstance(bb.engine, ViTEngine) and bb.engine.rope and bb.engine.R == 4 and bb.engine.eps == 1e-5 and bb.engine.P == 16
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
    _, key = bb(x)
    assert tuple(key.shape) == (2, 384, 6, 6) and bool(torch.isfinite(key).all())
    eq = bb.with_precision("f32eq")
    assert isinstance(eq.engine, SplitViTEngine) and eq.engine.rope and eq.engine.R == 4
    e = rel_l2(key, eq(x)[1])
    print(f"dinov3_vits16 @96 default vs f32eq: {e:.3e}")
    within("dinov3_vits16 default vs f32eq", e, 1.5e-3)           # the bound tests/test_gpu_registers.py holds this pair to
    # the gated sibling runs as well (SwiGLU entry points, F = 4 D)
    bp = backbone.random_init("dinov3_vits16plus", image_size=96, device=DEV, precision="split2h")
    assert bp.engine.mlp == N.UCOD_MLP_SWIGLU and bp.engine.F == 1536
    assert bool(torch.isfinite(bp(x)[1]).all())


def test_backbone_from_a_checkpoint_folder_reads_eps_and_rope_theta(tmp_path):
    from safetensors.torch import save_file
    from ucod_dpl_amd.engine.config import CfgNode
    z, sd, x, _ = g22("g46")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="dinov3_vit", num_attention_heads=2, num_register_tokens=4, rope_theta=37.0)))
    cfg = CfgNode(dict(backbone_type="huggingface", type="dinov3", backbone="facebook/dinov3-vits16-pretrain-lvd1689m", backbone_weights=str(tmp_path), precision="split3"))
    bb = backbone(cfg, device=DEV)
    assert bb.engine.eps == 1e-5 and bb.engine.rope_theta == 37.0 and bb.engine.R == 4
    key = bb(x.to(DEV))[1]
    ref37, ref100 = R3.forward_f64(x, sd, 2, theta=37.0), torch.from_numpy(z["key"])
    e = rel_l2(key, ref37)
    print(f"theta = 37 from config.json: {e:.3e} from its f64 key map, {rel_l2(key, ref100):.3e} from theta = 100's")
    assert e < R3.engine_bound("split3", z) and rel_l2(key, ref100) > 100 * e
    assert bb.with_precision("f16").engine.rope_theta == 37.0    # a property of the checkpoint: sibling engines get it
    # config.json against the tensor, as for DINOv2 with registers
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="dinov3_vit", num_attention_heads=2, num_register_tokens=1)))
    with pytest.raises(ValueError, match="num_register_tokens"):
        backbone(cfg, device=DEV)


def test_refusals():
    _, sd, x, _ = g22("g46")
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        ViTEngine(sd, heads=2, eps=1e-5, device=DEV, attn_variant=8)
    for eng in (make_engine("f16_resid32", sd, 2), make_engine("split3", sd, 2)):
        with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
            eng.forward_with_cls_attention(x.to(DEV))
    from ucod_dpl_amd.generate_pseudo_label import PseudoLabelGenerator
    gen = PseudoLabelGenerator(backbone.from_state_dict(sd, heads=2, eps=1e-5, device=DEV), th_bkg=0.6)
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        gen.raw_masks(x)
    # the drivers themselves: the fp8 path and the training passes take no table (size helpers answer 0 = invalid descriptor, before any launch)
    eng = make_engine("f16_resid32", sd, 2)
    d = eng._desc(2, 64, 96)
    lib16, libb = N.load("f16"), N.load("bf16")
    assert lib16.ucod_vit_workspace_bytes_mlp(C.byref(d), eng.mlp) > 0
    d.attn_variant = 8
    assert lib16.ucod_vit_workspace_bytes_mlp(C.byref(d), eng.mlp) == 0
    key = torch.empty(2, 128, 4, 6, device=DEV)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=DEV)
    table, _keep = eng._table(4, 6)
    assert lib16.ucod_vit_forward_mlp(C.byref(d), eng.mlp, table, N.ptr(x.to(DEV)), N.ptr(key), N.ptr(ws), ws.numel(), N.stream()) == -1
    d.rope = None
    assert lib16.ucod_vit_workspace_bytes_mlp(C.byref(d), eng.mlp) > 0
    t = N.VitTrainDesc()
    C.memmove(C.byref(t.vit), C.byref(eng._desc(2, 64, 96)), C.sizeof(N.VitDesc))
    t.vit.attn_variant, t.lora_r, t.lora_scaling = 2, 2, 2.0
    assert libb.ucod_vit_train_workspace_bytes(C.byref(t)) == 0 and libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) == 0
    t.vit.rope = None
    assert libb.ucod_vit_train_workspace_bytes(C.byref(t)) > 0 and libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) > 0


@pytest.mark.parametrize("precision", ["f16", "split2h"])
def test_a_dinov2_engine_is_untouched_by_a_dinov3_engine_in_the_same_process(precision):
    sd2 = random_state_dict("dinov2_vits14_reg", seed=2, image_size=70)
    bb = backbone.from_state_dict(sd2, heads=6, device=DEV, precision=precision)
    assert not bb.engine.rope and bb.engine._desc(2, 70, 70).rope is None
    x = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(8)).to(DEV)
    before = bb(x)[1].clone()
    _, sd3, x3, _ = g22("g46")
    make_engine("f16_resid32" if precision == "f16" else precision, sd3, 2)(x3.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bb(x)[1], before)
