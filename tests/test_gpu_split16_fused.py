"""GPU: fc1 -> activation -> fp16-term split in ONE launch (ucod_split16_gemm_act; the kSplit16 drains of csrc/gemm_bf16_epilogue.h) and the pass that uses it
(UCOD_SPLIT16_FUSE_MLP, SplitViTEngine(terms=2, term="f16", fuse_mlp=True), precision "split2hf").

The drain calls the activation and the split of ucod_split16_rows (gelu_exact / silu_f32 / split_pair, csrc/common.h) on the f32 value the unfused pair
(UCOD_EPI_BIAS_F32 + ucod_split16_rows) passes through memory, so wherever the two GEMMs sum K in one order the outputs are compared BIT FOR BIT; everything is also
measured against f64 with the unfused rows' bounds, and the engine against the unfused split2h engine and the three-term bf16 engine in the same test."""
import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N, ops, swiglu  # noqa: E402
from ucod_dpl_amd.vit_engine import SplitViTEngine  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import backbone  # noqa: E402
import split16_ref as R  # noqa: E402
from split16_ref import rel_l2  # noqa: E402
from test_gpu_split16 import FC1_SHAPES, relation, record, peaked  # noqa: E402,F401  (peaked: the module-scoped C2 fixture, instantiated again for this module)

DEV = "cuda"
S_LN, S_HID = 64.0, 16.0


def fused(xs, ws, bias_scaled, op, alpha, M, Nn, variant=0, guard=3):
    """ucod_split16_gemm_act into rows exactly 3 N (op 3: 3 N / 2) wide with `guard` rows of -7 behind the matrix."""
    width = 3 * Nn if op == 1 else 3 * Nn // 2
    out = torch.full((M + guard, width), -7.0, dtype=torch.float16, device=DEV)
    ops.gemm_act_split16(xs, ws, bias_scaled, op, alpha, S_HID, variant=variant, out=out)
    return out


def unfused(xs, ws, bias_scaled, op, alpha, M, Nn, variant=0, guard=3):
    """The pair the fused launch replaces: the f32 epilogue, then ucod_split16_rows."""
    K3 = xs.shape[1]
    f1 = torch.empty(M, Nn, dtype=torch.float32, device=DEV)
    ops._gemm_f16(N.EPI_BIAS_F32, xs, ws, f1, M, Nn, K3, bias=bias_scaled, variant=variant)
    Ko = Nn if op == 1 else Nn // 2
    out = torch.full((M + guard, 3 * Ko), -7.0, dtype=torch.float16, device=DEV)
    N.check(N.load("f16").ucod_split16_rows(N.ptr(f1), Nn, N.ptr(out), M, Ko, 0, op, alpha, S_HID, N.stream()), "ucod_split16_rows")
    return out


def value(out, M, Ko):
    """(hi + lo) / scale in f64, after the layout checks every row shares: hi | hi equal, lo the split of what hi leaves."""
    seg = out[:M].view(M, 3, Ko)
    assert torch.equal(seg[:, 0], seg[:, 1])
    hi, lo = seg[:, 0].float(), seg[:, 2].float()
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -24).all())
    return ((hi.double() + lo.double()) / S_HID).cpu()


def z_inputs(n, seed):
    """n draws from 1.2 N(0, 1) and what the scale-64 split keeps of them (22 bits: exact in f32)."""
    z = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 1.2
    hi, lo = R.split16(z, S_LN)
    return z, R.reconstruct(hi, lo, S_LN)


def test_gelu_accuracy_isolated_and_bit_equal_to_the_unfused_pair():
    """One-hot operands: x[m, 0] = z_m, w[n, 0] = 1, K = 128, bias 0 -- the accumulator is exactly S z~ and only the activation and the split contribute.
    rel-L2(fused) <= 2 rel-L2(unfused) + 2e-8, both against f64 (tests/test_split16_fused_host.py shows that the minimax GELU of the 16-bit drains misses this by 3x);
    the drain reuses gelu_exact, so the outputs are also the same bits."""
    M, Nn, K = 8220, 64, 128
    z, zt = z_inputs(M, 8220)
    x, w = torch.zeros(M, K), torch.zeros(Nn, K)
    x[:, 0], w[:, 0] = z, 1.0
    sw = ops.pow2_scale(w)
    S = S_LN * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=S_LN), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    bias = torch.zeros(Nn, device=DEV)
    ref = torch.nn.functional.gelu(zt)[:, None].expand(M, Nn)
    for variant in (0, 2, 12, 9, 13):
        a, b = fused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant), unfused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant)
        ef, eu = rel_l2(value(a, M, Nn), ref), rel_l2(value(b, M, Nn), ref)
        print(f"isolated GELU, variant {variant}: rel-L2 fused {ef:.3e}, unfused {eu:.3e}")
        record("split16_fused_gelu_isolated", dict(variant=variant, fused=ef, unfused=eu))
        assert ef <= 2 * eu + 2e-8, (variant, ef, eu)
        assert eu < 1.4e-7, eu                                       # (the host restatement's figure for the erf form)
        assert torch.equal(a, b), variant


def test_swiglu_accuracy_isolated_and_bit_equal_to_the_unfused_pair():
    """The same with x1 and x2 on two one-hot columns of the interleaved layout (GEMM column 8k + e is x1, 8k + 4 + e is x2 of hidden unit 4k + e)."""
    M, Nn, K = 8220, 128, 128
    (_, z1), (_, z2) = z_inputs(M, 1), z_inputs(M, 2)
    x, w = torch.zeros(M, K), torch.zeros(Nn, K)
    x[:, 0], x[:, 1] = z1.float(), z2.float()
    col = torch.arange(Nn)
    w[col % 8 < 4, 0] = 1.0
    w[col % 8 >= 4, 1] = 1.0
    sw = ops.pow2_scale(w)
    S = S_LN * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=S_LN), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    bias = torch.zeros(Nn, device=DEV)
    ref = (torch.nn.functional.silu(z1) * z2)[:, None].expand(M, Nn // 2)
    for variant in (0, 2, 12, 9, 13):
        a, b = fused(xs, ws, bias, 3, 1.0 / S, M, Nn, variant), unfused(xs, ws, bias, 3, 1.0 / S, M, Nn, variant)
        ef, eu = rel_l2(value(a, M, Nn // 2), ref), rel_l2(value(b, M, Nn // 2), ref)
        print(f"isolated SwiGLU, variant {variant}: rel-L2 fused {ef:.3e}, unfused {eu:.3e}")
        record("split16_fused_swiglu_isolated", dict(variant=variant, fused=ef, unfused=eu))
        assert ef <= 2 * eu + 2e-8, (variant, ef, eu)
        assert eu < 3e-7, eu                                         # (the row op's own bound, tests/test_gpu_split16.py)
        assert torch.equal(a, b), variant                            # (one nonzero product per sum: no summation order to differ in)


@pytest.mark.parametrize("M,Nn,K,variant", FC1_SHAPES)
def test_gelu_on_every_tile_path(M, Nn, K, variant):
    """The shapes of the unfused row (64 x 64, 128 x 128, one-shot large tiles 256 / 192 wide with their leftover patches, mixed-height; N a multiple of 192 or not).
    Output rows are exactly 3 N wide, so a store past column N lands in checked data or, behind the last row, in the guard rows.  Bound 2e-6: the unfused row's.
    GELU takes the leftover patches like the f32 epilogue, so the two sum K in the same order on every path: same bits."""
    g = torch.Generator().manual_seed(M + Nn)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05, torch.randn(Nn, generator=g) * 0.2
    ref = torch.nn.functional.gelu(x.double() @ w.double().t() + b.double())
    sw = ops.pow2_scale(w)
    S = S_LN * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=S_LN), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    bias = (b * S).to(DEV)
    out = fused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant)
    assert bool((out[M:] == -7.0).all())
    got = value(out, M, Nn)
    err = rel_l2(got, ref)
    print(f"fused fc1+GELU split2hf M={M} N={Nn} K={K} variant={variant}: rel-L2 {err:.3e}")
    record("split16_fused_fc1_gelu", dict(M=M, N=Nn, K=K, variant=variant, rel_l2=err))
    assert err < 2e-6, err
    assert maxdiff(got, ref) < 40 * 2e-6 * max(1.0, float(ref.abs().max()))
    assert torch.equal(out, unfused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant))


@pytest.mark.parametrize("M,Nn,K,variant", FC1_SHAPES)
def test_swiglu_on_every_tile_path(M, Nn, K, variant):
    """The same shapes with N read as the 2 F interleaved columns of weights_in.  Bound 3e-6: the linear row's 1e-6 on x2, and on x1 through SiLU's largest slope 1.1
    over the norm SiLU keeps of a centred input (~0.6) = 1.8e-6, added in quadrature (2.1e-6), with room for the f32 SiLU's 2e-7.  The unfused pair is measured beside
    it: err_fused <= 1.25 err_unfused + 1e-7 (SwiGLU has no leftover patches, so on the one-shot large tiles the two may sum K in different orders: not the same bits)."""
    g = torch.Generator().manual_seed(M + Nn + 1)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05, torch.randn(Nn, generator=g) * 0.2
    ref = swiglu.swiglu_interleaved(x.double() @ w.double().t() + b.double())
    sw = ops.pow2_scale(w)
    S = S_LN * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=S_LN), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    bias = (b * S).to(DEV)
    out = fused(xs, ws, bias, 3, 1.0 / S, M, Nn, variant)
    assert bool((out[M:] == -7.0).all())
    got = value(out, M, Nn // 2)
    err = rel_l2(got, ref)
    pair = (Nn // 2) % 8 == 0                                       # (ucod_split16_rows writes 8 output columns per thread: no unfused pair at N = 1000)
    eu = rel_l2(value(unfused(xs, ws, bias, 3, 1.0 / S, M, Nn, variant), M, Nn // 2), ref) if pair else float("nan")
    print(f"fused fc1+SwiGLU split2hf M={M} N={Nn} K={K} variant={variant}: rel-L2 {err:.3e} (unfused pair {eu:.3e})")
    record("split16_fused_fc1_swiglu", dict(M=M, N=Nn, K=K, variant=variant, rel_l2=err, unfused_rel_l2=eu))
    assert err < 3e-6, err
    assert not pair or err <= 1.25 * eu + 1e-7, (err, eu)
    assert maxdiff(got, ref) < 40 * 3e-6 * max(1.0, float(ref.abs().max()))


class own_counter:
    """The launches inside count into a word of this test's own (ucod_resid16_overflow_bind)."""

    def __init__(self):
        self.word = torch.zeros(1, dtype=torch.int32, device=DEV)

    def __enter__(self):
        N.check(N.load("f16").ucod_resid16_overflow_bind(self.word.data_ptr()), "bind")
        return self

    def __exit__(self, *exc):
        N.load("f16").ucod_resid16_overflow_bind(None)
        return False

    def take(self):
        torch.cuda.synchronize()
        n = int(self.word.item())
        self.word.zero_()
        return n


@pytest.mark.parametrize("M,Nn,variant", [(300, 256, 2), (300, 256, 12), (4111, 1000, 10), (4111, 1024, 9), (8220, 1024, 13), (8220, 1024, 14)])
def test_saturation_is_counted_exactly(M, Nn, variant):
    """Hidden values whose 16-fold exceeds 65 504 (one-hot operands, so the pre-activations are exact: 5 000 and 10 000 among draws from N(0, 1), all far from the
    edge 4 094): clamped, and the counter's increase equals the restatement's count -- dropped chunks (columns past N on the 192-wide tiles, rows past M) count nothing.
    A counted condition, not a fault."""
    K = 128
    z = torch.randn(M, generator=torch.Generator().manual_seed(M)) * 1.0
    z[::7], z[3::11], z[5::13] = 5000.0, 10000.0, -9000.0          # (GELU of -9000 is -0: not counted)
    sx = 4.0                                                       # 10 000 x 4 stays inside fp16's range on the way in
    hi, lo = R.split16(z, sx)
    zt = R.reconstruct(hi, lo, sx)
    x, w = torch.zeros(M, K), torch.zeros(Nn, K)
    x[:, 0], w[:, 0] = z, 1.0
    sw = ops.pow2_scale(w)
    S = sx * sw
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=sx), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    bias = torch.zeros(Nn, device=DEV)
    h = torch.nn.functional.gelu(zt).float()
    want = R.saturated(h, S_HID) * Nn
    assert want > 0
    with own_counter() as c:
        out = fused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant)
        got = c.take()
        ref_out = unfused(xs, ws, bias, 1, 1.0 / S, M, Nn, variant)
        got_unfused = c.take()
    assert got == want == got_unfused, (got, want, got_unfused)
    assert bool(torch.isfinite(out[:M].float()).all()) and bool((out[M:] == -7.0).all())
    assert torch.equal(out, ref_out)
    # SwiGLU: x1 = z (silu(z) = z for the large values), x2 = 1
    x[:, 1] = 1.0
    w.zero_()
    col = torch.arange(Nn)
    w[col % 8 < 4, 0] = 1.0
    w[col % 8 >= 4, 1] = 1.0
    xs, ws = ops.split_rows(x.to(DEV), 2, 0, term="f16", scale=sx), ops.split_rows(w.to(DEV), 2, 1, term="f16", scale=sw)
    want3 = R.saturated(torch.nn.functional.silu(zt).float(), S_HID) * (Nn // 2)
    with own_counter() as c:
        out3 = fused(xs, ws, bias, 3, 1.0 / S, M, Nn, variant)
        got3 = c.take()
    assert got3 == want3 > 0, (got3, want3)
    assert bool(torch.isfinite(out3[:M].float()).all()) and bool((out3[M:] == -7.0).all())


def test_refusals_on_the_device():
    xs = torch.zeros(64, 192, dtype=torch.float16, device=DEV)
    out = torch.zeros(64, 192, dtype=torch.float16, device=DEV)
    bias = torch.zeros(64, device=DEV)
    f, b = N.load("f16"), N.load("bf16")
    args = lambda op=1, Nn=64, alpha=1.0, scale=16.0, variant=0: (op, N.ptr(xs), N.ptr(xs), N.ptr(out), 64, Nn, 192, N.ptr(bias), alpha, scale, variant, N.stream())  # noqa: E731
    assert f.ucod_split16_gemm_act(*args()) == 0
    assert f.ucod_split16_gemm_act(*args(op=3)) == 0
    assert f.ucod_split16_gemm_act(*args(op=2)) == -1 and f.ucod_split16_gemm_act(*args(op=0)) == -1
    assert f.ucod_split16_gemm_act(*args(Nn=60)) == -1
    assert f.ucod_split16_gemm_act(*args(alpha=3.0)) == -1 and f.ucod_split16_gemm_act(*args(scale=12.0)) == -1
    assert f.ucod_split16_gemm_act(*args(variant=5)) == -1 and f.ucod_split16_gemm_act(*args(variant=15)) == -1      # laboratory / unknown variants
    assert b.ucod_split16_gemm_act(*args()) == -1                  # the bf16 library refuses
    for epi in (19, 20):                                           # the epilogues exist behind ucod_split16_gemm_act only
        assert f.ucod_gemm_bf16(epi, N.ptr(xs), N.ptr(xs), N.ptr(out), 64, 64, 192, N.ptr(bias), None, None, None, 0, 0, N.stream()) == -1
    torch.cuda.synchronize()


def engines(sd, heads):
    kw = dict(heads=heads, eps=1e-6, device=DEV)
    return SplitViTEngine(sd, terms=2, term="f16", fuse_mlp=True, **kw), SplitViTEngine(sd, terms=2, term="f16", **kw), SplitViTEngine(sd, terms=3, **kw)


def fused_bounds(ef, eu, e3):
    """The engine rows' relations: against the three-term engine (22 against 24 bits), and against the unfused fp16-term engine."""
    return relation(ef, e3) and ef <= 1.25 * eu + 1e-7


@pytest.mark.parametrize("name,heads", [("g8_dinov2_native", 2), ("g8_dinov2_interp", 2), ("g8_dinov1_native", 2), ("g8_dinov1_interp", 2)])
def test_fused_engine_against_reference_golden(name, heads):
    gd = load_golden(name)
    ef, eu, e3 = engines(sub(gd, "sd."), heads)
    assert ef.fuse_mlp and not eu.fuse_mlp and not e3.fuse_mlp and ef.half == "f16x2" and ef.term == "f16"
    x = gd["x"].to(DEV)
    key = ef(x).cpu()
    ef.check_overflow(wait=True)
    assert key.shape == gd["key"].shape
    errf, erru, err3 = rel_l2(key, gd["key"]), rel_l2(eu(x).cpu(), gd["key"]), rel_l2(e3(x).cpu(), gd["key"])
    print(f"{name}: key rel-L2 split2hf {errf:.3e}, split2h {erru:.3e}, split3 {err3:.3e}")
    record("split16_fused_golden", dict(name=name, split2hf=errf, split2h=erru, split3=err3))
    assert fused_bounds(errf, erru, err3), (errf, erru, err3)
    assert errf < 3e-6                                              # (the unfused row's absolute bound)
    # the fused pass needs less workspace, by at least the f32 fc1 buffer
    B, _, H, W = x.shape
    d = ef._desc(B, H, W)
    d.resid16 = d.ln_fold = d.full_last_layer = d.attn_variant = 0
    M = B * ((H // ef.P) * (W // ef.P) + 1)
    assert ef._ws_bytes(d) <= eu._ws_bytes(d) - M * ef.F * 4
    k1 = ef.forward(x, n_layers=1).cpu()                            # truncated passes and the asynchronous form work unchanged
    assert k1.shape == key.shape and not torch.equal(k1, key)
    k2, events = ef.forward_async(x)
    for e in events:
        torch.cuda.current_stream().wait_event(e)
    assert torch.equal(k2.cpu(), key)
    ef.check_overflow(wait=True)


@pytest.mark.parametrize("D,heads,L", [(128, 2, 3), (256, 4, 4)])
def test_fused_swiglu_engine_vs_restatement(D, heads, L):
    from swiglu_ref import random_swiglu_state_dict
    from test_gpu_swiglu import f64_key
    sd = random_swiglu_state_dict(D, heads, L, seed=D)
    img = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(5))
    _, ref, _ = f64_key(sd, img, heads, full_last_layer=False)
    ef, eu, e3 = engines(sd, heads)
    assert ef.mlp == N.UCOD_MLP_SWIGLU and ef.fuse_mlp
    key = ef(img.to(DEV))
    ef.check_overflow(wait=True)
    errf, erru, err3 = rel_l2(key, ref), rel_l2(eu(img.to(DEV)), ref), rel_l2(e3(img.to(DEV)), ref)
    print(f"SwiGLU D={D}: key rel-L2 split2hf {errf:.3e}, split2h {erru:.3e}, split3 {err3:.3e}")
    record("split16_fused_swiglu", dict(D=D, split2hf=errf, split2h=erru, split3=err3))
    assert fused_bounds(errf, erru, err3), (errf, erru, err3)


def test_c2_full_size_on_trained_like_weights(peaked):  # noqa: F811
    """ViT-B/14 at 518 x 518, full depth, trained-like weights: the fused engine against the f32 oracle, beside the unfused fp16-term engine and the three-term bf16
    engine on the same inputs; the unfused row's absolute bounds unchanged."""
    from test_gpu_parity_c2 import device_logits
    c = peaked
    img = c["img"].to(DEV)
    res = {}
    for name, eng in zip(("split2hf", "split2h", "split3"), engines(c["sd"], c["heads"])):
        key_dev = eng(img)
        eng.check_overflow(wait=True)
        assert bool(torch.isfinite(key_dev).all())
        fd = device_logits(key_dev, c["dec"], c["n"], c["D"])
        res[name] = dict(key_rel_l2=rel_l2(key_dev.cpu(), c["key"]), logit_max_abs=float((fd - c["fg"]).abs().max()), logit_rel_l2=rel_l2(fd, c["fg"]),
                         mask_flipped_fraction=float(((fd > 0) != (c["fg"] > 0)).float().mean()))
    print(f"c2 peaked: {res}")
    record("split16_fused_c2_peaked", res)
    a, u, b = res["split2hf"], res["split2h"], res["split3"]
    assert a["logit_max_abs"] <= 2e-4, a
    assert a["mask_flipped_fraction"] == 0.0
    for k in ("key_rel_l2", "logit_max_abs", "logit_rel_l2"):
        assert fused_bounds(a[k], u[k], b[k]), (k, a, u, b)


def test_key_map_does_not_depend_on_the_batch(peaked):  # noqa: F811
    c = peaked
    eng = SplitViTEngine(c["sd"], heads=c["heads"], eps=1e-6, device=DEV, terms=2, term="f16", fuse_mlp=True)
    img = torch.cat((c["img"], torch.randn(4, 3, 518, 518, generator=torch.Generator().manual_seed(5))), 0).to(DEV)
    k6 = eng(img).clone()
    k1 = eng(img[:1].contiguous())
    eng.check_overflow(wait=True)
    assert rel_l2(k1, k6[:1]) < 5e-6                             # other tile shapes = another f32 summation order, nothing else (the unfused row's bound)


def test_cls_attention_row():
    g = load_golden("g14_pseudo_label")
    x = g["x"].to(DEV)
    ref_att, kref = g["attn_cls"][:, :, 1:], g["key"][:, 1:, :]
    out = {}
    for name, eng in zip(("split2hf", "split2h", "split3"), engines(sub(g, "sd."), 2)):
        key, att = eng.forward_with_cls_attention(x)
        eng.check_overflow(wait=True)
        out[name] = (rel_l2(att, ref_att), rel_l2(key.cpu().flatten(2).transpose(1, 2), kref), att)
    print("CLS attention row / key rel-L2: " + ", ".join(f"{n} {v[0]:.3e} / {v[1]:.3e}" for n, v in out.items()))
    for i in (0, 1):
        assert fused_bounds(out["split2hf"][i], out["split2h"][i], out["split3"][i]), (i, out)
    assert out["split2hf"][0] < 2e-5 and out["split2hf"][1] < 5e-6      # (the unfused row's own bounds)
    assert maxdiff(out["split2hf"][2].sum(-1).cpu() + g["attn_cls"][:, :, 0], torch.ones(3, 2)) < 1e-5


def test_saturation_in_the_fused_engine_raises():
    """A pass whose hidden activations exceed the HIDDEN class's bound (4 094): the drain clamps and counts, check_overflow raises, the next clean pass does not."""
    gd = load_golden("g8_dinov2_native")
    sd = {k: v.clone() for k, v in sub(gd, "sd.").items()}
    eng = SplitViTEngine(sd, heads=2, eps=1e-6, device=DEV, terms=2, term="f16", fuse_mlp=True)
    x = gd["x"].to(DEV)
    good = eng(x).clone()
    eng.check_overflow(wait=True)
    hot = [k for k in sd if k.endswith("mlp.fc1.bias") or k.endswith("intermediate.dense.bias")]
    assert hot
    sd[hot[0]] = sd[hot[0]].clone()
    sd[hot[0]][:8] = 6000.0                                        # GELU(6000 + ...) x 16 > 65 504, while 6000 x S_fc1 stays a finite f32 bias
    bad = SplitViTEngine(sd, heads=2, eps=1e-6, device=DEV, terms=2, term="f16", fuse_mlp=True)
    key = bad(x)
    assert bool(torch.isfinite(key).all())                          # clamped, never inf / NaN
    with pytest.raises(FloatingPointError, match="split2hf"):
        bad.check_overflow(wait=True)
    assert torch.equal(eng(x), good)                                # the clean engine on the same device saw nothing
    eng.check_overflow(wait=True)


def test_precision_name_on_the_public_surface(tmp_path):
    """precision="split2hf" through backbone / with_precision / build_feature_cache / PseudoLabelGenerator / WindowFeatures; "split2h" on the same object still builds
    the unfused engine and "f32eq" the three-term one."""
    from ucod_dpl_amd.data.datasets import MultiCacheManager, build_feature_cache
    from ucod_dpl_amd.generate_pseudo_label import PseudoLabelGenerator
    from ucod_dpl_amd.engine.runner.loop_CORAL import WindowFeatures
    import inspect
    gd = load_golden("g8_dinov2_native")
    bb = backbone.from_state_dict(sub(gd, "sd."), heads=2, device=DEV)
    hf = bb.with_precision("split2hf")
    assert isinstance(hf.engine, SplitViTEngine) and hf.engine.term == "f16" and hf.engine.terms == 2 and hf.engine.fuse_mlp is True and hf.precision == "split2hf"
    assert bb.with_precision("split2hf") is hf and hf.with_precision("split2hf") is hf
    h = bb.with_precision("split2h")
    assert h is not hf and h.engine.term == "f16" and h.engine.fuse_mlp is False
    eq = bb.with_precision("f32eq")
    assert eq.engine.terms == 3 and eq.engine.term == "bf16" and eq.engine.fuse_mlp is False
    direct = backbone.from_state_dict(sub(gd, "sd."), heads=2, device=DEV, precision="split2hf")
    assert direct.engine.fuse_mlp is True and direct.precision == "split2hf"
    x = gd["x"]
    _, key = direct(x.to(DEV))
    assert rel_l2(key, gd["key"]) < 3e-6
    fc = MultiCacheManager(str(tmp_path), "dinov2", "val", "T").get_features_cache()
    assert build_feature_cache([x[i] for i in range(x.shape[0])], bb, fc, batch_size=2, device=DEV, precision="split2hf") == x.shape[0]
    for i in range(x.shape[0]):
        assert rel_l2(fc.read_file(i), gd["key"][i]) < 3e-6
    gen = PseudoLabelGenerator(bb, th_bkg=0.6, precision="split2hf")
    assert gen.engine is hf.engine
    assert PseudoLabelGenerator(bb, th_bkg=0.6).engine.terms == 3                   # defaults unchanged
    assert inspect.signature(WindowFeatures.__init__).parameters["precision"].default == "f32eq"
    assert inspect.signature(build_feature_cache).parameters["precision"].default == "f32eq"

    class _NoLoop:                                                 # WindowFeatures only keeps the loop object at construction
        pass
    wf = WindowFeatures(bb, _NoLoop(), window_size=3, grid=(56, 56), extractor_size=(84, 84), image_size=(56, 56), precision="split2hf")
    assert wf.fe is hf
