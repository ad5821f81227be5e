"""GPU: backbone-backward (LoRA) mode on DINOv3 ViT checkpoints -- the rotary embedding in both passes.

1  ucod_rope_qk_ld (csrc/rope.hip) in both libraries on fp16 / bf16 / f32 buffers with row pitch 3 D and 3 D + 64: the forward direction at pitch 3 D is ucod_rope_qk
   bit for bit; the transposed direction meets the criterion of tests/test_gpu_dinov3.py's kernel test against the f64 formula on the stored values,
   |got - ref| <= u |ref| + 4 * 2^-24 (|a cos| + |b sin|) (+ 2^-25 for fp16); as CONDITIONS the V third, every CLS / register row, every column at or beyond 3 D
   and the guard bands are bit for bit the pattern they were filled with; on f32 buffers <R x, y> = <x, R^T y> to 1e-6 relative; the refusals.
2  ViTLoRAEngine(allow_rope=True) against the G23 goldens (transformers' own f64 key map and LoRA gradients, tests/golden/make_golden_dinov3_lora.py): the key map
   under dinov3_ref.engine_bound("bf16", z) = 3 x transformers under bf16 autocast, which lies under half the smallest forward fault; every non-zero gradient under
   dinov3_lora_ref.grad_bar = max(4e-2 (5e-2 with dropout), 3 x that tensor's error under bf16 autocast), which tests/test_dinov3_lora_host.py shows to lie at
   least twice under what any fault of the backward rotation does to the q / k gradients of a rotating layer; structural zeros exact; two runs bit-identical.
   With dropout or a target subset the reference is the f64 restatement tests/dinov3_lora_ref.py (pinned on the goldens) with the engine's masks per chunk.
3  forward_nograd, clone_for_ema, merged_state_dict -> SplitViTEngine, merge_into, the adapter folder, the refusals, and a DINOv2 engine untouched by the flag.

Measured on an MI355X (conftest.within leaves every bounded figure in its tolerance audit file): key map against G23 2.9e-3 (g46; bound 1.13e-2) / 3.1 - 3.2e-3 (d256;
1.21e-2); worst gradient in units of its bar 0.32 - 0.39 (g46: 1.3 - 1.9e-2 of 4.0 - 5.0e-2) and 0.35 - 0.43 (d256: 2.1 - 2.6e-2 of 6.05e-2), gated MLP 1.4e-2 of 4e-2;
forward_nograd against forward_train 1.5e-3 (f32 stream) / 2.1e-5 (fp16 stream, the engine's own); merged split3 engine 4.3e-7 from transformers' f64 key map
(bound 2.2e-6; unmerged 5.1e-2).  The whole module runs in under 3 s.
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
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, ViTLoRAEngine, rope_table  # noqa: E402
from ucod_dpl_amd.models.modules import full_model as M  # noqa: E402
from oracle import vit as OV  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402
import registers_ref as RR  # noqa: E402

DEV = "cuda"
GUARD = 4096
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ELEM = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8), "f32": (torch.float32, 0.0)}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ================================================================================================ 1. the kernel
def pattern(B, tok, ld, dtype, seed):
    """[B, tok, ld] of N(0, 1) (every seventh token row times 2^-16: subnormal fp16 results) between two guard bands of further N(0, 1) values: everything the kernel
    must leave alone holds a pattern, not a constant."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(2 * GUARD + B * tok * ld, generator=g)
    full[GUARD:GUARD + B * tok * ld].view(B, tok, ld)[:, ::7] *= 2.0 ** -16
    return full.to(dtype)


def run_ld(lib, host, elem, table, B, tok, R, heads, ld, inverse):
    buf = host.to(DEV)
    payload = buf[GUARD:GUARD + B * tok * ld]
    rc = lib.ucod_rope_qk_ld(payload.data_ptr(), N.ROPE_ELEM_F32 if elem == "f32" else N.ROPE_ELEM_HALF, N.ptr(table), B, tok, R, heads, ld, inverse, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf.cpu()


def rotate_ref(v, table, inverse):
    """f64 rotation of v [B, n, 2 heads, 64] (the stored values) and the magnitude sum of its two products"""
    a, b = v[..., :32], v[..., 32:]
    c, s = table[:, None, :32].double(), table[:, None, 32:].double() * (-1.0 if inverse else 1.0)
    return torch.cat((a * c - b * s, b * c + a * s), -1), torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), -1)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("R", [0, 4])
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("lib_half,elem", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32")])
def test_rope_ld_kernel(lib_half, elem, heads, R, pad):
    lib = N.load(lib_half)
    dtype, u = ELEM[elem]
    B, gh, gw = 2, 4, 6
    n, D = gh * gw, 64 * heads
    tok, ld = 1 + R + n, 3 * D + pad
    table = rope_table(gh, gw)
    tdev = table.to(DEV)
    host = pattern(B, tok, ld, dtype, 100 * heads + 10 * R + pad)
    x = host[GUARD:GUARD + B * tok * ld].view(B, tok, ld)
    name = f"rope_ld {lib_half}:{elem} heads={heads} R={R} ld=3D+{pad}"

    def untouched(out):
        got = out[GUARD:GUARD + B * tok * ld].view(B, tok, ld)
        assert torch.equal(bits(out[:GUARD]), bits(host[:GUARD])) and torch.equal(bits(out[GUARD + B * tok * ld:]), bits(host[GUARD + B * tok * ld:])), "wrote outside the buffer"
        assert torch.equal(bits(got[:, :, 2 * D:]), bits(x[:, :, 2 * D:])), "the V third or a column at or beyond 3 D changed"
        assert torch.equal(bits(got[:, :1 + R]), bits(x[:, :1 + R])), "a CLS or register row changed"
        return got

    # forward direction: at pitch 3 D the existing entry point bit for bit; at any pitch the same values in the first 2 D columns
    fwd = untouched(run_ld(lib, host, elem, tdev, B, tok, R, heads, ld, 0))
    dense = x[:, :, :3 * D].contiguous().to(DEV)
    assert lib.ucod_rope_qk(N.ptr(dense), N.ROPE_ELEM_F32 if elem == "f32" else N.ROPE_ELEM_HALF, N.ptr(tdev), B, tok, R, heads, N.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(fwd[:, :, :3 * D].contiguous()), bits(dense.cpu())), "inverse = 0 is not ucod_rope_qk"
    # transposed direction against the f64 formula rounded once
    inv = untouched(run_ld(lib, host, elem, tdev, B, tok, R, heads, ld, 1))
    v = x[:, 1 + R:, :2 * D].double().reshape(B, n, 2 * heads, 64)
    ref, mag = rotate_ref(v, table, inverse=True)
    bound = u * ref.abs() + 4 * 2.0 ** -24 * mag + (2.0 ** -25 if elem == "f16" else 0.0)
    got = inv[:, 1 + R:, :2 * D].double().reshape(B, n, 2 * heads, 64)
    err = (got - ref).abs()
    if elem == "f16":
        assert bool(((ref.abs() < 2.0 ** -14) & (ref != 0)).any()), "the case holds no subnormal fp16 result"
    assert bool((err[bound == 0] == 0).all())
    assert float(ref.abs().max()) > 1.0 and float((got - v).abs().max()) > 0.1, "nothing was rotated"
    # (the directions differ: the transposed result is not the forward one)
    assert float((got - fwd[:, 1 + R:, :2 * D].double().reshape(B, n, 2 * heads, 64)).abs().max()) > 0.1
    within(name, float((err / bound.clamp_min(1e-300)).max()), 1.0 + 1e-12)
    if elem == "f32":
        # the adjoint identity <R x, y> = <x, R^T y>, both rotations by the kernel; y = R x (f64) + N(0, 1), so that the product is far from zero
        g = torch.Generator().manual_seed(7)
        yhost = host.clone()
        yv = yhost[GUARD:GUARD + B * tok * ld].view(B, tok, ld)
        yv[:, 1 + R:, :2 * D] = (rotate_ref(v, table, inverse=False)[0] + torch.randn(B, n, 2 * heads, 64, generator=g, dtype=torch.float64)).reshape(B, n, 2 * D).float()
        rty = run_ld(lib, yhost, elem, tdev, B, tok, R, heads, ld, 1)[GUARD:GUARD + B * tok * ld].view(B, tok, ld)
        lhs = float((fwd[:, 1 + R:, :2 * D].double() * yv[:, 1 + R:, :2 * D].double()).sum())
        rhs = float((x[:, 1 + R:, :2 * D].double() * rty[:, 1 + R:, :2 * D].double()).sum())
        assert abs(lhs) > 100.0
        within(name + " adjoint", abs(lhs - rhs) / abs(lhs), 1e-6)


def test_rope_ld_refuses_nonsense_without_writing():
    lib = N.load("bf16")
    B, tok, R, heads, ld = 2, 10, 4, 2, 448
    host = pattern(B, tok, ld, torch.bfloat16, 3)
    buf = host.to(DEV)
    p = buf[GUARD:].data_ptr()
    t = rope_table(1, 5).to(DEV)
    call = lambda q=p, elem=0, tab=None, B=B, tok=tok, R=R, heads=heads, ld=ld, inv=1: lib.ucod_rope_qk_ld(q, elem, N.ptr(t) if tab is None else tab, B, tok, R, heads, ld, inv, N.stream())  # noqa: E731
    assert call(ld=383) == -1 and call(ld=320) == -1              # ld < 3 D
    assert call(ld=388) == -1 and call(ld=390, elem=1) == -1       # rows off the 16-byte grid
    assert call(R=9) == -1 and call(R=12) == -1 and call(tok=5) == -1      # n_reg >= tok - 1
    assert call(q=p + 2) == -1 and call(tab=t.data_ptr() + 4) == -1 and call(inv=2) == -1 and call(elem=2) == -1 and call(B=0) == -1 and call(heads=0) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(buf.cpu()), bits(host))


# ================================================================================================ 2. the engine against G23
@functools.lru_cache(maxsize=None)
def g23(tag):
    z = np.load(os.path.join(GOLDEN, f"g23_dinov3_lora_{tag}.npz"))
    # (weights, inputs and LoRA matrices against the file: tests/test_dinov3_lora_host.py)
    lora = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/")}
    return z, R3.g22_state_dict(tag), lora, torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])


TARGET_SETS = {"default": None, "qv": ["q_proj", "v_proj"]}


def subset(lora, tset):
    t = TARGET_SETS[tset]
    return dict(lora) if t is None else {k: v for k, v in lora.items() if k.split(".")[4] in t}


def lora_engine(sd, heads, lora, targets=None, **kw):
    eng = ViTLoRAEngine(sd, heads=heads, r=RL.G23_R, lora_alpha=RL.G23_ALPHA, eps=1e-5, device=DEV, generator=torch.Generator().manual_seed(3), target_modules=targets,
                        allow_rope=True, **kw)
    assert sorted(eng.lora_state_dict()) == sorted(lora)
    eng.load_lora_state_dict(lora)
    return eng


def reference(tag, sd, lora, x, dkey, heads, bounds, seeds, p_drop, tok, D):
    """(key, gradients) of the f64 restatement, chunk by chunk with the engine's masks (each chunk has its own; gradients add)"""
    key_ref, gref = [], None
    for (b0, b1), seed in zip(bounds, seeds):
        masks = None
        if p_drop > 0:
            rows = (b1 - b0) * tok
            masks = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(R3.G22_LAYERS) for pi, nm in enumerate(RL.QKV)}
        k, g = RL.lora_grads(x[b0:b1], {**sd, **lora}, heads, dkey[b0:b1], RL.G23_SCALE, masks=masks, device=DEV)
        key_ref.append(k.cpu())
        gref = {n: v.cpu() for n, v in g.items()} if gref is None else {n: gref[n] + v.cpu() for n, v in g.items()}
    return torch.cat(key_ref, 0), gref


def check_passes(name, make, ref_of, x, dkey, key_bound, bar_of):
    """``make()`` builds the engine; ``ref_of(bounds, seeds)`` -> (key, gradients) of the reference for the chunks and dropout seeds the engine's step used."""
    eng = make()
    key = eng.forward_train(x.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    key_ref, gref = ref_of(list(eng._bounds), list(eng._chunk_seed))
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    assert sorted(got) == sorted(gref)
    key_err = rel_l2(key, key_ref)
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=lambda k: errs[k] / bar_of(k))
    print(f"{name}: key rel-L2 {key_err:.3e} (bound {key_bound:.2e}); worst gradient {errs[worst]:.3e} of bar {bar_of(worst):.2e} ({worst}); "
          f"largest {max(errs.values()):.3e}")
    within(name + " key", key_err, key_bound)
    for k, ref in gref.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    assert len(errs) > 0
    for k, e in errs.items():
        within(f"{name} {k}", e, bar_of(k))
    # two backward runs are bit-identical
    eng2 = make()
    eng2.forward_train(x.to(DEV))
    assert torch.equal(eng2.backward(dkey.to(DEV)), eng.lora_grad)
    return key


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tset", list(TARGET_SETS))
@pytest.mark.parametrize("tag", RL.G23_TAGS)
def test_lora_passes_on_dinov3_vs_f64_autograd(tag, tset, p_drop, streams):
    z, sd, lora_all, x, dkey = g23(tag)
    m = R3.G22[tag]
    lora = subset(lora_all, tset)
    tok = 1 + m["R"] + m["grid"][0] * m["grid"][1]

    def make():
        e = lora_engine(sd, m["heads"], lora, TARGET_SETS[tset], lora_dropout=p_drop, seed=1234)
        e.train_streams = streams
        return e

    eng = make()
    assert eng.rope and eng.allow_rope and eng.R == m["R"] and eng.targets == (True, tset == "default", True)
    t = eng._train_desc(2, x.shape[2], x.shape[3], 0)
    assert t.allow_rope == 1 and t.vit.rope == eng._rope(*m["grid"]).data_ptr()
    key_bound = R3.engine_bound("bf16", z)
    assert key_bound < 0.5 * min(float(z["fault_" + f]) for f in R3.FAULTS)      # a pass that rotates wrongly cannot stay inside
    if tset == "default" and p_drop == 0:                         # transformers' own f64 values
        ref_of = lambda bounds, seeds: (torch.from_numpy(z["key"]), {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad/")})  # noqa: E731
    else:                                                         # the restatement, with the masks of the engine's own step
        ref_of = lambda bounds, seeds: reference(tag, sd, lora, x, dkey, m["heads"], bounds, seeds, p_drop, tok, m["D"])  # noqa: E731
    check_passes(f"g23 {tag} {tset} p={p_drop} streams={streams}", make, ref_of, x, dkey, key_bound, lambda k: RL.grad_bar(z, k, p_drop))


def test_lora_passes_on_the_gated_mlp():
    """DINOv3 with the gated MLP (vits16plus / vith16plus; the G22 ``gated`` model) through the SwiGLU backward, against the restatement only (no golden holds its
    gradients): the project's bars, 4e-2 per gradient; the key map under 3 x transformers' bf16-autocast error of the G22 golden of the same model."""
    z22 = np.load(os.path.join(GOLDEN, "g22_dinov3_gated.npz"))
    sd, lora = R3.g22_state_dict("gated"), RL.g23_lora("gated")
    x, dkey = RL.g23_inputs("gated", seed=29)

    def make():
        e = lora_engine(sd, 2, lora, allow_swiglu=True)
        e.train_streams = 2
        return e

    with pytest.raises(NotImplementedError, match="allow_swiglu=True"):
        ViTLoRAEngine(sd, heads=2, eps=1e-5, device=DEV, allow_rope=True)
    eng = make()
    assert eng.mlp == N.UCOD_MLP_SWIGLU and eng.rope and eng.F == 384

    def ref_of(bounds, seeds):
        key_ref, gref = RL.lora_grads(x, {**sd, **lora}, 2, dkey, RL.G23_SCALE, device=DEV)
        return key_ref.cpu(), {k: v.cpu() for k, v in gref.items()}

    check_passes("g23 gated", make, ref_of, x, dkey, R3.engine_bound("bf16", z22), lambda k: 4e-2)


# ================================================================================================ 3. the rest of the surface
def test_nograd_ema_clone_merges_and_the_adapter_folder(tmp_path):
    z, sd, lora, x, dkey = g23("g46")
    eng = lora_engine(sd, 2, lora)
    xd = x.to(DEV)
    k_train = eng.forward_train(xd).clone()
    k_f16, k_f32 = eng.forward_nograd(xd, resid16=True).clone(), eng.forward_nograd(xd, resid16=False).clone()
    eng.check_overflow(wait=True)
    print(f"forward_nograd vs forward_train: f32 stream {rel_l2(k_f32, k_train):.2e}, fp16 stream {rel_l2(k_f16, k_train):.2e}")
    assert rel_l2(k_f32, k_train) < 2e-3 and rel_l2(k_f16, k_train) < 4e-3        # tests/test_gpu_lora_targets.py test 6
    within("g23 g46 forward_nograd key", rel_l2(k_f32, torch.from_numpy(z["key"])), R3.engine_bound("bf16", z))
    ema = eng.clone_for_ema()
    assert ema.rope and ema.allow_rope and ema._rope_cache is eng._rope_cache and ema._rope(4, 6).data_ptr() == eng._rope(4, 6).data_ptr()
    assert torch.equal(ema.forward_nograd(xd, resid16=False), k_f32) and torch.equal(ema.forward_train(xd), k_train)
    # merged_state_dict -> SplitViTEngine(terms=3): the golden's f64 key map (LoRA in transformers' own graph) within the f32-equivalent bound
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd) and not any(".lora_" in k for k in merged) and not any(k.endswith("k_proj.bias") for k in merged)
    changed = sorted(k for k in sd if not torch.equal(merged[k].cpu(), sd[k]))
    assert changed == sorted(f"model.layer.{i}.attention.{nm}.weight" for i in range(3) for nm in RL.QKV)
    key_ref = torch.from_numpy(z["key"])
    e_merged = rel_l2(SplitViTEngine(merged, heads=2, eps=1e-5, device=DEV, terms=3)(xd), key_ref)
    e_base = rel_l2(SplitViTEngine(sd, heads=2, eps=1e-5, device=DEV, terms=3)(xd), key_ref)
    bound = 4.0 * float(z["err_f32"]) + 1e-7
    print(f"merged DINOv3 engine (split3): {e_merged:.2e} (bound {bound:.2e}; unmerged {e_base:.2e})")
    within("g23 g46 merged split3", e_merged, bound)
    assert e_base > 100 * e_merged
    # merge_into a live default engine == rebuilding it (D = 128: no fold; the plain tables tensor for tensor)
    vit = ViTEngine(sd, heads=2, eps=1e-5, device=DEV)
    ptrs = [t.data_ptr() for row in vit.layers for t in row if t is not None]
    assert eng.merge_into(vit) is vit
    fresh = ViTEngine(merged, heads=2, eps=1e-5, device=DEV)
    for ra, rb in zip(vit.layers, fresh.layers):
        for a, b in zip(ra, rb):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    assert ptrs == [t.data_ptr() for row in vit.layers for t in row if t is not None]
    assert torch.equal(vit(xd), fresh(xd))
    with pytest.raises(ValueError, match="rotary"):
        eng.merge_into(ViTEngine(RR.g21_state_dict("native"), heads=2, device=DEV))
    # LoRABackbone.merge_and_unload: the frozen backbone of the adapted model, the checkpoint's eps and theta handed on
    bb = M.LoRABackbone(eng).merge_and_unload(precision="split3")
    assert bb.engine.rope and bb.engine.eps == 1e-5 and bb.engine.rope_theta == 100.0
    within("g23 g46 merge_and_unload split3", rel_l2(bb(xd)[1], key_ref), bound)
    # the adapter folder: names, config, and a bit-exact round trip into a second engine
    M.save_lora_adapter(eng, str(tmp_path))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / M.ADAPTER_WEIGHTS))
    assert sorted(saved) == sorted("base_model.model.ViT." + k for k in lora)
    assert json.loads((tmp_path / M.ADAPTER_CONFIG).read_text())["target_modules"] == ["q_proj", "k_proj", "v_proj"]
    other = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, allow_rope=True, generator=torch.Generator().manual_seed(9))
    assert not torch.equal(other.lora, eng.lora)
    M.load_lora_adapter(other, str(tmp_path))
    assert torch.equal(other.lora, eng.lora) and torch.equal(other.forward_train(xd), k_train)
    qv = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, allow_rope=True, target_modules=["q_proj", "v_proj"])
    with pytest.raises(ValueError, match="target_modules"):
        M.load_lora_adapter(qv, str(tmp_path))


def test_full_model_trains_through_load_lora():
    """load_lora with the build-only key, LoRABackbone and autograd: one differentiable pass gives the engine's gradients in ``lora.grad``; eps defaults to 1e-5."""
    from ucod_dpl_amd.engine.config import CfgNode
    z, sd, lora, x, dkey = g23("g46")
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        M.load_lora(CfgNode(dict(r=2, lora_alpha=4)), sd, 2, device=DEV)
    bb = M.load_lora(CfgNode(dict(r=2, lora_alpha=4, lora_dropout=0.0, allow_rope=True)), sd, 2, device=DEV)
    assert bb.engine.eps == 1e-5 and bb.engine.rope_theta == 100.0 and bb.engine.allow_rope
    assert M.load_lora(CfgNode(dict(r=2, lora_alpha=4, allow_rope=True, rope_theta=37.0)), sd, 2, device=DEV, eps=1e-6).engine.rope_theta == 37.0
    bb.engine.load_lora_state_dict(lora)
    key = bb(x.to(DEV))
    assert key.requires_grad
    (key * dkey.to(DEV)).sum().backward()
    got = bb.lora.grad
    assert tuple(got.shape) == tuple(bb.engine.lora.shape) and torch.equal(got, bb.engine.lora_grad)
    sa, _ = bb.engine._slices(1)
    ref = torch.from_numpy(z["grad/model.layer.0.attention.k_proj.lora_A.weight"])
    within("g23 g46 autograd k_proj A", rel_l2(got[0, sa].reshape(2, 128), ref), RL.grad_bar(z, "model.layer.0.attention.k_proj.lora_A.weight"))


def test_refusals_and_the_flag_without_a_table():
    z, sd, lora, x, dkey = g23("g46")
    with pytest.raises(NotImplementedError, match=r"DINOv3.*RoPE.*allow_rope=True$"):
        ViTLoRAEngine(sd, heads=2, eps=1e-5, device=DEV)
    eng = lora_engine(sd, 2, lora)
    with pytest.raises(NotImplementedError, match="DINOv3.*RoPE"):
        eng.forward_with_cls_attention(x.to(DEV))
    # the drivers: a table without the flag is refused by the size helpers and by the passes (before any launch), with it they run
    libb = N.load("bf16")
    t = eng._train_desc(3, 64, 96, 0)
    T, TT, TM, keep = eng._tables(4, 6, torch.zeros_like(eng.lora))
    need = libb.ucod_vit_train_workspace_bytes(C.byref(t))
    assert need > 0 and libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    key = torch.full((3, 128, 4, 6), -7.0, device=DEV)
    t.allow_rope = 0
    assert libb.ucod_vit_train_workspace_bytes(C.byref(t)) == 0 and libb.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) == 0
    xd = x.to(DEV)
    assert libb.ucod_vit_forward_train(C.byref(t), T, TT, N.ptr(xd), N.ptr(key), N.ptr(ws), ws.numel(), N.stream()) == -1
    assert libb.ucod_vit_forward_lora_infer(C.byref(t), T, TT, N.ptr(xd), N.ptr(key), N.ptr(ws), ws.numel(), N.stream()) == -1
    assert libb.ucod_vit_backward(C.byref(t), T, TT, N.ptr(dkey.to(DEV)), N.ptr(ws), ws.numel(), N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((key == -7.0).all()) and not bool(ws.any())
    # the plan does not change with a table
    t.allow_rope, rope = 1, t.vit.rope
    t.vit.rope = None
    assert libb.ucod_vit_train_workspace_bytes(C.byref(t)) == need
    t.vit.rope = rope
    # a DINOv2 engine (no table): the flag changes no bit of either pass
    sd2 = RR.g21_state_dict("native")
    gen = torch.Generator().manual_seed(7)
    img, dk = torch.randn(3, 3, 70, 70, generator=gen).to(DEV), torch.randn(3, 128, 5, 5, generator=gen).to(DEV)
    outs = []
    for flag in (False, True):
        e2 = ViTLoRAEngine(sd2, heads=2, device=DEV, generator=torch.Generator().manual_seed(3), lora_dropout=0.05, seed=5, allow_rope=flag)
        lsd = e2.lora_state_dict()
        e2.load_lora_state_dict({k: (0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(11)) if "lora_B" in k else v) for k, v in lsd.items()})
        assert not e2.rope and e2._train_desc(3, 70, 70, 0).allow_rope == int(flag) and e2._train_desc(3, 70, 70, 0).vit.rope is None
        k2 = e2.forward_train(img).clone()
        outs.append((k2, e2.backward(dk).clone(), e2.forward_nograd(img).clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
