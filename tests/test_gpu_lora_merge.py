"""GPU: the way out of LoRA mode -- merging the trained matrices into ordinary weights (peft's merge_and_unload: W + alpha/r B A on the modules
models/modules/full_model.py:47-72 wraps), refreshing a live engine in place, adapter files, and the runner's checkpoint / validation in backbone-backward mode.

1    ucod_lora_merge_f32 against the f64 helper (tests/lora_merge_ref.py, pinned on the CPU by tests/test_lora_merge_host.py), canary rows behind the output.
     Observed on MI355X: bit for bit (the kernel keeps w0 + scaling * sum as a multiply and an add; no one-ulp allowance is used).
2    ucod_fold_ln_linear against fold.fold_layernorm_linear on the same f32 inputs: weights and column sums bit for bit, the folded bias within one f32 ulp plus
     1e-12 * |q| sum_k |w beta| (the order of the f64 additions, where the sum cancels).
3    whole model: engines built from merged_state_dict() against the f64 LoRA forward (tests/lora_targets_ref.py), at the bars the existing engine tests use.
4    merge_into: the refreshed engine equals a fresh one built from the merged state dict, tensor for tensor; no reallocation, no drift.
5    merge_and_unload, save_lora_adapter / load_lora_adapter, and StandardRunner.save_checkpoint / val_feature_extractor.

Measured on MI355X (the `lora_merge_engines` / `lora_merge_refresh` rows tests 3 and 4 record): merged GELU D = 128 split3 4.8e-7 (bar 3e-6; the unmerged base
3.5e-1), bf16 2.9e-3 (6e-3), default 3.5e-4 (1e-3); merged SwiGLU D = 128 split3 5.0e-7 (bar 5e-6; unmerged 1.5e-2); refreshed folded engine at D = 256 6.4e-4
(GELU) / 5.5e-4 (SwiGLU) against the f64 LoRA forward, bit-identical to the fresh engine's key map, folded biases 0 ulp from the host's in every case.
"""
import functools
import json
import os

import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.fold import fold_layernorm_linear  # noqa: E402
from ucod_dpl_amd.vit_engine import SplitViTEngine, ViTEngine  # noqa: E402
import lora_merge_ref as M  # noqa: E402
import lora_targets_ref as R  # noqa: E402
from test_gpu_lora_targets import Guarded, checkpoint, record, rel_l2, targeted_engine  # noqa: E402

DEV = "cuda"
EINVAL = -1
P = N.ptr


def dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ------------------------------------------------------------------------------------------------ 1. the merge kernel
MERGE_SHAPES = [(37, 128, 2), (300, 768, 1), (64, 1536, 8), (770, 256, 21)]


@functools.lru_cache(maxsize=None)
def merge_operands(n, k, r):
    """f32 operands of one shape and the helper's result (computed once, never modified)."""
    g = torch.Generator().manual_seed(n + k + r)
    w0, A, B = 0.02 * torch.randn(n, k, generator=g), (torch.rand(r, k, generator=g) * 2 - 1) / k ** 0.5, 0.05 * torch.randn(n, r, generator=g)
    scaling = 4.0 / r
    return w0, A, B, scaling, M.merge(w0, A, B, scaling)


def run_merge(lib, w0, A, B, r, scaling, n, k):
    out = Guarded(n, k, torch.float32)
    rc = lib.ucod_lora_merge_f32(P(w0), P(A), P(B), r, scaling, out.ptr(), n, k, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside its output"
    got = out.payload.cpu()
    assert bool(torch.isfinite(got).all()), "left elements unwritten"
    return got


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("n,k,r", MERGE_SHAPES)
def test_lora_merge_f32(n, k, r, half):
    lib = N.load(half)
    w0, A, B, scaling, ref = merge_operands(n, k, r)
    w0d, Ad, Bd = dev(w0, A, B)
    got = run_merge(lib, w0d, Ad, Bd, r, scaling, n, k)
    again = run_merge(lib, w0d, Ad, Bd, r, scaling, n, k)
    assert torch.equal(got, again), "two runs differ"
    ulp = (torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs())
    worst = float(((got - ref).abs() / ulp).max())
    print(f"lora_merge_f32 {(n, k, r)} {half}: worst |got - ref| = {worst:.1f} ulp; |ref - w0| max {float((ref - w0).abs().max()):.2e}")
    assert torch.equal(got, ref), f"{worst} ulp from the f64 helper"
    assert float((ref - w0).abs().max()) > 1e-4                  # the update is not lost in the rounding
    assert torch.equal(run_merge(lib, w0d, Ad, torch.zeros_like(Bd), r, scaling, n, k), w0), "B = 0 must return the base weight"
    assert torch.equal(run_merge(lib, w0d, Ad, Bd, r, 0.0, n, k), w0), "scaling = 0 must return the base weight"


def test_lora_merge_refusals_leave_the_output_untouched():
    n, k, r = 37, 128, 2
    w0, A, B, scaling, _ = merge_operands(n, k, r)
    w0d, Ad, Bd = dev(w0, A, B)
    A22 = torch.zeros(22, k, device=DEV)
    B22 = torch.zeros(n, 22, device=DEV)
    out = torch.full((n, k), 3.0, device=DEV)
    st = N.stream()
    for lib in (N.load(), N.load("f16")):
        calls = {
            "null w0": lambda: lib.ucod_lora_merge_f32(None, P(Ad), P(Bd), r, scaling, P(out), n, k, st),
            "null A": lambda: lib.ucod_lora_merge_f32(P(w0d), None, P(Bd), r, scaling, P(out), n, k, st),
            "null B": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), None, r, scaling, P(out), n, k, st),
            "null out": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), P(Bd), r, scaling, None, n, k, st),
            "r 0": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), P(Bd), 0, scaling, P(out), n, k, st),
            "r 22": lambda: lib.ucod_lora_merge_f32(P(w0d), P(A22), P(B22), 22, scaling, P(out), n, k, st),
            "K % 64": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), P(Bd), r, scaling, P(out), n, 96, st),
            "K 0": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), P(Bd), r, scaling, P(out), n, 0, st),
            "N 0": lambda: lib.ucod_lora_merge_f32(P(w0d), P(Ad), P(Bd), r, scaling, P(out), 0, k, st),
            "misaligned w0": lambda: lib.ucod_lora_merge_f32(P(w0d) + 4, P(Ad), P(Bd), r, scaling, P(out), n - 1, k, st),
        }
        for name, call in calls.items():
            assert call() == EINVAL, name
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------ 2. the fold kernel
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n,k", [(37, 256), (300, 768), (20, 1536)])
def test_fold_ln_linear(n, k, scaled):
    g = torch.Generator().manual_seed(n + k)
    w, gamma, beta, b = 0.02 * torch.randn(n, k, generator=g), 1 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(k, generator=g), 0.02 * torch.randn(n, generator=g)
    q = None
    if scaled:                                                   # the Q-row pre-scale on the first rows, ones behind (and one odd value)
        q = torch.ones(n)
        q[:n // 3] = 0.125 * 1.4426950408889634
        q[-1] = 0.3
    wf_ref, bias_ref, cs_ref = fold_layernorm_linear(gamma, beta, w, b, row_scale=q, half=torch.float16)
    wd, gd_, bed, bd = dev(w, gamma, beta, b)
    qd = None if q is None else q.to(DEV)
    wf, bias, cs = Guarded(n, k, torch.float16), Guarded(1, n, torch.float32), Guarded(1, n, torch.float32)
    rc = N.load("f16").ucod_fold_ln_linear(P(wd), P(gd_), P(bed), P(bd), P(qd), wf.ptr(), bias.ptr(), cs.ptr(), n, k, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert wf.guards_intact() and bias.guards_intact() and cs.guards_intact(), "wrote outside its outputs"
    got_w, got_b, got_c = wf.payload.cpu(), bias.payload.cpu()[0], cs.payload.cpu()[0]
    assert bool(torch.isfinite(got_w.float()).all()) and bool(torch.isfinite(got_b).all()) and bool(torch.isfinite(got_c).all()), "left elements unwritten"
    assert torch.equal(got_w.view(torch.int16), wf_ref.view(torch.int16)), "folded weights differ"
    assert torch.equal(got_c, cs_ref), "column sums differ"
    ulp = torch.nextafter(bias_ref.abs(), torch.full_like(bias_ref, float("inf"))) - bias_ref.abs()
    qq = torch.ones(n, dtype=torch.float64) if q is None else q.double().abs()
    tol = ulp.double() + 1e-12 * qq * (w.double().abs() @ beta.double().abs())
    err = (got_b.double() - bias_ref.double()).abs()
    print(f"fold_ln_linear {(n, k)} scaled={scaled}: bias worst {float((err / ulp.double()).max()):.2f} ulp, {int((err > 0).sum())} of {n} differ")
    assert bool((err <= tol).all()), float((err / tol).max())
    # the bf16 build has no fold
    before = wf.payload.clone()
    assert N.load().ucod_fold_ln_linear(P(wd), P(gd_), P(bed), P(bd), P(qd), wf.ptr(), bias.ptr(), cs.ptr(), n, k, N.stream()) == EINVAL
    lib = N.load("f16")
    assert lib.ucod_fold_ln_linear(None, P(gd_), P(bed), P(bd), P(qd), wf.ptr(), bias.ptr(), cs.ptr(), n, k, N.stream()) == EINVAL
    assert lib.ucod_fold_ln_linear(P(wd), P(gd_), P(bed), P(bd), P(qd), wf.ptr(), bias.ptr(), cs.ptr(), n, 96, N.stream()) == EINVAL
    assert lib.ucod_fold_ln_linear(P(wd), P(gd_), P(bed), P(bd), P(qd), wf.ptr(), bias.ptr(), cs.ptr(), 0, k, N.stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(wf.payload.view(torch.int16), before.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 3. whole model, accuracy
SPLIT3_G8_BAR = 3e-6            # tests/test_gpu_split.py::test_split_engine_against_reference_golden, terms=3 on this golden
SPLIT3_SWIGLU_BAR = 5e-6        # tests/test_gpu_swiglu.py::test_engines_vs_restatement, "split3" (the same figure at D = 128 and D = 256)


@functools.lru_cache(maxsize=None)
def model_case(kind):
    """(LoRA engine, base state dict, heads, image on the device, f64 key map of the LoRA forward, merged state dict), built once per checkpoint kind."""
    sd, heads, L, image, B = checkpoint(kind, 128)
    targets = ["query", "key", "value", "fc1"] if kind == "gelu" else ["value", "weights_in"]
    eng = targeted_engine(sd, heads, targets)
    img = load_golden("g8_dinov2_native")["x"] if kind == "gelu" else torch.randn(B, 3, image, image, generator=torch.Generator().manual_seed(7))
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **eng.lora_state_dict()}.items() if v.is_floating_point()}
    ref = R.forward(img.to(DEV, torch.float64), full, heads, eng.scaling).cpu()
    return eng, sd, heads, img.to(DEV), ref, eng.merged_state_dict()


def test_merged_state_dict_is_a_copy_with_merged_targets():
    eng, sd, heads, img, ref, merged = model_case("gelu")
    assert sorted(merged) == sorted(sd) and not any(".lora_" in k for k in merged)
    lsd = {k: v.cpu() for k, v in eng.lora_state_dict().items()}
    for k, v in sd.items():
        mod = k[:-len(".weight")] if k.endswith(".weight") else None
        if mod is not None and mod + ".lora_A.weight" in lsd:
            want = M.merge(v, lsd[mod + ".lora_A.weight"], lsd[mod + ".lora_B.weight"], eng.scaling)
            assert merged[k].dtype == torch.float32 and merged[k].device == v.device and torch.equal(merged[k], want), k
            assert not torch.equal(merged[k], v)
        else:
            assert merged[k] is v, k                             # everything else: the same tensors
    # an untargeted projection (A = B = 0) comes out bit-identical to the base
    part = targeted_engine(sd, heads, ["query", "value"])
    pm = part.merged_state_dict()
    kk = "encoder.layer.1.attention.attention.key.weight"
    assert torch.equal(pm[kk], sd[kk]) and not torch.equal(pm[kk.replace("key", "query")], sd[kk.replace("key", "query")])


def test_engines_from_the_merged_state_dict_gelu():
    eng, sd, heads, img, ref, merged = model_case("gelu")
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(img), ref)
    e_base = rel_l2(SplitViTEngine(sd, heads=heads, device=DEV, terms=3)(img), ref)
    kb = ViTEngine(merged, heads=heads, device=DEV, half="bf16")(img).cpu()
    kd = ViTEngine(merged, heads=heads, device=DEV)(img).cpu()
    e_bf, e_def = rel_l2(kb, ref), rel_l2(kd, ref)
    record("lora_merge_engines", dict(kind="gelu", split3=e_merged, split3_unmerged=e_base, bf16=e_bf, default=e_def))
    print(f"merged gelu: split3 {e_merged:.2e} (unmerged base {e_base:.2e}), bf16 {e_bf:.2e}, default {e_def:.2e}")
    assert e_merged < SPLIT3_G8_BAR, e_merged
    assert e_base > 100 * SPLIT3_G8_BAR, e_base                  # the test has teeth: without the merge the engine runs another model
    # bf16: tests/test_gpu_kernels.py::test_vit_key_against_reference_golden (6e-3 relative L2, max-abs below a tenth of the largest value)
    assert e_bf < 6e-3 and maxdiff(kb, ref) < 0.1 * ref.abs().max().item(), e_bf
    # the default (fp16 operands): tests/test_gpu_kernels.py::test_vit_key_fp16_operands_against_reference_golden (1e-3 relative L2)
    assert e_def < 1e-3, e_def


def test_engines_from_the_merged_state_dict_swiglu():
    eng, sd, heads, img, ref, merged = model_case("swiglu")
    w = merged["encoder.layer.1.mlp.weights_in.weight"]
    assert w.shape == (2 * 344, 128) and w.dtype == torch.float32 and not torch.equal(w, sd["encoder.layer.1.mlp.weights_in.weight"])
    lsd = {k: v.cpu() for k, v in eng.lora_state_dict().items()}
    assert torch.equal(w, M.merge(sd["encoder.layer.1.mlp.weights_in.weight"], lsd["encoder.layer.1.mlp.weights_in.lora_A.weight"],
                                  lsd["encoder.layer.1.mlp.weights_in.lora_B.weight"], eng.scaling))
    assert merged["encoder.layer.1.attention.attention.query.weight"] is sd["encoder.layer.1.attention.attention.query.weight"]
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(img), ref)
    e_base = rel_l2(SplitViTEngine(sd, heads=heads, device=DEV, terms=3)(img), ref)
    record("lora_merge_engines", dict(kind="swiglu", split3=e_merged, split3_unmerged=e_base))
    print(f"merged swiglu: split3 {e_merged:.2e} (unmerged base {e_base:.2e})")
    assert e_merged < SPLIT3_SWIGLU_BAR, e_merged
    assert e_base > 100 * SPLIT3_SWIGLU_BAR, e_base


# ------------------------------------------------------------------------------------------------ 4. in-place refresh
FOLDED_BAR = 3e-3               # the folded fp16 default at D = 256: __graft_entry__.smoke() and tests/test_gpu_swiglu.py::test_engines_vs_restatement ("f16")
W_SLOTS = (N.QKV_W, N.FC1_W)


def snapshot(vit):
    return [[None if t is None else t.clone() for t in row] for row in vit.layers], [[None if t is None else t.clone() for t in row] for row in vit.fold_layers]


def same_tensors(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and torch.equal(x.view(torch.int16) if x.element_size() == 2 else x, y.view(torch.int16) if y.element_size() == 2 else y))
               for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def pointers(vit):
    return [None if t is None else t.data_ptr() for rows in (vit.layers, vit.fold_layers) for row in rows for t in row]


@pytest.mark.parametrize("kind,targets", [("gelu", ("query", "value", "fc1")), ("swiglu", ("value", "weights_in"))])
def test_merge_into_equals_a_fresh_engine(kind, targets):
    if kind == "gelu":
        sd, heads, L, image, B = checkpoint("gelu", 256)
    else:
        from swiglu_ref import random_swiglu_state_dict
        sd, heads, L, image, B = random_swiglu_state_dict(256, 4, 3, image_size=70, seed=256), 4, 3, 70, 2
    D = 256
    X, Y = targeted_engine(sd, heads, list(targets), gen_seed=3), targeted_engine(sd, heads, list(targets), gen_seed=4)
    vit = ViTEngine(sd, heads=heads, device=DEV)
    assert vit.ln_fold and vit.half == "f16" and vit.q_row_scale is not None and abs(float(vit.q_row_scale[0]) - 0.125 * 1.4426950408889634) < 1e-7
    img = torch.randn(B, 3, image, image, generator=torch.Generator().manual_seed(7)).to(DEV)
    key_base = vit(img).clone()
    ptrs, before = pointers(vit), snapshot(vit)
    assert X.merge_into(vit) is vit
    torch.cuda.synchronize()
    assert pointers(vit) == ptrs, "merge_into reallocated a tensor of the engine"
    after_x = snapshot(vit)
    fresh = ViTEngine(X.merged_state_dict(), heads=heads, device=DEV)
    # the plain tables: every tensor equal to the fresh engine's
    assert same_tensors(after_x[0], snapshot(fresh)[0])
    # the folded tables: weights and column sums bit for bit, biases by rule 2 (one f32 ulp + 1e-12 |q| sum |w beta|: f64 summation order)
    from ucod_dpl_amd.vit_engine import normalize_state_dict, _prepare_mlp
    _, mc = _prepare_mlp(normalize_state_dict(X.merged_state_dict()))
    worst_bias = 0.0
    for i, (fa, ff) in enumerate(zip(after_x[1], snapshot(fresh)[1])):
        for s, (x, y) in enumerate(zip(fa, ff)):
            if x is None or s in (N.QKV_B, N.FC1_B):
                continue
            assert torch.equal(x.view(torch.int16) if x.element_size() == 2 else x, y.view(torch.int16) if y.element_size() == 2 else y), (i, N.VIT_LAYER_SLOTS[s])
        for slot_b, wname, bname in ((N.QKV_B, "qkv_w", "ln1_b"), (N.FC1_B, "fc1_w", "ln2_b")):
            got, want = fa[slot_b].cpu(), ff[slot_b].cpu()
            q = vit.q_row_scale.cpu().double() if slot_b == N.QKV_B else torch.ones(got.numel(), dtype=torch.float64)
            ulp = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double()
            tol = ulp + 1e-12 * q * (mc["layers"][i][wname].double().abs() @ mc["layers"][i][bname].double().abs())
            err = (got.double() - want.double()).abs()
            worst_bias = max(worst_bias, float((err / ulp).max()))
            assert bool((err <= tol).all()), (i, N.VIT_LAYER_SLOTS[slot_b], float((err / tol).max()))
    # untargeted tensors (and the rows of the untargeted projections) are bit-identical to before; the targeted ones moved
    untouched_rows = [p for p, name in enumerate(("query", "key", "value")) if name not in targets]
    for tables_before, tables_after in zip(before, after_x):
        for rb, ra in zip(tables_before, tables_after):
            for s, (x, y) in enumerate(zip(rb, ra)):
                if x is None:
                    continue
                if s in (N.QKV_W, N.QKV_B, N.QKV_COLSUM):
                    for p in untouched_rows:
                        assert torch.equal(x[p * D:(p + 1) * D].float(), y[p * D:(p + 1) * D].float()), (N.VIT_LAYER_SLOTS[s], p)
                elif s not in (N.FC1_W, N.FC1_B, N.FC1_COLSUM):
                    assert torch.equal(x.float(), y.float()), N.VIT_LAYER_SLOTS[s]
    assert not torch.equal(before[0][0][N.QKV_W][:D].float(), after_x[0][0][N.QKV_W][:D].float()) or "query" not in targets
    assert not torch.equal(before[1][0][N.FC1_W].float(), after_x[1][0][N.FC1_W].float())
    # accuracy: the refreshed engine meets the fresh one's bar against the f64 LoRA forward
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **X.lora_state_dict()}.items() if v.is_floating_point()}
    ref = R.forward(img.double(), full, heads, X.scaling).cpu()
    k_live, k_fresh = vit(img), fresh(img)
    vit.check_overflow(wait=True)
    e_live, e_fresh, direct = rel_l2(k_live, ref), rel_l2(k_fresh, ref), rel_l2(k_live, k_fresh)
    record("lora_merge_refresh", dict(kind=kind, targets=",".join(targets), live=e_live, fresh=e_fresh, live_vs_fresh=direct, worst_bias_ulp=worst_bias,
                                      base_vs_ref=rel_l2(key_base, ref)))
    print(f"merge_into {kind} {targets}: live {e_live:.2e}, fresh {e_fresh:.2e}, live vs fresh {direct:.2e}, folded bias worst {worst_bias:.2f} ulp, base {rel_l2(key_base, ref):.2e}")
    assert e_live < FOLDED_BAR and e_fresh < FOLDED_BAR, (e_live, e_fresh)
    assert rel_l2(key_base, ref) > 5 * e_live                    # ... and the unrefreshed engine is clearly farther away: the refresh did something
    # no drift: X, Y, X again gives the tensors of the first X bit for bit (always merged from the f32 base)
    Y.merge_into(vit)
    after_y = snapshot(vit)
    assert not same_tensors(after_y[0], after_x[0]) and not same_tensors(after_y[1], after_x[1])
    X.merge_into(vit)
    again = snapshot(vit)
    assert same_tensors(again[0], after_x[0]) and same_tensors(again[1], after_x[1]) and pointers(vit) == ptrs


def test_merge_into_refusals():
    sd, heads, L, image, B = checkpoint("gelu", 128)
    eng = model_case("gelu")[0]
    with pytest.raises(NotImplementedError, match="merged_state_dict"):
        eng.merge_into(SplitViTEngine(sd, heads=heads, device=DEV, terms=2))
    sd256, heads256 = checkpoint("gelu", 256)[:2]
    with pytest.raises(ValueError, match="differ"):
        eng.merge_into(ViTEngine(sd256, heads=heads256, device=DEV))
    sw = checkpoint("swiglu", 128)
    with pytest.raises(ValueError, match="differ"):
        eng.merge_into(ViTEngine(sw[0], heads=sw[1], device=DEV))
    with pytest.raises(TypeError):
        eng.merge_into(targeted_engine(sd, heads, ["query"]))
    # a bf16 engine without the fold is refreshed too (plain tables only)
    vit = ViTEngine(sd, heads=heads, device=DEV, half="bf16")
    assert vit.fold_layers is None and vit.q_row_scale is None
    eng.merge_into(vit)
    fresh = ViTEngine(model_case("gelu")[5], heads=heads, device=DEV, half="bf16")
    assert same_tensors(vit.layers, fresh.layers)


# ------------------------------------------------------------------------------------------------ 5. public surface
def lora_cfg(targets):
    from ucod_dpl_amd.engine.config import CfgNode
    return CfgNode(dict(r=2, lora_alpha=4, lora_dropout=0.0, target_modules=list(targets)))


def test_merge_and_unload_and_adapter_round_trip(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.data.utils.feature_extractor import backbone
    from ucod_dpl_amd.models.modules.full_model import load_lora, load_lora_adapter, save_lora_adapter
    eng, sd, heads, img, ref, merged = model_case("gelu")
    targets = ["query", "key", "value", "fc1"]
    bb = load_lora(lora_cfg(targets), sd, heads=heads, device=DEV)
    bb.engine.load_lora_state_dict(eng.lora_state_dict())
    frozen = bb.merge_and_unload(precision="split3")
    assert isinstance(frozen, backbone) and isinstance(frozen.engine, SplitViTEngine) and frozen.precision == "split3"
    assert torch.equal(frozen(img)[1], SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(img))
    assert isinstance(bb.merge_and_unload().engine, ViTEngine)
    # adapter folder -> a second engine: equal arenas, equal key maps
    folder = save_lora_adapter(eng, str(tmp_path / "lora"))
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    assert sorted(tensors) == M.adapter_keys(3, ("query", "key", "value"), "fc1")
    cfg = json.load(open(os.path.join(folder, "adapter_config.json")))
    assert (cfg["r"], cfg["lora_alpha"], cfg["bias"], cfg["target_modules"]) == (2, 4, "none", targets)
    other = load_lora(lora_cfg(targets), sd, heads=heads, device=DEV, generator=torch.Generator().manual_seed(99)).engine
    assert not torch.equal(other.lora, eng.lora)
    load_lora_adapter(other, folder)
    assert torch.equal(other.lora, eng.lora)
    eng.eval()
    other.eval()
    assert torch.equal(other.forward_train(img), eng.forward_train(img))
    eng.train()
    with pytest.raises(ValueError, match="target_modules"):
        load_lora_adapter(load_lora(lora_cfg(["query", "value"]), sd, heads=heads, device=DEV).engine, folder)
    # the SwiGLU module's B travels in HF row order, unpadded
    sw = model_case("swiglu")[0]
    t2 = load_file(os.path.join(save_lora_adapter(sw, str(tmp_path / "sw")), "adapter_model.safetensors"))
    assert t2[M.ADAPTER_PREFIX + "1.mlp.weights_in.lora_B.weight"].shape == (688, 2)


def runner_cfg(tmp_path, sd):
    from safetensors.torch import save_file
    from ucod_dpl_amd.engine.config import CfgNode
    weights = tmp_path / "weights"
    weights.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(weights / "model.safetensors"))
    (weights / "config.json").write_text(json.dumps({"model_type": "dinov2", "num_attention_heads": 2, "layer_norm_eps": 1e-6}))
    return CfgNode(dict(
        model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, dis_use_features=False),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=6e-4, dis_lr0=1e-3, step_lr_size=2, dis_step_lr_size=2,
                       step_lr_gamma=0.95, dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1,
                       dis_intertrain=2, save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50),
        dataset_cfg=dict(feature_extractor_cfg=dict(type="dinov2", backbone_type="huggingface", backbone="facebook/dinov2-base", backbone_weights=str(weights))),
        log_cfg=dict(log_interval=50, log_path=str(tmp_path / "log"), multi_rank=[0])))


def test_runner_checkpoints_and_validates_the_lora_backbone(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.data.utils.feature_extractor import backbone
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    eng0, sd, heads, img, ref, _ = model_case("gelu")
    cfg = runner_cfg(tmp_path, sd)
    torch.manual_seed(3)
    # a runner without attach_lora_backbone: the single file of today, the frozen backbone in validation
    plain = StandardRunner(cfg)
    plain.save_checkpoint(1)
    ckp = os.path.join(cfg.log_cfg.log_path, "ckp")
    assert os.listdir(os.path.join(ckp, "epoch1.pth")) == ["model.safetensors"] and plain.val_feature_extractor() is None
    decoder_keys = sorted(plain.model.state_dict())
    # LoRA mode
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    eng = targeted_engine(sd, heads, ["query", "key", "value", "fc1"])
    loop.attach_lora_backbone(eng)
    assert runner.lora_engine is eng and runner.lora_engine_ema is loop.lora_engine_ema
    pl = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(11)) > 0.5).float()
    loop._process_batch_full(img, pl)
    runner.save_checkpoint(2)
    path = os.path.join(ckp, "epoch2.pth")
    assert sorted(os.listdir(path)) == ["lora", "lora_ema", "model.safetensors"]
    assert sorted(load_file(os.path.join(path, "model.safetensors"))) == decoder_keys
    want = M.adapter_keys(3, ("query", "key", "value"), "fc1")
    saved = load_file(os.path.join(path, "lora", "adapter_model.safetensors"))
    assert sorted(saved) == want and sorted(load_file(os.path.join(path, "lora_ema", "adapter_model.safetensors"))) == want
    k0 = M.ADAPTER_PREFIX + "0.mlp.fc1.lora_A.weight"
    assert torch.equal(saved[k0], eng.lora_state_dict()["encoder.layer.0.mlp.fc1.lora_A.weight"].cpu())
    # validation runs the trained backbone: the frozen one of the config, refreshed in place
    frozen_key = backbone(cfg.dataset_cfg.feature_extractor_cfg, device=runner.device)(img)[1].clone()
    fe = runner.val_feature_extractor()
    assert isinstance(fe, backbone) and isinstance(fe.engine, ViTEngine) and fe.engine.half == "f16"
    key = fe(img)[1].clone()
    assert rel_l2(key, frozen_key) > 1e-2
    fresh = ViTEngine(eng.merged_state_dict(), heads=heads, device=DEV)
    assert same_tensors(fe.engine.layers, fresh.layers) and torch.equal(key, fresh(img))       # (D = 128: no fold, so rule 4 is bit equality throughout)
    assert runner.val_feature_extractor() is fe                  # built once
    key_ema = runner.val_feature_extractor("ema")(img)[1].clone()
    assert torch.equal(key_ema, ViTEngine(loop.lora_engine_ema.merged_state_dict(), heads=heads, device=DEV)(img))
    with pytest.raises(ValueError, match="student"):
        runner.val_feature_extractor("teacher")
