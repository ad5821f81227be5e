"""GPU: backbone-backward (LoRA) mode with DINOv3's MLP input targeted (``allow_mlp_in``): ``up_proj`` on the plain MLP (the fc1 module's kernels), ``gate_proj`` /
``up_proj`` on the gated MLP (the pair kernels, UCOD_LORA_MLP_PAIR), against the G26 goldens -- transformers' own f64 key maps and gradients
(tests/golden/make_golden_dinov3_lora_mlp_in.py).

1  Every target set x dropout {0, 0.05} x streams {1, 2}: the key map within dinov3_ref.engine_bound("bf16") = 3 x transformers under bf16 autocast, every gradient
   within dinov3_lora_mlp_in_ref.grad_bar = max(4e-2 (5e-2 with dropout), 3 x that gradient under bf16 autocast), structural zeros -- the last layer's modules, and
   the untargeted one of the pair -- exactly zero, two runs bit-identical.  With dropout the reference is the f64 restatement under the engine's hash masks, chunk
   by chunk.  tests/test_dinov3_lora_mlp_in_host.py shows every such bar to lie under half of what a wrong block structure of the pair does.
2  "Every Linear" on the gated model (q, k, v, o, gate, up, down): the passes against the restatement at the project's bar; merged_state_dict -> a frozen ViTEngine
   and merge_into give the no-grad LoRA pass's key map; the adapter folder round-trips bit for bit; clone_for_ema.
3  bias="lora_only" with both of the pair targeted against the golden's bias gradients; a full_model step through load_lora with ``lora_cfg.allow_mlp_in``.
"""
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
from ucod_dpl_amd import vit_engine as V  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, ViTLoRAEngine  # noqa: E402
from ucod_dpl_amd.models.modules import full_model as M  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402
import dinov3_lora_mlp_in_ref as RM  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EVERY = list(RM.LEAVES)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def g26(tag):
    z = np.load(os.path.join(GOLDEN, f"g26_dinov3_lora_mlp_in_{tag}.npz"))
    return z, R3.g22_state_dict(tag), torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])


def engine(tag, targets, lora, **kw):
    m = R3.G22[tag]
    eng = ViTLoRAEngine(g26(tag)[1], heads=m["heads"], r=RM.G26_R, lora_alpha=RM.G26_ALPHA, eps=1e-5, device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=targets, allow_rope=True, allow_swiglu=m["gated"], allow_mlp_in=True, **kw)
    assert sorted(k for k in eng.lora_state_dict() if ".lora_" in k) == sorted(lora)
    eng.load_lora_state_dict({**{k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}, **lora})
    return eng


def reference(tag, lora, bounds, seeds, p_drop, leaves, bias_of=()):
    """(key, gradients) of the f64 restatement, chunk by chunk with the engine's masks (each chunk has its own; gradients add)"""
    z, sd, x, dkey = g26(tag)
    m = R3.G22[tag]
    tok = 1 + m["R"] + m["grid"][0] * m["grid"][1]
    key_ref, gref = [], None
    for (b0, b1), seed in zip(bounds, seeds):
        masks = RM.g26_masks(tag, leaves, (b1 - b0) * tok, seed, p_drop) if p_drop > 0 else None
        k, g = RM.grads(x[b0:b1], {**sd, **lora}, m["heads"], dkey[b0:b1], RM.G26_SCALE, masks=masks, device=DEV, bias_of=bias_of)
        key_ref.append(k.cpu())
        gref = {n: v.cpu() for n, v in g.items()} if gref is None else {n: gref[n] + v.cpu() for n, v in g.items()}
    return torch.cat(key_ref, 0), gref


def check_passes(name, make, ref_of, x, dkey, key_bound, bar_of):
    eng = make()
    key = eng.forward_train(x.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    key_ref, gref = ref_of(eng)
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    assert sorted(got) == sorted(gref)
    key_err = rel_l2(key, key_ref)
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=lambda k: errs[k] / bar_of(k))
    mlp = {k: e for k, e in errs.items() if ".mlp.gate_proj" in k or ".mlp.up_proj" in k}
    print(f"{name}: key rel-L2 {key_err:.3e} (bound {key_bound:.2e}); worst gradient {errs[worst]:.3e} of bar {bar_of(worst):.2e} ({worst}); "
          f"worst MLP-input gradient {max(mlp.values()):.3e}")
    within(name + " key", key_err, key_bound)
    for k, ref in gref.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    assert len(mlp) > 0
    for k, e in errs.items():
        within(f"{name} {k}", e, bar_of(k))
    eng2 = make()                                                 # two backward runs are bit-identical
    eng2.forward_train(x.to(DEV))
    assert torch.equal(eng2.backward(dkey.to(DEV)), eng.lora_grad)
    return eng


# ================================================================================================ 1. the target sets against G26
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tag,tset", [(t, s) for t in RM.G26_TAGS for s in RM.G26_SETS[t]])
def test_mlp_input_targets_vs_f64_autograd(tag, tset, p_drop, streams):
    z, sd, x, dkey = g26(tag)
    m = R3.G22[tag]
    targets = RM.g26_targets(tag, tset)
    lora = RM.g26_lora(tag, targets)

    def make():
        e = engine(tag, targets, lora, lora_dropout=p_drop, seed=RM.G26_ENGINE_SEED)
        e.train_streams = streams
        return e

    def ref_of(eng):
        if p_drop == 0:                                           # transformers' own f64 values
            return torch.from_numpy(z["key/" + tset]), {k[len(f"grad/{tset}/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"grad/{tset}/")}
        return reference(tag, lora, list(eng._bounds), list(eng._chunk_seed), p_drop, targets)

    key_bound = R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/" + tset]})
    eng = check_passes(f"g26 {tag} {tset} p={p_drop} streams={streams}", make, ref_of, x, dkey, key_bound, lambda k: RM.grad_bar(z, tset, k, p_drop))
    assert eng.mlp_pair == m["gated"] and eng.mlp_in_live and eng._out_flags == (N.LORA_MLP_PAIR if m["gated"] else 0) and len(eng.modules) == (7 if m["gated"] else 6)
    if p_drop > 0 and streams == 1:                               # the run whose shared_mask fault the golden stores: same seed, same truth
        assert list(eng._chunk_seed) == [RM.G26_DROP_SEED] and int(z["drop_seed"]) == RM.G26_DROP_SEED
        if tset == "both":
            got = eng.lora_state_dict(grads=True)
            n = "model.layer.0.mlp.up_proj.lora_A.weight"
            within(f"g26 gated both stored dropout truth {n}", rel_l2(got[n], torch.from_numpy(z["drop/" + n])), RM.grad_bar(z, tset, n, p_drop))
    if m["gated"] and tset != "both":                             # the untargeted one of the pair: A = 0, its rows of B = 0, its gradients exact zeros in the arena
        dead = eng.modules[V._MLP_IN2 if tset == "gate" else V._MLP_IN]
        assert not dead.targeted and float(eng.lora[:, dead.a].abs().max()) == 0.0 and float(eng.lora_grad[:, dead.a].abs().max()) == 0.0
        blk, gblk = (t[:, dead.b].reshape(eng.L, dead.n // 4, 2, 4, eng.r)[:, :, dead.part] for t in (eng.lora, eng.lora_grad))
        assert float(blk.abs().max()) == 0.0 and float(gblk.abs().max()) == 0.0
        assert float(eng.lora_grad[:eng.L - 1, dead.b].abs().max()) > 0          # (the live module's rows of the shared block are not zero)


# ================================================================================================ 2. every Linear of the gated block
def every_engine(**kw):
    lora = RM.g26_lora("gated")
    return engine("gated", EVERY, lora, allow_out=True, allow_swiglu_out=True, **kw), lora


def test_every_linear_of_the_gated_block(tmp_path):
    z, sd, x, dkey = g26("gated")
    z22 = np.load(os.path.join(GOLDEN, "g22_dinov3_gated.npz"))
    bound = R3.engine_bound("bf16", z22)
    lora = RM.g26_lora("gated")

    def make():
        e = every_engine()[0]
        e.train_streams = 2
        return e

    eng = check_passes("g26 gated every Linear", make, lambda e: reference("gated", lora, [(0, 3)], [0], 0.0, EVERY), x, dkey, bound, lambda k: 4e-2)
    assert [m.leaf for m in eng.modules if m.targeted] == ["q_proj", "k_proj", "v_proj", "gate_proj", "o_proj", "down_proj", "up_proj"]
    assert eng._out_flags == N.LORA_OUT_SWIGLU | N.LORA_MLP_PAIR
    xd = x.to(DEV)
    eng.eval()
    k_lora = eng.forward_nograd(xd, resid16=True).clone()
    eng.check_overflow(wait=True)
    # merged_state_dict -> a frozen ViTEngine: the no-grad LoRA pass's key map
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    changed = sorted(k for k in sd if not torch.equal(merged[k].cpu(), sd[k]))
    assert changed == sorted(f"model.layer.{i}.{RM.module_path(leaf)}.weight" for i in range(3) for leaf in RM.LEAVES)
    fresh = ViTEngine(merged, heads=2, eps=1e-5, device=DEV)
    k_merged, k_base = fresh(xd).clone(), ViTEngine(sd, heads=2, eps=1e-5, device=DEV)(xd).clone()
    print(f"every Linear merged: {rel_l2(k_merged, k_lora):.2e} from the no-grad LoRA pass (bound {bound:.2e}; unmerged {rel_l2(k_base, k_lora):.2e})")
    within("g26 gated every Linear merged vs nograd", rel_l2(k_merged, k_lora), bound)
    assert rel_l2(k_base, k_lora) > bound                           # (the adapters matter: the unmerged engine is outside)
    # merge_into a live engine == rebuilding it (D = 128: no fold; the plain tables tensor for tensor)
    vit = ViTEngine(sd, heads=2, eps=1e-5, device=DEV)
    assert eng.merge_into(vit) is vit
    for ra, rb in zip(vit.layers, fresh.layers):
        for a, b in zip(ra, rb):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    within("g26 gated every Linear merge_into vs nograd", rel_l2(vit(xd), k_lora), bound)
    # the adapter folder: names, config, and a bit-exact round trip into a second engine
    M.save_lora_adapter(eng, str(tmp_path))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / M.ADAPTER_WEIGHTS))
    assert sorted(saved) == sorted("base_model.model.ViT." + k for k in lora)
    for k, v in lora.items():                                     # HF's names and shapes: [r, D] and [F0, r], unpadded and de-interleaved
        assert torch.equal(saved["base_model.model.ViT." + k], v), k
    assert tuple(saved["base_model.model.ViT.model.layer.0.mlp.gate_proj.lora_B.weight"].shape) == (384, 2)
    assert sorted(json.loads((tmp_path / M.ADAPTER_CONFIG).read_text())["target_modules"]) == sorted(EVERY)
    other = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, allow_rope=True, allow_swiglu=True, allow_out=True, allow_swiglu_out=True,
                          allow_mlp_in=True, target_modules=EVERY, generator=torch.Generator().manual_seed(9))
    assert not torch.equal(other.lora, eng.lora)
    M.load_lora_adapter(other, str(tmp_path))
    assert torch.equal(other.lora, eng.lora)
    for a, b in zip(other.mlp_layers, eng.mlp_layers):
        assert torch.equal(bits(a[0]), bits(b[0]))
    one = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, allow_rope=True, allow_swiglu=True, allow_mlp_in=True, target_modules=["up_proj"])
    with pytest.raises(ValueError, match="target_modules"):
        M.load_lora_adapter(one, str(tmp_path))
    # clone_for_ema: own arena and own augmented weights_in, the same pass
    ema = eng.clone_for_ema().eval()
    assert ema.mlp_pair and ema.lora.data_ptr() != eng.lora.data_ptr() and ema.mlp_layers[0][0].data_ptr() != eng.mlp_layers[0][0].data_ptr()
    assert torch.equal(ema.forward_nograd(xd, resid16=True), k_lora)
    ema.lora.zero_()
    ema.repack()
    assert torch.equal(eng.forward_nograd(xd, resid16=True), k_lora) and rel_l2(ema.forward_nograd(xd, resid16=True), k_base) < bound


def test_fresh_engine_draws_a_per_module_and_keeps_the_earlier_stream():
    z, sd, x, dkey = g26("gated")
    kw = dict(heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, allow_rope=True, allow_swiglu=True, allow_mlp_in=True)
    a = ViTLoRAEngine(sd, generator=torch.Generator().manual_seed(9), target_modules=list(RL.QKV) + list(RM.PAIR), **kw)
    b = ViTLoRAEngine(sd, generator=torch.Generator().manual_seed(9), target_modules=list(RL.QKV), **kw)
    assert torch.equal(a.lora[:, :a.qkv_numel], b.lora[:, :b.qkv_numel])          # the new modules are drawn after the existing ones
    g, u = a.modules[V._MLP_IN], a.modules[V._MLP_IN2]
    for m in (g, u):                                              # A kaiming-uniform per module, B zeros
        A = a.lora[:, m.a]
        assert float(A.abs().max()) <= 1 / 128 ** 0.5 and float(A.abs().max()) > 0.9 / 128 ** 0.5 and abs(float(A.mean())) < 0.01
    assert not torch.equal(a.lora[:, g.a], a.lora[:, u.a]) and float(a.lora[:, g.b].abs().max()) == 0.0
    assert rel_l2(a.forward_train(x.to(DEV)), b.forward_train(x.to(DEV))) < 1e-3    # B = 0: the adapter is the identity (up to the GEMM's K = D + 64 walk)


# ================================================================================================ 3. trained biases; full_model
def test_lora_only_with_both_of_the_pair_matches_the_goldens_bias_gradients():
    z, sd, x, dkey = g26("gated")
    targets = RM.g26_targets("gated", "both")
    lora = RM.g26_lora("gated", targets)
    with pytest.raises(NotImplementedError, match="fused bias"):
        engine("gated", RM.g26_targets("gated", "up"), RM.g26_lora("gated", RM.g26_targets("gated", "up")), bias="lora_only")
    eng = engine("gated", targets, lora, bias="lora_only")
    eng.train_streams = 2
    key = eng.forward_train(x.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    bnames = sorted(k[len("bgrad/"):] for k in z.files if k.startswith("bgrad/"))
    assert sorted(k for k in got if k.endswith(".bias")) == bnames and len(bnames) == 3 * 4         # q, v, gate, up of every layer (k_proj has no bias)
    within("g26 gated both lora_only key", rel_l2(key, torch.from_numpy(z["key/both"])), R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/both"]}))
    worst = 0.0
    for n in bnames:
        ref = torch.from_numpy(z["bgrad/" + n])
        if float(ref.abs().max()) == 0.0:                         # the last layer's q, v and MLP never reach the key map
            assert float(got[n].abs().max()) == 0.0, n
            continue
        assert tuple(got[n].shape) == tuple(ref.shape)
        worst = max(worst, rel_l2(got[n], ref))
        within(f"g26 gated both lora_only {n}", rel_l2(got[n], ref), 4e-2)           # the project's LoRA-gradient bar (tests/test_gpu_lora_bias.py)
    print(f"lora_only with the pair: worst bias gradient {worst:.3e} (bar 4e-2)")
    for k in (k for k in got if ".lora_" in k):
        ref = torch.from_numpy(z["grad/both/" + k])
        if float(ref.abs().max()) != 0.0:
            within(f"g26 gated both lora_only {k}", rel_l2(got[k], ref), RM.grad_bar(z, "both", k))
    # the state dict carries each module's own half of the fused bias, as the checkpoint has it
    vals = eng.lora_state_dict()
    for leaf in RM.PAIR:
        assert torch.equal(vals[f"model.layer.0.mlp.{leaf}.bias"].cpu(), sd[f"model.layer.0.mlp.{leaf}.bias"])


def test_full_model_step_through_load_lora_changes_the_new_parameters_only():
    from ucod_dpl_amd.engine.config import CfgNode
    z, sd, x, dkey = g26("gated")
    targets = RM.g26_targets("gated", "both")
    cfg = dict(r=2, lora_alpha=4, lora_dropout=0.0, allow_rope=True, target_modules=targets)
    with pytest.raises(NotImplementedError) as e:                 # without the build-only key: today's refusal
        M.load_lora(CfgNode(cfg), sd, 2, device=DEV)
    assert V._REFUSED3["up_proj"] in str(e.value) or V._REFUSED3["gate_proj"] in str(e.value)
    bb = M.load_lora(CfgNode(dict(cfg, allow_mlp_in=True)), sd, 2, device=DEV)
    eng = bb.engine
    assert eng.allow_mlp_in and eng.mlp_pair
    eng.load_lora_state_dict(RM.g26_lora("gated", targets))
    frozen = [[None if t is None else t.clone() for t in row] for row in eng.layers]
    before, w_aug = eng.lora.clone(), eng.mlp_layers[0][0].clone()
    opt = torch.optim.SGD([bb.lora], lr=0.5)
    key = bb(x.to(DEV))
    (key * dkey.to(DEV)).sum().backward()
    assert torch.equal(bb.lora.grad, eng.lora_grad)
    ref = torch.from_numpy(z["grad/both/model.layer.0.mlp.gate_proj.lora_A.weight"])
    within("g26 gated autograd gate_proj A", rel_l2(bb.lora.grad[0, eng.modules[V._MLP_IN].a].reshape(2, 128), ref), RM.grad_bar(z, "both", "model.layer.0.mlp.gate_proj.lora_A.weight"))
    opt.step()
    eng.repack()
    for m in (eng.modules[V._MLP_IN], eng.modules[V._MLP_IN2]):   # the new parameters of the layers whose MLP runs moved
        assert not torch.equal(eng.lora[:2, m.a], before[:2, m.a]) and torch.equal(eng.lora[2, m.a], before[2, m.a])
    assert not torch.equal(eng.lora[:2, eng.modules[V._MLP_IN].b], before[:2, eng.modules[V._MLP_IN].b])
    assert not torch.equal(bits(eng.mlp_layers[0][0]), bits(w_aug))
    for ra, rb in zip(eng.layers, frozen):                        # and no frozen tensor did
        for a, b in zip(ra, rb):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    assert torch.equal(bits(eng.mlp_layers[0][0][:, :128]), bits(w_aug[:, :128]))
