"""GPU: backbone-backward (LoRA) mode on a gated DINOv3 model whose MLP is as wide as dinov3_vith16plus's (``allow_wide_mlp``, UCOD_LORA_WIDE): hidden 5120, so the
gate_proj / up_proj pair has N1 = 10240 rows and down_proj K = 5120 input columns, on a small trunk (tests/lora_wide_ref.py: D = 128, 2 heads, 4 registers, 2 layers,
3 x 3 x 64 x 96 images; only layer 0's MLP reaches the key map), against the G28 golden -- transformers' own f64 key maps and gradients
(tests/golden/make_golden_dinov3_lora_wide.py) -- and, with dropout or trained biases, the f64 restatement under the engine's masks, chunk by chunk.

1  Target sets [gate_proj, up_proj], [down_proj], every Linear x dropout {0, 0.05} x streams {1, 2} x bias {none, lora_only}: the key map within
   dinov3_ref.engine_bound("bf16") = 3 x transformers under bf16 autocast, every LoRA gradient within dinov3_lora_mlp_in_ref.grad_bar = max(4e-2 (5e-2 with dropout),
   3 x that gradient under bf16 autocast), bias gradients within the same 4e-2 / 5e-2, structural zeros exactly zero, two runs bit-identical.  The golden's two
   mutations (no forward term; t over the first 8192 columns) lie outside these bars (tests/test_lora_wide_host.py checks the stored distances on the CPU).
2  Every Linear: merged_state_dict -> a frozen ViTEngine and merge_into give the no-grad LoRA pass's key map, the unmerged engine does not; the adapter folder
   round-trips bit for bit.
3  Without the opt-in: today's refusal.  With it and narrow targets only, the engine without it: arena, key map, gradients and workspace size, bit for bit.
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
from ucod_dpl_amd.vit_engine import ViTEngine, ViTLoRAEngine  # noqa: E402
from ucod_dpl_amd.models.modules import full_model as M  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_mlp_in_ref as RM  # noqa: E402
import lora_wide_ref as RW  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g28_dinov3_lora_wide.npz")
OPT_INS = dict(allow_rope=True, allow_swiglu=True, allow_mlp_in=True, allow_out=True, allow_swiglu_out=True)
TOK = 1 + RW.G28["R"] + RW.G28["grid"][0] * RW.G28["grid"][1]


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def g28():
    x, dkey = RW.g28_inputs()
    return np.load(GOLDEN), RW.g28_state_dict(), x, dkey


def engine(targets, lora, **kw):
    kw = {**OPT_INS, "allow_wide_mlp": True, **kw}
    eng = ViTLoRAEngine(g28()[1], heads=RW.G28["heads"], r=RW.G28_R, lora_alpha=RW.G28_ALPHA, eps=1e-5, device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=list(targets), **kw)
    assert sorted(k for k in eng.lora_state_dict() if ".lora_" in k) == sorted(lora)
    eng.load_lora_state_dict({**{k: v for k, v in eng.lora_state_dict().items() if ".lora_" not in k}, **lora})
    return eng


def reference(lora, bounds, seeds, p_drop, leaves, bias_of=()):
    """(key, gradients) of the f64 restatement, chunk by chunk with the engine's masks (each chunk has its own; gradients add)"""
    z, sd, x, dkey = g28()
    key_ref, gref = [], None
    for (b0, b1), seed in zip(bounds, seeds):
        masks = RW.g28_masks(leaves, (b1 - b0) * TOK, seed, p_drop) if p_drop > 0 else None
        k, g = RW.grads(x[b0:b1], {**sd, **lora}, dkey[b0:b1], masks=masks, device=DEV, bias_of=bias_of)
        key_ref.append(k.cpu())
        gref = {n: v.cpu() for n, v in g.items()} if gref is None else {n: gref[n] + v.cpu() for n, v in g.items()}
    return torch.cat(key_ref, 0), gref


# ================================================================================================ 1. the target sets against G28
@pytest.mark.parametrize("bias", ["none", "lora_only"])
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("tset", list(RW.G28_SETS))
def test_wide_targets_vs_f64_autograd(tset, p_drop, streams, bias):
    z, sd, x, dkey = g28()
    leaves = RW.G28_SETS[tset]
    lora = RW.g28_lora(leaves)
    bias_of = sorted(f"model.layer.{i}.{RM.module_path(leaf)}.bias" for i in range(RW.G28_LAYERS) for leaf in leaves) if bias == "lora_only" else []
    bias_of = [n for n in bias_of if n in sd]                     # (k_proj has none)

    def make():
        e = engine(leaves, lora, lora_dropout=p_drop, seed=RW.G28_ENGINE_SEED, bias=bias)
        e.train_streams = streams
        return e

    eng = make()
    key = eng.forward_train(x.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    wide_in, wide_out = any(leaf in RM.PAIR for leaf in leaves), "down_proj" in leaves
    assert eng._wide and eng._out_flags == N.LORA_WIDE | (N.LORA_MLP_PAIR if wide_in else 0) | (N.LORA_OUT_SWIGLU if wide_out else 0)
    assert eng.N1 == 10240 and eng.mlp_pair == wide_in and eng.modules[5].k == 5120
    if p_drop == 0 and bias == "none":                            # transformers' own f64 values
        key_ref, gref = torch.from_numpy(z["key/" + tset]), {k[len(f"grad/{tset}/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"grad/{tset}/")}
    else:
        key_ref, gref = reference(lora, list(eng._bounds), list(eng._chunk_seed), p_drop, leaves, bias_of)
    if p_drop > 0 and streams == 1:
        assert list(eng._chunk_seed) == [RW.G28_DROP_SEED]
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    assert sorted(got) == sorted(gref)
    bar_of = lambda k: (4e-2 if p_drop == 0 else 5e-2) if k.endswith(".bias") else RW.grad_bar(z, tset, k, p_drop)  # noqa: E731
    key_bound = R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/" + tset]})
    key_err = rel_l2(key, key_ref)
    errs = {k: rel_l2(got[k], ref) for k, ref in gref.items() if float(ref.abs().max()) != 0.0}
    worst = max(errs, key=lambda k: errs[k] / bar_of(k))
    wide = {k: e for k, e in errs.items() if any(f".mlp.{leaf}." in k for leaf in RW.WIDE_LEAVES)}
    print(f"g28 {tset} p={p_drop} streams={streams} bias={bias}: key rel-L2 {key_err:.3e} (bound {key_bound:.2e}); worst gradient {errs[worst]:.3e} of bar "
          f"{bar_of(worst):.2e} ({worst}); worst wide-module gradient {max(wide.values()):.3e}")
    within(f"g28 {tset} key", key_err, key_bound)
    for k, ref in gref.items():                                   # structural zeros: the last layer's modules (all but k_proj)
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    assert len(wide) >= 2 * len(set(leaves) & set(RW.WIDE_LEAVES))
    for k, e in errs.items():
        within(f"g28 {tset} {k}", e, bar_of(k))
    # the golden's mutations would not pass: their stored distances are outside what was just asked
    assert float(z[f"mut/no_forward/{tset}/key"]) > key_bound
    if wide_in:
        for leaf in RM.PAIR:
            n = f"model.layer.0.mlp.{leaf}.lora_A.weight"
            assert float(z[f"mut/t_8192/{tset}/{n}"]) > bar_of(n)
    eng2 = make()                                                 # two runs are bit-identical
    eng2.forward_train(x.to(DEV))
    assert torch.equal(eng2.backward(dkey.to(DEV)), eng.lora_grad)


# ================================================================================================ 2. every Linear: merges and the adapter folder
def test_every_linear_merges_and_round_trips(tmp_path):
    z, sd, x, dkey = g28()
    lora = RW.g28_lora()
    bound = R3.engine_bound("bf16", {"err_bf16ac": z["err_bf16ac/every"]})
    eng = engine(RM.LEAVES, lora)
    assert [m.leaf for m in eng.modules if m.targeted] == ["q_proj", "k_proj", "v_proj", "gate_proj", "o_proj", "down_proj", "up_proj"]
    xd = x.to(DEV)
    eng.eval()
    k_lora = eng.forward_nograd(xd, resid16=True).clone()
    eng.check_overflow(wait=True)
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    changed = sorted(k for k in sd if not torch.equal(merged[k].cpu(), sd[k]))
    assert changed == sorted(f"model.layer.{i}.{RM.module_path(leaf)}.weight" for i in range(RW.G28_LAYERS) for leaf in RM.LEAVES)
    fresh = ViTEngine(merged, heads=2, eps=1e-5, device=DEV)
    k_merged, k_base = fresh(xd).clone(), ViTEngine(sd, heads=2, eps=1e-5, device=DEV)(xd).clone()
    print(f"g28 every Linear merged: {rel_l2(k_merged, k_lora):.2e} from the no-grad LoRA pass (bound {bound:.2e}; unmerged {rel_l2(k_base, k_lora):.2e})")
    within("g28 every Linear merged vs nograd", rel_l2(k_merged, k_lora), bound)
    assert rel_l2(k_base, k_lora) > bound                           # (the adapters matter: the unmerged engine is outside)
    vit = ViTEngine(sd, heads=2, eps=1e-5, device=DEV)
    assert eng.merge_into(vit) is vit
    for ra, rb in zip(vit.layers, fresh.layers):
        for a, b in zip(ra, rb):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    within("g28 every Linear merge_into vs nograd", rel_l2(vit(xd), k_lora), bound)
    # the adapter folder: HF's names and shapes, and a bit-exact round trip into a second engine
    M.save_lora_adapter(eng, str(tmp_path))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / M.ADAPTER_WEIGHTS))
    assert sorted(saved) == sorted("base_model.model.ViT." + k for k in lora)
    for k, v in lora.items():
        assert torch.equal(saved["base_model.model.ViT." + k], v), k
    assert tuple(saved["base_model.model.ViT.model.layer.0.mlp.gate_proj.lora_B.weight"].shape) == (5120, 2)
    assert tuple(saved["base_model.model.ViT.model.layer.0.mlp.down_proj.lora_A.weight"].shape) == (2, 5120)
    assert sorted(json.loads((tmp_path / M.ADAPTER_CONFIG).read_text())["target_modules"]) == sorted(RM.LEAVES)
    other = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, target_modules=list(RM.LEAVES), generator=torch.Generator().manual_seed(9),
                          allow_wide_mlp=True, **OPT_INS)
    assert not torch.equal(other.lora, eng.lora)
    M.load_lora_adapter(other, str(tmp_path))
    assert torch.equal(other.lora, eng.lora)
    for a, b in zip(other.mlp_layers, eng.mlp_layers):
        assert torch.equal(bits(a[0]), bits(b[0]))
    ema = eng.clone_for_ema().eval()                              # clone_for_ema keeps the wide passes
    assert ema._wide and torch.equal(ema.forward_nograd(xd, resid16=True), k_lora)


# ================================================================================================ 3. the opt-in
@pytest.mark.parametrize("targets", [RM.PAIR, ("down_proj",), RM.LEAVES])
def test_without_the_opt_in_the_refusal_is_todays(targets):
    z, sd, x, dkey = g28()
    with pytest.raises(NotImplementedError, match=r"(N1 = 10240.*8192.*dinov3_vith16plus)|(K = 5120.*K <= 4096)"):
        ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, target_modules=list(targets), **OPT_INS)
    from ucod_dpl_amd.engine.config import CfgNode
    cfg = dict(r=2, lora_alpha=4, lora_dropout=0.0, target_modules=list(targets), **{k: v for k, v in OPT_INS.items() if k != "allow_swiglu"})
    with pytest.raises(NotImplementedError, match="allow_wide_mlp=True"):
        M.load_lora(CfgNode(cfg), sd, 2, device=DEV)
    bb = M.load_lora(CfgNode(dict(cfg, allow_wide_mlp=True)), sd, 2, device=DEV)      # load_lora passes lora_cfg.allow_wide_mlp
    assert bb.engine.allow_wide_mlp and bb.engine._wide


def test_opt_in_with_narrow_targets_is_the_engine_without_it():
    z, sd, x, dkey = g28()
    runs = []
    for wide in (False, True):
        eng = ViTLoRAEngine(sd, heads=2, r=2, lora_alpha=4, eps=1e-5, device=DEV, target_modules=["q_proj"], generator=torch.Generator().manual_seed(3),
                            lora_dropout=0.05, seed=7, allow_wide_mlp=wide, **OPT_INS)
        eng.lora[:, eng.modules[0].b] = 0.05 * torch.randn(eng.lora[:, eng.modules[0].b].shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        eng.repack()
        key = eng.forward_train(x.to(DEV)).clone()
        grad = eng.backward(dkey.to(DEV)).clone()
        assert not eng._wide and eng._out_flags == 0 and eng.allow_wide_mlp == wide
        runs.append((eng.lora.clone(), key, grad, [w.numel() * w.element_size() for w in eng._tside_ws if w is not None], [m for m in eng.modules]))
    for a, b in zip(*runs):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    assert float(runs[0][2].abs().max()) > 0
