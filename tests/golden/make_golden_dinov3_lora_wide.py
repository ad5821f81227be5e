"""G28: golden key maps and LoRA gradients of transformers' DINOv3ViTModel (eager attention, f64, CPU) on a gated model whose MLP is as wide as
dinov3_vith16plus's -- hidden 5120, so N1 = 10240 rows of the fused weights_in and K = 5120 columns of down_proj -- the pin of the restatement in
tests/lora_wide_ref.py and of ``ViTLoRAEngine(allow_wide_mlp=True)``.  Built the way G26 is (make_golden_dinov3_lora_mlp_in.py; peft is not needed: W + s B A stands
in the weight's place through torch.func.functional_call).

Model (lora_wide_ref.G28): D = 128, 2 heads, 4 registers, F = 5120 gated, 2 layers, B = 3 images of 64 x 96 (a 4 x 6 grid).  LoRA: r = 2, lora_alpha = 4, no dropout.
Neither the state dict, nor the inputs, nor the LoRA tensors are stored: all three are drawn from stored seeds (the state dict is pinned by its sha256).
Target sets (lora_wide_ref.G28_SETS): ``pair`` (gate_proj, up_proj), ``down`` (down_proj), ``every`` (all seven Linears).  Stored per set <t>, in f32:

  key/<t>, grad/<t>/<name>          transformers' f64 key map and gradients
  err_f32/<t>, err_bf16ac/<t>       relative-L2 error of transformers' f32 key map and of its key map under torch.autocast("cpu", bfloat16)
  ebf/<t>/<name>                    relative-L2 error of that gradient from the same autograd under CPU bf16 autocast
  mut/<m>/<t>/key, mut/<m>/<t>/<name>   relative-L2 distance from the truth of the restatement's key map and gradients under mutation <m> (lora_wide_ref.MUTATIONS;
                                    t_8192 only where gate_proj / up_proj are targeted; a gradient whose truth is zero, or that the mutation removes, is not listed)

    python tests/golden/make_golden_dinov3_lora_wide.py      (needs transformers >= 5 with models/dinov3_vit; writes tests/golden/g28_dinov3_lora_wide.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (dinov3_ref, lora_wide_ref, ...)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
from transformers import DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import lora_wide_ref as RW  # noqa: E402


def hf_key_and_grads(model, sd, lora, x, dkey, dtype, autocast=None):
    """(key [B, D, gh, gw], {name: gradient}) of transformers' model with every targeted weight replaced by W + s B A (leaves in ``dtype``)"""
    base = {k: v.to(dtype) for k, v in sd.items()}
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in lora.items()}
    params = dict(base)
    for k in leaves:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            params[mod + ".weight"] = base[mod + ".weight"] + RW.G28_SCALE * leaves[mod + ".lora_B.weight"] @ leaves[k]
    keys = {}
    hook = model.model.layer[-1].attention.k_proj.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o))
    try:
        if autocast is None:
            torch.func.functional_call(model, params, (x.to(dtype),))
        else:
            with torch.autocast("cpu", dtype=autocast):
                torch.func.functional_call(model, params, (x.to(dtype),))
    finally:
        hook.remove()
    k = keys["k"]
    B, D, gh, gw = dkey.shape
    key = k[:, k.shape[1] - gh * gw:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
    names = sorted(leaves)
    grads = torch.autograd.grad((key.to(dtype) * dkey.to(dtype)).sum(), [leaves[n] for n in names], allow_unused=True)
    return key.detach(), {n: (torch.zeros_like(leaves[n]) if g is None else g.detach()) for n, g in zip(names, grads)}


def main():
    m = RW.G28
    sd = RW.g28_state_dict()
    x, dkey = RW.g28_inputs()
    gh, gw = m["grid"]
    cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=RW.G28_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                          image_size=16 * gh, num_register_tokens=m["R"], use_gated_mlp=True, hidden_act="silu", layer_norm_eps=1e-5, rope_theta=100.0,
                          attn_implementation="eager")
    model32 = DINOv3ViTModel(cfg).eval()
    model32.load_state_dict(sd, strict=True)
    full = dict(model32.state_dict())                           # (with mask_token, which functional_call wants too)
    model64 = DINOv3ViTModel(cfg).eval()
    model64.load_state_dict(sd, strict=True)
    inv_freq = model64.rope_embeddings.inv_freq.clone()         # f64 weights and arithmetic on the model's OWN f32 rotary table (make_golden_dinov3.py)
    model64.double()
    model64.rope_embeddings.inv_freq = inv_freq
    full64 = {k: v.double() for k, v in full.items()}
    out = dict(seed=np.int64(RW.G28_SEED), input_seed=np.int64(RW.G28_INPUT_SEED), lora_seed=np.int64(RW.G28_LORA_SEED), sd_sha256=np.array(R3.weights_sha256(sd)))
    report = []
    for tset, leaves in RW.G28_SETS.items():
        lora = RW.g28_lora(leaves)
        k32, _ = hf_key_and_grads(model32, full, lora, x, dkey, torch.float32)
        kbf, gbf = hf_key_and_grads(model32, full, lora, x, dkey, torch.float32, autocast=torch.bfloat16)
        k64, g64 = hf_key_and_grads(model64, full64, lora, x, dkey, torch.float64)
        assert k64.dtype == torch.float64 and k64.shape == dkey.shape
        out["key/" + tset] = k64.numpy().astype(np.float32)
        out["err_f32/" + tset], out["err_bf16ac/" + tset] = np.float64(R3.rel_l2(k32, k64)), np.float64(R3.rel_l2(kbf, k64))
        both = {**sd, **lora}
        own_key, own = RW.grads(x, both, dkey)
        assert R3.rel_l2(own_key, k64) < 1e-10
        ebf = []
        for n, g in g64.items():
            out[f"grad/{tset}/{n}"] = g.numpy().astype(np.float32)
            if float(g.abs().max()) == 0.0:
                assert float(own[n].abs().max()) == 0.0 and float(gbf[n].abs().max()) == 0.0, n
                continue
            assert R3.rel_l2(own[n], g) < 1e-9, (n, R3.rel_l2(own[n], g))
            out[f"ebf/{tset}/{n}"] = np.float64(R3.rel_l2(gbf[n], g))
            ebf.append(float(out[f"ebf/{tset}/{n}"]))
        line = f"{tset}: key err_f32 {float(out['err_f32/' + tset]):.2e} err_bf16ac {float(out['err_bf16ac/' + tset]):.2e} gradients under bf16 autocast {min(ebf):.2e} .. {max(ebf):.2e}"
        for mut in RW.MUTATIONS:
            if mut == "t_8192" and tset == "down":
                continue
            bad_key, bad = RW.grads(x, both, dkey, mutation=mut)
            out[f"mut/{mut}/{tset}/key"] = np.float64(R3.rel_l2(bad_key, k64))
            dist = {n: R3.rel_l2(bad[n], g64[n]) for n in bad if float(g64[n].abs().max()) != 0.0}
            for n, d in dist.items():
                out[f"mut/{mut}/{tset}/{n}"] = np.float64(d)
            line += f"; {mut}: key {float(out[f'mut/{mut}/{tset}/key']):.2e}" + (f", gradients {min(dist.values()):.2e} .. {max(dist.values()):.2e}" if dist else "")
        report.append(line)
    path = os.path.join(HERE, "g28_dinov3_lora_wide.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
