"""G26: golden key maps and LoRA gradients of transformers' DINOv3ViTModel (eager attention, f64, CPU) with LoRA on q_proj / k_proj / v_proj AND the MLP input
modules -- ``up_proj`` on the plain MLP, ``gate_proj`` / ``up_proj`` on the gated one -- the pin of the restatement in tests/dinov3_lora_mlp_in_ref.py and of
``ViTLoRAEngine(allow_mlp_in=True)``.  Built the way G23 is (make_golden_dinov3_lora.py).

Models: the G22 ones ``g46`` (D = 128, F = 512, plain), ``d256`` (D = 256, F = 1024, plain) and ``gated`` (D = 128, F0 = 384), 3 layers, B = 3 images, a 4 x 6 grid.
LoRA: r = 2, lora_alpha = 4, A kaiming-uniform, B = 0.05 randn (dinov3_lora_mlp_in_ref.g26_lora), put into transformers' graph by torch.func.functional_call with
W + s B A in place of W, no dropout.  Target sets (dinov3_lora_mlp_in_ref.G26_SETS): ``up`` on the plain models; ``gate``, ``up`` and ``both`` on the gated one.

Stored per file: x (f32, rounded to bf16), dkey (f32), ``lora/<name>`` (f32; a target set uses the names of its modules), sd_sha256, and per target set <t>:

  key/<t>, grad/<t>/<name>          transformers' f64 key map and gradients
  err_f32/<t>, err_bf16ac/<t>       relative-L2 error of transformers' f32 key map and of its key map under torch.autocast("cpu", bfloat16)
  ebf/<t>/<name>                    relative-L2 error of that gradient from the same autograd under CPU bf16 autocast

and, in the gated file, for the set ``both``:

  bgrad/<module>.bias               transformers' f64 gradient of the bias of every targeted module that has one (bias="lora_only")
  fault/<f>/<name>                  the gradients of the f64 restatement under one fault of the pair's block structure (dinov3_lora_mlp_in_ref.PAIR_FAULTS).
                                    halves_swapped and dense_b without dropout (their truth is grad/both/<name>); shared_mask from the dropout restatement at
                                    p = 0.05 under the counter-hash masks of seed drop_seed, whose truth is  drop/<name>  (the run the GPU test with dropout on one
                                    stream repeats)

    python tests/golden/make_golden_dinov3_lora_mlp_in.py      (needs transformers >= 5 with models/dinov3_vit; writes tests/golden/g26_dinov3_lora_mlp_in_<tag>.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (dinov3_ref, dinov3_lora_ref, dinov3_lora_mlp_in_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
from transformers import DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_mlp_in_ref as RM  # noqa: E402


def hf_key_and_grads(model, sd, lora, x, dkey, dtype, autocast=None, bias_of=()):
    """(key [B, D, gh, gw], {name: gradient}) of transformers' model with every targeted weight replaced by W + s B A (leaves in ``dtype``); ``bias_of``: bias
    names that are leaves too."""
    base = {k: v.to(dtype) for k, v in sd.items()}
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in lora.items()}
    leaves.update({k: base[k].detach().clone().requires_grad_(True) for k in bias_of})
    params = dict(base)
    for k in leaves:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            params[mod + ".weight"] = base[mod + ".weight"] + RM.G26_SCALE * leaves[mod + ".lora_B.weight"] @ leaves[k]
        elif k.endswith(".bias"):
            params[k] = leaves[k]
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
    for tag in RM.G26_TAGS:
        m = R3.G22[tag]
        sd = R3.g22_state_dict(tag)
        x, dkey = RM.g26_inputs(tag)
        gh, gw = m["grid"]
        cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=R3.G22_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                              image_size=16 * gh, num_register_tokens=m["R"], use_gated_mlp=m["gated"], hidden_act="silu" if m["gated"] else "gelu",
                              layer_norm_eps=1e-5, rope_theta=100.0, attn_implementation="eager")
        model32 = DINOv3ViTModel(cfg).eval()
        model32.load_state_dict(sd, strict=True)
        full = dict(model32.state_dict())                       # (with mask_token, which functional_call wants too)
        model64 = DINOv3ViTModel(cfg).eval()
        model64.load_state_dict(sd, strict=True)
        inv_freq = model64.rope_embeddings.inv_freq.clone()     # f64 weights and arithmetic on the model's OWN f32 rotary table (make_golden_dinov3.py)
        model64.double()
        model64.rope_embeddings.inv_freq = inv_freq
        full64 = {k: v.double() for k, v in full.items()}
        out = dict(x=x.numpy(), dkey=dkey.numpy(), seed=np.int64(RM.G26_SEED), input_seed=np.int64(RM.G26_INPUT_SEED[tag]), sd_sha256=np.array(R3.weights_sha256(sd)),
                   drop_seed=np.uint64(RM.G26_DROP_SEED))
        report = []
        for tset in RM.G26_SETS[tag]:
            lora = RM.g26_lora(tag, RM.g26_targets(tag, tset))
            k32, _ = hf_key_and_grads(model32, full, lora, x, dkey, torch.float32)
            kbf, gbf = hf_key_and_grads(model32, full, lora, x, dkey, torch.float32, autocast=torch.bfloat16)
            k64, g64 = hf_key_and_grads(model64, full64, lora, x, dkey, torch.float64)
            assert k64.dtype == torch.float64 and k64.shape == dkey.shape
            out["key/" + tset] = k64.numpy()
            out["err_f32/" + tset], out["err_bf16ac/" + tset] = np.float64(R3.rel_l2(k32, k64)), np.float64(R3.rel_l2(kbf, k64))
            both = {**sd, **lora}
            own_key, own = RM.grads(x, both, m["heads"], dkey, RM.G26_SCALE)
            assert R3.rel_l2(own_key, k64) < 1e-10
            ebf = []
            for n, g in g64.items():
                out["lora/" + n] = lora[n].numpy()
                out[f"grad/{tset}/{n}"] = g.numpy()
                if float(g.abs().max()) == 0.0:
                    assert float(own[n].abs().max()) == 0.0 and float(gbf[n].abs().max()) == 0.0, n
                    continue
                assert R3.rel_l2(own[n], g) < 1e-9, (n, R3.rel_l2(own[n], g))
                out[f"ebf/{tset}/{n}"] = np.float64(R3.rel_l2(gbf[n], g))
                ebf.append(float(out[f"ebf/{tset}/{n}"]))
            report.append(f"{tset}: key err_f32 {float(out['err_f32/' + tset]):.2e} err_bf16ac {float(out['err_bf16ac/' + tset]):.2e} gradients under bf16 autocast "
                          f"{min(ebf):.2e} .. {max(ebf):.2e}")
            if tset != "both":
                continue
            # bias="lora_only": the biases of the targeted modules that have one
            bias_of = sorted(k[:-len("lora_A.weight")] + "bias" for k in lora if k.endswith("lora_A.weight") and k[:-len("lora_A.weight")] + "bias" in sd)
            _, gb = hf_key_and_grads(model64, full64, lora, x, dkey, torch.float64, bias_of=bias_of)
            _, own_b = RM.grads(x, both, m["heads"], dkey, RM.G26_SCALE, bias_of=bias_of)
            for n in bias_of:
                assert R3.rel_l2(own_b[n], gb[n]) < 1e-9 or float(gb[n].abs().max()) == 0.0, n
                out["bgrad/" + n] = gb[n].numpy()
            # the pair's faults: gradients of the restatement
            tok = 1 + m["R"] + gh * gw
            masks = RM.g26_masks(tag, RM.g26_targets(tag, tset), RM.G26_B * tok)
            _, true_drop = RM.grads(x, both, m["heads"], dkey, RM.G26_SCALE, masks=masks)
            for f in RM.PAIR_FAULTS:
                _, bad = RM.grads(x, both, m["heads"], dkey, RM.G26_SCALE, masks=masks if f == "shared_mask" else None, fault=f)
                for n in g64:
                    out[f"fault/{f}/{n}"] = bad[n].numpy()
            for n in g64:
                out["drop/" + n] = true_drop[n].numpy()
        path = os.path.join(HERE, f"g26_dinov3_lora_mlp_in_{tag}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  " + "  ".join(report))


if __name__ == "__main__":
    main()
