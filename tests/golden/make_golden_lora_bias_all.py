"""G27: what peft's ``bias="all"`` selects on transformers' own module trees, and the gradients of those parameters (eager attention, f64, CPU) -- the pin of the
name rule and of the restatement in tests/lora_bias_all_ref.py, independent of the project's own forwards.

Models: ``dinov2`` = Dinov2Model(use_swiglu_ffn=True) at D = 128, 3 layers (the G24 model of tests/golden/make_golden_lora_swiglu_out.py) with LoRA on query / key /
value / weights_in / dense / weights_out (G24's matrices and inputs); ``dinov3`` = DINOv3ViTModel on G22's ``gated`` model with LoRA on q_proj / k_proj / v_proj /
gate_proj / up_proj (G26's matrices and inputs, tests/dinov3_lora_mlp_in_ref.py).  LoRA goes into transformers' graph as make_golden_lora_swiglu_out.py puts it:
torch.func.functional_call with W + s B A in place of W, no dropout.  Loss <key, dkey>, key = the last layer's key projection on the patch tokens.

Stored per file: ``names`` = the ``named_parameters()`` names containing "bias", in the model's order (peft's rule for bias="all": requires_grad on exactly these);
``grad/<name>`` (f64) for each -- zeros where autograd returns None (the final LayerNorm and the last layer's biases other than the key's and norm1's) and
``none/<name>`` = 1 there; x (f32), dkey (f32), ``lora/<name>`` (f32), key (f64), sd_sha256.

    python tests/golden/make_golden_lora_bias_all.py      (needs transformers >= 5; writes tests/golden/g27_lora_bias_all_{dinov2,dinov3}.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
import make_golden_lora_swiglu_out as G24  # noqa: E402  (its ``build``: the two transformers models)
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_mlp_in_ref as RM  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402


def case(tag):
    """(build tag of make_golden_lora_swiglu_out, state dict, LoRA matrices, scale, inputs)"""
    if tag == "dinov2":
        return "dinov2", RS.g24_state_dict("dinov2"), RS.g24_lora("dinov2"), RS.G24_SCALE, RS.g24_inputs("dinov2", RS.G24_INPUT_SEED["dinov2"])
    leaves = RM.g26_targets("gated", "both")
    return "gated", R3.g22_state_dict("gated"), RM.g26_lora("gated", leaves), RM.G26_SCALE, RM.g26_inputs("gated")


def one(tag):
    btag, sd, lora, scale, (x, dkey) = case(tag)
    model, hook_mod = G24.build(btag)
    names = [n for n, _ in model.named_parameters() if "bias" in n]
    if btag == "gated":      # f64 weights and arithmetic on the model's OWN f32 rotary table (make_golden_dinov3.py)
        inv_freq = model.rope_embeddings.inv_freq.clone()
        model.double()
        model.rope_embeddings.inv_freq = inv_freq
    else:
        model.double()
    params = {k: v.detach().double() for k, v in model.state_dict().items()}
    leaves = {n: params[n].clone().requires_grad_(True) for n in names}
    params.update(leaves)
    for k, a in lora.items():
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            params[mod + ".weight"] = params[mod + ".weight"] + scale * lora[mod + ".lora_B.weight"].double() @ a.double()
    keys = {}
    hook = hook_mod.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o))
    try:
        torch.func.functional_call(model, params, (x.double(),))
    finally:
        hook.remove()
    k = keys["k"]
    B, D, gh, gw = dkey.shape
    key = k[:, k.shape[1] - gh * gw:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
    grads = torch.autograd.grad((key * dkey.double()).sum(), [leaves[n] for n in names], allow_unused=True)
    out = dict(names=np.array(names), x=x.numpy(), dkey=dkey.numpy(), key=key.detach().numpy(), scale=np.float64(scale), sd_sha256=np.array(R3.weights_sha256(sd)))
    for n, g in zip(names, grads):
        out["grad/" + n] = (torch.zeros_like(leaves[n]) if g is None else g.detach()).numpy()
        out["none/" + n] = np.int64(g is None)
    for n, v in lora.items():
        out["lora/" + n] = v.numpy()
    return out


def main():
    for tag in ("dinov2", "dinov3"):
        out = one(tag)
        path = os.path.join(HERE, f"g27_lora_bias_all_{tag}.npz")
        np.savez_compressed(path, **out)
        none = [n for n in out["names"] if int(out["none/" + n])]
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  {len(out['names'])} bias parameters, {len(none)} without a gradient: {none}")


if __name__ == "__main__":
    main()
