"""G23: golden key maps and LoRA gradients of transformers' DINOv3ViTModel (eager attention, f64, CPU) with LoRA on q_proj / k_proj / v_proj of every layer -- the
pin of the restatement in tests/dinov3_lora_ref.py and of backbone-backward mode on a DINOv3 checkpoint (the rotation of q / k forward, its transpose on dq / dk).

Models: the G22 ones ``g46`` (D = 128, 2 heads, R = 4, 4 x 6 grid) and ``d256`` (D = 256, 4 heads), weights tests/dinov3_ref.g22_state_dict(tag) -- not stored, a
SHA-256 of their f32 bytes is.  LoRA: r = 2, lora_alpha = 4, A kaiming-uniform, B = 0.05 randn (dinov3_lora_ref.g23_lora), put into transformers' graph by
torch.func.functional_call with W + s B A in place of W, no dropout.  B = 3 images, loss <key, dkey>.

Stored per file: x (f32, rounded to bf16), dkey (f32), ``lora/<name>`` (f32), key (f64), ``grad/<name>`` (f64), sd_sha256, and relative-L2 distances from the f64
values:

  err_f32 / err_bf16ac            the key map of transformers' f32 forward and of its forward under torch.autocast("cpu", bfloat16)
  ebf/<name>                      that gradient from the same autograd under CPU bf16 autocast
  bf_<fault>/<name>               that gradient from the restatement in f64 with one BACKWARD fault (dinov3_lora_ref.BWD_FAULTS)
  fault_<name>                    the key map from the restatement with one FORWARD fault (dinov3_ref.FAULTS)

    python tests/golden/make_golden_dinov3_lora.py      (needs transformers >= 5 with models/dinov3_vit; writes tests/golden/g23_dinov3_lora_<tag>.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (dinov3_ref, dinov3_lora_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
from transformers import DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402


def hf_key_and_grads(model, sd, lora, x, dkey, dtype, autocast=None):
    """(key [B, D, gh, gw], {name: gradient}) of transformers' model with every targeted weight replaced by W + s B A (leaves in ``dtype``)."""
    base = {k: v.to(dtype) for k, v in sd.items()}
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in lora.items()}
    params = dict(base)
    for k in leaves:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            params[mod + ".weight"] = base[mod + ".weight"] + RL.G23_SCALE * leaves[mod + ".lora_B.weight"] @ leaves[k]
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
    for tag in RL.G23_TAGS:
        m = R3.G22[tag]
        sd = R3.g22_state_dict(tag)
        lora = RL.g23_lora(tag)
        x, dkey = RL.g23_inputs(tag)
        gh, gw = m["grid"]
        cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=R3.G22_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                              image_size=16 * gh, num_register_tokens=m["R"], use_gated_mlp=m["gated"], hidden_act="silu" if m["gated"] else "gelu",
                              layer_norm_eps=1e-5, rope_theta=100.0, attn_implementation="eager")
        model = DINOv3ViTModel(cfg).eval()
        model.load_state_dict(sd, strict=True)
        full = dict(model.state_dict())                         # (with mask_token, which functional_call wants too)
        k32, _ = hf_key_and_grads(model, full, lora, x, dkey, torch.float32)
        kbf, gbf = hf_key_and_grads(model, full, lora, x, dkey, torch.float32, autocast=torch.bfloat16)
        # f64 weights and arithmetic on the model's OWN f32 rotary table (make_golden_dinov3.py: the inv_freq buffer is put back after .double())
        inv_freq = model.rope_embeddings.inv_freq.clone()
        model.double()
        model.rope_embeddings.inv_freq = inv_freq
        full64 = {k: v.double() for k, v in full.items()}
        k64, g64 = hf_key_and_grads(model, full64, lora, x, dkey, torch.float64)
        assert k64.dtype == torch.float64 and k64.shape == dkey.shape
        out = dict(x=x.numpy(), dkey=dkey.numpy(), key=k64.numpy(), seed=np.int64(RL.G23_SEED), input_seed=np.int64(RL.G23_INPUT_SEED[tag]), sd_sha256=np.array(R3.weights_sha256(sd)),
                   err_f32=np.float64(R3.rel_l2(k32, k64)), err_bf16ac=np.float64(R3.rel_l2(kbf, k64)))
        both = {**sd, **lora}
        own_key, own = RL.lora_grads(x, both, m["heads"], dkey, RL.G23_SCALE)
        assert R3.rel_l2(own_key, k64) < 1e-10
        for n, g in g64.items():
            out["lora/" + n] = lora[n].numpy()
            out["grad/" + n] = g.numpy()
            if float(g.abs().max()) == 0.0:
                assert float(own[n].abs().max()) == 0.0 and float(gbf[n].abs().max()) == 0.0, n
                continue
            assert R3.rel_l2(own[n], g) < 1e-9, (n, R3.rel_l2(own[n], g))
            out["ebf/" + n] = np.float64(R3.rel_l2(gbf[n], g))
        for f in RL.BWD_FAULTS:
            _, bad = RL.lora_grads(x, both, m["heads"], dkey, RL.G23_SCALE, bwd_fault=f)
            for n, g in g64.items():
                if float(g.abs().max()) != 0.0:
                    out[f"bf_{f}/{n}"] = np.float64(R3.rel_l2(bad[n], g))
        for f in R3.FAULTS:
            out["fault_" + f] = np.float64(R3.rel_l2(RL.forward(x.double(), {k: v.double() for k, v in both.items()}, m["heads"], RL.G23_SCALE, fault=f), k64))
        # what makes the key map of the GPU test a pin (dinov3_lora_ref.G23_INPUT_SEED): the engine's bound lies under half the smallest forward fault
        assert 3.0 * float(out["err_bf16ac"]) < 0.5 * min(float(out["fault_" + f]) for f in R3.FAULTS), (tag, "pick the next input seed")
        path = os.path.join(HERE, f"g23_dinov3_lora_{tag}.npz")
        np.savez_compressed(path, **out)
        ebf = [float(v) for k, v in out.items() if k.startswith("ebf/")]
        hit = [float(out[f"bf_{f}/{n}"]) for f in RL.BWD_FAULTS for n in g64 if f"bf_{f}/{n}" in out and n.split(".")[2] != str(R3.G22_LAYERS - 1)
               and n.split(".")[4] in RL.TOUCHES[f]]
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  key err_f32 {float(out['err_f32']):.2e} err_bf16ac {float(out['err_bf16ac']):.2e}  "
              f"gradients under bf16 autocast {min(ebf):.2e} .. {max(ebf):.2e}  touched q / k gradients under a backward fault {min(hit):.2f} .. {max(hit):.2f}  " +
              "  ".join(f"{k} {float(v):.2e}" for k, v in out.items() if k.startswith("fault_")))


if __name__ == "__main__":
    main()
