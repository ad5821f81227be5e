"""G24: golden key maps and LoRA gradients of transformers' own models (eager attention, f64, CPU) with LoRA on every module of a SwiGLU block the engine can
target -- the pin of the restatement in tests/lora_swiglu_out_ref.py and of backbone-backward mode with the SwiGLU MLP's output projection targeted.

Models (tests/lora_swiglu_out_ref.py, G24_*): ``dinov2`` = Dinov2Model(use_swiglu_ffn=True) at D = 128, 3 layers, the tiny SwiGLU model of
tests/test_gpu_lora_targets.py (hidden width 344: the engine pads to 384), targets query / key / value / weights_in / dense / weights_out; ``gated`` = DINOv3ViTModel
on G22's ``gated`` model, targets q_proj / k_proj / v_proj / o_proj / down_proj.  Weights are not stored, a SHA-256 of their f32 bytes is.  LoRA: r = 2,
lora_alpha = 4, A uniform, B = 0.05 randn, on the output modules lora_out_ref.OUT_B_STD randn; put into transformers' graph by torch.func.functional_call with
W + s B A in place of W, no dropout.  B = 2 images, loss <key, dkey>.

Stored per file: x (f32, rounded to bf16), dkey (f32), ``lora/<name>`` (f32), key (f64), ``grad/<name>`` (f64), sd_sha256, and relative-L2 distances from the f64
values:

  err_f32 / err_bf16ac            the key map of transformers' f32 forward and of its forward under torch.autocast("cpu", bfloat16)
  ebf/<name>                      that gradient from the same autograd under CPU bf16 autocast
  f_<fault>/<name>                that gradient from the restatement in f64 with one fault of the new module (lora_swiglu_out_ref.FAULTS)

The input seed is the first of 24, 25, ... at which every fault lands at least three bars (lora_swiglu_out_ref.grad_bar: max(4e-2, 3 ebf)) from the truth on the
tensors it touches; it must equal lora_swiglu_out_ref.G24_INPUT_SEED.

    python tests/golden/make_golden_lora_swiglu_out.py      (needs transformers >= 5; writes tests/golden/g24_lora_swiglu_out_<tag>.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
from transformers import Dinov2Config, Dinov2Model, DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402


def build(tag):
    """(transformers' model in eval mode with the golden's weights, the module whose output is the key hook)"""
    sd = RS.g24_state_dict(tag)
    if tag == "dinov2":
        cfg = Dinov2Config(hidden_size=128, num_hidden_layers=3, num_attention_heads=RS.G24_HEADS, image_size=70, patch_size=14, mlp_ratio=4, use_swiglu_ffn=True,
                           layer_norm_eps=1e-6, attn_implementation="eager")
        model = Dinov2Model(cfg).eval()
        model.load_state_dict(sd, strict=True)
        return model, model.encoder.layer[-1].attention.attention.key
    m = R3.G22["gated"]
    gh, gw = m["grid"]
    cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=R3.G22_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                          image_size=16 * gh, num_register_tokens=m["R"], use_gated_mlp=True, hidden_act="silu", layer_norm_eps=1e-5, rope_theta=100.0,
                          attn_implementation="eager")
    model = DINOv3ViTModel(cfg).eval()
    model.load_state_dict(sd, strict=True)
    return model, model.model.layer[-1].attention.k_proj


def hf_key_and_grads(model, hook_mod, sd, lora, x, dkey, dtype, autocast=None):
    """(key [B, D, gh, gw], {name: gradient}) of transformers' model with every targeted weight replaced by W + s B A (leaves in ``dtype``)."""
    base = {k: v.to(dtype) for k, v in sd.items()}
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in lora.items()}
    params = dict(base)
    for k in leaves:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            params[mod + ".weight"] = base[mod + ".weight"] + RS.G24_SCALE * leaves[mod + ".lora_B.weight"] @ leaves[k]
    keys = {}
    hook = hook_mod.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o))
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


def one(tag, seed):
    """The golden's arrays at one input seed, or None when a fault does not land three bars away on a tensor it touches."""
    sd, lora = RS.g24_state_dict(tag), RS.g24_lora(tag)
    x, dkey = RS.g24_inputs(tag, seed)
    model, hook_mod = build(tag)
    full = dict(model.state_dict())
    k32, _ = hf_key_and_grads(model, hook_mod, full, lora, x, dkey, torch.float32)
    kbf, gbf = hf_key_and_grads(model, hook_mod, full, lora, x, dkey, torch.float32, autocast=torch.bfloat16)
    if tag == "gated":      # f64 weights and arithmetic on the model's OWN f32 rotary table (make_golden_dinov3.py)
        inv_freq = model.rope_embeddings.inv_freq.clone()
        model.double()
        model.rope_embeddings.inv_freq = inv_freq
    else:
        model.double()
    k64, g64 = hf_key_and_grads(model, hook_mod, {k: v.double() for k, v in full.items()}, lora, x, dkey, torch.float64)
    assert k64.dtype == torch.float64 and k64.shape == dkey.shape
    out = dict(x=x.numpy(), dkey=dkey.numpy(), key=k64.numpy(), lora_seed=np.int64(RS.G24_LORA_SEED), input_seed=np.int64(seed),
               sd_sha256=np.array(R3.weights_sha256(sd)), err_f32=np.float64(R3.rel_l2(k32, k64)), err_bf16ac=np.float64(R3.rel_l2(kbf, k64)))
    own_key, own = RS.g24_grads(tag, x, lora, dkey)
    assert R3.rel_l2(own_key, k64) < 1e-10
    for n, g in g64.items():
        out["lora/" + n] = lora[n].numpy()
        out["grad/" + n] = g.numpy()
        if float(g.abs().max()) == 0.0:
            assert float(own[n].abs().max()) == 0.0 and float(gbf[n].abs().max()) == 0.0, n
            continue
        assert R3.rel_l2(own[n], g) < 1e-9, (n, R3.rel_l2(own[n], g))
        out["ebf/" + n] = np.float64(R3.rel_l2(gbf[n], g))
    ok = True
    for f in RS.FAULTS:
        _, bad = RS.g24_grads(tag, x, lora, dkey, fault=f)
        for n, g in g64.items():
            if float(g.abs().max()) != 0.0:
                out[f"f_{f}/{n}"] = np.float64(R3.rel_l2(bad[n], g))
        hit = RS.touched(tag, f, list(g64))
        assert hit or not RS.TOUCHES[RS.G24_FAMILY[tag]][f], (tag, f)
        for n in hit:
            if float(out[f"f_{f}/{n}"]) < 3.0 * RS.grad_bar(out, n):
                print(f"  {tag} seed {seed}: fault {f} on {n}: {float(out[f'f_{f}/{n}']):.3e} < 3 x {RS.grad_bar(out, n):.3e}")
                ok = False
    return out if ok else None


def main():
    for tag in RS.G24_TAGS:
        for seed in range(24, 40):
            out = one(tag, seed)
            if out is not None:
                break
        else:
            raise SystemExit(f"{tag}: no input seed gives every fault three bars")
        assert seed == RS.G24_INPUT_SEED[tag], (tag, seed, "update lora_swiglu_out_ref.G24_INPUT_SEED")
        path = os.path.join(HERE, f"g24_lora_swiglu_out_{tag}.npz")
        np.savez_compressed(path, **out)
        ebf = [float(v) for k, v in out.items() if k.startswith("ebf/")]
        names = [k[5:] for k in out if k.startswith("grad/")]
        low = {f: min(float(out[f"f_{f}/{n}"]) / RS.grad_bar(out, n) for n in RS.touched(tag, f, names)) for f in RS.FAULTS if RS.touched(tag, f, names)}
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  seed {seed}  key err_f32 {float(out['err_f32']):.2e} err_bf16ac {float(out['err_bf16ac']):.2e}  "
              f"gradients under bf16 autocast {min(ebf):.2e} .. {max(ebf):.2e}  faults, in bars on the tensors they touch: " + "  ".join(f"{f} {v:.1f}" for f, v in low.items()))


if __name__ == "__main__":
    main()
