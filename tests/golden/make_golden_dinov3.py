"""G22: golden outputs of transformers' DINOv3ViTModel (eager attention, f64, CPU) -- the pin of the restatement in tests/dinov3_ref.py and of the engines'
rotary-position-embedding path.  Tiny models (3 layers, patch 16, head_dim 64, theta 100, eps 1e-5, B = 2): D = 128 / 2 heads / GELU with R = 4 register tokens on
a 4 x 6 grid (64 x 96 px: non-square) and on 6 x 6, the same at R = 1 and R = 0, D = 256 / 4 heads (where LayerNorm folds into the GEMMs), and D = 128 with the
gated MLP at F = 384.

Weights: tests/dinov3_ref.g22_state_dict(tag), PEAKED (q / k weights and the q bias times 8, LayerScale in [0.1, 1], non-zero v / o / MLP biases): on the flat
trunc-normal init a pass with no rotation at all is only ~7e-4 (relative L2) from the true key map, the size of the fp16 engine's own error; at gain 8 every
fault below is tens of times that.  Like G21 they are NOT stored (a D = 256 model alone is 3 MB of f32): the files keep the seed and a SHA-256 of the weights'
f32 bytes in key order, which the tests recompute.  Stored per file: x (f32; values rounded to bf16), key (f64: the last layer's k_proj output on the patch tokens,
[B, D, gh, gw], before rotation), and relative-L2 distances from that key map:

  err_f32 / err_f16ac / err_bf16ac   transformers' own f32 forward, and its forward under torch.autocast("cpu", float16 / bfloat16)
  fault_<name>                       the restatement in f64 with one fault switched on (dinov3_ref.FAULTS: no rotation, y / x blocks swapped, sine sign
                                     flipped, prefix tokens rotated too)

    python tests/golden/make_golden_dinov3.py      (needs transformers >= 5 with models/dinov3_vit; writes tests/golden/g22_dinov3_<tag>.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (dinov3_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle, which dinov3_ref imports)
from transformers import DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
import dinov3_ref as R3  # noqa: E402


def hf_key(model, x, autocast=None):
    keys = {}
    hook = model.model.layer[-1].attention.k_proj.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o.detach()))
    with torch.no_grad():
        if autocast is None:
            model(x)
        else:
            with torch.autocast("cpu", dtype=autocast):
                model(x)
    hook.remove()
    return keys["k"]


def main():
    for tag, m in R3.G22.items():
        sd = R3.g22_state_dict(tag)
        gh, gw = m["grid"]
        cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=R3.G22_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                              image_size=16 * gh, num_register_tokens=m["R"], use_gated_mlp=m["gated"], hidden_act="silu" if m["gated"] else "gelu",
                              layer_norm_eps=1e-5, rope_theta=100.0, attn_implementation="eager")
        model = DINOv3ViTModel(cfg).eval()
        model.load_state_dict(sd, strict=True)
        x = R3.g22_input(tag)
        nlead = 1 + m["R"]
        shape = lambda k: k[:, nlead:].reshape(R3.G22_B, gh, gw, -1).permute(0, 3, 1, 2)  # noqa: E731
        k32 = shape(hf_key(model, x))
        k16 = shape(hf_key(model, x, torch.float16))
        kb16 = shape(hf_key(model, x, torch.bfloat16))
        # (f64 weights and arithmetic on the model's OWN rotary table: .double() would also widen the inv_freq buffer and with it the angles, which the f32 model --
        # and every engine -- computes in f32; the buffer is put back so that cos / sin are the f32 values, cast)
        inv_freq = model.rope_embeddings.inv_freq.clone()
        model.double()
        model.rope_embeddings.inv_freq = inv_freq
        k64 = shape(hf_key(model, x.double()))
        assert k64.dtype == torch.float64 and k64.shape == (R3.G22_B, m["D"], gh, gw)
        out = dict(x=x.numpy(), key=k64.numpy(), seed=np.int64(R3.G22_SEED), gain=np.float64(R3.G22_GAIN), n_reg=np.int64(m["R"]),
                   sd_sha256=np.array(R3.weights_sha256(sd)), err_f32=np.float64(R3.rel_l2(k32, k64)), err_f16ac=np.float64(R3.rel_l2(k16, k64)),
                   err_bf16ac=np.float64(R3.rel_l2(kb16, k64)))
        own = R3.rel_l2(R3.forward_f64(x, sd, m["heads"]), k64)
        assert own < 1e-10, own
        for f in R3.FAULTS:
            out["fault_" + f] = np.float64(R3.rel_l2(R3.forward_f64(x, sd, m["heads"], fault=f), k64))
        path = os.path.join(HERE, f"g22_dinov3_{tag}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  restatement {own:.1e}  " +
              "  ".join(f"{k} {float(v):.2e}" for k, v in out.items() if k.startswith(("err_", "fault_"))))


if __name__ == "__main__":
    main()
