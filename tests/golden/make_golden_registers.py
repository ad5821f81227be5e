"""G21: golden outputs of transformers' Dinov2WithRegistersModel -- the pin of the restatement in tests/registers_ref.py and of the engines' register-token
path.  The G20 recipe (make_golden_swiglu.py): hidden 128, 2 heads x head_dim 64, 3 layers, patch 14, GELU MLP, B = 3; R = 4 register tokens on four grids -- native
(70 px on a 70-px checkpoint), up (70 on 56), down (70 on 98: the target grid is SMALLER than the stored one, where this model's antialias=True widens the
filter) and nonsquare (56 x 84 on 70) -- and one file at R = 1 (native).

Weights: tests/registers_ref.random_registers_state_dict(128, 2, 3, R, image_size=<pre>, seed=21), loaded into the HF model (register tokens ~ N(0, 0.5^2),
LayerScale in [0.1, 1]).  They are NOT stored: the files keep the seed and a SHA-256 of the weights' f32 bytes in key order, which the tests recompute.  Stored:
x, key (the last layer's key projection of the PATCH tokens only, [B, C, h, w]: CLS and the R registers dropped), last_hidden_state, cls_att =
attentions[-1][:, :, 0, 1 + R:] (softmax over all 1 + R + n keys, patch columns kept).

    python tests/golden/make_golden_registers.py      (needs transformers; writes tests/golden/g21_dinov2_registers_{native,up,down,nonsquare,r1}.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (registers_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle, which registers_ref imports)
from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel  # noqa: E402
from registers_ref import G21, G21_B, G21_D, G21_HEADS, G21_LAYERS, G21_SEED, g21_state_dict, weights_sha256  # noqa: E402


def main():
    for tag, ((H, W), pre, R) in G21.items():
        sd = g21_state_dict(tag)
        cfg = Dinov2WithRegistersConfig(hidden_size=G21_D, num_hidden_layers=G21_LAYERS, num_attention_heads=G21_HEADS, image_size=pre, patch_size=14, mlp_ratio=4,
                                        num_register_tokens=R, layer_norm_eps=1e-6, attn_implementation="eager")
        m = Dinov2WithRegistersModel(cfg).eval()
        m.load_state_dict(sd, strict=True)
        keys = {}
        m.encoder.layer[-1].attention.attention.key.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o.detach()))
        x = torch.randn(G21_B, 3, H, W, generator=torch.Generator().manual_seed(G21_SEED))
        with torch.no_grad():
            out = m(x, output_attentions=True)
        k = keys["k"]
        gh, gw = H // 14, W // 14
        assert k.shape[1] == 1 + R + gh * gw
        path = os.path.join(HERE, f"g21_dinov2_registers_{tag}.npz")
        np.savez_compressed(path, x=x.numpy(), key=k[:, 1 + R:].reshape(G21_B, gh, gw, -1).permute(0, 3, 1, 2).numpy(),
                            last_hidden_state=out.last_hidden_state.numpy(), cls_att=out.attentions[-1][:, :, 0, 1 + R:].numpy(),
                            seed=np.int64(G21_SEED), image_size=np.int64(pre), n_reg=np.int64(R), sd_sha256=np.array(weights_sha256(sd)))
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
