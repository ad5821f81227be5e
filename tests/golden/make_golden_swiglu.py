"""G20: golden outputs of transformers' Dinov2Model with the SwiGLU MLP (use_swiglu_ffn=True, modeling_dinov2.py:300-315,355) -- the pin of the restatement in
tests/swiglu_ref.py and of the engines' SwiGLU path.  The G8 recipe (make_golden.py, g8): hidden 128, 2 heads x head_dim 64, 3 layers, mlp_ratio 4 (F = 344, so the
engines' padding to 384 is exercised), a native grid (70 px on a 70 px pre-training grid) and an interpolated one (70 px on 56).

Weights: tests/swiglu_ref.random_swiglu_state_dict(128, 2, 3, image_size=<pre>, seed=20), loaded into the HF model.  They are NOT stored (3 layers of SwiGLU
weights are 2.4 MB in f32, over the size limit of a committed file): the files keep the seed, and a SHA-256 of the weights' f32 bytes in key order, which the
tests recompute, so a change of the generator fails loudly instead of comparing against other weights.  Stored: x, key (the last layer's key projection as the
reference's hook captures it, [B, C, h, w]), last_hidden_state, cls_att (the last layer's CLS attention row over the patch tokens, [B, heads, h w]).

    python tests/golden/make_golden_swiglu.py      (needs transformers; writes tests/golden/g20_dinov2_swiglu_{native,interp}.npz)
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (swiglu_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle, which swiglu_ref imports)
from transformers import Dinov2Config, Dinov2Model  # noqa: E402
from swiglu_ref import random_swiglu_state_dict  # noqa: E402

SEED, D, HEADS, LAYERS = 20, 128, 2, 3
GRIDS = {"native": (70, 70), "interp": (70, 56)}


def weights_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    for tag, (img, pre) in GRIDS.items():
        sd = random_swiglu_state_dict(D, HEADS, LAYERS, image_size=pre, seed=SEED)
        cfg = Dinov2Config(hidden_size=D, num_hidden_layers=LAYERS, num_attention_heads=HEADS, image_size=pre, patch_size=14, mlp_ratio=4,
                           use_swiglu_ffn=True, layer_norm_eps=1e-6, attn_implementation="eager")
        m = Dinov2Model(cfg).eval()
        m.load_state_dict(sd, strict=True)
        keys = {}
        m.encoder.layer[-1].attention.attention.key.register_forward_hook(lambda mod_, i, o: keys.__setitem__("k", o.detach()))
        x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(SEED))
        with torch.no_grad():
            out = m(x, output_attentions=True)
        k = keys["k"]
        g = img // 14
        path = os.path.join(HERE, f"g20_dinov2_swiglu_{tag}.npz")
        np.savez_compressed(path, x=x.numpy(), key=k[:, 1:].reshape(2, g, g, -1).permute(0, 3, 1, 2).numpy(),
                            last_hidden_state=out.last_hidden_state.numpy(), cls_att=out.attentions[-1][:, :, 0, 1:].numpy(),
                            seed=np.int64(SEED), image_size=np.int64(pre), sd_sha256=np.array(weights_sha256(sd)))
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
