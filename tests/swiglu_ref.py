"""Test helper: the DINOv2 forward with the SwiGLU MLP of ViT-g/14 (transformers modeling_dinov2.py:300-315, Dinov2SwiGLUFFN; selected by
config.use_swiglu_ffn, :355), restated on a flat HF-named state dict.  Everything but the MLP is oracle.vit's (layer_norm, attention, dinov2_pos_embed);
the arithmetic runs in the dtype of the inputs (f32 or f64)."""
import torch
import torch.nn.functional as F

from oracle import vit as OV


def swiglu_hidden(D, mlp_ratio=4):
    """modeling_dinov2.py:304-305."""
    return (int(int(D * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def swiglu_mlp(h, sd, p):
    """hidden = silu(x1) * x2, (x1, x2) = weights_in(h).chunk(2); weights_out(hidden)."""
    y = h @ sd[p + "mlp.weights_in.weight"].t() + sd[p + "mlp.weights_in.bias"]
    x1, x2 = y.chunk(2, dim=-1)
    return (F.silu(x1) * x2) @ sd[p + "mlp.weights_out.weight"].t() + sd[p + "mlp.weights_out.bias"]


def dinov2_swiglu_forward(img, sd, heads, patch=14, eps=1e-6, n_layers=None, full_last_layer=True):
    """(last_hidden_state after the final LayerNorm or None, key [B, D, h, w], cls_att [B, heads, h w] of the last layer)."""
    B, _, H, W = img.shape
    pre = "embeddings."
    x = OV.patch_embed(img, sd[pre + "patch_embeddings.projection.weight"], sd[pre + "patch_embeddings.projection.bias"], patch)
    x = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), x), 1)
    x = x + OV.dinov2_pos_embed(sd[pre + "position_embeddings"], H // patch, W // patch)
    L = n_layers if n_layers is not None else 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    gh, gw = H // patch, W // patch
    key = cls_att = None
    for i in range(L):
        p = f"encoder.layer.{i}."
        a = p + "attention.attention."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        q = h @ sd[a + "query.weight"].t() + sd[a + "query.bias"]
        k = h @ sd[a + "key.weight"].t() + sd[a + "key.bias"]
        if i == L - 1:
            key = k
            hd = q.shape[-1] // heads
            qc = q[:, 0].reshape(B, heads, hd)
            kk = k.reshape(B, -1, heads, hd).transpose(1, 2)
            cls_att = torch.softmax(torch.einsum("bhd,bhnd->bhn", qc, kk) * hd ** -0.5, -1)[:, :, 1:]
            if not full_last_layer:
                break
        v = h @ sd[a + "value.weight"].t() + sd[a + "value.bias"]
        o = OV.attention(q, k, v, heads)
        o = o @ sd[p + "attention.output.dense.weight"].t() + sd[p + "attention.output.dense.bias"]
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        x = swiglu_mlp(h, sd, p) * sd[p + "layer_scale2.lambda1"] + x
    last = OV.layer_norm(x, sd["layernorm.weight"], sd["layernorm.bias"], eps) if full_last_layer else None
    return last, key[:, 1:, :].reshape(B, gh, gw, -1).permute(0, 3, 1, 2), cls_att


def random_swiglu_state_dict(D, heads, L, patch=14, image_size=70, seed=0, ls=(0.1, 1.0)):
    """HF-named SwiGLU DINOv2 weights (Dinov2Model with use_swiglu_ffn=True) at any width: trunc-normal 0.02 matrices, non-trivial LayerNorm / LayerScale /
    biases (what the G8 goldens do to an HF init), F = swiglu_hidden(D) -- 344 at D = 128, so the padding to 384 is exercised."""
    g = torch.Generator().manual_seed(seed)
    tn = lambda *s: torch.nn.init.trunc_normal_(torch.empty(*s), std=0.02, a=-0.04, b=0.04, generator=g)  # noqa: E731
    rn = lambda *s: 0.1 * torch.randn(*s, generator=g)  # noqa: E731
    n = (image_size // patch) ** 2
    Fh = swiglu_hidden(D)
    sd = {"embeddings.cls_token": 0.05 * torch.randn(1, 1, D, generator=g), "embeddings.position_embeddings": 0.05 * torch.randn(1, n + 1, D, generator=g),
          "embeddings.patch_embeddings.projection.weight": tn(D, 3, patch, patch), "embeddings.patch_embeddings.projection.bias": rn(D),
          "embeddings.mask_token": torch.zeros(1, D)}
    for i in range(L):
        p = f"encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            sd[p + f"attention.attention.{nm}.weight"], sd[p + f"attention.attention.{nm}.bias"] = tn(D, D), rn(D)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = tn(D, D), rn(D)
        sd[p + "mlp.weights_in.weight"], sd[p + "mlp.weights_in.bias"] = tn(2 * Fh, D), rn(2 * Fh)
        sd[p + "mlp.weights_out.weight"], sd[p + "mlp.weights_out.bias"] = tn(D, Fh), rn(D)
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = 1.0 + rn(D), rn(D)
        sd[p + "layer_scale1.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
        sd[p + "layer_scale2.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
    sd["layernorm.weight"], sd["layernorm.bias"] = 1.0 + rn(D), rn(D)
    return sd
