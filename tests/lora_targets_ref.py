"""Test helper: the DINOv2 forward with peft-style LoRA on any of query / key / value and the MLP input projection (``fc1`` of the GELU MLP, ``weights_in`` of
the SwiGLU one; models/modules/full_model.py:47-72 hands ``target_modules`` to peft), restated on a flat HF-named state dict.  A module carries LoRA when the
state dict holds ``<module>.lora_A.weight`` [r, in] and ``<module>.lora_B.weight`` [out, r] (HF row order):

    y = base(x) + lora_B(lora_A(dropout(x))) * alpha / r

``masks`` maps (layer, "query" | "key" | "value" | "fc1" | "weights_in") to the [rows, D] dropout mask (0 or 1 / (1 - p)) of that module's LoRA input.
Everything but the LoRA branch is oracle.vit's / swiglu_ref's arithmetic; it runs in the dtype and on the device of the inputs."""
import torch
import torch.nn.functional as F

from oracle import vit as OV


def lora_linear(h, sd, name, scale, mask=None):
    y = h @ sd[name + ".weight"].t() + sd[name + ".bias"]
    if name + ".lora_A.weight" in sd:
        hd = h if mask is None else h * mask.to(h).reshape(h.shape)
        y = y + ((hd @ sd[name + ".lora_A.weight"].t()) @ sd[name + ".lora_B.weight"].t()) * scale
    return y


def forward(img, sd, heads, lora_scale, masks=None, patch=14, eps=1e-6):
    """The key map [B, D, h, w] of the last layer's key projection (key-minimal: the last layer's query / value / MLP never run)."""
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    pre = "embeddings."
    x = OV.patch_embed(img, sd[pre + "patch_embeddings.projection.weight"], sd[pre + "patch_embeddings.projection.bias"], patch)
    x = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), x), 1)
    x = x + OV.dinov2_pos_embed(sd[pre + "position_embeddings"], gh, gw).to(x)
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    swiglu = "encoder.layer.0.mlp.weights_in.weight" in sd
    m = (lambda i, nm: None) if masks is None else (lambda i, nm: masks.get((i, nm)))
    for i in range(L):
        p = f"encoder.layer.{i}."
        a = p + "attention.attention."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = lora_linear(h, sd, a + "key", lora_scale, m(i, "key"))
        if i == L - 1:
            return k[:, 1:, :].reshape(B, gh, gw, -1).permute(0, 3, 1, 2)
        q = lora_linear(h, sd, a + "query", lora_scale, m(i, "query"))
        v = lora_linear(h, sd, a + "value", lora_scale, m(i, "value"))
        o = OV.attention(q, k, v, heads)
        o = o @ sd[p + "attention.output.dense.weight"].t() + sd[p + "attention.output.dense.bias"]
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        if swiglu:
            x1, x2 = lora_linear(h, sd, p + "mlp.weights_in", lora_scale, m(i, "weights_in")).chunk(2, dim=-1)
            h = (F.silu(x1) * x2) @ sd[p + "mlp.weights_out.weight"].t() + sd[p + "mlp.weights_out.bias"]
        else:
            h = OV.gelu_erf(lora_linear(h, sd, p + "mlp.fc1", lora_scale, m(i, "fc1")))
            h = h @ sd[p + "mlp.fc2.weight"].t() + sd[p + "mlp.fc2.bias"]
        x = h * sd[p + "layer_scale2.lambda1"] + x
    raise AssertionError("unreachable")


def lora_grads(img, sd, heads, dkey, lora_scale, masks=None, dtype=torch.float64, device="cpu"):
    """(key, {LoRA parameter name: gradient of <key, dkey>}) by autograd over ``forward`` in ``dtype`` on ``device``; a matrix the key map does not depend on
    gets zeros."""
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    names = sorted(k for k in sdd if ".lora_" in k)
    for k in names:
        sdd[k].requires_grad_(True)
    key = forward(img.to(device, dtype), sdd, heads, lora_scale, masks)
    grads = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if g is None else g) for k, g in zip(names, grads)}


def merged_grads(img, sd, heads, dkey, lora_scale, dtype=torch.float64, device="cpu"):
    """The same without dropout through the merged weights W + alpha/r * B A of a LoRA-free forward: the second route the restatement is pinned on."""
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    names = sorted(k for k in sdd if ".lora_" in k)
    for k in names:
        sdd[k].requires_grad_(True)
    plain = {k: v for k, v in sdd.items() if ".lora_" not in k}
    for k in names:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            plain[mod + ".weight"] = plain[mod + ".weight"] + lora_scale * sdd[mod + ".lora_B.weight"] @ sdd[k]
    key = forward(img.to(device, dtype), plain, heads, lora_scale)
    grads = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if g is None else g) for k, g in zip(names, grads)}
