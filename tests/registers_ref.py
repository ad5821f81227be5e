"""Test helper: the forward of DINOv2 with registers (transformers models/dinov2_with_registers/modeling_dinov2_with_registers.py, Dinov2WithRegistersModel),
restated on a flat HF-named state dict, with peft-style LoRA on query / key / value / fc1 (tests/lora_targets_ref.py's convention) for the autograd references.

What differs from plain DINOv2 (Dinov2WithRegistersEmbeddings.forward): the token sequence of an image is [CLS | R register tokens | n patches]; CLS gets
``cls + pos[0]``, patch p ``patch + pos[1 + p]``, register j is ``register_tokens[j]`` with NO position row; the position rows are interpolated with
``antialias=True`` (bicubic, align_corners=False, explicit size, in f32): a wider filter when the target grid is smaller than the stored one, and torch's
antialiased cubic coefficient (-0.5, not -0.75) on every interpolated grid.  The encoder layers are plain DINOv2's.  The key map drops CLS AND the registers; the CLS attention row is the softmax over all 1 + R + n keys with the patch columns kept.

Everything but the embeddings is oracle.vit's arithmetic; it runs in the dtype and on the device of the inputs (f32 against the goldens, f64 as a reference).
Nothing under ucod_dpl_amd/ imports this file."""
import hashlib

import torch
import torch.nn.functional as F

from oracle import vit as OV
from lora_targets_ref import lora_linear


def pos_embed(pos, gh, gw, antialias=True):
    """Dinov2WithRegistersEmbeddings.interpolate_pos_encoding: pos [1, 1 + n0, D] -> [1, 1 + gh gw, D]; interpolation in f32 like HF, whatever dtype ``pos`` has."""
    n0 = pos.shape[1] - 1
    if n0 == gh * gw and gh == gw:
        return pos
    s = int(n0 ** 0.5)
    pp = pos[:, 1:].reshape(1, s, s, -1).permute(0, 3, 1, 2).to(torch.float32)
    pp = F.interpolate(pp, size=(gh, gw), mode="bicubic", align_corners=False, antialias=antialias).to(pos.dtype)
    return torch.cat((pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)), 1)


def forward(img, sd, heads, lora_scale=2.0, masks=None, patch=14, eps=1e-6, antialias=True, drop_registers=False, full_last_layer=True):
    """(last_hidden_state [B, 1 + R + n, D] or None, key [B, D, h, w] of the patch tokens, cls_att [B, heads, h w] = attentions[-1][:, :, 0, 1 + R:]).
    ``drop_registers``: the model as an engine that ignores embeddings.register_tokens runs it (what the pin must tell apart); ``antialias=False``: plain
    DINOv2's position interpolation.  ``masks``: (layer, module) -> [rows, D] LoRA-dropout mask over all B (1 + R + n) token rows."""
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    pre = "embeddings."
    x = OV.patch_embed(img, sd[pre + "patch_embeddings.projection.weight"], sd[pre + "patch_embeddings.projection.bias"], patch)
    x = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), x), 1)
    x = x + pos_embed(sd[pre + "position_embeddings"], gh, gw, antialias).to(x)
    reg = sd.get(pre + "register_tokens")
    R = 0 if (reg is None or drop_registers) else reg.shape[1]
    if R:
        x = torch.cat((x[:, :1], reg.to(x).expand(B, -1, -1), x[:, 1:]), 1)
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    m = (lambda i, nm: None) if masks is None else (lambda i, nm: masks.get((i, nm)))
    key = cls_att = None
    for i in range(L):
        p = f"encoder.layer.{i}."
        a = p + "attention.attention."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = lora_linear(h, sd, a + "key", lora_scale, m(i, "key"))
        q = lora_linear(h, sd, a + "query", lora_scale, m(i, "query"))
        if i == L - 1:
            key = k
            hd = q.shape[-1] // heads
            qc = q[:, 0].reshape(B, heads, hd)
            kk = k.reshape(B, -1, heads, hd).transpose(1, 2)
            cls_att = torch.softmax(torch.einsum("bhd,bhnd->bhn", qc, kk) * hd ** -0.5, -1)[:, :, 1 + R:]
            if not full_last_layer:
                break
        v = lora_linear(h, sd, a + "value", lora_scale, m(i, "value"))
        o = OV.attention(q, k, v, heads)
        o = o @ sd[p + "attention.output.dense.weight"].t() + sd[p + "attention.output.dense.bias"]
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = OV.gelu_erf(lora_linear(h, sd, p + "mlp.fc1", lora_scale, m(i, "fc1")))
        h = h @ sd[p + "mlp.fc2.weight"].t() + sd[p + "mlp.fc2.bias"]
        x = h * sd[p + "layer_scale2.lambda1"] + x
    last = OV.layer_norm(x, sd["layernorm.weight"], sd["layernorm.bias"], eps) if full_last_layer else None
    return last, key[:, 1 + R:, :].reshape(B, gh, gw, -1).permute(0, 3, 1, 2), cls_att


def forward_f64(img, sd, heads, device="cpu", **kw):
    """``forward`` in f64 on ``device`` (key-minimal), results on the CPU: (key, cls_att)."""
    sdd = {k: v.to(device, torch.float64) for k, v in sd.items() if v.is_floating_point()}
    _, key, att = forward(img.to(device, torch.float64), sdd, heads, full_last_layer=False, **kw)
    return key.cpu(), att.cpu()


def lora_grads(img, sd, heads, dkey, lora_scale, masks=None, dtype=torch.float64, device="cpu"):
    """(key, {LoRA parameter name: gradient of <key, dkey>}) by autograd over ``forward``; a matrix the key map does not depend on gets zeros."""
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    names = sorted(k for k in sdd if ".lora_" in k)
    for k in names:
        sdd[k].requires_grad_(True)
    _, key, _ = forward(img.to(device, dtype), sdd, heads, lora_scale, masks, full_last_layer=False)
    grads = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if g is None else g) for k, g in zip(names, grads)}


def random_registers_state_dict(D, heads, L, R, patch=14, image_size=70, seed=21, ls=(0.1, 1.0)):
    """HF-named weights of a Dinov2WithRegistersModel (GELU MLP) at any width: trunc-normal 0.02 matrices, non-trivial LayerNorm / biases, LayerScale drawn
    from ``ls`` (not all ones), register tokens ~ N(0, 0.5^2) -- HF's zero init would hide a dropped register.  The registers are drawn LAST, so R = 4 and R = 1
    share every other tensor."""
    g = torch.Generator().manual_seed(seed)
    tn = lambda *s: torch.nn.init.trunc_normal_(torch.empty(*s), std=0.02, a=-0.04, b=0.04, generator=g)  # noqa: E731
    rn = lambda *s: 0.1 * torch.randn(*s, generator=g)  # noqa: E731
    n = (image_size // patch) ** 2
    sd = {"embeddings.cls_token": 0.05 * torch.randn(1, 1, D, generator=g), "embeddings.position_embeddings": 0.05 * torch.randn(1, n + 1, D, generator=g),
          "embeddings.patch_embeddings.projection.weight": tn(D, 3, patch, patch), "embeddings.patch_embeddings.projection.bias": rn(D),
          "embeddings.mask_token": torch.zeros(1, D)}
    for i in range(L):
        p = f"encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            sd[p + f"attention.attention.{nm}.weight"], sd[p + f"attention.attention.{nm}.bias"] = tn(D, D), rn(D)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = tn(D, D), rn(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = tn(4 * D, D), rn(4 * D)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = tn(D, 4 * D), rn(D)
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = 1.0 + rn(D), rn(D)
        sd[p + "layer_scale1.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
        sd[p + "layer_scale2.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
    sd["layernorm.weight"], sd["layernorm.bias"] = 1.0 + rn(D), rn(D)
    sd["embeddings.register_tokens"] = 0.5 * torch.randn(1, R, D, generator=g)
    return sd


def weights_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


# the G21 files (tests/golden/make_golden_registers.py): tag -> (image (H, W), pre-training image size, R)
G21 = {"native": ((70, 70), 70, 4), "up": ((70, 70), 56, 4), "down": ((70, 70), 98, 4), "nonsquare": ((56, 84), 70, 4), "r1": ((70, 70), 70, 1)}
G21_SEED, G21_D, G21_HEADS, G21_LAYERS, G21_B = 21, 128, 2, 3, 3


def g21_state_dict(tag):
    _, pre, R = G21[tag]
    return random_registers_state_dict(G21_D, G21_HEADS, G21_LAYERS, R, image_size=pre, seed=G21_SEED)
