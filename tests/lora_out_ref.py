"""Test helper: the LoRA forwards of tests/registers_ref.py (DINOv2, with or without register tokens) and tests/dinov3_lora_ref.py (DINOv3) with peft-style LoRA
on the two OUTPUT projections as well -- ``attention.output.dense`` / ``mlp.fc2``, on a DINOv3 checkpoint ``attention.o_proj`` / ``mlp.down_proj``
(models/modules/full_model.py:47-72 hands ``target_modules`` to peft).  A module carries LoRA when the state dict holds ``<module>.lora_A.weight`` [r, in] and
``<module>.lora_B.weight`` [out, r]:

    y = base(x) + lora_B(lora_A(dropout(x))) * alpha / r

so the layer scale multiplies the LoRA term with the base output.  ``masks`` maps (layer, leaf name) to the [rows, in] dropout mask (0 or 1 / (1 - p)) of that
module's LoRA input; the output modules' masks come from ``out_masks`` (the engine's keys: 2 L + l and 3 L + l, projection 0, over [rows, D] and [rows, F]).

``cut_input_grad=True`` is the fault a backward can have here: the cotangent that the LoRA branch of an output module sends back into its input -- the ``t A``
term -- is dropped (the forward is unchanged).  Runs in the dtype and on the device of the inputs.  Nothing under ucod_dpl_amd/ imports this file."""
import torch

from oracle import vit as OV
import dinov3_ref as R3
import dinov3_lora_ref as R3L
import registers_ref as RR
from lora_targets_ref import lora_linear

OUT_LEAVES = {"dinov2": ("dense", "fc2"), "dinov3": ("o_proj", "down_proj")}


class _Cut(torch.autograd.Function):
    """identity whose backward returns zeros"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


def out_linear(x, sd, name, scale, mask=None, cut_input_grad=False):
    """``lora_linear`` for an output projection (a missing bias is zero: DINOv3 has them, k_proj aside, but the helper takes either)."""
    y = x @ sd[name + ".weight"].t() + (sd[name + ".bias"] if name + ".bias" in sd else 0)
    if name + ".lora_A.weight" in sd:
        xd = _Cut.apply(x) if cut_input_grad else x
        xd = xd if mask is None else xd * mask.to(x).reshape(x.shape)
        y = y + ((xd @ sd[name + ".lora_A.weight"].t()) @ sd[name + ".lora_B.weight"].t()) * scale
    return y


def out_masks(seed, L, rows, D, F, p, leaves=OUT_LEAVES["dinov2"]):
    """The engine's masks of the two output modules for one chunk of ``rows`` token rows: include/ucod_dpl.h, keys 2 L + l (over [rows, D]) and 3 L + l ([rows, F])."""
    m = {(i, leaves[0]): OV.lora_dropout_mask(seed, 2 * L + i, 0, rows, D, p) for i in range(L)}
    m.update({(i, leaves[1]): OV.lora_dropout_mask(seed, 3 * L + i, 0, rows, F, p) for i in range(L)})
    return m


def forward(img, sd, heads, lora_scale, masks=None, patch=14, eps=1e-6, cut_input_grad=False):
    """DINOv2 (register tokens when the state dict has them, with that model's antialiased position interpolation): the key map [B, D, h, w] of the last layer's key
    projection -- registers_ref.forward, key-minimal, with LoRA on dense and fc2 too."""
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    pre = "embeddings."
    x = OV.patch_embed(img, sd[pre + "patch_embeddings.projection.weight"], sd[pre + "patch_embeddings.projection.bias"], patch)
    x = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), x), 1)
    reg = sd.get(pre + "register_tokens")
    R = 0 if reg is None else reg.shape[1]
    pos = sd[pre + "position_embeddings"]
    x = x + (RR.pos_embed(pos, gh, gw, True) if reg is not None else OV.dinov2_pos_embed(pos, gh, gw)).to(x)
    if R:
        x = torch.cat((x[:, :1], reg.to(x).expand(B, -1, -1), x[:, 1:]), 1)
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    m = (lambda i, nm: None) if masks is None else (lambda i, nm: masks.get((i, nm)))
    for i in range(L):
        p = f"encoder.layer.{i}."
        a = p + "attention.attention."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = lora_linear(h, sd, a + "key", lora_scale, m(i, "key"))
        if i == L - 1:
            return k[:, 1 + R:, :].reshape(B, gh, gw, -1).permute(0, 3, 1, 2)
        q = lora_linear(h, sd, a + "query", lora_scale, m(i, "query"))
        v = lora_linear(h, sd, a + "value", lora_scale, m(i, "value"))
        o = out_linear(OV.attention(q, k, v, heads), sd, p + "attention.output.dense", lora_scale, m(i, "dense"), cut_input_grad)
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = OV.gelu_erf(lora_linear(h, sd, p + "mlp.fc1", lora_scale, m(i, "fc1")))
        x = out_linear(h, sd, p + "mlp.fc2", lora_scale, m(i, "fc2"), cut_input_grad) * sd[p + "layer_scale2.lambda1"] + x
    raise AssertionError("unreachable")


def forward_dinov3(img, sd, heads, lora_scale, masks=None, eps=1e-5, theta=100.0, patch=16, cut_input_grad=False):
    """DINOv3, non-gated MLP: dinov3_lora_ref.forward (its true rotation, forward and backward) with LoRA on o_proj and down_proj too."""
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    n = gh * gw
    x = OV.patch_embed(img, sd["embeddings.patch_embeddings.weight"], sd["embeddings.patch_embeddings.bias"], patch)
    reg = sd["embeddings.register_tokens"]
    R = reg.shape[1]
    x = torch.cat((sd["embeddings.cls_token"].expand(B, -1, -1), reg.expand(B, -1, -1), x), 1)
    cos, sin = (t.to(x) for t in R3.cos_sin(gh, gw, theta, None))
    pre = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    L = 1 + max(int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre))
    D = x.shape[-1]
    m = (lambda i, nm: None) if masks is None else (lambda i, nm: masks.get((i, nm)))

    def rot(t):
        t = t.reshape(B, 1 + R + n, heads, 64)
        return torch.cat((t[:, :1 + R], R3L._Rotate.apply(t[:, 1 + R:], cos, sin, "inverse")), 1).reshape(B, -1, D)

    for i in range(L):
        p = f"{pre}{i}."
        assert p + "mlp.gate_proj.weight" not in sd, "the gated MLP's down_proj is not built"
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = R3L.lora_linear(h, sd, p + "attention.k_proj", lora_scale, m(i, "k_proj"))
        if i == L - 1:
            return k[:, 1 + R:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
        q = R3L.lora_linear(h, sd, p + "attention.q_proj", lora_scale, m(i, "q_proj"))
        v = R3L.lora_linear(h, sd, p + "attention.v_proj", lora_scale, m(i, "v_proj"))
        o = out_linear(OV.attention(rot(q), rot(k), v, heads), sd, p + "attention.o_proj", lora_scale, m(i, "o_proj"), cut_input_grad)
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = OV.gelu_erf(h @ sd[p + "mlp.up_proj.weight"].t() + sd[p + "mlp.up_proj.bias"])
        x = out_linear(h, sd, p + "mlp.down_proj", lora_scale, m(i, "down_proj"), cut_input_grad) * sd[p + "layer_scale2.lambda1"] + x
    raise AssertionError("unreachable")


def lora_grads(img, sd, heads, dkey, lora_scale, masks=None, dtype=torch.float64, device="cpu", dinov3=False, **kw):
    """(key, {LoRA parameter name: gradient of <key, dkey>}) by autograd over ``forward`` / ``forward_dinov3`` in ``dtype`` on ``device``; a matrix the key map does
    not depend on gets zeros."""
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    names = sorted(k for k in sdd if ".lora_" in k)
    for k in names:
        sdd[k].requires_grad_(True)
    key = (forward_dinov3 if dinov3 else forward)(img.to(device, dtype), sdd, heads, lora_scale, masks, **kw)
    grads = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if g is None else g.detach()) for k, g in zip(names, grads)}


def random_out_lora(sd_shapes, r, b_std, seed):
    """LoRA matrices for the modules named in ``sd_shapes`` ({module path: (out, in)}), drawn in sorted order: A = U(+-1 / sqrt in), B = b_std randn (peft's B = 0 would
    make the branch, and dA, vanish)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for mod in sorted(sd_shapes):
        n_out, n_in = sd_shapes[mod]
        out[mod + ".lora_A.weight"] = (torch.rand(r, n_in, generator=g) * 2 - 1) / n_in ** 0.5
        out[mod + ".lora_B.weight"] = b_std * torch.randn(n_out, r, generator=g)
    return out


# ---- the cases tests/test_lora_out_host.py and tests/test_gpu_lora_out.py share
PATHS = {"query": "attention.attention.query", "key": "attention.attention.key", "value": "attention.attention.value", "fc1": "mlp.fc1",
         "dense": "attention.output.dense", "fc2": "mlp.fc2",
         "q_proj": "attention.q_proj", "k_proj": "attention.k_proj", "v_proj": "attention.v_proj", "o_proj": "attention.o_proj", "down_proj": "mlp.down_proj"}
OUT_NAMES = ("dense", "fc2", "o_proj", "down_proj")
B_STD = 0.05            # B of query / key / value / fc1: what tests/test_gpu_lora_targets.py draws
OUT_B_STD = 0.5         # B of the output modules: tests/test_lora_out_host.py asserts that this scale gives the GPU bars their teeth


def layer_path(sd):
    return next(p for p in ("encoder.layer.", "model.layer.", "layer.") if any(k.startswith(p + "0.") for k in sd))


def lora_for(sd, targets, r=2, seed=3, out_b_std=OUT_B_STD):
    """LoRA matrices of the ``targets`` (leaf names) in every layer of ``sd``: A = U(+-1 / sqrt in), B = B_STD randn (OUT_B_STD on the output modules; 0 gives peft's
    init there), drawn layer by layer in the order of ``targets``, A then B."""
    lay = layer_path(sd)
    L = 1 + max(int(k[len(lay):].split(".")[0]) for k in sd if k.startswith(lay))
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(L):
        for t in targets:
            mod = f"{lay}{i}.{PATHS[t]}"
            n_out, n_in = sd[mod + ".weight"].shape
            out[mod + ".lora_A.weight"] = (torch.rand(r, n_in, generator=g) * 2 - 1) / n_in ** 0.5
            out[mod + ".lora_B.weight"] = (out_b_std if t in OUT_NAMES else B_STD) * torch.randn(n_out, r, generator=g)
    return out


def without_out_modules(lora):
    """``lora`` without the output modules' matrices: the forward that ignores them."""
    return {k: v for k, v in lora.items() if not any(f".{PATHS[t]}.lora_" in k for t in OUT_NAMES)}


def d256_state_dict():
    """The D = 256 GELU model of tests/test_gpu_lora_targets.py (``checkpoint("gelu", 256)``): (state dict, heads, L, image size, batch)."""
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(21)
    m = Dinov2Model(Dinov2Config(hidden_size=256, num_hidden_layers=4, num_attention_heads=4, image_size=126, patch_size=14, mlp_ratio=4, layerscale_value=1.0)).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            if "position_embeddings" in n or "cls_token" in n:
                p.mul_(0.05)
    return {k: v.detach() for k, v in m.state_dict().items()}, 4, 4, 126, 3


def case_inputs(B, D, image, patch=14, seed=7):
    gen = torch.Generator().manual_seed(seed)
    gh = image // patch
    return torch.randn(B, 3, image, image, generator=gen), torch.randn(B, D, gh, gh, generator=gen)


TARGET_SETS = (("dense",), ("fc2",), ("query", "key", "value", "fc1", "dense", "fc2"), ("value", "dense"))
