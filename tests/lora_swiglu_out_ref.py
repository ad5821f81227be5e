"""Test helper: the f64 restatement of LoRA on the SwiGLU MLP's OUTPUT projection -- ``mlp.weights_out`` of a DINOv2 SwiGLU checkpoint (Dinov2SwiGLUFFN,
modeling_dinov2.py:300-315), ``mlp.down_proj`` of a gated DINOv3 one (models/modules/full_model.py:47-72 hands ``target_modules`` to peft).  It is
tests/lora_targets_ref.forward's SwiGLU branch and tests/dinov3_lora_ref.forward's gated branch with ``out_linear`` of tests/lora_out_ref.py on the attention
output projection and on the MLP output projection:

    hidden = silu(x1) * x2          y = base(hidden) + lora_B(lora_A(dropout(hidden))) * alpha / r

``masks`` maps (layer, leaf name) to the dropout mask (0 or 1 / (1 - p)) of that module's LoRA input.  The engine draws the MLP output module's mask over its PADDED
hidden width, idx = row * F + unit (include/ucod_dpl.h: UCOD_LORA_OUT_ACT_SWIGLU), so ``out_masks`` returns [rows, F] and the restatement uses the first F0 columns.

``fault`` is one of FAULTS, the three ways the new module's passes can be wrong:

    no_forward   the module's LoRA term is missing from the forward (its own gradients are then zero)
    no_dg        the cotangent its LoRA branch sends back into the hidden -- the ``t A`` term that dpre takes through both derivative factors -- is dropped
    da_silu      dA is taken from silu(x1) alone instead of silu(x1) * x2 (forward and every other gradient unchanged)

Runs in the dtype and on the device of the inputs.  Nothing under ucod_dpl_amd/ imports this file."""
import torch
import torch.nn.functional as F

from oracle import vit as OV
import dinov3_ref as R3
import dinov3_lora_ref as R3L
from lora_targets_ref import lora_linear
from lora_out_ref import out_linear, OUT_B_STD, B_STD

FAULTS = ("no_forward", "no_dg", "da_silu")
PATHS = {"query": "attention.attention.query", "key": "attention.attention.key", "value": "attention.attention.value", "weights_in": "mlp.weights_in",
         "dense": "attention.output.dense", "weights_out": "mlp.weights_out",
         "q_proj": "attention.q_proj", "k_proj": "attention.k_proj", "v_proj": "attention.v_proj", "o_proj": "attention.o_proj", "down_proj": "mlp.down_proj"}
OUT_NAMES = ("dense", "weights_out", "o_proj", "down_proj")
OUT_LEAVES = {"dinov2": ("dense", "weights_out"), "dinov3": ("o_proj", "down_proj")}
# the LoRA tensors a fault reaches DIRECTLY, in the layer where it happens, as (leaf name, "A" / "B"): the module's own matrices without its forward term; the module
# in front of the hidden's cotangent without the t A term (weights_in on DINOv2); the module's own A with the wrong hidden.  On DINOv3 no MLP input module is
# built (up_proj / gate_proj), so ``no_dg`` reaches no LoRA tensor directly there: everything upstream sees it only through LayerNorm 2 beside the residual path,
# 2 - 5 % on the gated G24 model -- below the bars.  Its teeth are the DINOv2 model's weights_in gradients and the kernel test, which checks dpre itself.
TOUCHES = {"dinov2": {"no_forward": (("weights_out", "A"), ("weights_out", "B")), "no_dg": (("weights_in", "A"), ("weights_in", "B")), "da_silu": (("weights_out", "A"),)},
           "dinov3": {"no_forward": (("down_proj", "A"), ("down_proj", "B")), "no_dg": (), "da_silu": (("down_proj", "A"),)}}


def padded(F0):
    """The engine's hidden width: F0 up to a multiple of 128 (ucod_dpl_amd/swiglu.py)."""
    return (F0 + 127) // 128 * 128


def swiglu_out_linear(x1, x2, sd, name, scale, mask=None, fault=None):
    """The MLP output projection on hidden = silu(x1) * x2, with the module's LoRA branch and its faults."""
    h = F.silu(x1) * x2
    if fault == "no_forward":
        return h @ sd[name + ".weight"].t() + sd[name + ".bias"]
    if mask is not None:
        mask = mask.to(h).reshape(-1, mask.shape[-1])[:, :h.shape[-1]].reshape(h.shape)      # (drawn over the padded width)
    if fault != "da_silu" or name + ".lora_A.weight" not in sd:
        return out_linear(h, sd, name, scale, mask, cut_input_grad=(fault == "no_dg"))
    # the value and the gradient to the hidden are the right ones; the gradient to A sees silu(x1) in the hidden's place
    A, Bm = sd[name + ".lora_A.weight"], sd[name + ".lora_B.weight"]
    m = 1.0 if mask is None else mask
    wrong = (F.silu(x1).detach() * m) @ A.t()
    u = (h * m) @ A.detach().t() + wrong - wrong.detach()
    return h @ sd[name + ".weight"].t() + sd[name + ".bias"] + (u @ Bm.t()) * scale


def out_masks(seed, L, rows, D, F0, p, leaves=OUT_LEAVES["dinov2"]):
    """The engine's masks of the two output modules for one chunk of ``rows`` token rows: keys 2 L + l over [rows, D] and 3 L + l over [rows, padded(F0)]."""
    m = {(i, leaves[0]): OV.lora_dropout_mask(seed, 2 * L + i, 0, rows, D, p) for i in range(L)}
    m.update({(i, leaves[1]): OV.lora_dropout_mask(seed, 3 * L + i, 0, rows, padded(F0), p) for i in range(L)})
    return m


def forward(img, sd, heads, lora_scale, masks=None, patch=14, eps=1e-6, fault=None):
    """DINOv2 with the SwiGLU MLP: the key map [B, D, h, w] of the last layer's key projection (key-minimal), LoRA on any of query / key / value / weights_in /
    dense / weights_out."""
    assert fault is None or fault in FAULTS
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    pre = "embeddings."
    x = OV.patch_embed(img, sd[pre + "patch_embeddings.projection.weight"], sd[pre + "patch_embeddings.projection.bias"], patch)
    x = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), x), 1)
    x = x + OV.dinov2_pos_embed(sd[pre + "position_embeddings"], gh, gw).to(x)
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
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
        o = out_linear(OV.attention(q, k, v, heads), sd, p + "attention.output.dense", lora_scale, m(i, "dense"))
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        x1, x2 = lora_linear(h, sd, p + "mlp.weights_in", lora_scale, m(i, "weights_in")).chunk(2, dim=-1)
        x = swiglu_out_linear(x1, x2, sd, p + "mlp.weights_out", lora_scale, m(i, "weights_out"), fault) * sd[p + "layer_scale2.lambda1"] + x
    raise AssertionError("unreachable")


def forward_dinov3(img, sd, heads, lora_scale, masks=None, eps=1e-5, theta=100.0, patch=16, fault=None):
    """DINOv3 with the gated MLP: dinov3_lora_ref.forward (its true rotation, forward and backward) with LoRA on o_proj and on the gated down_proj too."""
    assert fault is None or fault in FAULTS
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
    lin = lambda t, name: t @ sd[name + ".weight"].t() + sd[name + ".bias"]  # noqa: E731
    m = (lambda i, nm: None) if masks is None else (lambda i, nm: masks.get((i, nm)))

    def rot(t):
        t = t.reshape(B, 1 + R + n, heads, 64)
        return torch.cat((t[:, :1 + R], R3L._Rotate.apply(t[:, 1 + R:], cos, sin, "inverse")), 1).reshape(B, -1, D)

    for i in range(L):
        p = f"{pre}{i}."
        assert p + "mlp.gate_proj.weight" in sd, "the gated MLP only (the non-gated one: tests/lora_out_ref.forward_dinov3)"
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = R3L.lora_linear(h, sd, p + "attention.k_proj", lora_scale, m(i, "k_proj"))
        if i == L - 1:
            return k[:, 1 + R:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
        q = R3L.lora_linear(h, sd, p + "attention.q_proj", lora_scale, m(i, "q_proj"))
        v = R3L.lora_linear(h, sd, p + "attention.v_proj", lora_scale, m(i, "v_proj"))
        o = out_linear(OV.attention(rot(q), rot(k), v, heads), sd, p + "attention.o_proj", lora_scale, m(i, "o_proj"))
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        x = swiglu_out_linear(lin(h, p + "mlp.gate_proj"), lin(h, p + "mlp.up_proj"), sd, p + "mlp.down_proj", lora_scale, m(i, "down_proj"), fault) \
            * sd[p + "layer_scale2.lambda1"] + x
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


def layer_path(sd):
    return next(p for p in ("encoder.layer.", "model.layer.", "layer.") if any(k.startswith(p + "0.") for k in sd))


def lora_for(sd, targets, r=2, seed=3, out_b_std=OUT_B_STD):
    """lora_out_ref.lora_for with this file's names: A = U(+-1 / sqrt in), B = B_STD randn (OUT_B_STD on the output modules), layer by layer in the order of
    ``targets``, A then B.  Tensors in HF shape: A of weights_out is [r, F0], unpadded."""
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


def without(lora, leaf):
    """``lora`` without the matrices of the module ``leaf``: the forward that ignores it."""
    return {k: v for k, v in lora.items() if f".{PATHS[leaf]}.lora_" not in k}


# ---- the G24 files (tests/golden/make_golden_lora_swiglu_out.py): transformers' own graphs with W + s B A on every module this work makes reachable
#   dinov2   Dinov2Model(use_swiglu_ffn=True) at D = 128, 3 layers: the tiny SwiGLU model of tests/test_gpu_lora_targets.py (F0 = 344: the engine pads to 384)
#   gated    DINOv3ViTModel on G22's ``gated`` model (D = 128, F = 384, R = 4, 4 x 6 grid)
G24_TAGS = ("dinov2", "gated")
G24_TARGETS = {"dinov2": ("query", "key", "value", "weights_in", "dense", "weights_out"), "gated": ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")}
G24_FAMILY = {"dinov2": "dinov2", "gated": "dinov3"}
G24_B, G24_R, G24_ALPHA, G24_LORA_SEED = 2, 2, 4, 24
G24_SCALE = G24_ALPHA / G24_R
G24_HEADS = 2
# The seed of each golden's inputs: the first of 24, 25, ... at which every fault lands at least three bars (grad_bar below) from the truth on the tensors it touches
# (TOUCHES), judged from the reference's own figures; the generator asserts it.
G24_INPUT_SEED = {"dinov2": 24, "gated": 24}


def g24_state_dict(tag):
    if tag == "dinov2":
        from swiglu_ref import random_swiglu_state_dict
        return random_swiglu_state_dict(128, 2, 3, image_size=70, seed=128)
    return R3.g22_state_dict("gated")


def g24_lora(tag):
    return lora_for(g24_state_dict(tag), G24_TARGETS[tag], r=G24_R, seed=G24_LORA_SEED)


def g24_inputs(tag, seed=None):
    """(image [2, 3, H, W], dkey [2, 128, gh, gw]): N(0, 1), the image rounded to bf16 like the other goldens' inputs."""
    g = torch.Generator().manual_seed(G24_INPUT_SEED[tag] if seed is None else seed)
    (H, W), patch = ((70, 70), 14) if tag == "dinov2" else ((64, 96), 16)
    x = torch.randn(G24_B, 3, H, W, generator=g).to(torch.bfloat16).to(torch.float32)
    return x, torch.randn(G24_B, 128, H // patch, W // patch, generator=g)


def g24_grads(tag, x, lora, dkey, **kw):
    """The restatement's (key, gradients) on a G24 model."""
    return lora_grads(x, {**g24_state_dict(tag), **lora}, G24_HEADS, dkey, G24_SCALE, dinov3=(tag == "gated"), **kw)


def grad_bar(z, name, p_drop=0.0):
    """dinov3_lora_ref.grad_bar on a G24 golden: the project's 4e-2 (5e-2 with dropout) or 3 x the error of the same autograd under CPU bf16 autocast."""
    return R3L.grad_bar(z, name, p_drop)


def touched(tag, fault, names):
    """The gradient names among ``names`` that ``fault`` reaches directly, in the layers below the last (whose MLP and attention output never reach the key map)."""
    fam = G24_FAMILY[tag]
    lay = "encoder.layer." if fam == "dinov2" else "model.layer."
    L = 1 + max(int(n[len(lay):].split(".")[0]) for n in names)
    return [n for n in names for leaf, ab in TOUCHES[fam][fault]
            if n.endswith(f".{PATHS[leaf]}.lora_{ab}.weight") and int(n[len(lay):].split(".")[0]) < L - 1]
