"""Test helper: the G28 model -- a gated DINOv3 ViT whose MLP is as wide as dinov3_vith16plus's (hidden 5120: N1 = 10240 rows of the fused weights_in, K = 5120
columns of down_proj) on a small trunk (D = 128, 2 heads, 4 registers, 2 layers, 64 x 96 images) -- its LoRA tensors, inputs and dropout masks by seed, and the f64
restatement's key map and gradients (tests/dinov3_lora_mlp_in_ref.py: every Linear of a block) with two switches that restate what a wrong wide pass computes:

    no_forward   the MLP modules' LoRA terms are missing from the forward (gate_proj, up_proj, down_proj run as their base layers)
    t_8192       the backward's t = s dpre B_m of gate_proj / up_proj is summed over the first 8192 columns of the engine's interleaved dpre only -- hidden units
                 0 .. 4095 of each -- as the narrow gradient kernel's four vectors per thread would leave it; dB and everything else is complete

Only layer 0's MLP reaches the key map (the last layer runs LayerNorm 1 and k_proj only).  Nothing under ucod_dpl_amd/ imports this file."""
import contextlib

import torch

import dinov3_ref as R3
import dinov3_lora_ref as RL
import dinov3_lora_mlp_in_ref as RM

G28 = dict(D=128, heads=2, R=4, F=5120, gated=True, grid=(4, 6))
G28_LAYERS, G28_B, G28_SEED, G28_INPUT_SEED, G28_LORA_SEED = 2, 3, 28, 128, 228
G28_R, G28_ALPHA, G28_B_STD = 2, 4, 0.05
# down_proj's B is drawn ten times larger: its input, the gated hidden silu(g) * u, is an order of magnitude smaller than a LayerNorm output, and with 0.05 the
# module moves the key map by 3e-3 -- less than the bf16 engines' bound of 1.1e-2, so that a pass without it would go unnoticed
G28_B_STD_DOWN = 0.5
G28_SCALE = G28_ALPHA / G28_R
WIDE_LEAVES = ("gate_proj", "up_proj", "down_proj")
# target sets: the pair alone, the output projection alone, every Linear of a block
G28_SETS = {"pair": RM.PAIR, "down": ("down_proj",), "every": RM.LEAVES}
MUTATIONS = ("no_forward", "t_8192")
NARROW_UNITS = 8192 // 2                                     # hidden units of each of gate / up inside the first 8192 interleaved columns
# the dropout run of the GPU test on ONE stream: the engine's step 1 with seed 1234 (ViTLoRAEngine._begin_step / _seed_of_chunk)
G28_P_DROP, G28_ENGINE_SEED = 0.05, 1234
G28_DROP_SEED = (G28_ENGINE_SEED * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF


def g28_state_dict():
    return R3.random_dinov3_state_dict(G28["D"], G28["heads"], G28_LAYERS, G28["R"], G28["F"], True, seed=G28_SEED, gain=R3.G22_GAIN)


def g28_inputs():
    """(image [3, 3, 64, 96] rounded to bf16, dkey [3, 128, 4, 6]): N(0, 1)"""
    gh, gw = G28["grid"]
    g = torch.Generator().manual_seed(G28_INPUT_SEED)
    x = torch.randn(G28_B, 3, 16 * gh, 16 * gw, generator=g).to(torch.bfloat16).to(torch.float32)
    return x, torch.randn(G28_B, G28["D"], gh, gw, generator=g)


def g28_lora(leaves=RM.LEAVES):
    """LoRA matrices for the modules ``leaves``: A = U(-1 / sqrt fan_in, 1 / sqrt fan_in), B = 0.05 randn (down_proj: 0.5).  Every module of RM.LEAVES is drawn, layer by layer, A then
    B, whether asked for or not: a subset is the same numbers (dinov3_lora_mlp_in_ref.g26_lora's rule)."""
    g = torch.Generator().manual_seed(G28_LORA_SEED)
    D, F, out = G28["D"], G28["F"], {}
    for i in range(G28_LAYERS):
        for leaf in RM.LEAVES:
            k, n = (F, D) if leaf == "down_proj" else (D, F if leaf in RM.PAIR else D)
            a, b = (torch.rand(G28_R, k, generator=g) * 2 - 1) / k ** 0.5, (G28_B_STD_DOWN if leaf == "down_proj" else G28_B_STD) * torch.randn(n, G28_R, generator=g)
            if leaf in leaves:
                base = f"model.layer.{i}.{RM.module_path(leaf)}."
                out[base + "lora_A.weight"], out[base + "lora_B.weight"] = a, b
    return out


def g28_masks(leaves, rows, seed=G28_DROP_SEED, p_drop=G28_P_DROP):
    return RM.hash_masks(seed, leaves, G28_LAYERS, rows, {nm: (G28["F"] if nm == "down_proj" else G28["D"]) for nm in RM.LEAVES}, p_drop, True)


def _lora_linear_t_8192(h, sd, name, scale, mask=None):
    """dinov3_lora_ref.lora_linear, but the cotangent reaches u = drop(h) A^T of gate_proj / up_proj through B's first NARROW_UNITS rows only"""
    if name + ".lora_A.weight" not in sd or name.rsplit(".", 1)[-1] not in RM.PAIR:
        return _LORA_LINEAR(h, sd, name, scale, mask)
    y = h @ sd[name + ".weight"].t() + (sd[name + ".bias"] if name + ".bias" in sd else 0)
    hd = h if mask is None else h * mask.to(h).reshape(h.shape)
    u, Bm = hd @ sd[name + ".lora_A.weight"].t(), sd[name + ".lora_B.weight"]
    return y + torch.cat((u @ Bm[:NARROW_UNITS].t(), u.detach() @ Bm[NARROW_UNITS:].t()), -1) * scale


_LORA_LINEAR = RL.lora_linear


@contextlib.contextmanager
def _mutated(mutation):
    if mutation == "t_8192":
        RL.lora_linear = _lora_linear_t_8192
    try:
        yield
    finally:
        RL.lora_linear = _LORA_LINEAR


def grads(x, sd, dkey, masks=None, mutation=None, device="cpu", bias_of=()):
    """(key, {name: gradient}) of the restatement (RM.grads) for the LoRA tensors in ``sd``, under one of MUTATIONS or none"""
    assert mutation is None or mutation in MUTATIONS
    if mutation == "no_forward":
        sd = {k: v for k, v in sd.items() if not (".lora_" in k and k.split(".")[-3] in WIDE_LEAVES)}
        if not any(".lora_" in k for k in sd) and not bias_of:   # nothing left to differentiate: the key map alone
            sdd = {k: v.to(device, torch.float64) for k, v in sd.items() if v.is_floating_point()}
            with torch.no_grad():
                return RM.forward(x.to(device, torch.float64), sdd, G28["heads"], G28_SCALE, masks), {}
    with _mutated(mutation):
        return RM.grads(x, sd, G28["heads"], dkey, G28_SCALE, masks=masks, device=device, bias_of=bias_of)


def grad_bar(z, tset, name, p_drop=0.0):
    """dinov3_lora_mlp_in_ref.grad_bar on the G28 golden ``z``: max(4e-2 (5e-2 with dropout), 3 x that gradient's error under CPU bf16 autocast)"""
    return RM.grad_bar(z, tset, name, p_drop)
