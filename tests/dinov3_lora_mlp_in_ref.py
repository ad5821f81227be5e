"""Test helper: the forward of tests/dinov3_lora_ref.py (DINOv3 ViT up to the last layer's ``k_proj`` output on the patch tokens) with peft-style LoRA on ANY Linear
of a block -- attention.{q,k,v,o}_proj, mlp.{gate,up,down}_proj -- and its gradients by autograd, with the three faults a fused gate_proj / up_proj pair can have as
switches.  A module carries LoRA when the state dict holds ``<module>.lora_A.weight`` [r, in] and ``<module>.lora_B.weight`` [out, r]:

    y = base(h) + s (mask * h) A^T B^T          (mask: 0 or 1 / (1 - p) per element of the module's input; None = no dropout)

``masks`` maps (layer, leaf name) to the [rows, in] mask over all B (1 + R + n) token rows.

The engine runs gate_proj and up_proj of the gated MLP as ONE rank-2r module on the fused weights_in GEMM: A = [A_g | A_u], B block diagonal over the interleaved
rows, two dropout masks.  ``fault`` (one of PAIR_FAULTS) restates what a wrong block structure computes; it needs both modules in the state dict:

    shared_mask      up_proj's LoRA branch sees gate_proj's dropout mask (one mask for the pair; differs from the truth only under dropout)
    halves_swapped   B_g is applied to the up rows and B_u to the gate rows:      gate += s u_g B_u^T,   up += s u_u B_g^T
    dense_b          the cross blocks of B are live (B treated as dense [2F, 2r]): gate += s (u_g + u_u) B_g^T,   up += s (u_g + u_u) B_u^T

with u_p = (mask_p * h) A_p^T.  Runs in the dtype and on the device of the inputs.  Nothing under ucod_dpl_amd/ imports this file."""
import torch

from oracle import vit as OV
import dinov3_ref as R3
import dinov3_lora_ref as RL

PAIR_FAULTS = ("shared_mask", "halves_swapped", "dense_b")
PAIR = ("gate_proj", "up_proj")
LEAVES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
MLP_IN_KIND = 1                                              # the dropout key of the MLP input modules is kind * L + l (csrc/vit_train_driver.hip: dropout_of)
# leaf -> (kind, projection) on the gated MLP; on the plain MLP up_proj is the one MLP input module and keeps projection 0, exactly as DINOv2's fc1
DROP_KEY = {"q_proj": (0, 0), "k_proj": (0, 1), "v_proj": (0, 2), "gate_proj": (1, 0), "up_proj": (1, 1), "o_proj": (2, 0), "down_proj": (3, 0)}


def module_path(leaf):
    return ("attention." if leaf in LEAVES[:4] else "mlp.") + leaf


def forward(img, sd, heads, lora_scale, masks=None, eps=1e-5, theta=100.0, patch=16, fault=None):
    """key [B, D, gh, gw]: the last layer's k_proj output (LoRA included, before any rotation) on the patch tokens."""
    assert fault is None or fault in PAIR_FAULTS
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
    lin = lambda t, p, leaf, i: RL.lora_linear(t, sd, p + module_path(leaf), lora_scale, m(i, leaf))  # noqa: E731

    def rot(t):
        t = t.reshape(B, 1 + R + n, heads, 64)
        return torch.cat((t[:, :1 + R], R3.rotate(t[:, 1 + R:], cos, sin)), 1).reshape(B, -1, D)

    def down(t, name, mask):
        """u = (mask * t) A^T of module ``name``"""
        td = t if mask is None else t * mask.to(t).reshape(t.shape)
        return td @ sd[name + ".lora_A.weight"].t()

    for i in range(L):
        p = f"{pre}{i}."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = lin(h, p, "k_proj", i)
        if i == L - 1:
            return k[:, 1 + R:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
        q, v = lin(h, p, "q_proj", i), lin(h, p, "v_proj", i)
        o = lin(OV.attention(rot(q), rot(k), v, heads), p, "o_proj", i)
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        if p + "mlp.gate_proj.weight" in sd:
            if fault is None:
                g, u = lin(h, p, "gate_proj", i), lin(h, p, "up_proj", i)
            else:
                gn, un = p + "mlp.gate_proj", p + "mlp.up_proj"
                g, u = (h @ sd[nm + ".weight"].t() + sd[nm + ".bias"] for nm in (gn, un))
                ug, uu = down(h, gn, m(i, "gate_proj")), down(h, un, m(i, "gate_proj" if fault == "shared_mask" else "up_proj"))
                bg, bu = sd[gn + ".lora_B.weight"], sd[un + ".lora_B.weight"]
                if fault == "halves_swapped":
                    bg, bu = bu, bg
                if fault == "dense_b":
                    ug = uu = ug + uu
                g, u = g + lora_scale * ug @ bg.t(), u + lora_scale * uu @ bu.t()
            h = torch.nn.functional.silu(g) * u
        else:
            h = OV.gelu_erf(lin(h, p, "up_proj", i))
        x = lin(h, p, "down_proj", i) * sd[p + "layer_scale2.lambda1"] + x
    raise AssertionError("unreachable")


def grads(img, sd, heads, dkey, lora_scale, masks=None, dtype=torch.float64, device="cpu", bias_of=(), **kw):
    """(key, {name: gradient of <key, dkey>}) by autograd over ``forward`` for every LoRA matrix in ``sd`` and every ``<module>.bias`` named in ``bias_of``; a
    tensor the key map does not depend on gets zeros."""
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    names = sorted(k for k in sdd if ".lora_" in k) + sorted(bias_of)
    for k in names:
        sdd[k].requires_grad_(True)
    key = forward(img.to(device, dtype), sdd, heads, lora_scale, masks, **kw)
    gs = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if g is None else g.detach()) for k, g in zip(names, gs)}


def hash_masks(seed, leaves, L, rows, widths, p_drop, gated=True):
    """The engine's counter-hash masks (oracle.vit.lora_dropout_mask) of the modules ``leaves`` in layers 0 .. L-1 for ``rows`` token rows: ``widths`` maps a leaf
    to its input width.  Key = kind * L + l, one projection field per module of a kind (DROP_KEY; ``gated`` False: up_proj takes projection 0)."""
    proj = lambda nm: DROP_KEY[nm][1] if gated or nm != "up_proj" else 0  # noqa: E731
    return {(i, nm): OV.lora_dropout_mask(seed, DROP_KEY[nm][0] * L + i, proj(nm), rows, widths[nm], p_drop) for i in range(L) for nm in leaves}


# ---- the G26 files (tests/golden/make_golden_dinov3_lora_mlp_in.py): the G22 models g46, d256 (plain MLP: up_proj) and gated (gate_proj / up_proj)
G26_TAGS = ("g46", "d256", "gated")
G26_SEED, G26_B, G26_R, G26_ALPHA, G26_B_STD = 26, 3, 2, 4, 0.05
G26_SCALE = G26_ALPHA / G26_R
G26_INPUT_SEED = {"g46": 25, "d256": 24, "gated": 29}          # (the G23 inputs of the same models; gated: the seed tests/test_gpu_dinov3_lora.py uses)
# target sets per tag: q / k / v as in the reference's configuration, plus the MLP input modules under test
G26_SETS = {"g46": {"up": ("up_proj",)}, "d256": {"up": ("up_proj",)}, "gated": {"gate": ("gate_proj",), "up": ("up_proj",), "both": PAIR}}
# the dropout run the golden stores the ``shared_mask`` fault from: the engine's step 1 with seed 1234 on ONE stream (ViTLoRAEngine._begin_step / _seed_of_chunk)
G26_P_DROP, G26_ENGINE_SEED = 0.05, 1234
G26_DROP_SEED = (G26_ENGINE_SEED * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF


def g26_targets(tag, tset):
    return list(RL.QKV) + list(G26_SETS[tag][tset])


def g26_lora(tag, leaves=LEAVES):
    """LoRA matrices of a G26 golden for the modules ``leaves`` (those the model has): A kaiming-uniform(a = sqrt 5) = U(-1 / sqrt fan_in, 1 / sqrt fan_in),
    B = 0.05 randn.  Every module of LEAVES is drawn, layer by layer, A then B, whether asked for or not: a subset is the same numbers."""
    m = R3.G22[tag]
    g = torch.Generator().manual_seed(G26_SEED)
    out = {}
    for i in range(R3.G22_LAYERS):
        for leaf in LEAVES:
            if leaf == "gate_proj" and not m["gated"]:
                continue
            k, n = (m["F"], m["D"]) if leaf == "down_proj" else (m["D"], m["F"] if leaf in PAIR else m["D"])
            a, b = (torch.rand(G26_R, k, generator=g) * 2 - 1) / k ** 0.5, G26_B_STD * torch.randn(n, G26_R, generator=g)
            if leaf in leaves:
                base = f"model.layer.{i}.{module_path(leaf)}."
                out[base + "lora_A.weight"], out[base + "lora_B.weight"] = a, b
    return out


def g26_inputs(tag):
    return RL.g23_inputs(tag, seed=G26_INPUT_SEED[tag])


def g26_masks(tag, leaves, rows, seed=G26_DROP_SEED, p_drop=G26_P_DROP):
    m = R3.G22[tag]
    return hash_masks(seed, leaves, R3.G22_LAYERS, rows, {nm: (m["F"] if nm == "down_proj" else m["D"]) for nm in LEAVES}, p_drop, m["gated"])


def grad_bar(z, tset, name, p_drop=0.0):
    """The bound on the relative L2 error of the engine's gradient ``name`` against a G26 golden ``z``, target set ``tset``: dinov3_lora_ref.grad_bar's rule,
    max(4e-2 (5e-2 with dropout), 3 x that gradient's error under CPU bf16 autocast)."""
    return max(4e-2 if p_drop == 0 else 5e-2, 3.0 * float(z[f"ebf/{tset}/{name}"]))
