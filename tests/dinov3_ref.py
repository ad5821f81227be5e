"""Test helper: the forward of DINOv3 ViT (transformers models/dinov3_vit/modeling_dinov3_vit.py, DINOv3ViTModel in eval mode), restated on a flat HF-named state
dict, up to the last layer's ``k_proj`` output on the patch tokens -- the key map the project consumes -- with the four faults a rotary pass can have as switches.

The model: tokens [CLS | R registers | n patches] with NO position table (CLS = cls_token, register j = register_tokens[j], patch = conv output + bias); in every
layer q and k of the PATCH tokens are rotated per head (head_dim 64) by the angles of the patch's centre: inv_freq[j] = theta^-(4 j / 64), j = 0..15; patch (r, c)
of a gh x gw grid has y = 2 (r + 0.5) / gh - 1, x = 2 (c + 0.5) / gw - 1; angles [n, 32] = 2 pi y inv_freq (16), then 2 pi x inv_freq (16), computed in f32 (the
model forces f32 there and casts cos / sin to the activations' type); for i < 32: out[i] = v[i] cos_i - v[i + 32] sin_i, out[i + 32] = v[i + 32] cos_i + v[i] sin_i.
CLS / register rows and v are not rotated.  k_proj has no bias; the MLP is up_proj -> GELU -> down_proj or the gated down_proj(silu(gate_proj(x)) * up_proj(x)).
The key hook is the last layer's k_proj output BEFORE rotation.

It runs in the dtype of the inputs (f64 as the reference).  Nothing under ucod_dpl_amd/ imports this file."""
import hashlib
import math

import torch

from oracle import vit as OV

FAULTS = ("no_rotation", "swap_yx", "sin_sign", "rotate_prefix")


def cos_sin(gh, gw, theta=100.0, fault=None):
    """(cos, sin) f32 [n, 32]: DINOv3ViTRopePositionEmbedding.forward's values before its ``tile(2)``, written out independently of the engine's builder."""
    inv_freq = 1 / theta ** torch.arange(0, 1, 4 / 64, dtype=torch.float32)
    ys = (torch.arange(0.5, gh, dtype=torch.float32) / gh).repeat_interleave(gw)
    xs = (torch.arange(0.5, gw, dtype=torch.float32) / gw).repeat(gh)
    coords = 2.0 * torch.stack((xs, ys) if fault == "swap_yx" else (ys, xs), -1) - 1.0
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2)
    return torch.cos(angles), (-1.0 if fault == "sin_sign" else 1.0) * torch.sin(angles)


def rotate(t, cos, sin):
    """t [..., n, heads, 64], cos / sin [n, 32] -> the rotated tensor (apply_rotary_pos_emb with rotate_half, written per half)."""
    a, b = t[..., :32], t[..., 32:]
    c, s = cos[:, None, :].to(t), sin[:, None, :].to(t)
    return torch.cat((a * c - b * s, b * c + a * s), -1)


def forward(img, sd, heads, eps=1e-5, theta=100.0, patch=16, fault=None):
    """key [B, D, gh, gw]: the last layer's k_proj output on the patch tokens.  ``fault`` (one of FAULTS): the pass as a faulty engine would run it --
    no rotation at all, the y / x blocks swapped, the sine's sign flipped, or the prefix tokens (CLS, registers) rotated too (prefix token j by patch j's angles)."""
    assert fault is None or fault in FAULTS
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    n = gh * gw
    x = OV.patch_embed(img, sd["embeddings.patch_embeddings.weight"], sd["embeddings.patch_embeddings.bias"], patch)
    reg = sd["embeddings.register_tokens"]
    R = reg.shape[1]
    x = torch.cat((sd["embeddings.cls_token"].expand(B, -1, -1), reg.expand(B, -1, -1), x), 1)
    cos, sin = cos_sin(gh, gw, theta, fault)
    pre = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    L = 1 + max(int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre))
    D = x.shape[-1]
    lin = lambda t, name: t @ sd[name + ".weight"].t() + (sd[name + ".bias"] if name + ".bias" in sd else 0)  # noqa: E731

    def rot(t):
        t = t.reshape(B, 1 + R + n, heads, 64)
        if fault == "no_rotation":
            return t.reshape(B, -1, D)
        lead = rotate(t[:, :1 + R], cos[:1 + R], sin[:1 + R]) if fault == "rotate_prefix" else t[:, :1 + R]
        return torch.cat((lead, rotate(t[:, 1 + R:], cos, sin)), 1).reshape(B, -1, D)

    for i in range(L):
        p = f"{pre}{i}."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        k = lin(h, p + "attention.k_proj")
        if i == L - 1:
            return k[:, 1 + R:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
        q, v = lin(h, p + "attention.q_proj"), lin(h, p + "attention.v_proj")
        o = lin(OV.attention(rot(q), rot(k), v, heads), p + "attention.o_proj")
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        if p + "mlp.gate_proj.weight" in sd:
            h = torch.nn.functional.silu(lin(h, p + "mlp.gate_proj")) * lin(h, p + "mlp.up_proj")
        else:
            h = OV.gelu_erf(lin(h, p + "mlp.up_proj"))
        x = lin(h, p + "mlp.down_proj") * sd[p + "layer_scale2.lambda1"] + x


def forward_f64(img, sd, heads, **kw):
    sdd = {k: v.to(torch.float64) for k, v in sd.items()}
    return forward(img.to(torch.float64), sdd, heads, **kw)


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def random_dinov3_state_dict(D, heads, L, R, F, gated=False, patch=16, seed=22, gain=8.0, ls=(0.1, 1.0)):
    """HF-named weights of a DINOv3ViTModel (transformers 5.x layout), PEAKED: trunc-normal 0.02 matrices with q / k weights and the q bias times ``gain`` (the
    pre-softmax scores then have a spread of a few units: on the flat init a pass without any rotation is as close to the true key map as the fp16 engine is),
    LayerScale drawn from ``ls``, non-zero v / o / MLP biases, k_proj without a bias, register tokens ~ N(0, 0.5^2).  The registers are drawn LAST, so models that
    differ in R alone share every other tensor."""
    g = torch.Generator().manual_seed(seed)
    tn = lambda *s: torch.nn.init.trunc_normal_(torch.empty(*s), std=0.02, a=-0.04, b=0.04, generator=g)  # noqa: E731
    rn = lambda *s: 0.1 * torch.randn(*s, generator=g)  # noqa: E731
    sd = {"embeddings.cls_token": 0.5 * torch.randn(1, 1, D, generator=g), "embeddings.mask_token": torch.zeros(1, 1, D),
          "embeddings.patch_embeddings.weight": tn(D, 3, patch, patch), "embeddings.patch_embeddings.bias": rn(D)}
    for i in range(L):
        p = f"model.layer.{i}."
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = 1.0 + rn(D), rn(D)
        sd[p + "attention.k_proj.weight"] = gain * tn(D, D)
        sd[p + "attention.v_proj.weight"], sd[p + "attention.v_proj.bias"] = tn(D, D), rn(D)
        sd[p + "attention.q_proj.weight"], sd[p + "attention.q_proj.bias"] = gain * tn(D, D), gain * rn(D)
        sd[p + "attention.o_proj.weight"], sd[p + "attention.o_proj.bias"] = tn(D, D), rn(D)
        sd[p + "layer_scale1.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = 1.0 + rn(D), rn(D)
        if gated:
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.gate_proj.bias"] = tn(F, D), rn(F)
        sd[p + "mlp.up_proj.weight"], sd[p + "mlp.up_proj.bias"] = tn(F, D), rn(F)
        sd[p + "mlp.down_proj.weight"], sd[p + "mlp.down_proj.bias"] = tn(D, F), rn(D)
        sd[p + "layer_scale2.lambda1"] = ls[0] + (ls[1] - ls[0]) * torch.rand(D, generator=g)
    sd["norm.weight"], sd["norm.bias"] = 1.0 + rn(D), rn(D)
    sd["embeddings.register_tokens"] = 0.5 * torch.randn(1, R, D, generator=g)
    return sd


def weights_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


# the G22 files (tests/golden/make_golden_dinov3.py): tag -> dict(D, heads, R, F, gated, grid (gh, gw)); every model has 3 layers, patch 16, theta 100, eps 1e-5
G22 = {
    "g46": dict(D=128, heads=2, R=4, F=512, gated=False, grid=(4, 6)),
    "g66": dict(D=128, heads=2, R=4, F=512, gated=False, grid=(6, 6)),
    "r1": dict(D=128, heads=2, R=1, F=512, gated=False, grid=(4, 6)),
    "r0": dict(D=128, heads=2, R=0, F=512, gated=False, grid=(4, 6)),
    "d256": dict(D=256, heads=4, R=4, F=1024, gated=False, grid=(4, 6)),
    "gated": dict(D=128, heads=2, R=4, F=384, gated=True, grid=(4, 6)),
}
G22_SEED, G22_LAYERS, G22_B, G22_GAIN = 22, 3, 2, 8.0


def g22_state_dict(tag):
    m = G22[tag]
    return random_dinov3_state_dict(m["D"], m["heads"], G22_LAYERS, m["R"], m["F"], m["gated"], seed=G22_SEED, gain=G22_GAIN)


def g22_input(tag):
    """The goldens' input: N(0, 1) rounded to bf16 (so that the stored f32 array compresses to half), B images of the model's grid."""
    gh, gw = G22[tag]["grid"]
    x = torch.randn(G22_B, 3, 16 * gh, 16 * gw, generator=torch.Generator().manual_seed(G22_SEED))
    return x.to(torch.bfloat16).to(torch.float32)


# ---- the engine rows of tests/test_gpu_dinov3.py and their bounds (relative L2 of the key map against the golden's f64 key map), from the figures each golden stores:
#   split3 / split2h / split2hf   4 x transformers' own f32 error + 1e-7   (the rule tests/test_gpu_split16.py uses between these engines)
#   split2                        10 x that                               (the ratio of the project's existing bounds, 3e-5 to 3e-6)
#   fp16 operands                 3 x transformers under fp16 autocast    (the engines round at more points than autocast does: the stream, P, and q / k a second
#   bf16 operands                 3 x transformers under bf16 autocast     time after the rotation; DESIGN section 4's per-class table has those classes about equal)
SPLIT_ROWS, F16_ROWS = ("split3", "split2h", "split2hf", "split2"), ("f16_resid32", "f16_resid16")
ENGINE_ROWS = [(p, tag) for tag in G22 for p in SPLIT_ROWS + F16_ROWS] + [("f16_fold", "d256"), ("bf16", "d256")]


def engine_bound(precision, z):
    """the bound of one engine row on the golden ``z`` (an np.load of its file)"""
    if precision in ("split3", "split2h", "split2hf"):
        return 4.0 * float(z["err_f32"]) + 1e-7
    if precision == "split2":
        return 10.0 * (4.0 * float(z["err_f32"]) + 1e-7)
    if precision == "bf16":
        return 3.0 * float(z["err_bf16ac"])
    assert precision in F16_ROWS + ("f16_fold",)
    return 3.0 * float(z["err_f16ac"])
