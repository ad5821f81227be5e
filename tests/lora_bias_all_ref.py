"""Test helper: the f64 restatement of what LoRA ``bias="all"`` adds to ``bias="lora_only"`` (models/modules/full_model.py:53,66 hands ``bias`` to peft, whose rule
for "all" is requires_grad on every parameter with "bias" in its name): the LayerNorm betas of every layer and the patch embedding's bias.  It runs the forwards
tests/lora_bias_ref.py runs (tests/lora_out_ref.py, tests/lora_swiglu_out_ref.py) and, for the gated DINOv3 MLP with gate_proj / up_proj adapters,
tests/dinov3_lora_mlp_in_ref.py -- all of which read every bias from the state dict -- with those vectors as autograd leaves.

``norm_names`` lists them in the order of the backward's norm table (include/ucod_dpl.h: ucod_vit_backward_lora_bias_ex): the patch bias, then norm1 / norm2 of
every layer.  ``trained_names`` is peft's rule on a state dict, minus the final LayerNorm (which the key hook never reaches).  The two column-sum kernels have their
own f64 statements here as well (``colsum_lora``, ``colsum_tok``).  Nothing under ucod_dpl_amd/ imports this file."""
import torch

import lora_bias_ref as RB
import dinov3_lora_mlp_in_ref as RM

FINAL_NORMS = ("layernorm.bias", "norm.bias")


def patch_bias_name(sd):
    return "embeddings.patch_embeddings.bias" if "embeddings.patch_embeddings.bias" in sd else "embeddings.patch_embeddings.projection.bias"


def norm_names(sd):
    """[patch bias, norm1.bias of layer 0, norm2.bias of layer 0, norm1.bias of layer 1, ...]: the norm table's order"""
    lay = RB.layer_path(sd)
    return [patch_bias_name(sd)] + [f"{lay}{i}.norm{k}.bias" for i in range(RB.n_layers(sd)) for k in (1, 2)]


def trained_names(sd):
    """What peft's rule selects on ``sd`` ("bias" in the name), minus the final LayerNorm's bias."""
    return sorted(k for k in sd if "bias" in k and k not in FINAL_NORMS and ".lora_" not in k)


def norm_grads(img, sd, heads, dkey, lora_scale, masks=None, gated=False, dtype=torch.float64, device="cpu"):
    """{name: gradient of <key, dkey>} for ``norm_names(sd)`` by autograd; a vector the key map does not depend on (the last layer's norm2.bias) gets zeros.
    ``sd`` holds the LoRA matrices; ``gated``: the forward of tests/dinov3_lora_mlp_in_ref.py (DINOv3 with the MLP input modules)."""
    names = norm_names(sd)
    if gated:
        _, g = RM.grads(img, sd, heads, dkey, lora_scale, masks=masks, dtype=dtype, device=device, bias_of=names)
        return {k: g[k] for k in names}
    fwd, _ = RB.family(sd)
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    for k in names:
        sdd[k].requires_grad_(True)
    key = fwd(img.to(device, dtype), sdd, heads, lora_scale, masks)
    g = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(sdd[k]) if v is None else v.detach()) for k, v in zip(names, g)}


def colsum_lora(dy, t, a, masks):
    """out[n] = sum_m (dy[m][n] + sum_p masks[p][m][n] * (t[p] @ a[p])[m][n]) in f64: dy [M, D]; t[p] [M, r]; a[p] [r, D]; masks[p] [M, D] (0 or 1 / (1 - p))"""
    y = dy.double().clone()
    for tp, ap, mp in zip(t, a, masks):
        y += mp.double() * (tp.double() @ ap.double())
    return y.sum(0)


def colsum_tok(x, B, tok, first, scale=None):
    """out[n] = scale[n] * sum over images and tokens first .. tok - 1 of x [B * tok, N], in f64"""
    s = x.double().reshape(B, tok, -1)[:, first:].sum((0, 1))
    return s if scale is None else s * scale.double()


def all_grads(img, sd, heads, dkey, lora_scale, masks=None, gated=False, dtype=torch.float64, device="cpu", extra=()):
    """(key, {name: gradient of <key, dkey>}) for every LoRA matrix in ``sd`` and every name of ``trained_names(sd)`` by autograd; a tensor the key map does not
    depend on gets zeros (torch's grad = None: the last layer's biases other than the key's and norm1's)."""
    names = trained_names(sd) + list(extra)                       # (``extra``: further leaves, e.g. the CLS and register tokens)
    if gated:
        return RM.grads(img, sd, heads, dkey, lora_scale, masks=masks, dtype=dtype, device=device, bias_of=names)
    fwd, _ = RB.family(sd)
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    leaves = sorted(k for k in sdd if ".lora_" in k) + names
    for k in leaves:
        sdd[k].requires_grad_(True)
    key = fwd(img.to(device, dtype), sdd, heads, lora_scale, masks)
    g = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in leaves], allow_unused=True)
    return key.detach(), {k: (torch.zeros_like(sdd[k]) if v is None else v.detach()) for k, v in zip(leaves, g)}


def perturbed(sd, seed=11, scale=0.5):
    """Every trained bias moved by ``scale`` * randn * max(rms, 0.1): what a training run could have left (tests of the merges and the adapter)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in trained_names(sd):
        b = sd[name].float()
        out[name] = b + scale * torch.randn(b.shape, generator=g) * max(float(b.pow(2).mean().sqrt()), 0.1)
    return out


# The faults a backward can have here.  Three write whole tensors as zeros; two are the reasons the new kernels exist:
#   beta_without_lora_term   d beta taken from the dgrad output alone: the masked LoRA branch sum_p mask_p (t_p A_p) of the modules behind that LayerNorm left out
#   patch_all_rows           the patch bias summed over CLS / register rows too
FAULTS = ("beta_without_lora_term", "patch_all_rows", "beta1_layer0_dropped", "last_beta1_dropped", "untargeted_dropped")
LN1_LEAVES, LN2_LEAVES = ("query", "key", "value", "q_proj", "k_proj", "v_proj"), ("fc1", "weights_in", "up_proj", "gate_proj")


def lora_branch_of_beta(img, sd, heads, dkey, lora_scale, masks=None, gated=False, dtype=torch.float64, device="cpu"):
    """{norm bias name: the part of its gradient that arrives through the LoRA branches of the modules behind that LayerNorm}: sum over rows of
    mask (.) ((scale dy B) A), dy the row-wise cotangent of the module's output -- taken by autograd with the module's bias as a [B, tokens, n] leaf (a module
    without a bias, DINOv3's k_proj, gets a zero one: the forwards read biases from the state dict)."""
    fwd = RM.forward if gated else RB.family(sd)[0]
    lay, L = RB.layer_path(sd), RB.n_layers(sd)
    tok, _ = RB.geometry(img, sd)
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    mods = sorted(k[:-len(".lora_A.weight")] for k in sdd if k.endswith(".lora_A.weight") and k.rsplit(".", 3)[-3] in LN1_LEAVES + LN2_LEAVES)
    for m in mods:
        n = sdd[m + ".weight"].shape[0]
        b = sdd[m + ".bias"] if m + ".bias" in sdd else torch.zeros(n, dtype=dtype, device=device)
        sdd[m + ".bias"] = b.expand(img.shape[0], tok, n).clone().requires_grad_(True)
    key = fwd(img.to(device, dtype), sdd, heads, lora_scale, masks)
    rows = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[m + ".bias"] for m in mods], allow_unused=True)
    out = {}
    for m, dy in zip(mods, rows):
        if dy is None:
            continue
        i, leaf = int(m[len(lay):].split(".")[0]), m.rsplit(".", 1)[-1]
        dh = (lora_scale * dy @ sdd[m + ".lora_B.weight"]) @ sdd[m + ".lora_A.weight"]
        mask = None if masks is None else masks.get((i, leaf))
        if mask is not None:
            dh = dh * mask.to(dh).reshape(dh.shape)
        name = f"{lay}{i}.norm{1 if leaf in LN1_LEAVES else 2}.bias"
        out[name] = out.get(name, 0) + dh.sum((0, 1)).detach()
    return out


def with_fault(grads, sd, targeted_paths, fault, branch=None, lead=None):
    """``grads`` ({name: gradient}) as a backward with ``fault`` would return them.  ``targeted_paths``: the module paths below the layer path that carry an
    adapter; ``branch``: ``lora_branch_of_beta`` (beta_without_lora_term); ``lead``: {name: gradient} of the CLS and register tokens -- the sums of the first
    residual state's cotangent over those rows (patch_all_rows)."""
    assert fault in FAULTS
    lay, L = RB.layer_path(sd), RB.n_layers(sd)
    out = dict(grads)
    if fault == "beta_without_lora_term":
        for k, v in branch.items():
            out[k] = out[k] - v.to(out[k])
        return out
    if fault == "patch_all_rows":
        p = patch_bias_name(sd)
        out[p] = out[p] + sum(v.reshape(-1, v.shape[-1]).sum(0).to(out[p]) for v in lead.values())
        return out
    if fault == "beta1_layer0_dropped":
        hit = [f"{lay}0.norm1.bias"]
    elif fault == "last_beta1_dropped":
        hit = [f"{lay}{L - 1}.norm1.bias"]
    else:
        hit = [k for k in trained_names(sd) if k.startswith(lay) and ".norm" not in k and not any(k == f"{lay}{k[len(lay):].split('.')[0]}.{p}.bias" for p in targeted_paths)]
    for k in hit:
        out[k] = torch.zeros_like(out[k])
    return out


LEAD_TOKENS = ("embeddings.cls_token", "embeddings.register_tokens")


def errors(got, ref, sd):
    """tests/lora_bias_ref.py's measure extended: the betas join their layer's vector (their names stand below the layer path), the patch bias is a vector of its own."""
    patch = patch_bias_name(sd)
    names = trained_names(sd)
    out = RB.errors(got, {k: ref[k] for k in names if k != patch}, sd)
    out[patch] = float((got[patch].double().cpu() - ref[patch].double().cpu()).norm() / ref[patch].double().cpu().norm())
    return out


# ---- the G27 files (tests/golden/make_golden_lora_bias_all.py): transformers' own named_parameters() with "bias" in the name and their f64 gradients
G27_TAGS = ("dinov2", "dinov3")


def g27(tag):
    """(the npz, state dict, heads, LoRA matrices, lora scale, x, dkey, whether the forward is tests/dinov3_lora_mlp_in_ref.py's) of a G27 golden"""
    import os
    import numpy as np
    import dinov3_ref as R3
    import lora_swiglu_out_ref as RS
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"g27_lora_bias_all_{tag}.npz"))
    sd, heads = (RS.g24_state_dict("dinov2"), RS.G24_HEADS) if tag == "dinov2" else (R3.g22_state_dict("gated"), R3.G22["gated"]["heads"])
    # (the weights are drawn, not stored; tests/test_lora_bias_all_host.py checks their SHA-256 against the golden's, on the CPU, like the other goldens' host tests)
    lora = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/")}
    return z, sd, heads, lora, float(z["scale"]), torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"]), tag == "dinov3"


def g27_grads(z):
    """{name: f64 gradient} of the golden's bias parameters, the final LayerNorm's left out"""
    return {str(n): torch.from_numpy(z["grad/" + str(n)]) for n in z["names"] if str(n) not in FINAL_NORMS}
