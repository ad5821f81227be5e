"""Test helper: the f64 restatement of LoRA ``bias="lora_only"`` (models/modules/full_model.py:53,66 hands ``bias`` to peft: the bias of every module that carries an
adapter and has a bias is trained too, nothing else changes).  It runs the forwards of tests/lora_out_ref.py (DINOv2 GELU, with or without registers; non-gated
DINOv3) and tests/lora_swiglu_out_ref.py (DINOv2 SwiGLU; gated DINOv3) -- which read every bias from the state dict -- with the targeted modules' biases as leaves.

Each such bias goes in as a [B, tokens, n] leaf holding the bias in every row, so that autograd returns the cotangent of the module's output ROW BY ROW; the bias
gradient is its sum over the rows.  ``bias_grads`` forms that sum, or one of the FAULTS a backward can have here:

    no_lambda          the output projections' bias gradient without the layer scale (x += lambda * (acc + b) gives db = lambda * sum dx)
    k_from_q           the key bias summed from the query third of the QKV cotangent
    no_prefix_rows     CLS / register rows left out of the sum
    last_key_dropped   the last layer's key bias gradient written as zeros with the other last-layer biases

``errors`` is the measure of tests/test_gpu_lora_bias.py: per layer, the relative L2 error of all trained bias gradients concatenated (the key bias below the last
layer has a mathematically zero gradient without RoPE, so it is judged at the layer's scale), and per tensor for every tensor whose reference norm is at least 1e-3
of that vector's.  Where the key bias is the ONLY trained bias of a layer below the last there is no other scale in the vector: the reference is zero up to f64
rounding (1e-16 of its terms) and what a 16-bit backward returns is the rounding noise of a sum whose terms cancel.  The scale of such a sum is that of its terms,
so with ``scale`` = ``abs_sums`` (the column sums of |cotangent|) a layer whose reference norm is below CANCELLED of that scale is measured as
|got - ref| / |scale| and held to the same bar.  Runs in the dtype and on the device asked for.  Nothing under ucod_dpl_amd/ imports this file."""
import torch

import lora_out_ref as RO
import lora_swiglu_out_ref as RS

FAULTS = ("no_lambda", "k_from_q", "no_prefix_rows", "last_key_dropped")
PATHS = {**RO.PATHS, **RS.PATHS}
KEY_LEAVES, QUERY_LEAVES, OUT_LEAVES = ("key", "k_proj"), ("query", "q_proj"), {"dense": 1, "o_proj": 1, "fc2": 2, "weights_out": 2, "down_proj": 2}
BAR, BAR_LOOSE = 4e-2, 5e-2                 # the project's LoRA-gradient bars (tests/test_gpu_lora_targets.py): 5e-2 with dropout or at D = 256
MIN_SHARE = 1e-3                            # a tensor is judged on its own when its reference norm is at least this share of its layer's vector
CANCELLED = 1e-9                            # a layer's reference vector below this share of the sum of its terms' magnitudes is a cancelled sum: zero up to f64 rounding


def layer_path(sd):
    return RO.layer_path(sd)


def n_layers(sd):
    lay = layer_path(sd)
    return 1 + max(int(k[len(lay):].split(".")[0]) for k in sd if k.startswith(lay))


def family(sd):
    """(forward function, is DINOv3) for a state dict"""
    lay = layer_path(sd)
    if "embeddings.patch_embeddings.weight" in sd:
        return (RS.forward_dinov3 if lay + "0.mlp.gate_proj.weight" in sd else RO.forward_dinov3), True
    return (RS.forward if lay + "0.mlp.weights_in.weight" in sd else RO.forward), False


def bias_names(sd, targets):
    """``{layer path}{i}.{module}.bias`` of every targeted module (leaf names) that has a bias in ``sd``, all layers."""
    lay = layer_path(sd)
    return [f"{lay}{i}.{PATHS[t]}.bias" for i in range(n_layers(sd)) for t in targets if f"{lay}{i}.{PATHS[t]}.bias" in sd]


def leaf_of(name):
    return name.rsplit(".", 2)[-2]


def geometry(img, sd):
    """(tokens per image, number of leading CLS / register rows)"""
    w = sd["embeddings.patch_embeddings.weight"] if "embeddings.patch_embeddings.weight" in sd else sd["embeddings.patch_embeddings.projection.weight"]
    patch = w.shape[-1]
    reg = sd.get("embeddings.register_tokens")
    R = 0 if reg is None else reg.shape[1]
    return 1 + R + (img.shape[2] // patch) * (img.shape[3] // patch), 1 + R


def grads(img, sd, heads, dkey, lora_scale, targets, masks=None, dtype=torch.float64, device="cpu"):
    """(key, {LoRA parameter name: gradient}, {bias name: cotangent of the module's output, [B, tokens, n]}) of <key, dkey> by autograd.  A bias the key map does not
    depend on (the last layer's, the key's aside) gets zeros."""
    fwd, _ = family(sd)
    sdd = {k: v.to(device, dtype) for k, v in sd.items() if v.is_floating_point()}
    lnames = sorted(k for k in sdd if ".lora_" in k)
    bnames = bias_names(sd, targets)
    tok, _ = geometry(img, sd)
    for k in lnames:
        sdd[k].requires_grad_(True)
    for k in bnames:
        sdd[k] = sdd[k].expand(img.shape[0], tok, -1).clone().requires_grad_(True)
    key = fwd(img.to(device, dtype), sdd, heads, lora_scale, masks)
    g = torch.autograd.grad((key * dkey.to(device, dtype)).sum(), [sdd[k] for k in lnames + bnames], allow_unused=True)
    g = [torch.zeros_like(sdd[k]) if v is None else v.detach() for k, v in zip(lnames + bnames, g)]
    return key.detach(), dict(zip(lnames, g[:len(lnames)])), dict(zip(bnames, g[len(lnames):]))


def bias_grads(rows, sd, lead, fault=None):
    """{bias name: gradient [n]} from the row-wise cotangents of ``grads`` (``lead`` = CLS + register rows per image), with one of FAULTS or none."""
    assert fault is None or fault in FAULTS
    lay, L = layer_path(sd), n_layers(sd)
    out = {}
    for name, r in rows.items():
        i, leaf = int(name[len(lay):].split(".")[0]), leaf_of(name)
        g = (r[:, lead:] if fault == "no_prefix_rows" else r).sum((0, 1))
        if fault == "no_lambda" and leaf in OUT_LEAVES:
            g = g / sd[f"{lay}{i}.layer_scale{OUT_LEAVES[leaf]}.lambda1"].to(g)
        if fault == "k_from_q" and leaf in KEY_LEAVES:
            q = next(n for n in rows if n.startswith(f"{lay}{i}.") and leaf_of(n) in QUERY_LEAVES)
            g = rows[q].sum((0, 1))
        if fault == "last_key_dropped" and leaf in KEY_LEAVES and i == L - 1:
            g = torch.zeros_like(g)
        out[name] = g
    return out


def abs_sums(rows):
    """{bias name: sum over the rows of |cotangent|}: the scale of each bias gradient's terms (``errors``)"""
    return {name: r.abs().sum((0, 1)) for name, r in rows.items()}


def errors(got, ref, sd, scale=None):
    """{"layer {i}": rel-L2 of the layer's concatenated bias gradients, name: rel-L2 of a tensor with at least MIN_SHARE of its layer's norm} (layers whose reference
    is all zeros are left out: those gradients must be exact zeros, which the caller asserts).  ``scale`` (``abs_sums``): a layer whose reference is a cancelled sum
    is measured against the norm of its terms' magnitudes instead (module docstring)."""
    lay, out = layer_path(sd), {}
    for i in range(n_layers(sd)):
        names = sorted(n for n in ref if n.startswith(f"{lay}{i}."))
        if not names:
            continue
        r = torch.cat([ref[n].double().reshape(-1).cpu() for n in names])
        g = torch.cat([got[n].double().reshape(-1).cpu() for n in names])
        if float(r.norm()) == 0.0:
            continue
        if scale is not None:
            a = torch.cat([scale[n].double().reshape(-1).cpu() for n in names])
            if float(r.norm()) < CANCELLED * float(a.norm()):
                out[f"layer {i}"] = float((g - r).norm() / a.norm())
                continue
        out[f"layer {i}"] = float((g - r).norm() / r.norm())
        for n in names:
            rn = ref[n].double().cpu()
            if float(rn.norm()) >= MIN_SHARE * float(r.norm()):
                out[n] = float((got[n].double().cpu() - rn).norm() / rn.norm())
    return out


def perturbed_biases(sd, targets, seed=11, scale=0.5):
    """The targeted modules' biases moved by ``scale`` * randn * rms(bias): what a training run could have left (tests of the merges and the adapter)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in bias_names(sd, targets):
        b = sd[name].float()
        out[name] = b + scale * torch.randn(b.shape, generator=g) * b.pow(2).mean().sqrt()
    return out
