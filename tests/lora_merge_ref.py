"""Test helper: peft's merge of a LoRA module, W <- W + (lora_alpha / r) B A (what ``merge_and_unload()`` does to every module models/modules/full_model.py:47-72
wraps), in the rounding sequence of ucod_lora_merge_f32 (include/ucod_dpl.h), and the key names of a peft adapter file for the reference's ``ViTLoraWrapper``.

    out[n][k] = f32( f64(w0[n][k]) + f64(scaling) * sum_{j < r, ascending} f64(B[n][j]) * f64(A[j][k]) )

The sum is an explicit loop over j, not a matmul: every product of two f32 values is exact in f64, so the loop fixes the one thing that is not -- the order of
the additions -- and the result can be compared bit for bit."""
import torch

ADAPTER_PREFIX = "base_model.model.ViT.encoder.layer."


def merge_f64(w0, A, B, scaling):
    """The merged weight in f64, before the final rounding.  w0 [N, K]; A [r, K]; B [N, r]; ``scaling`` is rounded to f32 first, as the C ABI takes it."""
    s = torch.tensor(float(scaling), dtype=torch.float32).double()
    A, B = A.double(), B.double()
    acc = torch.zeros(w0.shape, dtype=torch.float64, device=w0.device)
    for j in range(A.shape[0]):
        acc = acc + B[:, j:j + 1] * A[j:j + 1, :]
    return w0.double() + s * acc


def merge(w0, A, B, scaling):
    """f32 result of ``merge_f64``: one round-to-nearest-even."""
    return merge_f64(w0, A, B, scaling).float()


def merged_state_dict(sd, scaling, dtype=None):
    """A LoRA-free copy of an HF-named state dict with ``<module>.lora_{A,B}.weight`` entries: every such module's weight merged (``dtype`` None: through
    ``merge``, f32; torch.float64: unrounded, for the f64 forward)."""
    out = {k: v for k, v in sd.items() if ".lora_" not in k}
    for k in sd:
        if k.endswith(".lora_A.weight"):
            mod = k[:-len(".lora_A.weight")]
            w0, A, B = sd[mod + ".weight"], sd[k], sd[mod + ".lora_B.weight"]
            out[mod + ".weight"] = merge_f64(w0, A, B, scaling) if dtype == torch.float64 else merge(w0.float(), A.float(), B.float(), scaling)
    return out


def adapter_keys(n_layers, targets, mlp_in=None):
    """The keys of adapter_model.safetensors: ``targets`` a subset of query / key / value, ``mlp_in`` "fc1" / "weights_in" or None."""
    mods = [f"attention.attention.{t}" for t in ("query", "key", "value") if t in targets] + ([f"mlp.{mlp_in}"] if mlp_in else [])
    return sorted(f"{ADAPTER_PREFIX}{i}.{m}.lora_{ab}.weight" for i in range(n_layers) for m in mods for ab in "AB")
