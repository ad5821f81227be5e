"""LoRA-backbone end-to-end model -- host-side mirror of models/modules/full_model.py (the reference file itself cannot be
imported: it needs ``peft`` and a module, ``models/modules/ocm.py``, that is not in the repository).

Same names and call shapes: ``load_lora(cfg, model)``, ``get_full_model(cfg, checkpoint_path)``,
``full_model(config, backbone, decoder)(inputs, ema=False, get_hidden_feature=False)``, ``freeze_lora`` / ``active_lora``,
``load_state_dict`` (decoder only, :146-147).  What runs underneath is the HIP training engine (``ViTLoRAEngine``):
LoRA r / lora_alpha / target modules as :47-72 (subsets of query, key, value, plus the MLP input projection; bias 'none' or 'lora_only'), the key hook of the last layer -> CLS
dropped -> NCHW -> bilinear 68x68 (:95-106), student backbone differentiable w.r.t. its LoRA matrices, EMA backbone
frozen.  ``enable_ocm`` is rejected: its module does not exist in the reference.  LoRA dropout (``lora_dropout``, 0.05 in the
reference config) is applied in train mode with counter-based masks (it cannot reproduce torch's RNG stream).

The way out of LoRA mode is here too: ``merge_and_unload`` (peft's name: W <- W + (lora_alpha / r) B A, then an ordinary frozen ``backbone`` at any precision) and
``save_lora_adapter`` / ``load_lora_adapter`` (peft's adapter folder: adapter_model.safetensors + adapter_config.json).
"""
import json
import os

import torch
from torch import nn

from ... import ops
from ...vit_engine import ViTLoRAEngine, check_lora_bias, is_dinov3
from ..uscod import baseline


class LoRABackbone(nn.Module):
    """nn.Module face of a ViTLoRAEngine: ONE flat parameter ``lora`` [L, P] that aliases the engine's arena (P = 6*r*D; with the MLP input projection
    targeted, r*(D + N1) more; with bias="lora_only" the trained biases at the end of each row)."""

    def __init__(self, engine: ViTLoRAEngine):
        super().__init__()
        self.engine = engine
        self.lora = nn.Parameter(engine.lora, requires_grad=True)          # same storage: optimiser steps are seen by the engine

    def forward(self, pixel_values):
        if self.lora.requires_grad and torch.is_grad_enabled():
            return self.engine.apply(pixel_values, self.lora)
        return self.engine.forward_train(pixel_values)

    def train(self, mode=True):
        self.engine.train(mode)                                    # LoRA dropout follows the module's mode, like peft's nn.Dropout
        return super().train(mode)

    def sync(self):
        """Re-derive the LoRA columns of the augmented GEMM weights after ``lora`` changed (optimiser step / EMA / load)."""
        self.engine.repack()

    def merge_and_unload(self, precision=None, **engine_kw):
        """peft's ``merge_and_unload()``: the trained matrices merged into the base weights (``ViTLoRAEngine.merged_state_dict``), returned as an ordinary frozen
        ``data.utils.feature_extractor.backbone`` at ``precision`` (None: the fp16 folded default; "bf16"; "split3" / "f32eq" ...).  This module is left as it is."""
        from ...data.utils.feature_extractor import backbone
        eng = self.engine
        if eng.rope:
            engine_kw.setdefault("rope_theta", eng.rope_theta)     # (a property of the checkpoint that its state dict does not hold)
        return backbone.from_state_dict(eng.merged_state_dict(), eng.heads, eps=eng.eps, device=eng.device, precision=precision, **engine_kw)


ADAPTER_PREFIX = "base_model.model.ViT.encoder.layer."      # peft's key prefix for the reference's wrapper (ViTLoraWrapper holds the HF model as ``ViT``)
ADAPTER_ROOT = "base_model.model.ViT."                      # ... in front of the checkpoint's own layer path (a DINOv3 checkpoint: ``model.layer.`` / ``layer.``)
ADAPTER_WEIGHTS, ADAPTER_CONFIG = "adapter_model.safetensors", "adapter_config.json"


def _adapter_prefix(engine):
    """(read with defaults, like ``lora_dropout`` below: anything with the engine's LoRA interface and DINOv2's names can be saved)"""
    return ADAPTER_ROOT + getattr(engine, "_layer_path", "encoder.layer.")                   # (DINOv2: ADAPTER_PREFIX)


def _adapter_targets(engine):
    """target_modules of an engine as peft lists them: the leaf names (query / key / value; q_proj / k_proj / v_proj on a DINOv3 checkpoint; with the output
    projections targeted also dense / fc2 -- weights_out on a SwiGLU checkpoint --, or o_proj / down_proj)"""
    if hasattr(engine, "modules"):
        return [m.leaf for m in engine.modules if m.targeted]
    # (anything with the engine's LoRA interface and DINOv2's names: ``targets`` and ``mlp_target`` alone)
    return [n for n, on in zip(("query", "key", "value"), engine.targets) if on] + ([engine.mlp_target] if engine.mlp_target is not None else [])


def save_lora_adapter(engine, folder):
    """Write the LoRA matrices of ``engine`` as a peft adapter folder: ``adapter_model.safetensors`` with the keys
    ``base_model.model.ViT.encoder.layer.{i}.attention.attention.query.lora_A.weight`` ... (shapes: ``lora_state_dict()``'s; B of ``weights_in`` in HF row order,
    unpadded) and ``adapter_config.json`` with r, lora_alpha, lora_dropout, bias and target_modules (models/modules/full_model.py:47-72).  ``bias`` is the
    engine's: "none", "all" (every ``...bias`` tensor of the checkpoint is stored: peft's rule ``"lora_" in k or "bias" in k``), or "lora_only" -- then the trained biases are stored beside the matrices under the module's own key, ``...query.bias`` (what peft's
    get_peft_model_state_dict derives from a ``lora_`` key: everything in front of ``lora_`` plus ``bias``).
    peft is not a dependency of this package: the layout is restated from peft's documented adapter format and has not been checked against the library -- the
    bias key in particular (recent peft versions hold the wrapped Linear as ``base_layer``, and which of the two names their loader expects is unverified)."""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    sd = engine.lora_state_dict(prefix=_adapter_prefix(engine))
    if getattr(engine, "bias", "none") == "all":
        # peft's rule for bias="all" stores every tensor with "bias" in its name: the trained value where trained (``lora_state_dict``), the checkpoint's otherwise
        # -- what is left is the final LayerNorm's bias, which the key hook never reaches
        for k, v in engine._base_sd.items():
            if "bias" in k and ADAPTER_ROOT + k not in sd:
                sd[ADAPTER_ROOT + k] = v
    save_file({k: v.detach().cpu().contiguous() for k, v in sd.items()}, os.path.join(folder, ADAPTER_WEIGHTS))
    alpha = float(engine.scaling) * int(engine.r)
    cfg = {"peft_type": "LORA", "r": int(engine.r), "lora_alpha": int(alpha) if alpha == int(alpha) else alpha,
           "lora_dropout": float(getattr(engine, "lora_dropout", 0.0)), "bias": str(getattr(engine, "bias", "none")), "target_modules": _adapter_targets(engine)}
    with open(os.path.join(folder, ADAPTER_CONFIG), "w") as f:
        json.dump(cfg, f, indent=2, sort_keys=True)
    return folder


def load_lora_adapter(engine, folder):
    """The inverse of ``save_lora_adapter``: read the folder into ``engine``'s arena.  An adapter whose r, lora_alpha, target_modules or bias mode differ from the
    engine's is refused (both sides are named): its matrices would not fit, or would be applied with another scale, or its trained biases would be dropped."""
    from safetensors.torch import load_file
    with open(os.path.join(folder, ADAPTER_CONFIG)) as f:
        cfg = json.load(f)
    mine = {"r": int(engine.r), "lora_alpha": float(engine.scaling) * int(engine.r), "target_modules": sorted(_adapter_targets(engine)),
            "bias": str(getattr(engine, "bias", "none"))}
    theirs = {"r": int(cfg["r"]), "lora_alpha": float(cfg["lora_alpha"]), "target_modules": sorted(cfg["target_modules"]), "bias": str(cfg.get("bias", "none"))}
    for k in ("r", "target_modules", "lora_alpha", "bias"):
        if mine[k] != theirs[k]:
            raise ValueError(f"LoRA adapter {folder}: {k} is {theirs[k]!r} in {ADAPTER_CONFIG}, {mine[k]!r} in the engine")
    engine.load_lora_state_dict(load_file(os.path.join(folder, ADAPTER_WEIGHTS)), prefix=_adapter_prefix(engine))
    return engine


def load_lora(config, state_dict, heads, device="cuda", generator=None, eps=None):
    """models/modules/full_model.py:47-72.  r == 0 is refused (the reference returns the bare model; use ``backbone`` then).  Either MLP kind of DINOv2 is taken:
    a SwiGLU checkpoint (facebook/dinov2-giant) trains through the engine's SwiGLU backward (``allow_swiglu``).  ``target_modules`` (:54,67: handed to peft as it
    is) may name any non-empty subset of query / key / value and the MLP input projection (``fc1``; ``weights_in`` on a SwiGLU checkpoint), matched by peft's
    suffix rule; ``dense`` / ``fc2`` / ``weights_out`` are refused with the reason (vit_engine.lora_targets) -- unless the build-only key ``allow_out`` (default
    False) is set: then ``dense`` and ``fc2`` (``o_proj`` and the non-gated ``down_proj`` on a DINOv3 checkpoint) are built as row kernels beside their GEMMs, and
    only the SwiGLU MLP's output projection stays refused.  The build-only key ``allow_swiglu_out`` (default False; needs ``allow_out``, and ``allow_rope`` on a
    DINOv3 checkpoint) lifts that too: ``weights_out`` on DINOv2 ViT-g/14, ``down_proj`` on a gated DINOv3 checkpoint whose hidden width is at most 4096.
    A DINOv3 checkpoint is taken with the build-only key ``allow_rope`` (default False: without it the engine refuses the rotary table; ``rope_theta``, default
    100, goes with it); its targets are subsets of q_proj / k_proj / v_proj -- and, with the build-only key ``allow_mlp_in`` (default False), ``up_proj`` and the
    gated MLP's ``gate_proj`` as well, so that with ``allow_out`` / ``allow_swiglu_out`` every Linear of a DINOv3 block is targetable (dinov3_vith16plus, whose
    MLP is wider than the register-resident row kernels take, is refused by name unless the build-only key ``allow_wide_mlp``, default False, is set: its MLP modules
    then run the wide row kernels, UCOD_LORA_WIDE).  ``bias`` (:53,66) is "none" or "lora_only" (the biases of the targeted modules are
    trained too: ``ViTLoRAEngine``); "all" -- every bias of the backbone but the final LayerNorm's, which the key hook never reaches -- is built with the
    build-only key ``allow_bias_all`` (default False) and refused with its reason without it; any other value is a ValueError, both before any device work.  ``eps=None``: 1e-5 for a DINOv3 state dict (DINOv3ViTConfig's default), 1e-6
    otherwise, as ``backbone.from_state_dict``."""
    r = getattr(config, "r", 2)
    if r == 0:
        raise ValueError("r == 0: no LoRA -- use data.utils.feature_extractor.backbone for the frozen path")
    alpha = getattr(config, "lora_alpha", 4)
    targets = getattr(config, "target_modules", None)                        # None: query / key / value, the reference's default
    if targets is not None and not isinstance(targets, str):
        targets = list(targets)
    allow_bias_all = bool(getattr(config, "allow_bias_all", False))
    bias = check_lora_bias(getattr(config, "bias", "none"), allow_bias_all)  # :53,66
    drop = float(getattr(config, "lora_dropout", 0.05))                      # :50
    if eps is None:
        eps = 1e-5 if is_dinov3(state_dict) else 1e-6
    return LoRABackbone(ViTLoRAEngine(state_dict, heads, r=r, lora_alpha=alpha, eps=eps, device=device, generator=generator, lora_dropout=drop, allow_swiglu=True,
                                      target_modules=targets, allow_rope=bool(getattr(config, "allow_rope", False)),
                                      rope_theta=float(getattr(config, "rope_theta", 100.0)), allow_out=bool(getattr(config, "allow_out", False)),
                                      allow_swiglu_out=bool(getattr(config, "allow_swiglu_out", False)), bias=bias,
                                      allow_mlp_in=bool(getattr(config, "allow_mlp_in", False)), allow_bias_all=allow_bias_all,
                                      allow_wide_mlp=bool(getattr(config, "allow_wide_mlp", False))))


class full_model(nn.Module):
    def __init__(self, config, backbone: LoRABackbone, decoder: baseline):
        super().__init__()
        self.config = config
        self.enable_ocm = bool(getattr(config.model_cfg, "enable_ocm", False))
        if self.enable_ocm:
            raise NotImplementedError("enable_ocm: models/modules/ocm.py is not part of the reference repository")
        self.backbone = backbone
        self.backbone_ema = LoRABackbone(backbone.engine.clone_for_ema())       # :84 copy.deepcopy(backbone)
        self.freeze_model(self.backbone_ema)
        self.decoder = decoder
        if getattr(config.model_cfg, "freeze_lora", False):
            self.freeze_lora()
        self.key = None
        self.hook_size = 68                                                      # :103 ih = iw = 68

    def hook_fn_key(self, key_map):
        """:95-106 -- the engine already returns the key projection with CLS dropped as [B,C,h,w]; bilinear to 68x68."""
        if key_map.requires_grad:
            self.key = ops.bilinear_resize_autograd(key_map, self.hook_size, self.hook_size)
        else:
            self.key = ops.bilinear_resize(key_map, self.hook_size, self.hook_size)
        return self.key

    def forward(self, inputs, ema=False, get_hidden_feature=False):
        if ema:
            with torch.no_grad():
                self.hook_fn_key(self.backbone_ema(inputs))
        else:
            self.hook_fn_key(self.backbone(inputs))
        if get_hidden_feature:
            return self.key
        if not ema:
            return self.decoder(self.key, ema=False)                             # (preds, preds_rev, extra_loss)
        return self.decoder(self.key, ema=True)

    def freeze_model(self, model, exclude_keywords=None):
        exclude_keywords = exclude_keywords or []
        for name, param in model.named_parameters():
            param.requires_grad = any(k in name.lower() for k in exclude_keywords)

    def freeze_lora(self):
        for name, param in self.backbone.named_parameters():
            if "lora" in name:
                param.requires_grad = False

    def active_lora(self):
        for name, param in self.backbone.named_parameters():
            if "lora" in name:
                param.requires_grad = True

    def load_state_dict(self, state_dict, strict=True):
        return self.decoder.load_state_dict(state_dict, strict=strict)

    def merge_and_unload(self, ema=False, precision=None):
        """The student's (``ema``: the EMA copy's) backbone with its LoRA matrices merged, as a frozen ``backbone`` at ``precision`` (LoRABackbone.merge_and_unload)."""
        return (self.backbone_ema if ema else self.backbone).merge_and_unload(precision=precision)


def get_full_model(cfg, backbone_state_dict, heads, checkpoint_path=None, device="cuda"):
    """:25-37 with the backbone weights passed in (the reference downloads them through build_feature_extractor)."""
    model = baseline(cfg.model_cfg).to(device)
    if checkpoint_path and os.path.isfile(checkpoint_path):
        from safetensors.torch import load_file
        model.load_state_dict(load_file(checkpoint_path, device=str(device)))
    fe = load_lora(getattr(cfg, "lora_cfg", object()), backbone_state_dict, heads, device=device)
    return full_model(cfg, fe, model)
