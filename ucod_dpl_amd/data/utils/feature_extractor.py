"""Frozen backbone wrapper -- host-side mirror of data/utils/feature_extractor.py::backbone (:31-59).

``backbone(fe_cfg)(img, reshape_keys=True) -> (outputs, key)`` where ``key`` is the LAST layer's key projection
(bias included, before the head split), CLS dropped, reshaped to ``[B,C,h,w]`` (:46-47,55-58).  ``outputs`` is
``None``: the reference's callers discard it (loop_UCOD_DPL.py:343, base_dataset.py:136-138) and the HIP engine
does not compute the dead tail of the last layer unless ``full_last_layer`` is requested.

Weights: the reference calls ``transformers.AutoModel.from_pretrained`` on ``fe_cfg.backbone_weights`` and falls
back to downloading ``fe_cfg.backbone`` (:17-25).  Here the checkpoint is read straight from that local directory
(``model.safetensors`` or ``pytorch_model.bin`` + ``config.json``) with no dependency on HF module attribute
paths (they changed in transformers 5.x and broke the reference's DINOv1 hook); there is no
network fallback.  ``backbone.from_state_dict`` / ``backbone.random_init`` cover tests and synthetic benchmarks.
"""
import json
import os
from pathlib import Path

import torch
from torch import nn

from ...vit_engine import ViTEngine, SplitViTEngine, is_dinov3
from ...engine.registry import BACKBONE_REGISTRY

# name -> (width D, heads, layers, patch, pretrain image size, layerscale?)
ARCHS = {
    "dinov2_vits14": (384, 6, 12, 14, 518, True),
    "dinov2_vitb14": (768, 12, 12, 14, 518, True),
    "dinov2_vitl14": (1024, 16, 24, 14, 518, True),
    "dinov2_vitg14": (1536, 24, 40, 14, 518, True),
    "dino_vits8": (384, 6, 12, 8, 224, False),
    "dino_vitb8": (768, 12, 12, 8, 224, False),
    # DINOv2 with registers (HF Dinov2WithRegistersModel, model_type "dinov2_with_registers"): the tuples of their plain siblings; the register count is in REGISTER_ARCHS
    "dinov2_vits14_reg": (384, 6, 12, 14, 518, True),
    "dinov2_vitb14_reg": (768, 12, 12, 14, 518, True),
    "dinov2_vitl14_reg": (1024, 16, 24, 14, 518, True),
    "dinov2_vitg14_reg": (1536, 24, 40, 14, 518, True),
    # DINOv3 (HF DINOv3ViTModel, model_type "dinov3_vit"): patch 16, 4 register tokens, no position table (rotary position embedding), MLP width 4 D -- GELU, or
    # gated SiLU for the "plus" models (SWIGLU_ARCHS).  ViT-7B/16 is left out: its head dimension is 128.
    "dinov3_vits16": (384, 6, 12, 16, 224, True),
    "dinov3_vitb16": (768, 12, 12, 16, 224, True),
    "dinov3_vitl16": (1024, 16, 24, 16, 224, True),
    "dinov3_vits16plus": (384, 6, 12, 16, 224, True),
    "dinov3_vith16plus": (1280, 20, 32, 16, 224, True),
}
# the DINOv3 architectures -> their register tokens (every released ViT has 4).  A table of its own, not entries of REGISTER_ARCHS: that table holds
# exactly the DINOv2-with-registers names, each the twin of a plain architecture, and tests/test_registers_host.py::test_register_archs pins it to those four
DINOV3_ARCHS = {"dinov3_vits16": 4, "dinov3_vitb16": 4, "dinov3_vitl16": 4, "dinov3_vits16plus": 4, "dinov3_vith16plus": 4}
# architectures with register tokens -> how many (embeddings.register_tokens [1, R, D]: R tokens between CLS and the patches, no position rows)
REGISTER_ARCHS = {"dinov2_vits14_reg": 4, "dinov2_vitb14_reg": 4, "dinov2_vitl14_reg": 4, "dinov2_vitg14_reg": 4}
HUB_TO_ARCH = {"facebook/dinov2-small": "dinov2_vits14", "facebook/dinov2-base": "dinov2_vitb14", "facebook/dinov2-large": "dinov2_vitl14",
               "facebook/dinov2-giant": "dinov2_vitg14", "facebook/dino-vits8": "dino_vits8", "facebook/dino-vitb8": "dino_vitb8",
               "facebook/dinov2-with-registers-small": "dinov2_vits14_reg", "facebook/dinov2-with-registers-base": "dinov2_vitb14_reg",
               "facebook/dinov2-with-registers-large": "dinov2_vitl14_reg", "facebook/dinov2-with-registers-giant": "dinov2_vitg14_reg",
               "facebook/dinov3-vits16-pretrain-lvd1689m": "dinov3_vits16", "facebook/dinov3-vits16plus-pretrain-lvd1689m": "dinov3_vits16plus",
               "facebook/dinov3-vitb16-pretrain-lvd1689m": "dinov3_vitb16", "facebook/dinov3-vitl16-pretrain-lvd1689m": "dinov3_vitl16",
               "facebook/dinov3-vitl16-pretrain-sat493m": "dinov3_vitl16", "facebook/dinov3-vith16plus-pretrain-lvd1689m": "dinov3_vith16plus"}
# architectures whose MLP is Dinov2SwiGLUFFN (config.use_swiglu_ffn, modeling_dinov2.py:300-315,355): weights_in [2F, D] / weights_out [D, F] instead of fc1 / fc2
# (DINOv3 "plus": config.use_gated_mlp, mlp.gate_proj / up_proj / down_proj with the intermediate width 4 D -- arithmetically the same MLP)
SWIGLU_ARCHS = {"dinov2_vitg14", "dinov2_vitg14_reg", "dinov3_vits16plus", "dinov3_vith16plus"}


def swiglu_hidden(D, mlp_ratio=4):
    """HF's SwiGLU hidden width (modeling_dinov2.py:304-305): 4096 at D = 1536."""
    return (int(int(D * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def random_state_dict(arch, seed=0, image_size=None, device=None):
    """Seeded HF-layout state dict with the architecture's shapes (trunc-normal sigma 0.02, HF init); throughput and
    parity tests do not depend on trained weights.  ``device="meta"``: shapes only (no allocation)."""
    if device is not None and torch.device(device).type == "meta":
        with torch.device("meta"):
            return _random_state_dict(arch, seed, image_size, lambda *s: torch.empty(*s))
    g = torch.Generator().manual_seed(seed)
    return _random_state_dict(arch, seed, image_size, lambda *s: torch.nn.init.trunc_normal_(torch.empty(*s), std=0.02, a=-0.04, b=0.04, generator=g))


def _random_state_dict_dinov3(arch, tn):
    """HF DINOv3ViTModel's layout (transformers 5.x) without ``embeddings.mask_token``: no position table, ``k_proj`` without a bias, MLP width 4 D (gated or not),
    register tokens drawn non-zero like every other tensor."""
    D, heads, L, P, _, _ = ARCHS[arch]
    F = 4 * D
    sd = {"embeddings.cls_token": tn(1, 1, D), "embeddings.register_tokens": tn(1, DINOV3_ARCHS[arch], D),
          "embeddings.patch_embeddings.weight": tn(D, 3, P, P), "embeddings.patch_embeddings.bias": torch.zeros(D)}
    for i in range(L):
        p = f"model.layer.{i}."
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = torch.ones(D) + tn(D), tn(D)
        sd[p + "attention.k_proj.weight"] = tn(D, D)
        for nm in ("v_proj", "q_proj", "o_proj"):
            sd[p + f"attention.{nm}.weight"], sd[p + f"attention.{nm}.bias"] = tn(D, D), tn(D)
        sd[p + "layer_scale1.lambda1"] = torch.ones(D)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = torch.ones(D) + tn(D), tn(D)
        for nm in (("gate_proj", "up_proj") if arch in SWIGLU_ARCHS else ("up_proj",)):
            sd[p + f"mlp.{nm}.weight"], sd[p + f"mlp.{nm}.bias"] = tn(F, D), tn(F)
        sd[p + "mlp.down_proj.weight"], sd[p + "mlp.down_proj.bias"] = tn(D, F), tn(D)
        sd[p + "layer_scale2.lambda1"] = torch.ones(D)
    sd["norm.weight"], sd["norm.bias"] = torch.ones(D), torch.zeros(D)
    return sd


def _random_state_dict(arch, seed, image_size, tn):
    if arch in DINOV3_ARCHS:
        return _random_state_dict_dinov3(arch, tn)
    D, heads, L, P, img, ls = ARCHS[arch]
    img = image_size or img
    n = (img // P) ** 2
    sd = {"embeddings.cls_token": tn(1, 1, D), "embeddings.position_embeddings": tn(1, n + 1, D),
          "embeddings.patch_embeddings.projection.weight": tn(D, 3, P, P), "embeddings.patch_embeddings.projection.bias": torch.zeros(D)}
    for i in range(L):
        p = f"encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            sd[p + f"attention.attention.{nm}.weight"], sd[p + f"attention.attention.{nm}.bias"] = tn(D, D), tn(D)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = tn(D, D), tn(D)
        if arch in SWIGLU_ARCHS:
            F = swiglu_hidden(D)
            sd[p + "mlp.weights_in.weight"], sd[p + "mlp.weights_in.bias"] = tn(2 * F, D), tn(2 * F)
            sd[p + "mlp.weights_out.weight"], sd[p + "mlp.weights_out.bias"] = tn(D, F), tn(D)
        else:
            sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = tn(4 * D, D), tn(4 * D)
            sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = tn(D, 4 * D), tn(D)
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = torch.ones(D) + tn(D), tn(D)
        if ls:
            sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"] = torch.ones(D), torch.ones(D)
    sd["layernorm.weight"], sd["layernorm.bias"] = torch.ones(D), torch.zeros(D)
    if arch in REGISTER_ARCHS:
        # drawn like every other tensor and LAST (the plain sibling's tensors are the same draws), NOT HF's zero init: a pass that dropped zero registers would still
        # differ from the plain model by four constant tokens only, one that dropped these is visibly wrong
        sd["embeddings.register_tokens"] = tn(1, REGISTER_ARCHS[arch], D)
    return sd


def trained_like_state_dict(arch, seed=0, image_size=None, qk_gain=4.0, layer_scale=(0.1, 1.0), massive=200.0):
    """``random_state_dict`` reshaped towards the statistics a TRAINED DINOv2 checkpoint shows (no checkpoint travels with this repository
    and there is no network): (1) query / key projections scaled by ``qk_gain`` each, which moves the pre-softmax scores from a standard
    deviation of ~0.3 (trunc-normal init: nearly uniform attention rows) to ~4, i.e. peaked rows whose entropy is far below ln(tokens);
    (2) LayerScale drawn from ``layer_scale`` instead of 1; (3) two "massive activation" channels: the position embedding puts
    +-``massive`` into them at the CLS token and a few patch tokens, so the residual stream carries values of that size through every
    layer.  Used by the parity tests and by bench.py's ``parity_full_size`` leg ("peaked" rows) next to the flat init."""
    D, heads, L, P, img, ls = ARCHS[arch]
    sd = random_state_dict(arch, seed, image_size)
    g = torch.Generator().manual_seed(seed + 7919)
    v3 = arch in DINOV3_ARCHS
    for i in range(L):
        p = f"model.layer.{i}." if v3 else f"encoder.layer.{i}."
        for nm in ("query", "key"):
            for k in ((f"attention.{nm[0]}_proj.weight", f"attention.{nm[0]}_proj.bias") if v3 else (f"attention.attention.{nm}.weight", f"attention.attention.{nm}.bias")):
                if p + k in sd:                                   # (DINOv3: k_proj has no bias)
                    sd[p + k] *= qk_gain
        if ls:
            lo, hi = layer_scale
            sd[p + "layer_scale1.lambda1"] = lo + (hi - lo) * torch.rand(D, generator=g)
            sd[p + "layer_scale2.lambda1"] = lo + (hi - lo) * torch.rand(D, generator=g)
    if massive and v3:
        # no position table: the massive channels sit in the CLS and register tokens (where a trained model with registers keeps them)
        for t in (sd["embeddings.cls_token"], sd["embeddings.register_tokens"]):
            t[0, :, 5 % D] = massive
            t[0, :, (D * 3) // 4] = -0.75 * massive
    elif massive:
        pos = sd["embeddings.position_embeddings"]
        n = pos.shape[1]
        for t in (0, 17 % n, 100 % n, n - 1):
            pos[0, t, 5 % D] = massive
            pos[0, t, (D * 3) // 4] = -0.75 * massive
    return sd


def _read_checkpoint(folder):
    folder = Path(folder).expanduser()
    cfg = {}
    if (folder / "config.json").exists():
        cfg = json.loads((folder / "config.json").read_text())
    if (folder / "model.safetensors").exists():
        from safetensors.torch import load_file
        return load_file(str(folder / "model.safetensors")), cfg
    if (folder / "pytorch_model.bin").exists():
        return torch.load(str(folder / "pytorch_model.bin"), map_location="cpu"), cfg
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {folder} (and no network to download "
                            f"one): place the HuggingFace checkpoint there or use backbone.from_state_dict")


@BACKBONE_REGISTRY.register()
class backbone(nn.Module):
    def __init__(self, config=None, state_dict=None, heads=None, eps=None, device="cuda", **engine_kw):
        super().__init__()
        self.config = config
        self.key = None
        if state_dict is None:
            if config is None:
                raise ValueError("backbone needs a feature_extractor_cfg or a state_dict")
            assert config.backbone_type == "huggingface"          # feature_extractor.py:16
            if "dino" not in config.type:
                raise ValueError(f"Unsupported model type: {config.type}")
            state_dict, hf_cfg = _read_checkpoint(config.backbone_weights)
            heads = heads or hf_cfg.get("num_attention_heads") or ARCHS[HUB_TO_ARCH[config.backbone]][1]
            if hf_cfg.get("model_type") == "dinov3_vit" or is_dinov3(state_dict):
                # DINOv3ViTConfig's defaults: layer_norm_eps 1e-5, rope_theta 100 (the inv_freq buffer is not in the checkpoint)
                if eps is None:
                    eps = hf_cfg.get("layer_norm_eps", 1e-5)
                engine_kw.setdefault("rope_theta", float(hf_cfg.get("rope_theta", 100.0)))
            if eps is None:
                # transformers' defaults when config.json omits the key: ViTConfig (the DINOv1 checkpoints) 1e-12, Dinov2Config 1e-6
                is_v2 = hf_cfg.get("model_type", "dinov2" if "dinov2" in config.type or "dinov2" in str(config.backbone) else "vit") in ("dinov2", "dinov2_with_registers")
                eps = hf_cfg.get("layer_norm_eps", 1e-6 if is_v2 else 1e-12)
            if "num_register_tokens" in hf_cfg or hf_cfg.get("model_type") == "dinov2_with_registers":
                # config.json against the tensor: a checkpoint whose two halves disagree would run with the wrong token count
                # (Dinov2WithRegistersConfig's default when the key is absent: 4)
                said = int(hf_cfg.get("num_register_tokens", 4))
                reg = next((v for k, v in state_dict.items() if k.endswith("embeddings.register_tokens")), None)
                have = 0 if reg is None else int(reg.shape[1])
                if said != have:
                    raise ValueError(f"config.json says num_register_tokens = {said}, the checkpoint's embeddings.register_tokens holds {have}")
        if heads is None:
            raise ValueError("heads is required with an explicit state_dict")
        if config is not None:
            # build-only keys of dataset_cfg.feature_extractor_cfg (absent from the shipped configs: the engine's defaults apply, and those ARE the
            # configuration bench.py quotes its headline on -- fp16 operands on the fp16 residual stream with LayerNorm folded into QKV / fc1 wherever the fold
            # exists, logits within 1e-3 of the f32 reference on the flat init; round 6)
            for k in ("half", "resid", "ln_fold", "attn_variant", "precision"):
                if k in config and k not in engine_kw:
                    engine_kw[k] = config[k]
        self._src = (state_dict, heads, eps or 1e-6, device)       # (references, not copies) what with_precision() rebuilds a sibling engine from
        self._siblings = {}
        self._rope_theta = float(engine_kw.pop("rope_theta", 100.0))      # a property of the checkpoint (DINOv3), so every sibling engine of with_precision() gets it
        self.precision, self.engine = self._make_engine(engine_kw.pop("precision", None), engine_kw)

    PRECISIONS = {"split2": 2, "split3": 3, "f32eq": 3, "split2h": 2, "split2hf": 2}
    TERM_TYPES = {"split2h": "f16", "split2hf": "f16"}           # (every other split precision: bf16 terms)
    FUSED_MLP = {"split2hf"}                                     # fc1 + activation + split in one launch (SplitViTEngine(fuse_mlp=True))

    def _make_engine(self, precision, engine_kw):
        """``precision``: None / "f16" / "bf16" -> the 16-bit ``ViTEngine`` (``half`` = that; None = the engine's default, fp16); "split2" / "split3" / "f32eq"
        (= split3) -> ``SplitViTEngine``: every matrix product on split bf16 operands with an f32 residual stream -- the reference's cached-feature pass runs the
        backbone in plain fp32 (data/datasets/base_dataset.py:124-138) and this is the engine that reproduces it to f32 rounding.  "split2h": the same engine on two
        fp16 terms per operand (22 significand bits at split2's three products; opt-in -- "f32eq" still means split3).  "split2hf": split2h with fc1, its activation and
        the split of the result fused into one launch (``fuse_mlp=True``; opt-in as well)."""
        state_dict, heads, eps, device = self._src
        engine_kw = dict(engine_kw, rope_theta=self._rope_theta)
        if precision in self.PRECISIONS:
            extra = {k: v for k, v in engine_kw.items() if k not in ("gemm_variant", "rope_theta")}
            if extra:
                raise ValueError(f"precision={precision!r} takes no {sorted(extra)}: the split-operand engine has one residual stream (f32) and one attention path")
            return precision, SplitViTEngine(state_dict, heads=heads, eps=eps, device=device, terms=self.PRECISIONS[precision],
                                             term=self.TERM_TYPES.get(precision, "bf16"), fuse_mlp=precision in self.FUSED_MLP, **engine_kw)
        if precision not in (None, "f16", "bf16"):
            raise ValueError(f"precision must be one of None, 'f16', 'bf16', {sorted(self.PRECISIONS)}; got {precision!r}")
        if precision is not None:
            if engine_kw.get("half", precision) != precision:
                raise ValueError(f"precision={precision!r} contradicts half={engine_kw['half']!r}")
            engine_kw = dict(engine_kw, half=precision)
        eng = ViTEngine(state_dict, heads=heads, eps=eps, device=device, **engine_kw)
        return eng.half, eng

    def with_precision(self, precision):
        """A ``backbone`` over the SAME checkpoint whose engine runs at ``precision`` (built once, then cached): ``build_feature_cache`` asks for "f32eq"."""
        if precision == self.precision or (precision == "f32eq" and self.precision == "split3"):
            return self
        if precision not in self._siblings:
            other = object.__new__(type(self))
            nn.Module.__init__(other)
            other.config, other.key, other._src, other._siblings = self.config, None, self._src, self._siblings
            other._rope_theta = self._rope_theta
            other.precision, other.engine = other._make_engine(precision, {})
            self._siblings[precision] = other
        return self._siblings[precision]

    @classmethod
    def from_state_dict(cls, state_dict, heads, eps=None, device="cuda", **kw):
        """``eps=None``: the LayerNorm epsilon of the checkpoint's model class -- DINOv3ViTConfig's default 1e-5 for a DINOv3 state dict, 1e-6 otherwise."""
        if eps is None:
            eps = 1e-5 if is_dinov3(state_dict) else 1e-6
        return cls(None, state_dict=state_dict, heads=heads, eps=eps, device=device, **kw)

    @classmethod
    def random_init(cls, arch, seed=0, image_size=None, device="cuda", **kw):
        # (eps: Dinov2Config's default 1e-6, DINOv3ViTConfig's 1e-5)
        return cls(None, state_dict=random_state_dict(arch, seed, image_size), heads=ARCHS[arch][1], eps=1e-5 if arch in DINOV3_ARCHS else 1e-6, device=device, **kw)

    def forward(self, input, reshape_keys=True):
        with torch.no_grad():
            key = self.engine(input)                              # [B,C,h,w]
        if not reshape_keys:                                      # the raw hook tensor minus CLS: [B,N-1,C]
            key = key.flatten(2).transpose(1, 2)
        self.key = key
        return None, self.key
