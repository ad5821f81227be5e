"""ViT backbone engines: each owns device copies of the weights in its operand form, the pointer table the C driver
walks, and reusable workspaces.  Accepts both checkpoint layouts the reference can meet:

* HuggingFace ``Dinov2Model`` / ``ViTModel`` state dicts (data/utils/feature_extractor.py:20,25) with
  ``attention.attention.{query,key,value}`` or (transformers>=5 ViT) ``attention.{q,k,v}_proj`` names;
* HuggingFace ``DINOv3ViTModel`` state dicts (no position table: rotary position embedding on the patch tokens' q and k, ``rope_table``);
* the in-repo DINO ``VisionTransformer`` (models/backbones/dino.py) with fused ``attn.qkv``.

Only what the key hook needs is computed by default (feature_extractor.py:46-47,55-58); see
``ucod_vit_forward`` in include/ucod_dpl.h.

``_BackboneEngine`` holds what the engines share (geometry, position rows, descriptor, table header, input checks, workspaces,
side-stream fan-out, one ``_SaturationGuard`` each); ``ViTEngine`` (16-bit operands) and ``SplitViTEngine`` (split operands) derive from it,
``ViTLoRAEngine`` (backbone-backward mode) is a ``ViTEngine``.  A layer is one 16-slot row built by ``layer_row`` and read by the slot
names of native.py (``N.QKV_W`` ...), never by number.
"""
import contextlib
import ctypes as C
import math
import os
import typing

import torch
import torch.nn.functional as F

from . import native as N
from .swiglu import lora_b_from_engine, lora_b_to_engine, padded_hidden
from . import ops


def _interp_pos_dinov2(pos, gh, gw, antialias=False):
    """transformers modeling_dinov2.py:57-95 (bicubic, size=, align_corners=False, computed in f32).  ``antialias``: what Dinov2WithRegistersEmbeddings
    .interpolate_pos_encoding passes (modeling_dinov2_with_registers.py: antialias=True) -- torch's antialiased bicubic filter widens where the target grid is
    SMALLER than the stored one (224 px on a 518-px checkpoint) and uses the cubic coefficient -0.5 instead of -0.75 everywhere, so the rows differ on every
    interpolated grid."""
    n0 = pos.shape[1] - 1
    if n0 == gh * gw and gh == gw:
        return pos
    s = int(n0 ** 0.5)
    pp = pos[:, 1:].reshape(1, s, s, -1).permute(0, 3, 1, 2).float()
    pp = F.interpolate(pp, size=(gh, gw), mode="bicubic", align_corners=False, antialias=bool(antialias))
    return torch.cat((pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)), 1)


def _interp_pos_dinov1(pos, gh, gw):
    """models/backbones/dino.py:202-221 (scale_factor + 0.1 trick)."""
    n0 = pos.shape[1] - 1
    if n0 == gh * gw and gh == gw:
        return pos
    s = int(math.sqrt(n0))
    pp = pos[:, 1:].reshape(1, s, s, -1).permute(0, 3, 1, 2)
    pp = F.interpolate(pp, scale_factor=((gh + 0.1) / math.sqrt(n0), (gw + 0.1) / math.sqrt(n0)), mode="bicubic")
    assert pp.shape[-2] == gh and pp.shape[-1] == gw
    return torch.cat((pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)), 1)


def is_dinov3(sd):
    """True for a HuggingFace DINOv3ViTModel state dict: a patch convolution named ``embeddings.patch_embeddings.weight`` and no position table."""
    return any(k.endswith("embeddings.patch_embeddings.weight") for k in sd) and not any(k.endswith("embeddings.position_embeddings") for k in sd)


def rope_table(gh, gw, theta=100.0):
    """The rotary table of a gh x gw patch grid, f32 [gh gw, 64] = cos[0:32] | sin[0:32] (what ucod_rope_qk reads): the operations of transformers'
    DINOv3ViTRopePositionEmbedding.forward in eval mode (modeling_dinov3_vit.py:95-121,153-200), in the same order and type, on the CPU -- bit for bit the first
    halves of the model's ``cos`` / ``sin`` (which are these 32 values tiled twice; the duplicate is not stored).  Row p = r gw + c: angles 2 pi y inv_freq
    (16 values), then 2 pi x inv_freq (16 values), y = 2 (r + 0.5) / gh - 1, x = 2 (c + 0.5) / gw - 1, inv_freq[j] = theta^-(4 j / 64)."""
    inv_freq = 1 / float(theta) ** torch.arange(0, 1, 4 / 64, dtype=torch.float32)
    coords_h = torch.arange(0.5, gh, dtype=torch.float32) / gh
    coords_w = torch.arange(0.5, gw, dtype=torch.float32) / gw
    coords = torch.stack(torch.meshgrid(coords_h, coords_w, indexing="ij"), dim=-1).flatten(0, 1)
    coords = 2.0 * coords - 1.0
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2)
    return torch.cat((torch.cos(angles), torch.sin(angles)), 1).contiguous()


def _normalize_dinov3(sd, out):
    """The DINOv3ViTModel layout (transformers 5.x: ``model.layer.{i}.``; checkpoints written by 4.56: ``layer.{i}.``): q / k / v / o_proj, ``k_proj`` without a
    bias (config.key_bias = False), ``mlp.up_proj`` -> GELU -> ``mlp.down_proj`` or the gated ``down_proj(silu(gate_proj(x)) * up_proj(x))``, which is DINOv2's
    SwiGLU with weights_in = cat(gate_proj, up_proj).  Any absent bias is zeros."""
    pref = next(k[:-len("embeddings.patch_embeddings.weight")] for k in sd if k.endswith("embeddings.patch_embeddings.weight"))
    g = lambda k: sd[pref + k]  # noqa: E731
    out["kind"], out["rope"], out["pos"] = "dinov3", True, None
    out["patch_w"], out["cls"] = g("embeddings.patch_embeddings.weight"), g("embeddings.cls_token").reshape(-1)
    D = out["cls"].shape[0]
    zeros = lambda n, like: torch.zeros(n, dtype=like.dtype, device=like.device)  # noqa: E731
    out["patch_b"] = sd.get(pref + "embeddings.patch_embeddings.bias", zeros(D, out["patch_w"]))
    reg = sd.get(pref + "embeddings.register_tokens")
    if reg is not None and (reg.dim() != 3 or reg.shape[0] != 1 or reg.shape[2] != D):
        raise ValueError(f"embeddings.register_tokens has shape {tuple(reg.shape)}, expected [1, R, {D}]")
    out["reg"] = reg[0] if reg is not None and reg.shape[1] > 0 else None
    lay = "model.layer." if any(k.startswith(pref + "model.layer.") for k in sd) else "layer."
    L = 1 + max(int(k[len(pref + lay):].split(".")[0]) for k in sd if k.startswith(pref + lay))
    gated = pref + lay + "0.mlp.gate_proj.weight" in sd
    if gated:
        out["mlp"] = "swiglu"
    for i in range(L):
        p = f"{pref}{lay}{i}."

        def lin(name):
            w = sd[p + name + ".weight"]
            return w, sd.get(p + name + ".bias", zeros(w.shape[0], w))

        (q_w, q_b), (k_w, k_b), (v_w, v_b) = (lin(f"attention.{n}_proj") for n in "qkv")
        proj_w, proj_b = lin("attention.o_proj")
        up_w, up_b = lin("mlp.up_proj")
        fc2_w, fc2_b = lin("mlp.down_proj")
        if gated:
            gate_w, gate_b = lin("mlp.gate_proj")
            fc1_w, fc1_b = torch.cat((gate_w, up_w), 0), torch.cat((gate_b, up_b), 0)       # HF SwiGLU row order: the silu rows, then the linear rows
        else:
            fc1_w, fc1_b = up_w, up_b
        out["layers"].append(dict(
            ln1_g=sd[p + "norm1.weight"], ln1_b=sd[p + "norm1.bias"], qkv_w=torch.cat((q_w, k_w, v_w), 0), qkv_b=torch.cat((q_b, k_b, v_b), 0),
            proj_w=proj_w, proj_b=proj_b, ls1=sd[p + "layer_scale1.lambda1"], ln2_g=sd[p + "norm2.weight"], ln2_b=sd[p + "norm2.bias"],
            fc1_w=fc1_w, fc1_b=fc1_b, fc2_w=fc2_w, fc2_b=fc2_b, ls2=sd[p + "layer_scale2.lambda1"]))
    return out


def normalize_state_dict(sd):
    """Map any supported checkpoint layout to a canonical dict:
    patch_w [D,C,P,P], patch_b, cls [D], pos [1,1+n,D], kind ('dinov2'|'dinov1'),
    layers: list of dict(ln1_g, ln1_b, qkv_w [3D,D], qkv_b, proj_w, proj_b, ls1|None, ln2_g, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b, ls2|None).
    A SwiGLU checkpoint (DINOv2 ViT-g/14: mlp.weights_in / mlp.weights_out, modeling_dinov2.py:300-315) also sets ``mlp = "swiglu"``; its fc1_w / fc1_b are
    weights_in [2F, D] / [2F] in HF's row order (x1 rows, then x2 rows) and fc2_w is weights_out [D, F] (swiglu.prepare pads and interleaves them).
    A DINOv2-with-registers checkpoint (HF Dinov2WithRegistersModel: embeddings.register_tokens [1, R, D], placed between CLS and the patch tokens, without
    position rows) also sets ``reg`` -- the register tokens [R, D], None for a [1, 0, D] tensor (R = 0) -- and ``pos_antialias = True``: that model interpolates
    its position rows with antialias=True, plain DINOv2 does not.  Read both with ``.get``: a dict without the key has neither entry and means R = 0, no
    antialias.  Register tokens on a DINOv1 layout are a ValueError.
    A DINOv3 checkpoint (HF DINOv3ViTModel; ``is_dinov3``) sets ``kind = "dinov3"``, ``rope = True``, ``pos = None`` (there is no position table: the engines
    rotate q and k of the patch tokens, ``rope_table``) and always ``reg`` (None for R = 0); a missing bias (``k_proj`` has none) is zeros, and a gated MLP is
    ``mlp = "swiglu"`` with fc1_w = cat(gate_proj, up_proj)."""
    sd = {k: v for k, v in sd.items()}
    out = {"layers": []}
    if is_dinov3(sd):
        return _normalize_dinov3(sd, out)
    if "cls_token" in sd and "pos_embed" in sd:                      # in-repo DINO
        out["kind"] = "dinov1"
        if any(k.split(".")[-1] in ("register_tokens", "reg_token") for k in sd):
            raise ValueError("register tokens in a DINOv1 (in-repo VisionTransformer) state dict: only DINOv2 with registers has them")
        out["patch_w"], out["patch_b"] = sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"]
        out["cls"], out["pos"] = sd["cls_token"].reshape(-1), sd["pos_embed"]
        L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        for i in range(L):
            p = f"blocks.{i}."
            out["layers"].append(dict(
                ln1_g=sd[p + "norm1.weight"], ln1_b=sd[p + "norm1.bias"], qkv_w=sd[p + "attn.qkv.weight"], qkv_b=sd[p + "attn.qkv.bias"],
                proj_w=sd[p + "attn.proj.weight"], proj_b=sd[p + "attn.proj.bias"], ls1=None,
                ln2_g=sd[p + "norm2.weight"], ln2_b=sd[p + "norm2.bias"], fc1_w=sd[p + "mlp.fc1.weight"], fc1_b=sd[p + "mlp.fc1.bias"],
                fc2_w=sd[p + "mlp.fc2.weight"], fc2_b=sd[p + "mlp.fc2.bias"], ls2=None))
        return out
    # HuggingFace: strip an optional model prefix ("dinov2." / "vit.")
    pref = ""
    for cand in ("", "dinov2.", "vit."):
        if cand + "embeddings.cls_token" in sd:
            pref = cand
            break
    g = lambda k: sd[pref + k]  # noqa: E731
    out["patch_w"], out["patch_b"] = g("embeddings.patch_embeddings.projection.weight"), g("embeddings.patch_embeddings.projection.bias")
    out["cls"], out["pos"] = g("embeddings.cls_token").reshape(-1), g("embeddings.position_embeddings")
    has_ls = any("layer_scale1" in k for k in sd)
    out["kind"] = "dinov2" if has_ls else "dinov1"
    if pref + "embeddings.register_tokens" in sd:
        reg = g("embeddings.register_tokens")
        if reg.dim() != 3 or reg.shape[0] != 1 or reg.shape[2] != out["cls"].shape[0]:
            raise ValueError(f"embeddings.register_tokens has shape {tuple(reg.shape)}, expected [1, R, {out['cls'].shape[0]}]")
        if out["kind"] != "dinov2":
            raise ValueError("register tokens in a DINOv1 (ViTModel, no LayerScale) state dict: only DINOv2 with registers has them")
        # (the key alone marks Dinov2WithRegistersModel, R = 0 included: its embeddings interpolate with antialias=True whatever R is)
        out["pos_antialias"] = True
        out["reg"] = reg[0] if reg.shape[1] > 0 else None
    lay = "encoder.layer." if any(k.startswith(pref + "encoder.layer.") for k in sd) else "encoder.layers."
    L = 1 + max(int(k[len(pref + lay):].split(".")[0]) for k in sd if k.startswith(pref + lay))
    swiglu = pref + lay + "0.mlp.weights_in.weight" in sd
    if swiglu:
        out["mlp"] = "swiglu"
    for i in range(L):
        p = f"{lay}{i}."

        def first(*names):
            for n in names:
                if pref + p + n in sd:
                    return sd[pref + p + n]
            raise KeyError(f"none of {names} under {pref + p}")

        q_w, k_w, v_w = (first(f"attention.attention.{n}.weight", f"attention.{n[0]}_proj.weight") for n in ("query", "key", "value"))
        q_b, k_b, v_b = (first(f"attention.attention.{n}.bias", f"attention.{n[0]}_proj.bias") for n in ("query", "key", "value"))
        out["layers"].append(dict(
            ln1_g=first("norm1.weight", "layernorm_before.weight"), ln1_b=first("norm1.bias", "layernorm_before.bias"),
            qkv_w=torch.cat((q_w, k_w, v_w), 0), qkv_b=torch.cat((q_b, k_b, v_b), 0),
            proj_w=first("attention.output.dense.weight", "attention.o_proj.weight"), proj_b=first("attention.output.dense.bias", "attention.o_proj.bias"),
            ls1=first("layer_scale1.lambda1") if has_ls else None,
            ln2_g=first("norm2.weight", "layernorm_after.weight"), ln2_b=first("norm2.bias", "layernorm_after.bias"),
            fc1_w=first("mlp.weights_in.weight") if swiglu else first("mlp.fc1.weight", "intermediate.dense.weight"),
            fc1_b=first("mlp.weights_in.bias") if swiglu else first("mlp.fc1.bias", "intermediate.dense.bias"),
            fc2_w=first("mlp.weights_out.weight") if swiglu else first("mlp.fc2.weight", "output.dense.weight"),
            fc2_b=first("mlp.weights_out.bias") if swiglu else first("mlp.fc2.bias", "output.dense.bias"),
            ls2=first("layer_scale2.lambda1") if has_ls else None))
    return out


def _prepare_mlp(c):
    """(MLP kind for the library's _mlp entry points, canonical dict whose fc1 / fc2 entries are what the tables hold).  SwiGLU: weights_in / its bias padded to
    F % 128 == 0 and interleaved in blocks of 4, weights_out padded (swiglu.prepare; host f32); GELU: ``c`` unchanged."""
    if c.get("mlp", "gelu") != "swiglu":
        return N.UCOD_MLP_GELU, c
    from .swiglu import prepare
    cpu = lambda t: t.detach().to("cpu", torch.float32)  # noqa: E731
    layers = []
    for l in c["layers"]:
        w_in, b_in, w_out = prepare(cpu(l["fc1_w"]), cpu(l["fc1_b"]), cpu(l["fc2_w"]))
        layers.append(dict(l, fc1_w=w_in, fc1_b=b_in, fc2_w=w_out))
    return N.UCOD_MLP_SWIGLU, dict(c, layers=layers)


_GEMMS = ("qkv", "proj", "fc1", "fc2")                       # the four GEMMs of a layer, in the order of SplitViTEngine.wscale


def layer_row(l, weight, vector, scales=None, aux=(None, None)):
    """One layer's row of the pointer table (native.VIT_LAYER_SLOTS) from a canonical layer dict: ``weight(t, name)`` converts the four matrices, ``vector(t)`` the ten
    vectors (ones for a missing LayerScale).  ``scales`` = (S_qkv, S_proj, S_fc1, S_fc2), the operand scales of the fp16-term split pass: each GEMM's bias goes in
    times its S, the LayerScale behind the out-projection / fc2 divided by it (include/ucod_dpl.h: ucod_vit_forward_split16).  ``aux``: what +14 / +15 hold."""
    row = []
    for name in N.VIT_LAYER_SLOTS[:N.AUX0]:
        if name.endswith("_w"):
            row.append(weight(l[name], name))
        else:
            row.append(vector(torch.ones(l["proj_b"].shape[0], dtype=torch.float32) if l[name] is None else l[name]))
    if scales is not None:
        S_qkv, S_proj, S_fc1, S_fc2 = scales
        for b, S in ((N.QKV_B, S_qkv), (N.PROJ_B, S_proj), (N.FC1_B, S_fc1), (N.FC2_B, S_fc2)):
            row[b] = row[b] * S
        row[N.LS1], row[N.LS2] = row[N.LS1] / S_proj, row[N.LS2] / S_fc2
    return row + list(aux)


# UCOD_MLP_ROWMAJOR=1: the A/B switch of the BLK16 MLP hidden (ViTEngine.__init__), read once per process
_MLP_ROWMAJOR = os.environ.get("UCOD_MLP_ROWMAJOR") == "1"


class _SaturationGuard:
    """The saturation counter of ONE engine's fp16 values (the fp16 residual stream, the operands of the fp16-term split pass): the device word the library's kernels
    count into while it is bound, its pinned host copy, and the events behind the copies still in flight.  Engines never share one, so that a saturation is
    reported by the engine that caused it."""

    def __init__(self, lib, device):
        self.lib, self.device = lib, device
        self.dev = self.host = None
        self.events = []

    @contextlib.contextmanager
    def bind(self):
        """The library's fp16 kernels launched from this thread count into THIS guard's device word (ucod_resid16_overflow_bind)."""
        if self.dev is None:
            self.dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        N.check(self.lib.ucod_resid16_overflow_bind(self.dev.data_ptr()), "ucod_resid16_overflow_bind")
        try:
            yield
        finally:
            self.lib.ucod_resid16_overflow_bind(None)

    def arm(self, stream):
        """Enqueue an asynchronous copy of the device word behind the pass just launched on ``stream``."""
        if self.host is None:
            self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        with self.bind():
            N.check(self.lib.ucod_resid16_overflow_fetch(self.host.data_ptr(), stream.cuda_stream), "ucod_resid16_overflow_fetch")
        ev = torch.cuda.Event()
        ev.record(stream)
        self.events.append(ev)
        del self.events[:-8]                                     # (only the latest copies matter: the counter never decreases)

    def take(self, wait=False):
        """The saturation count of the passes that have finished (``wait``: of every pass enqueued so far).  A non-zero count is handed out ONCE: the device word
        and its host copy are cleared before it is returned."""
        if self.host is None:                                    # no pass has counted anything
            return 0
        if wait:
            self._drain()
        elif not any(ev.query() for ev in self.events):
            return 0
        n = int(self.host[0])
        if n > 0:
            # before the reset: every fetch still queued on a side stream must have landed, or its (stale, non-zero) count would arrive
            # AFTER the host word is cleared and raise a second time for the same saturation
            self._drain()
            with self.bind():
                N.check(self.lib.ucod_resid16_overflow_reset(N.stream()), "ucod_resid16_overflow_reset")
            torch.cuda.current_stream(self.device).synchronize()
            self.host.zero_()
        return n

    def _drain(self):
        for ev in self.events:
            ev.synchronize()
        self.events = []


# (forward_with_cls_attention on DINOv3) why the CLS attention row is refused
_CLS_ROW_ON_ROPE = ("the CLS query's softmax row needs the ROTATED patch keys of the last layer, and the key map -- the hook's output, taken before the rotation -- "
                    "does not hold them")
# ... and the way in: ucod_cls_attention_rope rotates the patch keys as it reads them.  Opt-in, because the refusal above is pinned by tests
_CLS_ROW_WAY_IN = "; pass allow_rope=True for the row computed with the patch keys rotated on the fly (ucod_cls_attention_rope)"


def _chunk_bounds(B, ns):
    """B images as ns image-parallel sub-batches [(b0, b1), ...]."""
    return [(B * i // ns, B * (i + 1) // ns) for i in range(ns)]


class _BackboneEngine:
    """What every engine shares: the geometry of the checkpoint, the header of the pointer table (patch embedding, CLS, position rows) in front of its 16-slot layer
    rows (``layer_row``), the descriptor, input checks, workspaces, side streams and the saturation guard.  The defaults below are the split pass's (f32 stream,
    LayerNorm kernels, key-minimal); ``ViTEngine`` sets its own."""

    def _setup(self, state_dict, heads, eps, device, gemm_variant, lib_half, rope_theta=100.0):
        """Load the ``lib_half`` library and take the geometry from the checkpoint.  Returns (canonical dict with the MLP entries the tables hold, patch weight [D, Kpad]
        f32 on the device, k zero-padded): the subclass converts them to its operand form."""
        self.lib = N.load(lib_half)
        self.mlp, c = _prepare_mlp(normalize_state_dict(state_dict))
        self.kind, self.device = c["kind"], torch.device(device)
        self.D, self.C, self.P = c["patch_w"].shape[:3]
        self.heads = heads
        if self.D != heads * 64:
            raise ValueError(f"head_dim must be 64 (D={self.D}, heads={heads})")
        self.L = len(c["layers"])
        self.F = c["layers"][0]["fc2_w"].shape[1]                  # the MLP hidden width (SwiGLU: after padding; fc1 then has 2 F rows)
        self.eps, self.gemm_variant = float(eps), gemm_variant
        self.resid, self.resid16, self.ln_fold, self.full_last_layer, self.attn_variant = "f32", False, False, False, 0
        self.streams = 1                                           # image-parallel sub-batches on side streams (ViTEngine.forward)
        K = self.C * self.P * self.P
        self.Kpad = (K + 63) // 64 * 64
        pw = torch.zeros(self.D, self.Kpad, dtype=torch.float32, device=self.device)
        pw[:, :K] = self._f32(c["patch_w"]).reshape(self.D, K)
        # DINOv3: no position table (slot +3 of the header holds zeros, so the patch and CLS kernels are what they are) but a rotary table per grid (``_rope``)
        self.rope, self.rope_theta, self._rope_cache = bool(c.get("rope", False)), float(rope_theta), {}
        self._pos_src, self._pos_cache, self._pos_scale = (None if self.rope else c["pos"].detach().float().cpu()), {}, None
        self._pos_antialias = bool(c.get("pos_antialias", False))
        # register tokens (DINOv2 with registers): R rows between CLS and the patches; table slot +2 is then [(1 + R), D], the CLS row first (``_lead_rows``)
        reg = c.get("reg")
        self.R = 0 if reg is None else int(reg.shape[0])
        self._lead_src = c["cls"].reshape(1, -1) if self.R == 0 else torch.cat((c["cls"].reshape(1, -1).float(), reg.float().to(c["cls"].device)), 0)
        self._guard = _SaturationGuard(self.lib, self.device)
        self._ws = self._side = self._side_ws = None
        self.layers = []
        return c, pw

    def _f32(self, t):
        return t.detach().to(self.device, torch.float32).contiguous()

    def _lead_rows(self):
        """f32 [(1 + R), D] on the device: the CLS token followed by the register tokens (R = 0: the CLS row alone, [1, D])."""
        return self._f32(self._lead_src)

    def tokens(self, gh, gw):
        """tokens per image of a gh x gw grid: [CLS | R registers | gh gw patches]"""
        return 1 + self.R + gh * gw

    def _pos(self, gh, gw):
        """The position rows of a gh x gw grid (cached), times ``_pos_scale`` where the patch embedding's operands carry a scale (fp16 terms)."""
        key = (gh, gw)
        if key not in self._pos_cache:
            if self.rope:
                self._pos_cache[key] = torch.zeros(1 + gh * gw, self.D, dtype=torch.float32, device=self.device)
                return self._pos_cache[key]
            if self.kind == "dinov2":
                pos = _interp_pos_dinov2(self._pos_src, gh, gw, antialias=self._pos_antialias)
            else:
                pos = _interp_pos_dinov1(self._pos_src, gh, gw)
            pos = pos[0].to(self.device, torch.float32).contiguous()
            self._pos_cache[key] = pos if self._pos_scale is None else pos * self._pos_scale
        return self._pos_cache[key]

    def _rope(self, gh, gw):
        """The rotary table of a gh x gw grid on the device (cached like the position rows): f32 [gh gw, 64], ``rope_table``."""
        key = (gh, gw)
        if key not in self._rope_cache:
            self._rope_cache[key] = rope_table(gh, gw, self.rope_theta).to(self.device)
        return self._rope_cache[key]

    def _refuse_rope(self, what, why, way_in=""):
        if self.rope:
            raise NotImplementedError(f"{what} is not built for a DINOv3 checkpoint (rotary position embedding, RoPE): {why}{way_in}")

    def _cls_row(self, q, k_lead, key, R):
        """att f32 [B, heads, hw]: the CLS query's softmax row over the keys of ``k_lead`` [B, 1 + R, D] and the patch keys of the key map, patch columns kept.
        One kernel on every checkpoint (ucod_cls_attention_rope / _reg are its two instantiations): with a rotary table it rotates the patch keys as it reads them."""
        B, hw = key.shape[0], key.shape[-2] * key.shape[-1]
        att = torch.empty(B, self.heads, hw, dtype=torch.float32, device=self.device)
        if self.rope:
            table = self._rope(key.shape[-2], key.shape[-1])
            N.check(self.lib.ucod_cls_attention_rope(N.ptr(q), N.ptr(k_lead), N.ptr(key), N.ptr(table), N.ptr(att), B, self.heads, hw, R, 0.125, N.stream()),
                    "ucod_cls_attention_rope")
        else:
            N.check(self.lib.ucod_cls_attention_reg(N.ptr(q), N.ptr(k_lead), N.ptr(key), N.ptr(att), B, self.heads, hw, R, 0.125, N.stream()), "ucod_cls_attention")
        return att

    def _desc(self, B, H, W, L=None):
        d = N.VitDesc()
        d.B, d.C, d.H, d.W, d.P = B, self.C, H, W, self.P
        d.D, d.heads, d.F, d.L, d.Kpad = self.D, self.heads, self.F, (self.L if L is None else L), self.Kpad
        d.eps = self.eps
        d.full_last_layer = int(self.full_last_layer)
        d.gemm_variant, d.attn_variant = self.gemm_variant, self.attn_variant
        d.resid16, d.ln_fold = int(self.resid16), int(self.ln_fold)
        d.n_reg = self.R
        d.rope = self._rope(H // self.P, W // self.P).data_ptr() if self.rope else None      # (the cache keeps the table alive)
        return d

    def _table(self, gh, gw, rows=None):
        """(ctypes table, tensors kept alive): the header, then ``rows`` (default: ``self.layers``)."""
        ptrs = [self.patch_w, self.patch_b, self.cls, self._pos(gh, gw)]
        for row in self.layers if rows is None else rows:
            ptrs += row
        return (C.c_void_p * len(ptrs))(*[None if t is None else t.data_ptr() for t in ptrs]), ptrs

    def param_bytes(self):
        return self.patch_w.numel() * 2 + sum(t.numel() * t.element_size() for l in self.layers for t in l if t is not None)

    def _inputs(self, who, img, out, n_layers=None):
        """(img as contiguous f32, key map to write, H, W) of a pass; ``who`` names the engine in the message."""
        if n_layers is not None and not 1 <= n_layers <= self.L:
            raise ValueError(f"n_layers must be in [1, {self.L}]")
        if not img.is_cuda:
            raise RuntimeError(f"{who} needs a CUDA(ROCm) tensor; there is no CPU path")
        img = img.to(torch.float32).contiguous()
        B, _, H, W = img.shape
        key = out if out is not None else torch.empty(B, self.D, H // self.P, W // self.P, dtype=torch.float32, device=self.device)
        return img, key, H, W

    def _workspace(self, ws, need):
        """``ws`` if it holds ``need`` bytes, else a new buffer that does (the caller stores it back in its slot)."""
        if need == 0:
            raise ValueError("unsupported ViT geometry")
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def _fan_out(self, streams, bounds, fn, tensors, wait=True):
        """Run fn(i, b0, b1) for chunk i = bounds[i] on streams[i], after everything already enqueued on the current stream.  ``tensors``: caller-stream tensors the
        side streams touch (recorded on them so that the caching allocator does not recycle their memory early).  Returns one event per chunk; ``wait``: the
        current stream waits for them."""
        cur = torch.cuda.current_stream(self.device)
        start = torch.cuda.Event()
        start.record(cur)
        events = []
        for i, (st, (b0, b1)) in enumerate(zip(streams, bounds)):
            st.wait_event(start)
            for t in tensors:
                t.record_stream(st)
            with torch.cuda.stream(st):
                fn(i, b0, b1)
                done = torch.cuda.Event()
                done.record(st)
            events.append(done)
        if wait:
            for done in events:
                cur.wait_event(done)
        return events

    def forward_async(self, img, out=None):
        """Enqueue the pass on the side streams WITHOUT making the current stream wait: returns (key, events); the consumer
        calls ``torch.cuda.current_stream().wait_event(e)`` for each event before reading ``key``.  The side streams start
        after everything already enqueued on the current stream (so a ring of key buffers is safe to reuse)."""
        return self.forward(img, out=out, _async=True)


class ViTEngine(_BackboneEngine):
    """HIP ViT forward -> last-layer key map [B, D, H/P, W/P] (f32)."""

    def __init__(self, state_dict, heads, eps=1e-6, device="cuda", full_last_layer=False, gemm_variant=0, attn_variant=0, half="f16",
                 resid="auto", ln_fold="auto", rope_theta=100.0):
        """``rope_theta``: the base period of the rotary position embedding of a DINOv3 checkpoint (config.rope_theta; its inv_freq buffer is not in the state
        dict); unused for every other checkpoint.
        ``half``: 16-bit type of the GEMM / attention operands -- "f16" (default since round 6: IEEE fp16, what the reference's fp16-autocast
        launcher multiplies in; 8x finer rounding than bf16, logits within 1e-3 of the f32 reference at full depth on the flat init; the
        configuration bench.py's headline is measured on) or "bf16" (the dtype BASELINE configs[1] names; opt-in).  Each choice is its own build of
        the same kernels (native.load).
        ``attn_variant``: 0 / 2 the product attention kernel, 1 the generic-scale kernel, 8 the fp8 path of BASELINE configs[4]; 5 / 66 =
        attn_fwd_v5_kernel / attn_fwd_v6_kernel by name (the hand-placed assembly kernels of round 4 are laboratory code: ops.attention_asm).
        ``resid``: type of the residual stream x between the GEMM epilogues and LayerNorm -- "f32" (what the reference holds), "f16"
        (IEEE fp16: half the bytes of LayerNorm's read and of the out-proj / fc2 read-modify-write) or "auto".  "auto" is a property of
        the ENGINE, never of the batch size (an image's key map does not depend on how many images travel with it):
          * bf16 operands -> fp16 stream: its 11 significand bits are 8x finer than the bf16 operands every value is rounded to before
            it is used, so it never sets the error level (logit max-abs vs the f32 oracle 3.2e-3 with either stream);
          * fp16 operands -> fp16 stream WITH LayerNorm folded into QKV / fc1 where the fold exists (D % 256 == 0, D <= 1536, a 16-bit attention
            path: ViT-B / ViT-L; logits 6.0e-4 on the flat init, the fastest configuration), f32 stream otherwise (ViT-S; 3.8e-4).
        ``ln_fold``: LayerNorm 1 / 2 of every layer but the last folded into the QKV / fc1 GEMMs (ucod_gemm_lnfold, include/ucod_dpl.h): the fp16
        stream is the GEMM's A operand, the weights carry gamma, the epilogue applies the row's (rstd, -mean * rstd).  Needs fp16 operands AND the
        fp16 stream (an MFMA takes both operands in one type); "auto" = on exactly there.
        The fp16 stream SATURATES at +-65504 and counts every saturation on the device; ``check_overflow`` (polled by every later
        ``forward``, synchronously with UCOD_CHECK_RESID=1) raises FloatingPointError when the count is non-zero: a checkpoint whose
        activations do not fit fp16 is reported instead of producing inf -> NaN key maps.
        No 16-bit configuration meets 1e-3 on trained-like weights (profiles/r06_error_budget_f16.json: every op class carries ~1e-3 of it);
        ``SplitViTEngine`` (split-operand MFMA, f32 stream: f32-equivalent) is the one that does -- the feature-cache pass uses it."""
        if resid not in ("auto", "f32", "f16"):
            raise ValueError(f"resid must be 'auto', 'f32' or 'f16', got {resid!r}")
        if attn_variant not in (0, 1, 2, 8, 5, 66):
            raise ValueError(f"attn_variant must be 0, 1, 2, 5, 8 or 66 (laboratory kernels are reached through ops.attention(variant=...) / ops.attention_asm), got {attn_variant}")
        if ln_fold not in ("auto", True, False):
            raise ValueError(f"ln_fold must be 'auto', True or False, got {ln_fold!r}")
        self.half = half
        if attn_variant == 8 and is_dinov3(state_dict):
            raise NotImplementedError("attn_variant=8 (the fp8 attention path) is not built for a DINOv3 checkpoint (RoPE): its QKV epilogue writes e4m3 Q and K "
                                      "straight from the GEMM drain, in front of the rotation")
        c, pw = self._setup(state_dict, heads, eps, device, gemm_variant, half, rope_theta)
        self.resid, self.full_last_layer, self.attn_variant = resid, bool(full_last_layer), attn_variant
        fold_shape = half == "f16" and self.D % 256 == 0 and self.D <= 1536 and attn_variant != 8       # where ucod_gemm_lnfold exists
        self.resid16 = bool(resid == "f16" or (resid == "auto" and (half == "bf16" or (fold_shape and ln_fold is not False))))
        can_fold = fold_shape and self.resid16
        if ln_fold is True and not can_fold:
            raise ValueError("ln_fold needs half='f16' with the fp16 residual stream (resid='f16' or 'auto'), D % 256 == 0 and a 16-bit attention path")
        self.ln_fold = bool(can_fold and ln_fold is not False)
        f32, dev = self._f32, self.device
        bf = lambda t, name=None: ops.cast_bf16(f32(t), lib=self.lib)  # noqa: E731
        self.patch_w, self.patch_b, self.cls = bf(pw), f32(c["patch_b"]), self._lead_rows()
        self.layers = [layer_row(l, bf, f32) for l in c["layers"]]
        self.fold_layers = None
        self.q_row_scale = None                                    # [3D] f32 on the device: the row scale the folded QKV entries were built with (merge_into refolds with it)
        if self.ln_fold:
            self.fold_layers = []
            for l, src in zip(self.layers, c["layers"]):
                # (the folded QKV entries also carry the softmax pre-scale head_dim^-0.5 * log2 e on their Q rows -- what the unfolded pass applies as
                # a column scale in the epilogue -- so that the folded epilogue has no per-column multiply left; attn_variant 1 takes Q unscaled)
                # (set-up arithmetic on the HOST in f64 -- fold.py -- then one copy per tensor: no vendor-BLAS kernel runs on the device for it)
                cpu = lambda t: t.detach().to("cpu", torch.float32)  # noqa: E731
                qs = torch.ones(3 * self.D, dtype=torch.float32)
                if attn_variant != 1:
                    qs[:self.D] = 0.125 * 1.4426950408889634
                fl = list(l)
                fl[N.QKV_W], fl[N.QKV_B], fl[N.QKV_COLSUM] = (t.to(dev) for t in self._fold(cpu(src["ln1_g"]), cpu(src["ln1_b"]), cpu(src["qkv_w"]), cpu(src["qkv_b"]), row_scale=qs))
                fl[N.FC1_W], fl[N.FC1_B], fl[N.FC1_COLSUM] = (t.to(dev) for t in self._fold(cpu(src["ln2_g"]), cpu(src["ln2_b"]), cpu(src["fc1_w"]), cpu(src["fc1_b"])))
                self.fold_layers.append(fl)
            self.q_row_scale = qs.to(dev)                          # (attn_variant == 1 takes Q unscaled: all ones then)
        # The MLP hidden in MFMA-fragment order (blk16.py; include/ucod_dpl.h "BLK16"): fc2's weight once more with the layout's column permutation, built here
        # because the weights are frozen.  The driver uses it for the layers whose fc1 is LayerNorm-folded GELU on passes large enough for the large-tile kernels and
        # the plain weight everywhere else; UCOD_MLP_ROWMAJOR=1 (read once, at import) builds no permuted copy: every pass then runs the row-major pair.
        self.fc2_perm = None
        if self.ln_fold and self.mlp == N.UCOD_MLP_GELU and self.F % 64 == 0 and not _MLP_ROWMAJOR:
            from .blk16 import pi
            self._fc2_pi = pi(self.F).to(dev)
            self.fc2_perm = [torch.index_select(l[N.FC2_W], 1, self._fc2_pi) for l in self.layers]

    def refresh_fc2_perm(self, i):
        """Rebuild layer i's permuted fc2 weight from the plain one, in place (``ViTLoRAEngine.merge_into`` after it has written a merged fc2 weight)."""
        if self.fc2_perm is not None:
            torch.index_select(self.layers[i][N.FC2_W], 1, self._fc2_pi, out=self.fc2_perm[i])

    def _fc2_perm_table(self, n_layers=None):
        """ctypes table of the permuted fc2 weights of a pass over the first n_layers layers, or None (the row-major pair)."""
        if self.fc2_perm is None:
            return None
        L = self.L if n_layers is None else n_layers
        return (C.c_void_p * L)(*[t.data_ptr() for t in self.fc2_perm[:L]])

    def _fold(self, gamma, beta, w, b, row_scale=None):
        """LayerNorm(gamma, beta) followed by Linear(w, b) [* row_scale per output] as one GEMM on the un-normalised rows (include/ucod_dpl.h:
        ucod_gemm_lnfold): W' = 16-bit(q (.) W (.) gamma), column sums of the ROUNDED W' (what the MFMA multiplies by), b' = q (W beta + b) in f64."""
        from .fold import fold_layernorm_linear
        return fold_layernorm_linear(gamma, beta, w, b, row_scale=row_scale, half=torch.float16)      # (the fold exists in the fp16-operand build only)

    def _rows(self, L=None):
        """The rows of a pass over the first L layers.  With ln_fold every layer but the last OF THE PASS contributes its folded entries; the last keeps the
        plain ones (its LayerNorm 1 runs as a kernel and feeds the key hook)."""
        if not self.ln_fold:
            return self.layers
        last = (self.L if L is None else L) - 1
        return [l if i == last else fl for i, (l, fl) in enumerate(zip(self.layers, self.fold_layers))]

    def param_bytes(self):
        # the folded tables are a SECOND copy of every layer's QKV / fc1 weights (+ their folded biases and column sums); the plain copies stay because
        # the last layer of a (possibly truncated) pass runs unfolded
        # (+ the column-permuted copy of every fc2 weight: the BLK16 hidden)
        return super().param_bytes() + sum(t.numel() * t.element_size() for fl, l in zip(self.fold_layers or (), self.layers)
                                           for t, t0 in zip(fl, l) if t is not None and t is not t0) + sum(t.numel() * t.element_size() for t in self.fc2_perm or ())

    def check_overflow(self, wait=False):
        """Raise FloatingPointError if any finished pass saturated the fp16 residual stream.  ``wait``: block until every pass enqueued so far
        has finished (otherwise only passes that already have)."""
        n = self._guard.take(wait)
        if n > 0:
            how = "build the engine with resid='f32'" if self.resid16 else "call forward_nograd(..., resid16=False)"
            raise FloatingPointError(f"the fp16 residual stream of this engine saturated at +-65504 (or met a NaN) in {n} wave-lane(s)"
                                     + (" -- or a folded LayerNorm met a row with |mean| > 256 sigma (outside the fold's range)" if self.ln_fold else "")
                                     + f": the activations do not fit this configuration; {how}.  The counter is polled without blocking: the pass (or, for a training engine, the "
                                     f"optimiser step or steps) that consumed the clamped activations has already been applied -- discard its results "
                                     f"(UCOD_CHECK_RESID=1 checks synchronously after every pass).")

    _sync_check = os.environ.get("UCOD_CHECK_RESID") == "1"    # debug: check the saturation counter synchronously after every pass

    def forward(self, img, out=None, _async=False, n_layers=None):
        """``n_layers``: stop after that many encoder layers and return THAT layer's key map (diagnostics: the per-layer error
        table of bench.py); default = the whole backbone."""
        img, key, H, W = self._inputs("ViTEngine", img, out, n_layers)
        B = img.shape[0]
        table, _keep = self._table(H // self.P, W // self.P, self._rows(n_layers))
        perm = self._fc2_perm_table(n_layers)
        self.check_overflow()                                      # (non-blocking) passes that have finished since the last call

        def launch(b0, b1, ws):
            """images b0..b1 on the current stream, in ``ws`` or a larger workspace, which is returned"""
            d = self._desc(b1 - b0, H, W, n_layers)
            ws = self._workspace(ws, self.lib.ucod_vit_workspace_bytes_mlp(C.byref(d), self.mlp))
            with self._guard.bind():
                N.check(self.lib.ucod_vit_forward_blk16(C.byref(d), self.mlp, table, perm, N.ptr(img[b0:b1]), N.ptr(key[b0:b1]), N.ptr(ws), ws.numel(), N.stream()),
                        "ucod_vit_forward")
            if self.resid16:
                self._guard.arm(torch.cuda.current_stream(self.device))
            return ws

        ns = max(1, min(int(self.streams), B))
        if ns == 1 and not _async:
            self._ws = launch(0, B, self._ws)
            if self._sync_check:
                self.check_overflow(wait=True)
            return key
        # Image-parallel sub-batches on independent HIP streams: every kernel of the pass is per-image, so the halves are
        # independent and the tail of one stream's GEMM (a partial last round of 256-row tiles leaves most CUs idle) is filled by
        # the other stream's next kernel.  Results are identical to the single-stream pass (same kernels, same per-image math).
        if self._side is None or len(self._side) != ns:
            # Normal priority.  High-priority side streams (UCOD_SIDE_PRIORITY=-1) were measured: nothing on the pipelined frozen-backbone
            # step (10.16 vs 10.19 ms) and MINUS 17 % in backbone-backward mode (585 vs 702 images/s: the EMA teacher's pass on these
            # streams then starves the student's forward / backward on the training streams).
            prio = int(os.environ.get("UCOD_SIDE_PRIORITY", "0"))
            self._side = [torch.cuda.Stream(device=self.device, priority=prio) for _ in range(ns)]
            self._side_ws = [None] * ns

        def run(i, b0, b1):
            self._side_ws[i] = launch(b0, b1, self._side_ws[i])

        events = self._fan_out(self._side, _chunk_bounds(B, ns), run, (img, key), wait=not _async)
        if _async:
            return key, events
        if self._sync_check:
            self.check_overflow(wait=True)
        return key

    def forward_with_cls_attention(self, img, allow_rope=False):
        """(key [B,D,h,w], att [B,heads,h*w]): the key map plus ``outputs.attentions[-1][:, :, 0, 1:]`` of the HF model -- the CLS
        query's softmax row of the LAST layer, which is all the pseudo-label generator reads from the attentions
        (data/utils/found_bkg_mask.py:23; generate_pseudo_label.py:78-89).  Single-stream pass: the CLS projections are taken
        from the LayerNorm-1 output the pass leaves in its workspace.
        ``allow_rope``: on a DINOv3 checkpoint the method refuses without it; with it the row is ``attentions[-1][:, :, 0, 1 + R:]`` of DINOv3ViTModel, the patch
        keys rotated inside the row kernel (the key map returned stays the unrotated hook output).  On every other checkpoint it changes nothing."""
        if self.rope and not allow_rope:
            self._refuse_rope("forward_with_cls_attention", _CLS_ROW_ON_ROPE, _CLS_ROW_WAY_IN)
        if self.full_last_layer:
            raise RuntimeError("forward_with_cls_attention needs the key-minimal pass (full_last_layer=False)")
        ns, self.streams = self.streams, 1
        try:
            key = self.forward(img)
        finally:
            self.streams = ns
        B, _, H, W = img.shape
        lib = self.lib
        d = self._desc(B, H, W)
        off = lib.ucod_vit_last_ln1_offset_mlp(C.byref(d), self.mlp)
        R = self.R
        tok = self.tokens(key.shape[-2], key.shape[-1])
        last = self.layers[-1]
        q = torch.empty(B, self.D, dtype=torch.float32, device=self.device)
        k = torch.empty(B, 1 + R, self.D, dtype=torch.float32, device=self.device)      # the keys of CLS and of the R register tokens (in the softmax, not in the row)
        N.check(lib.ucod_cls_qk_reg(self._ws.data_ptr() + off, N.ptr(last[N.QKV_W]), N.ptr(last[N.QKV_B]), N.ptr(q), N.ptr(k), B, tok, self.D, R, N.stream()), "ucod_cls_qk")
        return key, self._cls_row(q, k, key, R)

    __call__ = forward


class SplitViTEngine(_BackboneEngine):
    """The frozen backbone at the REFERENCE's cached-feature precision: HIP ViT forward -> last-layer key map [B, D, H/P, W/P] (f32) with every matrix product
    computed on split operands (include/ucod_dpl.h: "split-operand backbone pass"; csrc/split.hip) -- f32 residual stream, f32 LayerNorm, exact-erf GELU,
    f32 softmax, each f32 GEMM / attention operand as a sum of ``terms`` bf16 values on the bf16 MFMA:

    * ``terms=2``: 16 significand bits per operand, 3x the matrix work of the 16-bit engines; mask logits within ~3e-5 of the f32 oracle at full size on the
      trained-like weights (tests/test_gpu_split.py), i.e. the configuration that meets the 1e-3 bar where the 16-bit engines do not;
    * ``terms=3`` (default): 24 bits, f32-equivalent, 6x -- what ``build_feature_cache`` uses by default, because the reference runs that pass in plain fp32
      (/root/reference/data/datasets/base_dataset.py:124-138: no autocast) and its speed does not matter.

    Same call interface as ``ViTEngine`` (``forward`` / ``forward_async`` / ``__call__``, ``D``, ``P``, ``streams``); key-minimal pass only."""

    def __init__(self, state_dict, heads, eps=1e-6, device="cuda", terms=3, gemm_variant=0, term="bf16", fuse_mlp=False, rope_theta=100.0):
        """``rope_theta``: as ``ViTEngine``.
        ``term="f16"`` (with ``terms=2``; precision name "split2h"): the two terms of every operand are IEEE fp16 values of a power-of-two multiple of it and the three
        partial products run on the fp16 MFMA (csrc/split16.hip, libucod_dpl_f16.so) -- 22 significand bits per operand at the matrix work of ``terms=2``.  Weights are
        scaled per tensor at load (largest magnitude into [2^13, 2^14)), activations per operand class (``ops.split16_class_scale``); a value beyond fp16's range
        is clamped and counted on the device, and ``check_overflow`` raises for a pass that met one.
        ``fuse_mlp=True`` (fp16 terms only; precision name "split2hf"): fc1, its activation and the split of the result run as ONE launch (ucod_split16_gemm_act)
        instead of the f32 GEMM epilogue followed by a row pass, and the workspace holds no f32 fc1 buffer.  The drain calls the row pass's own functions on the same
        f32 value: the key map is that of ``fuse_mlp=False`` up to the summation order of fc1's leftover tiles."""
        if terms not in (2, 3):
            raise ValueError(f"terms must be 2 or 3, got {terms!r}")
        if term not in ("bf16", "f16"):
            raise ValueError(f"term must be 'bf16' or 'f16', got {term!r}")
        if term == "f16" and terms != 2:
            raise ValueError(f"term='f16' is the two-term form: terms must be 2, got {terms!r}")
        if fuse_mlp and term != "f16":
            raise ValueError(f"fuse_mlp=True exists for the fp16-term form only (terms=2, term='f16'), got terms={terms!r}, term={term!r}")
        self.terms, self.term, self.half = int(terms), term, f"{term}x{int(terms)}"
        self.fuse_mlp = bool(fuse_mlp)
        self._flags = N.SPLIT16_FUSE_MLP if self.fuse_mlp else 0
        f16 = term == "f16"
        c, pw = self._setup(state_dict, heads, eps, device, gemm_variant, "f16" if f16 else "bf16", rope_theta)    # (each term type has its MFMA; either build refuses the other's split entry points)
        self.nprod = ops.split_products(terms)
        f32, D = self._f32, self.D
        sw = lambda t, s=1.0, role=1: ops.split_rows(f32(t), self.terms, role, term=term, scale=s)  # noqa: E731      (role 1: weights are the B side of y = x W^T)
        # fp16 terms: every weight carries a power-of-two scale s_w, and S = (activation class scale) x s_w of each GEMM goes into its bias (for the patch embedding
        # also the CLS and position rows) and out of its LayerScale vector, so that the stream is bit for bit what the unscaled product would give (csrc/split16.hip)
        wscale = ops.pow2_scale if f16 else (lambda t: 1.0)
        act = [ops.split16_class_scale(k) for k in (N.SPLIT16_LN, N.SPLIT16_ATT, N.SPLIT16_LN, N.SPLIT16_HIDDEN)] if f16 else None
        self.wscale = [wscale(pw)]                                # [patch, (qkv, proj, fc1, fc2) x L]: what the fp16-term driver reads
        self.patch_w, self.patch_b, self.cls = sw(pw, self.wscale[0]), f32(c["patch_b"]), self._lead_rows()
        if f16:
            self._pos_scale = ops.split16_class_scale(N.SPLIT16_PATCH) * self.wscale[0]
            self.patch_b, self.cls = self.patch_b * self._pos_scale, self.cls * self._pos_scale
        for l in c["layers"]:
            s = {g + "_w": wscale(l[g + "_w"]) for g in _GEMMS}
            self.wscale += s.values()
            self.layers.append(layer_row(l, lambda t, name: sw(t, s[name]), f32, scales=[a * w for a, w in zip(act, s.values())] if f16 else None,
                                         aux=(sw(l["qkv_w"][D:2 * D], s["qkv_w"], role=0), None)))       # +14: the K rows as the A side of the key hook's GEMM
        self._wscale_c = (C.c_float * len(self.wscale))(*self.wscale)
        last = c["layers"][-1]                        # f32 copies for forward_with_cls_attention: the CLS query / key of the LAST layer
        self._last = dict(ln_g=f32(last["ln1_g"]), ln_b=f32(last["ln1_b"]), wq=f32(last["qkv_w"][:D]), bq=f32(last["qkv_b"][:D]),
                          wk=f32(last["qkv_w"][D:2 * D]), bk=f32(last["qkv_b"][D:2 * D]))

    def _wscale_of(self, layer, gemm):
        """the weight scale of ``layer``'s GEMM ``gemm`` (a name of _GEMMS) in ``wscale``"""
        return self.wscale[1 + len(_GEMMS) * layer + _GEMMS.index(gemm)]

    def check_overflow(self, wait=False):
        """bf16 terms: nothing can saturate (bf16 has f32's range; interface of ViTEngine).  fp16 terms: raise FloatingPointError if a finished pass clamped an
        operand to +-65504 (or met a NaN) -- its key map is wrong and must be discarded.  ``wait``: block until every pass enqueued so far has finished."""
        if self.term != "f16":
            return None
        n = self._guard.take(wait)
        if n > 0:
            raise FloatingPointError(f"the fp16-term split pass (split2h / split2hf) clamped {n} operand element(s) to +-65504 (or met a NaN): an activation exceeded the bound of its "
                                     f"operand class (csrc/split16.hip) and the key maps of that pass are wrong -- use precision='split3' ('f32eq') for this checkpoint / "
                                     f"input.  The counter is polled without blocking; check_overflow(wait=True) checks every pass enqueued so far.")

    def _ws_bytes(self, d):
        if self.term == "f16":
            return self.lib.ucod_vit_split16_workspace_bytes_ex(C.byref(d), self.mlp, self._flags)
        return self.lib.ucod_vit_split_workspace_bytes_mlp(C.byref(d), self.terms, self.mlp)

    def _stream_offset(self, d):
        if self.term == "f16":
            return self.lib.ucod_vit_split16_stream_offset_ex(C.byref(d), self.mlp, self._flags)
        return self.lib.ucod_vit_split_stream_offset_mlp(C.byref(d), self.terms, self.mlp)

    def _run(self, img, key, ws, n_layers=None):
        """The pass on the current stream, in ``ws`` or a larger workspace, which is returned."""
        B, _, H, W = img.shape
        d = self._desc(B, H, W, n_layers)
        ws = self._workspace(ws, self._ws_bytes(d))
        table, _keep = self._table(H // self.P, W // self.P)
        if self.term == "f16":
            self.check_overflow()                                  # (non-blocking) passes that have finished since the last call
            with self._guard.bind():
                N.check(self.lib.ucod_vit_forward_split16_ex(C.byref(d), self.mlp, self._flags, table, self._wscale_c, 1 + len(_GEMMS) * d.L, N.ptr(img), N.ptr(key),
                                                             N.ptr(ws), ws.numel(), N.stream()), "ucod_vit_forward_split16_ex")
            self._guard.arm(torch.cuda.current_stream(self.device))
        else:
            N.check(self.lib.ucod_vit_forward_split_mlp(C.byref(d), self.terms, self.mlp, table, N.ptr(img), N.ptr(key), N.ptr(ws), ws.numel(), N.stream()),
                    "ucod_vit_forward_split")
        return ws

    def forward(self, img, out=None, _async=False, n_layers=None):
        img, key, H, W = self._inputs("SplitViTEngine", img, out, n_layers)
        if not _async:
            self._ws = self._run(img, key, self._ws, n_layers)
            return key
        # forward_async: the whole pass on ONE side stream (its workspace is several GB at batch 32: no image-parallel halves here)
        if self._side is None:
            self._side, self._side_ws = [torch.cuda.Stream(device=self.device)], [None]

        def run(i, b0, b1):
            self._side_ws[i] = self._run(img, key, self._side_ws[i], n_layers)

        return key, self._fan_out(self._side, _chunk_bounds(img.shape[0], 1), run, (img, key), wait=False)

    def forward_with_cls_attention(self, img, allow_rope=False):
        """(key [B,D,h,w], att [B,heads,h*w]) like ``ViTEngine.forward_with_cls_attention`` (``allow_rope`` included): the key map plus ``outputs.attentions[-1][:, :, 0, 1:]`` of the HF model
        (data/utils/found_bkg_mask.py:23; generate_pseudo_label.py:78-89 -- a plain fp32 pass under torch.no_grad() in the reference, which is why the
        pseudo-label generator asks for this engine).  The CLS rows of the last layer's input are taken from the f32 residual stream the pass leaves in its
        workspace, normalised by the f32 LayerNorm kernel, projected to the CLS query / key on split operands, and fed to the f32 attention-row kernel."""
        if self.rope and not allow_rope:
            self._refuse_rope("forward_with_cls_attention", _CLS_ROW_ON_ROPE, _CLS_ROW_WAY_IN)
        key = self.forward(img)
        B, _, H, W = img.shape
        off = self._stream_offset(self._desc(B, H, W))
        R = self.R
        tok = self.tokens(key.shape[-2], key.shape[-1])
        x = self._ws[off:off + B * tok * self.D * 4].view(torch.float32).view(B, tok, self.D)
        L_ = self._last
        # the CLS row and the R register rows of every image: all of them are keys of the CLS query's softmax, only the CLS row is a query
        h_lead = ops.layernorm(x[:, :1 + R].reshape(B * (1 + R), self.D).contiguous(), L_["ln_g"], L_["ln_b"], self.eps, out_f32=True)
        h_cls = h_lead if R == 0 else h_lead.view(B, 1 + R, self.D)[:, 0].contiguous()
        if self.term == "f16":
            # the scales of the pass itself, known at load: the LayerNorm class scale for the rows, the last layer's QKV weight scale (no device-to-host read here)
            sc = dict(term="f16", x_scale=ops.split16_class_scale(N.SPLIT16_LN), w_scale=self._wscale_of(self.L - 1, "qkv"))
            with self._guard.bind():
                q = ops.linear_split(h_cls, L_["wq"], L_["bq"], 2, **sc)
                k = ops.linear_split(h_lead, L_["wk"], L_["bk"], 2, **sc)
            self._guard.arm(torch.cuda.current_stream(self.device))
        else:
            q = ops.linear_split(h_cls, L_["wq"], L_["bq"], self.terms)
            k = ops.linear_split(h_lead, L_["wk"], L_["bk"], self.terms)
        return key, self._cls_row(q, k.contiguous(), key, R)

    __call__ = forward


_MASK64 = 0xFFFFFFFFFFFFFFFF
LORA_OUT_MAX_K = 4096                                        # include/ucod_dpl.h: the widest input the output projections' LoRA kernels take

# ---- LoRA mode: the six Linear modules of a layer that can carry an adapter, in arena / bias-table order (native.VIT_TRAIN_BIAS_SLOTS) ------------------------
_Q, _K, _V, _MLP_IN, _ATTN_OUT, _MLP_OUT = range(N.VIT_TRAIN_BIAS_STRIDE)
# their leaf names.  DINOv2 (HF Dinov2Model / ViTModel): q / k / v, the MLP input by MLP kind (modeling_dinov2.py:281-297 / :300-315), the output projections
# ``allow_out`` builds; DINOv3ViTModel's in the same order (its gated MLP keeps the plain one's names)
_QKV, _MLP_IN_LEAF, _OUT = ("query", "key", "value"), {"gelu": "fc1", "swiglu": "weights_in"}, ("dense", "fc2")
_QKV3, _OUT3 = ("q_proj", "k_proj", "v_proj"), ("o_proj", "down_proj")
# where each of the six lives in a frozen engine's row: weight, bias and column-sum slot, the LayerNorm folded into it (gamma, beta; none in front of an output
# projection)
_ENGINE_SLOTS = (((N.QKV_W, N.QKV_B, N.QKV_COLSUM, (N.LN1_G, N.LN1_B)),) * 3
                 + ((N.FC1_W, N.FC1_B, N.FC1_COLSUM, (N.LN2_G, N.LN2_B)), (N.PROJ_W, N.PROJ_B, None, None), (N.FC2_W, N.FC2_B, None, None)))


_MLP_IN2 = _MLP_OUT + 1                                     # the gated DINOv3 MLP's second input module (``lora_module_paths`` with ``pair``), behind the six


def lora_module_paths(family, mlp="gelu", pair=False):
    """The six modules' HF paths below ``{layer path}{i}.`` -- query, key, value, MLP input, attention output, MLP output -- of a checkpoint family ("dinov2": HF
    Dinov2Model / ViTModel; "dinov3": DINOv3ViTModel, whose gated MLP keeps the plain one's names) and MLP kind ("gelu" | "swiglu").
    ``pair`` (DINOv3's gated MLP, whose input is TWO peft modules on the one fused weights_in): seven paths -- ``mlp.gate_proj`` in the MLP input's place and
    ``mlp.up_proj`` behind the six (``_MLP_IN2``), so that every index of the six keeps its meaning."""
    if family == "dinov3" and pair:
        return tuple("attention." + n for n in _QKV3) + ("mlp.gate_proj", "attention." + _OUT3[0], "mlp." + _OUT3[1], "mlp.up_proj")
    if family == "dinov3":
        return tuple("attention." + n for n in _QKV3) + ("mlp.up_proj", "attention." + _OUT3[0], "mlp." + _OUT3[1])
    return (tuple("attention.attention." + n for n in _QKV)
            + ("mlp." + _MLP_IN_LEAF[mlp], "attention.output." + _OUT[0], "mlp." + (_OUT[1] if mlp == "gelu" else "weights_out")))


class LoRAModule(typing.NamedTuple):
    """One of the six modules as a ``ViTLoRAEngine`` holds it (``lora_modules``).  A is [r, k], B is [n, r]; ``k`` / ``n`` are the input width and row count in the
    engine, ``k_hf`` / ``n_hf`` in the checkpoint -- they differ only on the SwiGLU MLP, whose hidden width is padded to a multiple of 128 and whose ``weights_in``
    rows are interleaved (swiglu.py)."""
    path: str                  # below the layer path: "attention.attention.query", "attention.q_proj", "mlp.weights_in" ...
    targeted: bool
    k: int
    n: int
    k_hf: int
    n_hf: int
    a: slice                   # A and B in a layer's arena row; None for an untargeted module without a place in it (q / k / v always have theirs)
    b: slice
    bias_off: int              # the trained bias [n] in the arena row, or None (bias="none", not targeted, or no bias in the checkpoint)
    bias_cols: slice           # its bias in ``_bias_flat``
    w_slot: int                # the frozen engine's row: weight, bias, column sums (None: never folded), (gamma, beta) of the folded LayerNorm or None
    b_slot: int
    c_slot: int
    ln: tuple
    row0: int                  # its first row in that weight / bias (the fused QKV weight holds three modules)
    interleaved: bool          # rows in the engine's padded, interleaved order (SwiGLU ``weights_in``): B and the bias go through swiglu.lora_b_{to,from}_engine
    part: int = None           # 0 / 1: gate_proj / up_proj of the gated DINOv3 MLP.  The two share ONE B block (``b``) and ONE bias of 2n rows in the fused weights_in's
    #                            4-interleaved order -- row 8k + 4 part + e of the block is this module's row 4k + e (``n`` = the padded hidden width F, ``n_hf`` = F0)

    @property
    def leaf(self):
        return self.path.rsplit(".", 1)[-1]

    @property
    def nb(self):
        """rows of the B block ``b`` and of the bias in the arena: ``n``, or 2n for a module that shares them with its partner (``part``)"""
        return self.n if self.part is None else 2 * self.n

    def get_rows(self, block):
        """This module's rows of ``block`` [nb, c] (its B block, or its bias as [nb, 1], in the engine's order) as the checkpoint has them: [n_hf, c].  A copy where
        the orders differ, the tensor itself where they agree."""
        if self.part is None:
            return self.rows_to_hf(block)
        return block.reshape(self.n // 4, 2, 4, -1)[:, self.part].reshape(self.n, -1)[:self.n_hf]

    def set_rows(self, block, v):
        """The inverse: write ``v`` [n_hf, c] into this module's rows of ``block`` [nb, c] IN PLACE (padded rows: zeros; a partner's rows are not touched)."""
        if self.part is None:
            block.copy_(self.rows_from_hf(v))
            return
        rows = v.new_zeros(self.n, v.shape[1])
        rows[:self.n_hf] = v
        block.view(self.n // 4, 2, 4, -1)[:, self.part] = rows.view(self.n // 4, 4, -1)

    def a_to_hf(self, a):
        """A [r, k] as the checkpoint's names carry it, [r, k_hf]: the padded hidden units' columns (zeros) are dropped."""
        return a[:, :self.k_hf]

    def a_from_hf(self, a):
        return a if self.k == self.k_hf else torch.nn.functional.pad(a, (0, self.k - self.k_hf))

    def rows_to_hf(self, v):
        """B [n, r] (or the bias as [n, 1]) in the checkpoint's row order, [n_hf, ...]; the tensor itself where the orders agree."""
        return lora_b_from_engine(v, self.n_hf // 2) if self.interleaved else v

    def rows_from_hf(self, v):
        return lora_b_to_engine(v) if self.interleaved else v


def lora_modules(family, mlp, D, F, F0, r, hit, bias="none", has_bias=(True,) * 7):
    """The module table of a LoRA engine: six ``LoRAModule`` in the order query, key, value, MLP input, attention output, MLP output.  Host only.
    With SEVEN answers in ``hit`` (a gated DINOv3 checkpoint with one of gate_proj / up_proj targeted) the table has seven: ``mlp.gate_proj`` in the MLP input's
    place, ``mlp.up_proj`` last; the two are peft modules of their own (own A, own rows of B, HF's names and shapes outside the arena) over one arena block
    [A_g | A_u | B_m] where [A_m | B_m] would stand -- the layout of ucod_lora_mlp_pair_grad (include/ucod_dpl.h).
    ``family`` / ``mlp``: ``lora_module_paths``; ``D``: the width; ``F`` / ``F0``: the MLP's hidden width in the engine (SwiGLU: padded) and in the checkpoint;
    ``r``: the rank; ``hit``: which of the six are targeted (``resolve_lora_targets``); ``bias``: peft's mode; ``has_bias``: which have a bias in the checkpoint.
    A layer's arena row is  [A_q | B_q | A_k | B_k | A_v | B_v]  -- always, an untargeted one's at zero --, then [A | B] of the MLP input, the attention output and
    the MLP output where targeted, then (bias="lora_only") the biases of the targeted modules that have one -- (bias="all") of every module that has one, targeted
    or not -- in the same order (``lora_row_numel``); bias="all" puts [beta1 | beta2 | b_patch] behind them (``lora_norm_offsets``)."""
    swiglu = mlp == "swiglu"
    N1, N0 = (2 if swiglu else 1) * F, (2 if swiglu else 1) * F0
    pair = len(hit) > _MLP_IN2                                   # seven answers: the gated DINOv3 MLP's gate_proj / up_proj (``lora_module_paths`` with ``pair``)
    if pair and not (family == "dinov3" and swiglu):
        raise ValueError("a seventh module exists on a DINOv3 checkpoint with the gated MLP only")
    shapes = ((D, D, D, D),) * 3 + ((D, N1, D, N0), (D, D, D, D), (F, D, F0, D))          # (k, n, k_hf, n_hf)
    mods, at, col = [], 0, 0
    for j, (path, (k, n, k_hf, n_hf)) in enumerate(zip(lora_module_paths(family, mlp, pair), shapes)):
        a = b = None
        if pair and j == _MLP_IN:
            # the pair's one arena block [A_g | A_u | B_m (N1 x r)], there whenever one of the two is targeted (the other's A and rows of B then stay zero); this
            # entry is gate_proj, its partner (built below, behind the six) up_proj: each has its own A, both name the B block and the fused bias
            a, a_up, b = slice(at, at + r * k), slice(at + r * k, at + 2 * r * k), slice(at + 2 * r * k, at + r * (2 * k + N1))
            at = b.stop
            mods.append(LoRAModule(path, bool(hit[j]), k, F, k_hf, F0, a, b, None, slice(col, col + N1), *_ENGINE_SLOTS[j], 0, False, 0))
            col += N1
            continue
        if j <= _V or hit[j]:
            a, b = slice(at, at + r * k), slice(at + r * k, at + r * (k + n))
            at = b.stop
        mods.append(LoRAModule(path, bool(hit[j]), k, n, k_hf, n_hf, a, b, None, slice(col, col + n), *_ENGINE_SLOTS[j], j * D if j <= _V else 0,
                               swiglu and j == _MLP_IN))
        col += n
    if pair:
        g = mods[_MLP_IN]
        mods.append(g._replace(path=lora_module_paths(family, mlp, True)[_MLP_IN2], targeted=bool(hit[_MLP_IN2]), a=a_up, part=1))
    for j, m in enumerate(mods):
        if ((bias == "lora_only" and m.targeted) or bias == "all") and has_bias[j]:
            if m.part == 1 and mods[_MLP_IN].bias_off is not None:
                mods[j] = m._replace(bias_off=mods[_MLP_IN].bias_off)        # (the fused bias: one slot for both)
            else:
                mods[j], at = m._replace(bias_off=at), at + m.nb
    return tuple(mods)


def lora_row_numel(mods, bias="none"):
    """Length of a layer's arena row (bias="all": with the three vectors of ``lora_norm_offsets`` at its end)."""
    n = max([m.b.stop for m in mods if m.b is not None] + [m.bias_off + m.nb for m in mods if m.bias_off is not None])
    return n + (3 * mods[_Q].k if bias == "all" else 0)


def lora_norm_offsets(mods, bias="none"):
    """bias="all": where a layer's arena row holds (norm1.bias, norm2.bias, the patch embedding's bias), D values each, behind the Linear biases; None otherwise.
    The patch bias is live in row 0 only: in every other row its block holds exact zeros and is never read."""
    if bias != "all":
        return None
    at, D = lora_row_numel(mods), mods[_Q].k
    return at, at + D, at + 2 * D


# ---- target_modules -> which of the six --------------------------------------------------------------------------------------------------------------------------
_REFUSED = {                                                 # DINOv2 names: why a module of that leaf name is not built (``allow_out`` lifts dense / fc2)
    "dense": "its input is written by the attention kernel, which has no leading-dimension argument for the 64 LoRA columns",
    "fc2": "its input is written by the fc1 GEMM's drain, which has no leading-dimension argument for the 64 LoRA columns",
    "weights_out": "its input is written by the weights_in GEMM's drain, which has no leading-dimension argument for the 64 LoRA columns",
    "projection": "the patch embedding is a convolution over im2col rows, not a LayerNorm output",
}
_SWIGLU_OUT = ("its input, the SwiGLU hidden, is not a saved activation: it would have to be recomputed from the interleaved, padded [M, 2F] pre-activation, "
               "which is not built yet")
# (what the refusal says once that recomputation exists: the message above stays, with the way in behind it)
_SWIGLU_OUT_OPT_IN = _SWIGLU_OUT + ".  That recomputation runs only with the opt-in allow_swiglu_out=True (beside allow_out and allow_swiglu)"
_REFUSED3 = {                                                # DINOv3 names (``allow_out`` lifts o_proj and the plain MLP's down_proj)
    "o_proj": "its input is written by the attention kernel, which has no leading-dimension argument for the 64 LoRA columns",
    "down_proj": "its input is written by the MLP input GEMM's drain, which has no leading-dimension argument for the 64 LoRA columns",
    "up_proj": "the MLP input projection of a DINOv3 checkpoint is not built yet (on the gated MLP it is one of two peft modules, with gate_proj, on the one fused "
               "weights_in GEMM)",
    "gate_proj": "the gated MLP's input is two peft modules (gate_proj, up_proj) on the one fused weights_in GEMM: a LoRA module on one of them alone is not built",
    "patch_embeddings": "the patch embedding is a convolution over im2col rows, not a LayerNorm output",
}
_MLP_IN3 = ("gate_proj", "up_proj")                          # DINOv3's MLP input modules: what ``allow_mlp_in`` lifts
# (what their refusals say now that they are built: the messages above stay, with the way in behind them)
_MLP_IN_OPT_IN = (".  It runs only with the opt-in allow_mlp_in=True: up_proj on the fc1 GEMM's 64 extra K columns, the gated MLP's gate_proj / up_proj as a pair "
                  "of modules with a block-diagonal B (ucod_lora_mlp_pair_grad)")
LORA_MLP_MAX_N1 = 8192                                       # include/ucod_dpl.h: the most rows of the MLP input weight its gradient kernels take
_DINOV2_LEAVES = ("query", "key", "value", "dense", "fc1", "fc2", "weights_in", "weights_out", "projection")


class _Names(typing.NamedTuple):
    """What target resolution knows of a checkpoint family: the data in which ``lora_targets`` and ``lora_targets_dinov3`` differ."""
    layer_path: str            # in front of the layer number
    paths: tuple               # the six modules below it (``lora_module_paths``)
    more: tuple                # what else peft's suffix rule can name: further modules of a layer ...
    patch: str                 # ... and the patch embedding
    refused: dict              # leaf name -> why a module of that name is not built, under the opt-ins given
    ask: str                   # what an empty list is told to choose from
    foreign: typing.Callable   # (target, its last component) -> "that is the other family's name", or None
    swiglu: bool


def _dinov2_names(mlp, allow_out, allow_swiglu_out):
    refused = dict({k: v for k, v in _REFUSED.items() if k not in _OUT}, weights_out=_SWIGLU_OUT_OPT_IN) if allow_out else _REFUSED
    if allow_swiglu_out:
        refused = {k: v for k, v in refused.items() if k != "weights_out"}
    mlp_in, other = _MLP_IN_LEAF[mlp], _MLP_IN_LEAF["swiglu" if mlp == "gelu" else "gelu"]

    def foreign(t, last):
        if last == other:
            return f"target module {t!r}: this checkpoint has the {mlp.upper() if mlp == 'gelu' else 'SwiGLU'} MLP, whose input projection is {mlp_in!r}, not {other!r}"

    return _Names("encoder.layer.", lora_module_paths("dinov2", mlp), (), "embeddings.patch_embeddings.projection", refused, "query / key / value", foreign, mlp == "swiglu")


def _dinov3_names(gated, layer_path, allow_out, allow_swiglu_out, allow_mlp_in=False):
    refused = _REFUSED3
    if allow_out:
        refused = {k: v for k, v in _REFUSED3.items() if k not in _OUT3}
        if gated and not allow_swiglu_out:
            refused["down_proj"] = _SWIGLU_OUT_OPT_IN
    if allow_mlp_in:       # (on the plain MLP ``gate_proj`` names no module: its reason stays in the table for the "no such module" refusal)
        refused = {k: v for k, v in refused.items() if k not in (_MLP_IN3 if gated else _MLP_IN3[1:])}
    else:
        refused = dict(refused, **{k: _REFUSED3[k] + _MLP_IN_OPT_IN for k in _MLP_IN3})

    def foreign(t, last):
        if last in _DINOV2_LEAVES:
            return (f"target module {t!r} is a DINOv2 name: a DINOv3 checkpoint's attention projections are q_proj / k_proj / v_proj "
                    f"({layer_path}{{i}}.attention.{{q,k,v}}_proj)")

    if gated and allow_mlp_in:                                   # seven modules to choose from: gate_proj in the MLP input's place, up_proj behind the six
        return _Names(layer_path, lora_module_paths("dinov3", "swiglu", True), (), "embeddings.patch_embeddings", refused, "q_proj / k_proj / v_proj", foreign, True)
    return _Names(layer_path, lora_module_paths("dinov3"), ("mlp.gate_proj",) if gated else (), "embeddings.patch_embeddings", refused, "q_proj / k_proj / v_proj",
                  foreign, bool(gated))


def _check_swiglu_out(allow_out, allow_swiglu_out):
    if allow_swiglu_out and not allow_out:
        raise ValueError("allow_swiglu_out=True needs allow_out=True: the SwiGLU MLP's output projection is one of the output projections")


# (what the two width refusals below say now that wider kernels exist: their messages stay, with the way in behind them where it leads anywhere)
_WIDE_OPT_IN = (".  Wider kernels run only with the opt-in allow_wide_mlp=True: the MLP input's gradient kernel with five vectors per thread and one rank per pass "
                f"(N1 <= {N.LORA_WIDE_MAX_N1}), the output projection's forward in blocks of 512 threads (K <= {N.LORA_WIDE_MAX_K})")


def _check_swiglu_out_width(name, hidden, allow_wide_mlp=False):
    """The SwiGLU MLP's output projection is targeted: refuse a hidden width the kernels do not cover, here, before anything touches the device."""
    top = N.LORA_WIDE_MAX_K if allow_wide_mlp else LORA_OUT_MAX_K
    if hidden is not None and padded_hidden(hidden) > top:
        raise NotImplementedError(f"LoRA target module {name!r} is not built for this checkpoint: its input width K = {padded_hidden(hidden)} (the MLP's hidden width "
                                  f"{hidden}, padded) is beyond the kernels' K <= {top} -- a thread keeps the A values of its hidden units in registers"
                                  + ("" if allow_wide_mlp or padded_hidden(hidden) > N.LORA_WIDE_MAX_K else _WIDE_OPT_IN))


def _check_mlp_in_width(name, hidden, gated, allow_wide_mlp=False):
    """A DINOv3 MLP input module is targeted: refuse, by name and before anything touches the device, a checkpoint whose MLP input weight has more rows than the
    gradient kernels take (dinov3_vith16plus: hidden 5120, gated, N1 = 2 x 5120 = 10240 -- which ``allow_wide_mlp`` covers)."""
    if hidden is None:
        return
    n1 = 2 * padded_hidden(hidden) if gated else hidden
    top = N.LORA_WIDE_MAX_N1 if allow_wide_mlp else LORA_MLP_MAX_N1
    if n1 > top:
        raise NotImplementedError(f"LoRA target module {name!r} is not built for this checkpoint: its MLP input weight has N1 = {n1} rows (hidden width {hidden}"
                                  f"{', gate and up fused' if gated else ''}), beyond the gradient kernels' N1 <= {top} -- a thread keeps the B values of "
                                  f"its rows in registers (dinov3_vith16plus is the one such checkpoint)"
                                  + ("" if allow_wide_mlp or n1 > N.LORA_WIDE_MAX_N1 else _WIDE_OPT_IN))


def resolve_lora_targets(target_modules, names, n_layers, hidden=None, allow_wide_mlp=False):
    """``target_modules`` of peft's LoraConfig (models/modules/full_model.py:54,67 hands it over unchanged) -> which of the six modules are targeted, as six
    booleans in table order.  Matching is peft's: a module is targeted when its name equals a target or ends in ``.<target>``; the same modules must be hit in
    every layer; a name that hits a module that is not built (``names.refused``), no module at all, or the other family's module is refused with the reason.
    None = query / key / value, the reference's.  ``hidden``: the checkpoint's MLP hidden width, when known: a SwiGLU MLP output projection beyond the kernels'
    width is refused here, before anything touches the device; ``allow_wide_mlp`` moves those two widths to the wide kernels' (native.LORA_WIDE_MAX_*)."""
    if target_modules is None:
        return (True, True, True, False, False, False)
    if isinstance(target_modules, str):
        raise NotImplementedError(f"target_modules {target_modules!r}: a string is a regular expression to peft; only a list of module names is built")
    targets = list(target_modules)
    if not targets:
        raise ValueError(f"target_modules is empty: name at least one of {names.ask}")
    lay = names.layer_path
    modules = [f"{lay}{i}.{m}" for i in range(n_layers) for m in names.paths + names.more] + [names.patch]
    hit = set()
    for t in targets:
        if not isinstance(t, str) or not t:
            raise ValueError(f"target_modules entry {t!r} is not a module name")
        found = [n for n in modules if n == t or n.endswith("." + t)]
        last = t.rsplit(".", 1)[-1]
        if not found:
            if names.foreign(t, last):
                raise ValueError(names.foreign(t, last))
            raise NotImplementedError(f"LoRA target module {t!r} is not built: {names.refused.get(last, 'no Linear module of the backbone has that name')}")
        for n in found:
            leaf = n.rsplit(".", 1)[-1]
            if leaf in names.refused:
                raise NotImplementedError(f"LoRA target module {t!r} ({n}) is not built: {names.refused[leaf]}")
            hit.add(n)
    per_layer = [{n[len(f"{lay}{i}."):] for n in hit if n.startswith(f"{lay}{i}.")} for i in range(n_layers)]
    if any(pl != per_layer[0] for pl in per_layer):
        raise NotImplementedError(f"target_modules {targets}: the same modules must be targeted in every layer")
    if names.swiglu and names.paths[_MLP_OUT] in per_layer[0]:
        _check_swiglu_out_width(names.paths[_MLP_OUT].rsplit(".", 1)[-1], hidden, allow_wide_mlp)
    for p in names.paths[_MLP_IN:_MLP_IN + 1] + names.paths[_MLP_IN2:]:
        if p in per_layer[0] and p.rsplit(".", 1)[-1] in _MLP_IN3:
            _check_mlp_in_width(p.rsplit(".", 1)[-1], hidden, names.swiglu, allow_wide_mlp)
    return tuple(p in per_layer[0] for p in names.paths)


def _out_leaves(names, hit):
    """the leaf names of the output projections that are hit, as the two public functions return them"""
    return tuple(names.paths[j].rsplit(".", 1)[-1] for j in (_ATTN_OUT, _MLP_OUT) if hit[j])


def lora_targets(target_modules=None, mlp="gelu", n_layers=1, allow_out=False, allow_swiglu_out=False, hidden=None):
    """``resolve_lora_targets`` on DINOv2's names -> ((query, key, value) as booleans, the MLP input projection's name or None).  Built: any subset of query / key /
    value and the MLP input projection (``fc1`` on a GELU checkpoint, ``weights_in`` on a SwiGLU one) -- the modules whose input is a LayerNorm output, which the
    LayerNorm kernel can extend by the LoRA down-projection.
    ``allow_out=True`` also accepts the output projections ``dense`` (attention.output.dense) and, on a GELU checkpoint, ``fc2`` -- row kernels beside their GEMMs
    (include/ucod_dpl.h: ucod_lora_out_fwd) -- and returns a third element: the accepted ones of ("dense", "fc2"), in that order.  ``weights_out`` stays refused.
    ``allow_swiglu_out=True`` (needs ``allow_out``; ValueError without it) accepts ``weights_out`` on a SwiGLU checkpoint as well -- the hidden is recomputed from
    the saved pre-activation (UCOD_LORA_OUT_ACT_SWIGLU) -- and the third element is then drawn from ("dense", "weights_out")."""
    if mlp not in _MLP_IN_LEAF:
        raise ValueError(f"mlp must be 'gelu' or 'swiglu', got {mlp!r}")
    _check_swiglu_out(allow_out, allow_swiglu_out)
    names = _dinov2_names(mlp, allow_out, allow_swiglu_out)
    hit = resolve_lora_targets(target_modules, names, n_layers, hidden)
    mlp_hit = _MLP_IN_LEAF[mlp] if hit[_MLP_IN] else None
    return (hit[:3], mlp_hit, _out_leaves(names, hit)) if allow_out else (hit[:3], mlp_hit)


def lora_targets_dinov3(target_modules=None, gated=False, n_layers=1, layer_path="model.layer.", allow_out=False, allow_swiglu_out=False, hidden=None,
                        allow_mlp_in=False, allow_wide_mlp=False):
    """``resolve_lora_targets`` on a DINOv3 checkpoint's names, ``{layer_path}{i}.attention.{q,k,v,o}_proj`` and ``mlp.{up,down}_proj`` (gated: ``gate_proj`` too):
    any non-empty subset of q_proj / k_proj / v_proj.  Returns the (q, k, v) booleans; without ``allow_mlp_in`` no MLP input module is accepted.
    ``allow_out=True`` also accepts ``o_proj`` and, on a non-gated MLP, ``down_proj`` and returns ((q, k, v), the accepted ones of ("o_proj", "down_proj")); the
    gated MLP's ``down_proj`` stays refused -- unless ``allow_swiglu_out=True`` (needs ``allow_out``) is given as well (dinov3_vith16plus, hidden 5120, is refused).
    ``allow_mlp_in=True`` also accepts ``up_proj`` and, on the gated MLP, ``gate_proj`` (``gate_proj`` on a plain MLP stays refused; with ``hidden`` given,
    dinov3_vith16plus -- N1 = 10240 rows against the kernels' 8192 -- is refused by name) and returns one more element behind the others: the accepted ones of
    ("gate_proj", "up_proj"), in that order.
    ``allow_wide_mlp=True`` accepts no further name: it moves the two width refusals to the wide kernels' limits (native.LORA_WIDE_MAX_N1 / _MAX_K), so that
    dinov3_vith16plus's gate_proj / up_proj / down_proj pass."""
    _check_swiglu_out(allow_out, allow_swiglu_out)
    names = _dinov3_names(gated, layer_path, allow_out, allow_swiglu_out, allow_mlp_in)
    hit = resolve_lora_targets(target_modules, names, n_layers, hidden, allow_wide_mlp)
    if not allow_mlp_in:
        return (hit[:3], _out_leaves(names, hit)) if allow_out else hit[:3]
    mlp_in = tuple(names.paths[j].rsplit(".", 1)[-1] for j in (_MLP_IN, _MLP_IN2) if j < len(hit) and hit[j])
    return (hit[:3], _out_leaves(names, hit), mlp_in) if allow_out else (hit[:3], mlp_in)


def _dinov3_paths(sd):
    """(prefix in front of ``embeddings.``, layer path behind it) of a DINOv3 state dict: ("", "model.layer.") for transformers 5.x, "layer." for 4.56."""
    pref = next(k[:-len("embeddings.patch_embeddings.weight")] for k in sd if k.endswith("embeddings.patch_embeddings.weight"))
    return pref, ("model.layer." if any(k.startswith(pref + "model.layer.") for k in sd) else "layer.")


def _hf_prefix(sd):
    """What stands in front of the layer number in ``sd``'s names: ``encoder.layer.`` behind "", "dinov2." or "vit."; a DINOv3 state dict's own
    ``{model.,}layer.`` behind its prefix."""
    if is_dinov3(sd):
        pref, lay = _dinov3_paths(sd)
        return pref + lay
    for pref in ("", "dinov2.", "vit."):
        if pref + "encoder.layer.0.attention.attention.query.weight" in sd:
            return pref + "encoder.layer."
    raise NotImplementedError("merging takes a HuggingFace DINOv2 state dict (encoder.layer.{i}.attention.attention.{query,key,value}): the names "
                              "target_modules are matched against")


def lora_layout(state_dict, r, target_modules=None, bias="none", allow_out=False, allow_swiglu_out=False, canon=None, allow_mlp_in=False, allow_wide_mlp=False):
    """Host only: (layer path, module table) of a ``ViTLoRAEngine`` over ``state_dict`` -- the family's names, ``resolve_lora_targets`` with all its refusals,
    which modules have a bias in the checkpoint (DINOv3 ``k_proj`` has none), ``lora_modules``.  ``canon``: ``normalize_state_dict(state_dict)`` if at hand.
    ``allow_mlp_in`` (DINOv3 only; a DINOv2 checkpoint's MLP input needs no opt-in) and ``allow_wide_mlp``: ``lora_targets_dinov3``."""
    c = normalize_state_dict(state_dict) if canon is None else canon
    mlp = "swiglu" if c.get("mlp") == "swiglu" else "gelu"
    F0 = c["layers"][0]["fc1_w"].shape[0] // (2 if mlp == "swiglu" else 1)      # the checkpoint's own hidden width (SwiGLU: before padding)
    sw_out = bool(allow_swiglu_out and mlp == "swiglu")           # (on a GELU checkpoint the opt-in changes nothing: weights_out keeps its refusal's text)
    mlp_in3 = bool(allow_mlp_in and c.get("rope"))
    if c.get("rope"):
        family, names = "dinov3", _dinov3_names(mlp == "swiglu", _dinov3_paths(state_dict)[1], allow_out, sw_out, mlp_in3)
    else:
        family, names = "dinov2", _dinov2_names(mlp, allow_out, sw_out)
    hit = resolve_lora_targets(target_modules, names, len(c["layers"]), F0 if sw_out or mlp_in3 else None, allow_wide_mlp)
    if len(hit) > _MLP_IN2 and not (hit[_MLP_IN] or hit[_MLP_IN2]):         # neither of the gated pair: the table of six, as without the opt-in
        hit, names = hit[:_MLP_IN2], names._replace(paths=lora_module_paths(family))
    if bias == "all" and family == "dinov3" and mlp == "swiglu" and len(hit) <= _MLP_IN2:
        # (the table of six describes the gated MLP's input as ONE module ``up_proj`` with the fused bias: gate_proj.bias would have no name in the state dicts)
        raise NotImplementedError("LoRA bias='all' on a gated DINOv3 checkpoint is built with gate_proj or up_proj targeted (allow_mlp_in=True) only: their biases "
                                  "share the engine's one fused weights_in bias, which the module table carries as the pair's")
    if len(hit) > _MLP_IN2 and bias == "lora_only" and hit[_MLP_IN] != hit[_MLP_IN2]:
        raise NotImplementedError("LoRA bias='lora_only' with exactly one of gate_proj / up_proj targeted is not built: the two share the ONE fused bias of the "
                                  "engine's weights_in GEMM, and its gradient (the column sums of the pre-activation's cotangent) is computed over all of its 2F "
                                  "columns; target both, or neither, or use bias='none'")
    try:
        pref = _hf_prefix(state_dict)
    except NotImplementedError:                     # (a layout without HF module names: every Linear of it has a bias)
        pref = None
    has_bias = tuple(pref is None or f"{pref}0.{p}.bias" in state_dict for p in names.paths)
    return names.layer_path, lora_modules(family, mlp, c["patch_w"].shape[0], padded_hidden(F0) if mlp == "swiglu" else F0, F0, r, hit, bias, has_bias)


LORA_BIAS_MODES = ("none", "lora_only", "all")               # peft's LoraConfig.bias (models/modules/full_model.py:53,66)


def check_lora_bias(bias, allow_bias_all=False):
    """peft's ``LoraConfig.bias`` as this package builds it: "none" and "lora_only" pass; "all" passes with the opt-in ``allow_bias_all`` and is refused with its
    reason without it; anything else is a ValueError.  Host only: ``load_lora`` and ``ViTLoRAEngine`` call it before any device work."""
    if bias not in LORA_BIAS_MODES:
        raise ValueError(f"LoRA bias must be one of {LORA_BIAS_MODES} (peft's LoraConfig.bias), got {bias!r}")
    if bias == "all" and not allow_bias_all:
        raise NotImplementedError("LoRA bias='all' is not built: it also trains the LayerNorm and patch-embedding biases, and the LayerNorm backward of the "
                                  "backbone-backward passes produces no gradient of beta (it returns the input's cotangent only); bias='lora_only' -- the biases "
                                  "of the modules that carry an adapter -- is built, and so is 'all' with the opt-in allow_bias_all=True (lora_cfg.allow_bias_all), "
                                  "which takes those gradients from column sums beside the pass (ucod_vit_backward_lora_bias_ex)")
    return bias


class ViTLoRAEngine(ViTEngine):
    """Backbone-backward mode: the frozen ViT with peft-style LoRA on Linear modules of every encoder layer, as
    models/modules/full_model.py:47-72 configures it (r=2, lora_alpha=4, bias='none', target query / key / value; lora_A kaiming_uniform(a=sqrt 5), lora_B zeros).
    ``forward_train`` saves activations, ``backward`` turns the cotangent of the key map into LoRA gradients -- both entirely in the HIP library.  Every pass is ONE
    call of a _lora_out_ex entry point (``ucod_vit_forward_train_lora_out_ex`` / ``ucod_vit_backward_lora_out_ex`` / ``ucod_vit_forward_lora_infer_lora_out_ex``,
    include/ucod_dpl.h) with the MLP kind, ``_out_flags`` and the tables of the targeted modules; an untargeted module's table is NULL, and the pass then enqueues the
    launches it would without it.  LoRA dropout (``lora_dropout``, 0.05 in the reference config) is a counter-based hash mask on the LoRA branch's input in
    ``train()`` mode and off in ``eval()`` (include/ucod_dpl.h: ucod_lora_dropout).

    What can carry an adapter is described ONCE, in ``self.modules``: six ``LoRAModule`` (``lora_modules``) in the fixed order query, key, value, MLP input,
    attention output, MLP output.  Each states its HF path below the layer path, whether it is targeted, its shapes in the engine and in the checkpoint, its place in
    the arena, its bias, its slots in a frozen engine's row and the conversions between HF's order and the engine's; the state dicts, the merges, the adapter folder
    and the passes' tables all walk it.

        module             DINOv2 (``encoder.layer.{i}.``)            DINOv3 (``{model.,}layer.{i}.``)   input   needs
        query, key, value  attention.attention.{query,key,value}      attention.{q,k,v}_proj             D       --
        MLP input          mlp.fc1 | mlp.weights_in (SwiGLU)          mlp.up_proj; gated: mlp.gate_proj  D       r <= 8; DINOv3: allow_mlp_in
                                                                      and mlp.up_proj, a seventh entry
        attention output   attention.output.dense                     attention.o_proj                   D       allow_out, r <= 8
        MLP output         mlp.fc2 | mlp.weights_out (SwiGLU)         mlp.down_proj                      F       allow_out (SwiGLU / gated: + allow_swiglu_out), r <= 8

    DINOv3's gated MLP (vits16plus) has TWO input modules, ``mlp.gate_proj`` and ``mlp.up_proj``, on the engine's one fused, padded, 4-interleaved weights_in.  With
    ``allow_mlp_in`` and one of them targeted the table has seven entries -- gate_proj in the MLP input's place, up_proj behind the six (``_MLP_IN2``) --: each is a
    peft module of its own (own A, own rows of B, own dropout mask, HF's names and shapes outside the arena), both name ONE arena block and the one fused bias
    (``LoRAModule.part`` / ``get_rows`` / ``set_rows``), and the passes run the pair kernels (include/ucod_dpl.h: ucod_lora_mlp_pair_grad, UCOD_LORA_MLP_PAIR).  A
    hidden width whose fused weight has more than 8192 rows (dinov3_vith16plus: 2 x 5120) is refused by name -- unless ``allow_wide_mlp`` is given: the passes then
    carry UCOD_LORA_WIDE (only when a targeted module needs it) and size and run the MLP modules through the _wide row entry points, up to native.LORA_WIDE_MAX_N1 rows.

    ``target_modules`` (``resolve_lora_targets``, peft's suffix rule) picks among them; None = query / key / value.  Parameters live in ONE flat f32 arena
    ``self.lora`` [L, P], gradients in ``self.lora_grad`` with the same layout -- ready for a single flat all-reduce and the fused AdamW kernel.  A layer's row:

        [A_q | B_q | A_k | B_k | A_v | B_v]   always; an untargeted projection's A and B are held at zero -- their gradients are then zero by structure
                                              (t = s dqkv B = 0 gives dA = 0, u = 0 gives dB = 0) and the fused AdamW leaves an exact zero at zero
        [A_m (r x D) | B_m (N1 x r)]          if the MLP input is targeted; N1 = F (GELU) or 2F in the engine's padded, interleaved row order (SwiGLU)
        [A_g | A_u (r x D each) | B_m]        instead, if gate_proj or up_proj of the gated DINOv3 MLP is: row n of B_m is gate_proj's iff n % 8 < 4; an untargeted
                                              one of the two keeps A = 0 and its rows of B = 0 -- its gradients are zero by structure, as for q / k / v
        [A_o (r x D) | B_o (D x r)]           if the attention output is targeted
        [A_2 (r x F) | B_2 (D x r)]           if the MLP output is targeted; SwiGLU: F is the padded hidden width, the padded columns are zeros in the arena and
                                              absent outside it (the state dicts and the adapter folder carry A_2 as HF has it, [r, F0])
        [b_q | b_k | b_v | b_m | b_o | b_2]   bias="lora_only": the bias of every targeted module that has one in the checkpoint (DINOv3 ``k_proj`` has none)

    The output projections run as row kernels beside their GEMMs (include/ucod_dpl.h: ucod_lora_out_fwd / _grad_s / _grad_x); on the SwiGLU MLP the backward
    recomputes the hidden silu(x1) * x2 from the saved interleaved pre-activation (UCOD_LORA_OUT_ACT_SWIGLU; ``_out_flags`` carries UCOD_LORA_OUT_SWIGLU only when the
    module is targeted), and a hidden width beyond 4096 (dinov3_vith16plus: 5120) is refused: the kernels keep a thread's A values in registers -- with
    ``allow_wide_mlp`` the limit is native.LORA_WIDE_MAX_K (the forward runs in blocks of 512 threads).

    ``bias="lora_only"`` (peft's ``LoraConfig.bias``, full_model.py:53,66; with exactly one of gate_proj / up_proj targeted it is refused: the two share the fused
    bias) changes nothing else: forward = base(x) + scaling B(A(drop(x))) with the base layer's own
    bias, which dropout does not touch.  The trained biases start at the checkpoint's values (the MLP input's N1 values in the engine's order, padding zero).  The
    backward writes their gradients -- column sums of cotangents it already holds (include/ucod_dpl.h: ucod_colsum_det, ucod_vit_backward_lora_bias) -- into the same
    slots of the gradient arena; ``repack`` copies the arena's biases into the engine's own bias vectors, which (with ``clone_for_ema``'s) are private copies in that
    mode.  Every last-layer bias but the key's cannot receive a gradient (only the key projection reaches the key map): its arena slot holds zeros, which the fused
    AdamW keeps at an exact zero, and the state dicts, merges and the adapter take the checkpoint's value for it (``_bias_frozen``).  ``lora_state_dict`` /
    ``merged_state_dict`` / ``merge_into`` carry the biases as ``{layer path}{i}.{module}.bias`` in HF order.

    ``bias="all"`` (with ``allow_bias_all=True``; refused without it, ``check_lora_bias``) is peft's rule "every parameter with bias in its name": every module with
    a bias in the checkpoint has its arena slot, targeted or not, and the row ends in [beta1 | beta2 | b_patch] (``lora_norm_offsets``: norm1.bias, norm2.bias and
    the patch embedding's bias, the last live in row 0 only).  The backward runs ucod_vit_backward_lora_bias_ex with the norm table (``_norm_table``); the private
    bias buffer holds the three vectors too, and the patch bias and the LayerNorm beta slots of this engine's rows view it.  The last layer's beta2 is frozen like
    its Linear biases; the final LayerNorm's bias is not in the arena.  The state dicts carry ``{layer path}{i}.norm{1,2}.bias`` and the patch bias under its HF key;
    ``merge_into`` also re-folds every folded QKV / fc1, targeted or not (their folded bias depends on beta).  On a gated DINOv3 checkpoint it needs gate_proj or
    up_proj targeted (``lora_layout``)."""

    def __init__(self, state_dict, heads, r=2, lora_alpha=4, eps=1e-6, device="cuda", gemm_variant=0, generator=None, lora_dropout=0.0,
                 seed=0, resid="auto", allow_swiglu=False, target_modules=None, allow_rope=False, rope_theta=100.0, allow_out=False, allow_swiglu_out=False,
                 bias="none", allow_mlp_in=False, allow_bias_all=False, allow_wide_mlp=False):
        """``allow_swiglu``: accept a checkpoint with the SwiGLU MLP (DINOv2 ViT-g/14, modeling_dinov2.py:300-315).  Its passes run with
        UCOD_MLP_SWIGLU: the training-mode weights_in saves the interleaved pre-activation [M, 2F] and the weights_out dgrad's drain produces its cotangent
        (include/ucod_dpl.h: UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 / UCOD_EPI_SWIGLU_BWD_BF16).  Opt-in: ``load_lora`` (models/modules/full_model.py) switches it on.
        ``allow_rope``: accept a DINOv3 checkpoint (rotary position embedding; ``rope_theta`` as ``ViTEngine``).  Its passes rotate q / k of the patch rows between
        the QKV GEMM and attention and apply the transposed rotation to dq / dk behind attention backward (include/ucod_dpl.h: ucod_rope_qk_ld,
        ucod_vit_train_desc.allow_rope); a gated-MLP checkpoint (vits16plus / vith16plus) also needs ``allow_swiglu``.  Opt-in: ``lora_cfg.allow_rope``.
        ``allow_out``: let ``target_modules`` name the output projections (class docstring).  Opt-in: ``load_lora`` passes its ``lora_cfg.allow_out``.
        ``allow_swiglu_out``: let it name the SwiGLU MLP's output projection too (with ``allow_out`` and ``allow_swiglu``; on DINOv3 also ``allow_rope``).
        ``bias``: peft's ``LoraConfig.bias`` (class docstring): "none", "lora_only" or, with ``allow_bias_all``, "all"; ``load_lora`` passes ``lora_cfg.bias``.
        ``allow_mlp_in``: on a DINOv3 checkpoint, let ``target_modules`` name the MLP input modules -- ``up_proj``, and ``gate_proj`` on the gated MLP (class
        docstring).  On a DINOv2 checkpoint it changes nothing.  Opt-in: ``load_lora`` passes its ``lora_cfg.allow_mlp_in``.
        ``allow_bias_all``: let ``bias`` be "all" (class docstring); with "none" / "lora_only" it changes nothing.  Opt-in: ``lora_cfg.allow_bias_all``.
        ``allow_wide_mlp``: let the MLP modules be as wide as the wide kernels take (class docstring: dinov3_vith16plus); where every targeted module fits the
        narrow kernels it changes nothing.  Opt-in: ``lora_cfg.allow_wide_mlp``."""
        check_lora_bias(bias, allow_bias_all)
        canon = normalize_state_dict(state_dict)
        if allow_swiglu_out and not (allow_out and allow_swiglu and (allow_rope or not canon.get("rope"))):
            raise ValueError("allow_swiglu_out=True needs allow_out=True and allow_swiglu=True" + (", and allow_rope=True on a DINOv3 checkpoint" if canon.get("rope") else ""))
        if canon.get("rope") and not allow_rope:
            raise NotImplementedError("backbone-backward (LoRA) mode takes a DINOv3 checkpoint (rotary position embedding, RoPE: the passes rotate q / k and "
                                      "rotate dq / dk back) only with allow_rope=True")
        self.allow_rope, self.allow_out, self.allow_swiglu_out, self.allow_mlp_in = bool(allow_rope), bool(allow_out), bool(allow_swiglu_out), bool(allow_mlp_in)
        self._base_sd = state_dict                                 # (a reference, not a copy, like backbone._src) the f32 base weights every merge starts from
        self._merge_buf = self._mlp_src_rows = None
        self.allow_wide_mlp = bool(allow_wide_mlp)
        self._adopt(*lora_layout(state_dict, r, target_modules, bias, allow_out, allow_swiglu_out, canon=canon, allow_mlp_in=allow_mlp_in,
                                 allow_wide_mlp=allow_wide_mlp), bias)
        if canon.get("mlp") == "swiglu" and not allow_swiglu:
            raise NotImplementedError("backbone-backward (LoRA) mode takes a checkpoint with the SwiGLU MLP (DINOv2 ViT-g/14, modeling_dinov2.py:300-315) only with "
                                      "allow_swiglu=True (models/modules/full_model.py: load_lora passes it); the frozen-backbone engines (ViTEngine / "
                                      "SplitViTEngine) take it as it is")
        # resid: as ViTEngine ("auto" = the fp16 residual stream with bf16 operands).  Round 4: the training pass SAVES the stream in that
        # type and LayerNorm backward reads it (ucod_layernorm_bwd_ex); resid="f32" keeps the round-3 path.
        super().__init__(state_dict, heads, eps=eps, device=device, full_last_layer=False, gemm_variant=gemm_variant, attn_variant=2, resid=resid,
                         half="bf16", rope_theta=rope_theta)      # (the backbone-backward entry points exist in the bf16 build only: include/ucod_dpl.h, ucod_half_name)
        if not 0.0 <= lora_dropout < 1.0:
            raise ValueError("lora_dropout must be in [0, 1)")
        if 0.0 < lora_dropout < 1.0 / 1024:
            raise ValueError("lora_dropout below 1/1024 would be rounded to no dropout at all (the mask threshold is floor(1024 p): include/ucod_dpl.h, "
                             "ucod_lora_dropout); use 0 or a value >= 1/1024")
        # LoRA dropout (LoraConfig.lora_dropout, full_model.py:50): active while `self.training` is True; the mask of a step is a pure
        # function of (seed, step), regenerated by the backward kernels.  `eval()` / `train()` switch it like nn.Module does.
        self.lora_dropout, self.training = float(lora_dropout), True
        self._seed, self._step, self._step_seed = int(seed), 0, 0
        if r < 1 or 3 * r > N.LORA_AUG:
            raise ValueError(f"LoRA rank {r} unsupported (1 <= r <= {N.LORA_AUG // 3})")
        if N.load().ucod_layernorm_lora_fits(self.D, int(r), 3) != 1:
            raise ValueError(f"LoRA rank {r} at width {self.D}: the 3 r rows of A ({3 * int(r) * self.D * 4} bytes) do not fit one workgroup's LDS "
                             f"(include/ucod_dpl.h, ucod_layernorm_lora)")
        self.r, self.scaling = int(r), float(lora_alpha) / float(r)
        D, L, dev = self.D, self.L, self.device
        mlp_in, outs = self.modules[_MLP_IN], self.modules[_ATTN_OUT:_MLP_IN2]
        if self.mlp_in_live:
            if r > N.LORA_MLP_MAX_R:
                raise ValueError(f"LoRA rank {r} unsupported with the MLP input projection targeted (1 <= r <= {N.LORA_MLP_MAX_R}: its gradient kernel keeps a "
                                 f"lane's B values and accumulators in registers)")
            if self._row_fn("ucod_lora_mlp_pair_grad_workspace_bytes" if self.mlp_pair else "ucod_lora_mlp_grad_workspace_bytes")(self.N1, D) == 0:
                raise ValueError(f"the MLP input projection's LoRA kernels cover D <= 1536 and {self.N1} <= {N.LORA_WIDE_MAX_N1 if self._wide else 8192} rows of "
                                 f"{mlp_in.leaf}")
        for m in outs:
            if not m.targeted:
                continue
            if r > N.LORA_MLP_MAX_R:
                raise ValueError(f"LoRA rank {r} unsupported with an output projection targeted (1 <= r <= {N.LORA_MLP_MAX_R}: its kernels keep u and t {N.LORA_OUT_W} wide)")
            if self._row_fn("ucod_lora_out_grad_workspace_bytes")(r, m.k, D) == 0:
                top = N.LORA_WIDE_MAX_K if self._wide else 4096
                if m is outs[1] and self._out_flags:
                    raise NotImplementedError(f"LoRA on the SwiGLU MLP's output projection is not built for this hidden width: K = {m.k} is beyond the kernels' "
                                              f"K <= {top} (a thread keeps the A values of its hidden units in registers); D = {D} must be <= 1536")
                raise ValueError(f"the output projections' LoRA kernels cover D <= 1536 and an input width <= {top} (a multiple of 128), got D = {D}, width {m.k}")
        if self.bias_numel:
            self._setup_bias()
        self.lora = torch.zeros(L, self.numel, dtype=torch.float32, device=dev)
        # A: kaiming_uniform_(a=sqrt(5)) on [r, fan_in] = U(-1/sqrt(fan_in), 1/sqrt(fan_in)), B zeros.  q / k / v are drawn as one tensor whether targeted or not (an
        # untargeted projection keeps A = B = 0), then the MLP input, then the output modules, then the gated DINOv3 pair (gate_proj, up_proj; an untargeted one of
        # the two keeps A = 0 and its rows of B = 0): an engine without the later ones keeps its stream.
        bound = 1.0 / math.sqrt(D)
        a = (torch.rand(L, 3, r * D, generator=generator) * 2 - 1) * bound
        for p, m in enumerate(self.modules[:_MLP_IN]):
            if m.targeted:
                self.lora[:, m.a] = a[:, p].to(dev)
        if mlp_in.targeted and not self.mlp_pair:
            self.lora[:, mlp_in.a] = ((torch.rand(L, r * D, generator=generator) * 2 - 1) * bound).to(dev)
        for m in outs:
            if m.targeted:                              # (SwiGLU, padded: fan_in is the checkpoint's own width F0, the padded columns stay zero)
                a = (torch.rand(L, r, m.k_hf, generator=generator) * 2 - 1) / math.sqrt(m.k_hf)
                self.lora[:, m.a] = m.a_from_hf(a).reshape(L, r * m.k).to(dev)
        if self.mlp_pair:
            for m in (mlp_in, self.modules[_MLP_IN2]):
                if m.targeted:
                    self.lora[:, m.a] = ((torch.rand(L, r * D, generator=generator) * 2 - 1) * bound).to(dev)
        self._bias_init_arena()
        self.lora_grad = torch.zeros_like(self.lora)
        A = N.LORA_AUG
        self.train_layers = []                          # rows of the training table without its two LoRA slots (native.VIT_TRAIN_SLOTS)
        for l in self.layers:
            w_aug = torch.zeros(3 * D, D + A, dtype=torch.bfloat16, device=dev)
            w_aug[:, :D] = l[N.QKV_W]
            wt_aug = torch.zeros(D, 3 * D + A, dtype=torch.bfloat16, device=dev)
            wt_aug[:, :3 * D] = l[N.QKV_W].t()
            # (SwiGLU: fc1_w is the padded, interleaved weights_in [2F, D] -- its transpose's K order is the column order of the pre-activation's cotangent)
            self.train_layers.append([w_aug, wt_aug] + [l[w].t().contiguous() for w in (N.PROJ_W, N.FC1_W, N.FC2_W)])
        self.mlp_layers = []                            # native.VIT_TRAIN_MLP_SLOTS without the two LoRA slots: the augmented fc1 / weights_in weight
        if self.mlp_in_live:
            for l in self.layers:
                w_aug = torch.zeros(self.N1, D + A, dtype=torch.bfloat16, device=dev)
                w_aug[:, :D] = l[N.FC1_W]
                self.mlp_layers.append([w_aug])
        self.train_streams = 2                          # image-parallel sub-batches of the training passes (_chunks)
        self._tside = None
        self._saved_for = None
        self.repack()

    # ---- the module table and what is read from it -----------------------------------------------------------------------
    def _adopt(self, layer_path, modules, bias="none"):
        """Take a module table (``lora_layout``; host only).  Whatever the engine knows of its modules it reads from ``self.modules``; the attributes below are plain
        values derived from it here, once, for the passes and for callers that read them."""
        mods = self.modules = tuple(modules)
        self._layer_path, self.bias, self._bias_flat = layer_path, bias, None
        self.numel, self.norm_off = lora_row_numel(mods, bias), lora_norm_offsets(mods, bias)
        self.targets = tuple(m.targeted for m in mods[:_MLP_IN])                 # (query, key, value)
        self.mlp_pair = len(mods) > _MLP_IN2                                     # the gated DINOv3 MLP's gate_proj / up_proj: one arena block, the _pair kernels
        mlp_ins = [m for m in (mods[_MLP_IN],) + mods[_MLP_IN2:] if m.targeted]
        self.mlp_in_live = bool(mlp_ins)                                         # the passes carry the MLP table
        self.mlp_target = mlp_ins[0].leaf if mlp_ins else None                   # (the pair: the first targeted of gate_proj, up_proj; ``modules`` names both)
        self.out_targets = tuple(m.targeted for m in mods[_ATTN_OUT:_MLP_IN2])   # (attention output projection, MLP output projection)
        self.qkv_numel = mods[_V].b.stop
        self.out_off = [m.a.start if m.targeted else None for m in mods[_ATTN_OUT:_MLP_IN2]]
        self.bias_off = tuple(m.bias_off for m in mods[:_MLP_IN2])               # (the bias table's six slots; the pair's fused bias is the MLP input's)
        self.bias_numel = sum(m.nb for m in mods if m.bias_off is not None and m.part != 1) + (3 * mods[_Q].k if self.norm_off else 0)
        if self.mlp_pair and mods[_MLP_IN].bias_off != mods[_MLP_IN2].bias_off:
            raise ValueError("the fused bias of gate_proj / up_proj is trained for both or for neither (lora_layout refuses the rest)")
        self.N1, self._F0 = mods[_MLP_IN].nb, mods[_MLP_OUT].k_hf                 # rows of the MLP input weight in the engine; the checkpoint's own hidden width
        # (the flags word of the passes: a bit for the SwiGLU MLP's output projection and one for the gated pair, each set only with its module targeted)
        swiglu = mods[_MLP_IN].interleaved or self.mlp_pair                      # (the MLP input's rows are interleaved: whole, or as the pair's two halves)
        self._out_flags = (N.LORA_OUT_SWIGLU if mods[_MLP_OUT].targeted and swiglu else 0) | (N.LORA_MLP_PAIR if self.mlp_pair else 0)
        # (... and one for the wide row kernels, set only when ``allow_wide_mlp`` is given AND a targeted MLP module is beyond the narrow ones)
        self._wide = bool(getattr(self, "allow_wide_mlp", False) and ((self.mlp_in_live and self.N1 > LORA_MLP_MAX_N1)
                                                                      or (mods[_MLP_OUT].targeted and mods[_MLP_OUT].k > LORA_OUT_MAX_K)))
        self._out_flags |= N.LORA_WIDE if self._wide else 0

    def _row_fn(self, name):
        """A row entry point that has a _wide form: that form when the passes carry UCOD_LORA_WIDE, else the narrow one."""
        return getattr(self.lib, name + "_wide" if self._wide else name)

    def _slices(self, j):
        """(A, B) of module ``j`` in one layer's arena row."""
        return self.modules[j].a, self.modules[j].b

    def _mlp_slices(self):
        return self._slices(_MLP_IN)

    def _out_slices(self, m):
        """... of output module ``m`` (0 = attention output projection, 1 = MLP output projection)"""
        return self._slices(_ATTN_OUT + m)

    def _targeted(self):
        """(path below ``{layer path}{i}.``, table entry) of every targeted module"""
        return [(m.path, m) for m in self.modules if m.targeted]

    # ---- trained biases (bias="lora_only") ----------------------------------------------------------------------------
    def _setup_bias(self):
        """This engine's bias vectors move into one private buffer ``_bias_flat`` [L, 3D + N1 + D + D] (q | k | v | m | o | 2: ``LoRAModule.bias_cols``) that the rows
        of ``self.layers`` view -- so that ``repack`` is one strided copy per module and no tensor is shared with the checkpoint or a clone."""
        slots = dict.fromkeys(m.b_slot for m in self.modules)
        # (bias="all": behind them beta1 | beta2 | the patch bias -- the same patch vector in every row; row 0's is the one the passes read)
        norm = (lambda row: [row[N.LN1_B], row[N.LN2_B], self.patch_b]) if self.norm_off else (lambda row: [])
        self._bias_flat = torch.stack([torch.cat([row[s] for s in slots] + norm(row)) for row in self.layers])
        if self.norm_off:
            base = self._base_sd
            self._patch_key = next((k for k in ("embeddings.patch_embeddings.projection.bias", "embeddings.patch_embeddings.bias") if k in base), None)
            if self._patch_key is None:
                raise NotImplementedError("LoRA bias='all' needs HF's names (the patch embedding's bias is carried under its HF key)")
        self._link_bias()

    def _link_bias(self):
        """Point the bias slots of ``self.layers`` (a private list of rows) at ``_bias_flat``."""
        rows = []
        for row, f in zip(self.layers, self._bias_flat):
            row = list(row)
            for s in dict.fromkeys(m.b_slot for m in self.modules):
                cols = [m.bias_cols for m in self.modules if m.b_slot == s]
                row[s] = f[cols[0].start:cols[-1].stop]
            if self.norm_off:
                c0 = self._norm_cols()
                row[N.LN1_B], row[N.LN2_B] = f[c0:c0 + self.D], f[c0 + self.D:c0 + 2 * self.D]
            rows.append(row)
        self.layers = rows
        if self.norm_off:
            c0 = self._norm_cols()
            self.patch_b = self._bias_flat[0, c0 + 2 * self.D:c0 + 3 * self.D]

    def _norm_cols(self):
        """first column of [beta1 | beta2 | b_patch] in ``_bias_flat``: behind the Linear biases"""
        return max(m.bias_cols.stop for m in self.modules)

    def _norm_live(self):
        """bias="all": (arena columns, ``_bias_flat`` columns, the rows that are live) of beta1 (every layer: the last one's reaches the key map through the key
        projection), beta2 (below the last layer) and the patch bias (row 0)"""
        if not self.norm_off:
            return []
        D, c0 = self.D, self._norm_cols()
        return [(slice(o, o + D), slice(c0 + k * D, c0 + (k + 1) * D), Lj) for k, (o, Lj) in enumerate(zip(self.norm_off, (self.L, self.L - 1, 1)))]

    def _norm_names(self, prefix=None):
        """[(name, row, which of the three)]: ``{layer path}{i}.norm{1,2}.bias`` of every layer and the patch bias under its HF key (in front of it whatever
        ``prefix`` has in front of the layer path)"""
        if not self.norm_off:
            return []
        prefix = self._layer_path if prefix is None else prefix
        root = prefix[:len(prefix) - len(self._layer_path)] if prefix.endswith(self._layer_path) else ""
        return [(root + self._patch_key, 0, 2)] + [(f"{prefix}{i}.norm{k + 1}.bias", i, k) for i in range(self.L) for k in (0, 1)]

    def _norm_value(self, i, k, src=None):
        """beta1 / beta2 of layer ``i`` or the patch bias (``k`` = 0 / 1 / 2): from the arena (``src``), or the engine's own copy for a frozen slot"""
        o, cols, Lj = self._norm_live()[k]
        return self._bias_flat[i, cols] if i >= Lj else (self.lora if src is None else src)[i, o]

    def _bias_frozen(self, i, j):
        """True for a bias slot that cannot receive a gradient: every bias of the last layer but the key's (only the key projection reaches the key map).  torch's
        AdamW skips such a parameter (its grad is None); the flat arena would decay it by lr * wd per step, so its arena slot holds zeros -- an exact zero stays at
        zero -- and every reader takes the engine's own copy, which holds the checkpoint's value."""
        return i == self.L - 1 and j != _K

    def _bias_live(self):
        """(its columns in ``_bias_flat``, its arena columns, the layers below the frozen ones) of every trained bias (bias="all": and of the three norm vectors)"""
        return [(m.bias_cols, slice(m.bias_off, m.bias_off + m.nb), self.L if j == _K else self.L - 1) for j, m in enumerate(self.modules)
                if m.bias_off is not None and m.part != 1] \
            + [(cols, o, Lj) for o, cols, Lj in self._norm_live()]        # (the pair's fused bias once, at gate_proj's entry)

    def _bias_init_arena(self):
        """Trained biases start at the checkpoint's values; a slot that cannot receive a gradient (``_bias_frozen``) stays zero."""
        for cols, o, Lj in self._bias_live():
            self.lora[:Lj, o] = self._bias_flat[:Lj, cols]
            self.lora[Lj:, o] = 0.0

    def _repack_bias(self):
        """arena -> the engine's own bias vectors, one strided copy per trained module (frozen slots keep the checkpoint's value: ``_bias_frozen``)"""
        for cols, o, Lj in self._bias_live():
            self._bias_flat[:Lj, cols].copy_(self.lora[:Lj, o])

    def _bias_value(self, i, j, src=None):
        """The bias of module ``j`` in layer ``i`` as the engine orders it (gate_proj / up_proj: the fused bias, ``LoRAModule.nb`` values): from the arena (``src``, default ``self.lora``), or the checkpoint's for a frozen slot."""
        m = self.modules[j]
        if self._bias_frozen(i, j):
            return self._bias_flat[i, m.bias_cols]
        return (self.lora if src is None else src)[i, m.bias_off:m.bias_off + m.nb]

    def _bias_table(self, grad):
        """The bias table of the backward (native.VIT_TRAIN_BIAS_SLOTS: gradient destinations in ``grad`` [L, P]; NULL = not trained), or None without one."""
        if not self.bias_numel:
            return None
        ptrs = []
        for i in range(self.L):
            ptrs += [None if o is None else grad[i, o:].data_ptr() for o in self.bias_off]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def _norm_table(self, grad):
        """The norm table of the backward (include/ucod_dpl.h: ucod_vit_backward_lora_bias_ex -- [0] the patch bias, [1 + 2 l] beta1, [2 + 2 l] beta2 of layer l:
        gradient destinations in ``grad`` [L, P]), or None unless bias="all"."""
        if not self.norm_off:
            return None
        b1, b2, bp = self.norm_off
        ptrs = [grad[0, bp:].data_ptr()]
        for i in range(self.L):
            ptrs += [grad[i, b1:].data_ptr(), grad[i, b2:].data_ptr()]
        return (C.c_void_p * len(ptrs))(*ptrs)

    # ---- state dicts ------------------------------------------------------------------------------------------------------
    def lora_state_dict(self, grads=False, prefix=None):
        """peft-style names of the targeted modules, ``{layer path}{i}.{module path}.lora_{A,B}.weight`` in table order (class docstring), in HF's shapes: B of a SwiGLU
        ``weights_in`` [2 hidden, r] in HF row order, unpadded; A of a SwiGLU ``weights_out`` [r, hidden] without the padded columns.  Behind a layer's matrices, the
        trained biases (bias="lora_only") as ``{module path}.bias``: a frozen slot reads as the checkpoint's value, its gradient as zero.  ``prefix`` replaces the
        layer path."""
        prefix = self._layer_path if prefix is None else prefix
        src = self.lora_grad if grads else self.lora
        out = {}
        for i in range(self.L):
            for path, m in self._targeted():
                out[f"{prefix}{i}.{path}.lora_A.weight"] = m.a_to_hf(src[i, m.a].reshape(self.r, m.k)).clone()
                out[f"{prefix}{i}.{path}.lora_B.weight"] = m.get_rows(src[i, m.b].reshape(m.nb, self.r)).clone()
            for j, m in enumerate(self.modules):
                if m.bias_off is not None:
                    v = torch.zeros(m.nb, device=self.device) if grads and self._bias_frozen(i, j) else self._bias_value(i, j, src)
                    out[f"{prefix}{i}.{m.path}.bias"] = m.get_rows(v.reshape(-1, 1)).reshape(-1).clone()
        for name, i, k in self._norm_names(prefix):               # bias="all": the LayerNorm betas and the patch bias (a frozen slot: the checkpoint's value, gradient zero)
            frozen = i >= self._norm_live()[k][2]
            out[name] = torch.zeros(self.D, device=self.device) if grads and frozen else self._norm_value(i, k, src).clone()
        return out

    def load_lora_state_dict(self, sd, prefix=None):
        """The inverse of ``lora_state_dict``.  A LoRA key of a module this engine does not target is refused (its matrices are held at zero), and so is a tensor
        that does not have HF's shape (a padded or transposed one would load without a sound)."""
        prefix = self._layer_path if prefix is None else prefix
        mods = self._targeted()
        want = {f"{prefix}{i}.{path}.lora_{ab}.weight" for i in range(self.L) for path, _ in mods for ab in "AB"}
        extra = sorted(k for k in sd if ".lora_" in k and k.startswith(prefix) and k not in want)
        if extra:
            raise KeyError(f"LoRA matrices of modules this engine does not target ({', '.join(m.leaf for _, m in mods)} are): {extra[:4]}"
                           + (" ..." if len(extra) > 4 else ""))
        take = lambda k: sd[k].to(self.device, torch.float32)  # noqa: E731
        for i in range(self.L):
            for path, m in mods:
                base = f"{prefix}{i}.{path}"
                a, b = take(base + ".lora_A.weight"), take(base + ".lora_B.weight")
                if m is self.modules[_MLP_IN] and tuple(b.shape) != (m.n_hf, self.r):       # (the text this refusal has always had)
                    raise ValueError(f"{base}.lora_B.weight has shape {tuple(b.shape)}")
                if tuple(a.shape) != (self.r, m.k_hf) or tuple(b.shape) != (m.n_hf, self.r):
                    raise ValueError(f"{base}: lora_A has shape {tuple(a.shape)}, lora_B {tuple(b.shape)}")
                self.lora[i, m.a] = m.a_from_hf(a).reshape(-1)
                m.set_rows(self.lora[i, m.b].view(m.nb, self.r), b)              # (padded units load as zeros)
            for j, m in enumerate(self.modules):
                if m.bias_off is not None:
                    name = f"{prefix}{i}.{m.path}.bias"
                    v = take(name)
                    if tuple(v.shape) != (m.n_hf,):
                        raise ValueError(f"{name} has shape {tuple(v.shape)}, expected {(m.n_hf,)}")
                    m.set_rows(self._bias_value(i, j).view(-1, 1), v.reshape(-1, 1))                 # (a frozen slot: into the engine's own copy; its arena slot stays zero)
        for name, i, k in self._norm_names(prefix):
            v = take(name)
            if tuple(v.shape) != (self.D,):
                raise ValueError(f"{name} has shape {tuple(v.shape)}, expected {(self.D,)}")
            self._norm_value(i, k).copy_(v)
        self.repack()

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def _drop_p(self):
        return self.lora_dropout if self.training else 0.0

    def repack(self):
        """Refresh the LoRA columns of the augmented weights (call after every parameter update).  With dropout active the A^T
        columns of the dgrad weight are zero: the masked t A term is added by the LayerNorm-1 backward instead."""
        zero_a = int(self._drop_p() > 0.0)
        for i, tl in enumerate(self.train_layers):
            N.check(self.lib.ucod_lora_pack(N.ptr(self.lora[i]), self.r, self.scaling, N.ptr(tl[N.T_QKV_W_AUG]), N.ptr(tl[N.T_QKV_WT_AUG]), self.D, zero_a, N.stream()),
                    "ucod_lora_pack")
        for i, ml in enumerate(self.mlp_layers):               # the MLP module's B columns of fc1_w_aug (its A term is always added by the LayerNorm-2 backward)
            name = "ucod_lora_mlp_pair_pack" if self.mlp_pair else "ucod_lora_mlp_pack"      # (the pair: each row's B values in its own module's columns)
            N.check(self._row_fn(name)(self.lora[i, self.qkv_numel:].data_ptr(), self.r, self.scaling, N.ptr(ml[N.M_FC1_W_AUG]), self.N1, self.D, N.stream()), name)
        self._repack_bias()
        self._packed_zero_a = zero_a

    # ---- passes -----------------------------------------------------------------------------------------------------
    def _train_desc(self, B, H, W, seed):
        t = N.VitTrainDesc()
        t.vit = self._desc(B, H, W)
        t.lora_r, t.lora_scaling = self.r, self.scaling
        t.lora_dropout, t.seed = self._drop_p(), seed
        t.allow_rope = int(self.allow_rope)                        # (with a NULL table -- every checkpoint but DINOv3 -- the drivers never look at it)
        return t

    def _tables(self, gh, gw, grad):
        """(table of the plain rows, training table with ``grad`` [L, P] in its gradient slots, the MLP module's table or None, tensors kept alive)"""
        T, keep = self._table(gh, gw)
        tptrs, mptrs = [], []
        for i, tl in enumerate(self.train_layers):
            tptrs += tl + [self.lora[i], grad[i]]
        for i, ml in enumerate(self.mlp_layers):
            mptrs += ml + [self.lora[i, self.qkv_numel:], grad[i, self.qkv_numel:]]
        TM = (C.c_void_p * len(mptrs))(*[t.data_ptr() for t in mptrs]) if mptrs else None
        return T, (C.c_void_p * len(tptrs))(*[t.data_ptr() for t in tptrs]), TM, keep + tptrs + mptrs

    def _out_table(self, grad):
        """The output modules' table (native.VIT_TRAIN_OUT_SLOTS; an untargeted module's two slots are NULL) with ``grad`` [L, P] in its gradient slots, or None when
        neither is targeted -- the passes then enqueue the launches they always did."""
        if not any(self.out_targets):
            return None
        ptrs = []
        for i in range(self.L):
            for o in self.out_off:
                ptrs += [None, None] if o is None else [self.lora[i, o:].data_ptr(), grad[i, o:].data_ptr()]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def _pass_args(self, t, gh, gw, i):
        """What the three passes of chunk ``i`` hand the _lora_out_ex entry points: the leading arguments (descriptor, MLP kind, flags), the tables (T, TT, TM, TO)
        with the chunk's gradient buffer in their gradient slots -- TM / TO None when the module is not targeted; the size functions take these two alone -- and the
        tensors kept alive."""
        T, TT, TM, keep = self._tables(gh, gw, self._tside_grad[i])
        return (C.byref(t), self.mlp, self._out_flags), (T, TT, TM, self._out_table(self._tside_grad[i])), keep

    def _train_bytes(self, lead, tabs, i):
        """Workspace of chunk ``i``'s training pass and backward: with trained biases the _lora_bias size (the column sums' partials behind everything else)."""
        TB, TN = self._bias_table(self._tside_grad[i]), self._norm_table(self._tside_grad[i])
        if TN is not None:
            return self.lib.ucod_vit_train_workspace_bytes_lora_bias_ex(*lead, *tabs[2:], TB, TN)
        if TB is None:
            return self.lib.ucod_vit_train_workspace_bytes_lora_out_ex(*lead, *tabs[2:])
        return self.lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, *tabs[2:], TB)

    def _chunks(self, B):
        """Image-parallel sub-batches (``self.train_streams``, default 2): as in ViTEngine.forward, every kernel of both passes is
        per image except the LoRA-gradient reduction over rows, which is done per chunk into its own buffer and summed at the end."""
        ns = max(1, min(int(self.train_streams), B))
        if self._tside is None or len(self._tside) != ns:
            self._tside = [torch.cuda.Stream(device=self.device) for _ in range(ns)]
            self._tside_ws, self._iside_ws = [None] * ns, [None] * ns          # workspaces of forward_train (+ backward) / forward_nograd
            self._tside_grad = [torch.zeros_like(self.lora) for _ in range(ns)]
            self._chunk_seed = [0] * ns
        return _chunk_bounds(B, ns)

    def _begin_step(self, B):
        """What every pass starts with: its chunks, the next step's dropout seed, and the augmented weights in the form the current mode needs."""
        self._bounds = self._chunks(B)
        self._step += 1
        self._step_seed = (self._seed * 0x9E3779B97F4A7C15 + self._step) & _MASK64      # fresh masks every step
        if int(self._drop_p() > 0.0) != self._packed_zero_a:
            self.repack()                                           # train()/eval() changed which side carries the A term

    def _seed_of_chunk(self, i, b0):
        """(chunks index rows from 0: decorrelate them)"""
        return (self._step_seed + 0x51ED270B * (i + 1) * int(b0 > 0)) & _MASK64

    def forward_train(self, img, out=None):
        img, key, H, W = self._inputs("ViTLoRAEngine", img, out)
        gh, gw = H // self.P, W // self.P
        self.check_overflow()                                      # (non-blocking) training passes on the fp16 stream that have finished since the last call
        self._begin_step(img.shape[0])

        def run(i, b0, b1):
            t = self._train_desc(b1 - b0, H, W, self._seed_of_chunk(i, b0))
            self._chunk_seed[i] = t.seed
            lead, tabs, keep = self._pass_args(t, gh, gw, i)
            ws = self._tside_ws[i] = self._workspace(self._tside_ws[i], self._train_bytes(lead, tabs, i))
            with self._guard.bind():
                N.check(self.lib.ucod_vit_forward_train_lora_out_ex(*lead, *tabs, N.ptr(img[b0:b1]), N.ptr(key[b0:b1]), N.ptr(ws), ws.numel(), N.stream()),
                        "ucod_vit_forward_train_lora_out_ex")
            if self.resid16:
                self._guard.arm(torch.cuda.current_stream(self.device))

        self._fan_out(self._tside, self._bounds, run, (img, key))
        self._saved_for = (img.shape[0], H, W)
        return key

    def forward_nograd(self, img, out=None, resid16=True):
        """The pass of a LoRA backbone that needs no backward -- the EMA teacher (models/modules/full_model.py:84,108-111: backbone_ema under
        torch.no_grad()): same arithmetic as ``forward_train`` (LoRA aug columns, dropout masks of this engine's own seed stream when in
        train mode) with nothing saved, an inference-sized workspace and, by default, the fp16 residual stream of the frozen-backbone pass
        (bf16 operands: the stream's rounding is 8x finer than theirs).  Image-parallel chunks on the training side streams."""
        img, key, H, W = self._inputs("ViTLoRAEngine", img, out)
        gh, gw = H // self.P, W // self.P
        self._begin_step(img.shape[0])
        self.check_overflow()                                      # (non-blocking) teacher passes that have finished since the last call

        def run(i, b0, b1):
            t = self._train_desc(b1 - b0, H, W, self._seed_of_chunk(i, b0))
            t.vit.resid16 = int(bool(resid16))
            lead, tabs, keep = self._pass_args(t, gh, gw, i)
            ws = self._iside_ws[i] = self._workspace(self._iside_ws[i], self.lib.ucod_vit_lora_infer_workspace_bytes_lora_out_ex(*lead, *tabs[2:]))
            with self._guard.bind():
                N.check(self.lib.ucod_vit_forward_lora_infer_lora_out_ex(*lead, *tabs, N.ptr(img[b0:b1]), N.ptr(key[b0:b1]), N.ptr(ws), ws.numel(), N.stream()),
                        "ucod_vit_forward_lora_infer_lora_out_ex")
            # this engine's own stream type may be f32 (its backward reads it), but THIS pass may run the fp16 one: its saturation counter is
            # fetched behind every chunk and polled by the next call / check_overflow(wait=True) at the loop's boundaries
            if resid16:
                self._guard.arm(torch.cuda.current_stream(self.device))

        self._fan_out(self._tside, self._bounds, run, (img, key))
        return key

    def backward(self, dkey):
        """dkey [B, D, H/P, W/P] -> self.lora_grad (overwritten), returned as the flat [L, P] tensor (P = 6*r*D, plus r*(D + N1) with the MLP module, plus r*2D and
        r*(F + D) with the output modules)."""
        if self._saved_for is None:
            raise RuntimeError("backward() without a preceding forward_train()")
        B, H, W = self._saved_for
        gh, gw = H // self.P, W // self.P
        dkey = dkey.to(torch.float32).contiguous()
        if tuple(dkey.shape) != (B, self.D, gh, gw):
            raise ValueError(f"dkey shape {tuple(dkey.shape)} != {(B, self.D, gh, gw)}")

        def run(i, b0, b1):
            t = self._train_desc(b1 - b0, H, W, self._chunk_seed[i])
            lead, tabs, keep = self._pass_args(t, gh, gw, i)
            ws = self._tside_ws[i]
            TB, TN = self._bias_table(self._tside_grad[i]), self._norm_table(self._tside_grad[i])
            if TN is not None:                                     # bias="all": the same pass plus the sums of the LayerNorm betas and of the patch bias
                N.check(self.lib.ucod_vit_backward_lora_bias_ex(*lead, *tabs, TB, TN, N.ptr(dkey[b0:b1]), N.ptr(ws), ws.numel(), N.stream()),
                        "ucod_vit_backward_lora_bias_ex")
                return
            if TB is not None:                                     # trained biases: the same pass plus one column sum per bias, written into the chunk's arena copy
                N.check(self.lib.ucod_vit_backward_lora_bias(*lead, *tabs, TB, N.ptr(dkey[b0:b1]), N.ptr(ws), ws.numel(), N.stream()), "ucod_vit_backward_lora_bias")
                return
            N.check(self.lib.ucod_vit_backward_lora_out_ex(*lead, *tabs, N.ptr(dkey[b0:b1]), N.ptr(ws), ws.numel(), N.stream()), "ucod_vit_backward_lora_out_ex")

        self._fan_out(self._tside, self._bounds, run, (dkey,))
        if len(self._bounds) > 1:
            torch.sum(torch.stack(self._tside_grad[:len(self._bounds)]), dim=0, out=self.lora_grad)
        else:
            self.lora_grad.copy_(self._tside_grad[0])
        self._saved_for = None
        return self.lora_grad

    # ---- merging: the way out of LoRA mode ---------------------------------------------------------------------------
    _hf_prefix = staticmethod(_hf_prefix)

    def _stage(self, numel):
        """The reusable f32 staging buffer, at least ``numel`` elements."""
        if self._merge_buf is None or self._merge_buf.numel() < numel:
            self._merge_buf = torch.empty(numel, dtype=torch.float32, device=self.device)
        return self._merge_buf

    def _stage_weight(self, key, w, m, engine_rows):
        """Stage the f32 base weight ``w`` [n_hf, k_hf] of module ``m`` at the engine's width k (zero columns for the padded hidden units: the merge kernel wants
        K % 64 == 0, A's padded columns are zeros, the first k_hf columns are the HF weight) and, with ``engine_rows``, in the engine's row order.  Returns
        (the staged weight, the buffer of its shape that the merge writes)."""
        if tuple(w.shape) != (m.n_hf, m.k_hf):
            raise ValueError(f"{key} has shape {tuple(w.shape)}, expected {(m.n_hf, m.k_hf)}")
        gather = engine_rows and m.interleaved                     # SwiGLU weights_in: HF rows (+ one zero row for the padding), gathered into the engine's order
        n, k, lead = (m.n if engine_rows else m.n_hf), m.k, ((m.n_hf + 1) * m.k if gather else 0)
        buf = self._stage(lead + 2 * n * k)
        w0, merged = buf[lead:lead + n * k].view(n, k), buf[lead + n * k:lead + 2 * n * k].view(n, k)
        if gather:
            hf = buf[:lead].view(m.n_hf + 1, k)
            hf[:m.n_hf].copy_(w.detach())
            hf[m.n_hf].zero_()
            torch.index_select(hf, 0, self._engine_row_source(), out=w0)
        else:
            if m.k_hf != k:
                w0.zero_()
            w0[:, :m.k_hf].copy_(w.detach())
        return w0, merged

    def _merge(self, lib, w0, A, B, out, r=None):
        n, k = w0.shape
        N.check(lib.ucod_lora_merge_f32(N.ptr(w0), A.data_ptr(), N.ptr(B), self.r if r is None else r, self.scaling, N.ptr(out), n, k, N.stream()),
                "ucod_lora_merge_f32")

    def _engine_units(self, i, base, pref):
        """What ``merge_into`` merges in layer ``i``, one unit per weight block of the ENGINE: (key, base weight in HF's shape, the module that describes the block,
        A [R, k], B [n, R] in the engine's row order, R).  A targeted module is a unit of its own -- but gate_proj / up_proj of the gated MLP are ONE: the fused
        weights_in [2 F0, D] = cat(gate, up) with the rank-2r module  A = [A_g | A_u],  B = blockdiag(B_g, B_u) spread over the interleaved rows (an untargeted
        one of the two contributes zeros), so that the cast and the LayerNorm fold run over the engine's contiguous rows as for DINOv2's weights_in."""
        out, fused = [], None
        # (bias="all": an untargeted module behind a LayerNorm is a unit too, with A = B = 0 -- its folded bias q (W beta + b) depends on the trained beta)
        units = [(m.path, m) for m in self.modules if m.targeted or (self.norm_off and m.ln is not None)]
        for path, m in units:
            if m.part is None:
                key = f"{pref}{i}.{path}.weight"
                if m.a is None:                                    # (an untargeted MLP input: no place in the arena)
                    A, B = (torch.zeros(self.r * x, dtype=torch.float32, device=self.device) for x in (m.k, m.nb))
                else:
                    A, B = self.lora[i, m.a], self.lora[i, m.b]
                out.append((key, base[key], m, A, B, self.r))
            elif fused is None:
                g, up = self.modules[_MLP_IN], self.modules[_MLP_IN2]
                keys = [f"{pref}{i}.{x.path}.weight" for x in (g, up)]
                fused = g._replace(path="mlp.gate_proj+up_proj", n=g.nb, n_hf=2 * g.n_hf, interleaved=True, part=None)
                r, bm = self.r, self.lora[i, g.b].view(g.nb // 8, 2, 4, self.r)
                B = torch.zeros(g.nb // 8, 2, 4, 2 * r, dtype=torch.float32, device=self.device)
                B[:, 0, :, :r], B[:, 1, :, r:] = bm[:, 0], bm[:, 1]
                out.append((" + ".join(keys), torch.cat([base[k].detach() for k in keys], 0), fused, self.lora[i, g.a.start:up.a.stop], B.view(g.nb, 2 * r), 2 * r))
        return out

    def merged_state_dict(self, base_state_dict=None):
        """peft's ``merge_and_unload()`` as a state dict: a copy of the HF-named base state dict (default: the one this engine was built from) in which ``weight``
        of every targeted module is the merged f32 matrix  W + (lora_alpha / r) B A  (ucod_lora_merge_f32: f64 arithmetic, one rounding to f32) and, with
        bias="lora_only", ``bias`` the trained one; every other entry is the same tensor.  Any frozen-backbone engine built from it runs the adapted model.  Merging is
        the eval-mode function: dropout plays no part.  Everything is in HF's shapes and row order.  One module at a time through a reusable device buffer: stage,
        merge, copy back."""
        base = self._base_sd if base_state_dict is None else base_state_dict
        pref = self._hf_prefix(base)
        out = dict(base)
        for i in range(self.L):
            for path, m in self._targeted():
                key = f"{pref}{i}.{path}.weight"
                w = base[key]
                w0, merged = self._stage_weight(key, w, m, engine_rows=False)
                self._merge(self.lib, w0, self.lora[i, m.a], m.get_rows(self.lora[i, m.b].reshape(m.nb, self.r)).contiguous(), merged)
                out[key] = merged[:, :m.k_hf].contiguous().to(w.device, copy=True)
            for j, m in enumerate(self.modules):
                if m.bias_off is not None:
                    key = f"{pref}{i}.{m.path}.bias"
                    out[key] = m.get_rows(self._bias_value(i, j).reshape(-1, 1)).reshape(-1).to(base[key].device, base[key].dtype, copy=True)
        for name, i, k in self._norm_names(pref):                  # bias="all": the LayerNorm betas and the patch bias
            out[name] = self._norm_value(i, k).to(base[name].device, base[name].dtype, copy=True)
        return out

    def _engine_row_source(self):
        """SwiGLU: for every row of the engine's padded, interleaved weights_in the HF row it holds, or 2 F0 (a zero row behind the staged HF weight) for padding."""
        if self._mlp_src_rows is None:
            from .swiglu import interleave_perm
            F, F0 = self.F, self._F0
            j = interleave_perm(F)
            src = torch.where(j < F, j, j - F + F0)
            src = torch.where((j % F) < F0, src, torch.full_like(src, 2 * F0))
            self._mlp_src_rows = src.to(self.device)
        return self._mlp_src_rows

    def merge_into(self, engine):
        """Refresh a live ``ViTEngine`` of the same checkpoint IN PLACE with this engine's current LoRA matrices: for every targeted module of every layer the merged
        f32 weight (from the f32 base weights, never from ``engine``'s current ones: refreshing after every optimiser step cannot drift) is staged in the engine's
        shape, merged and cast into the existing 16-bit tensor of ``engine.layers``; where a LayerNorm stands in front of the module and ``engine.ln_fold`` is on, it
        is also folded (ucod_fold_ln_linear) into the existing tensors of ``engine.fold_layers``, with the Q-row pre-scale the engine was built with
        (``engine.q_row_scale``).  No tensor of ``engine`` is reallocated, untargeted tensors (and the rows of untargeted projections in the fused QKV weight) are
        not written.  Runs on the current stream, ordered with ``engine``'s passes there."""
        if isinstance(engine, SplitViTEngine):
            raise NotImplementedError("merge_into refreshes the 16-bit ViTEngine only; build a SplitViTEngine from merged_state_dict() (its operands are split "
                                      "per tensor with their own scales)")
        if not isinstance(engine, ViTEngine) or isinstance(engine, ViTLoRAEngine):
            raise TypeError(f"merge_into takes a frozen-backbone ViTEngine, got {type(engine).__name__}")
        mine, theirs = (self.D, self.L, self.F, self.heads, self.mlp), (engine.D, engine.L, engine.F, engine.heads, engine.mlp)
        if mine != theirs:
            raise ValueError(f"merge_into: the engines differ in (D, L, F, heads, MLP kind): {mine} here, {theirs} there")
        if self.rope != engine.rope:
            raise ValueError("merge_into: one engine is a DINOv3 (rotary) one, the other is not: they were not built from the same checkpoint")
        if self.R != engine.R:
            raise ValueError(f"merge_into: this engine has {self.R} register tokens, the other {engine.R}: they were not built from the same checkpoint")
        if engine.patch_w.device != self.lora.device:
            raise ValueError(f"merge_into: this engine is on {self.lora.device}, the other on {engine.patch_w.device}")
        base, lib, st = self._base_sd, engine.lib, N.stream
        pref = self._hf_prefix(base)
        base_ptrs = {v.untyped_storage().data_ptr() for v in base.values() if torch.is_tensor(v) and v.is_cuda} if self.bias_numel else ()
        if self.norm_off:                                          # bias="all": the patch bias, and below every layer's betas, before the folds read them
            if engine.patch_b.untyped_storage().data_ptr() in base_ptrs:
                engine.patch_b = engine.patch_b.clone()
            engine.patch_b.copy_(self._norm_value(0, 2))
        for i in range(self.L):
            row, fl = engine.layers[i], (engine.fold_layers[i] if engine.ln_fold else None)
            for k, slot in enumerate((N.LN1_B, N.LN2_B) if self.norm_off else ()):
                if row[slot].untyped_storage().data_ptr() in base_ptrs:
                    own = row[slot].clone()
                    if fl is not None and fl[slot] is row[slot]:
                        fl[slot] = own
                    row[slot] = own
                row[slot].copy_(self._norm_value(i, k))
            for j, m in enumerate(self.modules):                   # bias="lora_only": the trained biases into the live bias vectors first, so that the LayerNorm fold
                if m.bias_off is not None:                         # below reads them (its folded bias is b' = q (W beta + b))
                    slot = m.b_slot
                    if row[slot].untyped_storage().data_ptr() in base_ptrs:      # (an f32 state dict on the device: the engine's vector IS the checkpoint's -- the one
                        own = row[slot].clone()                                  #  case in which a tensor of ``engine`` is replaced, once, so that the base stays the base)
                        if fl is not None and fl[slot] is row[slot]:
                            fl[slot] = own
                        row[slot] = own
                    row[slot][m.row0:m.row0 + m.nb].copy_(self._bias_value(i, j))
            for key, w, m, A, B, rank in self._engine_units(i, base, pref):
                w0, merged = self._stage_weight(key, w, m, engine_rows=True)
                self._merge(lib, w0, A, B, merged, rank)
                n, k, r0, plain = m.n, m.k, m.row0, row[m.w_slot]
                N.check(lib.ucod_cast_f32_bf16(N.ptr(merged), plain.data_ptr() + r0 * k * plain.element_size(), n * k, st()), "ucod_cast_f32_bf16")
                if m.w_slot == N.FC2_W:
                    engine.refresh_fc2_perm(i)                     # (the BLK16 copy of fc2 follows the plain one)
                if fl is not None and m.ln is not None:            # (no LayerNorm stands in front of an output projection: no fold)
                    wf, bf, cs = fl[m.w_slot], fl[m.b_slot], fl[m.c_slot]
                    q = engine.q_row_scale.data_ptr() + r0 * 4 if m.w_slot == N.QKV_W else None
                    N.check(lib.ucod_fold_ln_linear(N.ptr(merged), N.ptr(row[m.ln[0]]), N.ptr(row[m.ln[1]]), row[m.b_slot].data_ptr() + r0 * 4, q,
                                                    wf.data_ptr() + r0 * k * wf.element_size(), bf.data_ptr() + r0 * 4, cs.data_ptr() + r0 * 4, n, k, st()), "ucod_fold_ln_linear")
        return engine


    # ---- torch.autograd / nn.Module integration ----------------------------------------------------------------------
    def clone_for_ema(self):
        """A second engine over the SAME frozen weight tensors with its own LoRA arena (models/modules/full_model.py:84:
        ``backbone_ema = copy.deepcopy(backbone)``; only the LoRA matrices can ever differ, so only they are duplicated) and its own
        saturation guard: the clone's passes are reported by the clone."""
        other = object.__new__(ViTLoRAEngine)
        other.__dict__.update(self.__dict__)
        other.lora = self.lora.clone()
        other.lora_grad = torch.zeros_like(self.lora)
        other.train_layers = [[t.clone() if s in (N.T_QKV_W_AUG, N.T_QKV_WT_AUG) else t for s, t in enumerate(tl)] for tl in self.train_layers]
        other.mlp_layers = [[t.clone() for t in ml] for ml in self.mlp_layers]          # (the augmented fc1 weight carries the clone's own B_m)
        if self._bias_flat is not None:                            # trained biases: the clone's bias vectors follow ITS arena (``repack``), so they are its own
            other._bias_flat = self._bias_flat.clone()
            other._link_bias()
        other._tside, other._saved_for = None, None
        other._merge_buf = None                                    # (its own staging buffer; the f32 base weights ``_base_sd`` are shared)
        other._guard = _SaturationGuard(self.lib, self.device)
        other._pos_cache = dict(self._pos_cache)
        # The reference's teacher is a deepcopy that stays in train mode (full_model.py:84; nobody calls eval() on it), so its LoRA
        # dropout is active too, with masks drawn independently of the student's: own seed stream, own step counter.
        other._seed = (self._seed * 0x2545F4914F6CDD1D + 0x5DEECE66D) & _MASK64
        other._step, other._step_seed = 0, 0
        other.repack()
        return other

    def apply(self, img, lora_param):
        """Differentiable call: key = f(img; lora_param).  ``lora_param`` must be a tensor sharing storage with ``self.lora``
        (see ``LoRABackbone``); its ``.grad`` receives ``self.lora_grad`` on backward."""
        return _LoRABackboneFn.apply(img, lora_param, self)


class _LoRABackboneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, lora_param, engine):
        if lora_param.data_ptr() != engine.lora.data_ptr():
            raise RuntimeError("lora_param must alias engine.lora")
        ctx.engine = engine
        return engine.forward_train(img)

    @staticmethod
    def backward(ctx, dkey):
        g = ctx.engine.backward(dkey.contiguous())
        return None, g.clone(), None
