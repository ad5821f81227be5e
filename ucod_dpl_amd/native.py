"""ctypes binding of libucod_dpl.so (C ABI in include/ucod_dpl.h).

There is deliberately NO fallback: if the shared library is missing, or a tensor is not on a
gfx950 device, the call raises.  PyTorch is used only for device memory and streams.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_native", "libucod_dpl.so")
# Experiment builds (`make -C ucod_dpl_amd/csrc variant ...`) are selected by tools/ with UCOD_DPL_EXPERIMENT_LIB; the variable is honoured
# only together with UCOD_DPL_ALLOW_EXPERIMENT=1, so that a stray environment variable cannot swap the product library.
if os.environ.get("UCOD_DPL_LIB"):
    raise RuntimeError("UCOD_DPL_LIB is no longer read (a stray variable must not swap the product library): use "
                       "UCOD_DPL_ALLOW_EXPERIMENT=1 UCOD_DPL_EXPERIMENT_LIB=<path> for an experiment build")
if os.environ.get("UCOD_DPL_EXPERIMENT_LIB") and os.environ.get("UCOD_DPL_ALLOW_EXPERIMENT") == "1":
    LIB_PATH = os.environ["UCOD_DPL_EXPERIMENT_LIB"]
ABI_VERSION = 5                                            # include/ucod_dpl.h: UCOD_ABI_VERSION

EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_SCALE_RESID_F32, EPI_PATCH_TOKENS_F32, EPI_KEY_NCHW_F32, EPI_BIAS_F32 = range(6)
EPI_GELU_BWD_BF16, EPI_BIAS_GELU_SAVE_BF16 = 6, 7          # ucod_gemm_bf16_train only (backbone-backward mode)
EPI_QKV_FP8 = 8                                            # QKV projection of the fp8 attention path
EPI_BIAS_SCALE_RESID_H16, EPI_PATCH_TOKENS_H16 = 9, 10     # f16 residual stream (VitDesc.resid16)
EPI_LNFOLD_BIAS_BF16, EPI_LNFOLD_GELU_BF16 = 11, 12        # ucod_gemm_lnfold only (LayerNorm folded into QKV / fc1; the fp16-operand build)
EPI_BIAS_SCALE_RESID_H16_STATS, EPI_PATCH_TOKENS_H16_STATS = 13, 14   # ucod_gemm_bf16_stats only (the producers that leave row partials)
EPI_BIAS_GELU_SPLIT2 = 15                                  # fc1 + GELU + two-term split of the result in one launch (the split-operand pass; bf16 library)
# SwiGLU MLP of DINOv2 ViT-g/14 on interleaved weights_in rows (include/ucod_dpl.h): 16-bit [M, N/2] (both libraries); the LayerNorm-folded form (ucod_gemm_lnfold,
# fp16-operand build); the two-term split operand of the result (bf16 library)
EPI_BIAS_SWIGLU_BF16, EPI_LNFOLD_SWIGLU_BF16, EPI_BIAS_SWIGLU_SPLIT2 = 16, 17, 18
# backbone-backward mode on the SwiGLU MLP (ucod_gemm_bf16_train only, bf16 library): the training-mode weights_in (hidden + saved interleaved pre-activation) and the
# weights_out dgrad whose drain writes the cotangent of the interleaved weights_in output
EPI_BIAS_SWIGLU_SAVE_BF16, EPI_SWIGLU_BWD_BF16 = 21, 22
EPI_LNFOLD_GELU_BLK16, EPI_BIAS_GELU_BLK16 = 23, 24        # fc1 + GELU with the hidden in BLK16 (MFMA-fragment) order: the A operand of ucod_gemm_bf16_blk16a
VIT_LAYER_STRIDE = 16
# the slots of one layer's row of the pointer table, in table order (include/ucod_dpl.h: ucod_vit_forward); "_w" entries are 16-bit (or split) matrices, the rest f32
VIT_LAYER_SLOTS = ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2", "aux0", "aux1")
LN1_G, LN1_B, QKV_W, QKV_B, PROJ_W, PROJ_B, LS1, LN2_G, LN2_B, FC1_W, FC1_B, FC2_W, FC2_B, LS2, AUX0, AUX1 = range(VIT_LAYER_STRIDE)
QKV_COLSUM, FC1_COLSUM = AUX0, AUX1                        # ln_fold tables: column sums of the folded QKV / fc1 weights (unused without the fold)
KEY_ROWS_A, SPLIT_UNUSED = AUX0, AUX1                      # split tables: the K rows of qkv_w as an A-side operand (key hook); +15 is never read there
VIT_TRAIN_STRIDE = 7
# one layer's row of the training table (ucod_vit_forward_train): five frozen weights the engine keeps, then the LoRA parameters and gradients of the pass
VIT_TRAIN_SLOTS = ("qkv_w_aug", "qkv_wt_aug", "proj_wt", "fc1_wt", "fc2_wt", "lora", "lora_grad")
T_QKV_W_AUG, T_QKV_WT_AUG, T_PROJ_WT, T_FC1_WT, T_FC2_WT, T_LORA, T_LORA_GRAD = range(VIT_TRAIN_STRIDE)
LORA_AUG = 64
# the per-layer table of a LoRA module on the MLP input projection (the _lora_mlp entry points): the augmented fc1 / weights_in weight, then its parameters and gradients
VIT_TRAIN_MLP_STRIDE = 3
VIT_TRAIN_MLP_SLOTS = ("fc1_w_aug", "lora_mlp", "lora_mlp_grad")
M_FC1_W_AUG, M_LORA, M_LORA_GRAD = range(VIT_TRAIN_MLP_STRIDE)
LORA_MLP_MAX_R = 8                                          # include/ucod_dpl.h: UCOD_LORA_MLP_MAX_R
# the per-layer table of the LoRA modules on the output projections (the _lora_out entry points): parameters and gradients of dense / o_proj, then of fc2 / down_proj;
# an untargeted module's two slots are NULL
VIT_TRAIN_OUT_STRIDE = 4
VIT_TRAIN_OUT_SLOTS = ("lora_dense", "lora_dense_grad", "lora_fc2", "lora_fc2_grad")
O_LORA_DENSE, O_LORA_DENSE_GRAD, O_LORA_FC2, O_LORA_FC2_GRAD = range(VIT_TRAIN_OUT_STRIDE)
LORA_OUT_W = 8                                              # include/ucod_dpl.h: UCOD_LORA_OUT_W (floats per row of the saved u and of t)
LORA_OUT_ACT_IDENTITY, LORA_OUT_ACT_GELU = 0, 1
LORA_OUT_ACT_SWIGLU = 2                                     # include/ucod_dpl.h: UCOD_LORA_OUT_ACT_SWIGLU (x_in / cot are the interleaved [rows, 2K] pre-activation / dpre)
LORA_OUT_SWIGLU = 1                                         # include/ucod_dpl.h: UCOD_LORA_OUT_SWIGLU (out_flags of the _lora_out_ex entry points)
LORA_MLP_PAIR = 4                                           # include/ucod_dpl.h: UCOD_LORA_MLP_PAIR (the MLP table holds the gated MLP's gate_proj / up_proj pair)
LORA_WIDE = 16                                              # include/ucod_dpl.h: UCOD_LORA_WIDE (the passes size and run the MLP modules through the _wide row entry points)
LORA_WIDE_MAX_N1, LORA_WIDE_MAX_K = 10240, 8192             # include/ucod_dpl.h: UCOD_LORA_WIDE_MAX_N1 / _MAX_K (what the wide kernels hold with no scratch memory)
# the per-layer table of the trained biases' gradient destinations (bias="lora_only": the _lora_bias entry points); NULL = that bias is not trained
VIT_TRAIN_BIAS_STRIDE = 6
VIT_TRAIN_BIAS_SLOTS = ("gb_q", "gb_k", "gb_v", "gb_m", "gb_o", "gb_2")

vp, ci, cf, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class VitDesc(C.Structure):
    _fields_ = [(n, ci) for n in ("B", "C", "H", "W", "P", "D", "heads", "F", "L", "Kpad")] + [("eps", cf)] + \
               [(n, ci) for n in ("full_last_layer", "gemm_variant", "attn_variant", "resid16", "ln_fold", "n_reg")] + \
               [("rope", vp)]             # (ctypes zero-fills: n_reg = 0 and rope = NULL -- no registers, no rotary embedding -- unless set)


class VitTrainDesc(C.Structure):
    _fields_ = [("vit", VitDesc), ("lora_r", ci), ("lora_scaling", cf), ("lora_dropout", cf), ("seed", C.c_ulonglong),
                ("allow_rope", ci)]       # (zero-filled: a rotary table in ``vit`` is refused by the training-pass drivers unless this is 1)


class LoraDropout(C.Structure):
    _fields_ = [("p", cf), ("seed", C.c_ulonglong), ("layer", ci)]


class DiscParams(C.Structure):
    _fields_ = [(n, vp) for n in ("w1", "g1", "b1", "w2", "g2", "b2", "w3", "g3", "b3", "lin_w", "lin_b",
                                  "rm1", "rv1", "rm2", "rv2", "rm3", "rv3", "nbt")]


class DiscGrads(C.Structure):
    _fields_ = [(n, vp) for n in ("w1", "g1", "b1", "w2", "g2", "b2", "w3", "g3", "b3", "lin_w", "lin_b")]


ROPE_ELEM_HALF, ROPE_ELEM_F32 = 0, 1          # element type of ucod_rope_qk's buffer: the library's 16-bit operand type / f32
LNB_DY_BF16 = 1                              # include/ucod_dpl.h: UCOD_LNB_DY_BF16 (flag of ucod_layernorm_bwd_ex / ucod_layernorm_param_grad: dy is bf16)
UCOD_MLP_GELU, UCOD_MLP_SWIGLU = 0, 1        # MLP kind of the _mlp backbone entry points (include/ucod_dpl.h)
# activation operand classes of the fp16-term split pass (ucod_split16_class_scale)
SPLIT16_LN, SPLIT16_QKV, SPLIT16_PROB, SPLIT16_ATT, SPLIT16_HIDDEN, SPLIT16_PATCH = range(6)
SPLIT16_FUSE_MLP = 1                            # flag of the ucod_vit_*_split16_ex entry points: fc1 + activation + split in one launch

# name -> (restype, argtypes); must list EVERY symbol include/ucod_dpl.h declares (tests/test_abi.py checks)
SIGNATURES = {
    "ucod_abi_version": (ci, []),
    "ucod_device_is_gfx950": (ci, []),
    "ucod_half_name": (C.c_char_p, []),
    "ucod_prof_enable": (ci, [ci]),
    "ucod_prof_num_classes": (ci, []),
    "ucod_prof_class_name": (C.c_char_p, [ci]),
    "ucod_prof_collect": (ci, [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "ucod_clock_probe": (ci, [vp, vp]),
    "ucod_split_products": (ci, [ci]),
    "ucod_split_rows": (ci, [vp, C.c_long, vp, ci, ci, ci, ci, ci, cf, vp]),
    "ucod_layernorm_split": (ci, [vp, vp, vp, vp, ci, ci, cf, ci, ci, vp]),
    "ucod_patch_im2col_split": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_attention_split_operand_bytes": (sz, [ci, ci, ci, ci]),
    "ucod_qkv_split": (ci, [vp, vp, ci, ci, ci, ci, cf, vp]),
    "ucod_attention_split_fwd": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "ucod_vit_split_workspace_bytes": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_split_stream_offset": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_forward_split": (ci, [C.POINTER(VitDesc), ci, C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_split_workspace_bytes_mlp": (sz, [C.POINTER(VitDesc), ci, ci]),
    "ucod_vit_split_stream_offset_mlp": (sz, [C.POINTER(VitDesc), ci, ci]),
    "ucod_vit_forward_split_mlp": (ci, [C.POINTER(VitDesc), ci, ci, C.POINTER(vp), vp, vp, vp, sz, vp]),
    # the split-operand pass on fp16 terms ("split2h", csrc/split16.hip): libucod_dpl_f16.so; the bf16 build returns UCOD_EINVAL
    "ucod_split16_class_scale": (cf, [ci]),
    "ucod_split16_rows": (ci, [vp, C.c_long, vp, ci, ci, ci, ci, cf, cf, vp]),
    "ucod_split16_layernorm": (ci, [vp, vp, vp, vp, ci, ci, cf, ci, cf, vp]),
    "ucod_split16_patch_im2col": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]),
    "ucod_split16_scale_f32": (ci, [vp, sz, cf, vp]),
    "ucod_split16_attention_operand_bytes": (sz, [ci, ci, ci]),
    "ucod_split16_qkv": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "ucod_split16_attention_fwd": (ci, [vp, vp, ci, ci, ci, cf, cf, vp]),
    "ucod_split16_mfma_subnormal_probe": (ci, [vp, vp]),
    "ucod_vit_split16_workspace_bytes": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_split16_stream_offset": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_forward_split16": (ci, [C.POINTER(VitDesc), ci, C.POINTER(vp), C.POINTER(cf), ci, vp, vp, vp, sz, vp]),
    # fc1 + activation + split in one launch, and the pass with options (UCOD_SPLIT16_FUSE_MLP: "split2hf")
    "ucod_split16_gemm_act": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, cf, cf, ci, vp]),
    "ucod_vit_split16_workspace_bytes_ex": (sz, [C.POINTER(VitDesc), ci, ci]),
    "ucod_vit_split16_stream_offset_ex": (sz, [C.POINTER(VitDesc), ci, ci]),
    "ucod_vit_forward_split16_ex": (ci, [C.POINTER(VitDesc), ci, ci, C.POINTER(vp), C.POINTER(cf), ci, vp, vp, vp, sz, vp]),
    "ucod_gemm_bf16": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, vp]),
    # DINOv3: rotary position embedding on the Q and K thirds of the patch rows of a QKV buffer, in place (csrc/rope.hip); elem = ROPE_ELEM_HALF / ROPE_ELEM_F32
    "ucod_rope_qk": (ci, [vp, ci, vp, ci, ci, ci, ci, vp]),
    # the same with a row pitch (elements) and a direction (1 = the transpose: cotangents of rotated q / k back to the projection outputs')
    "ucod_rope_qk_ld": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]),
    # DINOv2 with registers: the row-mapped drains, leading-row kernels, key-gradient scatter and CLS attention row for tok = 1 + n_reg + n tokens per image
    "ucod_gemm_bf16_reg": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, vp]),
    "ucod_gemm_bf16_stats_reg": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, vp, ci, vp]),
    "ucod_cls_rows_reg": (ci, [vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_cls_rows_h16_reg": (ci, [vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_cls_rows_h16_stats_reg": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_key_grad_tokens_reg": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "ucod_cls_qk_reg": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_cls_attention_reg": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    # DINOv3: the same row with the patch keys rotated on the fly by the [hw, 64] rotary table (4th argument)
    "ucod_cls_attention_rope": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    "ucod_gemm_lnfold": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, cf, vp, ci, vp]),
    "ucod_gemm_bf16_blk16a": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, vp]),
    "ucod_gemm_bf16_stats": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, vp, ci, vp]),
    "ucod_cls_rows_h16_stats": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_row_stats_h16": (ci, [vp, vp, ci, ci, cf, vp]),
    "ucod_gemm_reload_tuning": (None, []),
    "ucod_resid16_overflow_fetch": (ci, [vp, vp]),
    "ucod_resid16_overflow_reset": (ci, [vp]),
    "ucod_resid16_overflow_bind": (ci, [vp]),
    "ucod_layernorm": (ci, [vp, vp, vp, vp, ci, ci, cf, ci, vp]),
    "ucod_layernorm_h16": (ci, [vp, vp, vp, vp, ci, ci, cf, vp]),
    "ucod_attention_fwd": (ci, [vp, vp, ci, ci, ci, cf, ci, vp]),
    "ucod_attention_fp8_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_attention_fwd_fp8": (ci, [vp, vp, vp, sz, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_attention_fp8_zero_pad": (ci, [vp, ci, ci, ci, vp]),
    "ucod_attention_fwd_fp8_fused": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_patch_im2col": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_cls_rows": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_cls_rows_h16": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_fill_qscale": (ci, [vp, ci, cf, vp]),
    "ucod_fill_qscale3": (ci, [vp, ci, cf, cf, cf, vp]),
    "ucod_cast_f32_bf16": (ci, [vp, vp, sz, vp]),
    "ucod_vit_workspace_bytes": (sz, [C.POINTER(VitDesc)]),
    "ucod_vit_forward": (ci, [C.POINTER(VitDesc), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_workspace_bytes_mlp": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_forward_mlp": (ci, [C.POINTER(VitDesc), ci, C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_forward_blk16": (ci, [C.POINTER(VitDesc), ci, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_gemm_blk16_pair_ok": (ci, [ci, ci, ci, ci]),
    "ucod_vit_last_ln1_offset_mlp": (sz, [C.POINTER(VitDesc), ci]),
    "ucod_vit_train_workspace_bytes": (sz, [C.POINTER(VitTrainDesc)]),
    "ucod_vit_forward_train": (ci, [C.POINTER(VitTrainDesc), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_backward": (ci, [C.POINTER(VitTrainDesc), C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    "ucod_vit_lora_infer_workspace_bytes": (sz, [C.POINTER(VitTrainDesc)]),
    "ucod_vit_forward_lora_infer": (ci, [C.POINTER(VitTrainDesc), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    # the five training-pass entry points with the MLP kind (UCOD_MLP_*) behind the descriptor
    "ucod_vit_train_workspace_bytes_mlp": (sz, [C.POINTER(VitTrainDesc), ci]),
    "ucod_vit_forward_train_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_backward_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    "ucod_vit_lora_infer_workspace_bytes_mlp": (sz, [C.POINTER(VitTrainDesc), ci]),
    "ucod_vit_forward_lora_infer_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    # LoRA on the MLP input projection as well: its row kernels, and the five entry points with the module's own per-layer table (NULL = the _mlp forms)
    "ucod_layernorm_lora_mlp": (ci, [vp, ci, vp, vp, vp, ci, vp, ci, ci, cf, C.POINTER(LoraDropout), vp]),
    "ucod_lora_mlp_pack": (ci, [vp, ci, cf, vp, ci, ci, vp]),
    "ucod_lora_mlp_grad_workspace_bytes": (sz, [ci, ci]),
    "ucod_lora_mlp_grad": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_layernorm_bwd_lora_mlp": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, cf, vp, ci, vp, ci, C.POINTER(LoraDropout), vp]),
    # the gated MLP's pair gate_proj / up_proj on the fused weights_in: [A_g | A_u | B_m], two masks (LORA_MLP_PAIR selects them in the _lora_out_ex passes)
    "ucod_layernorm_lora_mlp_pair": (ci, [vp, ci, vp, vp, vp, ci, vp, ci, ci, cf, C.POINTER(LoraDropout), vp]),
    "ucod_lora_mlp_pair_pack": (ci, [vp, ci, cf, vp, ci, ci, vp]),
    "ucod_lora_mlp_pair_grad_workspace_bytes": (sz, [ci, ci]),
    "ucod_lora_mlp_pair_grad": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_layernorm_bwd_lora_mlp_pair": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, cf, vp, ci, vp, ci, C.POINTER(LoraDropout), vp]),
    "ucod_vit_train_workspace_bytes_lora_mlp": (sz, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp)]),
    "ucod_vit_forward_train_lora_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_backward_lora_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    "ucod_vit_lora_infer_workspace_bytes_lora_mlp": (sz, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp)]),
    "ucod_vit_forward_lora_infer_lora_mlp": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    # LoRA on the output projections (dense / fc2; o_proj / down_proj): its row kernels, and the five entry points with the modules' own per-layer table (NULL = _lora_mlp)
    "ucod_lora_out_grad_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_lora_out_fwd": (ci, [vp, vp, ci, cf, vp, vp, ci, vp, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_lora_out_grad_s": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, vp]),
    "ucod_lora_out_grad_x": (ci, [vp, ci, vp, vp, vp, ci, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_lora_out_grad_x_ex": (ci, [vp, ci, ci, vp, vp, vp, ci, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),      # (+ out_flags behind act: LORA_OUT_SWIGLU for act 2)
    # the _wide forms of the row entry points without a flags word: supersets, up to LORA_WIDE_MAX_N1 rows of the MLP input weight / LORA_WIDE_MAX_K input columns
    "ucod_lora_mlp_pack_wide": (ci, [vp, ci, cf, vp, ci, ci, vp]),
    "ucod_lora_mlp_pair_pack_wide": (ci, [vp, ci, cf, vp, ci, ci, vp]),
    "ucod_lora_mlp_grad_workspace_bytes_wide": (sz, [ci, ci]),
    "ucod_lora_mlp_pair_grad_workspace_bytes_wide": (sz, [ci, ci]),
    "ucod_lora_mlp_grad_wide": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_lora_mlp_pair_grad_wide": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_lora_out_grad_workspace_bytes_wide": (sz, [ci, ci, ci]),
    "ucod_lora_out_fwd_wide": (ci, [vp, vp, ci, cf, vp, vp, ci, vp, ci, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_lora_out_grad_s_wide": (ci, [vp, vp, vp, ci, cf, vp, vp, vp, sz, ci, ci, ci, vp]),
    "ucod_vit_train_workspace_bytes_lora_out": (sz, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_forward_train_lora_out": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_backward_lora_out": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    "ucod_vit_lora_infer_workspace_bytes_lora_out": (sz, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_forward_lora_infer_lora_out": (ci, [C.POINTER(VitTrainDesc), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    # the same five with one word of flags behind `mlp` (LORA_OUT_SWIGLU: the SwiGLU MLP's output projection in the fc2 slots); flags 0 = the forms above
    "ucod_vit_train_workspace_bytes_lora_out_ex": (sz, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_forward_train_lora_out_ex": (ci, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    "ucod_vit_backward_lora_out_ex": (ci, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    "ucod_vit_lora_infer_workspace_bytes_lora_out_ex": (sz, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_forward_lora_infer_lora_out_ex": (ci, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, sz, vp]),
    # LoRA bias="lora_only": deterministic column sums (elem = ROPE_ELEM_HALF / ROPE_ELEM_F32), and the backward / its size function with the bias table behind the
    # output modules' one (NULL = the _lora_out_ex forms)
    "ucod_colsum_det_workspace_bytes": (sz, [ci, ci]),
    "ucod_colsum_det": (ci, [vp, ci, ci, ci, ci, vp, vp, vp, sz, vp]),
    "ucod_vit_train_workspace_bytes_lora_bias": (sz, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_backward_lora_bias": (ci, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, sz, vp]),
    # LoRA bias="all": the column sum of a LayerNorm output's complete cotangent (dy + the masked LoRA branch; flags = LNB_DY_BF16 or 0), the column sum over the
    # patch rows of every image, and the backward / its size function with the norm table behind the bias table (NULL = the _lora_bias forms)
    "ucod_colsum_det_lora_workspace_bytes": (sz, [ci, ci]),
    "ucod_colsum_det_lora": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, ci, C.POINTER(LoraDropout), vp, vp, sz, vp]),
    "ucod_colsum_det_tok_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "ucod_colsum_det_tok": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]),
    "ucod_vit_train_workspace_bytes_lora_bias_ex": (sz, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "ucod_vit_backward_lora_bias_ex": (ci, [C.POINTER(VitTrainDesc), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                            vp, vp, sz, vp]),
    # merging trained LoRA matrices into ordinary weights, and the device form of the LayerNorm fold (fp16-operand build) for the merged weight
    "ucod_lora_merge_f32": (ci, [vp, vp, vp, ci, cf, vp, ci, ci, vp]),
    "ucod_fold_ln_linear": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "ucod_gemm_bf16_train": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, ci, vp]),
    "ucod_layernorm_lora_fits": (ci, [ci, ci, ci]),
    "ucod_layernorm_lora": (ci, [vp, vp, vp, vp, ci, vp, ci, ci, cf, C.POINTER(LoraDropout), vp]),
    "ucod_layernorm_lora_h16": (ci, [vp, vp, vp, vp, ci, vp, ci, ci, cf, C.POINTER(LoraDropout), vp]),
    "ucod_layernorm_bwd_lora": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, vp, vp, ci, C.POINTER(LoraDropout), vp]),
    "ucod_layernorm_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, vp]),
    "ucod_layernorm_bwd_ex": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, cf, vp]),
    "ucod_layernorm_bwd_lora_ex": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, cf, vp, vp, ci, C.POINTER(LoraDropout), vp]),
    "ucod_attention_fwd_lse": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_attention_bwd": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_key_grad_tokens": (ci, [vp, vp, ci, ci, ci, vp]),
    "ucod_lora_pack": (ci, [vp, ci, cf, vp, vp, ci, ci, vp]),
    "ucod_lora_grad_workspace_bytes": (sz, [ci]),
    "ucod_lora_grad": (ci, [vp, vp, vp, ci, cf, vp, ci, vp, sz, ci, ci, C.POINTER(LoraDropout), vp]),
    "ucod_bilinear_resize": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_bilinear_resize_adjoint": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_dba_project": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_dba_project_split_workspace_bytes": (sz, [ci, ci]),
    "ucod_dba_project_split": (ci, [vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, vp]),
    "ucod_dba_colnorm": (ci, [vp, ci, ci, vp, vp, ci, ci, vp]),
    "ucod_dba_heads_fwd": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "ucod_orth_workspace_bytes": (sz, [ci, ci]),
    "ucod_orth_gram_fwd": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "ucod_dba_bwd_workspace_bytes": (sz, [ci, ci]),
    "ucod_dba_bwd": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, ci, ci, vp]),
    "ucod_dba_wgrad": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_dba_wgrad_split": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_disc_saved_bytes": (sz, [ci, ci]),
    "ucod_disc_fwd": (ci, [vp, C.POINTER(DiscParams), vp, vp, ci, ci, ci, vp]),
    "ucod_disc_bwd_workspace_bytes": (sz, [ci, ci]),
    "ucod_disc_bwd": (ci, [vp, C.POINTER(DiscParams), vp, vp, C.POINTER(DiscGrads), ci, vp, ci, ci, vp]),
    "ucod_unfold3x3": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_bn_lrelu_workspace_bytes": (sz, [ci]),
    "ucod_bn_lrelu_train": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, cf, cf, cf, ci, vp, sz, vp]),
    "ucod_linear_sigmoid": (ci, [vp, vp, vp, vp, ci, ci, vp]),
    "ucod_bn_lrelu_train_save": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, cf, cf, cf, ci, vp, sz, vp]),
    "ucod_bn_lrelu_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, cf, cf, ci, vp, sz, vp]),
    "ucod_fold3x3": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_conv_wgrad_f32": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_linear_sigmoid_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "ucod_disc_bce": (ci, [vp, vp, vp, vp, vp, ci, cf, vp]),
    "ucod_apm_bce": (ci, [vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, ci, ci, vp]),
    # the gradient into the features of the discriminator's feature branch: implicit 3x3 convolution, its data-gradient weights, d(step loss)/d(p_s, p_p)
    "ucod_conv3x3_f32": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_conv3x3_dgrad_weights": (ci, [vp, vp, ci, ci, ci, vp]),
    "ucod_apm_bce_gprob": (ci, [vp, vp, vp, vp, vp, vp, cf, cf, ci, vp, vp, ci, ci, vp]),
    # the deterministic forms of the training step's reductions (no floating-point atomics; explicit workspace behind the default form's arguments)
    "ucod_dba_wgrad_det_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "ucod_dba_wgrad_det": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "ucod_conv_wgrad_f32_det_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "ucod_conv_wgrad_f32_det": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, sz, vp]),
    "ucod_dba_heads_fwd_det_workspace_bytes": (sz, [ci, ci]),
    "ucod_dba_heads_fwd_det": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, vp]),
    "ucod_dba_bwd_det_workspace_bytes": (sz, [ci, ci]),
    "ucod_dba_bwd_det": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, sz, ci, ci, vp]),
    "ucod_apm_bce_det_workspace_bytes": (sz, [ci]),
    "ucod_apm_bce_det": (ci, [vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, vp, sz, ci, ci, vp]),
    "ucod_disc_fwd_det_workspace_bytes": (sz, [ci, ci]),
    "ucod_disc_fwd_det": (ci, [vp, C.POINTER(DiscParams), vp, vp, ci, ci, ci, vp, sz, vp]),
    "ucod_disc_bwd_det_workspace_bytes": (sz, [ci, ci]),
    "ucod_disc_bwd_det": (ci, [vp, C.POINTER(DiscParams), vp, vp, C.POINTER(DiscGrads), ci, vp, sz, ci, ci, vp]),
    "ucod_binarize": (ci, [vp, vp, sz, ci, vp]),
    "ucod_ccl8_host": (ci, [vp, ci, ci, vp]),
    "ucod_pil_resize_u8_host": (ci, [vp, ci, ci, vp, ci, ci, ci]),
    "ucod_vit_last_ln1_offset": (sz, [C.POINTER(VitDesc)]),
    "ucod_cls_qk": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "ucod_cls_attention": (ci, [vp, vp, vp, vp, ci, ci, ci, cf, vp]),
    "ucod_bkg_seg": (ci, [vp, vp, cf, cf, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "ucod_ccl8_workspace_bytes": (sz, [ci, ci]),
    "ucod_ccl8_components": (ci, [vp, ci, ci, vp, ci, vp, vp, sz, vp]),
    "ucod_paste_workspace_bytes": (sz, [ci, ci, ci, ci, ci]),
    "ucod_paste_resized_u8": (ci, [vp, ci, ci, ci, vp, vp, ci, ci, vp, sz, vp]),
    "ucod_paste_resized_u8_multi": (ci, [vp, ci, ci, ci, vp, vp, vp, ci, ci, ci, vp, sz, vp]),
    "ucod_crop_resize_norm_multi": (ci, [vp, vp, ci, vp, vp, ci, vp, ci, ci, vp, sz, vp]),
    "ucod_crop_workspace_bytes": (sz, [ci, ci, ci, ci, ci]),
    "ucod_crop_resize_norm": (ci, [vp, ci, ci, vp, ci, vp, ci, ci, vp, sz, vp]),
    "ucod_cross_attention96_fwd": (ci, [vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp]),
    "ucod_gather_tokens": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "ucod_entropy_scores": (ci, [vp, ci, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_dwconv7_maskdec": (ci, [vp, vp, vp, vp, cf, vp, ci, ci, ci, ci, vp]),
    "ucod_window_scatter": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_window_loss": (ci, [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    # training of the refiner's window branch (HRE.CSF): the forward with the base-2 log-sum-exp, the head_dim-96 attention backward, the loss gradient, the
    # depthwise-conv + mask-head backward, LayerNorm parameter gradients (flags = LNB_DY_BF16 or 0), the transposed bf16 operand of a weight-gradient GEMM
    "ucod_cross_attention96_fwd_lse": (ci, [vp, ci, vp, vp, ci, vp, vp, ci, ci, ci, ci, vp]),
    "ucod_cross_attention96_bwd": (ci, [vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_window_loss_grad": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "ucod_dwconv7_maskdec_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, vp]),
    "ucod_layernorm_param_grad": (ci, [vp, ci, vp, vp, vp, vp, sz, ci, ci, cf, vp]),
    "ucod_transpose_pad_bf16": (ci, [vp, ci, ci, ci, ci, vp, vp]),
    # the gradient through the refiner's `outputs` (train_outputs): backward of the gated ensembler in l2 and the fuser, and the window scatter's adjoint
    "ucod_gated_ensemble_bwd_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_gated_ensemble_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, vp]),
    "ucod_window_gather": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "ucod_wgrad_bf16_det_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_wgrad_bf16_det_nsplit": (ci, [ci, ci, ci]),
    "ucod_wgrad_bf16_det": (ci, [vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, sz, vp]),
    "ucod_gated_ensemble_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_gated_ensemble": (ci, [vp, vp, vp, vp, vp, cf, vp, vp, vp, ci, ci, ci, vp]),
    "ucod_step_loss": (ci, [vp, vp, ci, vp, vp]),
    "ucod_copy_segments": (ci, [vp, vp, vp, ci, vp]),
    "ucod_zero_segments": (ci, [vp, vp, ci, vp]),
    "ucod_accumulators_prezeroed": (ci, [ci]),
    "ucod_adamw_ema": (ci, [vp, vp, vp, vp, vp, sz, cf, cf, cf, cf, cf, ci, cf, vp]),
    "ucod_cod_metrics_workspace_bytes": (sz, [ci, ci, ci]),
    "ucod_cod_metrics": (ci, [vp, vp, ci, ci, ci, vp, vp, sz, vp]),
}
COD_RECORD = 1032

LIB_PATH_F16 = os.path.join(_HERE, "_native", "libucod_dpl_f16.so")   # same sources built with -DUCOD_HALF_F16 (fp16 forward-path operands)
if os.environ.get("UCOD_DPL_EXPERIMENT_LIB_F16") and os.environ.get("UCOD_DPL_ALLOW_EXPERIMENT") == "1":
    LIB_PATH_F16 = os.environ["UCOD_DPL_EXPERIMENT_LIB_F16"]          # tools/: e.g. the -DUCOD_LAB_KNOBS build (`make -C ucod_dpl_amd/csrc knobs`)
_libs = {}


def load(half="bf16"):
    """Load a shared library (once each).  ``half`` selects the build: "bf16" (default, the product path of BASELINE configs[1]) or
    "f16" (the same kernels on IEEE fp16 operands -- the arithmetic type of the reference's fp16-autocast launcher).
    Raises if the library has not been built -- never falls back."""
    if half not in ("bf16", "f16"):
        raise ValueError(f"half must be 'bf16' or 'f16', got {half!r}")
    if half not in _libs:
        path = LIB_PATH if half == "bf16" else LIB_PATH_F16
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"or `make -C ucod_dpl_amd/csrc` (hipcc --offload-arch=gfx950). There is no fallback path.")
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.ucod_abi_version() != ABI_VERSION:
            raise ImportError(f"{path} has ABI version {lib.ucod_abi_version()}, this binding needs {ABI_VERSION}: rebuild it "
                              f"(`make -C ucod_dpl_amd/csrc`)")
        if lib.ucod_half_name().decode() != half:
            raise ImportError(f"{path} was built for {lib.ucod_half_name().decode()} operands, expected {half}")
        _libs[half] = lib
    return _libs[half]


# ---- the laboratory library (csrc/variants/*.hip, `make -C ucod_dpl_amd/csrc variants`): never loaded by the product path
LIB_PATH_LAB = os.path.join(_HERE, "_native", "libucod_dpl_variants.so")
LAB_SIGNATURES = {
    "ucod_attention_fwd_lab": (ci, [vp, vp, ci, ci, ci, cf, ci, vp]),
    "ucod_attention_fwd_asm_lab": (ci, [vp, vp, vp, ci, ci, ci, ci, vp]),     # the hand-placed assembly kernels (form 0 = pw64, 1 = pw32), optional LSE
    "ucod_gemm_bf16_lab": (ci, [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, vp]),
    "ucod_gemm_bf16_asm_lab": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "ucod_gemm_bf16_asm_lab_forms": (ci, []),
    "ucod_gemm_bf16_asm_lab_label": (C.c_char_p, [ci]),
}
ATTN_PRODUCT_VARIANTS = (0, 2, 5, 66)           # 5 / 66 = attn_fwd_v5_kernel / attn_fwd_v6_kernel by name
GEMM_PRODUCT_VARIANTS = (0, 1, 2, 9, 10, 12, 13, 14)


def have_lab():
    return os.path.exists(LIB_PATH_LAB)


def load_lab():
    """The experiment variants of rounds 1-2 (tools/, tests marked `variants`).  Raises if `make variants` has not been run."""
    if "lab" not in _libs:
        if not have_lab():
            raise ImportError(f"{LIB_PATH_LAB} is missing: build it with `make -C ucod_dpl_amd/csrc variants` (laboratory kernels; "
                              f"the product path never needs it)")
        lib = C.CDLL(LIB_PATH_LAB)
        for name, (res, args) in LAB_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _libs["lab"] = lib
    return _libs["lab"]


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("ucod_dpl_amd: tensor is not on a GPU; the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("ucod_dpl_amd: tensor must be contiguous")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}" + (" (invalid argument)" if rc == -1 else ""))
