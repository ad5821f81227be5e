/* ucod_dpl.h -- C ABI of libucod_dpl.so: the MI355X (gfx950) hot path of UCOD-DPL.
 *
 * The reference (Heartfirey/UCOD-DPL) is pure Python/PyTorch: it has no FFI of its own.  The
 * boundary this library replaces is therefore the set of ATen / HuggingFace op call sites on the
 * path BASELINE.json:north_star names; every entry point below cites the reference lines whose
 * device arithmetic it takes over (paths relative to the reference repo root).  The Python host
 * side (ucod_dpl_amd/) binds these with ctypes and re-exposes the reference's module interface
 * (models/uscod.py::baseline, models/discriminator.py::Discriminator,
 * data/utils/feature_extractor.py::backbone, engine/runner/loop_UCOD_DPL.py::TrainLoop).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous,
 *     stream-ordered and re-entrant; workspace sizes come from the *_workspace_bytes helpers;
 *   - return value: 0 on success, UCOD_EINVAL (-1) for rejected arguments, otherwise a hipError_t;
 *   - "bf16" buffers are raw uint16 bfloat16; "f32" are IEEE float.
 *   - tensors are dense row-major; [B,C,H,W] is NCHW exactly as the reference holds them.
 *
 * Environment switches read by the PRODUCT library -- three, all of them change which (deterministic) summation order a GEMM launch takes, none is a
 * measurement knob; they are read once per process (ucod_gemm_reload_tuning re-reads them), never on the launch path:
 *   UCOD_GEMM_NO_PATCH=1       ucod_gemm_bf16*: every output through the tile path.  By default a launch that ends a few tiles past
 *                              one or two whole rounds of CUs computes those tiles as 16x32 patches on the side, which sums K in a
 *                              different order: results stay deterministic but a row's low f32 bits then depend on where the row
 *                              sits in the batch.  Set this for bitwise batch-position independence.
 *   UCOD_GEMM_PATCH_ROUNDS=n   largest number of whole rounds for which the patch mode is considered (default 2).
 *   UCOD_GEMM_NO_MIXED=1       no mixed-height launches (the one-shot large tile with a partly filled last round instead).
 * Measurement knobs (alternative kernel forms, grid sizes, store policies: UCOD_RESIZE_ELEMENTWISE, UCOD_LN_*, UCOD_STATS_STRIPS, UCOD_RESID16_NT,
 * UCOD_LN_FOLD_NO_PARTIALS, UCOD_GEMM_GROUP_M / _COL_FAST / _ST_AUX, UCOD_LORA_GRAD_*, UCOD_DGRAD_F32) exist only in builds made with
 * -DUCOD_LAB_KNOBS (`make -C ucod_dpl_amd/csrc knobs`, used by tools/); libucod_dpl.so / libucod_dpl_f16.so ignore them (csrc/common.h: lab_env).
 */
#ifndef UCOD_DPL_H
#define UCOD_DPL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): ucod_vit_desc gained resid16 (shifts ucod_vit_train_desc), epilogues 9 / 10, ucod_resid16_overflow_*, ucod_gemm_reload_tuning;
 * the experiment variants of ucod_gemm_bf16 / ucod_attention_fwd left the product library.  native.load() refuses any other version. */
/* 3 (round 4): ucod_disc_params gained `nbt`; ucod_step_loss, ucod_disc_bce, the feature-branch discriminator's backward entry points and
 * the assembly attention variants (ucod_attention_fwd variant 64 / 32 / 5) were added. */
/* 4 (round 5): LayerNorm folded into its consumer GEMMs -- epilogues 11 - 14, ucod_gemm_lnfold, ucod_gemm_bf16_stats, ucod_cls_rows_h16_stats,
 * ucod_row_stats_h16, ucod_vit_desc.ln_fold, UCOD_VIT_LAYER_STRIDE 14 -> 16 (two column-sum slots per layer); ucod_zero_segments,
 * ucod_accumulators_prezeroed, the *_multi forms of the Look-Twice crop / paste; the assembly attention variants 64 / 32 of ucod_attention_fwd and the
 * UCOD_ATTN_ASM switch LEFT the product library (laboratory: ucod_attention_fwd_asm_lab of libucod_dpl_variants.so). */
/* 5 (round 6): the row partials of the LayerNorm fold hold (sum, M2 about the slot mean) and are merged with Chan's formula (was: raw sums of squares);
 * the split-operand (f32-equivalent) backbone pass: ucod_split_rows, ucod_layernorm_split, ucod_patch_im2col_split, ucod_qkv_split,
 * ucod_attention_split_fwd, ucod_vit_forward_split (+ their size helpers); ucod_clock_probe; the measurement knobs left the product build (UCOD_LAB_KNOBS). */
/* (still 5) backbone-backward mode on the SwiGLU MLP: epilogues 21 / 22 of ucod_gemm_bf16_train and the _mlp forms of the five training-pass entry points
 * (ucod_vit_train_workspace_bytes_mlp ... ucod_vit_forward_lora_infer_mlp); additions only, nothing existing changed. */
/* (still 5) DINOv2 with registers: ucod_vit_desc gained a trailing n_reg (0 = every caller that zero-fills the descriptor, as the ctypes binding does: the passes
 * are then launch for launch and bit for bit what they were) and the *_reg forms of the row-mapped GEMM drains, the leading-row kernels, the key-gradient scatter and
 * the CLS attention row were added.  ucod_vit_train_desc embeds the descriptor, so its LoRA fields moved by one int; callers build both from this header. */
/* (still 5) DINOv3 (rotary position embedding): ucod_vit_desc gained a trailing `rope` pointer (NULL = every caller that zero-fills the descriptor: the passes are then
 * launch for launch and bit for bit what they were) and ucod_rope_qk was added; the training-pass drivers refuse a non-NULL table. */
/* (still 5) LoRA through DINOv3: ucod_rope_qk_ld (row pitch + direction) was added and ucod_vit_train_desc gained a trailing allow_rope (0 = every caller that
 * zero-fills the descriptor: a table is refused as before); with it set the training-pass drivers rotate q / k forward and dq / dk back. */
/* (still 5) LoRA on the output projections (dense / fc2; o_proj / down_proj): ucod_lora_out_fwd, ucod_lora_out_grad_s, ucod_lora_out_grad_x and the _lora_out forms of
 * the five training-pass entry points were added; the _lora_mlp forms delegate to them with a NULL table and are launch for launch what they were. */
/* (still 5) LoRA on the SwiGLU MLP's output projection (weights_out; the gated down_proj): UCOD_LORA_OUT_ACT_SWIGLU of ucod_lora_out_grad_x_ex and the _lora_out_ex forms
 * of the five training-pass entry points (one word of flags: UCOD_LORA_OUT_SWIGLU) were added; the _lora_out forms delegate to them with flags 0. */
/* (still 5) The MLP hidden in MFMA-fragment order ("BLK16" below): epilogues 23 / 24, ucod_gemm_bf16_blk16a, ucod_gemm_blk16_pair_ok and
 * ucod_vit_forward_blk16 were added; the hidden's workspace slot is sized for 16 ceil(M / 16) rows; nothing existing changed. */
/* (still 5) The deterministic training step ("Deterministic forms" below): the _det forms of ucod_dba_wgrad, ucod_conv_wgrad_f32, ucod_dba_heads_fwd, ucod_dba_bwd,
 * ucod_apm_bce, ucod_disc_fwd and ucod_disc_bwd and their *_det_workspace_bytes helpers were added; additions only, the existing entry points are launch for launch
 * and bit for bit what they were. */
/* (still 5) LoRA bias="lora_only": ucod_colsum_det (+ its size helper), ucod_vit_train_workspace_bytes_lora_bias and ucod_vit_backward_lora_bias (the _lora_out_ex
 * forms plus a bias table) were added; additions only: every older backward / size entry point delegates with a NULL table and is launch for launch what it was. */
/* (still 5) LoRA bias="all": ucod_colsum_det_lora, ucod_colsum_det_tok (+ their size helpers), ucod_vit_train_workspace_bytes_lora_bias_ex and
 * ucod_vit_backward_lora_bias_ex (the _lora_bias forms plus a norm table) were added; additions only: the _lora_bias forms delegate with a NULL table. */
#define UCOD_ABI_VERSION 5
int ucod_abi_version(void);
/* 1 when a gfx950 device is visible to this process (hipGetDeviceProperties().gcnArchName) */
int ucod_device_is_gfx950(void);
/* 16-bit operand type this library was built for: "bf16" (libucod_dpl.so, BASELINE configs[1]) or "f16" (libucod_dpl_f16.so, built with
 * -DUCOD_HALF_F16: IEEE fp16 GEMM / attention operands, the arithmetic of the reference's fp16-autocast launcher,
 * scripts/launch_train_first_stage.sh; every "bf16" in the names and comments below then reads fp16; the backbone-backward entry points
 * (ucod_vit_forward_train, ucod_vit_backward, ucod_gemm_bf16_train, ucod_layernorm_*lora*, ucod_lora_*, ucod_attention_bwd, ...)
 * return UCOD_EINVAL there) */
const char* ucod_half_name(void);

/* Optional per-op timing with HIP events recorded on the launch stream around every launcher below (off by default;
 * bench.py turns it on over its timed region to price each kernel class against its roofline).
 * ucod_prof_collect synchronises the recorded events, fills total_ms[ncls] / count[ncls] and clears the log. */
int ucod_prof_enable(int on);
int ucod_prof_num_classes(void);
const char* ucod_prof_class_name(int cls);
int ucod_prof_collect(double* total_ms_host, long long* count_host);
/* One single-wave launch that stores (s_memtime, s_memrealtime) = (shader-clock cycle counter, constant 100 MHz counter) of the CU it runs on into
 * out_dev[0..1] (two uint64).  Two probes on the same stream bracket a region: (memtime_1 - memtime_0) / (memrealtime_1 - memrealtime_0) * 100 MHz is the
 * mean shader clock the chip HELD over the region (bench.py --sustain-s: the roofline fraction against MFMA rate x held clock). */
int ucod_clock_probe(unsigned long long* out_dev, void* stream);

/* ------------------------------------------------------------------ ViT backbone (rows B1-B8) */

/* GEMM epilogues: C[m][n] = sum_k A[m][k]*B[n][k], A:[M,K] B:[N,K] bf16, K contiguous (y = x W^T) */
enum {
  UCOD_EPI_BIAS_BF16 = 0,            /* out bf16[M,N] = C + bias[n]            QKV: modeling_dinov2.py:199-212, dino.py:103,110 */
  UCOD_EPI_BIAS_GELU_BF16 = 1,       /* out bf16[M,N] = gelu_erf(C + bias[n])  MLP fc1: modeling_dinov2.py:281-297, dino.py:77-93 */
  UCOD_EPI_BIAS_SCALE_RESID_F32 = 2, /* out f32[M,N] = resid + scale[n]*(C+bias[n])  out-proj/fc2 + LayerScale + residual:
                                        modeling_dinov2.py:238-253,272-278,361-381 (scale = ones for DINOv1, dino.py:139-140) */
  UCOD_EPI_PATCH_TOKENS_F32 = 3,     /* A = im2col patches [B*(tok-1),K]; out f32[B*tok,N] rows b*tok+1+p = C + bias[n] + pos[1+p][n]
                                        patch-embed conv + position embedding: modeling_dinov2.py:97-116,139-149, dino.py:144-159,223-235 */
  UCOD_EPI_KEY_NCHW_F32 = 4,         /* A = W_key [C,K], B = tokens [Bimg*tok,K]; out f32[Bimg,C,tok-1] = C + bias[m], CLS dropped:
                                        the key hook, data/utils/feature_extractor.py:42,46-47,55-58 */
  UCOD_EPI_BIAS_F32 = 5,             /* out f32[M,N] = C + bias[n] (final LayerNorm consumers / tests; dgrad GEMMs with bias NULL) */
  /* backbone-backward mode (row B9), ucod_gemm_bf16_train only: */
  UCOD_EPI_GELU_BWD_BF16 = 6,        /* out bf16[M,N] = C * gelu'(aux[m][n]), aux = saved fc1 pre-activation (fc2 dgrad) */
  UCOD_EPI_BIAS_GELU_SAVE_BF16 = 7,  /* out bf16 = gelu_erf(C + bias[n]) and out2 bf16 = C + bias[n] (training-mode fc1) */
  UCOD_EPI_BIAS_SCALE_RESID_H16 = 9, /* as UCOD_EPI_BIAS_SCALE_RESID_F32 with the residual stream kept in IEEE fp16: out f16[M,N] = sat(resid f16 +
                                        scale[n]*(C+bias[n])) (ucod_vit_desc.resid16; `resid` / `out` point at f16 rows).  sat = clamp to
                                        +-65504 (never inf); every clamp is counted: ucod_resid16_overflow_fetch.  Any shape. */
  UCOD_EPI_PATCH_TOKENS_H16 = 10,    /* as UCOD_EPI_PATCH_TOKENS_F32 with f16 token rows (same saturation) */
  UCOD_EPI_LNFOLD_BIAS_BF16 = 11,    /* ucod_gemm_lnfold only.  LayerNorm folded into the QKV projection (modeling_dinov2.py:348-353,199-212: norm1 -> query / key /
                                        value): A = the fp16 residual stream x itself, B = fp16(gamma (.) W), colsum[n] = sum_k B[n][k], bias = W beta + b,
                                        stats[m] = (rstd, -mean * rstd) of row m:  out 16-bit [M,N] = (stats[m][0] * C + stats[m][1] * colsum[n] + bias[n]) * scale[n] */
  UCOD_EPI_LNFOLD_GELU_BF16 = 12,    /* ucod_gemm_lnfold only.  The same fold for norm2 -> fc1 -> GELU (modeling_dinov2.py:365-373,281-297):
                                        out = gelu_erf(stats[m][0] * C + stats[m][1] * colsum[n] + bias[n]) */
  UCOD_EPI_BIAS_SCALE_RESID_H16_STATS = 13, /* ucod_gemm_bf16_stats only.  UCOD_EPI_BIAS_SCALE_RESID_H16 that also leaves, per output row and 64-column slot, the
                                        (sum S, M2 = sum of squared deviations from the slot's own mean S / 64) of the fp16 values it has just written:
                                        row_partials f32 [M][N/64][2].  The next ucod_gemm_lnfold merges a row's slots in its prologue (Chan's parallel-variance
                                        formula: nothing cancels, whatever |mean| / sigma) instead of reading `stats`: no statistics launch.  Large passes only
                                        (M >= 2048, N % 64 == 0); otherwise UCOD_EINVAL and nothing is launched */
  UCOD_EPI_PATCH_TOKENS_H16_STATS = 14,     /* ucod_gemm_bf16_stats only.  UCOD_EPI_PATCH_TOKENS_H16 with the same partials, indexed by OUTPUT token row (the CLS rows'
                                        partials come from ucod_cls_rows_h16_stats) */
  UCOD_EPI_BIAS_GELU_SPLIT2 = 15,    /* split-operand pass, two terms (csrc/split.hip): out bf16 [M, 3 N] = the A-side split operand (segments hi | hi | lo) of
                                        gelu_erf(C + bias[n]) -- fc1 + GELU + the split in ONE launch instead of UCOD_EPI_BIAS_F32 + ucod_split_rows(op 1): no f32
                                        round trip of the MLP hidden.  bf16 library; N % 8 == 0 */
  UCOD_EPI_BIAS_SWIGLU_BF16 = 16,    /* DINOv2 ViT-g MLP (Dinov2SwiGLUFFN, modeling_dinov2.py:300-315: hidden = silu(x1) * x2, (x1, x2) = weights_in(x).chunk(2)).
                                        B = weights_in with its rows INTERLEAVED in blocks of 4 (ucod_dpl_amd/swiglu.py): GEMM column 8k+e (e < 4) holds x1 unit 4k+e,
                                        column 8k+4+e holds x2 unit 4k+e.  out 16-bit [M, N/2] = silu(C+bias)[8k+e] * (C+bias)[8k+4+e] at column 4k+e; every
                                        pair sits inside one 8-column chunk of a tile, so nothing crosses a tile.  silu(x) = x / (1 + exp(-x)); -0 for x -> -inf,
                                        NaN propagates.  N % 8 == 0.  Both libraries */
  UCOD_EPI_LNFOLD_SWIGLU_BF16 = 17,  /* ucod_gemm_lnfold only.  The LayerNorm fold of UCOD_EPI_LNFOLD_GELU_BF16 (norm2 -> weights_in, modeling_dinov2.py:365-373,300-315),
                                        then the SwiGLU of UCOD_EPI_BIAS_SWIGLU_BF16: out fp16 [M, N/2] */
  UCOD_EPI_BIAS_SWIGLU_SPLIT2 = 18,  /* split-operand pass, two terms: out bf16 [M, 3 N/2] = the A-side split operand (segments hi | hi | lo, N/2 apart) of the SwiGLU
                                        of UCOD_EPI_BIAS_SWIGLU_BF16 (modeling_dinov2.py:300-315), SiLU to f32 accuracy.  bf16 library; N % 8 == 0 */
  UCOD_EPI_BIAS_GELU_SPLIT16 = 19,   /* ucod_split16_gemm_act only (ucod_gemm_bf16 refuses it).  fp16-term split pass: out fp16 [M, 3 N] = the A-side split operand
                                        (hi | hi | lo) of scale * gelu_exact(alpha * (C + bias[n])), saturation counted.  libucod_dpl_f16.so; N % 8 == 0 */
  UCOD_EPI_BIAS_SWIGLU_SPLIT16 = 20, /* ucod_split16_gemm_act only.  The same for the SwiGLU of UCOD_EPI_BIAS_SWIGLU_BF16's column layout, SiLU to f32 accuracy: out fp16
                                        [M, 3 N/2], segments N/2 apart */
  /* backbone-backward mode on the SwiGLU MLP (DINOv2 ViT-g/14, Dinov2SwiGLUFFN, modeling_dinov2.py:300-315), ucod_gemm_bf16_train only, bf16 library, large-tile
     kernels; N % 8 == 0, K >= 128, every row set within 31-bit byte offsets (M * 2 N(hidden) * 2 < 2^31): */
  UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 = 21, /* training-mode weights_in (B interleaved as for UCOD_EPI_BIAS_SWIGLU_BF16, N = 2 F): out bf16 [M, N/2] = exactly what
                                        UCOD_EPI_BIAS_SWIGLU_BF16 writes for the same variant (same silu, bias added where that launch adds it), and out2 bf16 [M, N] =
                                        C + bias[n] in the interleaved column order: the saved pre-activation (x1 | x2 of modeling_dinov2.py:311-312) */
  UCOD_EPI_SWIGLU_BWD_BF16 = 22,     /* weights_out dgrad (B = weights_out^T [N = F, K]): with g = C[m][4k+e] the cotangent of hidden unit 4k+e (modeling_dinov2.py:313-314
                                        differentiated), x1 = aux[m][8k+e], x2 = aux[m][8k+4+e] (aux = the saved pre-activation, bf16 [M, 2N]) and sig = 1/(1+exp(-x1)):
                                        out bf16 [M, 2N]:  out[m][8k+e] = g x2 sig (1 + x1 (1 - sig)),  out[m][8k+4+e] = g x1 sig  -- the cotangent of the interleaved
                                        weights_in output; f32 arithmetic, one bf16 rounding.  A lane's 8 GEMM columns drain into 32 contiguous bytes: no row of
                                        weights_out^T is duplicated */
  /* fc1 + GELU with the hidden in BLK16 (MFMA-fragment) order, the A operand of ucod_gemm_bf16_blk16a -- see "BLK16" below.  Large-tile kernels only (variant 0, 9 or
   * 13; N % 64 == 0, K >= 128, 16 ceil(M / 16) N 2 < 2^31); anything else is UCOD_EINVAL and the caller runs the row-major pair.  Every stored value is bit for bit
   * what the row-major epilogue of the same variant stores. */
  UCOD_EPI_LNFOLD_GELU_BLK16 = 23,   /* ucod_gemm_lnfold only: UCOD_EPI_LNFOLD_GELU_BF16, out 16-bit [16 ceil(M / 16), N] in BLK16 order */
  UCOD_EPI_BIAS_GELU_BLK16 = 24,     /* ucod_gemm_bf16: UCOD_EPI_BIAS_GELU_BF16, out 16-bit [16 ceil(M / 16), N] in BLK16 order */
  UCOD_EPI_QKV_FP8 = 8               /* QKV projection of the fp8 attention path (BASELINE configs[4]): out = e4m3 bytes
                                        [3 (q|k|v)][Bimg*heads][Npad][64], Npad = tokens rounded up to 64, value = clamp((C + bias[n]) *
                                        scale[n], +-448); N = 3*heads*64, M = Bimg*tokens_per_image; large-tile kernel only */
};
/* variant: 0 = auto, 1 = 128x128 register staging, 2 = 128x128 LDS-DMA, 12 = 64x64 tile with LDS-DMA (what auto picks when there are
 * fewer 128x128 tiles than CUs: batch-1 passes), 9 / 10 = 256x256 / 256x192 large tile (LDS-DMA in flight across barriers, staggered
 * wave groups, two barrier intervals per K-tile, leftover tiles as patches: what auto picks for one- and two-round launches),
 * 13 / 14 = the same loop with mixed-height tiles (whole rounds: what auto picks for three and more rounds).  3-8 (four intervals,
 * no stagger, persistent form) are laboratory variants: ucod_gemm_bf16_lab of libucod_dpl_variants.so (`make variants`), refused here.
 * Large-tile variants need N % 4 == 0 (N % 8 == 0 for bf16 output).  K % 64 == 0.  For UCOD_EPI_BIAS_BF16 a non-NULL `scale` [N] multiplies
 * (C + bias) per column before the bf16 rounding (used to fold the softmax scale into Q). */
int ucod_gemm_bf16(int epilogue, const void* A_bf16, const void* B_bf16, void* out, int M, int N, int K,
                   const float* bias, const float* scale, const float* resid, const float* pos,
                   int tokens_per_image, int variant, void* stream);
/* The two row-mapped drains for a checkpoint with register tokens (DINOv2 with registers, modeling_dinov2_with_registers.py): an image's tokens are
 * [CLS | n_reg registers | n patches], tokens_per_image = 1 + n_reg + n counts all of them (n_reg is NEVER packed into it).
 *   UCOD_EPI_PATCH_TOKENS_F32 / _H16: GEMM row b n + p -> token row b tok + 1 + n_reg + p, + pos row 1 + p (`pos` has 1 + n rows: registers have none); the
 *     CLS and register rows of `out` are not touched (ucod_cls_rows_reg writes them);
 *   UCOD_EPI_KEY_NCHW_F32: token column t of an image -> key-map column t - 1 - n_reg; CLS and register columns are dropped; out f32 [B, C, n].
 * Every output bound is formed from n.  Any other epilogue is parameterised by rows alone and is accepted with n_reg = 0 only, where this IS ucod_gemm_bf16. */
int ucod_gemm_bf16_reg(int epilogue, const void* A_bf16, const void* B_bf16, void* out, int M, int N, int K,
                       const float* bias, const float* scale, const float* resid, const float* pos,
                       int tokens_per_image, int n_reg, int variant, void* stream);
/* BLK16: an activation [M, F] of 16-bit values, F % 64 == 0, stored as the A operands of v_mfma_f32_16x16x32 instead of row-major, so that the producer (fc1) stores
 * its accumulators straight from registers and the consumer (fc2) copies whole operands into LDS.  Rows are padded to Mp = 16 ceil(M / 16); the buffer holds Mp F values.
 *   chunk (m, s, g): token row m, k-step s = 0 .. F/32 - 1, g = 0 .. 3: 16 bytes at byte offset  (((m / 16) (F / 32) + s) 64 + g 16 + (m % 16)) 16;
 *   element e = 0 .. 7 of the chunk is hidden unit  pi(32 s + 8 g + e) = 32 s + 16 (e >> 2) + 4 g + (e & 3).
 * One (m / 16, s) block is 1 KB in lane order (lane = 16 g + m % 16): one complete MFMA A operand.  pi permutes each group of 32 hidden units; the consumer's weight
 * carries the same permutation on its K axis, W'[n][k] = W[n][pi(k)] (a dot product does not depend on the order of k).  Rows M .. Mp - 1 of the last block are
 * UNSPECIFIED: they feed only output rows that are never stored, and the consumer keeps them out of its saturation test.
 * ucod_gemm_bf16_blk16a: UCOD_EPI_BIAS_SCALE_RESID_H16 (row_partials NULL, nslot 0) or UCOD_EPI_BIAS_SCALE_RESID_H16_STATS with A in BLK16 order [Mp, K] and B = W'.
 * M >= 2048, K >= 128, K % 64 == 0, N % 8 == 0 (STATS: N % 64 == 0), Mp K 2 < 2^31; UCOD_EINVAL otherwise.  Results differ from the row-major launch only by the order
 * of the f32 additions over K. */
int ucod_gemm_bf16_blk16a(int epilogue, const void* A_blk16, const void* B_perm, void* out, int M, int N, int K, const float* bias, const float* scale,
                          const void* resid, float* row_partials, int nslot, void* stream);
/* 1 when a BLK16 fc1 (N = F, K = D) and ucod_gemm_bf16_blk16a (N = D, K = F) on M rows both take a large-tile kernel for this ucod_gemm_bf16 variant, else 0 */
int ucod_gemm_blk16_pair_ok(int M, int F, int D, int gemm_variant);

/* LayerNorm folded into its consumer GEMM (epilogues UCOD_EPI_LNFOLD_*; libucod_dpl_f16.so only -- an MFMA takes both operands in one type and
 * the A operand here is the IEEE fp16 residual stream itself; the bf16 build returns UCOD_EINVAL).  Replaces nn.LayerNorm + nn.Linear of
 * modeling_dinov2.py:348-381 (norm1 -> attention, norm2 -> mlp) and dino.py:127-131:
 *   LN(x) W^T + b = rstd[m] * (x W'^T - mean[m] * colsum[n]) + bias'[n],   W' = fp16(gamma (.) W),  colsum[n] = sum_k W'[n][k] (of the ROUNDED
 *   W', so that the subtraction cancels what the MFMA summed),  bias' = W beta + b.
 * x_f16 [M,K] fp16, w_folded [N,K] fp16, colsum / bias_folded f32 [N], stats f32 [M][2] = (rstd, -mean * rstd) per row (ucod_row_stats_h16),
 * scale: optional column scale (UCOD_EPI_LNFOLD_BIAS_BF16 only), out fp16 [M,N].  N % 8 == 0, K % 64 == 0.  variant as ucod_gemm_bf16
 * (the 192-wide forms 10 / 14 are taken as 9 / 13). */
int ucod_gemm_lnfold(int epilogue, const void* x_f16, const void* w_folded, void* out, int M, int N, int K, const float* bias_folded,
                     const float* colsum, const float* stats, const float* row_partials, int nslot, float eps, const float* scale,
                     int variant, void* stream);
/* `stats` may be NULL when `row_partials` f32 [M][nslot][2] is given (nslot = K / 64, even, <= 24): per 64-column slot (S_i, M2_i) = (sum, sum of squared
 * deviations from S_i / 64) of x's row, left by the producer of x (ucod_gemm_bf16_stats / ucod_cls_rows_h16_stats); the kernel's prologue forms
 *   mean = sum_i S_i / K,  var = (sum_i M2_i + 64 sum_i (S_i / 64 - mean)^2) / K,  rstd = rsqrt(var + eps)   in f32
 * (ABI 5; ABI 4 stored raw sums of squares and formed E[x^2] - mean^2, which lost the variance of rows with |mean| >> sigma).  Same value as
 * ucod_row_stats_h16's two-pass form to f32 rounding.  The large-tile kernels only (a small shape is then run on them too). */
/* The producers of the fp16 residual stream with row partials (epilogues UCOD_EPI_*_STATS; arguments as ucod_gemm_bf16; `resid` / `out` f16 rows;
 * nslot = N / 64).  UCOD_EINVAL (nothing launched) for shapes the large-tile kernels do not take: use the plain epilogue and ucod_row_stats_h16 then. */
int ucod_gemm_bf16_stats(int epilogue, const void* A_bf16, const void* B_bf16, void* out, int M, int N, int K, const float* bias, const float* scale,
                         const void* resid_f16, const float* pos, int tokens_per_image, float* row_partials, int nslot, void* stream);
/* ucod_cls_rows_h16 that also writes the CLS rows' partials, slot by slot like the other rows' (nslot = D / 64) */
int ucod_cls_rows_h16_stats(void* x_f16, const float* cls, const float* pos, float* row_partials, int nslot, int B, int tok, int D, void* stream);
/* the same with register tokens: UCOD_EPI_PATCH_TOKENS_H16_STATS as in ucod_gemm_bf16_reg (the residual producer takes n_reg = 0 only: it has no row map), and the
 * leading rows -- CLS and the n_reg register rows of every image -- with their (S, M2) partials (cls_reg as in ucod_cls_rows_reg) */
int ucod_gemm_bf16_stats_reg(int epilogue, const void* A_bf16, const void* B_bf16, void* out, int M, int N, int K, const float* bias, const float* scale,
                             const void* resid_f16, const float* pos, int tokens_per_image, int n_reg, float* row_partials, int nslot, void* stream);
int ucod_cls_rows_h16_stats_reg(void* x_f16, const float* cls_reg, const float* pos, float* row_partials, int nslot, int B, int tok, int D, int n_reg, void* stream);
/* Row statistics of the fp16 residual stream for the folded epilogues: stats[m] = (rstd, -mean * rstd), two-pass in f32 over the row held in
 * registers, biased variance + eps like nn.LayerNorm.  x f16 [rows,D], D % 256 == 0, D <= 1536.
 * Range of the fold: x W'^T and mean * colsum cancel in f32, which costs ~2^-24 sqrt(K) |mean| / sigma of the output scale (0.2 fp16 ulp at 100 sigma).  Both
 * statistics paths (this kernel and the prologue of ucod_gemm_lnfold on row partials) COUNT every row with |mean| > 256 sigma into the saturation counter of the
 * fp16 stream (ucod_resid16_overflow_*): such a checkpoint is reported by ViTEngine.check_overflow, never folded silently; use ln_fold = 0 for it. */
int ucod_row_stats_h16(const void* x_f16, float* stats, int rows, int D, float eps, void* stream);
/* The UCOD_GEMM_* tuning variables (csrc/gemm_bf16_plan.h) are read once per process; this re-reads them (tests, sweep tools). */
void ucod_gemm_reload_tuning(void);

/* Saturation counter of the f16 residual stream (one word per device): how many wave-lanes had to clamp a value of x to +-65504 since the
 * last reset.  fetch = asynchronous 4-byte copy into (pinned) host memory on `stream`; the caller orders its own read behind it (event /
 * stream sync).  A non-zero count means the f16 stream cannot hold this checkpoint's activations: use resid16 = 0 (ViTEngine(resid="f32")). */
int ucod_resid16_overflow_fetch(unsigned* host_dst, void* stream);
int ucod_resid16_overflow_reset(void* stream);
/* A counter of the caller's own (round 4): the launches issued NEXT FROM THIS HOST THREAD count into `device_counter` (one zero-initialised
 * device word, e.g. one per engine) instead of the per-device word, and fetch / reset act on it; NULL restores the per-device word.  The
 * binding is host-side state read at launch time: bind, issue the pass, unbind. */
int ucod_resid16_overflow_bind(unsigned* device_counter);

/* nn.LayerNorm over the last dim (modeling_dinov2.py:348,353,365,373,441; dino.py:127,131,184):
 * x f32 [rows,D] -> y bf16 [rows,D] (or f32 when out_f32 != 0).  D % 128 == 0. */
/* (register tokens: a row kernel over `rows` = B tok rows; tok = 1 + n_reg + n needs nothing here) */
int ucod_layernorm(const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps,
                   int out_f32, void* stream);
/* the same with the residual stream in IEEE fp16 (ucod_vit_desc.resid16): x f16 [rows,D] -> y bf16 [rows,D]; statistics in f32 */
int ucod_layernorm_h16(const void* x_f16, const float* gamma, const float* beta, void* y, int rows, int D, float eps, void* stream);

/* softmax(Q K^T * scale) V per (image, head), head_dim 64 (modeling_dinov2.py:153-179; dino.py:113-117).
 * qkv bf16 [B*tok, 3*heads*64] rows = [q | k | v], heads contiguous; out bf16 [B*tok, heads*64].
 * scale != 0: the generic kernel (Q as the reference holds it, the scale applied inside the softmax, running max per tile).
 * scale == 0 declares that Q already carries head_dim^-0.5 * log2(e) (ucod_fill_qscale + the QKV epilogue scale do that inside
 * ucod_vit_forward) and selects the product kernel: K/V by buffer loads to LDS, -m as the score accumulator's initial value, deferred
 * max, probabilities fed back as MFMA operands from registers, f32 row sums, 16-byte output stores; query rows and 32-key blocks past
 * the last token are not computed.  variant: 0 or 2 (the same kernels), 5 / 66 = attn_fwd_v5_kernel / attn_fwd_v6_kernel by name; every other number is a laboratory variant
 * (ucod_attention_fwd_lab of libucod_dpl_variants.so) and is refused.  tok * heads * 384 must fit 32 bits. */
/* (register tokens: parameterised by `tok` alone -- registers are ordinary tokens of the sequence, tok = 1 + n_reg + n; unchanged) */
int ucod_attention_fwd(const void* qkv_bf16, void* out_bf16, int B, int tok, int heads, float scale, int variant,
                       void* stream);

/* The same attention with Q, K, V and the probabilities quantised to OCP e4m3 and both products on the block-scaled CDNA4 matrix
 * instruction v_mfma_scale_f32_32x32x64_f8f6f4 (BASELINE.json configs[4], the "fp8 attention path"; same reference lines as above).
 * qkv is the QKV projection's 16-bit output with Q pre-scaled by head_dim^-0.5 * log2(e) (as for scale == 0 above).  A first kernel
 * writes Q8 / K8 [B*heads][Npad][64] and the per-tile transposed Vt8 into `workspace` (ucod_attention_fp8_workspace_bytes), each
 * tensor multiplied by 2^q_exp / 2^k_exp / 2^v_exp before rounding (clamped to +-448); the inverse powers of two ride on the
 * instruction's E8M0 block scales.  ucod_vit_forward takes this path for attn_variant == 8 with (q_exp, k_exp, v_exp) = (5, 3, 3).
 * Tolerance (tests/test_gpu_fp8_attention.py): exact on e4m3-representable inputs; relative L2 <= 1e-1 against the f32 softmax
 * attention on Gaussian inputs (7.2e-2 measured: the error of a 64-term e4m3 score in the exponent). */
size_t ucod_attention_fp8_workspace_bytes(int B, int tok, int heads);
/* Fused form: `q8k8v8` is what ucod_gemm_bf16(UCOD_EPI_QKV_FP8, ...) wrote (column scales 2^q_exp * head_dim^-0.5 * log2 e, 2^k_exp,
 * 2^v_exp folded into its `scale` vector), V row-major like K and transposed on the fly by ds_read_b64_tr_b8: no conversion pass and
 * half the QKV output bytes.  ucod_attention_fp8_zero_pad clears the rows tokens..Npad-1 of all three tensors (once per workspace:
 * nothing writes them afterwards; a NaN byte there would survive the multiplication by a zero probability). */
int ucod_attention_fp8_zero_pad(void* q8k8v8, int B, int tok, int heads, void* stream);
/* (register tokens: parameterised by `tok` alone; unchanged) */
int ucod_attention_fwd_fp8_fused(const void* q8k8v8, void* out_bf16, int B, int tok, int heads, int q_exp, int k_exp, int v_exp, void* stream);
int ucod_attention_fwd_fp8(const void* qkv_bf16, void* out_bf16, void* workspace, size_t workspace_bytes, int B, int tok, int heads,
                           int q_exp, int k_exp, int v_exp, void* stream);

/* patch gather: img f32 [B,C,H,W] -> bf16 rows [B*(H/P)*(W/P), Kpad], k = c*P*P + py*P + px, zero padded
 * (the im2col view of the stride-P conv, modeling_dinov2.py:139-149 / dino.py:154-158).  Kpad % 64 == 0. */
int ucod_patch_im2col(const float* img, void* patches_bf16, int B, int C, int H, int W, int P, int Kpad, void* stream);

/* x f32 [B*tok, D]: row b*tok = cls + pos[0]  (modeling_dinov2.py:107-112; dino.py:227-232) */
int ucod_cls_rows(float* x, const float* cls, const float* pos, int B, int tok, int D, void* stream);
int ucod_cls_rows_h16(void* x_f16, const float* cls, const float* pos, int B, int tok, int D, void* stream);
/* the leading rows of an image with register tokens (Dinov2WithRegistersEmbeddings.forward): row b*tok = cls_reg[0] + pos[0], rows b*tok + 1 .. + n_reg =
 * cls_reg[1 .. n_reg] as they are (a register token has no position row).  cls_reg f32 [(1 + n_reg), D]: the CLS row followed by the register rows (table slot +2);
 * tok = 1 + n_reg + n.  n_reg = 0 is ucod_cls_rows / ucod_cls_rows_h16. */
int ucod_cls_rows_reg(float* x, const float* cls_reg, const float* pos, int B, int tok, int D, int n_reg, void* stream);
int ucod_cls_rows_h16_reg(void* x_f16, const float* cls_reg, const float* pos, int B, int tok, int D, int n_reg, void* stream);

/* v[0..D) = c, v[D..3D) = 1: the per-column factor of the fused QKV epilogue */
int ucod_fill_qscale(float* v, int D, float c, void* stream);
/* v[3*D] = cq for the q columns, ck for k, cv for v: the column scales of UCOD_EPI_QKV_FP8 (pre-scale and power-of-two range scales) */
int ucod_fill_qscale3(float* v, int D, float cq, float ck, float cv, void* stream);

/* f32 -> bf16 cast of n elements (weight preparation) */
int ucod_cast_f32_bf16(const float* src, void* dst_bf16, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backbone-backward mode.  The reference describes it in models/modules/full_model.py:47-72,79-126
 * (peft LoRA r=2, lora_alpha=4 on query/key/value of every encoder layer, all other weights frozen, key hook of the
 * last layer feeds the decoder); that file is not importable, so parity is pinned on HuggingFace Dinov2Model autograd
 * with the LoRA forward restated (tests/golden/g12_lora_backbone.npz).  LoRA rides on the GEMMs as UCOD_LORA_AUG
 * extra K columns -- see ucod_dpl_amd/csrc/vit_train.hip for the operand formats.
 * One layer's LoRA parameters / gradients (f32): [A_q (r x D) | B_q (D x r) | A_k | B_k | A_v | B_v], 3r <= UCOD_LORA_AUG. */
#define UCOD_LORA_AUG 64

/* ucod_gemm_bf16 with the training epilogues 6 / 7 (GELU) and 21 / 22 (SwiGLU) (large-tile kernels; N % 8 == 0, K >= 128; 21 / 22 take variant 0 / 1 / 2 (= auto
 * among the large tiles), 9, 10, 13, 14 and refuse the others).  For UCOD_EPI_BIAS_BF16 and
 * UCOD_EPI_BIAS_F32 (either entry point) a NULL bias means a plain product (K >= 128, N % 4 == 0, variant not 1/2/12). */
int ucod_gemm_bf16_train(int epilogue, const void* A, const void* B, void* out, int M, int N, int K, const float* bias,
                         const void* aux_bf16, void* out2_bf16, int variant, void* stream);

/* LoRA dropout (LoraConfig.lora_dropout, full_model.py:50: nn.Dropout on the input of every lora_A, an independent mask per target
 * module).  Counter-based (ABI 3: one mix per element for the three projections): with
 *   h = seed_lo ^ (idx * 0x9E3779B1);  h ^= seed_hi + layer * 0x85EBCA77;  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;
 *   h *= 0x846CA68B;  h ^= h >> 16;      (32-bit wrap-around arithmetic, idx = row * D + col)
 * element (row, col) of projection p (0 q, 1 k, 2 v) in `layer` is dropped iff  (h >> (10 * p)) & 1023  <  T,  T = floor(p_drop * 1024);
 * kept elements are scaled by 1 / (1 - T / 1024) (the effective drop probability is T / 1024).  Forward and backward regenerate the
 * mask; nothing is stored.
 * Pass NULL (or p == 0) for no dropout. */
typedef struct {
  float p;
  unsigned long long seed;   /* change it every step */
  int layer;
} ucod_lora_dropout;

/* y_aug bf16 [rows, D+64] = [ LayerNorm(x) | dropout_q(LN(x)) A_q^T, dropout_k(LN(x)) A_k^T, dropout_v(LN(x)) A_v^T (3r values) | 0 ]
 * Limit on (D, r): the kernel keeps the layer's 3 r rows of A in one workgroup's LDS, 3 * r * D * 4 bytes, which must fit what the device gives one
 * workgroup (queried once; 160 KiB on gfx950: r <= 17 at D = 768, r <= 13 at 1024, r <= 8 at 1536).  Past 64 KiB the launch asks for the larger
 * allocation itself.  A (D, r) that does not fit returns UCOD_EINVAL before any launch; ucod_layernorm_lora_fits(D, r, 3) tells beforehand
 * (modules = 3: q / k / v, 1: the MLP input projection; 1 = fits, 0 = refused or invalid), and the training passes refuse such a descriptor. */
int ucod_layernorm_lora_fits(int D, int r, int modules);
int ucod_layernorm_lora(const float* x, const float* gamma, const float* beta, const float* lora_layer, int r, void* y_aug_bf16,
                        int rows, int D, float eps, const ucod_lora_dropout* dropout, void* stream);
/* the same from an IEEE fp16 residual stream (the no-grad LoRA pass with vit.resid16) */
int ucod_layernorm_lora_h16(const void* x_f16, const float* gamma, const float* beta, const float* lora_layer, int r, void* y_aug_bf16,
                            int rows, int D, float eps, const ucod_lora_dropout* dropout, void* stream);

/* LayerNorm backward w.r.t. its input (frozen gamma/beta), fused with the residual add and the next GEMM's A operand:
 * dx f32 [rows,D] = dres (nullable) + dLN(dy; x, gamma);  s bf16 [rows,D] = next_scale (nullable: ones) * dx.
 * dx may alias dres or dy; either output may be NULL. */
int ucod_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* dres, const float* next_scale, float* dx,
                       void* s_bf16, int rows, int D, float eps, void* stream);
/* The same with the dropout-masked LoRA branch added to dy first:  dy += sum_p mask_p/(1-p) * (t_p A_p),  t = aug columns of
 * dqkv_aug [rows, 3D+64].  Used for LayerNorm-1 when dropout is on (the A^T columns of WqkvT_aug are then zero, ucod_lora_pack). */
int ucod_layernorm_bwd_lora(const float* dy, const float* x, const float* gamma, const float* dres, const float* next_scale, float* dx,
                            void* s_bf16, int rows, int D, float eps, const void* dqkv_aug_bf16, const float* lora_layer, int r,
                            const ucod_lora_dropout* dropout, void* stream);
/* Both with 16-bit inputs (round 4): flags & UCOD_LNB_DY_BF16: dy is bf16 [rows,D] (what ucod_vit_backward's dgrad GEMMs write: half the bytes on the
 * GEMM's store-bound drain and on this kernel's read side; the upstream gradient is rounded to 8 mantissa bits once, the residual cotangent
 * stream dx stays f32); flags & UCOD_LNB_X_F16 (only together with DY_BF16): x is IEEE fp16 (the saved residual stream of a training pass
 * with vit.resid16).  flags = 0: the two functions above. */
#define UCOD_LNB_DY_BF16 1
#define UCOD_LNB_X_F16 2
int ucod_layernorm_bwd_ex(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                          void* s_bf16, int rows, int D, float eps, void* stream);
int ucod_layernorm_bwd_lora_ex(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                               void* s_bf16, int rows, int D, float eps, const void* dqkv_aug_bf16, const float* lora_layer, int r,
                               const ucod_lora_dropout* dropout, void* stream);

/* Attention forward that also returns the base-2 log-sum-exp of the scaled scores, lse f32 [B, heads, tok]
 * (Q must carry head_dim^-0.5 * log2(e), as for ucod_attention_fwd with scale == 0). */
/* (register tokens: ucod_attention_fwd_lse / ucod_attention_bwd take `tok` = 1 + n_reg + n like any other token count; unchanged) */
int ucod_attention_fwd_lse(const void* qkv_bf16, void* out_bf16, float* lse, int B, int tok, int heads, void* stream);

/* Attention backward (eager_attention_forward of modeling_dinov2.py:153-179 differentiated): qkv as in the forward
 * (Q pre-scaled), out/dout bf16 [B*tok, D], lse from ucod_attention_fwd_lse; delta f32 [B, heads, tok] is scratch.
 * dqkv bf16 rows of length ld_dqkv (>= 3D) = gradient w.r.t. the UNSCALED q | k | v projections. */
int ucod_attention_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse, float* delta,
                       void* dqkv_bf16, int ld_dqkv, int B, int tok, int heads, void* stream);

/* dkey f32 [B, D, tok-1] (cotangent of the key hook) -> rows of dqkv_aug bf16 [B*tok, 3D+64]: k third = dkey^T (CLS row 0),
 * q and v thirds and the aug columns zero. */
int ucod_key_grad_tokens(const float* dkey, void* dqkv_aug_bf16, int B, int tok, int D, void* stream);
/* the same for tok = 1 + n_reg + n tokens per image: dkey f32 [B, D, n] goes to the K third of token rows 1 + n_reg .. tok - 1; the CLS row and the n_reg register
 * rows, which the key hook drops, get zeros there like the q / v thirds */
int ucod_key_grad_tokens_reg(const float* dkey, void* dqkv_aug_bf16, int B, int tok, int D, int n_reg, void* stream);

/* Fill the aug columns of Wqkv_aug bf16 [3D, D+64] (alpha/r * B_q|B_k|B_v on the block diagonal) and of WqkvT_aug bf16
 * [D, 3D+64] (A_q^T|A_k^T|A_v^T; zeros when zero_a_columns != 0, the dropout case) from one layer's LoRA parameters.  Either
 * matrix may be NULL. */
int ucod_lora_pack(const float* lora_layer, int r, float scaling, void* w_aug_bf16, void* wt_aug_bf16, int D, int zero_a_columns,
                   void* stream);

/* One layer's LoRA gradients from dqkv_aug [rows, 3D+64] and h_aug [rows, D+64]; also writes t = alpha/r * dqkv B into the
 * aug columns of dqkv_aug (consumed by the dgrad GEMM).  grad_layer has the parameter layout; accumulate != 0 adds. */
size_t ucod_lora_grad_workspace_bytes(int D);
/* (register tokens: the LoRA row kernels -- ucod_layernorm_lora*, ucod_lora_grad, ucod_layernorm_bwd*, the _lora_mlp forms -- work on M = B tok rows; unchanged) */
int ucod_lora_grad(void* dqkv_aug_bf16, const void* h_aug_bf16, const float* lora_layer, int r, float scaling, float* grad_layer,
                   int accumulate, void* workspace, size_t workspace_bytes, int rows, int D, const ucod_lora_dropout* dropout, void* stream);

/* Whole frozen backbone forward up to the last layer's key projection: one call enqueues every kernel.
 * Pointer table (HOST array of DEVICE pointers; "w" entries are bf16 [out,in], the rest f32):
 *   [0] patch_w bf16 [D,Kpad] (zero padded k)  [1] patch_b [D]  [2] cls [D]  [3] pos [tok,D] (already interpolated)
 *   layer l at base = 4 + UCOD_VIT_LAYER_STRIDE*l:
 *     +0 ln1_g  +1 ln1_b  +2 qkv_w bf16 [3D,D] (rows q|k|v)  +3 qkv_b [3D]  +4 proj_w bf16 [D,D]  +5 proj_b
 *     +6 ls1 [D] (LayerScale lambda1; ones for DINOv1)  +7 ln2_g  +8 ln2_b  +9 fc1_w bf16 [F,D]  +10 fc1_b [F]
 *     +11 fc2_w bf16 [D,F]  +12 fc2_b [D]  +13 ls2 [D]
 *     +14 qkv_colsum [3D]  +15 fc1_colsum [F]   (ln_fold only, else unused: with ln_fold the entries +2 / +3 / +9 / +10 of every layer BUT THE LAST
 *     of the pass hold the folded forms fp16(gamma (.) W) and W beta + b, and +14 / +15 the column sums of the folded weights; for
 *     attn_variant != 1 the Q rows of the folded qkv entries are also multiplied by head_dim^-0.5 * log2(e), the pre-scale the unfolded
 *     pass applies as a column scale; the last layer keeps plain weights -- its LayerNorm 1 runs as a kernel and feeds the key hook)
 * The last layer uses only ln1 and the K slice (rows D..2D-1) of qkv_w / qkv_b: that projection, bias included and
 * before the head split, is what the reference's forward hook captures (feature_extractor.py:42,46-47).
 * key_out f32 [B, D, H/P, W/P].  full_last_layer != 0 additionally runs the rest of the last layer exactly as the
 * reference does (its output is discarded there too); key_out is identical either way. */
#define UCOD_VIT_LAYER_STRIDE 16
typedef struct {
  int B, C, H, W, P;      /* images */
  int D, heads, F, L;     /* width, heads (head_dim = D/heads = 64), MLP width, layers */
  int Kpad;               /* padded C*P*P */
  float eps;              /* LayerNorm eps (1e-6 for DINOv2 / DINO) */
  int full_last_layer;
  int gemm_variant;       /* ucod_gemm_bf16's variant for every GEMM of the pass (0 = auto) */
  int attn_variant;       /* 0 (auto) / 2: pre-scaled-Q product kernel; 1: generic-scale kernel; 8: the fp8 path of BASELINE configs[4]; 5 / 66: the
                             two pre-scaled-Q kernels by name; anything else is refused (UCOD_EINVAL) */
  int resid16;            /* 1: the residual stream x lives in IEEE fp16 instead of f32 (11 significand bits: 8x finer than the bf16 GEMM
                             operands it feeds, so the bf16 build's accuracy is unchanged to its own rounding).  Halves the bytes of
                             LayerNorm's read and of the out-proj / fc2 read-modify-write epilogues.  Values saturate at +-65504 and every
                             saturation is counted (ucod_resid16_overflow_fetch): a checkpoint whose residual stream exceeds fp16's range
                             is reported, never silently turned into inf / NaN.  0: f32 (exact accumulation; what the reference holds).
                             Logit max-abs vs the f32 reference at full size, random-init weights: bf16 operands 3.2e-3 either way; fp16
                             operands 3.8e-4 (f32 stream) / 6.4e-4 (fp16 stream).  Works for any batch size (small passes take the
                             128 x 128 / 64 x 64 kernels with the same epilogue). */
  int ln_fold;            /* 1 (libucod_dpl_f16.so with resid16 = 1 only): LayerNorm 1 / 2 of every layer but the last are folded into the QKV / fc1
                             GEMMs (ucod_gemm_lnfold): the fp16 stream is the A operand, no LayerNorm output is written or rounded.  The table then
                             carries folded weights (see the table layout).  0: LayerNorm kernels. */
  int n_reg;              /* register tokens of the checkpoint (DINOv2 with registers: 4; 0 otherwise).  Every whole-pass driver (ucod_vit_forward*, _split*, _split16*,
                             _forward_train* / _backward* / _forward_lora_infer*) then runs tok = 1 + n_reg + n tokens per image, [CLS | registers | patches]: table slot +2
                             is f32 [(1 + n_reg), D] (the CLS row, then the register rows; fp16-term pass: times S_patch like CLS / pos), slot +3 stays [1 + n, D];
                             workspace sizes, ucod_vit_last_ln1_offset* and the stream offsets count tok rows; key_out stays [B, D, H/P, W/P] (patch tokens only).
                             0: launch for launch and bit for bit the pass without the field. */
  const float* rope;      /* DINOv3 (HF DINOv3ViTModel): device pointer to the rotary table of THIS grid, f32 [n, 64] = cos[0:32] | sin[0:32] per patch token (ucod_rope_qk);
                             NULL = no rotary embedding (every checkpoint but DINOv3): launch for launch and bit for bit the pass without the field.  With a table
                             ucod_vit_forward* runs one ucod_rope_qk launch between the QKV GEMM (plain or LayerNorm-folded) and the attention kernel of every layer that runs
                             attention, on the 16-bit QKV buffer; the split passes (_split*, _split16*) run it on the f32 QKV output in front of ucod_qkv_split /
                             ucod_split16_qkv (split terms are never rotated).  The key hook is the last layer's K projection BEFORE rotation, so a key-minimal pass
                             runs no rotation in its last layer.  Table slot +3 then holds zeros [1 + n, D] (DINOv3 has no position table).  attn_variant == 8 with a
                             table is UCOD_EINVAL (the fp8 epilogue writes e4m3 Q / K straight from the GEMM drain); the training-pass drivers
                             (ucod_vit_forward_train* / _backward* / _forward_lora_infer*) take a table only with ucod_vit_train_desc.allow_rope = 1. */
} ucod_vit_desc;
/* Rotary position embedding of DINOv3 (transformers modeling_dinov3_vit.py: apply_rotary_pos_emb with rotate_half) on the Q and K thirds of the PATCH rows of a
 * QKV buffer [B tok, 3 heads 64], in place.  tok = 1 + n_reg + n; token row t >= 1 + n_reg of an image is patch p = t - 1 - n_reg and uses table row p of
 * cos_sin f32 [n, 64] = cos[0:32] | sin[0:32] (the model's cos / sin are that half tiled twice); for i < 32 of every head of Q and of K:
 *   out[i] = v[i] cos[i] - v[i + 32] sin[i],  out[i + 32] = v[i + 32] cos[i] + v[i] sin[i]
 * in f32, rounded once to the element type.  elem: UCOD_ROPE_ELEM_HALF = the library's 16-bit operand type (ucod_half_name), UCOD_ROPE_ELEM_F32 = f32 (the QKV
 * output of the split passes).  CLS rows, register rows and the V third are neither read nor written.  The map is linear in v: it commutes with the softmax
 * pre-scale on the Q rows and (exactly) with a power-of-two operand scale.  B, tok, heads > 0, 0 <= n_reg < tok - 1.  csrc/rope.hip. */
#define UCOD_ROPE_ELEM_HALF 0
#define UCOD_ROPE_ELEM_F32 1
int ucod_rope_qk(void* qkv, int elem, const float* cos_sin, int B, int tok, int n_reg, int heads, void* stream);
/* The same with a row pitch and a direction (backbone-backward mode).  buf [B tok, ld] with ld >= 3 heads 64 elements and ld * sizeof(element) a multiple of 16:
 * columns 0 .. 2 D - 1 of the patch rows are rotated, the V third, the CLS / register rows and every column at or beyond 3 D (the 64 LoRA columns of dqkv_aug) are
 * neither read nor written.  inverse = 0: ucod_rope_qk (which is this call with ld = 3 D).  inverse = 1: the transpose, i.e. the sine negated,
 *   out[i] = v[i] cos[i] + v[i + 32] sin[i],  out[i + 32] = v[i + 32] cos[i] - v[i] sin[i]
 * -- what takes the cotangents of rotated q / k back to those of the projection outputs.  f32 arithmetic, one rounding.  Every other refusal as ucod_rope_qk;
 * UCOD_EINVAL before any launch. */
int ucod_rope_qk_ld(void* buf, int elem, const float* cos_sin, int B, int tok, int n_reg, int heads, int ld, int inverse, void* stream);
size_t ucod_vit_workspace_bytes(const ucod_vit_desc* d);
int ucod_vit_forward(const ucod_vit_desc* d, const void* const* table_host, const float* img, float* key_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ split-operand (f32-equivalent) backbone pass (rows B1-B8 at the reference's fp32)
 * The reference builds its cached training features with the backbone in plain fp32 (data/datasets/base_dataset.py:124-138: no autocast; only the Look-Twice
 * extractor is autocast, engine/runner/loop_UCOD_DPL.py:289-290).  This pass computes every matrix product of the ViT with both f32 operands written as sums
 * of `terms` bf16 values -- 2: a0 b0 + a0 b1 + a1 b0 (16 significand bits per operand, 3x the MFMA work; logits within 3e-5 of the f32 oracle on trained-like
 * weights), 3: + a1 b1 + a0 b2 + a2 b0 (24 bits: f32-equivalent, 6x) -- each partial product exact in the MFMA's f32 accumulator, f32 residual stream, f32
 * two-pass LayerNorm, exact-erf GELU, f32 softmax.  The partial products ride on ucod_gemm_bf16 by concatenation along K: an [M, K] operand is stored as
 * bf16 [M, P K], P = ucod_split_products(terms) = 3 / 6, segment p of an A-side operand (role 0) holding term {0,0,1,1,0,2}[p] and of a B-side operand (role 1)
 * term {0,1,0,1,2,0}[p].  libucod_dpl.so only (bf16 MFMA); the fp16 build returns UCOD_EINVAL.  csrc/split.hip. */
int ucod_split_products(int terms);
/* in f32 [M, K] with row pitch ld_in floats -> out bf16 [M, P K].  op 0: the values; 1: exact-erf GELU of them (modeling_dinov2.py:289); 2: times alpha;
 * 3: SwiGLU (modeling_dinov2.py:300-315) of rows 2 K wide interleaved as for UCOD_EPI_BIAS_SWIGLU_BF16 (input column 8k+e is x1, 8k+4+e is x2 of output
 * column 4k+e; ld_in >= 2 K).  K % 8 == 0 */
int ucod_split_rows(const float* in, long ld_in, void* out_bf16, int M, int K, int terms, int role, int op, float alpha, void* stream);
/* nn.LayerNorm (two-pass f32) of f32 rows, written as the split operand of the next GEMM: out bf16 [rows, P D].  D % 128 == 0, D <= 1536 */
int ucod_layernorm_split(const float* x, const float* gamma, const float* beta, void* out_bf16, int rows, int D, float eps, int terms, int role, void* stream);
/* ucod_patch_im2col with split output: patches bf16 [B gh gw, P Kpad] (A side) */
int ucod_patch_im2col_split(const float* img, void* patches_bf16, int B, int C, int H, int W, int P, int Kpad, int terms, void* stream);
/* f32 qkv [B tok, 3 heads 64] (the QKV projection through UCOD_EPI_BIAS_F32) -> the attention kernel's operands in `operands` (ucod_attention_split_operand_bytes):
 * Qc | Kc bf16 [B heads][tok_pad][terms 64] (one 64-wide segment per term; Q times qscale before the split; tok_pad = tok rounded up to 32, pad rows zero)
 * and Vt bf16 [terms][B heads][64][tok_pad] */
size_t ucod_attention_split_operand_bytes(int B, int tok, int heads, int terms);
int ucod_qkv_split(const float* qkv, void* operands, int B, int tok, int heads, int terms, float qscale, void* stream);
/* softmax(Q K^T hd^-0.5) V (modeling_dinov2.py:153-179) on those operands, Q carrying head_dim^-0.5 log2 e; scores, softmax and accumulation in f32, the
 * probabilities split into `terms` bf16 values in registers.  out bf16 [B tok, P heads 64]: the A-side split operand of the out-projection. */
int ucod_attention_split_fwd(const void* operands, void* out_split_bf16, int B, int tok, int heads, int terms, void* stream);
/* The whole pass, image -> last-layer key map f32 [B, D, H/P, W/P] (data/utils/feature_extractor.py:42-59), key-minimal (d->full_last_layer must be 0; resid16,
 * ln_fold and attn_variant of the descriptor are ignored).  Table as ucod_vit_forward's with every weight matrix in its split form:
 *   +0 patch_w bf16 [D, P Kpad] (B side)  +1 patch_b  +2 cls  +3 pos;  layer l at 4 + UCOD_VIT_LAYER_STRIDE l:  +2 qkv_w [3D, P D]  +4 proj_w [D, P D]
 *   +9 fc1_w [F, P D]  +11 fc2_w [D, P F]  (B side),  +14 the K rows of qkv_w as an A-side operand [D, P D] (key hook; needed for the last layer of the pass),
 *   the f32 vectors (+0 +1 +3 +5 +6 +7 +8 +10 +12 +13) as in ucod_vit_forward. */
size_t ucod_vit_split_workspace_bytes(const ucod_vit_desc* d, int terms);
/* byte offset of the f32 residual stream x [B tok, D] inside that workspace: after the pass it holds the input of the pass's last layer (whose CLS rows the pseudo-label
 * generator's attention row is computed from, generate_pseudo_label.py:78-89); (size_t)-1 for a descriptor the pass does not take */
size_t ucod_vit_split_stream_offset(const ucod_vit_desc* d, int terms);
int ucod_vit_forward_split(const ucod_vit_desc* d, int terms, const void* const* table_host, const float* img, float* key_out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* MLP kind of a backbone pass (the _mlp entry points; ucod_vit_desc is unchanged and the entry points without the suffix are the UCOD_MLP_GELU case):
 * UCOD_MLP_GELU: fc1 -> exact-erf GELU -> fc2 (Dinov2MLP, modeling_dinov2.py:281-297).
 * UCOD_MLP_SWIGLU: weights_in -> SwiGLU -> weights_out (Dinov2SwiGLUFFN, modeling_dinov2.py:300-315; DINOv2 ViT-g/14).  Table entries +9 / +10 hold weights_in
 * [2F, D] (split form [2F, P D]) and its bias [2F] with the rows interleaved in blocks of 4 (UCOD_EPI_BIAS_SWIGLU_BF16), +15 (ln_fold) its column sums [2F],
 * +11 weights_out [D, F] (split [D, P F]); d->F is the hidden width after padding (zero rows / columns: exact, silu(0) 0 = 0), F % 128 == 0.  The fc1 launch
 * writes the hidden [M, F] straight from its epilogue (UCOD_EPI_BIAS_SWIGLU_BF16 / UCOD_EPI_LNFOLD_SWIGLU_BF16 / UCOD_EPI_BIAS_SWIGLU_SPLIT2); the three-term
 * split pass goes through UCOD_EPI_BIAS_F32 [M, 2F] and ucod_split_rows op 3. */
enum { UCOD_MLP_GELU = 0, UCOD_MLP_SWIGLU = 1 };
size_t ucod_vit_workspace_bytes_mlp(const ucod_vit_desc* d, int mlp);
int ucod_vit_forward_mlp(const ucod_vit_desc* d, int mlp, const void* const* table_host, const float* img, float* key_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* ucod_vit_forward_mlp with the MLP hidden in BLK16 order where it pays (see "BLK16" above).  fc2_perm_host: NULL (= ucod_vit_forward_mlp), or d->L host pointers,
 * each NULL or that layer's fc2 weight with the BLK16 column permutation, W'[n][k] = W[n][pi(k)], 16-bit [D, F].  A layer with an entry whose fc1 is LayerNorm-folded
 * GELU (ln_fold, not the last layer of the pass) and whose two launches both take a large-tile kernel (ucod_gemm_blk16_pair_ok) writes its hidden with
 * UCOD_EPI_LNFOLD_GELU_BLK16 and reads it with ucod_gemm_bf16_blk16a; every other layer, a small pass (Look-Twice at batch 1) and the SwiGLU MLP run the row-major pair
 * on table entry +11.  Same workspace (ucod_vit_workspace_bytes_mlp).  Key maps differ from the row-major pass only by the order of fc2's f32 additions over K. */
int ucod_vit_forward_blk16(const ucod_vit_desc* d, int mlp, const void* const* table_host, const void* const* fc2_perm_host, const float* img, float* key_out,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t ucod_vit_last_ln1_offset_mlp(const ucod_vit_desc* d, int mlp);
size_t ucod_vit_split_workspace_bytes_mlp(const ucod_vit_desc* d, int terms, int mlp);
size_t ucod_vit_split_stream_offset_mlp(const ucod_vit_desc* d, int terms, int mlp);
int ucod_vit_forward_split_mlp(const ucod_vit_desc* d, int terms, int mlp, const void* const* table_host, const float* img, float* key_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ the split-operand pass on fp16 TERMS ("split2h"; csrc/split16.hip)
 * The same three fp32 passes of the reference (data/datasets/base_dataset.py:124-138, generate_pseudo_label.py:71-89, data/datasets/lr_dataset.py:97-157; arithmetic
 * modeling_dinov2.py:38-149,153-235,238-297,300-315,342-381) with every f32 operand v as TWO IEEE fp16 terms of a power-of-two multiple of it,
 *   hi = fp16(s v),  lo = fp16(s v - hi):   |v - (hi + lo) / s| <= max(2^-22 |v|, 2^-25 / s),
 * and every product as the three partial products hi hi + hi lo + lo hi on the fp16 MFMA: 22 significand bits per operand at the matrix work of the two-term bf16
 * form (16 bits), half that of the three-term one (24 bits).  An [M, K] operand is fp16 [M, 3 K]: role 0 (A side) hi | hi | lo, role 1 (B side) hi | lo | hi; the
 * GEMMs are ucod_gemm_bf16 of libucod_dpl_f16.so with K' = 3 K, whose accumulator then holds s_a s_b times the product (csrc/split16.hip says how the factor
 * leaves through the existing epilogues' bias / scale arguments, exactly).  `scale` arguments must be powers of two (UCOD_EINVAL otherwise).  |s v| > 65504 is
 * clamped and COUNTED into the saturation counter of the fp16 stream (ucod_resid16_overflow_*).  libucod_dpl_f16.so only; the bf16 build returns UCOD_EINVAL
 * (and the fp16 build keeps refusing ucod_split_* / ucod_vit_forward_split*). */
enum { UCOD_SPLIT16_LN = 0, UCOD_SPLIT16_QKV = 1, UCOD_SPLIT16_PROB = 2, UCOD_SPLIT16_ATT = 3, UCOD_SPLIT16_HIDDEN = 4, UCOD_SPLIT16_PATCH = 5, UCOD_SPLIT16_NUM_CLASSES = 6 };
/* the scale the pass gives an activation operand class (LayerNorm output, q / k / v, probabilities, attention output, MLP hidden, patches); 0 for an unknown class */
float ucod_split16_class_scale(int cls);
/* f32 [M, K] (row pitch ld_in elements) -> fp16 [M, 3 K] of scale * f(in); op 0: f = identity, 1: exact-erf GELU of alpha * in, 2: alpha * in, 3: SwiGLU of alpha *
 * rows 2 K wide interleaved as for UCOD_EPI_BIAS_SWIGLU_BF16.  K % 8 == 0, ld_in % 4 == 0 */
int ucod_split16_rows(const float* in, long ld_in, void* out_f16, int M, int K, int role, int op, float alpha, float scale, void* stream);
/* nn.LayerNorm (two-pass f32) of f32 rows times `scale`, as a split operand fp16 [rows, 3 D].  D / 128 in {1, 2, 3, 4, 5, 6, 8, 10, 12} */
int ucod_split16_layernorm(const float* x, const float* gamma, const float* beta, void* out_f16, int rows, int D, float eps, int role, float scale, void* stream);
/* ucod_patch_im2col with split output: patches fp16 [B gh gw, 3 Kpad] (A side) of scale * pixel */
int ucod_split16_patch_im2col(const float* img, void* patches_f16, int B, int C, int H, int W, int P, int Kpad, float scale, void* stream);
/* in place x[i] *= alpha, alpha a power of two (the operand scales leaving the token rows / the key map) */
int ucod_split16_scale_f32(float* x, size_t n, float alpha, void* stream);
/* f32 qkv [B tok, 3 heads 64] times in_mul -> the attention kernel's operands (ucod_split16_attention_operand_bytes): Qc | Kc fp16 [B heads][tok_pad][2 64]
 * (hi | lo; Q times qscale), Vt fp16 [2][B heads][64][tok_pad]; every value times `scale` before its split; tok_pad = tok rounded up to 32, pad rows zero */
size_t ucod_split16_attention_operand_bytes(int B, int tok, int heads);
int ucod_split16_qkv(const float* qkv, void* operands, int B, int tok, int heads, float in_mul, float qscale, float scale, void* stream);
/* softmax(Q K^T) V (modeling_dinov2.py:153-179; the softmax scale and log2 e are inside Q) on those operands (`scale` = the one ucod_split16_qkv was given), f32
 * online softmax, probabilities times 2^14 as two fp16 terms.  out fp16 [B tok, 3 heads 64]: out_scale times the result as the A-side operand of the out-projection */
int ucod_split16_attention_fwd(const void* operands, void* out_split_f16, int B, int tok, int heads, float scale, float out_scale, void* stream);
/* out2_dev[0] = 2^-24 (the smallest fp16 subnormal) times 2^14 and out2_dev[1] = 2^-14 (the smallest normal) times 2^14, each as one v_mfma_f32_32x32x16_f16:
 * 2^-10 / 1 if the matrix pipe keeps subnormal fp16 inputs, 0 / 1 if it flushes them */
int ucod_split16_mfma_subnormal_probe(float* out2_dev, void* stream);
/* The whole key-minimal pass (as ucod_vit_forward_split_mlp).  Table as there with fp16 split weights, each scaled by wscale_host[...] (1 + 4 L powers of two: patch_w,
 * then per layer qkv_w (also the +14 key rows), proj_w, fc1_w, fc2_w), and with the f32 vectors of a GEMM carrying its operand scales S = s_act s_w:
 *   +1 patch_b, +2 cls, +3 pos times S_patch;  +3 qkv_b times S_qkv;  +5 proj_b times S_proj, +6 LayerScale 1 / S_proj;  +10 fc1_b times S_fc1;
 *   +12 fc2_b times S_fc2, +13 LayerScale 2 / S_fc2       (s_act = ucod_split16_class_scale of PATCH, LN, ATT, LN, HIDDEN)
 * No allocation, no synchronisation.  ucod_vit_split16_stream_offset: as ucod_vit_split_stream_offset. */
size_t ucod_vit_split16_workspace_bytes(const ucod_vit_desc* d, int mlp);
size_t ucod_vit_split16_stream_offset(const ucod_vit_desc* d, int mlp);
int ucod_vit_forward_split16(const ucod_vit_desc* d, int mlp, const void* const* table_host, const float* wscale_host, int n_wscale, const float* img, float* key_out,
                             void* workspace, size_t workspace_bytes, void* stream);
/* fc1 + activation + split in ONE launch: out = the A-side split operand (hi | hi | lo) of scale * f(alpha * (A B^T + bias)), where A [M, K3] and B [N, K3] are
 * K-concatenated fp16 split operands, bias_scaled [N] is the bias times the operands' scales S = s_a s_w and alpha = 1 / S.  op as ucod_split16_rows: 1 exact-erf GELU
 * (out fp16 [M, 3 N]), 3 SwiGLU of the interleaved x1 / x2 columns of UCOD_EPI_BIAS_SWIGLU_BF16 (out fp16 [M, 3 N/2], segments N/2 apart); others refused.  The drain
 * calls the activation and the split of ucod_split16_rows on the same f32 value, so the result equals ucod_gemm_bf16(UCOD_EPI_BIAS_F32) + ucod_split16_rows bit for
 * bit wherever the two GEMMs sum K in the same order (every tile path of one `variant`; the leftover patches of variants 9 / 10 exist for op 1 only).  Values beyond
 * +-65504 and NaN are clamped and counted like there.  alpha and scale powers of two, N % 8 == 0, K3 % 64 == 0, M * 3 N * 2 bytes (op 3: M * 3 N) below 2^31;
 * variant as ucod_gemm_bf16 (0, 1, 2, 12, 9, 10, 13, 14) */
int ucod_split16_gemm_act(int op, const void* a_f16, const void* b_f16, void* out_f16, int M, int N, int K3, const float* bias_scaled, float alpha, float scale,
                          int variant, void* stream);
/* The pass with options.  flags = 0: ucod_vit_forward_split16 launch for launch (the three entry points above are this case).  UCOD_SPLIT16_FUSE_MLP: fc1 runs as ONE
 * ucod_split16_gemm_act instead of UCOD_EPI_BIAS_F32 + ucod_split16_rows, and the workspace holds no f32 fc1 buffer (M F 4 bytes less, M 2F 4 for SwiGLU).  Unknown
 * flag bits: UCOD_EINVAL (sizes: 0, offset: (size_t)-1) */
enum { UCOD_SPLIT16_FUSE_MLP = 1 };
size_t ucod_vit_split16_workspace_bytes_ex(const ucod_vit_desc* d, int mlp, int flags);
size_t ucod_vit_split16_stream_offset_ex(const ucod_vit_desc* d, int mlp, int flags);
int ucod_vit_forward_split16_ex(const ucod_vit_desc* d, int mlp, int flags, const void* const* table_host, const float* wscale_host, int n_wscale, const float* img,
                                float* key_out, void* workspace, size_t workspace_bytes, void* stream);

/* Backbone-backward mode, whole passes (row B9; operand formats in ucod_dpl_amd/csrc/vit_train.hip): a training forward that saves its activations, the backward
 * that turns the cotangent of the key map into LoRA gradients, and a no-grad forward.  The tables, the workspace and what each pass enqueues are described once, at
 * the _lora_out_ex forms that close this section: new callers should use those.  The four older tiers of entry points remain, each the _lora_out_ex form with the
 * arguments it lacks at their neutral values; one driver body serves them all (ucod_dpl_amd/csrc/vit_train_driver.hip). */
#define UCOD_VIT_TRAIN_STRIDE 7
typedef struct {
  ucod_vit_desc vit;
  int lora_r;                    /* models/modules/full_model.py:48: r = 2 */
  float lora_scaling;            /* lora_alpha / r = 4 / 2 */
  float lora_dropout;            /* full_model.py:50: 0.05 in the reference config; 0 = off (eval mode) */
  unsigned long long seed;       /* dropout seed of THIS step: forward_train and backward must be given the same value */
  int allow_rope;                /* 1: the passes take vit.rope (DINOv3): every layer but the last runs one ucod_rope_qk_ld(qkv, HALF, rope, ..., 3 D, 0) between the QKV GEMM
                                    and attention -- in the training pass on the SAVED qkv -- and ucod_vit_backward* one ucod_rope_qk_ld(dqkv_aug, HALF, rope, ..., 3 D + 64, 1)
                                    between ucod_attention_bwd and the LoRA-gradient kernel; the last layer's key hook stays in front of any rotation.  0 (every caller
                                    that zero-fills the descriptor): a non-NULL vit.rope is UCOD_EINVAL, sizes 0.  With vit.rope == NULL the flag changes nothing. */
} ucod_vit_train_desc;
/* The _lora_out_ex forms with mlp = UCOD_MLP_GELU, out_flags = 0, mlp_table_host = out_table_host = NULL. */
size_t ucod_vit_train_workspace_bytes(const ucod_vit_train_desc* t);
int ucod_vit_forward_train(const ucod_vit_train_desc* t, const void* const* table_host, const void* const* train_table_host,
                           const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream);
int ucod_vit_backward(const ucod_vit_train_desc* t, const void* const* table_host, const void* const* train_table_host,
                      const float* dkey, void* workspace, size_t workspace_bytes, void* stream);
size_t ucod_vit_lora_infer_workspace_bytes(const ucod_vit_train_desc* t);
int ucod_vit_forward_lora_infer(const ucod_vit_train_desc* t, const void* const* table_host, const void* const* train_table_host,
                                const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream);
/* The _lora_out_ex forms with out_flags = 0, mlp_table_host = out_table_host = NULL (the MLP kind of the pass: UCOD_MLP_*). */
size_t ucod_vit_train_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp);
int ucod_vit_forward_train_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                               const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream);
int ucod_vit_backward_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                          const float* dkey, void* workspace, size_t workspace_bytes, void* stream);
size_t ucod_vit_lora_infer_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp);
int ucod_vit_forward_lora_infer_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                                    const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream);

/* LoRA on the MLP input projection as well (models/modules/full_model.py:47-72: `target_modules` is handed to peft, so `fc1` -- `weights_in` on a SwiGLU
 * checkpoint -- is an ordinary target there).  The projection's input is LayerNorm 2's output, so the module rides on the fc1 GEMM the way q / k / v ride on the
 * QKV GEMM: 64 extra K columns, of which the first r are used.  N1 = F (GELU) or 2F (SwiGLU, the padded 4-interleaved row order of ucod_vit_forward_mlp).
 * One layer's parameters / gradients (f32): [A_m (r x D) | B_m (N1 x r)], 1 <= r <= UCOD_LORA_MLP_MAX_R (the gradient kernel keeps a lane's B_m values and
 * their accumulators in registers, two ranks per pass).  Dropout: the module's own mask is projection 0 of ucod_lora_dropout with layer = L + l.
 *   forward   h2_aug [M, D+64] = [ LN2(x) | drop(LN2(x)) A_m^T (r values) | 0 ]              (ucod_layernorm_lora_mlp)
 *             fc1_w_aug [N1, D+64] = [ fc1_w | alpha/r * B_m (dense rows) | 0 ]               (ucod_lora_mlp_pack)
 *   backward  dpre [M, N1] has no aug columns (the fc2 dgrad's drain writes it), so t = alpha/r * dpre B_m goes to a scratch [M, 64] and the t A_m term of
 *             d LN2 is added by the LayerNorm-2 backward (ucod_layernorm_bwd_lora_mlp), with or without dropout. */
#define UCOD_LORA_MLP_MAX_R 8
/* y_aug bf16 [rows, D+64] = [ LayerNorm(x) | dropout(LN(x)) A_m^T (r values) | 0 ]: ucod_layernorm_lora for ONE module, a_m f32 [r, D]; x_f16 != 0: x is the
 * IEEE fp16 residual stream, else f32 (full_model.py:47-72) */
int ucod_layernorm_lora_mlp(const void* x, int x_f16, const float* gamma, const float* beta, const float* a_m, int r, void* y_aug_bf16, int rows, int D,
                            float eps, const ucod_lora_dropout* dropout, void* stream);
/* aug columns of fc1_w_aug bf16 [N1, D+64] from one layer's [A_m | B_m]: column D + j = alpha/r * B_m[:, j] for j < r, zero beyond (full_model.py:47-72) */
int ucod_lora_mlp_pack(const float* lora_mlp, int r, float scaling, void* fc1_w_aug_bf16, int N1, int D, void* stream);
/* One layer's gradients of the MLP module in one pass over dpre bf16 [rows, N1] and h2_aug bf16 [rows, D+64] per two ranks (full_model.py:47-72):
 *   t bf16 [rows, 64] = alpha/r * dpre B_m (r values, the rest zero);  dB_m = alpha/r * dpre^T u (u = aug columns of h2_aug);  dA_m = t^T dropout(h2), from the
 * bf16-rounded t.  grad_mlp f32 [r (D + N1)] is overwritten.  Deterministic: per-block partials in `workspace`, summed in a fixed order.  N1 % 128 == 0,
 * N1 <= 8192, D % 128 == 0, D <= 1536. */
size_t ucod_lora_mlp_grad_workspace_bytes(int N1, int D);
int ucod_lora_mlp_grad(const void* dpre_bf16, const void* h2_aug_bf16, const float* lora_mlp, int r, float scaling, float* grad_mlp, void* t_bf16,
                       void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream);
/* ucod_layernorm_bwd_lora_ex for ONE module whose t lives anywhere (full_model.py:47-72):  dy += mask/(1-p) * (t A_m), t bf16 rows of length ldt (r values
 * used), a_m f32 [r, D]; dropout NULL or p == 0: the unmasked term. */
int ucod_layernorm_bwd_lora_mlp(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                void* s_bf16, int rows, int D, float eps, const void* t_bf16, int ldt, const float* a_m, int r,
                                const ucod_lora_dropout* dropout, void* stream);
/* The gated MLP's input (DINOv3 vits16plus: down_proj(silu(gate_proj(x)) * up_proj(x))) is TWO peft modules, gate_proj and up_proj, each with its own A, B and
 * dropout mask, on the ONE fused, padded, 4-interleaved weights_in GEMM: engine row 8k+e is gate row 4k+e for e < 4, row 8k+4+e is up row 4k+e.  The pair is a
 * rank-2r module whose B is block diagonal.  One layer's parameters / gradients (f32): [A_g (r x D) | A_u (r x D) | B_m (N1 x r)], N1 = 2F, B_m in the engine's row
 * order (row n is gate's iff n % 8 < 4: byte for byte the single module's B_m), padded rows zero.  A module of the pair that is not targeted has A = 0 and its
 * rows of B = 0; its gradients are then exact zeros (u = 0 gives dB = 0, t = 0 gives dA = 0).  Masks: gate_proj is projection 0, up_proj projection 1 of
 * ucod_lora_dropout with layer = L + l.  1 <= r <= UCOD_LORA_MLP_MAX_R.
 * ucod_layernorm_lora_mlp_pair (full_model.py:47-72): y_aug bf16 [rows, D+64] = [ LN(x) | drop_0(LN x) A_g^T (r) | drop_1(LN x) A_u^T (r) | 0 ], a_pair f32 [2r, D]. */
int ucod_layernorm_lora_mlp_pair(const void* x, int x_f16, const float* gamma, const float* beta, const float* a_pair, int r, void* y_aug_bf16, int rows, int D,
                                 float eps, const ucod_lora_dropout* dropout, void* stream);
/* aug columns of fc1_w_aug bf16 [N1, D+64] from one layer's [A_g | A_u | B_m] (full_model.py:47-72): row n gets alpha/r * B_m[n][j] at column D + mod(n) r + j
 * (mod(n) = 0 for a gate row, 1 for an up row); every other aug column is zero.  N1 % 8 == 0, N1 <= 8192. */
int ucod_lora_mlp_pair_pack(const float* lora_pair, int r, float scaling, void* fc1_w_aug_bf16, int N1, int D, void* stream);
/* Both modules' gradients of one layer in ONE pass over dpre bf16 [rows, N1] and h2_aug bf16 [rows, D+64] per two ranks (full_model.py:47-72): of a thread's
 * 16-byte dpre vector elements 0-3 are gate's and 4-7 up's;  t bf16 [rows, 64]: column p r + j = alpha/r * sum over module p's rows n of dpre[:, n] B_m[n][j], the
 * rest zero;  dB_m[n] = alpha/r * dpre[:, n]^T u_mod(n);  dA_p = t_p^T drop_p(h2), from the bf16-rounded t.  grad_pair f32 [r (2D + N1)] is overwritten.
 * Deterministic: per-block partials in `workspace`, summed in a fixed order by a reduce kernel; no float atomics.  N1 % 128 == 0, N1 <= 8192, D % 128 == 0,
 * D <= 1536 (else the size is 0 and the call UCOD_EINVAL before any launch; a workspace that is too small: UCOD_ENOMEM).  Every instantiation runs both modules in
 * one pass: none of them spills to scratch memory, so the launch function has no two-pass case. */
size_t ucod_lora_mlp_pair_grad_workspace_bytes(int N1, int D);
int ucod_lora_mlp_pair_grad(const void* dpre_bf16, const void* h2_aug_bf16, const float* lora_pair, int r, float scaling, float* grad_pair, void* t_bf16,
                            void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream);
/* ucod_layernorm_bwd_lora_mlp for the pair (full_model.py:47-72):  dy += mask_0/(1-p) * (t_g A_g) + mask_1/(1-p) * (t_u A_u), t_p at columns p r + j of the
 * bf16 rows of length ldt >= 2r, a_pair f32 [2r, D]. */
int ucod_layernorm_bwd_lora_mlp_pair(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                     void* s_bf16, int rows, int D, float eps, const void* t_bf16, int ldt, const float* a_pair, int r,
                                     const ucod_lora_dropout* dropout, void* stream);
/* The _lora_out_ex forms with out_table_host = NULL, out_flags = 0 (TM, the MLP module's own per-layer table, is described there; layer l at UCOD_VIT_TRAIN_MLP_STRIDE*l). */
#define UCOD_VIT_TRAIN_MLP_STRIDE 3
size_t ucod_vit_train_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* mlp_table_host);
int ucod_vit_forward_train_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                                    const void* const* mlp_table_host, const float* img, float* key_out, void* workspace, size_t workspace_bytes,
                                    void* stream);
int ucod_vit_backward_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                               const void* const* mlp_table_host, const float* dkey, void* workspace, size_t workspace_bytes, void* stream);
size_t ucod_vit_lora_infer_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* mlp_table_host);
int ucod_vit_forward_lora_infer_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                                         const void* const* mlp_table_host, const float* img, float* key_out, void* workspace, size_t workspace_bytes,
                                         void* stream);

/* LoRA on the output projections as well (models/modules/full_model.py:47-72: `target_modules` is handed to peft, so attention.output.dense / mlp.fc2 -- o_proj /
 * down_proj on a DINOv3 checkpoint -- are ordinary targets there; peft's module computes  result = base(x) + scaling * B(A(dropout(x)))).  Their inputs are written by the
 * attention kernel and by the fc1 drain, which have no room for 64 LoRA columns, so the module runs BESIDE its GEMM as row kernels.  For a module with input
 * x_in bf16 [M, K] and layer scale lambda (K = D, lambda = ls1 for dense: x_in = the attention output; K = F, lambda = ls2 for fc2: x_in = the hidden):
 *   forward   u [M, 8] f32 = drop(x_in) A^T (r values, zeros beyond);   x[m, :] += lambda * (scaling * u[m, :] B^T)   on the stream the GEMM has just written
 *   backward  with s = bf16(lambda * dx), the operand the dgrad GEMM takes:   t [M, 8] f32 = scaling * s B,   dB = scaling * s^T u,   dA = t^T drop(x_in),
 *             cotangent of x_in += mask/(1-p) * (t A)   (fc2: the cotangent buffer holds dpre = dg * gelu'(pre), so the term carries gelu'(pre) too)
 * One module's parameters / gradients of one layer (f32): [A (r x K) | B (D x r)], 1 <= r <= UCOD_LORA_MLP_MAX_R (u and t rows are UCOD_LORA_OUT_W wide).
 * K % 128 == 0, 128 <= K <= 4096 (a thread keeps the A values of its two 16-byte vectors in registers), D % 128 == 0, D <= 1536.
 * Dropout keys: the mask is projection 0 of ucod_lora_dropout over idx = row * K + col with `layer` = 2 L + l for dense and 3 L + l for fc2 -- distinct from the
 * q / k / v keys (l) and the MLP input projection's (L + l).  Every gradient is a sum of per-block partials in a fixed order: two runs are bit-identical. */
#define UCOD_LORA_OUT_W 8
#define UCOD_LORA_OUT_ACT_IDENTITY 0   /* x_in is the buffer itself (dense: the saved attention output) */
#define UCOD_LORA_OUT_ACT_GELU 1       /* x_in = gelu(pre), the buffer is the saved pre-activation (fc2); gelu / gelu' are the fc1 drains' own fit */
/* the SwiGLU MLP's output projection (Dinov2SwiGLUFFN.weights_out; the gated DINOv3 down_proj): K = the padded hidden width F, x_in_bf16 is the saved pre-activation
 * [rows, 2K] interleaved in blocks of 4 (UCOD_EPI_BIAS_SWIGLU_BF16: columns 8k + e hold x1 of hidden unit 4k + e, columns 8k + 4 + e its x2), cot_bf16 is dpre
 * [rows, 2K] in the same order, A is [r, K] in hidden-unit order, the mask index is row * K + unit.  The hidden h = silu(x1) * x2 is recomputed, never stored:
 *   dA[j][u] += t[row][j] * m * h,   dg = m * sum_j t[row][j] A[j][u],   dpre(x1) += dg * x2 * sig * (1 + x1 (1 - sig)),   dpre(x2) += dg * x1 * sig
 * with m = mask/(1-p), sig = sigmoid(x1); silu and the two factors are the weights_in / weights_out-dgrad drains' own.  Padded units (x1 = x2 = 0, zero A column)
 * give exact zeros.  Its buffers are twice as wide as those of the other forms, so it has its own way in: ucod_lora_out_grad_x_ex with UCOD_LORA_OUT_SWIGLU in
 * out_flags.  ucod_lora_out_grad_x itself, whose callers hold [rows, K] buffers, keeps refusing act = 2 as the invalid argument it always was. */
#define UCOD_LORA_OUT_ACT_SWIGLU 2
/* bytes of the per-block partials either gradient kernel needs; 0 for sizes outside the limits above */
size_t ucod_lora_out_grad_workspace_bytes(int r, int K, int D);
/* x_stream[m, :] += lambda * (scaling * (drop(x_in[m, :]) A^T) B^T), rows of D f32 (stream_f16 = 0) or IEEE fp16 (1: clamped and counted like the stream's other
 * writers); lambda f32 [D] or NULL (ones); u_out f32 [rows, 8] receives u, or NULL (the no-grad pass).  Runs right behind the residual GEMM (full_model.py:47-72). */
int ucod_lora_out_fwd(const void* x_in_bf16, const float* lora_out, int r, float scaling, const float* lambda, void* x_stream, int stream_f16, float* u_out,
                      int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream);
/* t f32 [rows, 8] = scaling * s B (zeros beyond r) and the B part of grad_out (overwritten): dB = scaling * s^T u; s bf16 [rows, D], u f32 [rows, 8].  Must run
 * before the driver reuses s's buffer (full_model.py:47-72). */
int ucod_lora_out_grad_s(const void* s_bf16, const float* u, const float* lora_out, int r, float scaling, float* grad_out, float* t_out, void* workspace,
                         size_t workspace_bytes, int rows, int K, int D, void* stream);
/* the A part of grad_out (overwritten): dA = t^T drop(x_in), and cot[m, :] += act'(.) * mask/(1-p) * (t[m, :] A) in place, cot bf16 [rows, K]; act = UCOD_LORA_OUT_ACT_*
 * (GELU: x_in_bf16 is the saved pre-activation, x_in = gelu(pre) is recomputed, never stored) (full_model.py:47-72). */
int ucod_lora_out_grad_x(const void* x_in_bf16, int act, void* cot_bf16, const float* t, const float* lora_out, int r, float* grad_out, void* workspace,
                         size_t workspace_bytes, int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream);
/* ucod_lora_out_grad_x with one word of flags behind `act` (UCOD_LORA_OUT_SWIGLU, defined below: needed for, and only meaningful with, UCOD_LORA_OUT_ACT_SWIGLU; an
 * unknown bit is UCOD_EINVAL).  out_flags = 0 is ucod_lora_out_grad_x, which delegates here. */
int ucod_lora_out_grad_x_ex(const void* x_in_bf16, int act, int out_flags, void* cot_bf16, const float* t, const float* lora_out, int r, float* grad_out,
                            void* workspace, size_t workspace_bytes, int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream);
/* Hidden widths past the register-resident forms (full_model.py:47-72: peft takes any Linear; DINOv3 ViT-H+/16 has a gated MLP of hidden width 5120, so
 * N1 = 10240 and K = 5120).  The _wide entry points below are supersets of their namesakes: at N1 <= 8192 / K <= 4096 they enqueue the same launches with the same
 * workspace size and give the same bits; above, up to UCOD_LORA_WIDE_MAX_N1 / UCOD_LORA_WIDE_MAX_K (what the wide kernels hold with no scratch memory),
 *   ucod_lora_mlp_grad_wide / _pair_grad_wide   run the gradient kernel with FIVE 16-byte dpre vectors per thread and ONE rank per pass (r passes over dpre; the
 *                                               partials are [modules][D] | [N1] per block, so the workspace is half the narrow formula's at the same N1),
 *   ucod_lora_out_fwd_wide                      runs blocks of 512 threads with two 16-byte vectors each (eight wave partials, summed as two groups of four),
 *   the others                                  run their one kernel (one thread per element, or K spread over blockIdx.y) with the real width.
 * Same formulas, rounding points, dropout keys and mask indices as the narrow forms; D % 128 == 0, D <= 1536, r <= UCOD_LORA_MLP_MAX_R, widths % 128 == 0 as there
 * (else the size is 0 and the call UCOD_EINVAL before any launch).  UCOD_LORA_WIDE in the flags word of ucod_lora_out_grad_x_ex is that function's wide form; in
 * out_flags of the pass entry points (below) it makes the pass call the wide forms. */
#define UCOD_LORA_WIDE 16
#define UCOD_LORA_WIDE_MAX_N1 10240
#define UCOD_LORA_WIDE_MAX_K 8192
int ucod_lora_mlp_pack_wide(const float* lora_mlp, int r, float scaling, void* fc1_w_aug_bf16, int N1, int D, void* stream);
int ucod_lora_mlp_pair_pack_wide(const float* lora_pair, int r, float scaling, void* fc1_w_aug_bf16, int N1, int D, void* stream);
size_t ucod_lora_mlp_grad_workspace_bytes_wide(int N1, int D);
size_t ucod_lora_mlp_pair_grad_workspace_bytes_wide(int N1, int D);
int ucod_lora_mlp_grad_wide(const void* dpre_bf16, const void* h2_aug_bf16, const float* lora_mlp, int r, float scaling, float* grad_mlp, void* t_bf16,
                            void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream);
int ucod_lora_mlp_pair_grad_wide(const void* dpre_bf16, const void* h2_aug_bf16, const float* lora_pair, int r, float scaling, float* grad_pair, void* t_bf16,
                                 void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream);
size_t ucod_lora_out_grad_workspace_bytes_wide(int r, int K, int D);
int ucod_lora_out_fwd_wide(const void* x_in_bf16, const float* lora_out, int r, float scaling, const float* lambda, void* x_stream, int stream_f16, float* u_out,
                           int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream);
int ucod_lora_out_grad_s_wide(const void* s_bf16, const float* u, const float* lora_out, int r, float scaling, float* grad_out, float* t_out, void* workspace,
                              size_t workspace_bytes, int rows, int K, int D, void* stream);
/* The _lora_out_ex forms with out_flags = 0: they refuse the fc2 slots on the SwiGLU MLP (TO, the output modules' own per-layer table, is described there; layer l at
 * UCOD_VIT_TRAIN_OUT_STRIDE*l). */
#define UCOD_VIT_TRAIN_OUT_STRIDE 4
size_t ucod_vit_train_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* mlp_table_host, const void* const* out_table_host);
int ucod_vit_forward_train_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                                    const void* const* mlp_table_host, const void* const* out_table_host, const float* img, float* key_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
int ucod_vit_backward_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                               const void* const* mlp_table_host, const void* const* out_table_host, const float* dkey, void* workspace, size_t workspace_bytes,
                               void* stream);
size_t ucod_vit_lora_infer_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* mlp_table_host, const void* const* out_table_host);
int ucod_vit_forward_lora_infer_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* table_host, const void* const* train_table_host,
                                         const void* const* mlp_table_host, const void* const* out_table_host, const float* img, float* key_out, void* workspace,
                                         size_t workspace_bytes, void* stream);
/* The whole passes, in full: the _lora_out_ex forms.  Every argument an older tier lacks has a neutral value here -- mlp = UCOD_MLP_GELU, out_flags = 0, a NULL
 * mlp_table_host / out_table_host -- and with it the pass enqueues, launch for launch, and refuses, refusal for refusal, what that tier does; the size functions return
 * the same bytes.  An unknown MLP kind or an unknown bit of out_flags: UCOD_EINVAL, sizes 0.  bf16 build only (ucod_half_name).
 *
 * Tables (HOST arrays of DEVICE pointers).  T = table_host, the table of ucod_vit_forward (UCOD_MLP_SWIGLU: +9 / +10 / +11 are those of ucod_vit_forward_mlp: weights_in
 * [2F, D] and its bias interleaved in blocks of 4, weights_out [D, F]; d->F the padded hidden width).
 *   TT = train_table_host, layer l at UCOD_VIT_TRAIN_STRIDE*l:
 *     +0 qkv_w_aug bf16 [3D, D+64]   +1 qkv_wT_aug bf16 [D, 3D+64]   (aug columns maintained by ucod_lora_pack)
 *     +2 proj_w^T bf16 [D,D]   +3 fc1_w^T bf16 [D,F]   +4 fc2_w^T bf16 [F,D]   (frozen; transposed once by the host)
 *     +5 LoRA parameters f32 [6*r*D]   +6 LoRA gradients f32 [6*r*D] (overwritten by ucod_vit_backward*)
 *     UCOD_MLP_SWIGLU (Dinov2SwiGLUFFN, modeling_dinov2.py:300-315; DINOv2 ViT-g/14): +3 is the transpose of the interleaved weights_in, bf16 [D, 2F] (its K order is
 *     the column order of the pre-activation's cotangent), +4 the transpose of weights_out, bf16 [F, D].
 *   TM = mlp_table_host or NULL, the LoRA module on the MLP input projection (full_model.py:47-72), layer l at UCOD_VIT_TRAIN_MLP_STRIDE*l:
 *     +0 fc1_w_aug bf16 [N1, D+64] (aug columns maintained by ucod_lora_mlp_pack)   +1 LoRA parameters f32 [r (D + N1)]   +2 LoRA gradients f32 [r (D + N1)]
 *     Needs lora_r <= UCOD_LORA_MLP_MAX_R (else UCOD_EINVAL, sizes 0).
 *   TO = out_table_host or NULL, the LoRA modules on the output projections (full_model.py:47-72; result = base(x) + scaling * B(A(dropout(x)))), layer l at
 *   UCOD_VIT_TRAIN_OUT_STRIDE*l:
 *     +0 dense parameters f32 [r (D + D)] or NULL   +1 dense gradients   +2 fc2 parameters f32 [r (F + D)] or NULL   +3 fc2 gradients
 *     A module is targeted when layer 0's parameter slot is not NULL (the same modules in every layer); a table that names none is UCOD_EINVAL.  Needs lora_r <=
 *     UCOD_LORA_MLP_MAX_R and the sizes of ucod_lora_out_grad_workspace_bytes (else UCOD_EINVAL, sizes 0).  With UCOD_MLP_SWIGLU the fc2 slots need UCOD_LORA_OUT_SWIGLU.
 *
 * ucod_vit_forward_train*: image -> key_out, saving its activations in `workspace`; ucod_vit_backward* must be given the same, untouched workspace and the same
 * descriptor (seed included).  dkey f32 [B, D, H/P, W/P] = cotangent of key_out.  gemm_variant of the embedded desc applies; attention is the pre-scaled kernel.  With
 * lora_dropout > 0 the aug A^T columns of qkv_wT_aug must have been packed as zeros (ucod_lora_pack).  Saved per layer: the two residual-stream states (f32, or IEEE
 * fp16 with vit.resid16), LayerNorm 1's output with the LoRA down-projection, qkv, the attention output, the log-sum-exp, the fc1 pre-activation bf16 [M, F] -- with
 * UCOD_MLP_SWIGLU the interleaved one, bf16 [M, 2F], from UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 -- and, with TO, u of each targeted module (M * 32 bytes per layer and module).
 * ucod_vit_forward_lora_infer*: the no-grad pass of the LoRA backbone -- the EMA teacher of models/modules/full_model.py:84,108-111 (backbone_ema under
 * torch.no_grad()): the arithmetic of ucod_vit_forward_train* (the same launches but ucod_attention_fwd, the plain fc1 epilogues -- UCOD_EPI_BIAS_SWIGLU_BF16 for
 * SwiGLU -- and no u stored; the same dropout masks for the same seed) with nothing saved for a backward; t->vit.resid16 may be 1 (fp16 residual stream, as
 * ucod_vit_forward).  Own, inference-sized workspace, to which TO adds no byte.
 *
 * Per layer below the last (the last runs LayerNorm 1 and the key projection only; the gradients of its MLP and output modules are written as zeros):
 *   q / k / v    ride on the QKV GEMM as 64 extra K columns; vit.rope (allow_rope) adds the rotations the descriptor describes.
 *   SwiGLU       the backward runs the weights_out dgrad through UCOD_EPI_SWIGLU_BWD_BF16 into dpre bf16 [M, 2F] (which the hidden's buffer is sized for) and the plain
 *                weights_in dgrad with K = 2F.  Everything outside the MLP is the GELU pass's.
 *   TM           the forward runs ucod_layernorm_lora_mlp and fc1 with K = D+64; the backward recomputes h2_aug from the saved residual stream, runs ucod_lora_mlp_grad
 *                and ucod_layernorm_bwd_lora_mlp.
 *   TO           the forward runs one ucod_lora_out_fwd behind each targeted module's residual GEMM; the backward one ucod_lora_out_grad_s + ucod_lora_out_grad_x per
 *                module: fc2's behind the fc2 dgrad and in front of ucod_lora_mlp_grad / the fc1 dgrad, dense's between the out-proj dgrad and ucod_attention_bwd.
 * Dropout keys (`layer` of ucod_lora_dropout): kind * L + l with kind 0 = q / k / v, 1 = the MLP input projection, 2 = dense, 3 = fc2, in all three passes.
 *
 * out_flags:
 *   UCOD_LORA_OUT_SWIGLU   with UCOD_MLP_SWIGLU, slot +2 may be non-NULL: the LoRA module of the SwiGLU MLP's output projection (weights_out; the gated DINOv3
 *                          down_proj), parameters f32 [r (F + D)] with F the padded hidden width (K = F <= 4096 as above: ViT-g and vits16plus; vith16plus's
 *                          F = 5120 needs UCOD_LORA_WIDE).  Per layer below the last: one ucod_lora_out_fwd on the hidden [M, F] behind the weights_out residual GEMM (key
 *                          3 L + l; the training pass saves u in the fc2 module's slots, so the workspace is the GELU formula with K = F); in the backward, behind
 *                          the UCOD_EPI_SWIGLU_BWD_BF16 GEMM, ucod_lora_out_grad_s on s and ucod_lora_out_grad_x_ex(pre, UCOD_LORA_OUT_ACT_SWIGLU, dpre) in front of
 *                          ucod_layernorm_lora_mlp / ucod_lora_mlp_grad and the weights_in dgrad.  The last layer's gradients are written as zeros.  With
 *                          UCOD_MLP_GELU the flag changes nothing.
 *   UCOD_LORA_MLP_PAIR     (full_model.py:47-72) valid only with UCOD_MLP_SWIGLU and a non-NULL TM (else UCOD_EINVAL, sizes 0): TM describes the gated MLP's PAIR
 *                          gate_proj / up_proj -- slots +1 / +2 are [A_g | A_u | B_m], r (2D + N1) floats, +0's aug columns maintained by ucod_lora_mlp_pair_pack --
 *                          and all three passes run ucod_layernorm_lora_mlp_pair / ucod_lora_mlp_pair_grad / ucod_layernorm_bwd_lora_mlp_pair where they ran the
 *                          single module's kernels (dropout key L + l, projections 0 and 1).  The last layer's r (2D + N1) gradients are written as zeros.
 *   UCOD_LORA_WIDE         (defined above; full_model.py:47-72) the pass sizes and runs the MLP and fc2 modules through the _wide row entry points, so TM may have
 *                          N1 up to UCOD_LORA_WIDE_MAX_N1 and TO's fc2 slots F up to UCOD_LORA_WIDE_MAX_K (vith16plus: 10240 and 5120).  Valid only where a table
 *                          needs it -- TM with N1 > 8192, or fc2 slots with F > 4096 -- else UCOD_EINVAL, sizes 0: a pass the narrow forms cover has one spelling. */
#define UCOD_LORA_OUT_SWIGLU 1
#define UCOD_LORA_MLP_PAIR 4
size_t ucod_vit_train_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* mlp_table_host,
                                                  const void* const* out_table_host);
int ucod_vit_forward_train_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* table_host, const void* const* train_table_host,
                                       const void* const* mlp_table_host, const void* const* out_table_host, const float* img, float* key_out, void* workspace,
                                       size_t workspace_bytes, void* stream);
int ucod_vit_backward_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* table_host, const void* const* train_table_host,
                                  const void* const* mlp_table_host, const void* const* out_table_host, const float* dkey, void* workspace, size_t workspace_bytes,
                                  void* stream);
size_t ucod_vit_lora_infer_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* mlp_table_host,
                                                       const void* const* out_table_host);
int ucod_vit_forward_lora_infer_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* table_host, const void* const* train_table_host,
                                            const void* const* mlp_table_host, const void* const* out_table_host, const float* img, float* key_out, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* LoRA bias="lora_only" (models/modules/full_model.py:53,66: `bias` of lora_cfg is handed to peft's LoraConfig; "lora_only" sets requires_grad on the bias of every
 * module that carries an adapter and has a bias, and changes nothing else: forward = base(x) + scaling * B(A(drop(x))) with the base layer's own bias, which
 * dropout does not touch).  For y = x W^T + b the bias gradient is the column sum over token rows of y's cotangent.
 *
 * ucod_colsum_det (full_model.py:53,66; csrc/colsum.hip): out[n] = col_scale[n] * sum_{m < M} x[m][n] for n < N, accumulated in f32; col_scale NULL = ones.  x is
 * [M, ld] row-major, elem = UCOD_ROPE_ELEM_HALF (the library's 16-bit operand type) or UCOD_ROPE_ELEM_F32; ld >= N in elements and ld * sizeof(element) a multiple
 * of 16 (the rule of ucod_rope_qk_ld); x 16-byte aligned; columns N .. ld - 1 are never read.  `out` [N] is overwritten.  Deterministic, no floating-point
 * atomics: slabs = min(128, ceil(M / 64)) -- a function of M alone -- row slabs of ceil(M / slabs) rows; inside a slab a thread adds rows rt, rt + 16, ... of its
 * 16-byte column vector in ascending order, the sixteen row threads of a column are added in ascending rt, the workgroup stores workspace[slab][n] (f32
 * [slabs][N]), and a second launch adds the slabs in ascending order, multiplies by col_scale and stores.  Two runs are bit-identical.
 * ucod_colsum_det_workspace_bytes (full_model.py:53,66): slabs * N * 4, or 0 for M < 1 or N % 8 != 0 (N < 8 included).
 * UCOD_EINVAL before any launch, nothing written: a null x / out / workspace, an unknown elem, M < 1, N % 8 != 0, ld < N, a misaligned ld or x, a workspace that is
 * too small.  Both builds. */
size_t ucod_colsum_det_workspace_bytes(int M, int N);
int ucod_colsum_det(const void* x, int elem, int M, int N, int ld, const float* col_scale, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The backward with trained biases (full_model.py:53,66): ucod_vit_backward_lora_out_ex plus TB = bias_table_host, HOST array of DEVICE pointers, layer l at
 * UCOD_VIT_TRAIN_BIAS_STRIDE*l:
 *     +0 gb_q f32 [D]   +1 gb_k [D]   +2 gb_v [D]   +3 gb_m [N1] (fc1 / weights_in; SwiGLU: the engine's padded, interleaved order)   +4 gb_o [D] (dense / o_proj)
 *     +5 gb_2 [D] (fc2 / weights_out / down_proj);  NULL = that bias is not trained (a module without a bias in the checkpoint, or one that is not targeted)
 * Every non-NULL slot is overwritten with one ucod_colsum_det per layer below the last:
 *   gb_q / gb_k / gb_v  the thirds of dqkv_aug [M, 3D+64] (columns 0 / D / 2D, ld = 3D+64) behind ucod_attention_bwd and the DINOv3 un-rotation, in front of
 *                       ucod_lora_grad: the cotangents of the projection outputs (the softmax pre-scale is applied behind the bias, and attention backward
 *                       returns dq of the unscaled q); when all three slots are set and lie side by side (gb_k = gb_q + D, gb_v = gb_q + 2 D, as one arena row
 *                       holds them) they are written by ONE call over the 3 D columns
 *   gb_m                the completed dpre [M, N1], behind ucod_lora_out_grad_x_ex, in front of ucod_layernorm_lora_mlp / the fc1 dgrad
 *   gb_o, gb_2          the residual GEMMs compute x += lambda * (acc + b), so db = lambda * sum_rows dx: the column sums of s = bf16(lambda * dx), the operand of
 *                       the out-proj / fc2 dgrad GEMM, with no col_scale -- gb_2 at the top of the layer (before h2_aug reuses s's buffer), gb_o behind the
 *                       LayerNorm-2 backward that writes s
 * In the last layer only the key projection reaches the key map: gb_k there is the column sum of what ucod_key_grad_tokens_reg scattered (CLS and register rows
 * are zeros), the other five slots are written as zeros.  The partials of ucod_colsum_det (sized for its widest calls, N = 3 D and N = N1) are one more entry at the end of the
 * workspace, counted only with a non-NULL table: ucod_vit_train_workspace_bytes_lora_bias (full_model.py:53,66) with NULL returns the bytes of ucod_vit_train_workspace_bytes_lora_out_ex, and
 * ucod_vit_backward_lora_bias with NULL enqueues its launches; every older backward / size entry point delegates here with NULL.  ucod_vit_forward_train_lora_out_ex
 * must have been given a workspace of at least the _lora_bias size (it uses the leading bytes).  The forward passes need no new entry point: they read biases
 * from table_host. */
#define UCOD_VIT_TRAIN_BIAS_STRIDE 6
size_t ucod_vit_train_workspace_bytes_lora_bias(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* mlp_table_host,
                                                const void* const* out_table_host, const void* const* bias_table_host);
int ucod_vit_backward_lora_bias(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* table_host, const void* const* train_table_host,
                                const void* const* mlp_table_host, const void* const* out_table_host, const void* const* bias_table_host, const float* dkey,
                                void* workspace, size_t workspace_bytes, void* stream);

/* LoRA bias="all" (models/modules/full_model.py:53,66: peft sets requires_grad on every parameter with "bias" in its name -- the LayerNorm betas, the patch
 * embedding's bias and the bias of every Linear, targeted or not; nothing else changes).  Two more column sums and a further tier of the backward.
 *
 * ucod_colsum_det_lora (full_model.py:53,66; csrc/vit_train.hip, beside ln_bwd_kernel, on its Drop / drop_scale): the gradient of a LayerNorm's beta, where the
 * LayerNorm backward adds the masked LoRA branch to dy in registers and the complete cotangent never reaches memory:
 *   out[n] = sum_{m < M} ( dy[m][n] + sum_{p < np} drop_scale_p(m D + n) * sum_{j < r} t_p[m][j] * A_p[j][n] ),  n < D
 * with the operands of ucod_layernorm_bwd_lora_ex / _lora_mlp / _lora_mlp_pair: dy [M, D] bf16 (flags & UCOD_LNB_DY_BF16) or f32 (UCOD_LNB_X_F16 is accepted and
 * means nothing here), 16-byte aligned; t bf16 at t_bf16[m * ldt + p * r + j] (for q / k / v the caller passes dqkv_aug + 3 D with ldt = 3 D + 64); A_p at
 * lora + p * astride, astride = 2 r D for np = 3 (one layer's [A_q | B_q | A_k | ...]) and r D for np = 1 / 2 (A_m; [A_g | A_u]), 8-byte aligned; mask p of the
 * dropout descriptor (NULL or p = 0: scale 1).  np in {1, 2, 3}; np * r <= 64 for np = 3, r <= UCOD_LORA_MLP_MAX_R otherwise.  t_bf16 NULL: no branch (lora, np, r,
 * ldt and dropout are not looked at) and the result is ucod_colsum_det's on the same dy, bit for bit.
 * Deterministic by ucod_colsum_det's rule: slabs = min(128, ceil(M / 64)), a thread adds its rows in ascending order, the sixteen row threads in ascending order, a
 * second launch the slabs in ascending order; no floating-point atomics; two runs are bit-identical.  r = 2 and r = 4 (and r = 8 with one or two modules) keep the thread's A vectors
 * in registers across its rows and read t two values per load (t 4-byte aligned, ldt even); other ranks take a generic loop.  workspace: ucod_colsum_det_lora_workspace_bytes (full_model.py:53,66) = slabs * D * 4, or 0 for M < 1 or
 * D % 128 != 0.  UCOD_EINVAL before any launch, nothing written: a null dy / out / workspace, unknown flag bits, M < 1, D % 128 != 0, a misaligned pointer, a
 * workspace that is too small and, with t_bf16 set, a null lora, np or r out of range, ldt < np * r, p outside [0, 1).  bf16 library only.
 *
 * ucod_colsum_det_tok (full_model.py:53,66; csrc/colsum.hip): the patch embedding's bias gradient -- the column sums over the patch rows only (CLS and register
 * rows are no conv outputs):  out[n] = col_scale[n] * sum_{b < B} sum_{first <= i < tok} x[b * tok + i][n].  Element types, pitch, alignment and refusals of
 * ucod_colsum_det; additionally refuses first < 0 or first >= tok.  slabs = min(128, ceil(B (tok - first) / 64)) over the selected rows in ascending order; with
 * first = 0 the bits of ucod_colsum_det at M = B tok.  ucod_colsum_det_tok_workspace_bytes (full_model.py:53,66): slabs * N * 4, or 0.  Both builds. */
size_t ucod_colsum_det_lora_workspace_bytes(int M, int D);
int ucod_colsum_det_lora(const void* dy, int flags, int M, int D, const void* t_bf16, int ldt, const float* lora, int np, int r, const ucod_lora_dropout* dropout,
                         float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t ucod_colsum_det_tok_workspace_bytes(int B, int tok, int first, int N);
int ucod_colsum_det_tok(const void* x, int elem, int B, int tok, int first, int N, int ld, const float* col_scale, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The backward with trained LayerNorm and patch-embedding biases (full_model.py:53,66): ucod_vit_backward_lora_bias plus TN = norm_table_host, HOST array of
 * 1 + 2 L DEVICE pointers:  [0] gb_patch f32 [D]   [1 + 2 l] g_beta1 of layer l [D]   [2 + 2 l] g_beta2 of layer l [D];  NULL = not trained.
 *   g_beta1[l]  every layer, behind the QKV dgrad that leaves dh: ucod_colsum_det of dh with dropout off (the branch rode on the GEMM), ucod_colsum_det_lora with
 *               np = 3 over dh, the aug columns of dqkv_aug and the layer's arena row with dropout on -- the operands of the LayerNorm-1 backward
 *   g_beta2[l]  l < L - 1, behind the fc1 dgrad: ucod_colsum_det_lora with np = 1 (2 with UCOD_LORA_MLP_PAIR) over dh, the t scratch and the module's A when the
 *               pass has an MLP table, ucod_colsum_det otherwise; the last layer's is written as zeros (its MLP never runs)
 *   gb_patch    with this slot set the LayerNorm-1 backward also runs at layer 0 (dres = dx, or NULL for L = 1; no column scale, no 16-bit copy), and
 *               ucod_colsum_det_tok sums the first residual state's cotangent dx over the patch rows (first = 1 + n_reg)
 * The six Linear slots of TB are filled as before.  The partials share TB's entry of the workspace, which is sized for the widest call of either table and counted
 * only with a non-NULL table.  A NULL TN is ucod_vit_backward_lora_bias launch for launch and byte for byte; every older entry point delegates with NULL. */
size_t ucod_vit_train_workspace_bytes_lora_bias_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* mlp_table_host,
                                                   const void* const* out_table_host, const void* const* bias_table_host, const void* const* norm_table_host);
int ucod_vit_backward_lora_bias_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* table_host, const void* const* train_table_host,
                                   const void* const* mlp_table_host, const void* const* out_table_host, const void* const* bias_table_host,
                                   const void* const* norm_table_host, const float* dkey, void* workspace, size_t workspace_bytes, void* stream);

/* The way out of LoRA mode: merging the trained matrices into ordinary weights (csrc/lora_merge.hip), so that every frozen-backbone engine runs the adapted model.
 * peft's merge of a LoRA module (what merge_and_unload() does to each module models/modules/full_model.py:47-72 wraps):  W <- W + (lora_alpha / r) B A.
 *   out[n][k] = f32( f64(w0[n][k]) + f64(scaling) * sum_{j < r, ascending} f64(B[n][j]) * f64(A[j][k]) )
 * w0, out f32 [N, K] (distinct buffers); A f32 [r, K]; B f32 [N, r]; scaling = lora_alpha / r.  The kernel does not know the row order: the caller passes w0 and B in
 * the same one (HF order for an export; the engine's padded, interleaved weights_in order for an in-place refresh, where the padded rows of B are zero and come out
 * as w0's zeros).  In f64 every product of two f32 values is exact, so the result does not depend on FMA formation; one HBM pass over the weight.
 * UCOD_EINVAL before any launch: a null pointer, r < 1, r > UCOD_LORA_AUG / 3, N < 1, K % 64 != 0 (or K < 64), w0 / A / out not 16-byte aligned.  Both builds. */
int ucod_lora_merge_f32(const float* w0, const float* A, const float* B, int r, float scaling, float* out, int N, int K, void* stream);
/* The device form of the LayerNorm fold (fold.py: fold_layernorm_linear; ucod_gemm_lnfold's operands) for a weight that was just merged by ucod_lora_merge_f32
 * (full_model.py:47-72; W + (lora_alpha / r) B A is `w` here), with the host's rounding sequence, q[n] = row_scale[n] or 1:
 *   wf[n][k]  = fp16( f32( (f64(w[n][k]) * f64(gamma[k])) * f64(q[n]) ) )          colsum[n] = f32( sum_k f64(wf[n][k]) )   (of the ROUNDED values; exact in f64)
 *   bias_f[n] = f32( (sum_k f64(w[n][k]) * f64(beta[k]) + f64(b[n])) * f64(q[n]) )                                          (f64 partial sums, shuffle reduce)
 * w f32 [N, K]; gamma, beta f32 [K]; b f32 [N]; row_scale f32 [N] or NULL; wf fp16 [N, K]; bias_f, colsum f32 [N].  libucod_dpl_f16.so only -- the bf16 build
 * returns UCOD_EINVAL, like ucod_gemm_lnfold.  UCOD_EINVAL also for a null pointer, N < 1, K % 64 != 0 (or K < 64), w / gamma / beta not 16-byte aligned. */
int ucod_fold_ln_linear(const float* w, const float* gamma, const float* beta, const float* b, const float* row_scale_or_null, void* wf_f16, float* bias_f,
                        float* colsum, int N, int K, void* stream);

/* ------------------------------------------------------------------ decoder / APM path (rows A1-A8) */

/* F.interpolate(mode='bilinear', align_corners=False) on `planes` independent [ih,iw] maps
 * (engine/runner/loop_UCOD_DPL.py:153-154,236,241,305,315,356-358). */
int ucod_bilinear_resize(const float* in, float* out, int planes, int ih, int iw, int oh, int ow, void* stream);
/* Transpose of the above: gin [planes,ih,iw] = U^T gout [planes,oh,ow] (same taps and weights as the forward).  The
 * training step runs the 1x1 decoupling conv and its weight gradient on the backbone's native 37x37 grid and moves
 * d / gd across the resize instead of the 768-channel features (conv and resize commute).  UCOD_EINVAL when a source index
 * of either axis can be reached by more than 16 outputs: min(ceil(2 out / in) + 1, out) > 16, up-sampling beyond 7.5x. */
int ucod_bilinear_resize_adjoint(const float* gout, float* gin, int planes, int ih, int iw, int oh, int ow, void* stream);

/* 1x1 "decoupling" conv as an exact-f32 MFMA GEMM (models/modules/DBA.py:13,35):
 * d[b][n][p] = sum_c W[n][c]*x[b][c][p] + bias[n];  x [B,C,HW], W [Nout,C], d [B,Nout,HW].
 * Nout = 128 (one decoder) or 256 (student rows 0..127 | teacher rows 128..255 sharing the x read). */
int ucod_dba_project(const float* x, const float* W, const float* bias, float* d, int B, int C, int HW, int Nout,
                     void* stream);
/* The same contraction on the bf16 matrix pipe with every f32 operand split into three bf16 terms (24 significand bits) and the six
 * partial products of weight >= 2^-16 accumulated in f32: f32-equivalent (what is dropped is below 2^-24 |W x| per term, the rounding of
 * an f32 FMA chain), 2.7x less matrix-pipe time than v_mfma_f32_32x32x2_f32.  C % 16 == 0, Nout = 128 or 256.
 * ws: ucod_dba_project_split_workspace_bytes(C, Nout) bytes, 16-byte aligned (the pre-split W planes). */
size_t ucod_dba_project_split_workspace_bytes(int C, int Nout);
int ucod_dba_project_split(const float* x, const float* W, const float* bias, float* d, void* ws, size_t ws_bytes, int B, int C, int HW,
                           int Nout, void* stream);

/* L2 norm over the PIXEL axis of (d * emb) per (image, channel), clamped at 1e-12
 * (F.normalize(dim=1) on [B,HW,64], DBA.py:40-41).  d is a [B, ld_c, HW] buffer, channels c0..c0+127 used;
 * emb [2,64] -> channel c scales by emb[c/64][c%64].  norm out [B,128]. */
int ucod_dba_colnorm(const float* d, int ld_c, int c0, const float* emb, float* norm, int B, int HW, void* stream);

/* gate + heads (DBA.py:48-52): a = sigmoid(f*d)+d, fg = w_fg.a1 + b_fg, bg = w_bg.a2 + b_bg, f = d*emb/norm.
 * head_w [2,64] = (conv_out_fg.weight, conv_out_bg.weight), head_b [2].  fg,bg [B,HW] (bg may be NULL).
 * sdiag (may be NULL) [B] receives sum_p (f1_p . f2_p)^2, the diagonal term of the orthogonality loss. */
int ucod_dba_heads_fwd(const float* d, int ld_c, int c0, const float* emb, const float* norm, const float* head_w,
                       const float* head_b, float* fg, float* bg, float* sdiag, int B, int HW, void* stream);

/* Orthogonality loss in Gram form (DBA.py:25-29 rewritten):
 * gram [B,2,64,64] (G1,G2 of the normalised features), sdiag [B] = sum_i (f1_i.f2_i)^2 from ucod_dba_heads_fwd,
 * loss[0] = (sum_b tr(G1 G2) - sum_b sdiag[b]) / (B*HW*HW).  ws: ucod_orth_workspace_bytes. */
size_t ucod_orth_workspace_bytes(int B, int HW);
int ucod_orth_gram_fwd(const float* d, int ld_c, int c0, const float* emb, const float* norm, const float* sdiag,
                       float* gram, float* loss, void* ws, int B, int HW, void* stream);

/* Backward of heads + gate + HW-axis normalisation + Gram orthogonality loss w.r.t. d (closed form,
 * SURVEY.md section 7).  gfg,gbg [B,HW] upstream logit grads, gextra = dL/d(extra_loss).
 * Outputs: gd [B,128,HW]; g_head_w [2,64], g_head_b [2], g_dec_bias [128] (each zeroed inside, then accumulated).
 * The gradient of learnable_embedding is analytically zero (its scale cancels under the HW-axis normalisation;
 * the reference's autograd value is f32 cancellation noise) and is not produced. */
size_t ucod_dba_bwd_workspace_bytes(int B, int HW);
int ucod_dba_bwd(const float* d, int ld_c, int c0, const float* emb, const float* norm, const float* head_w,
                 const float* gram, const float* gfg, const float* gbg, float gextra, float* gd, float* g_head_w,
                 float* g_head_b, float* g_dec_bias, void* ws, int B, int HW, void* stream);

/* weight gradient of the decoupling conv: gW[n][c] += sum_{b,p} gd[b][n][p]*x[b][c][p]  (f32 MFMA, split-K
 * over (b, pixel chunks) with f32 atomics into gW [128,C], which is zeroed inside first). */
int ucod_dba_wgrad(const float* gd, const float* x, float* gW, int B, int C, int HW, void* stream);
/* The same weight gradient on the bf16 matrix pipe, both operands split into three bf16 terms while staged (see ucod_dba_project_split:
 * f32-equivalent); split-K over (image, pixel chunk) with f32 atomics, gW zeroed inside first. */
int ucod_dba_wgrad_split(const float* gd, const float* x, float* gW, int B, int C, int HW, void* stream);

/* APM discriminator forward, always train-mode BatchNorm (models/discriminator.py:60-70,86-95;
 * dis_use_features=False).  params (f32, reference state_dict order):
 *   w1 [32,1,3,3] g1 b1 [32]  w2 [16,32,3,3] g2 b2 [16]  w3 [8,16,3,3] g3 b3 [8]  lin_w [8*ceil(fs/4)^2] lin_b [1]
 * running = (rm1,rv1,rm2,rv2,rm3,rv3) updated in place with momentum 0.1 when update_running != 0.
 * mask [B,1,fs,fs] -> prob [B].  `saved` (ucod_disc_saved_bytes) keeps pre-BN activations + batch statistics
 * for ucod_disc_bwd. */
typedef struct {
  const float *w1, *g1, *b1, *w2, *g2, *b2, *w3, *g3, *b3, *lin_w, *lin_b;
  float *rm1, *rv1, *rm2, *rv2, *rm3, *rv3;
  long long* nbt; /* ABI 3: the three num_batches_tracked counters as ONE int64[3] (or NULL): += 1 per call with update_running */
} ucod_disc_params;
size_t ucod_disc_saved_bytes(int B, int fs);
int ucod_disc_fwd(const float* mask, const ucod_disc_params* p_host, float* prob, void* saved, int B, int fs,
                  int update_running, void* stream);
/* gradient of sum_b gprob[b]*prob[b] w.r.t. the 11 parameter tensors, written (not accumulated unless
 * accumulate != 0) into grads laid out in the same order/shapes as ucod_disc_params' const members.
 * (engine/runner/loop_UCOD_DPL.py:244-251) */
typedef struct { float *w1, *g1, *b1, *w2, *g2, *b2, *w3, *g3, *b3, *lin_w, *lin_b; } ucod_disc_grads;
size_t ucod_disc_bwd_workspace_bytes(int B, int fs);
int ucod_disc_bwd(const float* mask, const ucod_disc_params* p_host, const void* saved, const float* gprob,
                  const ucod_disc_grads* g_host, int accumulate, void* ws, int B, int fs, void* stream);

/* APM fusion + both BCE-with-logits losses + their logit gradients in one pass
 * (engine/runner/loop_UCOD_DPL.py:257-272 and :161-173):
 *   w[b] = clamp(0.5*(1+cos(pi*|p_s-p_p|)) + epoch_frac, 0, 1);  merged = pl*(1-w) + (sigmoid(teacher)>0.5)*w
 *   losses[0] = mean BCEWithLogits(fg, merged), losses[1] = mean BCEWithLogits(bg, 1-merged),
 *   losses[2] = dis_loss = mean BCE(p_s, 0);  gfg = (sigmoid(fg)-merged)/(B*HW)*gscale, gbg likewise.
 * pl, teacher, fg, bg, merged, gfg, gbg: [B,HW]; p_s, p_p, w: [B].  losses [4] (zeroed inside; [3] unused). */
int ucod_apm_bce(const float* pl, const float* teacher, const float* fg, const float* bg, const float* p_s,
                 const float* p_p, float epoch_frac, float gscale, float* w, float* merged, float* gfg, float* gbg,
                 float* losses, int B, int HW, void* stream);
/* out[i] = (sigmoid(x[i]) > 0.5) when logits != 0, else (x[i] > 0.5), as 0/1 floats (loop_UCOD_DPL.py:240-241,258-261) */
int ucod_binarize(const float* x, float* out, size_t n, int logits, void* stream);

/* torch.optim.AdamW step + EMA teacher update over a flat f32 arena
 * (engine/runner/runner.py:282-298; loop_UCOD_DPL.py:178,186-191).  ema may be NULL. */
/* loss of TrainLoop._process_batch (loop_UCOD_DPL.py:161-169): out[0] = losses[0] + losses[1] + extra[0] (- losses[2] unless finetune), from
 * the four scalars ucod_apm_bce left in `losses` and the orthogonality loss -- one launch instead of three elementwise adds (ABI 3). */
int ucod_step_loss(const float* losses, const float* extra, int finetune, float* out, void* stream);
/* dst[q][0..n[q]) = src[q][0..n[q]) for q < count <= 4, one launch (host arrays of device pointers / element counts; f32).  What
 * loop_UCOD_DPL.py's refresh of the shared student | teacher projection needs per step instead of four device-to-device copies. */
int ucod_copy_segments(float* const* dst, const float* const* src, const size_t* n, int count, void* stream);
/* One launch that zeroes up to eight device regions (HOST arrays of DEVICE pointers and byte counts, 4-byte aligned): the accumulating outputs of a
 * whole step at once.  Together with ucod_accumulators_prezeroed it replaces the memset each accumulating entry point otherwise issues in front of
 * its kernel (round 4: seven rocclr fills among the ~125 launches of a student step). */
int ucod_zero_segments(void* const* dst, const size_t* bytes, int count, void* stream);
/* on != 0: for the calls issued NEXT FROM THIS HOST THREAD the caller guarantees that these outputs are already zero (ucod_zero_segments), and the entry
 * points skip their own memset: `sdiag` of ucod_dba_heads_fwd, `losses` of ucod_apm_bce, g_head_w / g_head_b / g_dec_bias of ucod_dba_bwd, `gW` of
 * ucod_dba_wgrad / ucod_dba_wgrad_split, and the last 112 doubles of ucod_disc_fwd's `saved` buffer (its BatchNorm sums -- which every ucod_disc_fwd call
 * also LEAVES zero, so a saved buffer that was allocated zeroed stays valid call after call).  Host-side state, like ucod_resid16_overflow_bind: set it,
 * issue the step, clear it. */
int ucod_accumulators_prezeroed(int on);
int ucod_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float ema_alpha, void* stream);

/* Discriminator WITH the feature branch (models/discriminator.py:77-95, dis_use_features=True; no shipped config enables it): forward only, from
 * generic pieces.  A ConvBlock(Cin, Cout, 3, stride, 1) is  ucod_unfold3x3 -> ucod_dba_project(W.reshape(Cout, Cin*9) zero-padded to Kpad columns,
 * zero bias) -> ucod_bn_lrelu_train.
 * ucod_unfold3x3: x f32 [B,C,H,W] -> out f32 [B,Kpad,Ho*Wo], row c*9 + ky*3 + kx = the input shifted by (ky-1, kx-1) with zero padding (F.unfold
 *   order), rows >= C*9 zero; Ho = (H-1)/stride + 1; stride 1 or 2; Kpad % 16 == 0 for the GEMM.
 * ucod_bn_lrelu_train: y f32 [B,C,HW] in place: training-mode nn.BatchNorm2d (batch statistics, biased variance; running buffers updated with
 *   `momentum` and the unbiased variance when update_running != 0) followed by LeakyReLU(slope).  Statistics in f64, deterministic.
 * ucod_linear_sigmoid: out[b] = sigmoid(x[b,:] . w + bias[0]). */
int ucod_unfold3x3(const float* x, float* out, int B, int C, int H, int W, int stride, int Kpad, void* stream);
size_t ucod_bn_lrelu_workspace_bytes(int C);
int ucod_bn_lrelu_train(float* y, const float* gamma, const float* beta, float* running_mean, float* running_var, int B, int C, int HW, float eps,
                        float momentum, float slope, int update_running, void* workspace, size_t workspace_bytes, void* stream);
int ucod_linear_sigmoid(const float* x, const float* w, const float* bias, float* out, int B, int K, void* stream);
/* Training that discriminator (the discriminator phase, engine/runner/loop_UCOD_DPL.py:230-255, with dis_use_features=True): the backward of the
 * same pieces.  A ConvBlock's backward is  ucod_bn_lrelu_bwd -> ucod_conv_wgrad_f32 (weight gradient from the saved unfold) -> [input gradient:
 * ucod_dba_project with W^T on the gradient, then ucod_fold3x3].
 * ucod_bn_lrelu_train_save: as ucod_bn_lrelu_train, out of place (y_pre is kept for the backward) and with the batch statistics left in `stats`
 *   (ucod_bn_lrelu_workspace_bytes(C) bytes, owned by the caller until the backward has run).
 * ucod_bn_lrelu_bwd: gout = dL/d(block output) -> gy_pre = dL/d(conv output); dgamma / dbeta written, or added to when accumulate != 0 (the phase
 *   calls the discriminator twice per step).  f64 sums in a fixed order.
 * ucod_fold3x3: the adjoint of ucod_unfold3x3 (col2im): gcols [B,Kpad,Ho*Wo] -> gx [B,C,H,W].
 * ucod_conv_wgrad_f32: gW [Nout,C] (+)= sum_{b,p} gd[b][n][p] * cols[b][c][p]  (exact-f32 MFMA, split over pixel chunks, f32 atomics).
 * ucod_linear_sigmoid_bwd: gprob = dL/dprob -> gx [B,K], gw [K], gb [1] (written or accumulated).
 * ucod_disc_bce: nn.BCELoss(cat(probs_student, probs_pseudo), [0..0, 1..1]) (mean over 2B, logs clamped at -100 like torch) -> loss[0], and its
 *   gradient times `inv` / (the mean's 1 / 2B is part of inv = 1 / (2 B world)) with torch's max(p (1 - p), 1e-12) denominator. */
int ucod_bn_lrelu_train_save(const float* y_pre, float* y_out, const float* gamma, const float* beta, float* running_mean, float* running_var, int B, int C,
                             int HW, float eps, float momentum, float slope, int update_running, void* stats, size_t stats_bytes, void* stream);
int ucod_bn_lrelu_bwd(const float* y_pre, const float* gout, float* gy_pre, const void* stats, const float* gamma, const float* beta, float* dgamma,
                      float* dbeta, int B, int C, int HW, float eps, float slope, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int ucod_fold3x3(const float* gcols, float* gx, int B, int C, int H, int W, int stride, int Kpad, void* stream);
int ucod_conv_wgrad_f32(const float* gd, const float* cols, float* gW, int B, int C, int HW, int Nout, int accumulate, void* stream);
int ucod_linear_sigmoid_bwd(const float* x, const float* w, const float* prob, const float* gprob, float* gx, float* gw, float* gb, int B, int K,
                            int accumulate, void* stream);
int ucod_disc_bce(const float* probs_student, const float* probs_pseudo, float* g_student, float* g_pseudo, float* loss, int B, float inv, void* stream);
/* The gradient INTO the features (backbone-backward mode with dis_use_features=True: the student's features are trained, so the step's loss reaches them
 * through the discriminator's featureConv as well).
 * ucod_conv3x3_f32: a 3x3 / stride 1 / pad 1 convolution without the unfold buffer.  x f32 [B,C,H,W], Wmat f32 [Nout,Kpad] row-major with column
 *   c*9 + ky*3 + kx (F.unfold order; Kpad % 16 == 0, Kpad >= 9C, 16-byte aligned) -> y f32 [B,Nout,H*W].  The tile, K order and K-tiling of ucod_dba_project
 *   with the rows of every K-tile gathered straight from x (zero padding by select): the SAME MFMAs on the same values in the same order as ucod_unfold3x3
 *   (stride 1) followed by ucod_dba_project with a zero bias, so y equals that route's bit for bit.  No atomics, no split-K: deterministic.  A NULL pointer,
 *   a non-positive size, a bad Kpad or a misaligned Wmat returns UCOD_EINVAL before anything is launched.
 * ucod_conv3x3_dgrad_weights: W f32 [Cout,Cin,3,3] -> Wd f32 [Cin,Kpad], Kpad = 16 * ceil(9 Cout / 16):  Wd[ci][co*9 + t] = W[co][ci][8 - t], columns
 *   >= 9 Cout zero (a copy: exact).  The data gradient of the pad-1 convolution y = conv(x; W) is the pad-1 convolution of gy with both spatial axes of the
 *   kernel flipped and the channel axes exchanged:  gx = ucod_conv3x3_f32(gy, Wd)  -- no [B, 9C, HW] buffer, no fold pass.
 * ucod_apm_bce_gprob: the step loss's gradient with respect to the two discriminator probabilities (ucod_apm_bce holds them constant).  With D = p_s - p_p,
 *   u = 0.5 (1 + cos(pi |D|)) + epoch_frac, tb = sigmoid(teacher) > 0.5 (binarised as in ucod_apm_bce):
 *     gw[b]   = 1/(B HW) sum_p (bg - fg)[b,p] (tb - pl)[b,p]        (d/dt BCEWithLogits(x, t) = -x; the bg term's target is 1 - merged)
 *     dw/dD   = -0.5 pi sin(pi |D|) sign(D) when 0 <= u <= 1, else 0 (inclusive, as torch's clamp backward; sign(0) = 0 as torch's abs)
 *     gp_p[b] = -gscale gw[b] dw/dD
 *     gp_s[b] = +gscale gw[b] dw/dD  [ - gscale (1/B) p_s / max(p_s (1 - p_s), 1e-12)  when finetune == 0: `loss -= dis_loss`, torch's BCELoss backward at target 0 ]
 *   One workgroup per image, the HW sum in a fixed order: deterministic. */
int ucod_conv3x3_f32(const float* x, const float* Wmat, float* y, int B, int C, int H, int W, int Nout, int Kpad, void* stream);
int ucod_conv3x3_dgrad_weights(const float* W, float* Wd, int Cout, int Cin, int Kpad, void* stream);
int ucod_apm_bce_gprob(const float* pl, const float* teacher, const float* fg, const float* bg, const float* p_s, const float* p_p, float epoch_frac,
                       float gscale, int finetune, float* gp_s, float* gp_p, int B, int HW, void* stream);

/* ------------------------------------------------------------------ Deterministic forms of the training step
 *
 * The entry points above sum across workgroups with floating-point atomics in seven places (the two weight-gradient kernels, sdiag of the heads kernel, the three
 * small gradients of ucod_dba_bwd, the loss cells of ucod_apm_bce, the BatchNorm sums of ucod_disc_fwd, the Linear gradients of ucod_disc_bwd): their results
 * depend on the order in which workgroups retire and differ from run to run in the last bits.  A `_det` form executes NO floating-point atomic: every workgroup
 * stores its partial to a cell of its own in a caller-provided workspace, and a following launch adds the cells in an order that is a pure function of the
 * problem shape -- never of a device query, an environment variable or ucod_accumulators_prezeroed.  Two calls on equal inputs give equal bits.
 *
 * Common rules: `ws` is `*_det_workspace_bytes(...)` bytes (0 = the shape is invalid), 4-byte aligned (8 for ucod_disc_fwd_det); nothing is allocated inside; a NULL
 * pointer, an invalid shape or a workspace that is too small returns UCOD_EINVAL before anything is launched or written.  Outputs are WRITTEN: what they held
 * before (NaN included) does not matter, and ucod_accumulators_prezeroed is not consulted.  Every output the default form computes without an atomic (fg, bg, gd, w,
 * merged, gfg, gbg, the pre-BN activations ...) is bit-identical to the default form's: same kernel body, same arithmetic.
 *
 * ucod_dba_wgrad_det: gW [128,C] = sum_{b,p} gd[b][n][p] x[b][c][p].  exact = 0: the three-term bf16 kernel of ucod_dba_wgrad_split; exact != 0: the f32-MFMA kernel of
 *   ucod_dba_wgrad.  SUMMATION ORDER (part of the contract): the pixel axis is cut into nchunk chunks; workgroup (image b, chunk) stores its f32 accumulator tile
 *   with plain vector stores to plane q = b * nchunk + chunk of ws, laid out ws[q][n][c] (n = weight-gradient row, c = feature channel; Q = B * nchunk planes,
 *   Q = workspace_bytes / (4 * 128 * C)); a second launch then writes, one thread per element,
 *       gW[n][c] = (accumulate ? gW[n][c] : 0) + ws[0][n][c] + ws[1][n][c] + ... + ws[Q-1][n][c]
 *   sequentially in ascending q, in f32 (ucod_dba_wgrad_det never accumulates).  nchunk depends on (B, C, HW) -- and Nout -- only; it may differ from the atomic form's.
 * ucod_conv_wgrad_f32_det: the same for gW [Nout,C] with any Nout (ws[q][n][c], n < Nout) and the `accumulate` of ucod_conv_wgrad_f32.
 * ucod_dba_heads_fwd_det: sdiag[b] = ws[b][0] + ws[b][1] + ... ascending, ws[b][j] = the share of the j-th 256-pixel workgroup (ws [B][ceil(HW/256)] f32).
 *   ws may be NULL when sdiag is.
 * ucod_dba_bwd_det: ws = the default form's workspace, then the per-image sums part[b][258] = (g_dec_bias terms [128] | g_head_w terms [128] | g_head_b terms [2]);
 *   each gradient is the sum over b ascending.
 * ucod_apm_bce_det: ws[b][3] = image b's terms of losses[0..2]; losses[k] = the sum over b ascending; losses[3] = 0.
 * ucod_disc_fwd_det: the BatchNorm (sum, sum of squares) of each convolution become per-workgroup f64 partials in ws, summed in ascending workgroup order in f64.  The
 *   running statistics and `nbt` behave as in ucod_disc_fwd.  The f64 sums at the end of `saved` are neither read nor written, so a caller may alternate the two forms
 *   on one zero-initialised `saved` buffer.
 * ucod_disc_bwd_det: ws = the default form's workspace, then per-image partials of g.lin_w and g.lin_b, added in ascending b (with the `accumulate` of ucod_disc_bwd). */
size_t ucod_dba_wgrad_det_workspace_bytes(int B, int C, int HW, int exact);
int ucod_dba_wgrad_det(const float* gd, const float* x, float* gW, int B, int C, int HW, int exact, void* ws, size_t ws_bytes, void* stream);
size_t ucod_conv_wgrad_f32_det_workspace_bytes(int B, int C, int HW, int Nout);
int ucod_conv_wgrad_f32_det(const float* gd, const float* cols, float* gW, int B, int C, int HW, int Nout, int accumulate, void* ws, size_t ws_bytes,
                            void* stream);
size_t ucod_dba_heads_fwd_det_workspace_bytes(int B, int HW);
int ucod_dba_heads_fwd_det(const float* d, int ld_c, int c0, const float* emb, const float* norm, const float* head_w, const float* head_b, float* fg,
                           float* bg, float* sdiag, void* ws, size_t ws_bytes, int B, int HW, void* stream);
size_t ucod_dba_bwd_det_workspace_bytes(int B, int HW);
int ucod_dba_bwd_det(const float* d, int ld_c, int c0, const float* emb, const float* norm, const float* head_w, const float* gram, const float* gfg,
                     const float* gbg, float gextra, float* gd, float* g_head_w, float* g_head_b, float* g_dec_bias, void* ws, size_t ws_bytes, int B,
                     int HW, void* stream);
size_t ucod_apm_bce_det_workspace_bytes(int B);
int ucod_apm_bce_det(const float* pl, const float* teacher, const float* fg, const float* bg, const float* p_s, const float* p_p, float epoch_frac,
                     float gscale, float* w, float* merged, float* gfg, float* gbg, float* losses, void* ws, size_t ws_bytes, int B, int HW, void* stream);
size_t ucod_disc_fwd_det_workspace_bytes(int B, int fs);
int ucod_disc_fwd_det(const float* mask, const ucod_disc_params* p_host, float* prob, void* saved, int B, int fs, int update_running, void* ws,
                      size_t ws_bytes, void* stream);
size_t ucod_disc_bwd_det_workspace_bytes(int B, int fs);
int ucod_disc_bwd_det(const float* mask, const ucod_disc_params* p_host, const void* saved, const float* gprob, const ucod_disc_grads* g_host,
                      int accumulate, void* ws, size_t ws_bytes, int B, int fs, void* stream);

/* ------------------------------------------------------------------ Look-Twice (rows L1-L3) */

/* 8-connected component labelling of a HOST uint8 [H,W] mask (non-zero = foreground) into HOST int32 labels
 * (0 = background, k = k-th component in OpenCV's numbering: raster order of the components' first 2 x 2 blocks -- the order in which
 * the block-based labelling of cv2.connectedComponents(connectivity=8) creates and flattens its labels); returns the number of labels
 * INCLUDING the background, like cv2.connectedComponents (engine/runner/loop_UCOD_DPL.py:366).  < 0 on error. */
int ucod_ccl8_host(const uint8_t* mask_host, int H, int W, int32_t* labels_host);

/* Pillow Image.resize on an 8-bit single-channel HOST image: antialiased separable resample with 22-bit fixed-point
 * coefficients, horizontal then vertical pass (filter 0 = BILINEAR, 1 = BICUBIC, the Pillow default used for the
 * 'L' mask at loop_UCOD_DPL.py:350).  Bit-identical to Pillow. */
int ucod_pil_resize_u8_host(const uint8_t* src_host, int h, int w, uint8_t* dst_host, int oh, int ow, int filter);

/* Pseudo-label generator (generate_pseudo_label.py:71-94, data/utils/found_bkg_mask.py:4-86).
 * ucod_vit_last_ln1_offset: byte offset, inside the workspace of ucod_vit_forward (full_last_layer == 0), of the last layer's
 * LayerNorm-1 output bf16 [B*tok, D]; valid until the next pass on that workspace.
 * ucod_cls_qk: q_cls, k_cls f32 [B,D] = that layer's query / key projection of token 0 (qkv_w bf16 [3D,D], qkv_b f32 [3D]).
 * ucod_cls_attention: att f32 [B,heads,hw] = outputs.attentions[-1][:, :, 0, 1:] -- softmax of the CLS query over CLS + all
 * patch keys, patch columns only -- with the patch keys taken from key_map f32 [B, D, hw] (the backbone's NCHW output).
 * ucod_bkg_seg: found_bkg_mask.py:31-86 with up_size = grid: bkg_mask, sim_map f32 [B,hw] (sim_map already multiplied by
 * 1 - bkg_mask and normalised by the batch-wide maximum, :81-82), cos_row f32 [B,hw], seed int32 [B], beta f32 [B,heads];
 * scratch4 = 4 bytes of device scratch. */
size_t ucod_vit_last_ln1_offset(const ucod_vit_desc* d);
int ucod_cls_qk(const void* h_ln1_bf16, const void* qkv_w_bf16, const float* qkv_b, float* q_cls, float* k_cls, int B, int tok, int D, void* stream);
int ucod_cls_attention(const float* q_cls, const float* k_cls, const float* key_map, float* att, int B, int heads, int hw, float scale, void* stream);
/* With register tokens (tok = 1 + n_reg + hw): ucod_cls_qk_reg also projects the keys of tokens 1 .. n_reg into k_lead f32 [B, 1 + n_reg, D] (row 0 = the CLS key);
 * ucod_cls_attention_reg = outputs.attentions[-1][:, :, 0, 1 + n_reg:] -- the softmax runs over all tok keys (the n_reg + 1 of k_lead in its maximum and
 * denominator, the patch keys from the key map), the patch columns are returned, so a row sums to less than 1 by the CLS and register weights.
 * ucod_cls_attention_rope: the same row of a DINOv3 model (rotary position embedding), where the last layer rotates the PATCH keys -- not the CLS query, not the
 * CLS and register keys of k_lead -- before the product.  key_map stays the UNROTATED k_proj output (what the key hook hands out and ucod_bkg_seg reads);
 * cos_sin is the f32 [hw, 64] table of ucod_vit_desc.rope (cos 32 | sin 32 per patch, 16-byte aligned), and patch j scores
 * scale * sum_{i<32} c_j[i] (q[i] k_j[i] + q[i+32] k_j[i+32]) + s_j[i] (q[i+32] k_j[i] - q[i] k_j[i+32]) = scale * q . rotate(k_j): no rotated copy of the key
 * map is formed (the kernel sums it key column by key column against the query turned back by the patch's angles: with zero angles the scores are
 * ucod_cls_attention_reg's bit for bit).  Same grid, threads and LDS as ucod_cls_attention_reg (one kernel, two instantiations), everything f32; UCOD_EINVAL before any launch for a null
 * pointer (cos_sin included), B / heads / hw <= 0, hw > 12000, n_reg < 0 or > 1023, a misaligned table. */
int ucod_cls_qk_reg(const void* h_ln1_bf16, const void* qkv_w_bf16, const float* qkv_b, float* q_cls, float* k_lead, int B, int tok, int D, int n_reg, void* stream);
int ucod_cls_attention_reg(const float* q_cls, const float* k_lead, const float* key_map, float* att, int B, int heads, int hw, int n_reg, float scale, void* stream);
int ucod_cls_attention_rope(const float* q_cls, const float* k_lead, const float* key_map, const float* cos_sin, float* att, int B, int heads, int hw, int n_reg,
                            float scale, void* stream);
int ucod_bkg_seg(const float* att, const float* key_map, float th_bkg, float epsilon, int apply_weights, float* bkg_mask, float* sim_map,
                 float* cos_row, int* seed, float* beta, void* scratch4, int B, int heads, int hw, void* stream);

/* GPU Look-Twice tail.
 * ucod_ccl8_components: 8-connected components of a DEVICE uint8 [H,W] mask (non-zero = foreground) -> a DEVICE table of
 * `*count` rows {root, area, xmin, xmax, ymin, ymax, order} (7 x int32; at most `capacity` rows are written, *count may exceed it),
 * in arbitrary order.  root = linear index of the component's first pixel in raster order; order = raster index of its first 2 x 2
 * block: sorting rows by `order` yields cv2.connectedComponents' label order (labels 1..n, see ucod_ccl8_host) --
 * loop_UCOD_DPL.py:366-384 needs only area and bounding box per label. */
size_t ucod_ccl8_workspace_bytes(int H, int W);
int ucod_ccl8_components(const uint8_t* mask_dev, int H, int W, int32_t* table_dev, int capacity, int32_t* count_dev, void* workspace,
                         size_t workspace_bytes, void* stream);

/* For each box i (HOST int32 [nbox,4] = x,y,w,h in canvas pixels, pasted in order): Pillow-BICUBIC resize of the DEVICE
 * uint8 mask i ([nbox, sh, sw]) to (w,h) and paste into the DEVICE uint8 canvas [CH,CW], clipped to the canvas
 * (Image.resize + Image.paste, loop_UCOD_DPL.py:346-352).  Bit-identical to Pillow.  w,h <= 0 is rejected like PIL does. */
size_t ucod_paste_workspace_bytes(int nbox, int max_w, int max_h, int sh, int sw);
int ucod_paste_resized_u8(const uint8_t* masks_dev, int nbox, int sh, int sw, const int32_t* boxes_host, uint8_t* canvas_dev, int CH, int CW,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The same for boxes that belong to SEVERAL canvases `canvases_dev` u8 [ncanvas,CH,CW] (the batched Look-Twice validation of BASELINE configs[3]: every
 * image of a validation batch in one call): box_canvas_host int32 [nbox] names each box's canvas (NULL: all on canvas 0); boxes are pasted in the order
 * given, so one canvas's boxes keep their order. */
int ucod_paste_resized_u8_multi(const uint8_t* masks_dev, int nbox, int sh, int sw, const int32_t* boxes_host, const int32_t* box_canvas_host,
                                uint8_t* canvases_dev, int ncanvas, int CH, int CW, void* workspace, size_t workspace_bytes, void* stream);

/* Batched crop + Pillow-BILINEAR resize + ToTensor + ImageNet Normalize on the GPU
 * (PIL crop + torchvision Resize/ToTensor/Normalize, loop_UCOD_DPL.py:282-286,341-342).
 * img u8 [H,W,3] (HWC, device); boxes_host int32 [nbox,4] = (x,y,w,h) in source pixels (regions outside the image read
 * as zero, as PIL's crop does); out f32 [nbox,3,oh,ow].  The 8-bit intermediate is bit-identical to Pillow's. */
size_t ucod_crop_workspace_bytes(int nbox, int max_crop_h, int max_crop_w, int oh, int ow);
int ucod_crop_resize_norm(const uint8_t* img, int H, int W, const int32_t* boxes_host, int nbox, float* out, int oh, int ow,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The same for boxes cut from SEVERAL source images in one launch pair ("batch all crops of all images"): imgs_host = HOST array of nimg
 * DEVICE pointers to u8 [H_i,W_i,3] images, hw_host int32 [nimg,2] = (H_i, W_i), box_image_host int32 [nbox] = source image of each box. */
int ucod_crop_resize_norm_multi(const uint8_t* const* imgs_host, const int32_t* hw_host, int nimg, const int32_t* box_image_host,
                                const int32_t* boxes_host, int nbox, float* out, int oh, int ow, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ CORAL SparseRefiner (rows R1-R4), inference */

/* Cross-attention core of nn.MultiheadAttention with head_dim 96 (models/modules/mlp.py:122,143; 8 heads on C=768):
 * softmax(Q K^T) V per (window, head).  q bf16 [B*Nq, ldq] (head h at columns h*96.., PRE-SCALED by 96^-0.5*log2(e));
 * k, v bf16 rows of stride ldkv (may point into one [k|v] buffer); out bf16 [B*Nq, heads*96]. */
int ucod_cross_attention96_fwd(const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv, void* out_bf16,
                               int B, int Nq, int Nk, int heads, void* stream);

/* out[(i*HW + p)*C + c] = src[(src_idx[i]*C + c)*HW + p]: window gather (models/modules/ASR.py:13-20) fused with
 * CSF._BCHW_to_BLC (models/modules/CSF.py:29-31).  src f32 [*,C,HW], src_idx int32 [n] (device), out f32 [n*HW, C]. */
int ucod_gather_tokens(const float* src, const int* src_idx, float* out, int n, int C, int HW, void* stream);

/* EntropySelector scores (models/modules/ASR.py:42-48): entropy = -p*log(max(p,1e-5)) with p = preds (use_sigmoid == 0) or
 * sigmoid(preds); scores = adaptive_avg_pool2d(entropy, (ws,ws)).  preds, entropy f32 [B,1,H,W]; scores f32 [B,ws,ws]. */
int ucod_entropy_scores(const float* preds, int use_sigmoid, float* entropy, float* scores, int B, int H, int W, int ws, void* stream);

/* depthwise 7x7 conv (padding 3, bias) + 1x1 mask head (models/modules/CSF.py:13-25,41-42) on token-major activations:
 * x f32 [n,H,W,C]; dw_tapmajor f32 [49,C] (= depthwise_conv.weight [C,1,7,7] transposed), dw_bias [C], w1 [C], b1;
 * out f32 [n,1,H,W]. */
int ucod_dwconv7_maskdec(const float* x_tokens, const float* dw_tapmajor, const float* dw_bias, const float* w1, float b1, float* out,
                         int n, int H, int W, int C, void* stream);

/* HRE.concate_windows (models/modules/HRE.py:18-39): out f32 [B,1,ws*H,ws*W] = 0, then window i [H,W] placed at
 * (coords[i][0]*H, coords[i][1]*W) of image win_img[i], divided by (1 + 1e-6).  coords int32 [n,2], win_img int32 [n] (device). */
int ucod_window_scatter(const float* windows, const int* coords, const int* win_img, float* out, int n, int B, int H, int W, int ws,
                        void* stream);

/* SparseRefiner.cal_ex_loss, training mode (models/UDLR.py:52-75): the IoU-weighted window loss.  window_preds f32 [n,1,H,W] (logits of
 * the selected windows), h_targets f32 [B*ws*ws,1,H,W] (per-window high-resolution targets, all windows), win_flat int32 [n] = b*ws*ws + j of
 * each selected window (raster order, as mask.flatten() selects), l_up f32 [B,1,ws*H,ws*W] = the first-stage logits resized bilinearly.
 * Per window: l = sigmoid(l_up block) > 0.5; iou of (targets > 0.5 -- after a sigmoid when targets_are_logits, binary_iou's "max > 1"
 * heuristic which the caller evaluates over all selected targets) with l; w = clamp(1.5 iou, 0, 1);
 * part[i] = sum_pixels w BCEWithLogits(x, t) + (1 - w) BCEWithLogits(x, l);  loss_out[0] = sum(part) / (2 n H W) (f64 sum, fixed order).
 * iou_out [n] optional. */
int ucod_window_loss(const float* window_preds, const float* h_targets, const int* win_flat, const float* l_up, int targets_are_logits,
                     float* part, float* iou_out, float* loss_out, int n, int B, int H, int W, int ws, void* stream);

/* GatedEnsembler (models/modules/GE_pix_level.py:16-25) after the bilinear resize of l1: 19x19 zero-padded average of
 * sigmoid(l1), its entropy normalised by the maximum over the WHOLE batch, gate = ((1 - en/en_max) + mean sigmoid(l1))/2,
 * y = l1*gate + l2*(1-gate), out = fuser(y) (1x1 conv 1->64, ReLU, 1x1 conv 64->1).  All maps f32 [B,1,h,w].
 * workspace: ucod_gated_ensemble_workspace_bytes(B, h, w) = 4 * (2 B h w + B ceil(h w / 256) + 1) bytes -- the entropy map, sigmoid(l1), one partial sum of
 * sigmoid(l1) per 256-pixel workgroup and the batch maximum; it need not be initialised.  The mean of sigmoid(l1) is the sum of an image's partials in a
 * fixed order and the maximum an integer atomicMax: the call executes no floating-point atomic and two runs are bit-identical at every size. */
size_t ucod_gated_ensemble_workspace_bytes(int B, int h, int w);
int ucod_gated_ensemble(const float* l1_up, const float* l2, const float* fuser0_w, const float* fuser0_b, const float* fuser2_w,
                        float fuser2_b, float* out, float* weight_out, void* workspace, int B, int h, int w, void* stream);

/* ------------------------------------------------------------------ CORAL SparseRefiner, training of the window branch (HRE.CSF)
 * The backward of ex_loss (models/UDLR.py:52-75) through models/modules/CSF.py:38-43 and the CrossAttentionBlock of models/modules/mlp.py:134-148,
 * with respect to the 18 HRE.CSF parameters.  The dgrad products are ucod_gemm_bf16_train, the bias gradients ucod_colsum_det, the input cotangent of
 * norm_mlp ucod_layernorm_bwd_ex; a weight gradient dW [N,K] = dY^T X is ucod_gemm_bf16(UCOD_EPI_BIAS_F32, A = dY^T, B = X^T, K = Mp, bias NULL) on the
 * two transposes ucod_transpose_pad_bf16 writes.  Every reduction below runs in a fixed order without floating-point atomics: two runs are bit-identical.
 * The kernels work on bf16 in both builds.  ABI stays 5 (additions only). */

/* ucod_cross_attention96_fwd (mlp.py:122,143) that also returns the base-2 log-sum-exp of the scaled scores, lse f32 [B, heads, Nq].  The same kernel
 * with the pointer set: out is bit-identical to ucod_cross_attention96_fwd's.  UCOD_EINVAL: a null pointer, a non-positive size, ldq / ldkv not a multiple
 * of 8, B or heads above 65535, B * heads * Nq >= 2^31. */
int ucod_cross_attention96_fwd_lse(const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv, void* out_bf16, float* lse,
                                   int B, int Nq, int Nk, int heads, void* stream);

/* Its backward (mlp.py:122,143 differentiated: nn.MultiheadAttention's softmax(q k^T 96^-0.5) v per (window, head), dropout 0).  q, k, v, ldq, ldkv as in
 * the forward (q PRE-SCALED by 96^-0.5 * log2(e)); out, dout bf16 [B*Nq, heads*96]; lse from ucod_cross_attention96_fwd_lse; delta f32 [B, heads, Nq] is
 * scratch (rowsum(dout * out), written by the first kernel, read by the second).  dq bf16 rows of stride lddq, dk / dv bf16 rows of stride lddkv (they may
 * point into one [dk | dv] buffer) = the gradients w.r.t. the UNSCALED projections, ucod_attention_bwd's convention: with P = 2^(q' k^T - lse),
 * dP = dout v^T, dS = P * (dP - delta):  dq = 96^-0.5 dS k,  dk = ln(2) dS^T q',  dv = P^T dout  (P and dS enter their products rounded to bf16).
 * Columns past heads*96 of a dq / dk / dv row are not written.  Two kernels (queries per wave; keys per wave).
 * UCOD_EINVAL before any launch: a null pointer, a non-positive size, a leading dimension that is not a multiple of 8 or is below heads*96, a pointer
 * that is not 16-byte aligned, B or heads above 65535, B * heads * Nq >= 2^31. */
int ucod_cross_attention96_bwd(const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv, const void* out_bf16, const void* dout_bf16,
                               const float* lse, float* delta, void* dq_bf16, int lddq, void* dk_bf16, void* dv_bf16, int lddkv, int B, int Nq, int Nk,
                               int heads, void* stream);

/* d ex_loss / d window_preds (models/UDLR.py:62-75 differentiated), arguments as ucod_window_loss: g f32 [n,1,H,W] =
 * upstream[0] / (2 n H W) * (sigmoid(x) - (w t + (1 - w) l)),  w = clamp(1.5 iou[i], 0, 1) from the iou_out ucod_window_loss wrote, l = sigmoid(l_up) > 0.5,
 * t = h_targets[win_flat[i]] as given (also when the targets are logits: cal_ex_loss hands them to the BCE unchanged).  w, l and t carry no gradient
 * (binary_iou works on integers).  upstream: DEVICE scalar, the cotangent of the loss; NULL = 1.  UCOD_EINVAL: a null pointer other than upstream,
 * a non-positive size, n > 65535, H * W >= 2^29. */
int ucod_window_loss_grad(const float* window_preds, const float* h_targets, const int* win_flat, const float* l_up, const float* iou,
                          const float* upstream, float* g, int n, int B, int H, int W, int ws, void* stream);

/* Backward of ucod_dwconv7_maskdec (models/modules/CSF.py:13-25,41-42 differentiated) for the cotangent g f32 [n,1,H,W] of its output; x_tokens,
 * dw_tapmajor, dw_bias, w1 as in the forward.  With S[tap,c] = sum_{i,p} g[i,p] x[i,p+tap,c] (zero padding) and G = sum g:
 *   d_dw f32 [C,49] (depthwise_conv.weight's own layout) = w1[c] S[tap,c];  d_dw_bias [C] = w1[c] G;  d_w1 [C] = dw_bias[c] G + sum_tap dw[tap,c] S[tap,c];
 *   d_b1 [1] = G;  dx_tokens f32 [n,H,W,C] = w1[c] sum_tap dw[tap,c] g[i,q-tap].
 * workspace: slabs * 49 * C floats, slabs = min(n * H, 64); slab s holds the partial S of image rows [s * ceil(n H / slabs), ...), the slabs are added in
 * ascending order.  UCOD_EINVAL: a null pointer, a non-positive size, n or H above 65535, n * H * W >= 2^29, a workspace that is too small. */
int ucod_dwconv7_maskdec_bwd(const float* g, const float* x_tokens, const float* dw_tapmajor, const float* dw_bias, const float* w1, float* d_dw,
                             float* d_dw_bias, float* d_w1, float* d_b1, float* dx_tokens, void* workspace, size_t workspace_bytes, int n, int H, int W,
                             int C, void* stream);

/* LayerNorm parameter gradients (nn.LayerNorm of mlp.py:136-138,146 differentiated: norm_q, norm_kv, norm_mlp): dgamma[c] = sum_r dy[r,c] xhat[r,c],
 * dbeta[c] = sum_r dy[r,c], xhat = (x - mean) * rsqrt(var + eps) from row statistics recomputed here.  dy f32 [rows,D], or bf16 with
 * flags = UCOD_LNB_DY_BF16; x f32 [rows,D].  workspace: slabs * 2 * D floats, slabs = min(128, ceil(rows / 64)); row slabs of ceil(rows / slabs) rows,
 * added in ascending order.  UCOD_EINVAL: a null pointer, rows < 1, D not a multiple of 64 or above 1024, another flag, a workspace that is too small. */
int ucod_layernorm_param_grad(const void* dy, int flags, const float* x, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                              int rows, int D, float eps, void* stream);

/* Operand of a weight-gradient product (the nn.Linear layers of mlp.py:122,141-143 differentiated in their weights): src rows [M, ld] of f32
 * (src_is_bf16 = 0) or bf16 (1), columns 0 .. cols-1 -> dst bf16 [cols, Mp] = src^T rounded to nearest even, Mp = max(128, 64 * ceil(M / 64)), exact
 * zeros in columns M .. Mp-1.  UCOD_EINVAL: a null pointer, a non-positive size, ld < cols, another src_is_bf16. */
int ucod_transpose_pad_bf16(const void* src, int src_is_bf16, int M, int cols, int ld, void* dst_bf16, void* stream);

/* ------------------------------------------------------------------ CORAL SparseRefiner, the gradient through `outputs` (SparseRefiner(train_outputs=True))
 * Backward of ucod_gated_ensemble (models/modules/GE_pix_level.py:16-25 differentiated) in l2 and in the fuser's four parameters, for the cotangent g_out
 * f32 [B,1,h,w] of `out`.  l1_up, l2 as in the forward; ge_w = the weight_out the forward wrote (a function of the first-stage logits alone: no gradient is
 * formed for it or for l1_up).  Per pixel i, with w = ge_w[i], y = l1_up[i] w + l2[i] (1 - w) (recomputed), z_k = a_k y + c_k, m_k = [z_k > 0] (torch's
 * ReLU subgradient: 0 at z_k == 0), a = fuser0_w, c = fuser0_b, d = fuser2_w, G = g_out[i]:
 *   dl2 f32 [B,1,h,w]: dl2[i] = G (1 - w) sum_k d_k a_k m_k;   d_fuser2_b [1] = sum_i G;   d_fuser2_w [64]: sum_i G max(z_k, 0);
 *   d_fuser0_w [64]: sum_i G d_k m_k y;   d_fuser0_b [64]: sum_i G d_k m_k.
 * The 193 sums: one partial per workgroup (a tile of 256 pixels of one image, walked in pixel order) in `workspace`
 * (ucod_gated_ensemble_bwd_workspace_bytes(B, h, w) = B * ceil(h w / 256) * 193 floats), then added in ascending order in f64: no floating-point atomics,
 * two runs are bit-identical.  UCOD_EINVAL before any launch: a null pointer, a non-positive size, B > 65535, B * h * w >= 2^29, a workspace that is too
 * small.  ABI stays 5 (additions only). */
size_t ucod_gated_ensemble_bwd_workspace_bytes(int B, int h, int w);
int ucod_gated_ensemble_bwd(const float* l1_up, const float* l2, const float* ge_w, const float* fuser0_w, const float* fuser0_b, const float* fuser2_w,
                            const float* g_out, float* dl2, float* d_fuser0_w, float* d_fuser0_b, float* d_fuser2_w, float* d_fuser2_b, void* workspace,
                            size_t workspace_bytes, int B, int h, int w, void* stream);

/* The adjoint of ucod_window_scatter (models/modules/HRE.py:18-39 differentiated in the windows): a gather.  dl2 f32 [B,1,ws*H,ws*W]; coords, win_img, n,
 * B, H, W, ws as in the forward;  g f32 [n,1,H,W]:  g[i,py,px] (+)= dl2[win_img[i], coords[i].y*H + py, coords[i].x*W + px] / (1 + 1e-6)  -- the selected
 * windows are distinct cells, so the count the forward divides by is 1.  accumulate = 1 adds into the g ucod_window_loss_grad wrote (one g for one CSF
 * backward), 0 writes g alone.  n == 0: nothing to do, UCOD_OK.  A window whose coords or image index lie outside [0, ws) / [0, B) is left untouched.
 * UCOD_EINVAL: a null pointer with n > 0, a non-positive size, n < 0 or n > 65535, B * ws * H * ws * W >= 2^29, accumulate other than 0 / 1. */
int ucod_window_gather(const float* dl2, const int* coords, const int* win_img, float* g, int accumulate, int n, int B, int H, int W, int ws, void* stream);

/* ------------------------------------------------------------------ CORAL SparseRefiner, the optimizer step (SparseRefiner(direct_wgrad=True))
 * Weight gradient of an nn.Linear (mlp.py:122,141-143 differentiated in the weights) from the TOKEN-major operands, with no transposed copy in global
 * memory:  dW[n][k] (+)= sum_m dy[m][n] x[m][k];  dy bf16 [M, ld_dy], x bf16 [M, ld_x], dW f32 [N, ld_dw]; bf16 products accumulated in f32 on the MFMA.
 * The token axis is split deterministically:
 *   nsplit(M, N, K):  tiles = ceil(N / 128) * ceil(K / 128);  n = floor((256 + tiles / 2) / tiles) [integer tiles / 2] clamped to [1, ceil(M / 64)];
 *                     chunk = 64 * ceil(ceil(M / n) / 64);  nsplit = ceil(M / chunk)      (a function of the three sizes only; chunk(nsplit) == chunk)
 * chunk s owns rows [s chunk, min(M, (s + 1) chunk)); a workgroup owns one 128 x 128 tile of one chunk and walks it in 64-row slabs, one
 * v_mfma_f32_32x32x16_bf16 per 16 rows; its f32 partial goes to workspace[s][N][K]; a second kernel adds the partials in ascending s in f32 and then
 * writes the sum to dW, or (accumulate != 0) adds it to dW.  nsplit == 1: no workspace (it may be NULL), the tile is written or added to dW directly.
 * No atomics: two runs are bit-identical.  7 chunks at 768 x 768 (252 workgroups), 4 at 1536 x 768, 2 at 3072 x 768 and 768 x 3072.
 * ucod_wgrad_bf16_det_workspace_bytes = nsplit > 1 ? nsplit * N * K * 4 : 0; both helpers return 0 for sizes the entry point refuses.
 * UCOD_EINVAL with nothing launched: a null pointer (workspace only where it is needed), M < 1, N or K not a positive multiple of 64, ld_dy < N, ld_x < K,
 * ld_dw < K, ld_dy or ld_x not a multiple of 4 or dy / x not 8-byte aligned (row starts must be), dW or workspace not 4-byte aligned, a workspace that is
 * too small.  bf16 in both libraries.  ABI stays 5 (additions only). */
size_t ucod_wgrad_bf16_det_workspace_bytes(int M, int N, int K);
int ucod_wgrad_bf16_det_nsplit(int M, int N, int K);
int ucod_wgrad_bf16_det(const void* dy_bf16, int ld_dy, const void* x_bf16, int ld_x, float* dW, int ld_dw, int M, int N, int K, int accumulate, void* ws,
                        size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ COD measures (row N4: engine/utils/metrics/metric.py::statistics)
 * pred, gt f32 [B,H,W] (any range: the measures min-max normalise the prediction and threshold the normalised ground truth at 0.5,
 * _prepare_data :125-133).  out f64 [B][UCOD_COD_RECORD], per image:
 *   [0] MAE  [1] ACC  [2] IoU  [3] S-measure  [4] weighted F  [5] adaptive E  [6] adaptive F  [7] ground-truth foreground pixels,
 *   [8..263] E-measure over the 256 thresholds, [264..519] F-measure curve (beta^2 = 0.3), [520..775] precision, [776..1031] recall
 * -- exactly what one statistics.step() appends to its seven measure objects; get_result() is means over images of these.
 * float64 arithmetic throughout, fixed reduction trees (deterministic); agreement with the reference's numpy is to summation order.
 * A constant prediction follows the reference's integer branch (pred.astype(int)); constants outside [0, 2) are not supported. */
#define UCOD_COD_RECORD 1032
size_t ucod_cod_metrics_workspace_bytes(int B, int H, int W);
int ucod_cod_metrics(const float* pred, const float* gt, int B, int H, int W, double* out, void* workspace, size_t workspace_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
