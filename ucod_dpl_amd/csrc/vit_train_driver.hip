// Host-side driver of the backbone-backward mode (models/modules/full_model.py:79-126: LoRA-wrapped
// backbone -> last-layer key hook -> decoder).  Two C calls, each enqueues a whole pass on the caller's stream:
//   ucod_vit_forward_train   image -> key map, saving what the backward needs (per layer: the two residual-stream states in
//                            f32, LN1 output + LoRA down-projection, qkv, attention output, log-sum-exp, fc1 pre-activation)
//   ucod_vit_backward        cotangent of the key map -> LoRA gradients of every layer (all other weights are frozen, so no
//                            weight-gradient GEMMs: dgrad only, ~2x the forward FLOPs with the recomputed attention scores)
// The _mlp forms take the MLP kind: UCOD_MLP_SWIGLU (Dinov2SwiGLUFFN, modeling_dinov2.py:300-315) saves the interleaved pre-activation [M, 2F] from the weights_in
// drain (UCOD_EPI_BIAS_SWIGLU_SAVE_BF16) and turns the hidden cotangent into dpre [M, 2F] in the weights_out dgrad's drain (UCOD_EPI_SWIGLU_BWD_BF16).
// The _lora_mlp forms take the per-layer table of a LoRA module on the MLP input projection (fc1 / weights_in; full_model.py:47-72 hands target_modules to peft):
// LayerNorm 2 then writes h2_aug [M, D+64] with the module's down-projection, fc1 runs with K = D+64 against fc1_w_aug, and the backward recomputes h2_aug from the
// saved residual stream, takes the module's gradients from dpre (ucod_lora_mlp_grad) and adds t A_m in the LayerNorm-2 backward.  A NULL table is the _mlp form.
// DINOv3 (vit.rope with allow_rope = 1): every layer but the last rotates q / k of the patch rows in place between the QKV GEMM and attention (the last layer's key hook
// is taken in front of any rotation), and the backward applies the transposed rotation to dq / dk behind ucod_attention_bwd (ucod_rope_qk_ld).  Plans do not change.
// The _lora_out forms take the per-layer table of the LoRA modules on the output projections (attention.output.dense / mlp.fc2; o_proj / down_proj): their inputs have
// no aug columns, so each module is one row kernel behind its residual GEMM (ucod_lora_out_fwd: x += lambda * scaling * (drop(x_in) A^T) B^T, u saved) and two in the
// backward (ucod_lora_out_grad_s on the dgrad GEMM's operand s, ucod_lora_out_grad_x on x_in and its cotangent).  Dropout keys 2L + l (dense) and 3L + l (fc2).
// A NULL table is the _lora_mlp form.
// The _lora_out_ex forms take one word of flags: with UCOD_LORA_OUT_SWIGLU the fc2 slots may be filled on the SwiGLU MLP too (Dinov2SwiGLUFFN.weights_out; the gated
// DINOv3 down_proj): the forward kernel reads the hidden [M, F] as ever, the backward recomputes it from the saved interleaved pre-activation
// (ucod_lora_out_grad_x_ex with UCOD_LORA_OUT_ACT_SWIGLU on pre / dpre [M, 2F]).  Flags 0 is the _lora_out form.
// No allocation, no sync.  Operand formats of the LoRA "aug" columns: vit_train.hip.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace {

struct TPlan {
  int M, tok, L;
  size_t x_in, x_mid, h_aug, qkv, att, lse, pre;           // per-layer arrays: base offset; stride below
  size_t s_x, s_h, s_qkv, s_att, s_lse, s_pre;
  size_t h2, g, patch, qscale;                             // forward transients
  size_t dx, dh, s, da, dqkv, delta, lgw;                  // backward scratch (dpre aliases g, s aliases h2)
  size_t tm, mgw, mgw_bytes;                               // MLP LoRA module: t scratch [M, 64], partials of ucod_lora_mlp_grad
  size_t u_o, u_2, s_u, t_out, ogw, ogw_bytes;             // output modules: saved u [M, 8] per layer (dense, fc2), t scratch [M, 8], partials of ucod_lora_out_grad_*
  size_t total;
};

inline size_t up(size_t v) { return (v + 255) / 256 * 256; }

bool valid_qkv(const ucod_vit_train_desc* t) {
  if (!t) return false;
  const ucod_vit_desc* d = &t->vit;
  return d->B > 0 && d->C > 0 && d->P > 0 && d->H > 0 && d->W > 0 && d->H % d->P == 0 && d->W % d->P == 0 && d->D > 0 && d->heads > 0 &&
         d->D == d->heads * 64 && d->D % 128 == 0 && d->F % 128 == 0 && d->L >= 1 && d->Kpad % 64 == 0 && d->Kpad >= d->C * d->P * d->P &&
         t->lora_r >= 1 && 3 * t->lora_r <= UCOD_LORA_AUG && t->lora_dropout >= 0.f && t->lora_dropout < 1.f &&
         (d->rope == nullptr || t->allow_rope == 1) &&              // DINOv3: only a caller that names the rotary passes (allow_rope) gets them; a zero-filled field refuses a table
         d->n_reg >= 0 && d->n_reg <= 1023 && (d->resid16 == 0 || d->resid16 == 1);   // resid16: the saved residual stream is IEEE fp16 (round 4: LayerNorm backward reads it)
}

inline bool known_mlp(int mlp) { return mlp == UCOD_MLP_GELU || mlp == UCOD_MLP_SWIGLU; }
inline int fc1_width(const ucod_vit_desc* d, int mlp) { return mlp == UCOD_MLP_SWIGLU ? 2 * d->F : d->F; }
// mlpl: the pass carries a LoRA module on the MLP input projection (its rank limit and the widths its gradient kernel covers)
inline bool valid_mlpl(const ucod_vit_train_desc* t, int mlp, bool mlpl) {
  return !mlpl || (t->lora_r <= UCOD_LORA_MLP_MAX_R && ucod_lora_mlp_grad_workspace_bytes(fc1_width(&t->vit, mlp), t->vit.D) != 0);
}
// the output modules a table names (layer 0's parameter slots: the same modules in every layer), and whether the pass can carry them
struct OutMods { bool o, f; };
inline OutMods out_mods(const void* const* TO) { return OutMods{TO && TO[0] != nullptr, TO && TO[2] != nullptr}; }
inline size_t out_gw_bytes(const ucod_vit_train_desc* t, OutMods m) {
  const size_t a = m.o ? ucod_lora_out_grad_workspace_bytes(t->lora_r, t->vit.D, t->vit.D) : 0, b = m.f ? ucod_lora_out_grad_workspace_bytes(t->lora_r, t->vit.F, t->vit.D) : 0;
  return a > b ? a : b;
}
inline bool valid_out(const ucod_vit_train_desc* t, int mlp, const void* const* TO, int out_flags) {
  const OutMods m = out_mods(TO);
  if (out_flags & ~UCOD_LORA_OUT_SWIGLU) return false;            // an unknown flag bit
  if (!TO) return true;
  if (!m.o && !m.f) return false;                                 // a table that names no module
  // (SwiGLU: the hidden is recomputed from the interleaved, padded [M, 2F] pre-activation -- only with the _ex forms' UCOD_LORA_OUT_SWIGLU)
  if (m.f && mlp != UCOD_MLP_GELU && !(out_flags & UCOD_LORA_OUT_SWIGLU)) return false;
  return (!m.o || ucod_lora_out_grad_workspace_bytes(t->lora_r, t->vit.D, t->vit.D) != 0) && (!m.f || ucod_lora_out_grad_workspace_bytes(t->lora_r, t->vit.F, t->vit.D) != 0);
}
bool valid(const ucod_vit_train_desc* t, int mlp = UCOD_MLP_GELU, bool mlpl = false, const void* const* TO = nullptr, int out_flags = 0) {
  return valid_qkv(t) && known_mlp(mlp) && valid_mlpl(t, mlp, mlpl) && valid_out(t, mlp, TO, out_flags);
}

TPlan make_plan(const ucod_vit_train_desc* t, int mlp, bool mlpl = false, const void* const* TO = nullptr) {
  const ucod_vit_desc* d = &t->vit;
  TPlan p;
  const int gh = d->H / d->P, gw = d->W / d->P;
  p.tok = gh * gw + 1 + d->n_reg;                                  // [CLS | n_reg register tokens | patches]
  p.M = d->B * p.tok;
  p.L = d->L;
  const size_t M = p.M, D = d->D, F = d->F, L = d->L;
  const size_t FP = mlp == UCOD_MLP_SWIGLU ? 2 * F : F;      // width of the saved pre-activation and of its cotangent (SwiGLU: x1 | x2 interleaved)
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += up(bytes); return r; };
  p.s_x = up(M * D * (d->resid16 ? 2 : 4));
  p.s_h = up(M * (D + UCOD_LORA_AUG) * 2);
  p.s_qkv = up(M * 3 * D * 2);
  p.s_att = up(M * D * 2);
  p.s_lse = up((size_t)d->B * d->heads * p.tok * 4);
  p.s_pre = up(M * FP * 2);
  p.x_in = take(p.s_x * L);
  p.x_mid = take(p.s_x * (L - 1));
  p.h_aug = take(p.s_h * L);
  p.qkv = take(p.s_qkv * (L - 1));
  p.att = take(p.s_att * (L - 1));
  p.lse = take(p.s_lse * (L - 1));
  p.pre = take(p.s_pre * (L - 1));
  p.h2 = take(M * (D + (mlpl ? UCOD_LORA_AUG : 0)) * 2);      // (MLP LoRA module: h2_aug; s [M, D] still fits)
  p.g = take(M * FP * 2);                                     // the hidden [M, F]; the backward's dpre [M, FP] aliases it
  p.patch = take((size_t)d->B * gh * gw * d->Kpad * 2);
  p.qscale = take(3 * D * 4);
  p.dx = take(M * D * 4);
  p.dh = take(M * D * 4);
  p.s = p.h2;
  p.da = take(M * D * 2);
  p.dqkv = take(M * (3 * D + UCOD_LORA_AUG) * 2);
  p.delta = take((size_t)d->B * d->heads * p.tok * 4);
  p.lgw = take(ucod_lora_grad_workspace_bytes(d->D));
  p.tm = p.mgw = p.mgw_bytes = 0;
  if (mlpl) {
    p.tm = take(M * UCOD_LORA_AUG * 2);
    p.mgw_bytes = ucod_lora_mlp_grad_workspace_bytes((int)FP, d->D);
    p.mgw = take(p.mgw_bytes);
  }
  p.u_o = p.u_2 = p.s_u = p.t_out = p.ogw = p.ogw_bytes = 0;
  if (TO) {                                                     // (behind everything else: without a table no offset and no byte differs)
    const OutMods m = out_mods(TO);
    p.s_u = up(M * UCOD_LORA_OUT_W * 4);
    if (m.o) p.u_o = take(p.s_u * (L - 1));
    if (m.f) p.u_2 = take(p.s_u * (L - 1));
    p.t_out = take(M * UCOD_LORA_OUT_W * 4);
    p.ogw_bytes = out_gw_bytes(t, m);
    p.ogw = take(p.ogw_bytes);
  }
  p.total = o;
  return p;
}

}  // namespace

#define RUN(call)                \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != 0) return rc__;  \
  } while (0)

extern "C" size_t ucod_vit_train_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM, const void* const* TO) {
  return valid(t, mlp, TM != nullptr, TO, out_flags) ? make_plan(t, mlp, TM != nullptr, TO).total : 0;
}
extern "C" size_t ucod_vit_train_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* TM, const void* const* TO) {
  return ucod_vit_train_workspace_bytes_lora_out_ex(t, mlp, 0, TM, TO);
}
extern "C" size_t ucod_vit_train_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* TM) {
  return ucod_vit_train_workspace_bytes_lora_out(t, mlp, TM, nullptr);
}
extern "C" size_t ucod_vit_train_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp) { return ucod_vit_train_workspace_bytes_lora_mlp(t, mlp, nullptr); }
extern "C" size_t ucod_vit_train_workspace_bytes(const ucod_vit_train_desc* t) { return ucod_vit_train_workspace_bytes_mlp(t, UCOD_MLP_GELU); }

extern "C" int ucod_vit_forward_train_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT,
                                                  const void* const* TM, const void* const* TO, const float* img, float* key_out, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  UCOD_BF16_ONLY();
  if (!valid(t, mlp, TM != nullptr, TO, out_flags) || !T || !TT || !img || !key_out || !workspace) return UCOD_EINVAL;
  const ucod_vit_desc* d = &t->vit;
  const bool swiglu = mlp == UCOD_MLP_SWIGLU;
  const TPlan p = make_plan(t, mlp, TM != nullptr, TO);
  const OutMods om = out_mods(TO);
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, gv = d->gemm_variant, KA = D + UCOD_LORA_AUG;
  float* qscale = (float*)(ws + p.qscale);
  void* h2 = ws + p.h2;
  void* g = ws + p.g;
  void* patches = ws + p.patch;
  RUN(ucod_fill_qscale(qscale, D, 0.125f * 1.4426950408889634f, stream));

  const bool r16 = d->resid16 != 0;                               // fp16 residual stream (saved as such: half the bytes forward and backward)
  const int epi_patch = r16 ? UCOD_EPI_PATCH_TOKENS_H16 : UCOD_EPI_PATCH_TOKENS_F32;
  const int epi_resid = r16 ? UCOD_EPI_BIAS_SCALE_RESID_H16 : UCOD_EPI_BIAS_SCALE_RESID_F32;
  float* x0 = (float*)(ws + p.x_in);
  RUN(ucod_patch_im2col(img, patches, d->B, d->C, d->H, d->W, d->P, d->Kpad, stream));
  RUN(ucod_gemm_bf16_reg(epi_patch, patches, T[0], x0, d->B * (tok - 1 - d->n_reg), D, d->Kpad, (const float*)T[1], nullptr, nullptr,
                         (const float*)T[3], tok, d->n_reg, gv, stream));
  if (r16) RUN(ucod_cls_rows_h16_reg(x0, (const float*)T[2], (const float*)T[3], d->B, tok, D, d->n_reg, stream));
  else RUN(ucod_cls_rows_reg(x0, (const float*)T[2], (const float*)T[3], d->B, tok, D, d->n_reg, stream));

  for (int l = 0; l < d->L; ++l) {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    const bool last = (l == d->L - 1);
    float* x_in = (float*)(ws + p.x_in + p.s_x * l);
    void* h_aug = ws + p.h_aug + p.s_h * l;
    const ucod_lora_dropout drop{t->lora_dropout, t->seed, l};
    if (r16) RUN(ucod_layernorm_lora_h16(x_in, (const float*)W[0], (const float*)W[1], (const float*)X[5], t->lora_r, h_aug, M, D, d->eps,
                                         t->lora_dropout > 0.f ? &drop : nullptr, stream));
    else RUN(ucod_layernorm_lora(x_in, (const float*)W[0], (const float*)W[1], (const float*)X[5], t->lora_r, h_aug, M, D, d->eps,
                                 t->lora_dropout > 0.f ? &drop : nullptr, stream));
    if (last) {   // key hook: K rows of the augmented qkv weight; [B,D,h,w] out
      const char* wk = (const char*)X[0] + (size_t)D * KA * 2;
      RUN(ucod_gemm_bf16_reg(UCOD_EPI_KEY_NCHW_F32, wk, h_aug, key_out, D, M, KA, (const float*)W[3] + D, nullptr, nullptr, nullptr, tok, d->n_reg, gv, stream));
      break;
    }
    float* x_mid = (float*)(ws + p.x_mid + p.s_x * l);
    float* x_next = (float*)(ws + p.x_in + p.s_x * (l + 1));
    void* qkv = ws + p.qkv + p.s_qkv * l;
    void* att = ws + p.att + p.s_att * l;
    float* lse = (float*)(ws + p.lse + p.s_lse * l);
    void* pre = ws + p.pre + p.s_pre * l;
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_BF16, h_aug, X[0], qkv, M, 3 * D, KA, (const float*)W[3], qscale, nullptr, nullptr, tok, gv, stream));
    // DINOv3: q and k of the patch rows are rotated in the SAVED buffer, so that the backward's recomputed scores see the operands attention saw
    if (d->rope) RUN(ucod_rope_qk_ld(qkv, UCOD_ROPE_ELEM_HALF, d->rope, d->B, tok, d->n_reg, d->heads, 3 * D, 0, stream));
    RUN(ucod_attention_fwd_lse(qkv, att, lse, d->B, tok, d->heads, stream));
    RUN(ucod_gemm_bf16(epi_resid, att, W[4], x_mid, M, D, D, (const float*)W[5], (const float*)W[6], x_in, nullptr, tok, gv, stream));
    const void* const* Z = TO ? TO + UCOD_VIT_TRAIN_OUT_STRIDE * l : nullptr;
    if (om.o) {   // LoRA on the attention output projection: x_mid += ls1 * scaling * (drop(att) A_o^T) B_o^T, u saved (its own mask: key 2L + l)
      const ucod_lora_dropout drop_o{t->lora_dropout, t->seed, 2 * d->L + l};
      RUN(ucod_lora_out_fwd(att, (const float*)Z[0], t->lora_r, t->lora_scaling, (const float*)W[6], x_mid, r16, (float*)(ws + p.u_o + p.s_u * l), M, D, D,
                            t->lora_dropout > 0.f ? &drop_o : nullptr, stream));
    }
    if (TM) {   // LoRA on the MLP input projection: LayerNorm 2 + down-projection, fc1 over K = D+64 against fc1_w_aug (its own mask: key L + l)
      const void* const* Y = TM + UCOD_VIT_TRAIN_MLP_STRIDE * l;
      const ucod_lora_dropout drop_m{t->lora_dropout, t->seed, d->L + l};
      RUN(ucod_layernorm_lora_mlp(x_mid, r16, (const float*)W[7], (const float*)W[8], (const float*)Y[1], t->lora_r, h2, M, D, d->eps,
                                  t->lora_dropout > 0.f ? &drop_m : nullptr, stream));
      RUN(ucod_gemm_bf16_train(swiglu ? UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 : UCOD_EPI_BIAS_GELU_SAVE_BF16, h2, Y[0], g, M, fc1_width(d, mlp), KA, (const float*)W[10],
                               nullptr, pre, gv, stream));
    } else {
      if (r16) RUN(ucod_layernorm_h16(x_mid, (const float*)W[7], (const float*)W[8], h2, M, D, d->eps, stream));
      else RUN(ucod_layernorm(x_mid, (const float*)W[7], (const float*)W[8], h2, M, D, d->eps, 0, stream));
      if (swiglu) RUN(ucod_gemm_bf16_train(UCOD_EPI_BIAS_SWIGLU_SAVE_BF16, h2, W[9], g, M, 2 * F, D, (const float*)W[10], nullptr, pre, gv, stream));
      else RUN(ucod_gemm_bf16_train(UCOD_EPI_BIAS_GELU_SAVE_BF16, h2, W[9], g, M, F, D, (const float*)W[10], nullptr, pre, gv, stream));
    }
    RUN(ucod_gemm_bf16(epi_resid, g, W[11], x_next, M, D, F, (const float*)W[12], (const float*)W[13], x_mid, nullptr, tok, gv, stream));
    if (om.f) {   // LoRA on the MLP output projection: x_next += ls2 * scaling * (drop(g) A_2^T) B_2^T, u saved (key 3L + l)
      const ucod_lora_dropout drop_f{t->lora_dropout, t->seed, 3 * d->L + l};
      RUN(ucod_lora_out_fwd(g, (const float*)Z[2], t->lora_r, t->lora_scaling, (const float*)W[13], x_next, r16, (float*)(ws + p.u_2 + p.s_u * l), M, F, D,
                            t->lora_dropout > 0.f ? &drop_f : nullptr, stream));
    }
  }
  return UCOD_OK;
}
extern "C" int ucod_vit_forward_train_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                               const void* const* TO, const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_train_lora_out_ex(t, mlp, 0, T, TT, TM, TO, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                               const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_train_lora_out(t, mlp, T, TT, TM, nullptr, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* img,
                                          float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_train_lora_mlp(t, mlp, T, TT, nullptr, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* img,
                                      float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_train_mlp(t, UCOD_MLP_GELU, T, TT, img, key_out, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
// No-grad pass of the LoRA backbone: what the EMA teacher of models/modules/full_model.py:84,108-111 runs (backbone_ema under
// torch.no_grad()).  Same arithmetic as ucod_vit_forward_train -- LoRA as 64 extra K columns of the QKV / key GEMMs, dropout masks
// from the same counter hash -- but nothing is saved: one residual buffer updated in place, plain GELU epilogue, no log-sum-exp, and
// the residual stream may be IEEE fp16 (vit.resid16) like the frozen-backbone pass.  Workspace ~ the inference pass's.
namespace {
struct IPlan {
  size_t x, h_aug, h2, qkv, a, g, patch, qscale, total;
  int M, tok;
};
bool valid_infer(const ucod_vit_train_desc* t) {
  if (!t) return false;
  const ucod_vit_desc* d = &t->vit;
  return d->B > 0 && d->C > 0 && d->P > 0 && d->H > 0 && d->W > 0 && d->H % d->P == 0 && d->W % d->P == 0 && d->D > 0 && d->heads > 0 &&
         d->D == d->heads * 64 && d->D % 128 == 0 && d->F % 128 == 0 && d->L >= 1 && d->Kpad % 64 == 0 && d->Kpad >= d->C * d->P * d->P &&
         t->lora_r >= 1 && 3 * t->lora_r <= UCOD_LORA_AUG && t->lora_dropout >= 0.f && t->lora_dropout < 1.f && d->n_reg >= 0 && d->n_reg <= 1023 && (d->resid16 == 0 || d->resid16 == 1) &&
         (d->rope == nullptr || t->allow_rope == 1);                // (DINOv3: as valid_qkv)
}
IPlan make_iplan(const ucod_vit_train_desc* t, bool mlpl = false) {
  const ucod_vit_desc* d = &t->vit;
  IPlan p;
  const int gh = d->H / d->P, gw = d->W / d->P;
  p.tok = gh * gw + 1 + d->n_reg;                                  // [CLS | n_reg register tokens | patches]
  p.M = d->B * p.tok;
  const size_t M = p.M, D = d->D, F = d->F;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += up(bytes); return r; };
  p.x = take(M * D * (d->resid16 ? 2 : 4));
  p.h_aug = take(M * (D + UCOD_LORA_AUG) * 2);
  p.h2 = take(M * (D + (mlpl ? UCOD_LORA_AUG : 0)) * 2);
  p.qkv = take(M * 3 * D * 2);
  p.a = take(M * D * 2);
  p.g = take(M * F * 2);                                      // (either kind: the hidden [M, F]; SwiGLU's weights_in output never reaches memory)
  p.patch = take((size_t)d->B * gh * gw * d->Kpad * 2);
  p.qscale = take(3 * D * 4);
  p.total = o;
  return p;
}
}  // namespace

// (the no-grad pass saves nothing: the output modules add no workspace byte)
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM,
                                                                  const void* const* TO) {
  return valid_infer(t) && known_mlp(mlp) && valid_mlpl(t, mlp, TM != nullptr) && valid_out(t, mlp, TO, out_flags) ? make_iplan(t, TM != nullptr).total : 0;
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* TM, const void* const* TO) {
  return ucod_vit_lora_infer_workspace_bytes_lora_out_ex(t, mlp, 0, TM, TO);
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* TM) {
  return ucod_vit_lora_infer_workspace_bytes_lora_out(t, mlp, TM, nullptr);
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp) { return ucod_vit_lora_infer_workspace_bytes_lora_mlp(t, mlp, nullptr); }
extern "C" size_t ucod_vit_lora_infer_workspace_bytes(const ucod_vit_train_desc* t) { return ucod_vit_lora_infer_workspace_bytes_mlp(t, UCOD_MLP_GELU); }

extern "C" int ucod_vit_forward_lora_infer_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT,
                                                       const void* const* TM, const void* const* TO, const float* img, float* key_out, void* workspace,
                                                       size_t workspace_bytes, void* stream) {
  UCOD_BF16_ONLY();
  if (!valid_infer(t) || !known_mlp(mlp) || !valid_mlpl(t, mlp, TM != nullptr) || !valid_out(t, mlp, TO, out_flags) || !T || !TT || !img || !key_out || !workspace) return UCOD_EINVAL;
  const OutMods om = out_mods(TO);
  const bool swiglu = mlp == UCOD_MLP_SWIGLU;
  const ucod_vit_desc* d = &t->vit;
  const IPlan p = make_iplan(t, TM != nullptr);
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, gv = d->gemm_variant, KA = D + UCOD_LORA_AUG;
  const bool r16 = d->resid16 != 0;
  float* x = (float*)(ws + p.x);
  void* h_aug = ws + p.h_aug;
  void* h2 = ws + p.h2;
  void* qkv = ws + p.qkv;
  void* a = ws + p.a;
  void* g = ws + p.g;
  void* patches = ws + p.patch;
  float* qscale = (float*)(ws + p.qscale);
  const int epi_patch = r16 ? UCOD_EPI_PATCH_TOKENS_H16 : UCOD_EPI_PATCH_TOKENS_F32;
  const int epi_resid = r16 ? UCOD_EPI_BIAS_SCALE_RESID_H16 : UCOD_EPI_BIAS_SCALE_RESID_F32;
  RUN(ucod_fill_qscale(qscale, D, 0.125f * 1.4426950408889634f, stream));
  RUN(ucod_patch_im2col(img, patches, d->B, d->C, d->H, d->W, d->P, d->Kpad, stream));
  RUN(ucod_gemm_bf16_reg(epi_patch, patches, T[0], x, d->B * (tok - 1 - d->n_reg), D, d->Kpad, (const float*)T[1], nullptr, nullptr, (const float*)T[3], tok, d->n_reg, gv, stream));
  if (r16) RUN(ucod_cls_rows_h16_reg(x, (const float*)T[2], (const float*)T[3], d->B, tok, D, d->n_reg, stream));
  else RUN(ucod_cls_rows_reg(x, (const float*)T[2], (const float*)T[3], d->B, tok, D, d->n_reg, stream));
  for (int l = 0; l < d->L; ++l) {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    const ucod_lora_dropout drop{t->lora_dropout, t->seed, l};
    const ucod_lora_dropout* dp = t->lora_dropout > 0.f ? &drop : nullptr;
    if (r16) RUN(ucod_layernorm_lora_h16(x, (const float*)W[0], (const float*)W[1], (const float*)X[5], t->lora_r, h_aug, M, D, d->eps, dp, stream));
    else RUN(ucod_layernorm_lora(x, (const float*)W[0], (const float*)W[1], (const float*)X[5], t->lora_r, h_aug, M, D, d->eps, dp, stream));
    if (l == d->L - 1) {
      const char* wk = (const char*)X[0] + (size_t)D * KA * 2;
      RUN(ucod_gemm_bf16_reg(UCOD_EPI_KEY_NCHW_F32, wk, h_aug, key_out, D, M, KA, (const float*)W[3] + D, nullptr, nullptr, nullptr, tok, d->n_reg, gv, stream));
      break;
    }
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_BF16, h_aug, X[0], qkv, M, 3 * D, KA, (const float*)W[3], qscale, nullptr, nullptr, tok, gv, stream));
    if (d->rope) RUN(ucod_rope_qk_ld(qkv, UCOD_ROPE_ELEM_HALF, d->rope, d->B, tok, d->n_reg, d->heads, 3 * D, 0, stream));
    RUN(ucod_attention_fwd(qkv, a, d->B, tok, d->heads, 0.f, 0, stream));
    RUN(ucod_gemm_bf16(epi_resid, a, W[4], x, M, D, D, (const float*)W[5], (const float*)W[6], x, nullptr, tok, gv, stream));
    const void* const* Z = TO ? TO + UCOD_VIT_TRAIN_OUT_STRIDE * l : nullptr;
    if (om.o) {   // (as the training pass: same arithmetic, same mask keys, u not saved)
      const ucod_lora_dropout drop_o{t->lora_dropout, t->seed, 2 * d->L + l};
      RUN(ucod_lora_out_fwd(a, (const float*)Z[0], t->lora_r, t->lora_scaling, (const float*)W[6], x, r16, nullptr, M, D, D, t->lora_dropout > 0.f ? &drop_o : nullptr,
                            stream));
    }
    if (TM) {
      const void* const* Y = TM + UCOD_VIT_TRAIN_MLP_STRIDE * l;
      const ucod_lora_dropout drop_m{t->lora_dropout, t->seed, d->L + l};
      RUN(ucod_layernorm_lora_mlp(x, r16, (const float*)W[7], (const float*)W[8], (const float*)Y[1], t->lora_r, h2, M, D, d->eps,
                                  t->lora_dropout > 0.f ? &drop_m : nullptr, stream));
      RUN(ucod_gemm_bf16(swiglu ? UCOD_EPI_BIAS_SWIGLU_BF16 : UCOD_EPI_BIAS_GELU_BF16, h2, Y[0], g, M, fc1_width(d, mlp), KA, (const float*)W[10], nullptr, nullptr,
                         nullptr, tok, gv, stream));
    } else {
      if (r16) RUN(ucod_layernorm_h16(x, (const float*)W[7], (const float*)W[8], h2, M, D, d->eps, stream));
      else RUN(ucod_layernorm(x, (const float*)W[7], (const float*)W[8], h2, M, D, d->eps, 0, stream));
      if (swiglu) RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_SWIGLU_BF16, h2, W[9], g, M, 2 * F, D, (const float*)W[10], nullptr, nullptr, nullptr, tok, gv, stream));
      else RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_GELU_BF16, h2, W[9], g, M, F, D, (const float*)W[10], nullptr, nullptr, nullptr, tok, gv, stream));
    }
    RUN(ucod_gemm_bf16(epi_resid, g, W[11], x, M, D, F, (const float*)W[12], (const float*)W[13], x, nullptr, tok, gv, stream));
    if (om.f) {
      const ucod_lora_dropout drop_f{t->lora_dropout, t->seed, 3 * d->L + l};
      RUN(ucod_lora_out_fwd(g, (const float*)Z[2], t->lora_r, t->lora_scaling, (const float*)W[13], x, r16, nullptr, M, F, D, t->lora_dropout > 0.f ? &drop_f : nullptr,
                            stream));
    }
  }
  return UCOD_OK;
}
extern "C" int ucod_vit_forward_lora_infer_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                                    const void* const* TO, const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_lora_infer_lora_out_ex(t, mlp, 0, T, TT, TM, TO, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                                    const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_lora_infer_lora_out(t, mlp, T, TT, TM, nullptr, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* img,
                                               float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_lora_infer_lora_mlp(t, mlp, T, TT, nullptr, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* img,
                                           float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_lora_infer_mlp(t, UCOD_MLP_GELU, T, TT, img, key_out, workspace, workspace_bytes, stream);
}

extern "C" int ucod_vit_backward_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT,
                                             const void* const* TM, const void* const* TO, const float* dkey, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  UCOD_BF16_ONLY();
  if (!valid(t, mlp, TM != nullptr, TO, out_flags) || !T || !TT || !dkey || !workspace) return UCOD_EINVAL;
  const ucod_vit_desc* d = &t->vit;
  const bool swiglu = mlp == UCOD_MLP_SWIGLU;
  const TPlan p = make_plan(t, mlp, TM != nullptr, TO);
  const OutMods om = out_mods(TO);
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, gv = d->gemm_variant, KQ = 3 * D + UCOD_LORA_AUG, r = t->lora_r;
  float* dx = (float*)(ws + p.dx);
  float* dh = (float*)(ws + p.dh);
  void* s = ws + p.s;
  void* dpre = ws + p.g;
  void* da = ws + p.da;
  void* dqkv = ws + p.dqkv;
  float* delta = (float*)(ws + p.delta);
  void* lgw = ws + p.lgw;
  const size_t lgw_bytes = ucod_lora_grad_workspace_bytes(D);

  // dgrad outputs that feed a LayerNorm backward (dh) are written as bf16 (UCOD_DGRAD_F32=1: f32, the round-3 path): the GEMM's drain and the
  // LayerNorm backward's read side move half the bytes; the residual cotangent stream (dx) stays f32
  static const bool dgrad16_env = !(ucod::lab_env("UCOD_DGRAD_F32") && ucod::lab_env("UCOD_DGRAD_F32")[0] == '1');
  const bool r16 = d->resid16 != 0;                               // the saved residual stream is fp16 (then the dgrad outputs are bf16 whatever the variable says)
  const bool dgrad16 = dgrad16_env || r16;
  const int epi_dh = dgrad16 ? UCOD_EPI_BIAS_BF16 : UCOD_EPI_BIAS_F32;
  const int lnb_flags = (dgrad16 ? UCOD_LNB_DY_BF16 : 0) | (r16 ? UCOD_LNB_X_F16 : 0);
  auto ln_bwd_plain = [&](const void* dy, const void* x, const float* gam, const float* dres, const float* next_scale) -> int {
    return ucod_layernorm_bwd_ex(dy, x, lnb_flags, gam, dres, next_scale, dx, s, M, D, d->eps, stream);
  };
  auto qkv_side = [&](int l) -> int {   // dqkv_aug (k/q/v thirds filled) -> LoRA grads of layer l, dh = d LN1 output
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    const void* h_aug = ws + p.h_aug + p.s_h * l;
    const ucod_lora_dropout drop{t->lora_dropout, t->seed, l};
    RUN(ucod_lora_grad(dqkv, h_aug, (const float*)X[5], r, t->lora_scaling, (float*)X[6], 0, lgw, lgw_bytes, M, D,
                       t->lora_dropout > 0.f ? &drop : nullptr, stream));
    RUN(ucod_gemm_bf16(epi_dh, dqkv, X[1], dh, M, D, KQ, nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    return UCOD_OK;
  };

  // LayerNorm-1 backward of layer l: with dropout on, the masked LoRA branch t A is added here (it cannot ride on the dgrad GEMM)
  auto ln1_bwd = [&](int l, const void* dy, const void* x, const float* gam, const float* dres, const float* next_scale) -> int {
    if (t->lora_dropout > 0.f) {
      const ucod_lora_dropout drop{t->lora_dropout, t->seed, l};
      const float* lora_l = (const float*)(TT + UCOD_VIT_TRAIN_STRIDE * l)[5];
      return ucod_layernorm_bwd_lora_ex(dy, x, lnb_flags, gam, dres, next_scale, dx, s, M, D, d->eps, dqkv, lora_l, r, &drop, stream);
    }
    return ln_bwd_plain(dy, x, gam, dres, next_scale);
  };

  // last layer: only the key projection reaches the loss (its MLP never runs: the module's gradients there are zeros, written as such)
  const int last = d->L - 1;
  if (TM) {
    const size_t n_m = (size_t)r * (size_t)(D + fc1_width(d, mlp)) * sizeof(float);
    if (hipMemsetAsync(const_cast<void*>((TM + UCOD_VIT_TRAIN_MLP_STRIDE * last)[2]), 0, n_m, (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
  }
  if (TO) {   // (nor do its attention output and fc2: zeros, written as such)
    const void* const* Z = TO + UCOD_VIT_TRAIN_OUT_STRIDE * last;
    if (om.o && hipMemsetAsync(const_cast<void*>(Z[1]), 0, (size_t)r * (size_t)(D + D) * sizeof(float), (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
    if (om.f && hipMemsetAsync(const_cast<void*>(Z[3]), 0, (size_t)r * (size_t)(F + D) * sizeof(float), (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
  }
  RUN(ucod_key_grad_tokens_reg(dkey, dqkv, d->B, tok, D, d->n_reg, stream));
  RUN(qkv_side(last));
  if (last == 0) return UCOD_OK;
  {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * last;
    const void* const* Wp = T + 4 + UCOD_VIT_LAYER_STRIDE * (last - 1);
    RUN(ln1_bwd(last, dh, (const float*)(ws + p.x_in + p.s_x * last), (const float*)W[0], nullptr, (const float*)Wp[13]));
  }
  for (int l = last - 1; l >= 0; --l) {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    const float* x_in = (const float*)(ws + p.x_in + p.s_x * l);
    const float* x_mid = (const float*)(ws + p.x_mid + p.s_x * l);
    const void* qkv = ws + p.qkv + p.s_qkv * l;
    const void* att = ws + p.att + p.s_att * l;
    const float* lse = (const float*)(ws + p.lse + p.s_lse * l);
    const void* pre = ws + p.pre + p.s_pre * l;
    // MLP branch: s = ls2 * dx  ->  fc2 dgrad (x gelu')  ->  fc1 dgrad  ->  LN2 backward + residual
    // (SwiGLU: the weights_out dgrad's drain writes the cotangent of the interleaved weights_in output, dpre [M, 2F]; X[3] = weights_in^T [D, 2F] in that column order)
    if (swiglu) {
      RUN(ucod_gemm_bf16_train(UCOD_EPI_SWIGLU_BWD_BF16, s, X[4], dpre, M, F, D, nullptr, pre, nullptr, gv, stream));
    } else {
      RUN(ucod_gemm_bf16_train(UCOD_EPI_GELU_BWD_BF16, s, X[4], dpre, M, F, D, nullptr, pre, nullptr, gv, stream));
    }
    const void* const* Z = TO ? TO + UCOD_VIT_TRAIN_OUT_STRIDE * l : nullptr;
    if (om.f) {
      // LoRA on the MLP output projection, while `s` (= bf16(ls2 * dx), the fc2 dgrad's operand) is still there: t = scaling * s B_2 and dB_2 from s and the saved u,
      // then dA_2 from t and the hidden recomputed as gelu(pre), and dpre += gelu'(pre) * mask/(1-p) * (t A_2) -- completed before anything below reads dpre
      // (SwiGLU, UCOD_LORA_OUT_SWIGLU: the hidden is silu(x1) * x2 of the interleaved pre [M, 2F], and dpre [M, 2F] takes the term through both derivative factors)
      const ucod_lora_dropout drop_f{t->lora_dropout, t->seed, 3 * d->L + l};
      float* gz = (float*)const_cast<void*>(Z[3]);
      RUN(ucod_lora_out_grad_s(s, (const float*)(ws + p.u_2 + p.s_u * l), (const float*)Z[2], r, t->lora_scaling, gz, (float*)(ws + p.t_out), ws + p.ogw, p.ogw_bytes,
                               M, F, D, stream));
      RUN(ucod_lora_out_grad_x_ex(pre, swiglu ? UCOD_LORA_OUT_ACT_SWIGLU : UCOD_LORA_OUT_ACT_GELU, swiglu ? UCOD_LORA_OUT_SWIGLU : 0, dpre,
                                  (const float*)(ws + p.t_out), (const float*)Z[2], r, gz, ws + p.ogw, p.ogw_bytes, M, F, D,
                                  t->lora_dropout > 0.f ? &drop_f : nullptr, stream));
    }
    const ucod_lora_dropout drop_m{t->lora_dropout, t->seed, d->L + l};
    const ucod_lora_dropout* dp_m = t->lora_dropout > 0.f ? &drop_m : nullptr;
    const void* const* Y = TM ? TM + UCOD_VIT_TRAIN_MLP_STRIDE * l : nullptr;
    if (TM) {
      // LoRA on the MLP input projection.  `s` (the fc2 dgrad's operand) has been consumed: its buffer takes h2_aug, recomputed from the saved residual
      // stream with the forward's launch (same mask), and is rewritten by the LayerNorm-2 backward below, after the gradient kernel has read it
      void* h2_aug = ws + p.h2;
      RUN(ucod_layernorm_lora_mlp(x_mid, r16, (const float*)W[7], (const float*)W[8], (const float*)Y[1], r, h2_aug, M, D, d->eps, dp_m, stream));
      RUN(ucod_lora_mlp_grad(dpre, h2_aug, (const float*)Y[1], r, t->lora_scaling, (float*)const_cast<void*>(Y[2]), ws + p.tm, ws + p.mgw, p.mgw_bytes, M,
                             fc1_width(d, mlp), D, dp_m, stream));
    }
    RUN(ucod_gemm_bf16(epi_dh, dpre, X[3], dh, M, D, fc1_width(d, mlp), nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    if (TM) RUN(ucod_layernorm_bwd_lora_mlp(dh, x_mid, lnb_flags, (const float*)W[7], dx, (const float*)W[6], dx, s, M, D, d->eps, ws + p.tm, UCOD_LORA_AUG,
                                            (const float*)Y[1], r, dp_m, stream));
    else RUN(ln_bwd_plain(dh, x_mid, (const float*)W[7], dx, (const float*)W[6]));
    // attention branch: s = ls1 * dx  ->  out-proj dgrad  ->  attention backward  ->  LoRA grads + qkv dgrad  ->  LN1 backward
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_BF16, s, X[2], da, M, D, D, nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    if (om.o) {   // LoRA on the attention output projection: s = bf16(ls1 * dx); da += mask/(1-p) * (t A_o) before attention backward reads it
      const ucod_lora_dropout drop_o{t->lora_dropout, t->seed, 2 * d->L + l};
      float* gz = (float*)const_cast<void*>(Z[1]);
      RUN(ucod_lora_out_grad_s(s, (const float*)(ws + p.u_o + p.s_u * l), (const float*)Z[0], r, t->lora_scaling, gz, (float*)(ws + p.t_out), ws + p.ogw, p.ogw_bytes,
                               M, D, D, stream));
      RUN(ucod_lora_out_grad_x(att, UCOD_LORA_OUT_ACT_IDENTITY, da, (const float*)(ws + p.t_out), (const float*)Z[0], r, gz, ws + p.ogw, p.ogw_bytes, M, D, D,
                               t->lora_dropout > 0.f ? &drop_o : nullptr, stream));
    }
    RUN(ucod_attention_bwd(qkv, att, da, lse, delta, dqkv, KQ, d->B, tok, d->heads, stream));
    // DINOv3: dq / dk above are the cotangents of the ROTATED operands; the LoRA-gradient kernel and the QKV dgrad want those of the projection outputs,
    // d(pre) = R^T d(post) -- the same table with the sine negated, on the q | k thirds of dqkv_aug (attention_bwd.hip stores dq at 0, dk at D, dv at 2 D)
    if (d->rope) RUN(ucod_rope_qk_ld(dqkv, UCOD_ROPE_ELEM_HALF, d->rope, d->B, tok, d->n_reg, d->heads, KQ, 1, stream));
    RUN(qkv_side(l));
    if (l > 0) {
      const void* const* Wp = T + 4 + UCOD_VIT_LAYER_STRIDE * (l - 1);
      RUN(ln1_bwd(l, dh, x_in, (const float*)W[0], dx, (const float*)Wp[13]));
    }
  }
  return UCOD_OK;
}
extern "C" int ucod_vit_backward_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                          const void* const* TO, const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_backward_lora_out_ex(t, mlp, 0, T, TT, TM, TO, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                          const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_backward_lora_out(t, mlp, T, TT, TM, nullptr, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* dkey,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_backward_lora_mlp(t, mlp, T, TT, nullptr, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* dkey,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return ucod_vit_backward_mlp(t, UCOD_MLP_GELU, T, TT, dkey, workspace, workspace_bytes, stream);
}
