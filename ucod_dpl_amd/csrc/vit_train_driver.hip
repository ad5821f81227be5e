// Host-side driver of the backbone-backward mode (models/modules/full_model.py:79-126: LoRA-wrapped
// backbone -> last-layer key hook -> decoder).  Three passes, each enqueued whole on the caller's stream:
//   forward, saving     image -> key map, keeping per layer what the backward needs: the two residual-stream states (f32, or fp16 with vit.resid16), LN1 output + LoRA
//                       down-projection (h_aug), qkv (DINOv3: with q / k of the patch rows already rotated, so that the recomputed scores see the operands attention
//                       saw), attention output, log-sum-exp, the fc1 pre-activation ([M, F]; SwiGLU: x1 | x2 interleaved, [M, 2F]) and u [M, 8] of each output module
//   forward, not saving the same launches on one buffer of each kind, the residual stream updated in place: what the EMA teacher runs (full_model.py:84,108-111)
//   backward            cotangent of the key map -> LoRA gradients of every layer (all other weights are frozen, so no weight-gradient GEMMs: dgrad only, ~2x the
//                       forward FLOPs with the recomputed attention scores)
// One body serves both forwards (`forward`; the four places where it asks `save` are all that differs), so they cannot drift apart: the same arithmetic, the same
// dropout masks for the same seed.  A call is a Pass: the descriptor, the MLP kind, one word of flags and four tables, of which two are optional --
//   T, TT   the plain rows and the training table: LoRA on q / k / v rides on the QKV GEMM as 64 extra K columns (operand formats of the "aug" columns: vit_train.hip)
//   TM      LoRA on the MLP input projection (fc1 / weights_in; with UCOD_LORA_MLP_PAIR in the flags the gated MLP's two modules gate_proj / up_proj on the fused
//           weights_in, the _pair forms of the three kernels below): LayerNorm 2 writes h2_aug [M, D+64] with the module's down-projection, fc1 runs with K = D+64 against
//           fc1_w_aug; the backward recomputes h2_aug from the saved residual stream, takes the gradients from dpre (ucod_lora_mlp_grad) and adds t A_m in the
//           LayerNorm-2 backward
//   TO      LoRA on the output projections (attention.output.dense / mlp.fc2; o_proj / down_proj): their inputs have no aug columns, so each module is one row kernel
//           behind its residual GEMM (ucod_lora_out_fwd: x += lambda * scaling * (drop(x_in) A^T) B^T) and two in the backward (ucod_lora_out_grad_s on the dgrad GEMM's
//           operand s, ucod_lora_out_grad_x_ex on x_in and its cotangent).  On the SwiGLU MLP the fc2 slots need UCOD_LORA_OUT_SWIGLU in the flags: the backward then
//           recomputes the hidden from the saved interleaved pre-activation (UCOD_LORA_OUT_ACT_SWIGLU on pre / dpre [M, 2F])
// and, for the backward alone, a fifth --
//   TB      bias="lora_only" (full_model.py:53,66): gradient destinations of the targeted modules' biases, six slots per layer (gb_q, gb_k, gb_v [D], gb_m [N1],
//           gb_o, gb_2 [D]; NULL = not trained).  For y = x W^T + b the gradient is the column sum over token rows of y's cotangent, and every such cotangent is a
//           live buffer here: the thirds of dqkv (behind the DINOv3 un-rotation), the completed dpre, and s = bf16(lambda * dx) of the two residual dgrads (the
//           residual GEMMs compute x += lambda * (acc + b), so db = lambda * sum dx).  One ucod_colsum_det each; the forwards read biases from the plain rows.
// and a sixth, behind it --
//   TN      bias="all" (full_model.py:53,66), behind TB: gradient destinations of the patch embedding's bias and of the two LayerNorm betas of every layer
//           ([0] gb_patch, [1 + 2 l] g_beta1, [2 + 2 l] g_beta2; NULL = not trained): column sums of dh (ucod_colsum_det, or ucod_colsum_det_lora where the LayerNorm
//           backward adds the masked LoRA branch in registers) and of the first residual state's cotangent over the patch rows (ucod_colsum_det_tok)
// The last layer runs LayerNorm 1 and the key projection only: the gradients of its MLP and output modules are written as zeros.
// Dropout: every module has its own mask, keyed kind * L + l (`dropout_of`: q / k / v, the MLP input, dense, fc2 = kinds 0 .. 3).
// Every exported symbol -- five functions in five suffix tiers, the older tiers being the _lora_out_ex forms with NULL tables / flags 0, and the _lora_bias and
// _lora_bias_ex tiers of the backward and its size function -- fills in a Pass and calls one of the five functions below.  No allocation, no sync.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace {

// what a call is (TM / TO NULL: that module is not in the pass; the size functions leave T and TT NULL)
struct Pass {
  const ucod_vit_train_desc* t;
  int mlp, out_flags;
  const void* const* T;
  const void* const* TT;
  const void* const* TM;
  const void* const* TO;
  const void* const* TB;                                   // backward only (every other pass leaves it NULL)
  const void* const* TN;                                   // backward only: bias="all", behind TB
};

struct Plan {
  bool save;                                               // the training pass's plan: per-layer slots; else one buffer of each kind (strides 0) and no lse / pre / u
  int M, tok;
  size_t x_in, x_mid, h_aug, qkv, att, lse, pre;           // per-layer arrays: base offset; stride below
  size_t s_x, s_h, s_qkv, s_att, s_lse, s_pre;
  size_t h2, g, patch, qscale;                             // forward transients
  size_t dx, dh, s, da, dqkv, delta, lgw;                  // backward scratch (dpre aliases g, s aliases h2)
  size_t tm, mgw, mgw_bytes;                               // MLP LoRA module: t scratch [M, 64], partials of ucod_lora_mlp_grad
  size_t u_o, u_2, s_u, t_out, ogw, ogw_bytes;             // output modules: saved u [M, 8] per layer (dense, fc2), t scratch [M, 8], partials of ucod_lora_out_grad_*
  size_t bgw, bgw_bytes;                                   // bias gradients (TB, TN): partials of ucod_colsum_det and its _lora / _tok forms
  size_t total;
};

inline size_t up(size_t v) { return (v + 255) / 256 * 256; }

inline bool known_mlp(int mlp) { return mlp == UCOD_MLP_GELU || mlp == UCOD_MLP_SWIGLU; }
inline int fc1_width(const ucod_vit_desc* d, int mlp) { return mlp == UCOD_MLP_SWIGLU ? 2 * d->F : d->F; }
// mlpl: the pass carries a LoRA module on the MLP input projection (its rank limit and the widths its gradient kernel covers)
// pair (UCOD_LORA_MLP_PAIR): the table describes gate_proj / up_proj of the gated MLP -- only with UCOD_MLP_SWIGLU and a table
// wide (UCOD_LORA_WIDE): the pass sizes and runs the MLP and output modules through the _wide row entry points, supersets of the narrow ones
inline bool is_pair(int out_flags) { return (out_flags & UCOD_LORA_MLP_PAIR) != 0; }
inline bool is_wide(int out_flags) { return (out_flags & UCOD_LORA_WIDE) != 0; }
inline size_t mlp_gw_bytes(const ucod_vit_train_desc* t, int mlp, int out_flags) {
  const int N1 = fc1_width(&t->vit, mlp);
  if (is_wide(out_flags)) return is_pair(out_flags) ? ucod_lora_mlp_pair_grad_workspace_bytes_wide(N1, t->vit.D) : ucod_lora_mlp_grad_workspace_bytes_wide(N1, t->vit.D);
  return is_pair(out_flags) ? ucod_lora_mlp_pair_grad_workspace_bytes(N1, t->vit.D) : ucod_lora_mlp_grad_workspace_bytes(N1, t->vit.D);
}
inline bool valid_mlpl(const ucod_vit_train_desc* t, int mlp, bool mlpl, int out_flags) {
  if (is_pair(out_flags) && !(mlpl && mlp == UCOD_MLP_SWIGLU)) return false;
  return !mlpl || (t->lora_r <= UCOD_LORA_MLP_MAX_R && mlp_gw_bytes(t, mlp, out_flags) != 0);
}
// the output modules a table names (layer 0's parameter slots: the same modules in every layer), and whether the pass can carry them
struct OutMods { bool o, f; };
inline OutMods out_mods(const void* const* TO) { return OutMods{TO && TO[0] != nullptr, TO && TO[2] != nullptr}; }
inline size_t out_ws(const ucod_vit_train_desc* t, int K, bool wide) {
  return wide ? ucod_lora_out_grad_workspace_bytes_wide(t->lora_r, K, t->vit.D) : ucod_lora_out_grad_workspace_bytes(t->lora_r, K, t->vit.D);
}
inline size_t out_gw_bytes(const ucod_vit_train_desc* t, OutMods m, bool wide) {
  const size_t a = m.o ? out_ws(t, t->vit.D, wide) : 0, b = m.f ? out_ws(t, t->vit.F, wide) : 0;
  return a > b ? a : b;
}
inline bool valid_out(const ucod_vit_train_desc* t, int mlp, const void* const* TM, const void* const* TO, int out_flags) {
  const OutMods m = out_mods(TO);
  if (out_flags & ~(UCOD_LORA_OUT_SWIGLU | UCOD_LORA_MLP_PAIR | UCOD_LORA_WIDE)) return false;   // an unknown flag bit
  const bool wide = is_wide(out_flags);
  // (the wide bit only where a table needs it: a pass the narrow forms cover has one spelling)
  if (wide && !(TM && fc1_width(&t->vit, mlp) > 8192) && !(m.f && t->vit.F > 4096)) return false;
  if (!TO) return true;
  if (!m.o && !m.f) return false;                                 // a table that names no module
  // (SwiGLU: the hidden is recomputed from the interleaved, padded [M, 2F] pre-activation -- only with UCOD_LORA_OUT_SWIGLU)
  if (m.f && mlp != UCOD_MLP_GELU && !(out_flags & UCOD_LORA_OUT_SWIGLU)) return false;
  return (!m.o || out_ws(t, t->vit.D, wide) != 0) && (!m.f || out_ws(t, t->vit.F, wide) != 0);
}
bool valid(const Pass& c) {
  const ucod_vit_train_desc* t = c.t;
  if (!t) return false;
  const ucod_vit_desc* d = &t->vit;
  return d->B > 0 && d->C > 0 && d->P > 0 && d->H > 0 && d->W > 0 && d->H % d->P == 0 && d->W % d->P == 0 && d->D > 0 && d->heads > 0 &&
         d->D == d->heads * 64 && d->D % 128 == 0 && d->F % 128 == 0 && d->L >= 1 && d->Kpad % 64 == 0 && d->Kpad >= d->C * d->P * d->P &&
         t->lora_r >= 1 && 3 * t->lora_r <= UCOD_LORA_AUG && ucod_layernorm_lora_fits(d->D, t->lora_r, 3) == 1 &&   // (the 3 r A rows fit one workgroup's LDS)
         t->lora_dropout >= 0.f && t->lora_dropout < 1.f &&
         (d->rope == nullptr || t->allow_rope == 1) &&              // DINOv3: only a caller that names the rotary passes (allow_rope) gets them; a zero-filled field refuses a table
         d->n_reg >= 0 && d->n_reg <= 1023 && (d->resid16 == 0 || d->resid16 == 1) &&   // resid16: the saved residual stream is IEEE fp16 (round 4: LayerNorm backward reads it)
         known_mlp(c.mlp) && valid_mlpl(t, c.mlp, c.TM != nullptr, c.out_flags) && valid_out(t, c.mlp, c.TM, c.TO, c.out_flags);
}

Plan train_plan(const Pass& c) {
  const ucod_vit_train_desc* t = c.t;
  const ucod_vit_desc* d = &t->vit;
  const bool mlpl = c.TM != nullptr;
  Plan p;
  p.save = true;
  const int gh = d->H / d->P, gw = d->W / d->P;
  p.tok = gh * gw + 1 + d->n_reg;                                  // [CLS | n_reg register tokens | patches]
  p.M = d->B * p.tok;
  const size_t M = p.M, D = d->D, L = d->L;
  const size_t FP = fc1_width(d, c.mlp);                      // width of the saved pre-activation and of its cotangent (SwiGLU: x1 | x2 interleaved)
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
    p.mgw_bytes = mlp_gw_bytes(t, c.mlp, c.out_flags);
    p.mgw = take(p.mgw_bytes);
  }
  p.u_o = p.u_2 = p.s_u = p.t_out = p.ogw = p.ogw_bytes = 0;
  if (c.TO) {                                                   // (behind everything else: without a table no offset and no byte differs)
    const OutMods m = out_mods(c.TO);
    p.s_u = up(M * UCOD_LORA_OUT_W * 4);
    if (m.o) p.u_o = take(p.s_u * (L - 1));
    if (m.f) p.u_2 = take(p.s_u * (L - 1));
    p.t_out = take(M * UCOD_LORA_OUT_W * 4);
    p.ogw_bytes = out_gw_bytes(t, m, is_wide(c.out_flags));
    p.ogw = take(p.ogw_bytes);
  }
  p.bgw = p.bgw_bytes = 0;
  if (c.TB || c.TN) {                                           // (behind everything else, like TO: without a table no offset and no byte differs)
    if (c.TB) {
      const size_t a = ucod_colsum_det_workspace_bytes(p.M, 3 * d->D), b = ucod_colsum_det_workspace_bytes(p.M, (int)FP);   // (the widest calls: q | k | v at once, dpre)
      p.bgw_bytes = a > b ? a : b;
    }
    if (c.TN) {   // (TN's calls are all M or fewer rows by D columns: with TB they fit what it counted, and no byte is added)
      const size_t a = ucod_colsum_det_lora_workspace_bytes(p.M, d->D), b = ucod_colsum_det_tok_workspace_bytes(d->B, p.tok, 1 + d->n_reg, d->D);
      if (a > p.bgw_bytes) p.bgw_bytes = a;
      if (b > p.bgw_bytes) p.bgw_bytes = b;
    }
    p.bgw = take(p.bgw_bytes);
  }
  p.total = o;
  return p;
}

// The no-grad pass saves nothing: one residual buffer updated in place (x_in == x_mid, every stride 0), no log-sum-exp, no pre-activation, and the output modules add
// no workspace byte.  Workspace ~ the inference pass's; the residual stream may be IEEE fp16 (vit.resid16) like the frozen-backbone pass's.
Plan infer_plan(const Pass& c) {
  const ucod_vit_desc* d = &c.t->vit;
  Plan p = {};
  const int gh = d->H / d->P, gw = d->W / d->P;
  p.tok = gh * gw + 1 + d->n_reg;
  p.M = d->B * p.tok;
  const size_t M = p.M, D = d->D, F = d->F;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += up(bytes); return r; };
  p.x_in = p.x_mid = take(M * D * (d->resid16 ? 2 : 4));
  p.h_aug = take(M * (D + UCOD_LORA_AUG) * 2);
  p.h2 = take(M * (D + (c.TM ? UCOD_LORA_AUG : 0)) * 2);
  p.qkv = take(M * 3 * D * 2);
  p.att = take(M * D * 2);
  p.g = take(M * F * 2);                                      // (either kind: the hidden [M, F]; SwiGLU's weights_in output never reaches memory)
  p.patch = take((size_t)d->B * gh * gw * d->Kpad * 2);
  p.qscale = take(3 * D * 4);
  p.total = o;
  return p;
}

// the per-layer pointers of a pass, from its plan
struct Slots {
  const Plan& p;
  char* ws;
  char* at(size_t base, size_t stride, int l) const { return ws + base + stride * l; }
  float* x_in(int l) const { return (float*)at(p.x_in, p.s_x, l); }
  float* x_mid(int l) const { return (float*)at(p.x_mid, p.s_x, l); }
  float* x_next(int l) const { return x_in(l + 1); }                        // (not saving: the same buffer, the residual GEMMs run in place)
  void* h_aug(int l) const { return at(p.h_aug, p.s_h, l); }
  void* qkv(int l) const { return at(p.qkv, p.s_qkv, l); }
  void* att(int l) const { return at(p.att, p.s_att, l); }
  float* lse(int l) const { return p.save ? (float*)at(p.lse, p.s_lse, l) : nullptr; }
  void* pre(int l) const { return p.save ? at(p.pre, p.s_pre, l) : nullptr; }
  float* u_o(int l) const { return p.save ? (float*)at(p.u_o, p.s_u, l) : nullptr; }
  float* u_2(int l) const { return p.save ? (float*)at(p.u_2, p.s_u, l) : nullptr; }
};

// The dropout mask of one module in one layer, or NULL with dropout off.  The key is kind * L + l: forward, no-grad forward and backward all take it from here.
enum ModKind { MOD_QKV = 0, MOD_MLP_IN = 1, MOD_DENSE = 2, MOD_FC2 = 3 };
struct Dropout {
  ucod_lora_dropout desc;
  bool on;
  const ucod_lora_dropout* ptr() const { return on ? &desc : nullptr; }
};
inline Dropout dropout_of(const ucod_vit_train_desc* t, ModKind kind, int l) {
  return Dropout{{t->lora_dropout, t->seed, (int)kind * t->vit.L + l}, t->lora_dropout > 0.f};
}

// the kernels that come in a pair, one per type of the residual stream (r16: IEEE fp16, else f32)
inline int layernorm_lora(bool r16, const void* x, const float* gam, const float* bet, const float* lora, int r, void* y_aug, int M, int D, float eps,
                          const ucod_lora_dropout* drop, void* stream) {
  return r16 ? ucod_layernorm_lora_h16(x, gam, bet, lora, r, y_aug, M, D, eps, drop, stream)
             : ucod_layernorm_lora((const float*)x, gam, bet, lora, r, y_aug, M, D, eps, drop, stream);
}
inline int layernorm(bool r16, const void* x, const float* gam, const float* bet, void* y, int M, int D, float eps, void* stream) {
  return r16 ? ucod_layernorm_h16(x, gam, bet, y, M, D, eps, stream) : ucod_layernorm((const float*)x, gam, bet, y, M, D, eps, 0, stream);
}
inline int cls_rows(bool r16, float* x, const float* cls_reg, const float* pos, int B, int tok, int D, int n_reg, void* stream) {
  return r16 ? ucod_cls_rows_h16_reg(x, cls_reg, pos, B, tok, D, n_reg, stream) : ucod_cls_rows_reg(x, cls_reg, pos, B, tok, D, n_reg, stream);
}

#define RUN(call)                \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != 0) return rc__;  \
  } while (0)

size_t train_bytes(const Pass& c) { return valid(c) ? train_plan(c).total : 0; }
size_t infer_bytes(const Pass& c) { return valid(c) ? infer_plan(c).total : 0; }

// Both forward passes.  `save`: the training pass (per-layer slots, log-sum-exp, the *_SAVE_BF16 fc1 drains, u of the output modules); else the no-grad pass.
int forward(const Pass& c, bool save, const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  UCOD_BF16_ONLY();
  if (!valid(c) || !c.T || !c.TT || !img || !key_out || !workspace) return UCOD_EINVAL;
  const ucod_vit_train_desc* t = c.t;
  const ucod_vit_desc* d = &t->vit;
  const bool swiglu = c.mlp == UCOD_MLP_SWIGLU, pair = is_pair(c.out_flags), wide = is_wide(c.out_flags);
  const Plan p = save ? train_plan(c) : infer_plan(c);
  const OutMods om = out_mods(c.TO);
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  const Slots at{p, ws};
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, gv = d->gemm_variant, KA = D + UCOD_LORA_AUG;
  float* qscale = (float*)(ws + p.qscale);
  void* h2 = ws + p.h2;
  void* g = ws + p.g;
  void* patches = ws + p.patch;
  RUN(ucod_fill_qscale(qscale, D, 0.125f * 1.4426950408889634f, stream));

  const bool r16 = d->resid16 != 0;                               // fp16 residual stream (saved as such: half the bytes forward and backward)
  const int epi_patch = r16 ? UCOD_EPI_PATCH_TOKENS_H16 : UCOD_EPI_PATCH_TOKENS_F32;
  const int epi_resid = r16 ? UCOD_EPI_BIAS_SCALE_RESID_H16 : UCOD_EPI_BIAS_SCALE_RESID_F32;
  const int epi_fc1 = save ? (swiglu ? UCOD_EPI_BIAS_SWIGLU_SAVE_BF16 : UCOD_EPI_BIAS_GELU_SAVE_BF16) : (swiglu ? UCOD_EPI_BIAS_SWIGLU_BF16 : UCOD_EPI_BIAS_GELU_BF16);
  float* x0 = at.x_in(0);
  RUN(ucod_patch_im2col(img, patches, d->B, d->C, d->H, d->W, d->P, d->Kpad, stream));
  RUN(ucod_gemm_bf16_reg(epi_patch, patches, c.T[0], x0, d->B * (tok - 1 - d->n_reg), D, d->Kpad, (const float*)c.T[1], nullptr, nullptr,
                         (const float*)c.T[3], tok, d->n_reg, gv, stream));
  RUN(cls_rows(r16, x0, (const float*)c.T[2], (const float*)c.T[3], d->B, tok, D, d->n_reg, stream));

  for (int l = 0; l < d->L; ++l) {
    const void* const* W = c.T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const void* const* X = c.TT + UCOD_VIT_TRAIN_STRIDE * l;
    float* x_in = at.x_in(l);
    void* h_aug = at.h_aug(l);
    RUN(layernorm_lora(r16, x_in, (const float*)W[0], (const float*)W[1], (const float*)X[5], t->lora_r, h_aug, M, D, d->eps, dropout_of(t, MOD_QKV, l).ptr(), stream));
    if (l == d->L - 1) {   // key hook: K rows of the augmented qkv weight; [B,D,h,w] out
      const char* wk = (const char*)X[0] + (size_t)D * KA * 2;
      RUN(ucod_gemm_bf16_reg(UCOD_EPI_KEY_NCHW_F32, wk, h_aug, key_out, D, M, KA, (const float*)W[3] + D, nullptr, nullptr, nullptr, tok, d->n_reg, gv, stream));
      break;
    }
    float* x_mid = at.x_mid(l);
    float* x_next = at.x_next(l);
    void* qkv = at.qkv(l);
    void* att = at.att(l);
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_BF16, h_aug, X[0], qkv, M, 3 * D, KA, (const float*)W[3], qscale, nullptr, nullptr, tok, gv, stream));
    // DINOv3: q and k of the patch rows are rotated in the SAVED buffer, so that the backward's recomputed scores see the operands attention saw
    if (d->rope) RUN(ucod_rope_qk_ld(qkv, UCOD_ROPE_ELEM_HALF, d->rope, d->B, tok, d->n_reg, d->heads, 3 * D, 0, stream));
    if (save) RUN(ucod_attention_fwd_lse(qkv, att, at.lse(l), d->B, tok, d->heads, stream));
    else RUN(ucod_attention_fwd(qkv, att, d->B, tok, d->heads, 0.f, 0, stream));
    RUN(ucod_gemm_bf16(epi_resid, att, W[4], x_mid, M, D, D, (const float*)W[5], (const float*)W[6], x_in, nullptr, tok, gv, stream));
    const void* const* Z = c.TO ? c.TO + UCOD_VIT_TRAIN_OUT_STRIDE * l : nullptr;
    if (om.o)   // LoRA on the attention output projection: x_mid += ls1 * scaling * (drop(att) A_o^T) B_o^T, u saved or dropped
      RUN(ucod_lora_out_fwd(att, (const float*)Z[0], t->lora_r, t->lora_scaling, (const float*)W[6], x_mid, r16, at.u_o(l), M, D, D, dropout_of(t, MOD_DENSE, l).ptr(),
                            stream));
    const void* fc1_w = W[9];
    int fc1_k = D;
    if (c.TM) {   // LoRA on the MLP input projection: LayerNorm 2 + down-projection, fc1 over K = D+64 against fc1_w_aug
      const void* const* Y = c.TM + UCOD_VIT_TRAIN_MLP_STRIDE * l;
      // (UCOD_LORA_MLP_PAIR: the gated MLP's gate_proj / up_proj, two down-projections with masks 0 and 1 of the same key)
      RUN((pair ? ucod_layernorm_lora_mlp_pair : ucod_layernorm_lora_mlp)(x_mid, r16, (const float*)W[7], (const float*)W[8], (const float*)Y[1], t->lora_r, h2, M, D,
                                                                          d->eps, dropout_of(t, MOD_MLP_IN, l).ptr(), stream));
      fc1_w = Y[0];
      fc1_k = KA;
    } else {
      RUN(layernorm(r16, x_mid, (const float*)W[7], (const float*)W[8], h2, M, D, d->eps, stream));
    }
    if (save) RUN(ucod_gemm_bf16_train(epi_fc1, h2, fc1_w, g, M, fc1_width(d, c.mlp), fc1_k, (const float*)W[10], nullptr, at.pre(l), gv, stream));
    else RUN(ucod_gemm_bf16(epi_fc1, h2, fc1_w, g, M, fc1_width(d, c.mlp), fc1_k, (const float*)W[10], nullptr, nullptr, nullptr, tok, gv, stream));
    RUN(ucod_gemm_bf16(epi_resid, g, W[11], x_next, M, D, F, (const float*)W[12], (const float*)W[13], x_mid, nullptr, tok, gv, stream));
    if (om.f)   // LoRA on the MLP output projection: x_next += ls2 * scaling * (drop(g) A_2^T) B_2^T, u saved or dropped
      RUN((wide ? ucod_lora_out_fwd_wide : ucod_lora_out_fwd)(g, (const float*)Z[2], t->lora_r, t->lora_scaling, (const float*)W[13], x_next, r16, at.u_2(l), M, F, D, dropout_of(t, MOD_FC2, l).ptr(), stream));
  }
  return UCOD_OK;
}

int backward(const Pass& c, const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  UCOD_BF16_ONLY();
  if (!valid(c) || !c.T || !c.TT || !dkey || !workspace) return UCOD_EINVAL;
  const ucod_vit_train_desc* t = c.t;
  const ucod_vit_desc* d = &t->vit;
  const void* const* T = c.T;
  const void* const* TT = c.TT;
  const void* const* TM = c.TM;
  const void* const* TO = c.TO;
  const bool swiglu = c.mlp == UCOD_MLP_SWIGLU, pair = is_pair(c.out_flags), wide = is_wide(c.out_flags);
  const Plan p = train_plan(c);
  const OutMods om = out_mods(TO);
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  const Slots at{p, ws};
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, N1 = fc1_width(d, c.mlp), gv = d->gemm_variant, KQ = 3 * D + UCOD_LORA_AUG, r = t->lora_r;
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
  // (s_out: the 16-bit operand of the next dgrad GEMM -- `s`, or NULL where nothing follows: layer 0 under bias="all")
  auto ln_bwd_plain = [&](const void* dy, const void* x, const float* gam, const float* dres, const float* next_scale, void* s_out) -> int {
    return ucod_layernorm_bwd_ex(dy, x, lnb_flags, gam, dres, next_scale, dx, s_out, M, D, d->eps, stream);
  };
  // a bias gradient: the column sums of a 16-bit cotangent buffer (TB; `dst` NULL = that bias is not trained)
  const void* const* TB = c.TB;
  auto bias_grad = [&](const void* dst, const void* cot, int n, int ld) -> int {
    if (!dst) return UCOD_OK;
    return ucod_colsum_det(cot, UCOD_ROPE_ELEM_HALF, M, n, ld, nullptr, (float*)const_cast<void*>(dst), ws + p.bgw, p.bgw_bytes, stream);
  };
  auto bias_zero = [&](const void* dst, int n) -> int {
    if (dst && hipMemsetAsync(const_cast<void*>(dst), 0, (size_t)n * sizeof(float), (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
    return UCOD_OK;
  };
  auto qkv_side = [&](int l) -> int {   // dqkv_aug (k/q/v thirds filled) -> LoRA grads of layer l, dh = d LN1 output
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    if (TB) {   // q / k / v biases: the thirds of dqkv, cotangents of the projection outputs (the last layer: only the key third reaches the key map)
      const void* const* G = TB + UCOD_VIT_TRAIN_BIAS_STRIDE * l;
      const bool is_last = l == d->L - 1;
      // (all three trained and side by side, as one arena row holds them: one pass over the 3 D columns instead of three over D)
      const bool together = !is_last && G[0] && G[1] == (const float*)G[0] + D && G[2] == (const float*)G[0] + 2 * D;
      if (together) {
        RUN(bias_grad(G[0], dqkv, 3 * D, KQ));
      } else {
        if (is_last) RUN(bias_zero(G[0], D));
        else RUN(bias_grad(G[0], dqkv, D, KQ));
        RUN(bias_grad(G[1], (const char*)dqkv + (size_t)D * 2, D, KQ));
        if (is_last) RUN(bias_zero(G[2], D));
        else RUN(bias_grad(G[2], (const char*)dqkv + (size_t)2 * D * 2, D, KQ));
      }
    }
    RUN(ucod_lora_grad(dqkv, at.h_aug(l), (const float*)X[5], r, t->lora_scaling, (float*)X[6], 0, lgw, lgw_bytes, M, D, dropout_of(t, MOD_QKV, l).ptr(), stream));
    RUN(ucod_gemm_bf16(epi_dh, dqkv, X[1], dh, M, D, KQ, nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    return UCOD_OK;
  };

  // LayerNorm-1 backward of layer l: with dropout on, the masked LoRA branch t A is added here (it cannot ride on the dgrad GEMM)
  auto ln1_bwd = [&](int l, const void* dy, const void* x, const float* gam, const float* dres, const float* next_scale, void* s_out) -> int {
    const Dropout drop = dropout_of(t, MOD_QKV, l);
    if (drop.on) {
      const float* lora_l = (const float*)(TT + UCOD_VIT_TRAIN_STRIDE * l)[5];
      return ucod_layernorm_bwd_lora_ex(dy, x, lnb_flags, gam, dres, next_scale, dx, s_out, M, D, d->eps, dqkv, lora_l, r, drop.ptr(), stream);
    }
    return ln_bwd_plain(dy, x, gam, dres, next_scale, s_out);
  };

  // bias="all" (TN): the LayerNorm betas and the patch embedding's bias.  d beta = the column sums of the LayerNorm output's COMPLETE cotangent: dh, plus the masked
  // LoRA branch wherever the LayerNorm backward adds it in registers -- then from that kernel's own operands (ucod_colsum_det_lora)
  const void* const* TN = c.TN;
  const int dh_elem = dgrad16 ? UCOD_ROPE_ELEM_HALF : UCOD_ROPE_ELEM_F32;
  auto beta1_grad = [&](int l) -> int {   // behind qkv_side(l), which leaves dh; in front of whatever next overwrites dh
    float* dst = TN ? (float*)const_cast<void*>(TN[1 + 2 * l]) : nullptr;
    if (!dst) return UCOD_OK;
    const Dropout drop = dropout_of(t, MOD_QKV, l);
    if (!drop.on) return ucod_colsum_det(dh, dh_elem, M, D, D, nullptr, dst, ws + p.bgw, p.bgw_bytes, stream);   // (the branch rode on the dgrad GEMM)
    return ucod_colsum_det_lora(dh, lnb_flags, M, D, (const char*)dqkv + (size_t)3 * D * 2, KQ, (const float*)(TT + UCOD_VIT_TRAIN_STRIDE * l)[5], 3, r, drop.ptr(), dst,
                                ws + p.bgw, p.bgw_bytes, stream);
  };
  auto beta2_grad = [&](int l, const void* const* Y, const Dropout& drop_m) -> int {   // behind the fc1 dgrad; dpre has no aug columns, so the branch is always added
    float* dst = TN ? (float*)const_cast<void*>(TN[2 + 2 * l]) : nullptr;
    if (!dst) return UCOD_OK;
    if (!Y) return ucod_colsum_det(dh, dh_elem, M, D, D, nullptr, dst, ws + p.bgw, p.bgw_bytes, stream);
    return ucod_colsum_det_lora(dh, lnb_flags, M, D, ws + p.tm, UCOD_LORA_AUG, (const float*)Y[1], pair ? 2 : 1, r, drop_m.ptr(), dst, ws + p.bgw, p.bgw_bytes, stream);
  };
  // the patch embedding's bias: the first residual state's cotangent, which the pass otherwise never forms (layer 0's LayerNorm-1 backward), over the patch rows
  auto patch_grad = [&](const float* dres) -> int {
    if (!TN || !TN[0]) return UCOD_OK;
    RUN(ln1_bwd(0, dh, at.x_in(0), (const float*)(T + 4)[0], dres, nullptr, nullptr));
    return ucod_colsum_det_tok(dx, UCOD_ROPE_ELEM_F32, d->B, tok, 1 + d->n_reg, D, D, nullptr, (float*)const_cast<void*>(TN[0]), ws + p.bgw, p.bgw_bytes, stream);
  };

  // last layer: only the key projection reaches the loss (its MLP never runs: the module's gradients there are zeros, written as such)
  const int last = d->L - 1;
  if (TM) {
    const size_t n_m = (size_t)r * (size_t)((pair ? 2 : 1) * D + N1) * sizeof(float);
    if (hipMemsetAsync(const_cast<void*>((TM + UCOD_VIT_TRAIN_MLP_STRIDE * last)[2]), 0, n_m, (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
  }
  if (TO) {   // (nor do its attention output and fc2: zeros, written as such)
    const void* const* Z = TO + UCOD_VIT_TRAIN_OUT_STRIDE * last;
    if (om.o && hipMemsetAsync(const_cast<void*>(Z[1]), 0, (size_t)r * (size_t)(D + D) * sizeof(float), (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
    if (om.f && hipMemsetAsync(const_cast<void*>(Z[3]), 0, (size_t)r * (size_t)(F + D) * sizeof(float), (hipStream_t)stream) != hipSuccess) return UCOD_EINVAL;
  }
  if (TB) {   // (nor do the biases of its MLP and output projections)
    const void* const* G = TB + UCOD_VIT_TRAIN_BIAS_STRIDE * last;
    RUN(bias_zero(G[3], N1));
    RUN(bias_zero(G[4], D));
    RUN(bias_zero(G[5], D));
  }
  if (TN) RUN(bias_zero(TN[2 + 2 * last], D));   // (nor does its LayerNorm 2)
  RUN(ucod_key_grad_tokens_reg(dkey, dqkv, d->B, tok, D, d->n_reg, stream));
  RUN(qkv_side(last));
  RUN(beta1_grad(last));
  if (last == 0) return patch_grad(nullptr);
  {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * last;
    const void* const* Wp = T + 4 + UCOD_VIT_LAYER_STRIDE * (last - 1);
    RUN(ln1_bwd(last, dh, at.x_in(last), (const float*)W[0], nullptr, (const float*)Wp[13], s));
  }
  for (int l = last - 1; l >= 0; --l) {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const void* const* X = TT + UCOD_VIT_TRAIN_STRIDE * l;
    const float* x_in = at.x_in(l);
    const float* x_mid = at.x_mid(l);
    const void* qkv = at.qkv(l);
    const void* att = at.att(l);
    const void* pre = at.pre(l);
    const void* const* G = TB ? TB + UCOD_VIT_TRAIN_BIAS_STRIDE * l : nullptr;
    // fc2 / weights_out bias: x_next = x_mid + ls2 * (g W2^T + b2), so db2 = ls2 * sum dx = the column sums of s = bf16(ls2 * dx), before anything reuses its buffer
    if (G) RUN(bias_grad(G[5], s, D, D));
    // MLP branch: s = ls2 * dx  ->  fc2 dgrad (x gelu')  ->  fc1 dgrad  ->  LN2 backward + residual
    // (SwiGLU: the weights_out dgrad's drain writes the cotangent of the interleaved weights_in output, dpre [M, 2F]; X[3] = weights_in^T [D, 2F] in that column order)
    RUN(ucod_gemm_bf16_train(swiglu ? UCOD_EPI_SWIGLU_BWD_BF16 : UCOD_EPI_GELU_BWD_BF16, s, X[4], dpre, M, F, D, nullptr, pre, nullptr, gv, stream));
    const void* const* Z = TO ? TO + UCOD_VIT_TRAIN_OUT_STRIDE * l : nullptr;
    if (om.f) {
      // LoRA on the MLP output projection, while `s` (= bf16(ls2 * dx), the fc2 dgrad's operand) is still there: t = scaling * s B_2 and dB_2 from s and the saved u,
      // then dA_2 from t and the hidden recomputed as gelu(pre), and dpre += gelu'(pre) * mask/(1-p) * (t A_2) -- completed before anything below reads dpre
      // (SwiGLU, UCOD_LORA_OUT_SWIGLU: the hidden is silu(x1) * x2 of the interleaved pre [M, 2F], and dpre [M, 2F] takes the term through both derivative factors)
      float* gz = (float*)const_cast<void*>(Z[3]);
      RUN((wide ? ucod_lora_out_grad_s_wide : ucod_lora_out_grad_s)(s, at.u_2(l), (const float*)Z[2], r, t->lora_scaling, gz, (float*)(ws + p.t_out), ws + p.ogw, p.ogw_bytes, M, F, D, stream));
      RUN(ucod_lora_out_grad_x_ex(pre, swiglu ? UCOD_LORA_OUT_ACT_SWIGLU : UCOD_LORA_OUT_ACT_GELU, (swiglu ? UCOD_LORA_OUT_SWIGLU : 0) | (wide ? UCOD_LORA_WIDE : 0), dpre,
                                  (const float*)(ws + p.t_out), (const float*)Z[2], r, gz, ws + p.ogw, p.ogw_bytes, M, F, D, dropout_of(t, MOD_FC2, l).ptr(), stream));
    }
    // fc1 / weights_in bias: the column sums of the completed dpre (SwiGLU: the engine's padded, interleaved column order; padded columns hold exact zeros)
    if (G) RUN(bias_grad(G[3], dpre, N1, N1));
    const Dropout drop_m = dropout_of(t, MOD_MLP_IN, l);
    const void* const* Y = TM ? TM + UCOD_VIT_TRAIN_MLP_STRIDE * l : nullptr;
    if (TM) {
      // LoRA on the MLP input projection.  `s` (the fc2 dgrad's operand) has been consumed: its buffer takes h2_aug, recomputed from the saved residual
      // stream with the forward's launch (same mask), and is rewritten by the LayerNorm-2 backward below, after the gradient kernel has read it
      void* h2_aug = ws + p.h2;
      // (UCOD_LORA_MLP_PAIR: the three calls take their _pair forms -- same arguments, [A_g | A_u | B_m] behind Y[1] / Y[2])
      RUN((pair ? ucod_layernorm_lora_mlp_pair : ucod_layernorm_lora_mlp)(x_mid, r16, (const float*)W[7], (const float*)W[8], (const float*)Y[1], r, h2_aug, M, D,
                                                                          d->eps, drop_m.ptr(), stream));
      const auto mlp_grad = wide ? (pair ? ucod_lora_mlp_pair_grad_wide : ucod_lora_mlp_grad_wide) : (pair ? ucod_lora_mlp_pair_grad : ucod_lora_mlp_grad);
      RUN(mlp_grad(dpre, h2_aug, (const float*)Y[1], r, t->lora_scaling, (float*)const_cast<void*>(Y[2]), ws + p.tm, ws + p.mgw, p.mgw_bytes, M, N1, D,
                   drop_m.ptr(), stream));
    }
    RUN(ucod_gemm_bf16(epi_dh, dpre, X[3], dh, M, D, N1, nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    RUN(beta2_grad(l, Y, drop_m));
    if (TM) RUN((pair ? ucod_layernorm_bwd_lora_mlp_pair : ucod_layernorm_bwd_lora_mlp)(dh, x_mid, lnb_flags, (const float*)W[7], dx, (const float*)W[6], dx, s, M, D, d->eps, ws + p.tm, UCOD_LORA_AUG,
                                            (const float*)Y[1], r, drop_m.ptr(), stream));
    else RUN(ln_bwd_plain(dh, x_mid, (const float*)W[7], dx, (const float*)W[6], s));
    // attention branch: s = ls1 * dx  ->  out-proj dgrad  ->  attention backward  ->  LoRA grads + qkv dgrad  ->  LN1 backward
    // (dense / o_proj bias: db_o = ls1 * sum dx = the column sums of s, which stays as it is until the LayerNorm-1 backward rewrites it)
    if (G) RUN(bias_grad(G[4], s, D, D));
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_BF16, s, X[2], da, M, D, D, nullptr, nullptr, nullptr, nullptr, tok, gv, stream));
    if (om.o) {   // LoRA on the attention output projection: s = bf16(ls1 * dx); da += mask/(1-p) * (t A_o) before attention backward reads it
      float* gz = (float*)const_cast<void*>(Z[1]);
      RUN(ucod_lora_out_grad_s(s, at.u_o(l), (const float*)Z[0], r, t->lora_scaling, gz, (float*)(ws + p.t_out), ws + p.ogw, p.ogw_bytes, M, D, D, stream));
      RUN(ucod_lora_out_grad_x(att, UCOD_LORA_OUT_ACT_IDENTITY, da, (const float*)(ws + p.t_out), (const float*)Z[0], r, gz, ws + p.ogw, p.ogw_bytes, M, D, D,
                               dropout_of(t, MOD_DENSE, l).ptr(), stream));
    }
    RUN(ucod_attention_bwd(qkv, att, da, at.lse(l), delta, dqkv, KQ, d->B, tok, d->heads, stream));
    // DINOv3: dq / dk above are the cotangents of the ROTATED operands; the LoRA-gradient kernel and the QKV dgrad want those of the projection outputs,
    // d(pre) = R^T d(post) -- the same table with the sine negated, on the q | k thirds of dqkv_aug (attention_bwd.hip stores dq at 0, dk at D, dv at 2 D)
    if (d->rope) RUN(ucod_rope_qk_ld(dqkv, UCOD_ROPE_ELEM_HALF, d->rope, d->B, tok, d->n_reg, d->heads, KQ, 1, stream));
    RUN(qkv_side(l));
    RUN(beta1_grad(l));
    if (l > 0) {
      const void* const* Wp = T + 4 + UCOD_VIT_LAYER_STRIDE * (l - 1);
      RUN(ln1_bwd(l, dh, x_in, (const float*)W[0], dx, (const float*)Wp[13], s));
    }
  }
  return patch_grad(dx);
}

}  // namespace

// The exported symbols (include/ucod_dpl.h): five functions in five tiers.  Each fills in Pass{t, mlp, out_flags, T, TT, TM, TO} -- an older tier with UCOD_MLP_GELU,
// 0 or NULL where it has no argument -- and calls its function above.
extern "C" size_t ucod_vit_train_workspace_bytes(const ucod_vit_train_desc* t) { return train_bytes(Pass{t, UCOD_MLP_GELU, 0, nullptr, nullptr, nullptr, nullptr}); }
extern "C" size_t ucod_vit_train_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp) { return train_bytes(Pass{t, mlp, 0, nullptr, nullptr, nullptr, nullptr}); }
extern "C" size_t ucod_vit_train_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* TM) {
  return train_bytes(Pass{t, mlp, 0, nullptr, nullptr, TM, nullptr});
}
extern "C" size_t ucod_vit_train_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* TM, const void* const* TO) {
  return train_bytes(Pass{t, mlp, 0, nullptr, nullptr, TM, TO});
}
extern "C" size_t ucod_vit_train_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM, const void* const* TO) {
  return train_bytes(Pass{t, mlp, out_flags, nullptr, nullptr, TM, TO});
}

extern "C" int ucod_vit_forward_train(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* img, float* key_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return forward(Pass{t, UCOD_MLP_GELU, 0, T, TT, nullptr, nullptr}, true, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* img, float* key_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, nullptr, nullptr}, true, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                               const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, TM, nullptr}, true, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                               const void* const* TO, const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, TM, TO}, true, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_train_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT,
                                                  const void* const* TM, const void* const* TO, const float* img, float* key_out, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, out_flags, T, TT, TM, TO}, true, img, key_out, workspace, workspace_bytes, stream);
}

extern "C" int ucod_vit_backward(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* dkey, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return backward(Pass{t, UCOD_MLP_GELU, 0, T, TT, nullptr, nullptr}, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* dkey, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, 0, T, TT, nullptr, nullptr}, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM, const float* dkey,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, 0, T, TT, TM, nullptr}, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                          const void* const* TO, const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, 0, T, TT, TM, TO}, dkey, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_backward_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT, const void* const* TM,
                                             const void* const* TO, const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, out_flags, T, TT, TM, TO}, dkey, workspace, workspace_bytes, stream);
}

// bias="lora_only": the backward and its workspace with the bias table (NULL = the _lora_out_ex forms, which delegate with NULL)
extern "C" size_t ucod_vit_train_workspace_bytes_lora_bias(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM, const void* const* TO,
                                                           const void* const* TB) {
  return train_bytes(Pass{t, mlp, out_flags, nullptr, nullptr, TM, TO, TB});
}
extern "C" int ucod_vit_backward_lora_bias(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT, const void* const* TM,
                                           const void* const* TO, const void* const* TB, const float* dkey, void* workspace, size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, out_flags, T, TT, TM, TO, TB}, dkey, workspace, workspace_bytes, stream);
}

// bias="all": the same two with the norm table (NULL = the _lora_bias forms, which delegate with NULL)
extern "C" size_t ucod_vit_train_workspace_bytes_lora_bias_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM, const void* const* TO,
                                                              const void* const* TB, const void* const* TN) {
  return train_bytes(Pass{t, mlp, out_flags, nullptr, nullptr, TM, TO, TB, TN});
}
extern "C" int ucod_vit_backward_lora_bias_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT, const void* const* TM,
                                              const void* const* TO, const void* const* TB, const void* const* TN, const float* dkey, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return backward(Pass{t, mlp, out_flags, T, TT, TM, TO, TB, TN}, dkey, workspace, workspace_bytes, stream);
}

extern "C" size_t ucod_vit_lora_infer_workspace_bytes(const ucod_vit_train_desc* t) { return infer_bytes(Pass{t, UCOD_MLP_GELU, 0, nullptr, nullptr, nullptr, nullptr}); }
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_mlp(const ucod_vit_train_desc* t, int mlp) {
  return infer_bytes(Pass{t, mlp, 0, nullptr, nullptr, nullptr, nullptr});
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* TM) {
  return infer_bytes(Pass{t, mlp, 0, nullptr, nullptr, TM, nullptr});
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* TM, const void* const* TO) {
  return infer_bytes(Pass{t, mlp, 0, nullptr, nullptr, TM, TO});
}
extern "C" size_t ucod_vit_lora_infer_workspace_bytes_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* TM, const void* const* TO) {
  return infer_bytes(Pass{t, mlp, out_flags, nullptr, nullptr, TM, TO});
}

extern "C" int ucod_vit_forward_lora_infer(const ucod_vit_train_desc* t, const void* const* T, const void* const* TT, const float* img, float* key_out,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, UCOD_MLP_GELU, 0, T, TT, nullptr, nullptr}, false, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const float* img, float* key_out,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, nullptr, nullptr}, false, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_lora_mlp(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                                    const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, TM, nullptr}, false, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_lora_out(const ucod_vit_train_desc* t, int mlp, const void* const* T, const void* const* TT, const void* const* TM,
                                                    const void* const* TO, const float* img, float* key_out, void* workspace, size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, 0, T, TT, TM, TO}, false, img, key_out, workspace, workspace_bytes, stream);
}
extern "C" int ucod_vit_forward_lora_infer_lora_out_ex(const ucod_vit_train_desc* t, int mlp, int out_flags, const void* const* T, const void* const* TT,
                                                       const void* const* TM, const void* const* TO, const float* img, float* key_out, void* workspace,
                                                       size_t workspace_bytes, void* stream) {
  return forward(Pass{t, mlp, out_flags, T, TT, TM, TO}, false, img, key_out, workspace, workspace_bytes, stream);
}
