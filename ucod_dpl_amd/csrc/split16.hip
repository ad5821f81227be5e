// Split-operand backbone forward on fp16 TERMS ("split2h"): every f32 operand of a matrix product as a sum of TWO IEEE fp16 values of a power-of-two multiple of it,
//   hi = fp16(s v),   lo = fp16(s v - hi)        (the subtraction is exact in f32; s = 2^e per operand, so multiplying and dividing by it is exact)
// and the product as the three partial products a_hi b_hi + a_hi b_lo + a_lo b_hi, each exact in the f32 accumulator of the fp16 MFMA.  An fp16 term carries 11
// significand bits, two carry 22: the dropped a_lo b_lo has relative weight 2^-22, against 2^-16 for the two-term bf16 form (split.hip, terms = 2) at the SAME
// three products, and 2^-24 for the three-term bf16 form at six.
//
// Error model of the split (tests/test_split16_host.py restates it on the host, tests/test_gpu_split16.py checks the kernels against that restatement):
//   |v - (hi + lo) / s| <= max(2^-22 |v|, 2^-25 / s)
// The first term is the rounding of lo to 11 bits; the second is fp16's subnormal spacing 2^-24 (half of it), which lo meets when |s v| < 2^-3.  fp16 also
// SATURATES: |s v| > 65504 has no finite hi.  So every operand class carries a scale chosen from a stated bound on its values (kScale below), every writer clamps
// to +-65504 and COUNTS the elements it had to clamp into the saturation counter of the fp16 stream (common.h: resid16_overflow_counter; polled by the engine's
// check_overflow), and weights are scaled per tensor at load so that max |s w| lies in (2^13, 2^14] (the engine; ucod_split16_rows takes any power of two).
//
// The partial products ride on the EXISTING fp16-build GEMM kernels (gemm_bf16.hip with -DUCOD_HALF_F16) by concatenation along K, exactly as in split.hip: an
// [M, K] operand is fp16 [M, 3 K], A side (role 0) = hi | hi | lo, B side (role 1) = hi | lo | hi.  The accumulator then holds s_a s_b times the product.  The
// factor leaves it exactly, through the arguments the epilogues already take (the kernels are untouched):
//   UCOD_EPI_BIAS_SCALE_RESID_F32   resid + scale (C + bias):  bias' = s_a s_b bias, scale' = scale / (s_a s_b)  -- (C + bias') = s_a s_b (C / (s_a s_b) + bias) to
//                                   the last bit (a power of two commutes with rounding), so the stream is what the unscaled product would give, bit for bit
//   UCOD_EPI_BIAS_F32               bias' = s_a s_b bias: the f32 result is s_a s_b times QKV / fc1; the consumer (ucod_split16_qkv, ucod_split16_rows) multiplies
//                                   by 1 / (s_a s_b) as it reads
//   UCOD_EPI_PATCH_TOKENS_F32       bias', pos' (and the CLS rows) times s_a s_b, then one in-place pass x *= 1 / (s_a s_b)       (ucod_split16_scale_f32)
//   UCOD_EPI_KEY_NCHW_F32           bias' = s_a s_b bias, then the same in-place pass over the key map
// fc1 can also leave as the split operand of fc2 straight from the GEMM's drain (ucod_split16_gemm_act; UCOD_SPLIT16_FUSE_MLP in the pass):
//   UCOD_EPI_BIAS_GELU_SPLIT16 /    bias' = s_a s_b bias, act_alpha = 1 / (s_a s_b), act_scale = the HIDDEN class scale: the drain calls gelu_exact / silu_f32 and
//   UCOD_EPI_BIAS_SWIGLU_SPLIT16    split_pair (common.h) on the f32 value the pair above passes through memory -- the same bits, one launch, no f32 [M, F] buffer
// Everything between the GEMMs is f32 as in split.hip: residual stream, two-pass LayerNorm, exact-erf GELU / f32 SiLU, softmax.
//
// Attention (attn_split16_kernel): attn_split_kernel<2, 1> of split.hip on v_mfma_f32_32x32x16_f16 -- same LDS layout, software pipeline and register budget (a
// term is 2 bytes either way).  Q (times head_dim^-0.5 log2 e), K and V carry the q/k/v class scale s; the scores leave the MFMA as s^2 S and enter the exponential
// through one FMA, exp2(s^-2 S' - m).  The probabilities lie in [0, 1]: scaled by 2^14 before their split (hi <= 16384, lo's floor 2^-39), and the output is
// divided by 2^14 s together with the softmax denominator.
//
// Does the fp16 MFMA keep SUBNORMAL fp16 inputs?  ucod_split16_mfma_subnormal_probe multiplies 2^-24 (the smallest subnormal) by 2^14 on the matrix pipe: 2^-10 if
// kept, 0 if flushed.  DESIGN.md section 5.2 records what the hardware answers; with flushed inputs a lo term below 2^-14 is lost whole and the floor of the
// model above is 2^-14 / s instead of 2^-25 / s.
//
// Reference arithmetic: transformers modeling_dinov2.py:38-149,153-235,238-297,300-315,342-381 and data/utils/feature_extractor.py:42-59 (key hook) -- the three
// passes the reference runs in plain fp32: data/datasets/base_dataset.py:124-138, generate_pseudo_label.py:71-89, data/datasets/lr_dataset.py:97-157.
// fp16-operand build only (libucod_dpl_f16.so); the bf16 build exports the same names and returns UCOD_EINVAL.
#include <cmath>
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace s16 {

// Operand classes and their scales.  Bound = 65504 / scale; floor of the reconstruction = 2^-25 / scale.
//   LN      LayerNorm output: |(x - mean) rstd| <= sqrt(D - 1) < 39.2 for D <= 1536, times |gamma| (<= ~10 in DINOv2 checkpoints) plus beta: bound 1023
//   QKV     q (already times 0.18), k, v: projections of LayerNorm rows; bound 2047
//   PROB    softmax probabilities, [0, 1]: bound 3.998
//   ATT     attention output, a convex combination of v rows: the bound of QKV
//   HIDDEN  GELU / SwiGLU output of the MLP (the massive activations of DINOv2 are born here: hundreds): bound 4094
//   PATCH   normalised pixels (ImageNet statistics: |v| <= 2.65; random test images: ~6): bound 127.9
constexpr float kScale[UCOD_SPLIT16_NUM_CLASSES] = {64.f, 32.f, 16384.f, 32.f, 16.f, 512.f};

inline bool pow2_ok(float s) {                                   // a finite normal power of two whose reciprocal is normal too
  int e = 0;
  return s > 0.f && std::isfinite(s) && std::frexp(s, &e) == 0.5f && e > -100 && e < 100;
}
inline bool ln_width_ok(int D) {                                 // the D / 128 cases layernorm_split16_kernel is instantiated for
  if (D <= 0 || (D % 128) != 0) return false;
  const int n = D / 128;
  return n == 1 || n == 2 || n == 3 || n == 4 || n == 5 || n == 6 || n == 8 || n == 10 || n == 12;
}
inline int blocks_for(long total) { const long b = (total + 255) / 256; return (int)(b < 65536 ? (b > 0 ? b : 1) : 65536); }

}  // namespace s16
}  // namespace ucod

#ifdef UCOD_HALF_F16
namespace ucod {
namespace s16 {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// gelu_exact and split_pair -- (hi pair, lo pair) of two already scaled values, counted and clamped -- live in common.h: the fused fc1 drain shares them
// probabilities and other values known to lie inside the range: no clamp, no count
__device__ __forceinline__ u32x2 split_pair_inrange(float a, float b) {
  const unsigned hi = pack_f16x2(a, b);
  float ha, hb;
  unpack_f16x2(hi, ha, hb);
  return (u32x2){hi, pack_f16x2(a - ha, b - hb)};
}
__device__ __forceinline__ void report(unsigned sat, unsigned* ovf) {
  if (sat != 0u && ovf) atomicAdd(ovf, sat);
}

// 8 consecutive scaled f32 values -> hi / lo words
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& hi, u32x4& lo, unsigned& sat) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const u32x2 t = split_pair(v[2 * e], v[2 * e + 1], sat);
    hi[e] = t[0];
    lo[e] = t[1];
  }
}
// ... -> one 16-byte store per segment of the K-concatenated GEMM layout: role 0 (A side) hi | hi | lo, role 1 (B side) hi | lo | hi
__device__ __forceinline__ void store_split8(const float (&v)[8], h_raw* __restrict__ seg0, long seg_stride, int role, unsigned& sat) {
  u32x4 hi, lo;
  split8(v, hi, lo, sat);
  *reinterpret_cast<u32x4*>(seg0) = hi;
  *reinterpret_cast<u32x4*>(seg0 + seg_stride) = role ? lo : hi;
  *reinterpret_cast<u32x4*>(seg0 + 2 * seg_stride) = role ? hi : lo;
}

// ---- f32 [M, K] (row pitch ld_in) -> fp16 [M, 3 K] of scale * f(alpha * in); op 0: f = identity with alpha ignored, 1: exact-erf GELU, 2: identity,
// 3: SwiGLU of rows 2 K wide interleaved in blocks of 4 (include/ucod_dpl.h, UCOD_EPI_BIAS_SWIGLU_BF16)
__global__ __launch_bounds__(256) void split16_rows_kernel(const float* __restrict__ in, long ld_in, h_raw* __restrict__ out, int M, int K, int role, int op, float alpha,
                                                           float scale, unsigned* __restrict__ ovf) {
  const int k8 = K >> 3;
  const long total = (long)M * k8;
  unsigned sat = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / k8;
    const int c = (int)(i - m * k8) * 8;
    float v[8];
    if (op == 3) {                                                 // output columns c .. c+7 <- input columns 2c .. 2c+15: (x1 | x2) of c .. c+3, then of c+4 .. c+7
      const float4* src = reinterpret_cast<const float4*>(in + m * ld_in + 2 * c);
      const float4 x1a = src[0], x2a = src[1], x1b = src[2], x2b = src[3];
      const float a1[8] = {x1a.x, x1a.y, x1a.z, x1a.w, x1b.x, x1b.y, x1b.z, x1b.w}, a2[8] = {x2a.x, x2a.y, x2a.z, x2a.w, x2b.x, x2b.y, x2b.z, x2b.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = silu_f32(a1[e] * alpha) * (a2[e] * alpha) * scale;
    } else {
      const float4* src = reinterpret_cast<const float4*>(in + m * ld_in + c);
      const float4 a = src[0], b = src[1];
      const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (op == 1 ? gelu_exact(x[e] * alpha) : op == 2 ? x[e] * alpha : x[e]) * scale;
    }
    store_split8(v, out + m * 3L * K + c, K, role, sat);
  }
  report(sat, ovf);
}

// ---- LayerNorm (two-pass f32, biased variance + eps: nn.LayerNorm, modeling_dinov2.py:348-381) of an f32 row, written as the split operand of the next GEMM.
// One wave per row, the row in registers; lane l holds columns 2 l + 128 i (D % 128 == 0).
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_split16_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                h_raw* __restrict__ out, int rows, int D, float eps, int role, float scale, unsigned* __restrict__ ovf) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float2* xr = reinterpret_cast<const float2*>(x + (size_t)row * D);
  float2 v[NCH];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    v[i] = xr[lane + 64 * i];
    s += v[i].x + v[i].y;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const float a = v[i].x - mean, b = v[i].y - mean;
    q += a * a + b * b;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  const float2* g2 = reinterpret_cast<const float2*>(gamma);
  const float2* b2 = reinterpret_cast<const float2*>(beta);
  unsigned* orow = reinterpret_cast<unsigned*>(out + (size_t)row * 3 * D);
  const int seg = D >> 1;                                        // segment pitch in 32-bit words
  unsigned sat = 0;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const float2 g = g2[lane + 64 * i], b = b2[lane + 64 * i];
    const float o0 = (v[i].x - mean) * rstd * g.x + b.x, o1 = (v[i].y - mean) * rstd * g.y + b.y;
    const u32x2 t = split_pair(o0 * scale, o1 * scale, sat);
    const int w = lane + 64 * i;
    orow[w] = t[0];
    orow[seg + w] = role ? t[1] : t[0];
    orow[2 * seg + w] = role ? t[0] : t[1];
  }
  report(sat, ovf);
}

// ---- img [B,C,H,W] f32 -> split patches fp16 [B gh gw, 3 Kpad] (A side); one thread per (patch, k pair); k >= C P P is zero padding
__global__ __launch_bounds__(256) void im2col_split16_kernel(const float* __restrict__ img, h_raw* __restrict__ out, int B, int C, int H, int W, int Pp, int Kpad, int gh, int gw,
                                                             float scale, unsigned* __restrict__ ovf) {
  const int kp = Kpad >> 1;
  const size_t total = (size_t)B * gh * gw * kp;
  const int K = C * Pp * Pp;
  unsigned sat = 0;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(idx % kp) * 2;
    const size_t m = idx / kp;
    const int px = (int)(m % gw), py = (int)((m / gw) % gh), b = (int)(m / ((size_t)gw * gh));
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k + j;
      if (kk < K) {
        const int c = kk / (Pp * Pp), r = kk - c * Pp * Pp;
        const int dy = r / Pp, dx = r - dy * Pp;
        v[j] = img[(((size_t)b * C + c) * H + (py * Pp + dy)) * W + (px * Pp + dx)] * scale;
      } else {
        v[j] = 0.f;
      }
    }
    const u32x2 t = split_pair(v[0], v[1], sat);
    h_raw* orow = out + m * (size_t)3 * Kpad + k;
    *reinterpret_cast<unsigned*>(orow) = t[0];
    *reinterpret_cast<unsigned*>(orow + Kpad) = t[0];
    *reinterpret_cast<unsigned*>(orow + 2 * (size_t)Kpad) = t[1];
  }
  report(sat, ovf);
}

// ---- in-place x *= alpha (alpha a power of two: exact) -- the token rows after the patch embedding and the key map after the key hook
__global__ __launch_bounds__(256) void scale_f32_kernel(float* __restrict__ x, size_t n, float alpha) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] *= alpha;
}

// ---- f32 qkv [B tok, 3 D] (times `in_mul`: the reciprocal of the QKV GEMM's operand scales) -> the attention kernel's operands, per (image, head), padded to
// tok_pad = 32-row blocks (pad rows are zeros); every value times `scale` before its split:
//   Qc [BH][tok_pad][2 64]   hi | lo of Q times qscale = head_dim^-0.5 log2 e
//   Kc [BH][tok_pad][2 64]   hi | lo of K
//   Vt [2][BH][64][tok_pad]  V transposed, one plane per term
// One workgroup per (32-token block, image * head).
__global__ __launch_bounds__(256) void qkv_split16_kernel(const float* __restrict__ qkv, h_raw* __restrict__ Qc, h_raw* __restrict__ Kc, h_raw* __restrict__ Vt, int tok, int tok_pad,
                                                          int heads, int D, float in_mul, float qscale, float scale, unsigned* __restrict__ ovf) {
  __shared__ float vs[32][65];
  const int tb = blockIdx.x, bh = blockIdx.y;
  const int b = bh / heads, hd = bh - b * heads;
  const int tid = threadIdx.x;
  const int tl = tid >> 3, d8 = (tid & 7) * 8;
  const int t = tb * 32 + tl;
  const bool live = t < tok;
  float q[8], k[8], v[8];
  if (live) {
    const float* row = qkv + ((size_t)b * tok + t) * 3 * D + hd * 64 + d8;
    const float4 q0 = *reinterpret_cast<const float4*>(row), q1 = *reinterpret_cast<const float4*>(row + 4);
    const float4 k0 = *reinterpret_cast<const float4*>(row + D), k1 = *reinterpret_cast<const float4*>(row + D + 4);
    const float4 v0 = *reinterpret_cast<const float4*>(row + 2 * D), v1 = *reinterpret_cast<const float4*>(row + 2 * D + 4);
    const float qq[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}, kk[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    // (in_mul and scale are powers of two: only the multiplication by qscale rounds, as in split.hip)
#pragma unroll
    for (int e = 0; e < 8; ++e) { q[e] = (qq[e] * in_mul) * qscale * scale; k[e] = kk[e] * in_mul * scale; v[e] = vv[e] * in_mul * scale; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = k[e] = v[e] = 0.f;
  }
  unsigned sat = 0;
  const size_t orow = ((size_t)bh * tok_pad + t) * 128 + d8;
  u32x4 hi, lo;
  split8(q, hi, lo, sat);
  *reinterpret_cast<u32x4*>(Qc + orow) = hi;
  *reinterpret_cast<u32x4*>(Qc + orow + 64) = lo;
  split8(k, hi, lo, sat);
  *reinterpret_cast<u32x4*>(Kc + orow) = hi;
  *reinterpret_cast<u32x4*>(Kc + orow + 64) = lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) vs[tl][d8 + e] = v[e];
  __syncthreads();
  const int d = tid >> 2, tq = (tid & 3) * 8;
  float vt[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) vt[e] = vs[tq + e][d];
  split8(vt, hi, lo, sat);
  const size_t plane = (size_t)gridDim.y * 64 * tok_pad;
  const size_t vo = ((size_t)bh * 64 + d) * tok_pad + tb * 32 + tq;
  *reinterpret_cast<u32x4*>(Vt + vo) = hi;
  *reinterpret_cast<u32x4*>(Vt + plane + vo) = lo;
  report(sat, ovf);
}

// ---- attention on fp16-term operands (eager_attention_forward, modeling_dinov2.py:153-179: softmax(Q K^T hd^-0.5) V).  Structure, LDS layout, key-row
// permutation and software pipeline: attn_split_kernel<2, 1> of split.hip, which documents them; what differs is the MFMA (v_mfma_f32_32x32x16_f16), the scales
// (file header) and the probability split.
template <int V>
struct IntTag { static constexpr int value = V; };

struct Lds {
  static constexpr int KROW = 2 * 64 + 8;                        // fp16 elements per staged K row (hi | lo + 16 bytes of padding)
  static constexpr int VROW = 32 + 8;                            // fp16 elements per staged V^T row (32 keys)
  static constexpr int K_ELEMS = 32 * KROW, V_ELEMS = 2 * 64 * VROW;
  static constexpr int STAGE = K_ELEMS + V_ELEMS;
  static constexpr int K_PIECES = 32 * 2 * 8, V_PIECES = 2 * 64 * 4;       // 16-byte pieces per block
  static constexpr int KPT = K_PIECES / 256, VPT = V_PIECES / 256;
};

// term pairs of the three products: (A term, B term) = (hi, hi), (hi, lo), (lo, hi)
#define S16_A(p) ((p) == 2 ? 1 : 0)
#define S16_B(p) ((p) == 1 ? 1 : 0)

__global__ __launch_bounds__(256, 2) void attn_split16_kernel(const h_raw* __restrict__ Qc, const h_raw* __restrict__ Kc, const h_raw* __restrict__ Vt, h_raw* __restrict__ out, int tok,
                                                              int tok_pad, int heads, int D, float inv_qk, float out_mul, unsigned* __restrict__ ovf) {
  using L = Lds;
  constexpr int P = 3, TERMS = 2, NCH = 4;                       // 32-element chunks of a 128-element row: chunk 2 t + c = half c of term t
  static_assert(L::K_PIECES % 256 == 0 && L::V_PIECES % 256 == 0, "whole pieces per thread");
  extern __shared__ __attribute__((aligned(16))) h_raw lds16[];   // two stages of [K block | V^T block]
  h_raw* lds = lds16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = (blockIdx.x * 4 + wave) * 32;
  const bool active = q0 < tok_pad;                              // (a wave past the padded queries still copies its share of every block and meets the barriers)
  const int bh = blockIdx.y;
  const int b = bh / heads, hd = bh - b * heads;
  const int n = lane & 31, h = lane >> 5;
  const size_t rowlen = 128;
  const size_t plane = (size_t)gridDim.y * 64 * tok_pad;
  const h_raw* ksrc[L::KPT];
  int kdst[L::KPT];
#pragma unroll
  for (int i = 0; i < L::KPT; ++i) {
    const int piece = tid + 256 * i, row = piece / 16, c = piece - row * 16;
    ksrc[i] = Kc + ((size_t)bh * tok_pad + row) * rowlen + c * 8;
    kdst[i] = row * L::KROW + c * 8;
  }
  const h_raw* vsrc[L::VPT];
  int vdst[L::VPT];
#pragma unroll
  for (int i = 0; i < L::VPT; ++i) {
    const int piece = tid + 256 * i, row = piece >> 2, c = piece & 3;        // row = term * 64 + d
    const int t = row >> 6, d = row & 63;
    vsrc[i] = Vt + t * plane + ((size_t)bh * 64 + d) * tok_pad + c * 8;
    vdst[i] = L::K_ELEMS + row * L::VROW + c * 8;
  }
  u32x4 kreg[L::KPT], vreg[L::VPT];
  const int nkb = tok_pad >> 5;
  auto fetch = [&](int kk, int vk) {                             // K block kk (if it exists) and V^T block vk (if >= 0) into registers
    if (kk < nkb) {
#pragma unroll
      for (int i = 0; i < L::KPT; ++i) kreg[i] = *reinterpret_cast<const u32x4*>(ksrc[i] + (size_t)kk * 32 * rowlen);
    }
    if (vk >= 0) {
#pragma unroll
      for (int i = 0; i < L::VPT; ++i) vreg[i] = *reinterpret_cast<const u32x4*>(vsrc[i] + (size_t)vk * 32);
    }
  };
  auto stash = [&](int stage, bool with_v) {
    h_raw* base = lds + stage * L::STAGE;
#pragma unroll
    for (int i = 0; i < L::KPT; ++i) *reinterpret_cast<u32x4*>(base + kdst[i]) = kreg[i];
    if (with_v) {
#pragma unroll
      for (int i = 0; i < L::VPT; ++i) *reinterpret_cast<u32x4*>(base + vdst[i]) = vreg[i];
    }
  };
  f16x8 qreg[NCH][2];
  {
    int qr = q0 + n;
    qr = qr < tok_pad ? qr : tok_pad - 1;                        // (a tile that starts past the padded rows re-reads the last padded row: never stored)
    const h_raw* qrow = Qc + ((size_t)bh * tok_pad + qr) * rowlen + h * 16;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      qreg[j][0] = *reinterpret_cast<const f16x8*>(qrow + j * 32);
      qreg[j][1] = *reinterpret_cast<const f16x8*>(qrow + j * 32 + 8);
    }
  }
  const int pin = (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1);   // pi(n)
  const int koff = pin * L::KROW + h * 16;                       // this lane's K row in a stage
  const int voff = L::K_ELEMS + n * L::VROW + 8 * h;             // this lane's V^T row (term 0, channel n) in a stage
  f32x16 o0 = (f32x16){0}, o1 = (f32x16){0};
  float m_run = -INFINITY, l_run = 0.f;                          // (m in the true score's units, log2)
  auto scores = [&](const h_raw* stage_base, f32x16& s) {
    s = (f32x16){0};
    const h_raw* krow = stage_base + koff;
    f16x8 ka[NCH][2];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      ka[j][0] = *reinterpret_cast<const f16x8*>(krow + j * 32);
      ka[j][1] = *reinterpret_cast<const f16x8*>(krow + j * 32 + 8);
    }
#pragma unroll
    for (int pr = 0; pr < P; ++pr) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka[2 * S16_A(pr) + c][0], qreg[2 * S16_B(pr) + c][0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka[2 * S16_A(pr) + c][1], qreg[2 * S16_B(pr) + c][1], s, 0, 0, 0);
      }
    }
  };
  auto pv = [&](const h_raw* stage_base, const f16x8 (&pp)[TERMS][2]) {   // o += V^T(block in the stage) P^T(pp)
    const h_raw* vrow = stage_base + voff;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8 va[TERMS][2];
#pragma unroll
      for (int tt = 0; tt < TERMS; ++tt) {
        va[tt][0] = *reinterpret_cast<const f16x8*>(vrow + (tt * 64) * L::VROW + 16 * st);
        va[tt][1] = *reinterpret_cast<const f16x8*>(vrow + (tt * 64 + 32) * L::VROW + 16 * st);
      }
#pragma unroll
      for (int pr = 0; pr < P; ++pr) {
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va[S16_A(pr)][0], pp[S16_B(pr)][st], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va[S16_A(pr)][1], pp[S16_B(pr)][st], o1, 0, 0, 0);
      }
    }
  };
  f32x16 sA, sB;
  f16x8 pA[TERMS][2], pB[TERMS][2];
#pragma unroll
  for (int tt = 0; tt < TERMS; ++tt) pA[tt][0] = pA[tt][1] = pB[tt][0] = pB[tt][1] = __builtin_bit_cast(f16x8, (u32x4){0u, 0u, 0u, 0u});
  fetch(0, -1);
  stash(1, false);                                               // K(0) alone, in the K area of stage 1
  fetch(1, -1);
  stash(0, false);                                               // stage 0 = [K(1) | zeros: there is no block -1]
  for (int i = tid; i < L::V_ELEMS / 8; i += 256) *reinterpret_cast<u32x4*>(lds + L::K_ELEMS + i * 8) = (u32x4){0u, 0u, 0u, 0u};
  __syncthreads();
  if (active) scores(lds + L::STAGE, sA);
  __syncthreads();                                               // every wave has read K(0) before iteration 0 overwrites stage 1
  // one block: scores of block kb + 1 into sn, P V of block kb - 1 with pp, softmax of block kb (scores in sc) into pn
  auto step = [&](int kb, f32x16& sc, f32x16& sn, const f16x8 (&pp)[TERMS][2], f16x8 (&pn)[TERMS][2], auto masked) {
    const h_raw* st_base = lds + (kb & 1) * L::STAGE;
    fetch(kb + 2, kb);                                           // for the next iteration's stage [K(kb + 2) | V^T(kb)]; in flight under this block's MFMAs
    if (active) {
      scores(st_base, sn);                                       // K(kb + 1) (in the last iteration: a stale block, result unused)
      pv(st_base, pp);                                           // V^T(kb - 1) with the previous block's probabilities
      // register i of lane (n, h) = key kb * 32 + 16 (i / 8) + 8 h + (i % 8)
      if constexpr (decltype(masked)::value) {
        const int lim = tok - kb * 32;                           // keys of this block that exist
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[i] = (16 * (i >> 3) + 8 * h + (i & 7) < lim) ? sc[i] : -INFINITY;
      }
      float mx = sc[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sc[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx * inv_qk);             // (inv_qk > 0: the maximum of the scaled scores is the scaled maximum)
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float p[16], rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        p[i] = __builtin_amdgcn_exp2f(fmaf(sc[i], inv_qk, -m_new));
        rs += p[i];
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // probabilities times 2^14 -> hi / lo operands per PV step (consumed by the NEXT step's pv)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        u32x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const u32x2 t = split_pair_inrange(p[8 * st + 2 * e] * 16384.f, p[8 * st + 2 * e + 1] * 16384.f);
          hi[e] = t[0];
          lo[e] = t[1];
        }
        pn[0][st] = __builtin_bit_cast(f16x8, hi);
        pn[1][st] = __builtin_bit_cast(f16x8, lo);
      }
      // hints: one MFMA, then a handful of vector instructions, over the iteration's 24 MFMAs (LLVM's IGroupLP; groups it cannot fill are skipped)
#pragma unroll
      for (int g = 0; g < 8 * P; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      }
      // everything above was independent of this iteration's MFMAs; the rescale is not
#pragma unroll
      for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
    }
    stash((kb + 1) & 1, true);                                   // the other stage = [K(kb + 2) | V^T(kb)]: every wave left it at the previous barrier
    __syncthreads();
  };
  using No = IntTag<0>;
  using Yes = IntTag<1>;
  int kb = 0;
  for (; kb + 2 <= nkb - 1; kb += 2) {
    step(kb, sA, sB, pA, pB, No{});
    step(kb + 1, sB, sA, pB, pA, No{});
  }
  if (kb < nkb - 1) {                                            // one more unmasked block, then the last one
    step(kb, sA, sB, pA, pB, No{});
    step(kb + 1, sB, sA, pB, pA, Yes{});
    if (active) pv(lds + (nkb & 1) * L::STAGE, pA);              // the last block's P V (its V^T was staged by the last step)
  } else {
    step(kb, sA, sB, pA, pB, Yes{});
    if (active) pv(lds + (nkb & 1) * L::STAGE, pB);
  }
  if (!active) return;
  const int q = q0 + n;
  if (q >= tok) return;
  const float inv = out_mul / l_run;                             // out_mul = out_scale / (2^14 s_v): a power of two
  // O^T register i of lane (n, h): channel 32 dt + 8 (i / 4) + 4 h + i % 4 of query q -> the A-side split operand of the out-projection, row b tok + q
  h_raw* orow = out + ((size_t)b * tok + q) * (size_t)3 * D + hd * 64;
  unsigned sat = 0;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 hi, lo;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float x0 = (dt ? o1[4 * g + 2 * e] : o0[4 * g + 2 * e]) * inv, x1 = (dt ? o1[4 * g + 2 * e + 1] : o0[4 * g + 2 * e + 1]) * inv;
        const u32x2 t = split_pair(x0, x1, sat);
        hi[e] = t[0];
        lo[e] = t[1];
      }
      const int d = 32 * dt + 8 * g + 4 * h;
      *reinterpret_cast<u32x2*>(orow + d) = hi;
      *reinterpret_cast<u32x2*>(orow + (size_t)D + d) = hi;
      *reinterpret_cast<u32x2*>(orow + 2 * (size_t)D + d) = lo;
    }
  }
  report(sat, ovf);
}

// one wave: C = A B^T with A[0][0] = a, B[0][0] = b (fp16 bit patterns), everything else zero; lane 0 stores C[0][0]
__global__ __launch_bounds__(64) void mfma_probe_kernel(float* __restrict__ out, unsigned a_bits, unsigned b_bits, int slot) {
  const int lane = threadIdx.x;
  u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (lane == 0) { a[0] = a_bits & 0xFFFFu; b[0] = b_bits & 0xFFFFu; }        // row / column 0, k = 0
  f32x16 c = (f32x16){0};
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  if (lane == 0) out[slot] = c[0];
}

}  // namespace s16
}  // namespace ucod
#endif  // UCOD_HALF_F16

using namespace ucod;

#ifdef UCOD_HALF_F16
#define S16_F16_ONLY() do { } while (0)
#else
#define S16_F16_ONLY() return UCOD_EINVAL
#endif

extern "C" float ucod_split16_class_scale(int cls) { return (cls >= 0 && cls < UCOD_SPLIT16_NUM_CLASSES) ? s16::kScale[cls] : 0.f; }

extern "C" int ucod_split16_rows(const float* in, long ld_in, void* out, int M, int K, int role, int op, float alpha, float scale, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!in || !out || M <= 0 || K <= 0 || (K & 7) != 0 || ld_in < K || (ld_in & 3) != 0 || (role != 0 && role != 1) || op < 0 || op > 3 || !s16::pow2_ok(scale)) return UCOD_EINVAL;
  if (op == 3 && ld_in < 2L * K) return UCOD_EINVAL;             // (op 3 reads rows 2 K wide)
  UCOD_PROF(PROF_SPLIT, stream);
  hipLaunchKernelGGL(s16::split16_rows_kernel, dim3(s16::blocks_for((long)M * (K >> 3))), dim3(256), 0, (hipStream_t)stream, in, ld_in, (h_raw*)out, M, K, role, op, alpha, scale,
                     resid16_overflow_counter());
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" int ucod_split16_gemm_act(int op, const void* a_f16, const void* b_f16, void* out_f16, int M, int N, int K3, const float* bias_scaled, float alpha, float scale,
                                     int variant, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!a_f16 || !b_f16 || !out_f16 || !bias_scaled || M <= 0 || N <= 0 || (N & 7) != 0 || K3 <= 0 || (op != 1 && op != 3) || !s16::pow2_ok(alpha) || !s16::pow2_ok(scale))
    return UCOD_EINVAL;
  return gemm_split16_act(op == 1 ? UCOD_EPI_BIAS_GELU_SPLIT16 : UCOD_EPI_BIAS_SWIGLU_SPLIT16, a_f16, b_f16, out_f16, M, N, K3, bias_scaled, alpha, scale, variant, stream);
#endif
}

extern "C" int ucod_split16_layernorm(const float* x, const float* gamma, const float* beta, void* out, int rows, int D, float eps, int role, float scale, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!x || !gamma || !beta || !out || rows <= 0 || !s16::ln_width_ok(D) || (role != 0 && role != 1) || !s16::pow2_ok(scale)) return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_SPLIT, stream);
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  unsigned* ovf = resid16_overflow_counter();
#define LNS_CASE(n) \
  case n: hipLaunchKernelGGL((s16::layernorm_split16_kernel<n>), grid, block, 0, s, x, gamma, beta, (h_raw*)out, rows, D, eps, role, scale, ovf); break;
  switch (D / 128) {
    LNS_CASE(1) LNS_CASE(2) LNS_CASE(3) LNS_CASE(4) LNS_CASE(5) LNS_CASE(6) LNS_CASE(8) LNS_CASE(10) LNS_CASE(12)
    default: return UCOD_EINVAL;
  }
#undef LNS_CASE
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" int ucod_split16_patch_im2col(const float* img, void* patches, int B, int C, int H, int W, int P, int Kpad, float scale, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!img || !patches || B <= 0 || C <= 0 || P <= 0 || H <= 0 || W <= 0 || H % P || W % P || Kpad < C * P * P || (Kpad % 64) != 0 || !s16::pow2_ok(scale)) return UCOD_EINVAL;
  const int gh = H / P, gw = W / P;
  UCOD_PROF(PROF_IM2COL, stream);
  hipLaunchKernelGGL(s16::im2col_split16_kernel, dim3(s16::blocks_for((long)B * gh * gw * (Kpad / 2))), dim3(256), 0, (hipStream_t)stream, img, (h_raw*)patches, B, C, H, W, P, Kpad,
                     gh, gw, scale, resid16_overflow_counter());
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" int ucod_split16_scale_f32(float* x, size_t n, float alpha, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!x || n == 0 || !s16::pow2_ok(alpha)) return UCOD_EINVAL;
  UCOD_PROF(PROF_SPLIT, stream);
  hipLaunchKernelGGL(s16::scale_f32_kernel, dim3(s16::blocks_for((long)n)), dim3(256), 0, (hipStream_t)stream, x, n, alpha);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" size_t ucod_split16_attention_operand_bytes(int B, int tok, int heads) {
  if (B <= 0 || tok <= 0 || heads <= 0) return 0;
  const size_t tok_pad = (size_t)(tok + 31) / 32 * 32, bh = (size_t)B * heads;
  return 3 * bh * tok_pad * 2 * 64 * 2;                          // Qc | Kc | Vt, two fp16 terms each
}

extern "C" int ucod_split16_qkv(const float* qkv, void* operands, int B, int tok, int heads, float in_mul, float qscale, float scale, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!qkv || !operands || B <= 0 || tok <= 0 || heads <= 0 || !s16::pow2_ok(in_mul) || !s16::pow2_ok(scale) || !(qscale > 0.f)) return UCOD_EINVAL;
  const int tok_pad = (tok + 31) / 32 * 32, bh = B * heads;
  if (bh > 65535) return UCOD_EINVAL;
  const size_t qk = (size_t)bh * tok_pad * 128;
  h_raw* Qc = (h_raw*)operands;
  h_raw* Kc = Qc + qk;
  h_raw* Vt = Kc + qk;
  UCOD_PROF(PROF_SPLIT, stream);
  hipLaunchKernelGGL(s16::qkv_split16_kernel, dim3(tok_pad / 32, bh), dim3(256), 0, (hipStream_t)stream, qkv, Qc, Kc, Vt, tok, tok_pad, heads, heads * 64, in_mul, qscale, scale,
                     resid16_overflow_counter());
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" int ucod_split16_attention_fwd(const void* operands, void* out_split, int B, int tok, int heads, float scale, float out_scale, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!operands || !out_split || B <= 0 || tok <= 0 || heads <= 0 || !s16::pow2_ok(scale) || !s16::pow2_ok(out_scale)) return UCOD_EINVAL;
  const int tok_pad = (tok + 31) / 32 * 32, bh = B * heads;
  if (bh > 65535) return UCOD_EINVAL;
  const size_t qk = (size_t)bh * tok_pad * 128;
  const h_raw* Qc = (const h_raw*)operands;
  const h_raw* Kc = Qc + qk;
  const h_raw* Vt = Kc + qk;
  UCOD_PROF(PROF_ATTN_SPLIT, stream);
  constexpr size_t lds = 2 * s16::Lds::STAGE * sizeof(h_raw);
  static_assert(lds <= 64 * 1024, "two stages fit the default dynamic LDS limit");
  hipLaunchKernelGGL(s16::attn_split16_kernel, dim3(cdiv(tok_pad, 128), bh), dim3(256), lds, (hipStream_t)stream, Qc, Kc, Vt, (h_raw*)out_split, tok, tok_pad, heads, heads * 64,
                     1.0f / (scale * scale), out_scale / (16384.f * scale), resid16_overflow_counter());
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

extern "C" int ucod_split16_mfma_subnormal_probe(float* out2_dev, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!out2_dev) return UCOD_EINVAL;
  // slot 0: 2^-24 (smallest subnormal, bits 0x0001) times 2^14 (0x7400) = 2^-10 if the input is kept; slot 1: 2^-14 (smallest normal, 0x0400) times 2^14 = 1 (control)
  hipLaunchKernelGGL(s16::mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out2_dev, 0x0001u, 0x7400u, 0);
  hipLaunchKernelGGL(s16::mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out2_dev, 0x0400u, 0x7400u, 1);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#endif
}

// ------------------------------------------------------------------------------------------------ the pass
namespace {
struct Plan16 {
  size_t off_x, off_h, off_qkv, off_att, off_a, off_f1, off_g, off_patch, total;
  int M, tok;
};
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
Plan16 plan16(const ucod_vit_desc* d, int mlp, int flags) {
  Plan16 p;
  const int gh = d->H / d->P, gw = d->W / d->P;
  p.tok = gh * gw + 1 + d->n_reg;                                  // [CLS | n_reg register tokens | patches]
  p.M = d->B * p.tok;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o = up256(o + bytes); return r; };
  p.off_x = take((size_t)p.M * d->D * 4);
  p.off_h = take((size_t)p.M * 3 * d->D * 2);
  p.off_qkv = take((size_t)p.M * 3 * d->D * 4);
  p.off_att = take(ucod_split16_attention_operand_bytes(d->B, p.tok, d->heads));
  p.off_a = take((size_t)p.M * 3 * d->D * 2);
  // fc1's f32 output (2 F wide for SwiGLU); not with UCOD_SPLIT16_FUSE_MLP, where fc1 writes the split hidden itself
  p.off_f1 = (flags & UCOD_SPLIT16_FUSE_MLP) ? o : take((size_t)p.M * d->F * (mlp == UCOD_MLP_SWIGLU ? 2 : 1) * 4);
  p.off_g = take((size_t)p.M * 3 * d->F * 2);
  p.off_patch = take((size_t)d->B * gh * gw * 3 * d->Kpad * 2);
  p.total = o;
  return p;
}
// (the LayerNorm widths are asked of the LayerNorm launcher's own predicate: a geometry this accepts is one every kernel of the pass takes)
bool valid16(const ucod_vit_desc* d, int mlp, int flags) {
  return d && (flags & ~UCOD_SPLIT16_FUSE_MLP) == 0 && (mlp == UCOD_MLP_GELU || mlp == UCOD_MLP_SWIGLU) && d->B > 0 && d->C > 0 && d->P > 0 && d->H > 0 && d->W > 0 && d->H % d->P == 0 && d->W % d->P == 0 && d->heads > 0 &&
         d->D == d->heads * 64 && s16::ln_width_ok(d->D) && d->F > 0 && d->F % 128 == 0 && d->L >= 1 && d->Kpad % 64 == 0 && d->Kpad >= d->C * d->P * d->P &&
         d->full_last_layer == 0 && (long)d->B * d->heads <= 65535 && d->n_reg >= 0 && d->n_reg <= 1023;
}
}  // namespace

#define RUN(call)                \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != 0) return rc__;  \
  } while (0)

extern "C" size_t ucod_vit_split16_workspace_bytes_ex(const ucod_vit_desc* d, int mlp, int flags) { return valid16(d, mlp, flags) ? plan16(d, mlp, flags).total : 0; }
extern "C" size_t ucod_vit_split16_stream_offset_ex(const ucod_vit_desc* d, int mlp, int flags) { return valid16(d, mlp, flags) ? plan16(d, mlp, flags).off_x : (size_t)-1; }
extern "C" size_t ucod_vit_split16_workspace_bytes(const ucod_vit_desc* d, int mlp) { return ucod_vit_split16_workspace_bytes_ex(d, mlp, 0); }
extern "C" size_t ucod_vit_split16_stream_offset(const ucod_vit_desc* d, int mlp) { return ucod_vit_split16_stream_offset_ex(d, mlp, 0); }

extern "C" int ucod_vit_forward_split16(const ucod_vit_desc* d, int mlp, const void* const* T, const float* wscale, int n_wscale, const float* img, float* key_out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return ucod_vit_forward_split16_ex(d, mlp, 0, T, wscale, n_wscale, img, key_out, workspace, workspace_bytes, stream);
}

extern "C" int ucod_vit_forward_split16_ex(const ucod_vit_desc* d, int mlp, int flags, const void* const* T, const float* wscale, int n_wscale, const float* img, float* key_out,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  S16_F16_ONLY();
#ifdef UCOD_HALF_F16
  if (!valid16(d, mlp, flags) || !T || !wscale || n_wscale != 1 + 4 * d->L || !img || !key_out || !workspace) return UCOD_EINVAL;
  for (int i = 0; i < n_wscale; ++i)
    if (!s16::pow2_ok(wscale[i])) return UCOD_EINVAL;
  const Plan16 p = plan16(d, mlp, flags);
  const bool swiglu = mlp == UCOD_MLP_SWIGLU, fuse_mlp = (flags & UCOD_SPLIT16_FUSE_MLP) != 0;
  if (workspace_bytes < p.total) return UCOD_ENOMEM;
  char* ws = (char*)workspace;
  float* x = (float*)(ws + p.off_x);
  void* h = ws + p.off_h;
  float* qkv = (float*)(ws + p.off_qkv);
  void* att = ws + p.off_att;
  void* a = ws + p.off_a;
  float* f1 = (float*)(ws + p.off_f1);
  void* g = ws + p.off_g;
  void* patches = ws + p.off_patch;
  const int M = p.M, tok = p.tok, D = d->D, F = d->F, gv = d->gemm_variant, R = d->n_reg, np = tok - 1 - R;
  const float sLN = s16::kScale[UCOD_SPLIT16_LN], sQKV = s16::kScale[UCOD_SPLIT16_QKV], sATT = s16::kScale[UCOD_SPLIT16_ATT], sHID = s16::kScale[UCOD_SPLIT16_HIDDEN],
              sPATCH = s16::kScale[UCOD_SPLIT16_PATCH];
  // (the register rows of slot +2 carry S_patch like the CLS row: one in-place pass removes it from every token row)
  // the table's biases / position rows / CLS row / LayerScale vectors carry the operand scales of their GEMM (file header); the driver removes what is left
  RUN(ucod_split16_patch_im2col(img, patches, d->B, d->C, d->H, d->W, d->P, d->Kpad, sPATCH, stream));
  RUN(ucod_gemm_bf16_reg(UCOD_EPI_PATCH_TOKENS_F32, patches, T[0], x, d->B * np, D, 3 * d->Kpad, (const float*)T[1], nullptr, nullptr, (const float*)T[3], tok, R, gv, stream));
  RUN(ucod_cls_rows_reg(x, (const float*)T[2], (const float*)T[3], d->B, tok, D, R, stream));
  RUN(ucod_split16_scale_f32(x, (size_t)M * D, 1.0f / (sPATCH * wscale[0]), stream));
  for (int l = 0; l < d->L; ++l) {
    const void* const* W = T + 4 + UCOD_VIT_LAYER_STRIDE * l;
    const float* ws_l = wscale + 1 + 4 * l;                       // qkv, proj, fc1, fc2
    const bool last = (l == d->L - 1);
    RUN(ucod_split16_layernorm(x, (const float*)W[0], (const float*)W[1], h, M, D, d->eps, last ? 1 : 0, sLN, stream));
    if (last) {
      // key hook (feature_extractor.py:42,46-47,55-58): rows = channels (A = the K rows of the split QKV weight, A side), columns = tokens (B side)
      if (!W[14]) return UCOD_EINVAL;
      RUN(ucod_gemm_bf16_reg(UCOD_EPI_KEY_NCHW_F32, W[14], h, key_out, D, M, 3 * D, (const float*)W[3] + D, nullptr, nullptr, nullptr, tok, R, gv, stream));
      RUN(ucod_split16_scale_f32(key_out, (size_t)d->B * D * np, 1.0f / (sLN * ws_l[0]), stream));
      break;
    }
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_F32, h, W[2], qkv, M, 3 * D, 3 * D, (const float*)W[3], nullptr, nullptr, nullptr, tok, gv, stream));
    // DINOv3: the rotation runs on the f32 projection, which still carries the power-of-two operand scales (they pass through a linear map exactly)
    if (d->rope) RUN(ucod_rope_qk(qkv, UCOD_ROPE_ELEM_F32, d->rope, d->B, tok, R, d->heads, stream));
    RUN(ucod_split16_qkv(qkv, att, d->B, tok, d->heads, 1.0f / (sLN * ws_l[0]), 0.125f * 1.4426950408889634f, sQKV, stream));
    RUN(ucod_split16_attention_fwd(att, a, d->B, tok, d->heads, sQKV, sATT, stream));
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_SCALE_RESID_F32, a, W[4], x, M, D, 3 * D, (const float*)W[5], (const float*)W[6], x, nullptr, tok, gv, stream));
    RUN(ucod_split16_layernorm(x, (const float*)W[7], (const float*)W[8], h, M, D, d->eps, 0, sLN, stream));
    if (fuse_mlp) {
      // fc1, activation and split in one launch: the drain runs what the row pass below runs, on the same f32 value
      RUN(ucod_split16_gemm_act(swiglu ? 3 : 1, h, W[9], g, M, swiglu ? 2 * F : F, 3 * D, (const float*)W[10], 1.0f / (sLN * ws_l[2]), sHID, gv, stream));
    } else {
      // fc1 through the f32 epilogue, then activation + split in one row pass (exact-erf GELU / f32 SiLU on the unscaled value)
      RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_F32, h, W[9], f1, M, swiglu ? 2 * F : F, 3 * D, (const float*)W[10], nullptr, nullptr, nullptr, tok, gv, stream));
      RUN(ucod_split16_rows(f1, swiglu ? 2L * F : F, g, M, F, 0, swiglu ? 3 : 1, 1.0f / (sLN * ws_l[2]), sHID, stream));
    }
    RUN(ucod_gemm_bf16(UCOD_EPI_BIAS_SCALE_RESID_F32, g, W[11], x, M, D, 3 * F, (const float*)W[12], (const float*)W[13], x, nullptr, tok, gv, stream));
  }
  return UCOD_OK;
#endif
}
