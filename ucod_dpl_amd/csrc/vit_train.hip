// Backbone-backward mode (models/modules/full_model.py:47-72,79-126: LoRA r=2, alpha=4 on the query /
// key / value projections of every layer, everything else frozen).  Row-wise kernels of the training pass; the GEMMs and
// the attention kernels live in gemm_bf16.hip / attention.hip / attention_bwd.hip, the pass itself in vit_train_driver.hip.
//
// LoRA rides on the big GEMMs as 64 extra K columns ("aug" columns), so no GEMM kernel knows about it:
//   forward   h_aug  [M, D+64]  = [ LN1(x) | u = LN1(x) A^T (3r values: q,k,v) | 0 ]        (ucod_layernorm_lora)
//             Wqkv_aug [3D, D+64] = [ Wqkv | alpha/r * B on the block diagonal | 0 ]         (ucod_lora_pack)
//             qkv = h_aug Wqkv_aug^T  ==  LN1(x) Wqkv^T + alpha/r * (LN1(x) A^T) B^T
//   backward  dqkv_aug [M, 3D+64] = [ dqkv | t = alpha/r * dqkv B (3r values) | 0 ]          (ucod_lora_grad)
//             WqkvT_aug [D, 3D+64] = [ Wqkv^T | A^T | 0 ]                                     (ucod_lora_pack)
//             dLN1 = dqkv_aug WqkvT_aug^T  ==  dqkv Wqkv + t A
//             dA = t^T LN1(x),  dB = alpha/r * dqkv^T u                                        (ucod_lora_grad)
// Parameter layout of one layer in the flat LoRA arena (f32): [A_q (r x D) | B_q (D x r) | A_k | B_k | A_v | B_v].
// With LoRA dropout on, u is computed from the dropped LN1(x) (one mask per projection), dA from the same dropped input, and the
// t A term of dLN1 is added -- masked -- by the LayerNorm-1 backward instead of the dgrad GEMM (A^T columns packed as zeros).
#include <type_traits>
#include "common.h"
#include "../../include/ucod_dpl.h"
#include "colsum.h"               // the workgroup shape, slab rule and second launch of the deterministic column sums (ucod_colsum_det_lora)
#include "gemm_bf16_epilogue.h"   // gelu_erf2 / gelu_grad2: the fc1 drains' fit, which ucod_lora_out_grad_x recomputes the hidden with

namespace ucod {

constexpr int AUG = UCOD_LORA_AUG;

// LoRA dropout (LoraConfig.lora_dropout of models/modules/full_model.py:50,63: nn.Dropout on the input of every lora_A, one
// independent mask per target module).  Counter-based: the keep decision of element (row, col) of projection p in layer l is a
// pure function of (seed, 3*l + p, row*D + col), so forward and backward regenerate the same mask and nothing is stored.
// ABI 3 (round 4): ONE 32-bit mix per element serves the three projections -- bits 0-9 decide query, 10-19 key, 20-29 value, each against
// floor(p * 1024) -- instead of one mix per projection: 3 instead of 9 quarter-rate integer multiplies per element in ln_lora / ln_bwd
// (the hash was half of ln_lora's time).  The drop probability is therefore p_eff = floor(1024 p) / 1024 and the kept
// elements are scaled by 1 / (1 - p_eff), so the mask stays unbiased.
struct Drop {
  unsigned seed_lo, seed_hi, thresh;     // drop iff the projection's 10-bit field < thresh  (thresh = floor(p * 1024))
  int key0;                              // layer
  float inv_keep;                        // 1 / (1 - thresh / 1024); 0 thresh = dropout off
};
__host__ __device__ __forceinline__ unsigned drop_hash(unsigned seed_lo, unsigned seed_hi, unsigned key, unsigned idx) {
  unsigned h = seed_lo ^ (idx * 0x9E3779B1u);
  h ^= seed_hi + key * 0x85EBCA77u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ float drop_scale(const Drop& d, int p, unsigned idx) {
  // (the compiler shares the mix between the three projections of one element: a pure function of (d, idx))
  return ((drop_hash(d.seed_lo, d.seed_hi, (unsigned)d.key0, idx) >> (10 * p)) & 1023u) < d.thresh ? 0.f : d.inv_keep;
}
static Drop make_drop(const ucod_lora_dropout* dd) {
  Drop d{0u, 0u, 0u, 0, 1.f};
  if (dd && dd->p > 0.f) {
    d.seed_lo = (unsigned)(dd->seed & 0xFFFFFFFFull);
    d.seed_hi = (unsigned)(dd->seed >> 32);
    const double t = (double)dd->p * 1024.0;
    d.thresh = t >= 1023.0 ? 1023u : (unsigned)t;
    d.key0 = dd->layer;
    d.inv_keep = 1.0f / (1.0f - (float)d.thresh / 1024.0f);
  }
  return d;
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm forward + LoRA down-projection.  One wave per row, D = 128*NCH, row in registers (as layernorm_kernel).
// ---------------------------------------------------------------------------------------------------------------------
// XH16: the residual stream is IEEE fp16 (the no-grad pass of the EMA teacher, ucod_vit_forward_lora_infer with resid16) instead of f32
// NP: modules sharing the row -- 3 (query, key, value: `lora` is the layer's [A_q | B_q | A_k | B_k | A_v | B_v]), 1 (the MLP input projection: `lora` is A_m) or
// 2 (gate_proj and up_proj of the gated MLP: `lora` is [A_g | A_u]).  A_p sits at lora + p * astride: 2 r D between q / k / v, r D between the adjacent pair
template <int NCH, bool XH16 = false, int NP = 3>
__global__ __launch_bounds__(256) void ln_lora_kernel(const void* __restrict__ x_, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ lora,
                                                      int r, bf16_raw* __restrict__ y, int rows, int D, float eps, Drop drop, int astride) {
  // the 3r LoRA A rows live in LDS for the whole block (they were re-read from L2 for every row: 92 us against 33 us for the plain
  // LayerNorm); each wave walks rows block-stride, two rows in flight (as layernorm_kernel)
  extern __shared__ float a_lds[];                               // [NP r][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < NP * r * D; i += 256) {
    const int p = i / (r * D), rem = i - p * r * D;               // A_p at lora + p*astride
    a_lds[i] = lora[(size_t)p * astride + rem];
  }
  __syncthreads();
  constexpr int R = 2;
  const float2* g2 = reinterpret_cast<const float2*>(gamma);
  const float2* b2 = reinterpret_cast<const float2*>(beta);
  for (int row0 = (blockIdx.x * 4 + wave) * R; row0 < rows; row0 += gridDim.x * 4 * R) {
    float2 v[R][NCH];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = (row0 + q) < rows ? (row0 + q) : rows - 1;
      if constexpr (XH16) {
        const unsigned* xr = reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned short*>(x_) + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < NCH; ++i) unpack_f16x2(xr[lane + 64 * i], v[q][i].x, v[q][i].y);
      } else {
        const float2* xr = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(x_) + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < NCH; ++i) v[q][i] = xr[lane + 64 * i];
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = row0 + q;
      if (row >= rows) break;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) s += v[q][i].x + v[q][i].y;
      const float mean = wave_sum(s) / (float)D;
      float qq = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const float a = v[q][i].x - mean, b = v[q][i].y - mean;
        qq += a * a + b * b;
      }
      const float rstd = rsqrtf(wave_sum(qq) / (float)D + eps);
      bf16_raw* yr = y + (size_t)row * (D + AUG);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const float2 g = g2[lane + 64 * i], b = b2[lane + 64 * i];
        v[q][i].x = (v[q][i].x - mean) * rstd * g.x + b.x;
        v[q][i].y = (v[q][i].y - mean) * rstd * g.y + b.y;
        reinterpret_cast<unsigned*>(yr)[lane + 64 * i] = pack_bf16x2(v[q][i].x, v[q][i].y);
      }
      // u[j] = <dropout_p(LN(x)), A[j]>, j = p*r + rank
      float mine = 0.f;
      for (int p = 0; p < NP; ++p) {
        float2 vm[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          vm[i] = v[q][i];
          if (drop.thresh) {
            const unsigned idx = (unsigned)row * (unsigned)D + 2u * (unsigned)(lane + 64 * i);
            vm[i].x *= drop_scale(drop, p, idx);
            vm[i].y *= drop_scale(drop, p, idx + 1u);
          }
        }
        for (int jr = 0; jr < r; ++jr) {
          const int j = p * r + jr;
          const float2* a2 = reinterpret_cast<const float2*>(a_lds + (size_t)j * D);
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < NCH; ++i) {
            const float2 a = a2[lane + 64 * i];
            d += vm[i].x * a.x + vm[i].y * a.y;
          }
          d = wave_sum(d);
          if (lane == j) mine = d;
        }
      }
      yr[D + lane] = f32_to_bf16(lane < NP * r ? mine : 0.f);
    }
  }
}

// The same for D % 256 == 0 (ViT-B 768, ViT-L 1024) with a lane owning FOUR consecutive columns per chunk (round 4): 16-byte (f32) / 8-byte (fp16)
// loads, 8-byte stores instead of 4-byte ones, and the dropout mix of an element computed ONCE for its three masks (in the form above the compiler
// shared it between only some of the projections: 177 v_mul_lo_u32 per two rows instead of 72).
template <int NV, bool XH16, int NP = 3>
__global__ __launch_bounds__(256) void ln_lora4_kernel(const void* __restrict__ x_, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ lora,
                                                       int r, bf16_raw* __restrict__ y, int rows, int D, float eps, Drop drop, int astride) {
  extern __shared__ float a_lds[];                               // [NP r][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < NP * r * D; i += 256) {
    const int p = i / (r * D), rem = i - p * r * D;
    a_lds[i] = lora[(size_t)p * astride + rem];
  }
  __syncthreads();
  constexpr int R = 2;
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4* g4 = reinterpret_cast<const f4*>(gamma);
  const f4* b4 = reinterpret_cast<const f4*>(beta);
  f4 gm[NV], bt[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { gm[i] = g4[lane + 64 * i]; bt[i] = b4[lane + 64 * i]; }
  for (int row0 = (blockIdx.x * 4 + wave) * R; row0 < rows; row0 += gridDim.x * 4 * R) {
    f4 v[R][NV];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = (row0 + q) < rows ? (row0 + q) : rows - 1;
      if constexpr (XH16) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4* xr = reinterpret_cast<const h4*>(reinterpret_cast<const _Float16*>(x_) + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const h4 h = xr[lane + 64 * i];
          v[q][i] = (f4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        }
      } else {
        const f4* xr = reinterpret_cast<const f4*>(reinterpret_cast<const float*>(x_) + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < NV; ++i) v[q][i] = xr[lane + 64 * i];
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = row0 + q;
      if (row >= rows) break;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) s += (v[q][i][0] + v[q][i][1]) + (v[q][i][2] + v[q][i][3]);
      const float mean = wave_sum(s) / (float)D;
      float qq = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = v[q][i][e] - mean;
          qq += a * a;
        }
      const float rstd = rsqrtf(wave_sum(qq) / (float)D + eps);
      bf16_raw* yr = y + (size_t)row * (D + AUG);
      unsigned hsh[NV][4];                                        // the element's one mix: bits 0-9 query, 10-19 key, 20-29 value
#pragma unroll
      for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][i][e] = (v[q][i][e] - mean) * rstd * gm[i][e] + bt[i][e];
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        reinterpret_cast<u2*>(yr)[lane + 64 * i] = (u2){pack_bf16x2(v[q][i][0], v[q][i][1]), pack_bf16x2(v[q][i][2], v[q][i][3])};
        if (drop.thresh) {
          const unsigned idx = (unsigned)row * (unsigned)D + 4u * (unsigned)(lane + 64 * i);
#pragma unroll
          for (int e = 0; e < 4; ++e) hsh[i][e] = drop_hash(drop.seed_lo, drop.seed_hi, (unsigned)drop.key0, idx + (unsigned)e);
        }
      }
      float mine = 0.f;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        f4 vm[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          vm[i] = v[q][i];
          if (drop.thresh) {
#pragma unroll
            for (int e = 0; e < 4; ++e) vm[i][e] *= ((hsh[i][e] >> (10 * p)) & 1023u) < drop.thresh ? 0.f : drop.inv_keep;
          }
        }
        for (int jr = 0; jr < r; ++jr) {
          const int j = p * r + jr;
          const f4* a4 = reinterpret_cast<const f4*>(a_lds + (size_t)j * D);
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const f4 a = a4[lane + 64 * i];
            d += (vm[i][0] * a[0] + vm[i][1] * a[1]) + (vm[i][2] * a[2] + vm[i][3] * a[3]);
          }
          d = wave_sum(d);
          if (lane == j) mine = d;
        }
      }
      yr[D + lane] = f32_to_bf16(lane < NP * r ? mine : 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm backward w.r.t. its input (gamma / beta are frozen), fused with the residual add and with the column scale +
// bf16 cast the NEXT dgrad GEMM wants as its A operand:
//   g = dy * gamma;  dx_ln = rstd * (g - mean(g) - xhat * mean(g * xhat));   dx = dres + dx_ln;   s = bf16(scale * dx)
// ---------------------------------------------------------------------------------------------------------------------
// LORA: dy additionally receives the dropout-masked LoRA branch  sum_p mask_p/keep * (t_p A_p)  (t = aug columns of dqkv_aug); with
// dropout off that term rides on the dgrad GEMM instead (A^T columns of WqkvT_aug) and this kernel is launched with LORA = false.
// One wave per row; a lane owns NCH chunks of VW consecutive floats (VW = 4: 16-byte accesses, rows of a multiple of 256 floats; VW = 2 for
// the other widths).  Everything the row needs from memory -- x, dy, the residual cotangent -- is requested before the first reduction, so
// that one latency covers all three streams (round 3: 103 -> see profiles/r03_ln_bwd.txt).
// DYB: dy arrives as bf16 (the dgrad GEMMs of the backward driver write their output in the 16-bit type: half the bytes on both sides).
// XH: x (the saved LayerNorm input = the residual stream) is IEEE fp16 (training pass with vit.resid16).
// LORA: 0, or the number of modules whose branch is added -- 3 (q / k / v: t at tq[p r + j], A_p at lora + p astride, astride = 2 r D), 1 (the MLP input
// projection: lora = A_m) or 2 (gate_proj / up_proj of the gated MLP: lora = [A_g | A_u], astride = r D; masks 0 and 1)
template <int NCH, int VW, int LORA, bool DYB, bool XH>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy_, const void* __restrict__ x_,
                                                     const float* __restrict__ gamma, const float* __restrict__ dres,
                                                     const float* __restrict__ scale, float* __restrict__ dx,
                                                     bf16_raw* __restrict__ sout, int rows, int D, float eps,
                                                     const bf16_raw* __restrict__ tq, int ldt, const float* __restrict__ lora, int r, Drop drop,
                                                     int astride) {
  typedef float vecf __attribute__((ext_vector_type(VW)));
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const vecf* xr = reinterpret_cast<const vecf*>(reinterpret_cast<const float*>(x_) + (size_t)row * D);
  typedef unsigned short vech __attribute__((ext_vector_type(VW)));
  const vecf* dyr = reinterpret_cast<const vecf*>(reinterpret_cast<const float*>(dy_) + (size_t)row * D);
  const vech* dyh = reinterpret_cast<const vech*>(reinterpret_cast<const bf16_raw*>(dy_) + (size_t)row * D);
  const vecf* rr = dres ? reinterpret_cast<const vecf*>(dres + (size_t)row * D) : nullptr;
  const vecf* g2 = reinterpret_cast<const vecf*>(gamma);
  vecf v[NCH], g[NCH], res[NCH];
  if constexpr (XH) {
    typedef _Float16 vecx __attribute__((ext_vector_type(VW)));
    const vecx* xh = reinterpret_cast<const vecx*>(reinterpret_cast<const _Float16*>(x_) + (size_t)row * D);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const vecx h = xh[lane + 64 * i];
#pragma unroll
      for (int e = 0; e < VW; ++e) v[i][e] = (float)h[e];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NCH; ++i) v[i] = xr[lane + 64 * i];
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if constexpr (DYB) {
      const vech h = dyh[lane + 64 * i];
#pragma unroll
      for (int e = 0; e < VW; ++e) g[i][e] = bf16_to_f32(h[e]);
    } else {
      g[i] = dyr[lane + 64 * i];
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) res[i] = rr ? rr[lane + 64 * i] : (vecf)(0.f);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    vecf d = g[i];
    if constexpr (LORA > 0) {
      const unsigned idx = (unsigned)row * (unsigned)D + (unsigned)VW * (unsigned)(lane + 64 * i);
      auto branch = [&](auto rc) {                                // rank known at compile time: the 3 r coefficient / A-row loads go out together
        constexpr int R = decltype(rc)::value;
        vecf av[LORA][R];
        float t[LORA][R];
#pragma unroll
        for (int p = 0; p < LORA; ++p)
#pragma unroll
          for (int jr = 0; jr < R; ++jr) {
            t[p][jr] = bf16_to_f32(tq[(size_t)row * ldt + p * R + jr]);
            av[p][jr] = reinterpret_cast<const vecf*>(lora + (size_t)p * astride + (size_t)jr * D)[lane + 64 * i];
          }
#pragma unroll
        for (int p = 0; p < LORA; ++p) {
          vecf acc = (vecf)(0.f);
#pragma unroll
          for (int jr = 0; jr < R; ++jr) acc += t[p][jr] * av[p][jr];
#pragma unroll
          for (int e = 0; e < VW; ++e) d[e] += acc[e] * drop_scale(drop, p, idx + (unsigned)e);
        }
      };
      if (r == 2) branch(std::integral_constant<int, 2>{});
      else if (r == 4) branch(std::integral_constant<int, 4>{});
      else if (r == 1) branch(std::integral_constant<int, 1>{});
      else {
        for (int p = 0; p < LORA; ++p) {
          vecf acc = (vecf)(0.f);
          for (int jr = 0; jr < r; ++jr) {
            const float t = bf16_to_f32(tq[(size_t)row * ldt + p * r + jr]);
            const vecf av = reinterpret_cast<const vecf*>(lora + (size_t)p * astride + (size_t)jr * D)[lane + 64 * i];
            acc += t * av;
          }
#pragma unroll
          for (int e = 0; e < VW; ++e) d[e] += acc[e] * drop_scale(drop, p, idx + (unsigned)e);
        }
      }
    }
    g[i] = d * g2[lane + 64 * i];
#pragma unroll
    for (int e = 0; e < VW; ++e) s += v[i][e];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    v[i] -= mean;
#pragma unroll
    for (int e = 0; e < VW; ++e) q += v[i][e] * v[i][e];
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    v[i] *= rstd;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      sg += g[i][e];
      sgx += g[i][e] * v[i][e];
    }
  }
  const float mg = wave_sum(sg) / (float)D, mgx = wave_sum(sgx) / (float)D;
  const vecf* sc2 = scale ? reinterpret_cast<const vecf*>(scale) : nullptr;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    vecf o;
#pragma unroll
    for (int e = 0; e < VW; ++e) o[e] = rstd * (g[i][e] - mg - v[i][e] * mgx) + res[i][e];
    if (dx) reinterpret_cast<vecf*>(dx + (size_t)row * D)[lane + 64 * i] = o;
    if (sout) {
      const vecf c = sc2 ? sc2[lane + 64 * i] : (vecf)(1.f);
      typedef unsigned vecu __attribute__((ext_vector_type(VW / 2)));
      vecu w;
#pragma unroll
      for (int e = 0; e < VW / 2; ++e) w[e] = pack_bf16x2(o[2 * e] * c[2 * e], o[2 * e + 1] * c[2 * e + 1]);
      reinterpret_cast<vecu*>(sout + (size_t)row * D)[lane + 64 * i] = w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Cotangent of the key hook, [B, D, h*w] f32 (CLS dropped, NCHW) -> token-major rows of dqkv_aug: the k third gets the
// transposed values (CLS row 0, and the nreg register-token rows behind it, which the key hook drops too), the q and v thirds are zero (the last
// layer's q / v never reach the loss).  Block = (image, 32 tokens); 32x32 LDS transposes over the channel axis.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_grad_tokens_kernel(const float* __restrict__ dkey, bf16_raw* __restrict__ dqkv, int tok,
                                                              int D, int nreg) {
  __shared__ float tile[32][33];
  const int b = blockIdx.y, t0 = blockIdx.x * 32;
  const int hw = tok - 1 - nreg, ld = 3 * D + AUG;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
  bf16_raw* base = dqkv + (size_t)b * tok * ld;
  // zero q, v (and aug) of these rows
  for (int rr = 0; rr < 32; ++rr) {
    const int t = t0 + rr;
    if (t >= tok) break;
    bf16_raw* rowp = base + (size_t)t * ld;
    for (int c = threadIdx.x; c < D; c += 256) { rowp[c] = 0; rowp[2 * D + c] = 0; }
    if (threadIdx.x < AUG) rowp[3 * D + threadIdx.x] = 0;
  }
  for (int c0 = 0; c0 < D; c0 += 32) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + ty + 8 * k, t = t0 + tx;                 // read: tokens contiguous
      float v = 0.f;
      if (t > nreg && t < tok) v = dkey[((size_t)b * D + c) * hw + (t - 1 - nreg)];
      tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = t0 + ty + 8 * k, c = c0 + tx;                 // write: channels contiguous
      if (t < tok) base[(size_t)t * ld + D + c] = f32_to_bf16(tile[tx][ty + 8 * k]);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA pack: aug columns of Wqkv_aug [3D, D+64] and WqkvT_aug [D, 3D+64] from one layer's LoRA parameters.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lora_pack_kernel(const float* __restrict__ lora, int r, float scaling, bf16_raw* __restrict__ w_aug,
                                                        bf16_raw* __restrict__ wt_aug, int D, int zero_at) {
  const int idx = blockIdx.x * 256 + threadIdx.x;                // one thread per (row, aug column) of either matrix
  const int n_fwd = 3 * D * AUG;
  if (idx < n_fwd) {
    if (!w_aug) return;
    const int n = idx / AUG, j = idx - n * AUG;                  // row n of Wqkv (which of q/k/v: p), aug column j
    const int p = n / D, nn = n - p * D;
    float v = 0.f;
    if (j >= p * r && j < (p + 1) * r) v = scaling * lora[(size_t)p * 2 * r * D + (size_t)r * D + (size_t)nn * r + (j - p * r)];   // B_p[nn][j']
    w_aug[(size_t)n * (D + AUG) + D + j] = f32_to_bf16(v);
    return;
  }
  const int k = idx - n_fwd;
  if (k >= D * AUG || !wt_aug) return;
  const int d = k / AUG, j = k - d * AUG;
  float v = 0.f;
  if (j < 3 * r && !zero_at) {                                   // zero_at: dropout on -- the (masked) A term is added by ln_bwd instead
    const int p = j / r, jj = j - p * r;
    v = lora[(size_t)p * 2 * r * D + (size_t)jj * D + d];        // A_p[jj][d]
  }
  wt_aug[(size_t)d * (3 * D + AUG) + 3 * D + j] = f32_to_bf16(v);
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA gradients of one layer, ranks [j0, j0+RW) of each of q, k, v in one pass over dqkv and LN1(x):
//   t[m][p][j]  = scaling * sum_n dqkv[m][pD+n] * B_p[n][j]          -> aug columns of dqkv_aug (bf16)
//   dA_p[j][d] += t[m][p][j] * h[m][d]
//   dB_p[n][j] += scaling * dqkv[m][pD+n] * u[m][p][j]                (u = aug columns of h_aug)
// Block = 6 waves = 2 row streams x 3 projections: wave (p, s) walks rows s, s+2*gridDim, ... and touches only the p-th
// third of dqkv, so its state is 2*RW*NCH*2 accumulators + the lane's B values (~110 VGPRs: 4 waves per SIMD, where the
// first version -- one wave for all three thirds, 332 VGPRs, one wave per SIMD -- sat on the load latency of every row).
// The next row's loads are issued before the current row's arithmetic.  Lane owns columns {2*lane, 2*lane+1} + 128*i of
// its D-wide slice.  Per-block partials, summed in a fixed order by lora_grad_reduce_kernel (deterministic).
// ---------------------------------------------------------------------------------------------------------------------
// VW = columns per lane and chunk: 2 (4-byte loads) or, for D % 256 == 0, 4 (8-byte loads: half the load instructions per row -- round 4)
// NS = row streams per block (block = 3 NS waves): the per-block combine and the partials the reduce kernel walks are paid once per NS streams
template <int NCH, int RW, int VW, int NS>
__global__ __launch_bounds__(192 * NS) void lora_grad_kernel(bf16_raw* __restrict__ dqkv, const bf16_raw* __restrict__ h,
                                                        const float* __restrict__ lora, int r, int j0, float scaling,
                                                        float* __restrict__ partial, int rows, int D, Drop drop) {
  extern __shared__ float lds[];                                  // block reduction buffer [3][RW][D] | [3][D][RW]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = wave % 3, strm = wave / 3;
  const int ldq = 3 * D + AUG, ldh = D + AUG;
  // this lane's B_p[n][j0 + j] (n = its 2*NCH columns)
  float bw[NCH][VW][RW];
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < VW; ++e)
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        const int n = VW * (lane + 64 * i) + e;
        bw[i][e][j] = (j0 + j < r) ? lora[(size_t)p * 2 * r * D + (size_t)r * D + (size_t)n * r + j0 + j] : 0.f;
      }
  float accA[RW][NCH][VW], accB[NCH][VW][RW];
#pragma unroll
  for (int j = 0; j < RW; ++j)
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < VW; ++e) accA[j][i][e] = accB[i][e][j] = 0.f;
  const int step = gridDim.x * NS;
  int row = blockIdx.x * NS + strm;
  typedef unsigned uvw __attribute__((ext_vector_type(VW / 2)));
  // PF rows of this wave in flight beside the one being reduced.  Measured (round 4, ViT-B, 32 images): PF = 1 -> 153-158 us per launch, PF = 4 -> 161-169
  // (185 VGPRs: two waves per SIMD), 4-byte or 8-byte loads alike: the kernel is bound neither by load latency nor by load width.
  constexpr int PF = 1;
  uvw dw[PF][NCH], hw_[PF][NCH];
  unsigned uw[PF];
  auto issue = [&](int k, int rw) {
    const uvw* dq = reinterpret_cast<const uvw*>(dqkv + (size_t)rw * ldq + (size_t)p * D);
    const uvw* hr = reinterpret_cast<const uvw*>(h + (size_t)rw * ldh);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      dw[k][i] = dq[lane + 64 * i];
      hw_[k][i] = hr[lane + 64 * i];
    }
    // u[p][j0 .. j0+RW): bf16 pair read as one dword when aligned, else two halves (wave-uniform address: broadcast)
    const bf16_raw* up = h + (size_t)rw * ldh + D + p * r + j0;
    const unsigned lo = up[0], hi = (RW > 1 && j0 + 1 < r) ? up[1] : 0u;
    uw[k] = lo | (hi << 16);
  };
#pragma unroll
  for (int k = 0; k < PF; ++k)
    if (row + k * step < rows) issue(k, row + k * step);
  while (row < rows) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      if (row >= rows) break;
      float dv[NCH][VW], hv[NCH][VW], u[RW], t[RW];
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int w = 0; w < VW / 2; ++w) {
          dv[i][2 * w] = __uint_as_float(dw[k][i][w] << 16);
          dv[i][2 * w + 1] = __uint_as_float(dw[k][i][w] & 0xFFFF0000u);
          hv[i][2 * w] = __uint_as_float(hw_[k][i][w] << 16);
          hv[i][2 * w + 1] = __uint_as_float(hw_[k][i][w] & 0xFFFF0000u);
        }
      u[0] = __uint_as_float(uw[k] << 16);
      if (RW > 1) u[1] = __uint_as_float(uw[k] & 0xFFFF0000u);
      const int cur = row;
      if (drop.thresh) {                                             // dA sees the SAME dropped input the forward's lora_A saw
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const unsigned idx = (unsigned)cur * (unsigned)D + (unsigned)VW * (unsigned)(lane + 64 * i);
#pragma unroll
          for (int e = 0; e < VW; ++e) hv[i][e] *= drop_scale(drop, p, idx + (unsigned)e);
        }
      }
      if (row + PF * step < rows) issue(k, row + PF * step);         // this slot's next row, PF rows ahead
      row += step;
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            s += dv[i][e] * bw[i][e][j];
            accB[i][e][j] += dv[i][e] * u[j];
          }
        t[j] = bf16_to_f32(f32_to_bf16(scaling * wave_sum(s)));      // the dgrad GEMM sees the bf16 value: use it for dA too
        if (lane == 0 && j0 + j < r) dqkv[(size_t)cur * ldq + 3 * D + p * r + j0 + j] = f32_to_bf16(t[j]);
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int e = 0; e < VW; ++e) accA[j][i][e] += t[j] * hv[i][e];
      }
    }
  }
  // block combine: [3][RW][D] (dA window) then [3][D][RW] (dB window); stream 0 writes, stream 1 adds
  const int nA = 3 * RW * D, nB = 3 * D * RW;
  float* out = partial + (size_t)blockIdx.x * (nA + nB);
  for (int s2 = 0; s2 < NS; ++s2) {
    if (strm == s2) {
#pragma unroll
      for (int j = 0; j < RW; ++j)
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            const int d = VW * (lane + 64 * i) + e;
            const int ia = (p * RW + j) * D + d, ib = nA + (p * D + d) * RW + j;
            if (s2 == 0) {
              lds[ia] = accA[j][i][e];
              lds[ib] = scaling * accB[i][e][j];
            } else {
              lds[ia] += accA[j][i][e];
              lds[ib] += scaling * accB[i][e][j];
            }
          }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nA + nB; i += 192 * NS) out[i] = lds[i];
}

// The front of every reduce kernel here, called by all 256 threads of the workgroup: partial [nblk][n] summed over the block list in a fixed order.  A workgroup
// takes 32 elements x 8 slices of the block list (a single thread walking all 512 partials was latency-bound): slice sl adds blocks sl, sl + 8, ... in ascending
// order, then the slices are added in ascending order through LDS.  True for the one thread that holds the total `s` of element `i` (slice 0, i < n).
__device__ __forceinline__ bool sum_partials(const float* __restrict__ partial, int nblk, int n, int& i, float& s) {
  __shared__ float red[8][33];
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  i = blockIdx.x * 32 + e;
  s = 0.f;
  if (i < n) {
#pragma unroll 4
    for (int b = sl; b < nblk; b += 8) s += partial[(size_t)b * n + i];
  }
  red[sl][e] = s;
  __syncthreads();
  if (sl != 0 || i >= n) return false;
  s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += red[k][e];
  return true;
}

// grad layout = parameter layout of the layer: [A_q | B_q | A_k | B_k | A_v | B_v]; accumulate = add to existing content
template <int RW>
__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ partial, int nblk, int r, int j0, float* __restrict__ grad,
                                                               int D, int accumulate) {
  const int nA = 3 * RW * D, nB = 3 * D * RW;
  int i;
  float s;
  if (!sum_partials(partial, nblk, nA + nB, i, s)) return;
  int p, j, d;
  size_t dst;
  if (i < nA) {
    p = i / (RW * D);
    j = (i - p * RW * D) / D;
    d = i - p * RW * D - j * D;
    if (j0 + j >= r) return;
    dst = (size_t)p * 2 * r * D + (size_t)(j0 + j) * D + d;
  } else {
    const int k = i - nA;
    p = k / (D * RW);
    d = (k - p * D * RW) / RW;
    j = k - p * D * RW - d * RW;
    if (j0 + j >= r) return;
    dst = (size_t)p * 2 * r * D + (size_t)r * D + (size_t)d * r + j0 + j;
  }
  grad[dst] = accumulate ? grad[dst] + s : s;
}

constexpr int LORA_GRAD_BLOCKS = 512;                            // (1024 measured: 153 -> 183 us per launch: more partials to combine, no more rows in flight per SIMD)

}  // namespace ucod

using namespace ucod;

// LDS one workgroup may have on the current device, queried once (gfx950: 160 KiB, of which a launch gets more than 64 KiB only after asking for it with
// hipFuncAttributeMaxDynamicSharedMemorySize); SIZE_MAX when no device answers, so that descriptor checks made without one refuse nothing on its account
static size_t lds_per_block() {
  static const size_t v = [] {
    hipDeviceProp_t pr;
    int dv = 0;
    if (hipGetDevice(&dv) != hipSuccess || hipGetDeviceProperties(&pr, dv) != hipSuccess) {
      (void)hipGetLastError();
      return (size_t)SIZE_MAX;
    }
    size_t m = pr.sharedMemPerBlock;
    if (pr.sharedMemPerBlockOptin > m) m = pr.sharedMemPerBlockOptin;
    if (pr.maxSharedMemoryPerMultiProcessor > m) m = pr.maxSharedMemoryPerMultiProcessor;   // (a CU's whole LDS can go to one workgroup)
    return m;
  }();
  return v;
}
static inline size_t ln_lora_lds_bytes(int D, int r, int np) { return (size_t)np * (size_t)r * (size_t)D * sizeof(float); }

extern "C" int ucod_layernorm_lora_fits(int D, int r, int modules) {
  if (D <= 0 || r < 1 || (modules != 1 && modules != 3) || modules * r > AUG) return 0;
  return ln_lora_lds_bytes(D, r, modules) <= lds_per_block() ? 1 : 0;
}

// a staging buffer past 64 KiB has to be asked for (per device: at every such launch, as ucod_lora_grad does)
template <typename K>
static inline hipError_t ask_lds(K kern, size_t lds) {
  return lds > 65536 ? hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

// np: 3 = the q / k / v modules of one layer (lora = the layer's arena row), 1 = the MLP input projection (lora = A_m), 2 = the gated MLP's pair (lora = [A_g | A_u])
static int launch_ln_lora(const void* x, bool x_h16, const float* gamma, const float* beta, const float* lora, int r, void* y_aug, int rows, int D, float eps,
                          const ucod_lora_dropout* dropout, void* stream, int np = 3) {
  if (!x || !gamma || !beta || !lora || !y_aug || rows <= 0 || D <= 0 || (D % 128) != 0 || r < 1 || np * r > AUG) return UCOD_EINVAL;
  if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
  if (ln_lora_lds_bytes(D, r, np) > lds_per_block()) return UCOD_EINVAL;      // the np r A rows do not fit one workgroup's LDS: refused before any launch
  UCOD_PROF(np == 3 ? PROF_LN : PROF_LN_LORA_MLP, stream);
  const Drop drop = make_drop(dropout);
  static const int lnl_env = [] { const char* e = ucod::lab_env("UCOD_LN_LORA_NBLK"); return e ? atoi(e) : 0; }();          // measurement knob
  const int lnl_max = lnl_env > 0 ? lnl_env : 2048;
  const int nblk = cdiv(rows, 8) < lnl_max ? cdiv(rows, 8) : lnl_max;   // block-stride over rows: the A rows are staged once per block
  dim3 grid(nblk), block(256);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = ln_lora_lds_bytes(D, r, np);
  const int astride = (np == 3 ? 2 : 1) * r * D;                  // from A_p to A_{p+1}: B_p lies between q / k / v, the pair's two are adjacent
  static const bool narrow = ucod::lab_env("UCOD_LN_LORA_NARROW") != nullptr;     // measurement knob: the 8-byte / 4-byte form
#define LNL(kern)                                                                                                       \
  do {                                                                                                                  \
    const hipError_t e = ask_lds(kern, lds);                                                                            \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(kern, grid, block, lds, s, x, gamma, beta, lora, r, (bf16_raw*)y_aug, rows, D, eps, drop, astride); \
  } while (0)
  if ((D % 256) == 0 && D <= 1536 && !narrow) {
    switch (D / 256) {
#define C4(n)                                                                                                                                        \
  case n:                                                                                                                                            \
    if (np == 1 && x_h16) LNL((ln_lora4_kernel<n, true, 1>)); \
    else if (np == 1) LNL((ln_lora4_kernel<n, false, 1>));    \
    else if (np == 2 && x_h16) LNL((ln_lora4_kernel<n, true, 2>)); \
    else if (np == 2) LNL((ln_lora4_kernel<n, false, 2>));    \
    else if (x_h16) LNL((ln_lora4_kernel<n, true>)); \
    else LNL((ln_lora4_kernel<n, false>));          \
    break;
      C4(1) C4(2) C4(3) C4(4) C4(5) C4(6)
#undef C4
    }
    UCOD_CHECK_LAUNCH();
    return UCOD_OK;
  }
  switch (D / 128) {
#define C(n)                                                                                                                                         \
  case n:                                                                                                                                            \
    if (np == 1 && x_h16) LNL((ln_lora_kernel<n, true, 1>)); \
    else if (np == 1) LNL((ln_lora_kernel<n, false, 1>));    \
    else if (np == 2 && x_h16) LNL((ln_lora_kernel<n, true, 2>)); \
    else if (np == 2) LNL((ln_lora_kernel<n, false, 2>));    \
    else if (x_h16) LNL((ln_lora_kernel<n, true>));      \
    else LNL((ln_lora_kernel<n, false>));           \
    break;
    C(1) C(2) C(3) C(4) C(5) C(6) C(8) C(10) C(12)
#undef C
    default: return UCOD_EINVAL;
  }
#undef LNL
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_layernorm_lora(const float* x, const float* gamma, const float* beta, const float* lora, int r, void* y_aug, int rows,
                                   int D, float eps, const ucod_lora_dropout* dropout, void* stream) {
  UCOD_BF16_ONLY();
  return launch_ln_lora(x, false, gamma, beta, lora, r, y_aug, rows, D, eps, dropout, stream);
}

extern "C" int ucod_layernorm_lora_h16(const void* x_f16, const float* gamma, const float* beta, const float* lora, int r, void* y_aug, int rows,
                                       int D, float eps, const ucod_lora_dropout* dropout, void* stream) {
  UCOD_BF16_ONLY();
  return launch_ln_lora(x_f16, true, gamma, beta, lora, r, y_aug, rows, D, eps, dropout, stream);
}

static int launch_ln_bwd(const void* dy, bool dy_bf16, const void* x, bool x_f16, const float* gamma, const float* dres, const float* next_scale, float* dx, void* s_bf16,
                         int rows, int D, float eps, const bf16_raw* tq, int ldt, const float* lora, int r, const Drop& drop, hipStream_t s, int np = 3) {
  dim3 grid(cdiv(rows, 4)), block(256);
  const bool lo = tq != nullptr;
  const int astride = (np == 3 ? 2 : 1) * r * D;             // from A_p to A_{p+1} (launch_ln_lora)
  if (x_f16 && !dy_bf16) return UCOD_EINVAL;                // (the fp16 stream comes with bf16 dgrad outputs: the driver's only use)
#define L(n, vw, lora_, dyb_, xh_) hipLaunchKernelGGL((ln_bwd_kernel<n, vw, lora_, dyb_, xh_>), grid, block, 0, s, dy, x, gamma, dres, next_scale, dx, (bf16_raw*)s_bf16, rows, D, eps, tq, ldt, lora, r, drop, astride)
#define C(n, vw)                                                                                                                               \
  case n:                                                                                                                                      \
    if (lo && np == 1 && x_f16) L(n, vw, 1, true, true);                                                                                       \
    else if (lo && np == 1 && dy_bf16) L(n, vw, 1, true, false);                                                                               \
    else if (lo && np == 1) L(n, vw, 1, false, false);                                                                                         \
    else if (lo && np == 2 && x_f16) L(n, vw, 2, true, true);                                                                                  \
    else if (lo && np == 2 && dy_bf16) L(n, vw, 2, true, false);                                                                               \
    else if (lo && np == 2) L(n, vw, 2, false, false);                                                                                         \
    else if (lo && x_f16) L(n, vw, 3, true, true);                                                                                             \
    else if (lo && dy_bf16) L(n, vw, 3, true, false);                                                                                          \
    else if (lo) L(n, vw, 3, false, false);                                                                                                    \
    else if (x_f16) L(n, vw, 0, true, true);                                                                                                   \
    else if (dy_bf16) L(n, vw, 0, true, false);                                                                                                \
    else L(n, vw, 0, false, false);                                                                                                            \
    break;
  if (D % 256 == 0) {                                      // 16-byte accesses
    switch (D / 256) {
      C(1, 4) C(2, 4) C(3, 4) C(4, 4) C(5, 4) C(6, 4)
      default: return UCOD_EINVAL;
    }
  } else {
    switch (D / 128) {
      C(1, 2) C(3, 2) C(5, 2) C(7, 2) C(9, 2) C(11, 2)
      default: return UCOD_EINVAL;
    }
  }
#undef C
#undef L
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                  void* s_bf16, int rows, int D, float eps, void* stream) {
  UCOD_BF16_ONLY();
  if (!dy || !x || !gamma || (!dx && !s_bf16) || rows <= 0 || D <= 0 || (D % 128) != 0) return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_BWD, stream);
  return launch_ln_bwd(dy, false, x, false, gamma, dres, next_scale, dx, s_bf16, rows, D, eps, nullptr, 0, nullptr, 0, make_drop(nullptr), (hipStream_t)stream);
}

extern "C" int ucod_layernorm_bwd_ex(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                     void* s_bf16, int rows, int D, float eps, void* stream) {
  UCOD_BF16_ONLY();
  if (!dy || !x || !gamma || (!dx && !s_bf16) || rows <= 0 || D <= 0 || (D % 128) != 0 || (flags & ~3)) return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_BWD, stream);
  return launch_ln_bwd(dy, (flags & UCOD_LNB_DY_BF16) != 0, x, (flags & UCOD_LNB_X_F16) != 0, gamma, dres, next_scale, dx, s_bf16, rows, D, eps, nullptr, 0, nullptr, 0,
                       make_drop(nullptr), (hipStream_t)stream);
}

extern "C" int ucod_layernorm_bwd_lora(const float* dy, const float* x, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                       void* s_bf16, int rows, int D, float eps, const void* dqkv_aug, const float* lora_layer, int r,
                                       const ucod_lora_dropout* dropout, void* stream) {
  UCOD_BF16_ONLY();
  if (!dy || !x || !gamma || (!dx && !s_bf16) || rows <= 0 || D <= 0 || (D % 128) != 0 || !dqkv_aug || !lora_layer || r < 1 || 3 * r > AUG ||
      !dropout || dropout->p < 0.f || dropout->p >= 1.f)
    return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_BWD, stream);
  return launch_ln_bwd(dy, false, x, false, gamma, dres, next_scale, dx, s_bf16, rows, D, eps, (const bf16_raw*)dqkv_aug + 3 * D, 3 * D + AUG, lora_layer, r,
                       make_drop(dropout), (hipStream_t)stream);
}

extern "C" int ucod_layernorm_bwd_lora_ex(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                          void* s_bf16, int rows, int D, float eps, const void* dqkv_aug, const float* lora_layer, int r,
                                          const ucod_lora_dropout* dropout, void* stream) {
  UCOD_BF16_ONLY();
  if (!dy || !x || !gamma || (!dx && !s_bf16) || rows <= 0 || D <= 0 || (D % 128) != 0 || !dqkv_aug || !lora_layer || r < 1 || 3 * r > AUG ||
      !dropout || dropout->p < 0.f || dropout->p >= 1.f || (flags & ~3))
    return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_BWD, stream);
  return launch_ln_bwd(dy, (flags & UCOD_LNB_DY_BF16) != 0, x, (flags & UCOD_LNB_X_F16) != 0, gamma, dres, next_scale, dx, s_bf16, rows, D, eps,
                       (const bf16_raw*)dqkv_aug + 3 * D, 3 * D + AUG, lora_layer, r, make_drop(dropout), (hipStream_t)stream);
}

extern "C" int ucod_key_grad_tokens_reg(const float* dkey, void* dqkv_aug, int B, int tok, int D, int n_reg, void* stream) {
  UCOD_BF16_ONLY();
  if (!dkey || !dqkv_aug || B <= 0 || n_reg < 0 || tok < 2 + n_reg || D <= 0 || (D % 32) != 0 || B > 65535) return UCOD_EINVAL;
  UCOD_PROF(PROF_LORA, stream);
  hipLaunchKernelGGL(key_grad_tokens_kernel, dim3(cdiv(tok, 32), B), dim3(256), 0, (hipStream_t)stream, dkey, (bf16_raw*)dqkv_aug, tok, D, n_reg);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_key_grad_tokens(const float* dkey, void* dqkv_aug, int B, int tok, int D, void* stream) {
  return ucod_key_grad_tokens_reg(dkey, dqkv_aug, B, tok, D, 0, stream);
}

extern "C" int ucod_lora_pack(const float* lora_layer, int r, float scaling, void* w_aug, void* wt_aug, int D, int zero_a_columns, void* stream) {
  UCOD_BF16_ONLY();
  if (!lora_layer || (!w_aug && !wt_aug) || r < 1 || 3 * r > AUG || D <= 0) return UCOD_EINVAL;
  UCOD_PROF(PROF_LORA, stream);
  const int n = 3 * D * AUG + D * AUG;
  hipLaunchKernelGGL(lora_pack_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, lora_layer, r, scaling, (bf16_raw*)w_aug,
                     (bf16_raw*)wt_aug, D, zero_a_columns);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" size_t ucod_lora_grad_workspace_bytes(int D) { return (size_t)LORA_GRAD_BLOCKS * (size_t)(12 * D) * sizeof(float); }

extern "C" int ucod_lora_grad(void* dqkv_aug, const void* h_aug, const float* lora_layer, int r, float scaling, float* grad_layer,
                              int accumulate, void* workspace, size_t workspace_bytes, int rows, int D, const ucod_lora_dropout* dropout,
                              void* stream) {
  UCOD_BF16_ONLY();
  if (!dqkv_aug || !h_aug || !lora_layer || !grad_layer || !workspace || r < 1 || 3 * r > AUG || rows <= 0 || D <= 0 || (D % 128) != 0)
    return UCOD_EINVAL;
  if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
  if (workspace_bytes < ucod_lora_grad_workspace_bytes(D)) return UCOD_ENOMEM;
  UCOD_PROF(PROF_LORA, stream);
  const Drop drop = make_drop(dropout);
  hipStream_t s = (hipStream_t)stream;
  constexpr int RW = 2;                                           // ranks per pass (the reference's r = 2 is one pass)
  static const int ns_env = [] { const char* e = ucod::lab_env("UCOD_LORA_GRAD_STREAMS"); return e ? atoi(e) : 0; }();   // measurement knob: 2 or 4 row streams per block
  // D > 1024 (ViT-g: 1536): two row streams per block -- a wave's state is 2 * RW * (D / 64) accumulators + as many B values, 12 chunks of them only fit the
  // registers of a 6-wave block (LGW below) -- and a block reduction buffer past 64 KiB, which the launch has to ask for
  const bool wide = D > 1024;
  const int NSr = wide ? 2 : ns_env == 2 ? 2 : ns_env == 5 ? 5 : 4;
  static const int nb_env = [] { const char* e = ucod::lab_env("UCOD_LORA_GRAD_NBLK"); return e ? atoi(e) : 0; }();       // measurement knob (<= LORA_GRAD_BLOCKS)
  // default: one block per CU (12 waves of 4 row streams x 3 projections), a whole round -- round 4: 512 blocks of 6 waves 158 us -> 109 us per launch at
  // ViT-B / 32 images (fewer partials to combine and to reduce; 384 blocks = 1.5 rounds: 140 us)
  static const int n_cu = [] { hipDeviceProp_t pr; int dv = 0; (void)hipGetDevice(&dv); return hipGetDeviceProperties(&pr, dv) == hipSuccess ? pr.multiProcessorCount : 256; }();
  const int nb_max = nb_env > 0 && nb_env <= LORA_GRAD_BLOCKS ? nb_env : (n_cu < LORA_GRAD_BLOCKS ? n_cu : LORA_GRAD_BLOCKS);
  const int nblk = rows < nb_max * NSr ? cdiv(rows, NSr) : nb_max;
  const size_t lds_bytes = (size_t)6 * D * RW * sizeof(float);      // B window (3*D*RW) <= block reduction buffer (6*D*RW)
  for (int j0 = 0; j0 < r; j0 += RW) {
    static const bool narrow = ucod::lab_env("UCOD_LORA_GRAD_WIDE") == nullptr;      // default: the 4-byte-load form (88 VGPRs; the 8-byte one: 148, 4 % slower)
#define LG(n, vw)                                                                                                                                   \
  do {                                                                                                                                              \
    if (NSr == 2) hipLaunchKernelGGL((lora_grad_kernel<n, RW, vw, 2>), dim3(nblk), dim3(384), lds_bytes, s, (bf16_raw*)dqkv_aug, (const bf16_raw*)h_aug, lora_layer, r, j0, scaling, (float*)workspace, rows, D, drop); \
    else if (NSr == 5) hipLaunchKernelGGL((lora_grad_kernel<n, RW, vw, 5>), dim3(nblk), dim3(960), lds_bytes, s, (bf16_raw*)dqkv_aug, (const bf16_raw*)h_aug, lora_layer, r, j0, scaling, (float*)workspace, rows, D, drop); \
    else hipLaunchKernelGGL((lora_grad_kernel<n, RW, vw, 4>), dim3(nblk), dim3(768), lds_bytes, s, (bf16_raw*)dqkv_aug, (const bf16_raw*)h_aug, lora_layer, r, j0, scaling, (float*)workspace, rows, D, drop);     \
  } while (0)
#define LGW(n)                                                                                                                                      \
  do {                                                                                                                                              \
    const void* kern = (const void*)lora_grad_kernel<n, RW, 2, 2>;                                                                                  \
    if (lds_bytes > 65536) {                                                                                                                        \
      const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);   /* (per device: asked for at every launch) */ \
      if (e != hipSuccess) return (int)e;                                                                                                           \
    }                                                                                                                                               \
    hipLaunchKernelGGL((lora_grad_kernel<n, RW, 2, 2>), dim3(nblk), dim3(384), lds_bytes, s, (bf16_raw*)dqkv_aug, (const bf16_raw*)h_aug, lora_layer, r, j0, scaling, (float*)workspace, rows, D, drop); \
  } while (0)
    if (wide) {
      switch (D / 128) {
        case 10: LGW(10); break;
        case 12: LGW(12); break;
        default: return UCOD_EINVAL;
      }
    } else if ((D % 256) == 0 && D <= 1024 && !narrow) {
      switch (D / 256) {
        case 1: LG(1, 4); break;
        case 2: LG(2, 4); break;
        case 3: LG(3, 4); break;
        case 4: LG(4, 4); break;
      }
    } else {
      switch (D / 128) {
#define C(n) case n: LG(n, 2); break;
        C(1) C(2) C(3) C(4) C(5) C(6) C(8)
#undef C
        default: return UCOD_EINVAL;
      }
    }
#undef LG
#undef LGW
    UCOD_CHECK_LAUNCH();
    hipLaunchKernelGGL((lora_grad_reduce_kernel<RW>), dim3(cdiv(6 * RW * D, 32)), dim3(256), 0, s, (const float*)workspace, nblk, r, j0,
                       grad_layer, D, accumulate);
    UCOD_CHECK_LAUNCH();
  }
  return UCOD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA on the MLP input projection (fc1; weights_in of the SwiGLU MLP; DINOv3's up_proj / gate_proj): NM modules on the one GEMM of width N1 whose input is
// LayerNorm 2's output.  NM = 1 is the single module (the _lora_mlp entry points).  NM = 2 is the gated MLP's pair (the _lora_mlp_pair entry points; DINOv3
// vits16plus: down_proj(silu(gate_proj(x)) * up_proj(x)); full_model.py:47-72 hands target_modules to peft, to which gate_proj and up_proj are TWO modules, each
// with its own A, B and dropout mask): both sit on the fused, padded, 4-interleaved weights_in, engine row 8k+e is gate row 4k+e for e < 4, row 8k+4+e is up row
// 4k+e, so together they are a rank-2r module whose B is block diagonal.  mod(n) is the module of row n: (n % 8 >= 4) at NM = 2, else 0.
//   forward   h2_aug [M, D+64] = [ LN2(x) | u_0 = drop_0(LN2 x) A_0^T (r) | .. | u_{NM-1} (r) | 0 ]                         (ln_lora*_kernel with NP = NM)
//             fc1_w_aug [N1, D+64]: row n carries alpha/r * B_m[n][:] at columns D + mod(n) r ..., zeros in every other aug column  (lora_mlp_pack_kernel)
//   backward  dpre [M, N1] comes out of the fc2 dgrad's drain without aug columns, so
//             t_p = alpha/r * dpre[:, rows of p] B_p -> scratch [M, 64] at columns p r + j,  dB rows of p = alpha/r * dpre^T u_p,  dA_p = t_p^T drop_p(LN2 x)
//             in ONE pass over dpre per two ranks (lora_mlp_grad_kernel), and d LN2 += sum_p mask_p/(1-p) (t_p A_p) in the LayerNorm-2 backward
//             (ln_bwd_kernel with LORA = NM)
// Parameter layout of one layer (f32): [A_0 (r x D) | .. | A_{NM-1} (r x D) | B_m (N1 x r)], B_m in the engine's row order -- the pair's is byte for byte the
// single module's.  An untargeted module of the pair has A = 0 and its rows of B = 0; its gradients are then zero by structure (u = 0 gives dB = 0, t = 0 gives
// dA = 0), because no sum here mixes the two modules' elements.
// ---------------------------------------------------------------------------------------------------------------------
namespace ucod {

__global__ __launch_bounds__(256) void lora_mlp_pack_kernel(const float* __restrict__ lora, int nm, int r, float scaling, bf16_raw* __restrict__ w_aug, int N1,
                                                            int D) {
  const int idx = blockIdx.x * 256 + threadIdx.x;                // one thread per (row, aug column)
  if (idx >= N1 * AUG) return;
  const int n = idx / AUG, c = idx - n * AUG;
  const int j = c - ((nm == 2 && (n & 4)) ? r : 0);              // rank within the row's own module (the pair's gate: n % 8 < 4)
  const float v = (j >= 0 && j < r) ? scaling * lora[(size_t)nm * r * D + (size_t)n * r + j] : 0.f;            // B_m[n][j]
  w_aug[(size_t)n * (D + AUG) + D + c] = f32_to_bf16(v);
}

constexpr int MLP_RB = 4;                                        // rows per iteration = waves per block (wave q writes row q's t)
constexpr int MLP_RW = 2;                                        // ranks per pass, as lora_grad_kernel (the reference's r = 2 is one pass; r = 8 reads dpre four times)
static inline int mlp_grad_max_blocks(int N1) { return N1 > 4096 ? 256 : 512; }   // one block per CU at 4 vectors per thread (256 VGPRs + AGPRs: one wave per SIMD), else two

// Ranks [j0, j0 + 2) of the NM modules in one pass over dpre and h2_aug.  The block's 256 threads share a row: thread `tid` owns the 16-byte vectors tid + 256 i
// of the dpre row (its B_m values and dB accumulators stay in registers for all the block's rows) and the column pairs tid + 256 i of h2 (dA accumulators).  MLP_RB
// rows are loaded together, their partial t summed over the block through LDS (one barrier per MLP_RB rows: two buffers in turn), rounded to bf16 as the
// LayerNorm-2 backward will read it, and used for dA.  At NM = 2 a 16-byte dpre vector holds four gate elements (0-3) and four up elements (4-7): bw / accB keep
// their shape, each element taking u of its own module; the row sum s, the bf16-rounded t and accA carry the module index, dA of module p uses mask p.  No element
// has two owners in a block, so the partials go straight to memory: [NM][2][D] | [N1][2] per block, summed in a fixed order by lora_mlp_grad_reduce_kernel.  Rows
// past the end load nothing and contribute zeros.
// RW = 1, NVT = 5 is the wide form (8192 < N1 <= UCOD_LORA_WIDE_MAX_N1): a fifth vector per thread fits the register file only with one rank per pass, so it
// reads dpre r times; its partials are [NM][D] | [N1] per block.
// Measured: 2.0 TB/s at ViT-B and at ViT-g, where <1, 4, *> takes 256 VGPRs + 125-145 AGPRs (one wave per SIMD) and nothing overlaps a group's
// loads.  h2 is the smaller operand (D+64 against N1 columns) and is read with 4-byte loads.
template <int NM, int NVT, int NPT, int RW = MLP_RW>
__global__ __launch_bounds__(256) void lora_mlp_grad_kernel(const bf16_raw* __restrict__ dpre, const bf16_raw* __restrict__ h, const float* __restrict__ lora,
                                                            int r, int j0, float scaling, float* __restrict__ partial, bf16_raw* __restrict__ tout, int rows,
                                                            int N1, int D, Drop drop) {
  constexpr int RB = MLP_RB;
  __shared__ float red[2][4][RB][NM][RW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NV = N1 / 8, NP2 = D / 2, ldh = D + AUG;
  const float* Bm = lora + (size_t)NM * r * D;
  float bw[NVT][8][RW], accB[NVT][8][RW], accA[NM][RW][NPT][2];
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    const int v = tid + 256 * i;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        bw[i][e][j] = (v < NV && j0 + j < r) ? Bm[(size_t)(8 * v + e) * r + j0 + j] : 0.f;
        accB[i][e][j] = 0.f;
      }
  }
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int i = 0; i < NPT; ++i) accA[m][j][i][0] = accA[m][j][i][1] = 0.f;
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  int buf = 0;
  for (int row0 = blockIdx.x * RB; row0 < rows; row0 += gridDim.x * RB, buf ^= 1) {
    u4 dw[RB][NVT];
    unsigned hw_[RB][NPT];
    float u[RB][NM][RW];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const bool live = row0 + q < rows;
      const int row = live ? row0 + q : rows - 1;
      const u4* dr = reinterpret_cast<const u4*>(dpre + (size_t)row * N1);
      const unsigned* hr = reinterpret_cast<const unsigned*>(h + (size_t)row * ldh);
#pragma unroll
      for (int i = 0; i < NVT; ++i) dw[q][i] = (live && tid + 256 * i < NV) ? dr[tid + 256 * i] : (u4)(0u);
#pragma unroll
      for (int i = 0; i < NPT; ++i) hw_[q][i] = (live && tid + 256 * i < NP2) ? hr[tid + 256 * i] : 0u;
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int j = 0; j < RW; ++j)                                // (block-uniform address; j0 + j < r <= 8 keeps m r + j0 + j inside the 64 aug columns)
          u[q][m][j] = (live && j0 + j < r) ? bf16_to_f32(h[(size_t)row * ldh + D + m * r + j0 + j]) : 0.f;
    }
    float t[RB][NM][RW];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      float s[NM][RW];
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int j = 0; j < RW; ++j) s[m][j] = 0.f;
#pragma unroll
      for (int i = 0; i < NVT; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int m = NM == 2 ? w / 2 : 0;                       // the pair: words 0, 1 = elements 0-3 (gate), words 2, 3 = elements 4-7 (up)
          const float d0 = __uint_as_float(dw[q][i][w] << 16), d1 = __uint_as_float(dw[q][i][w] & 0xFFFF0000u);
#pragma unroll
          for (int j = 0; j < RW; ++j) {
            s[m][j] += d0 * bw[i][2 * w][j] + d1 * bw[i][2 * w + 1][j];
            accB[i][2 * w][j] += d0 * u[q][m][j];
            accB[i][2 * w + 1][j] += d1 * u[q][m][j];
          }
        }
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int j = 0; j < RW; ++j) {
          const float ws = wave_sum(s[m][j]);
          if (lane == 0) red[buf][wave][q][m][j] = ws;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int j = 0; j < RW; ++j)     // the LayerNorm-2 backward sees the bf16 value: use it for dA too
          t[q][m][j] = bf16_to_f32(f32_to_bf16(scaling * ((red[buf][0][q][m][j] + red[buf][1][q][m][j]) + (red[buf][2][q][m][j] + red[buf][3][q][m][j]))));
    // wave q writes the 64 t columns of row q: the first pass every column (zeros beyond NM r), later passes their two per module.  Lane = m r + jj.
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (q != wave || row0 + q >= rows) continue;
      const int m = (NM == 2 && lane >= r) ? 1 : 0, c = lane - m * r - j0;      // c: this lane's rank within the pass
      const bool mine = lane < NM * r && c >= 0 && c < RW && j0 + c < r;
      const float t0 = m ? t[q][NM - 1][0] : t[q][0][0], t1 = m ? t[q][NM - 1][RW - 1] : t[q][0][RW - 1];
      const float val = mine ? (c == 0 ? t0 : t1) : 0.f;
      if (j0 == 0 || mine) tout[(size_t)(row0 + q) * AUG + lane] = f32_to_bf16(val);
    }
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        float h0 = __uint_as_float(hw_[q][i] << 16), h1 = __uint_as_float(hw_[q][i] & 0xFFFF0000u);
        float k0[NM], k1[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) k0[m] = k1[m] = 1.f;
        if (drop.thresh) {                                       // dA_p sees the SAME dropped input the forward's lora_A of module p saw (one mix, NM fields)
          const unsigned idx = (unsigned)(row0 + q) * (unsigned)D + 2u * (unsigned)(tid + 256 * i);
          // One module: its scale goes into h here and k stays 1.  (Measured with kernel-resource-usage: k kept past the branch costs five of the nine NM = 1
          // forms 4-10 registers; h scaled per module in here costs <2, 1, 1> a wave per SIMD.  Both give the same bits: t * (h * scale).)
          if constexpr (NM == 1) {
            h0 *= drop_scale(drop, 0, idx);
            h1 *= drop_scale(drop, 0, idx + 1u);
          } else {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              k0[m] = drop_scale(drop, m, idx);
              k1[m] = drop_scale(drop, m, idx + 1u);
            }
          }
        }
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
          for (int j = 0; j < RW; ++j) {
            accA[m][j][i][0] += t[q][m][j] * (h0 * k0[m]);
            accA[m][j][i][1] += t[q][m][j] * (h1 * k1[m]);
          }
      }
  }
  float* out = partial + (size_t)blockIdx.x * (size_t)(NM * RW * D + N1 * RW);
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const int c = tid + 256 * i;
        if (c < NP2) *reinterpret_cast<float2*>(out + (size_t)(m * RW + j) * D + 2 * c) = make_float2(accA[m][j][i][0], accA[m][j][i][1]);
      }
  out += NM * RW * D;
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    const int v = tid + 256 * i;
    if (v >= NV) continue;
    typedef float f4 __attribute__((ext_vector_type(4)));
    if constexpr (RW == 2) {
#pragma unroll
      for (int e = 0; e < 8; e += 2)     // rows 8v+e, 8v+e+1 of [N1][2]: four consecutive floats
        *reinterpret_cast<f4*>(out + (size_t)(8 * v + e) * RW) =
            (f4){scaling * accB[i][e][0], scaling * accB[i][e][1], scaling * accB[i][e + 1][0], scaling * accB[i][e + 1][1]};
    } else {
      static_assert(RW == 1 || RW == 2, "one or two ranks per pass");
#pragma unroll
      for (int e = 0; e < 8; e += 4)     // rows 8v+e .. 8v+e+3 of [N1][1]
        *reinterpret_cast<f4*>(out + (size_t)(8 * v + e)) =
            (f4){scaling * accB[i][e][0], scaling * accB[i][e + 1][0], scaling * accB[i][e + 2][0], scaling * accB[i][e + 3][0]};
    }
  }
}

// partial [nblk][nm * RW D + RW N1] -> grad [A (nm x r x D) | B_m (N1 x r)], ranks [j0, j0 + RW)
template <int RW>
__global__ __launch_bounds__(256) void lora_mlp_grad_reduce_kernel(const float* __restrict__ partial, int nblk, int nm, int r, int j0, float* __restrict__ grad,
                                                                   int N1, int D) {
  const int nA = nm * RW * D;
  int i;
  float s;
  if (!sum_partials(partial, nblk, nA + N1 * RW, i, s)) return;
  if (i < nA) {
    const int mj = i / D, d = i - mj * D, m = mj / RW, j = mj - m * RW;
    if (j0 + j < r) grad[(size_t)m * r * D + (size_t)(j0 + j) * D + d] = s;
  } else {
    const int k = i - nA, row = k / RW, j = k - row * RW;
    if (j0 + j < r) grad[(size_t)nm * r * D + (size_t)row * r + j0 + j] = s;
  }
}

}  // namespace ucod

// The ten entry points below are these five with modules = 1 (_lora_mlp) or 2 (_lora_mlp_pair).
static int mlp_ln_lora(const void* x, int x_f16, const float* gamma, const float* beta, const float* a, int r, void* y_aug, int rows, int D, float eps,
                       const ucod_lora_dropout* dropout, void* stream, int modules) {
  UCOD_BF16_ONLY();
  if (r < 1 || r > UCOD_LORA_MLP_MAX_R) return UCOD_EINVAL;
  return launch_ln_lora(x, x_f16 != 0, gamma, beta, a, r, y_aug, rows, D, eps, dropout, stream, modules);
}

// wide: the _wide entry points, whose N1 may reach UCOD_LORA_WIDE_MAX_N1; up to 8192 they run what the narrow ones run
static inline int mlp_max_n1(bool wide) { return wide ? UCOD_LORA_WIDE_MAX_N1 : 8192; }

static int mlp_pack(const float* lora, int r, float scaling, void* fc1_w_aug, int N1, int D, void* stream, int modules, bool wide = false) {
  UCOD_BF16_ONLY();
  if (!lora || !fc1_w_aug || r < 1 || r > UCOD_LORA_MLP_MAX_R || N1 <= 0 || N1 > mlp_max_n1(wide) || (modules == 2 && (N1 % 8) != 0) || D <= 0) return UCOD_EINVAL;
  UCOD_PROF(PROF_LORA, stream);
  hipLaunchKernelGGL(lora_mlp_pack_kernel, dim3(cdiv((long)N1 * AUG, 256)), dim3(256), 0, (hipStream_t)stream, lora, modules, r, scaling, (bf16_raw*)fc1_w_aug, N1,
                     D);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

static size_t mlp_grad_workspace_bytes(int N1, int D, int modules, bool wide = false) {
  if (N1 <= 0 || N1 > mlp_max_n1(wide) || (N1 % 128) != 0 || D <= 0 || D > 1536 || (D % 128) != 0) return 0;
  return (size_t)mlp_grad_max_blocks(N1) * (size_t)((N1 > 8192 ? 1 : MLP_RW) * (modules * D + N1)) * sizeof(float);      // (the wide form: one rank per pass)
}

static int mlp_grad(const void* dpre, const void* h2_aug, const float* lora, int r, float scaling, float* grad, void* t_bf16, void* workspace, size_t workspace_bytes,
                    int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream, int modules, bool wide = false) {
  UCOD_BF16_ONLY();
  if (!dpre || !h2_aug || !lora || !grad || !t_bf16 || !workspace || r < 1 || r > UCOD_LORA_MLP_MAX_R || rows <= 0) return UCOD_EINVAL;
  const size_t need = mlp_grad_workspace_bytes(N1, D, modules, wide);
  if (need == 0) return UCOD_EINVAL;
  if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
  if (workspace_bytes < need) return UCOD_ENOMEM;
  UCOD_PROF(PROF_LORA_MLP_GRAD, stream);
  const Drop drop = make_drop(dropout);
  hipStream_t s = (hipStream_t)stream;
  const int cap = mlp_grad_max_blocks(N1);
  const int nblk = cdiv(rows, MLP_RB) < cap ? cdiv(rows, MLP_RB) : cap;
  const int nvt = cdiv(N1 / 8, 256), npt = cdiv(D / 2, 256);       // 1..4 vectors (the wide form: 5), 1..3 column pairs per thread
  const int rw = nvt > 4 ? 1 : MLP_RW;
  for (int j0 = 0; j0 < r; j0 += rw) {
#define MGK(nm, v, p, w) hipLaunchKernelGGL((lora_mlp_grad_kernel<nm, v, p, w>), dim3(nblk), dim3(256), 0, s, (const bf16_raw*)dpre, (const bf16_raw*)h2_aug, lora, r, \
                                            j0, scaling, (float*)workspace, (bf16_raw*)t_bf16, rows, N1, D, drop)
#define MG(v, p, w)                     \
  do {                                  \
    if (modules == 2) MGK(2, v, p, w);  \
    else MGK(1, v, p, w);               \
  } while (0)
#define MGP(v, w)                   \
  do {                              \
    if (npt == 1) MG(v, 1, w);      \
    else if (npt == 2) MG(v, 2, w); \
    else MG(v, 3, w);               \
  } while (0)
    if (nvt == 1) MGP(1, MLP_RW);
    else if (nvt == 2) MGP(2, MLP_RW);
    else if (nvt <= 4) MGP(4, MLP_RW);                            // (3 vectors per thread run the 4-vector form: the fourth is never live)
    else MGP(5, 1);                                               // (UCOD_LORA_WIDE_MAX_N1 / 8 / 256 = 5)
#undef MGP
#undef MG
#undef MGK
    UCOD_CHECK_LAUNCH();
    const dim3 rgrid(cdiv((long)rw * (modules * D + N1), 32));
    if (rw == 1) hipLaunchKernelGGL(lora_mlp_grad_reduce_kernel<1>, rgrid, dim3(256), 0, s, (const float*)workspace, nblk, modules, r, j0, grad, N1, D);
    else hipLaunchKernelGGL(lora_mlp_grad_reduce_kernel<MLP_RW>, rgrid, dim3(256), 0, s, (const float*)workspace, nblk, modules, r, j0, grad, N1, D);
    UCOD_CHECK_LAUNCH();
  }
  return UCOD_OK;
}

static int mlp_ln_bwd(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx, void* s_bf16, int rows,
                      int D, float eps, const void* t_bf16, int ldt, const float* a, int r, const ucod_lora_dropout* dropout, void* stream, int modules) {
  UCOD_BF16_ONLY();
  if (!dy || !x || !gamma || (!dx && !s_bf16) || rows <= 0 || D <= 0 || (D % 128) != 0 || !t_bf16 || ldt < modules * r || !a || r < 1 || r > UCOD_LORA_MLP_MAX_R ||
      (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) || (flags & ~3))
    return UCOD_EINVAL;
  UCOD_PROF(PROF_LN_BWD_LORA_MLP, stream);
  return launch_ln_bwd(dy, (flags & UCOD_LNB_DY_BF16) != 0, x, (flags & UCOD_LNB_X_F16) != 0, gamma, dres, next_scale, dx, s_bf16, rows, D, eps,
                       (const bf16_raw*)t_bf16, ldt, a, r, make_drop(dropout), (hipStream_t)stream, modules);
}

extern "C" int ucod_layernorm_lora_mlp(const void* x, int x_f16, const float* gamma, const float* beta, const float* a_m, int r, void* y_aug, int rows, int D,
                                       float eps, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_ln_lora(x, x_f16, gamma, beta, a_m, r, y_aug, rows, D, eps, dropout, stream, 1);
}
extern "C" int ucod_layernorm_lora_mlp_pair(const void* x, int x_f16, const float* gamma, const float* beta, const float* a_pair, int r, void* y_aug, int rows,
                                            int D, float eps, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_ln_lora(x, x_f16, gamma, beta, a_pair, r, y_aug, rows, D, eps, dropout, stream, 2);
}
extern "C" int ucod_lora_mlp_pack(const float* lora_mlp, int r, float scaling, void* fc1_w_aug, int N1, int D, void* stream) {
  return mlp_pack(lora_mlp, r, scaling, fc1_w_aug, N1, D, stream, 1);
}
extern "C" int ucod_lora_mlp_pair_pack(const float* lora_pair, int r, float scaling, void* fc1_w_aug, int N1, int D, void* stream) {
  return mlp_pack(lora_pair, r, scaling, fc1_w_aug, N1, D, stream, 2);
}
extern "C" size_t ucod_lora_mlp_grad_workspace_bytes(int N1, int D) { return mlp_grad_workspace_bytes(N1, D, 1); }
extern "C" size_t ucod_lora_mlp_pair_grad_workspace_bytes(int N1, int D) { return mlp_grad_workspace_bytes(N1, D, 2); }
extern "C" int ucod_lora_mlp_grad(const void* dpre, const void* h2_aug, const float* lora_mlp, int r, float scaling, float* grad_mlp, void* t_bf16,
                                  void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_grad(dpre, h2_aug, lora_mlp, r, scaling, grad_mlp, t_bf16, workspace, workspace_bytes, rows, N1, D, dropout, stream, 1);
}
extern "C" int ucod_lora_mlp_pair_grad(const void* dpre, const void* h2_aug, const float* lora_pair, int r, float scaling, float* grad_pair, void* t_bf16,
                                       void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_grad(dpre, h2_aug, lora_pair, r, scaling, grad_pair, t_bf16, workspace, workspace_bytes, rows, N1, D, dropout, stream, 2);
}
// The wide forms (include/ucod_dpl.h): N1 up to UCOD_LORA_WIDE_MAX_N1; up to 8192 the launches, the workspace and the bits of the forms above.
static_assert(UCOD_LORA_WIDE_MAX_N1 == 5 * 256 * 8 && UCOD_LORA_WIDE_MAX_K == 2 * 512 * 8, "the wide kernels' vectors per thread");
extern "C" int ucod_lora_mlp_pack_wide(const float* lora_mlp, int r, float scaling, void* fc1_w_aug, int N1, int D, void* stream) {
  return mlp_pack(lora_mlp, r, scaling, fc1_w_aug, N1, D, stream, 1, true);
}
extern "C" int ucod_lora_mlp_pair_pack_wide(const float* lora_pair, int r, float scaling, void* fc1_w_aug, int N1, int D, void* stream) {
  return mlp_pack(lora_pair, r, scaling, fc1_w_aug, N1, D, stream, 2, true);
}
extern "C" size_t ucod_lora_mlp_grad_workspace_bytes_wide(int N1, int D) { return mlp_grad_workspace_bytes(N1, D, 1, true); }
extern "C" size_t ucod_lora_mlp_pair_grad_workspace_bytes_wide(int N1, int D) { return mlp_grad_workspace_bytes(N1, D, 2, true); }
extern "C" int ucod_lora_mlp_grad_wide(const void* dpre, const void* h2_aug, const float* lora_mlp, int r, float scaling, float* grad_mlp, void* t_bf16,
                                       void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_grad(dpre, h2_aug, lora_mlp, r, scaling, grad_mlp, t_bf16, workspace, workspace_bytes, rows, N1, D, dropout, stream, 1, true);
}
extern "C" int ucod_lora_mlp_pair_grad_wide(const void* dpre, const void* h2_aug, const float* lora_pair, int r, float scaling, float* grad_pair, void* t_bf16,
                                            void* workspace, size_t workspace_bytes, int rows, int N1, int D, const ucod_lora_dropout* dropout, void* stream) {
  return mlp_grad(dpre, h2_aug, lora_pair, r, scaling, grad_pair, t_bf16, workspace, workspace_bytes, rows, N1, D, dropout, stream, 2, true);
}
extern "C" int ucod_layernorm_bwd_lora_mlp(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                           void* s_bf16, int rows, int D, float eps, const void* t_bf16, int ldt, const float* a_m, int r,
                                           const ucod_lora_dropout* dropout, void* stream) {
  return mlp_ln_bwd(dy, x, flags, gamma, dres, next_scale, dx, s_bf16, rows, D, eps, t_bf16, ldt, a_m, r, dropout, stream, 1);
}
extern "C" int ucod_layernorm_bwd_lora_mlp_pair(const void* dy, const void* x, int flags, const float* gamma, const float* dres, const float* next_scale, float* dx,
                                                void* s_bf16, int rows, int D, float eps, const void* t_bf16, int ldt, const float* a_pair, int r,
                                                const ucod_lora_dropout* dropout, void* stream) {
  return mlp_ln_bwd(dy, x, flags, gamma, dres, next_scale, dx, s_bf16, rows, D, eps, t_bf16, ldt, a_pair, r, dropout, stream, 2);
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA bias="all" (full_model.py:53,66): the gradient of a LayerNorm's beta is the column sum of the COMPLETE cotangent of its output.  Where ln_bwd_kernel<.., LORA>
// adds the masked branch sum_p mask_p/(1-p) (t_p A_p) to dy in registers (LayerNorm 1 with dropout on, LayerNorm 2 whenever the MLP input carries an adapter), that
// cotangent never reaches memory, so the sum is taken here from the same operands and through the same Drop / drop_scale:
//   out[n] = sum_m ( dy[m][n] + sum_p drop_scale_p(m D + n) * sum_j t_p[m][j] A_p[j][n] )
// The structure and the order of every addition are those of colsum_partial_kernel / colsum_finish_kernel (csrc/colsum.hip): grid (column groups, slabs), 16 row
// threads x 16 column vectors of 16 bytes, a thread adds rows rt, rt + 16, ... of its slab in ascending order, the row threads are added through LDS in ascending
// rt, a second launch adds the slabs in ascending order (csrc/colsum.h: the constants, colsum_slabs and colsum_finish_kernel are that file's).  No float atomics;
// without a branch the entry point calls ucod_colsum_det itself.
// R > 0 (r = 2, 4; r = 8 with one or two modules): the rank is known at compile time, the NP * R vectors of A for the thread's columns stay in registers across its rows, and a module's R values
// of t are read as R / 2 four-byte loads (the host sends a t that is not 4-byte aligned to the generic loop).  R = 0: the generic rank loop, A from L1 / L2 in
// every row -- r = 8 with THREE modules would be 192 registers of A beside the row's own, so it stays here, with every other rank.  The 16 column threads of a row thread read the same
// t addresses: broadcast loads.
// ---------------------------------------------------------------------------------------------------------------------
namespace ucod {

template <bool F32, int NP, int R>
__global__ __launch_bounds__(CS_THREADS) void colsum_lora_partial_kernel(const void* __restrict__ dy, float* __restrict__ part, int M, int D, int rows_per_slab,
                                                                          const bf16_raw* __restrict__ tq, int ldt, const float* __restrict__ lora, int r, int astride,
                                                                          Drop drop) {
  constexpr int VW = F32 ? 4 : 8;                                // columns per 16-byte vector of dy
  constexpr int NA = (NP > 0 && R > 0) ? NP * R : 1;
  __shared__ float sm[CS_RT][CS_CV * VW];
  const int cv = threadIdx.x % CS_CV, rt = threadIdx.x / CS_CV;
  const int col0 = (blockIdx.x * CS_CV + cv) * VW;
  const long r0 = (long)blockIdx.y * rows_per_slab;
  const long r1 = r0 + rows_per_slab < (long)M ? r0 + rows_per_slab : (long)M;
  float acc[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) acc[e] = 0.f;
  if (col0 < D) {                                                // (D % 128 == 0: a vector that starts below D ends below it)
    auto a_row = [&](int p, int j, float* a) {                   // A_p[j][col0 .. col0 + VW): 8-byte loads (the arena's alignment, as ln_bwd_kernel with VW = 2)
      const float2* src = reinterpret_cast<const float2*>(lora + (size_t)p * astride + (size_t)j * D + col0);
#pragma unroll
      for (int e = 0; e < VW / 2; ++e) {
        const float2 v = src[e];
        a[2 * e] = v.x;
        a[2 * e + 1] = v.y;
      }
    };
    float av[NA][VW];
    if constexpr (NP > 0 && R > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < R; ++j) a_row(p, j, av[p * R + j]);
    }
#pragma unroll 4
    for (long m = r0 + rt; m < r1; m += CS_RT) {
      float d[VW];
      if constexpr (F32) {
        const f32x4 v = *(const f32x4*)((const float*)dy + (size_t)m * D + col0);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = v[e];
      } else {
        const u32x4 v = *(const u32x4*)((const bf16_raw*)dy + (size_t)m * D + col0);
#pragma unroll
        for (int e = 0; e < 4; ++e) unpack_h2(v[e], d[2 * e], d[2 * e + 1]);
      }
      if constexpr (NP > 0) {
        const unsigned idx = (unsigned)m * (unsigned)D + (unsigned)col0;   // the element index of ln_lora / ln_bwd: the forward's mask, element for element
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          float b[VW];
#pragma unroll
          for (int e = 0; e < VW; ++e) b[e] = 0.f;
          if constexpr (R > 0) {
            float t[R];
            const unsigned* t2 = reinterpret_cast<const unsigned*>(tq + (size_t)m * ldt + p * R);      // (R even, tq 4-byte aligned, ldt even: the host's rule)
#pragma unroll
            for (int j = 0; j < R / 2; ++j) unpack_h2(t2[j], t[2 * j], t[2 * j + 1]);
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
              for (int e = 0; e < VW; ++e) b[e] += t[j] * av[p * R + j][e];
          } else {
            for (int j = 0; j < r; ++j) {
              const float t = bf16_to_f32(tq[(size_t)m * ldt + p * r + j]);
              float a[VW];
              a_row(p, j, a);
#pragma unroll
              for (int e = 0; e < VW; ++e) b[e] += t * a[e];
            }
          }
          if (drop.thresh) {
#pragma unroll
            for (int e = 0; e < VW; ++e) d[e] += b[e] * drop_scale(drop, p, idx + (unsigned)e);
          } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) d[e] += b[e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[e] += d[e];
    }
  }
#pragma unroll
  for (int e = 0; e < VW; ++e) sm[rt][cv * VW + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < CS_CV * VW) {
    const int n = blockIdx.x * CS_CV * VW + threadIdx.x;
    float s = sm[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < CS_RT; ++q) s += sm[q][threadIdx.x];
    if (n < D) part[(size_t)blockIdx.y * D + n] = s;
  }
}

}  // namespace ucod

extern "C" size_t ucod_colsum_det_lora_workspace_bytes(int M, int D) {
  if (M < 1 || D < 128 || D % 128 != 0) return 0;
  return (size_t)colsum_slabs(M) * (size_t)D * sizeof(float);
}

extern "C" int ucod_colsum_det_lora(const void* dy, int flags, int M, int D, const void* t_bf16, int ldt, const float* lora, int np, int r,
                                    const ucod_lora_dropout* dropout, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  UCOD_BF16_ONLY();
  if (!dy || !out || !workspace || (flags & ~3)) return UCOD_EINVAL;
  const size_t need = ucod_colsum_det_lora_workspace_bytes(M, D);
  if (need == 0 || workspace_bytes < need) return UCOD_EINVAL;
  if ((((uintptr_t)dy) & 15) || ((((uintptr_t)out) | ((uintptr_t)workspace)) & 3)) return UCOD_EINVAL;
  if (t_bf16) {
    if (!lora || (np != 1 && np != 2 && np != 3) || r < 1 || np * r > AUG || (np != 3 && r > UCOD_LORA_MLP_MAX_R) || ldt < np * r) return UCOD_EINVAL;
    if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
    if ((((uintptr_t)lora) & 7) || (((uintptr_t)t_bf16) & 1)) return UCOD_EINVAL;
  }
  const bool f32 = !(flags & UCOD_LNB_DY_BF16);
  // without a branch: ucod_colsum_det itself (D % 128 == 0 and the alignment checked above are within its rules)
  if (!t_bf16) return ucod_colsum_det(dy, f32 ? UCOD_ROPE_ELEM_F32 : UCOD_ROPE_ELEM_HALF, M, D, D, nullptr, out, workspace, workspace_bytes, stream);
  UCOD_PROF(PROF_COLSUM, stream);
  const int slabs = colsum_slabs(M), rows_per_slab = (int)(((long)M + slabs - 1) / slabs);
  const int astride = (np == 3 ? 2 : 1) * r * D;             // from A_p to A_{p+1} (launch_ln_bwd)
  const Drop drop = make_drop(dropout);
  const bool t4 = !(((uintptr_t)t_bf16) & 3) && !(ldt & 1);   // a module's t values can be read two at a time
  const bf16_raw* tq = (const bf16_raw*)t_bf16;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  const dim3 grid(cdiv(D, CS_CV * (f32 ? 4 : 8)), slabs), block(CS_THREADS);
#define L(f, np_, r_) hipLaunchKernelGGL((colsum_lora_partial_kernel<f, np_, r_>), grid, block, 0, s, dy, part, M, D, rows_per_slab, tq, ldt, lora, r, astride, drop)
#define P(f, np_)                                 \
  do {                                            \
    if (r == 2 && t4) L(f, np_, 2);               \
    else if (r == 4 && t4) L(f, np_, 4);          \
    else L(f, np_, 0);                            \
  } while (0)
#define P8(f, np_)                                \
  do {                                            \
    if (r == 8 && t4) L(f, np_, 8);               \
    else P(f, np_);                               \
  } while (0)
#define F(f)                                      \
  do {                                            \
    if (np == 1) P8(f, 1);                        \
    else if (np == 2) P8(f, 2);                   \
    else P(f, 3);                                 \
  } while (0)
  if (f32) F(true);
  else F(false);
#undef F
#undef P8
#undef P
#undef L
  UCOD_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv(D, CS_THREADS)), dim3(CS_THREADS), 0, s, part, (const float*)nullptr, out, D, slabs);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA on the output projections (attention.output.dense / o_proj, mlp.fc2 / down_proj; full_model.py:47-72 hands target_modules to peft, whose module computes
// result = base(x) + scaling * B(A(dropout(x)))).  Their inputs -- the attention kernel's output, the fc1 drain's hidden -- have no room for aug columns, so the
// module runs BESIDE its GEMM as row kernels:
//   forward   u [M, 8] f32 = drop(x_in) A^T (r values, the rest zero);  x[m, :] += lambda * (alpha/r * u[m, :] B^T)  behind the residual GEMM      (ucod_lora_out_fwd)
//   backward  s = bf16(lambda * dx), the dgrad GEMM's operand:  t [M, 8] f32 = alpha/r * s B,  dB = alpha/r * s^T u                                  (ucod_lora_out_grad_s)
//             dA = t^T drop(x_in);  cotangent of x_in += act'(pre) * mask/(1-p) * (t A), in the bf16 buffer the dgrad GEMM wrote                     (ucod_lora_out_grad_x)
// x_in is the saved attention output (identity) or gelu(pre) recomputed from the saved pre-activation with the drains' own fit (gelu_erf2 / gelu_grad2).
// Parameter layout of one module of one layer (f32): [A (r x K) | B (D x r)], K = D (dense) or F (fc2).  Mask: projection 0 of the counter hash over [M, K].
// Gradients: per-block partials, summed in a fixed order by lora_out_reduce_kernel -- no float atomics.
// ---------------------------------------------------------------------------------------------------------------------
namespace ucod {

constexpr int OUT_W = UCOD_LORA_OUT_W;                            // floats per row of u and t
constexpr int OUT_RB = 4;                                        // rows a block (grad_s) or a thread (grad_x) has in flight
static inline int out_grad_s_blocks(int rows) { return cdiv(rows, OUT_RB) < 512 ? cdiv(rows, OUT_RB) : 512; }
static inline int out_grad_x_blocks(int rows) { return cdiv(rows, OUT_RB) < 256 ? cdiv(rows, OUT_RB) : 256; }

// A block's 256 threads share a row: thread `tid` owns the 16-byte vectors tid + 256 i of x_in (its A values stay in registers for all the block's rows); the r dot
// products are summed over the block through LDS (one barrier per row: two buffers in turn), thread j < 8 stores u[row][j], then the D-wide row of the stream is
// updated with lambda * alpha/r * B from LDS ([RW][D]: consecutive threads read consecutive 16 bytes).  XH16: the stream is IEEE fp16 (clamped and counted like
// every writer of that stream).  u_out NULL (the no-grad pass): nothing is saved.
// NT = 512 is the wide form (4096 < K <= UCOD_LORA_WIDE_MAX_K): two vectors per thread of a block twice as wide, two waves per SIMD at up to 256 registers, eight
// wave partials summed as two groups of four.
template <int NVT, int RW, bool XH16, int NT = 256>
__global__ __launch_bounds__(NT) void lora_out_fwd_kernel(const bf16_raw* __restrict__ x_in, const float* __restrict__ lora, const float* __restrict__ lam, int r,
                                                           float scaling, void* __restrict__ xs, float* __restrict__ u_out, int rows, int K, int D, Drop drop,
                                                           unsigned* __restrict__ ovf) {
  extern __shared__ __attribute__((aligned(16))) float out_smem[];
  float* sB = out_smem;                                          // [RW][D]
  constexpr int NW = NT / 64;
  static_assert(NW == 4 || NW == 8, "four or eight waves");
  float* red = out_smem + RW * D;                                // [2][NW][RW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NV = K / 8;
  const float* Bo = lora + (size_t)r * K;
  float a[NVT][8][RW];
#pragma unroll
  for (int i = 0; i < NVT; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int j = 0; j < RW; ++j) a[i][e][j] = (tid + NT * i < NV && j < r) ? lora[(size_t)j * K + 8 * (tid + NT * i) + e] : 0.f;
  for (int idx = tid; idx < RW * D; idx += NT) {
    const int j = idx / D, d = idx - j * D;
    sB[idx] = j < r ? (lam ? lam[d] : 1.f) * scaling * Bo[(size_t)d * r + j] : 0.f;
  }
  __syncthreads();
  typedef float f4 __attribute__((ext_vector_type(4)));
  bool sat = false;
  int buf = 0;
  for (int row = blockIdx.x; row < rows; row += gridDim.x, buf ^= 1) {
    const u32x4* xr = reinterpret_cast<const u32x4*>(x_in + (size_t)row * K);
    float s[RW];
#pragma unroll
    for (int j = 0; j < RW; ++j) s[j] = 0.f;
#pragma unroll
    for (int i = 0; i < NVT; ++i) {
      const int v = tid + NT * i;
      const u32x4 w = v < NV ? xr[v] : (u32x4)(0u);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x0 = __uint_as_float(w[q] << 16), x1 = __uint_as_float(w[q] & 0xFFFF0000u);
        if (drop.thresh) {
          const unsigned idx = (unsigned)row * (unsigned)K + 8u * (unsigned)v + 2u * (unsigned)q;
          x0 *= drop_scale(drop, 0, idx);
          x1 *= drop_scale(drop, 0, idx + 1u);
        }
#pragma unroll
        for (int j = 0; j < RW; ++j) s[j] += x0 * a[i][2 * q][j] + x1 * a[i][2 * q + 1][j];
      }
    }
    float* rb = red + buf * NW * RW;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const float ws = wave_sum(s[j]);
      if (lane == 0) rb[wave * RW + j] = ws;
    }
    __syncthreads();
    auto waves = [&](int j) {
      const float lo = (rb[j] + rb[RW + j]) + (rb[2 * RW + j] + rb[3 * RW + j]);
      if constexpr (NW == 8) return lo + ((rb[4 * RW + j] + rb[5 * RW + j]) + (rb[6 * RW + j] + rb[7 * RW + j]));
      else return lo;
    };
    float u[RW];
#pragma unroll
    for (int j = 0; j < RW; ++j) u[j] = waves(j);
    if (u_out && tid < OUT_W) u_out[(size_t)row * OUT_W + tid] = tid < RW ? waves(tid) : 0.f;
    for (int c = tid; c < D / 4; c += NT) {
      f4 acc = (f4)(0.f);
#pragma unroll
      for (int j = 0; j < RW; ++j) acc += u[j] * *reinterpret_cast<const f4*>(sB + j * D + 4 * c);
      if constexpr (XH16) {
        u32x2* p = reinterpret_cast<u32x2*>(xs) + (size_t)row * (D / 4) + c;
        const u32x2 w = *p;
        float x0, x1, x2, x3;
        unpack_f16x2(w[0], x0, x1);
        unpack_f16x2(w[1], x2, x3);
        x0 += acc[0], x1 += acc[1], x2 += acc[2], x3 += acc[3];
        sat |= beyond_f16(x0) || beyond_f16(x1) || beyond_f16(x2) || beyond_f16(x3);
        *p = (u32x2){pack_f16x2(clamp_f16(x0), clamp_f16(x1)), pack_f16x2(clamp_f16(x2), clamp_f16(x3))};
      } else {
        f4* p = reinterpret_cast<f4*>(xs) + (size_t)row * (D / 4) + c;
        *p += acc;
      }
    }
  }
  if (XH16 && sat) atomicAdd(ovf, 1u);
}

// t and the partials of dB in one pass over s [rows, D] and u [rows, 8].  The block's threads share OUT_RB rows at a time: thread `tid` owns the column pairs
// tid + 256 i of s (its B values and dB accumulators stay in registers), the partial t of the rows is summed through LDS (one barrier per OUT_RB rows), thread
// 8 q + j stores t[row0 + q][j].  Partials [D][r] per block.
template <int NPT, int RW>
__global__ __launch_bounds__(256) void lora_out_grad_s_kernel(const bf16_raw* __restrict__ s, const float* __restrict__ u, const float* __restrict__ Bo, int r,
                                                              float scaling, float* __restrict__ partial, float* __restrict__ tout, int rows, int D) {
  constexpr int RB = OUT_RB;
  __shared__ float red[2][4][RB][RW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NP2 = D / 2;
  float bw[NPT][2][RW], accB[NPT][2][RW];
#pragma unroll
  for (int i = 0; i < NPT; ++i)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        bw[i][e][j] = (tid + 256 * i < NP2 && j < r) ? Bo[(size_t)(2 * (tid + 256 * i) + e) * r + j] : 0.f;
        accB[i][e][j] = 0.f;
      }
  int buf = 0;
  for (int row0 = blockIdx.x * RB; row0 < rows; row0 += gridDim.x * RB, buf ^= 1) {
    unsigned sw[RB][NPT];
    float uu[RB][RW];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const bool live = row0 + q < rows;
      const int row = live ? row0 + q : rows - 1;
      const unsigned* sr = reinterpret_cast<const unsigned*>(s + (size_t)row * D);
#pragma unroll
      for (int i = 0; i < NPT; ++i) sw[q][i] = (live && tid + 256 * i < NP2) ? sr[tid + 256 * i] : 0u;
#pragma unroll
      for (int j = 0; j < RW; ++j) uu[q][j] = (live && j < r) ? u[(size_t)row * OUT_W + j] : 0.f;      // (block-uniform address)
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      float ss[RW];
#pragma unroll
      for (int j = 0; j < RW; ++j) ss[j] = 0.f;
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const float d0 = __uint_as_float(sw[q][i] << 16), d1 = __uint_as_float(sw[q][i] & 0xFFFF0000u);
#pragma unroll
        for (int j = 0; j < RW; ++j) {
          ss[j] += d0 * bw[i][0][j] + d1 * bw[i][1][j];
          accB[i][0][j] += d0 * uu[q][j];
          accB[i][1][j] += d1 * uu[q][j];
        }
      }
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        const float ws = wave_sum(ss[j]);
        if (lane == 0) red[buf][wave][q][j] = ws;
      }
    }
    __syncthreads();
    if (tid < RB * OUT_W) {
      const int q = tid / OUT_W, j = tid - q * OUT_W;
      if (row0 + q < rows)
        tout[(size_t)(row0 + q) * OUT_W + j] = j < RW ? scaling * ((red[buf][0][q][j] + red[buf][1][q][j]) + (red[buf][2][q][j] + red[buf][3][q][j])) : 0.f;
    }
  }
  float* out = partial + (size_t)blockIdx.x * (size_t)D * r;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int c = tid + 256 * i;
    if (c >= NP2) continue;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < RW; ++j)
        if (j < r) out[(size_t)(2 * c + e) * r + j] = scaling * accB[i][e][j];
  }
}

// dA partials and the cotangent update in one pass over x_in [rows, K] and its cotangent [rows, K] (bf16, in place).  No row is shared: thread (blockIdx.y, tid)
// owns ONE 16-byte vector of every row (its A values and dA accumulators stay in registers), the row's t comes from memory (block-uniform address), OUT_RB rows are
// in flight.  GELU: x_in = gelu(pre) and the term carries gelu'(pre) -- the cotangent buffer already holds dpre = dg * gelu'(pre).  Partials [r][K] per blockIdx.x.
template <int RW, bool GELU>
__global__ __launch_bounds__(128) void lora_out_grad_x_kernel(const bf16_raw* __restrict__ xin, bf16_raw* __restrict__ cot, const float* __restrict__ t,
                                                              const float* __restrict__ A, int r, float* __restrict__ partial, int rows, int K, Drop drop) {
  constexpr int RB = OUT_RB;
  const int v = blockIdx.y * 128 + threadIdx.x;
  if (v >= K / 8) return;                                        // (no barrier below)
  float a[8][RW], acc[8][RW];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      a[e][j] = j < r ? A[(size_t)j * K + 8 * v + e] : 0.f;
      acc[e][j] = 0.f;
    }
  for (int row0 = blockIdx.x * RB; row0 < rows; row0 += gridDim.x * RB) {
    u32x4 xw[RB], cw[RB];
    float tt[RB][RW];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const bool live = row0 + q < rows;
      const size_t row = live ? row0 + q : rows - 1;
      xw[q] = reinterpret_cast<const u32x4*>(xin + row * K)[v];
      cw[q] = reinterpret_cast<const u32x4*>(cot + row * K)[v];
#pragma unroll
      for (int j = 0; j < RW; ++j) tt[q][j] = (live && j < r) ? t[row * OUT_W + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (row0 + q >= rows) break;
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float x0 = __uint_as_float(xw[q][w] << 16), x1 = __uint_as_float(xw[q][w] & 0xFFFF0000u);
        float c0 = __uint_as_float(cw[q][w] << 16), c1 = __uint_as_float(cw[q][w] & 0xFFFF0000u);
        float g0 = 1.f, g1 = 1.f;
        if constexpr (GELU) {
          const f32x2 gr = gelu_grad2((f32x2){x0, x1}), gx = gelu_erf2((f32x2){x0, x1});
          g0 = gr[0], g1 = gr[1];
          x0 = gx[0], x1 = gx[1];
        }
        if (drop.thresh) {
          const unsigned idx = (unsigned)(row0 + q) * (unsigned)K + 8u * (unsigned)v + 2u * (unsigned)w;
          const float m0 = drop_scale(drop, 0, idx), m1 = drop_scale(drop, 0, idx + 1u);
          x0 *= m0, x1 *= m1;
          g0 *= m0, g1 *= m1;
        }
        float ta0 = 0.f, ta1 = 0.f;
#pragma unroll
        for (int j = 0; j < RW; ++j) {
          ta0 += tt[q][j] * a[2 * w][j];
          ta1 += tt[q][j] * a[2 * w + 1][j];
          acc[2 * w][j] += tt[q][j] * x0;
          acc[2 * w + 1][j] += tt[q][j] * x1;
        }
        o[w] = pack_bf16x2(c0 + g0 * ta0, c1 + g1 * ta1);
      }
      reinterpret_cast<u32x4*>(cot + (size_t)(row0 + q) * K)[v] = o;
    }
  }
  typedef float f4 __attribute__((ext_vector_type(4)));
  float* out = partial + (size_t)blockIdx.x * (size_t)r * K + 8 * v;
#pragma unroll
  for (int j = 0; j < RW; ++j)
    if (j < r) {
      *reinterpret_cast<f4*>(out + (size_t)j * K) = (f4){acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
      *reinterpret_cast<f4*>(out + (size_t)j * K + 4) = (f4){acc[4][j], acc[5][j], acc[6][j], acc[7][j]};
    }
}

// The SwiGLU form (UCOD_LORA_OUT_ACT_SWIGLU; Dinov2SwiGLUFFN's weights_out, the gated DINOv3 down_proj): the same structure over the saved interleaved
// pre-activation [rows, 2K] and its cotangent dpre [rows, 2K] (include/ucod_dpl.h: UCOD_EPI_BIAS_SWIGLU_BF16 -- 16 bytes hold x1 | x2 of four hidden units).  Thread
// (blockIdx.y, tid) owns the 16-byte vector of hidden units 4v .. 4v+3 of every row: 4 x r values of A and 4 x r accumulators.  The hidden h = silu(x1) * x2 is
// recomputed with the weights_in drain's silu_fast and never stored; the term's two derivative factors are the weights_out dgrad drain's own (swiglu_bwd1 with
// g = mask/(1-p) * (t A)).  A padded unit has x1 = x2 = 0 and a zero A column: h, dA and both terms are exact zeros.  Partials [r][K] per blockIdx.x.
template <int RW>
__global__ __launch_bounds__(128) void lora_out_grad_x_swiglu_kernel(const bf16_raw* __restrict__ pre, bf16_raw* __restrict__ dpre, const float* __restrict__ t,
                                                                     const float* __restrict__ A, int r, float* __restrict__ partial, int rows, int K, Drop drop) {
  constexpr int RB = OUT_RB;
  const int v = blockIdx.y * 128 + threadIdx.x;
  if (v >= K / 4) return;                                        // (no barrier below)
  float a[4][RW], acc[4][RW];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      a[e][j] = j < r ? A[(size_t)j * K + 4 * v + e] : 0.f;
      acc[e][j] = 0.f;
    }
  const size_t ld = 2 * (size_t)K;
  for (int row0 = blockIdx.x * RB; row0 < rows; row0 += gridDim.x * RB) {
    u32x4 xw[RB], cw[RB];
    float tt[RB][RW];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const bool live = row0 + q < rows;
      const size_t row = live ? row0 + q : rows - 1;
      xw[q] = reinterpret_cast<const u32x4*>(pre + row * ld)[v];
      cw[q] = reinterpret_cast<const u32x4*>(dpre + row * ld)[v];
#pragma unroll
      for (int j = 0; j < RW; ++j) tt[q][j] = (live && j < r) ? t[row * OUT_W + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (row0 + q >= rows) break;
      float d1[4], d2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {                              // words 0, 1: x1 of units 4v .. 4v+3; words 2, 3: x2
        const unsigned w1 = xw[q][e >> 1], w2 = xw[q][2 + (e >> 1)];
        const float x1 = __uint_as_float((e & 1) ? (w1 & 0xFFFF0000u) : (w1 << 16)), x2 = __uint_as_float((e & 1) ? (w2 & 0xFFFF0000u) : (w2 << 16));
        float h = silu_fast(x1) * x2, m = 1.f;
        if (drop.thresh) m = drop_scale(drop, 0, (unsigned)(row0 + q) * (unsigned)K + 4u * (unsigned)v + (unsigned)e);
        h *= m;
        float ta = 0.f;
#pragma unroll
        for (int j = 0; j < RW; ++j) {
          ta += tt[q][j] * a[e][j];
          acc[e][j] += tt[q][j] * h;
        }
        swiglu_bwd1(m * ta, x1, x2, d1[e], d2[e]);
      }
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const float c10 = __uint_as_float(cw[q][w] << 16), c11 = __uint_as_float(cw[q][w] & 0xFFFF0000u);
        const float c20 = __uint_as_float(cw[q][2 + w] << 16), c21 = __uint_as_float(cw[q][2 + w] & 0xFFFF0000u);
        o[w] = pack_bf16x2(c10 + d1[2 * w], c11 + d1[2 * w + 1]);
        o[2 + w] = pack_bf16x2(c20 + d2[2 * w], c21 + d2[2 * w + 1]);
      }
      reinterpret_cast<u32x4*>(dpre + (size_t)(row0 + q) * ld)[v] = o;
    }
  }
  typedef float f4 __attribute__((ext_vector_type(4)));
  float* out = partial + (size_t)blockIdx.x * (size_t)r * K + 4 * v;
#pragma unroll
  for (int j = 0; j < RW; ++j)
    if (j < r) *reinterpret_cast<f4*>(out + (size_t)j * K) = (f4){acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
}

// partial [nblk][n] -> out [n] (sum_partials: blocks in ascending order inside each of 8 slices, then the slices)
__global__ __launch_bounds__(256) void lora_out_reduce_kernel(const float* __restrict__ partial, int nblk, int n, float* __restrict__ out) {
  int i;
  float s;
  if (sum_partials(partial, nblk, n, i, s)) out[i] = s;
}

// wide: the _wide entry points and UCOD_LORA_WIDE, whose K may reach UCOD_LORA_WIDE_MAX_K; up to 4096 they run what the narrow ones run
static inline bool lora_out_dims_ok(int r, int K, int D, bool wide = false) {
  return r >= 1 && r <= UCOD_LORA_MLP_MAX_R && K >= 128 && K <= (wide ? UCOD_LORA_WIDE_MAX_K : 4096) && (K % 128) == 0 && D >= 128 && D <= 1536 && (D % 128) == 0;
}

}  // namespace ucod

static size_t out_grad_workspace_bytes(int r, int K, int D, bool wide) {
  if (!lora_out_dims_ok(r, K, D, wide)) return 0;
  const size_t bs = (size_t)512 * (size_t)D * r, bx = (size_t)256 * (size_t)r * K;      // the most blocks either gradient kernel runs
  return (bs > bx ? bs : bx) * sizeof(float);
}
extern "C" size_t ucod_lora_out_grad_workspace_bytes(int r, int K, int D) { return out_grad_workspace_bytes(r, K, D, false); }
extern "C" size_t ucod_lora_out_grad_workspace_bytes_wide(int r, int K, int D) { return out_grad_workspace_bytes(r, K, D, true); }

static int out_fwd(const void* x_in, const float* lora_out, int r, float scaling, const float* lambda, void* x_stream, int stream_f16, float* u_out, int rows, int K,
                   int D, const ucod_lora_dropout* dropout, void* stream, bool wide) {
  UCOD_BF16_ONLY();
  if (!x_in || !lora_out || !x_stream || rows <= 0 || !lora_out_dims_ok(r, K, D, wide) || (stream_f16 != 0 && stream_f16 != 1)) return UCOD_EINVAL;
  if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
  UCOD_PROF(PROF_LORA_OUT_FWD, stream);
  const Drop drop = make_drop(dropout);
  const int rw = r <= 2 ? 2 : 8, nvt = K / 8 <= 256 ? 1 : 2;
  const int nt = K > 4096 ? 512 : 256;                            // (the wide form: two vectors per thread of 512)
  const int nblk = rows < 2048 ? rows : 2048;
  const size_t lds = (size_t)(rw * D + 2 * (nt / 64) * rw) * sizeof(float);
  unsigned* ovf = stream_f16 ? resid16_overflow_counter() : nullptr;
#define OF(v, w, h, n) hipLaunchKernelGGL((lora_out_fwd_kernel<v, w, h, n>), dim3(nblk), dim3(n), lds, (hipStream_t)stream, (const bf16_raw*)x_in, lora_out, lambda, r, \
                                          scaling, x_stream, u_out, rows, K, D, drop, ovf)
#define OFH(v, w, n)                   \
  do {                                 \
    if (stream_f16) OF(v, w, true, n); \
    else OF(v, w, false, n);           \
  } while (0)
  if (nt == 512 && rw == 2) OFH(2, 2, 512);
  else if (nt == 512) OFH(2, 8, 512);
  else if (nvt == 1 && rw == 2) OFH(1, 2, 256);
  else if (nvt == 1) OFH(1, 8, 256);
  else if (rw == 2) OFH(2, 2, 256);
  else OFH(2, 8, 256);
#undef OFH
#undef OF
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_lora_out_fwd(const void* x_in, const float* lora_out, int r, float scaling, const float* lambda, void* x_stream, int stream_f16, float* u_out,
                                 int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream) {
  return out_fwd(x_in, lora_out, r, scaling, lambda, x_stream, stream_f16, u_out, rows, K, D, dropout, stream, false);
}
extern "C" int ucod_lora_out_fwd_wide(const void* x_in, const float* lora_out, int r, float scaling, const float* lambda, void* x_stream, int stream_f16,
                                      float* u_out, int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream) {
  return out_fwd(x_in, lora_out, r, scaling, lambda, x_stream, stream_f16, u_out, rows, K, D, dropout, stream, true);
}

static int out_grad_s(const void* s_bf16, const float* u, const float* lora_out, int r, float scaling, float* grad_out, float* t_out, void* workspace,
                      size_t workspace_bytes, int rows, int K, int D, void* stream, bool wide) {
  UCOD_BF16_ONLY();
  if (!s_bf16 || !u || !lora_out || !grad_out || !t_out || !workspace || rows <= 0) return UCOD_EINVAL;
  const size_t need = out_grad_workspace_bytes(r, K, D, wide);
  if (need == 0) return UCOD_EINVAL;
  if (workspace_bytes < need) return UCOD_ENOMEM;
  UCOD_PROF(PROF_LORA_OUT_GRAD_S, stream);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = out_grad_s_blocks(rows), npt = cdiv(D / 2, 256);
  const float* Bo = lora_out + (size_t)r * K;
#define GS(p, w) hipLaunchKernelGGL((lora_out_grad_s_kernel<p, w>), dim3(nblk), dim3(256), 0, st, (const bf16_raw*)s_bf16, u, Bo, r, scaling, (float*)workspace, t_out, \
                                    rows, D)
#define GSW(p)            \
  do {                    \
    if (r <= 2) GS(p, 2); \
    else GS(p, 8);        \
  } while (0)
  if (npt == 1) GSW(1);
  else if (npt == 2) GSW(2);
  else GSW(3);
#undef GSW
#undef GS
  UCOD_CHECK_LAUNCH();
  hipLaunchKernelGGL(lora_out_reduce_kernel, dim3(cdiv((long)D * r, 32)), dim3(256), 0, st, (const float*)workspace, nblk, D * r, grad_out + (size_t)r * K);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_lora_out_grad_s(const void* s_bf16, const float* u, const float* lora_out, int r, float scaling, float* grad_out, float* t_out, void* workspace,
                                    size_t workspace_bytes, int rows, int K, int D, void* stream) {
  return out_grad_s(s_bf16, u, lora_out, r, scaling, grad_out, t_out, workspace, workspace_bytes, rows, K, D, stream, false);
}
extern "C" int ucod_lora_out_grad_s_wide(const void* s_bf16, const float* u, const float* lora_out, int r, float scaling, float* grad_out, float* t_out,
                                         void* workspace, size_t workspace_bytes, int rows, int K, int D, void* stream) {
  return out_grad_s(s_bf16, u, lora_out, r, scaling, grad_out, t_out, workspace, workspace_bytes, rows, K, D, stream, true);
}

// (the SwiGLU form reads and writes rows of 2K values where the other forms have K: it is taken only with UCOD_LORA_OUT_SWIGLU in out_flags, so that a caller of
//  ucod_lora_out_grad_x, whose buffers are [rows, K], can never reach it -- there act = 2 stays the invalid argument it was)
extern "C" int ucod_lora_out_grad_x_ex(const void* x_in, int act, int out_flags, void* cot_bf16, const float* t, const float* lora_out, int r, float* grad_out,
                                       void* workspace, size_t workspace_bytes, int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream) {
  UCOD_BF16_ONLY();
  if (!x_in || !cot_bf16 || !t || !lora_out || !grad_out || !workspace || rows <= 0 || (out_flags & ~(UCOD_LORA_OUT_SWIGLU | UCOD_LORA_WIDE)) ||
      (act != UCOD_LORA_OUT_ACT_IDENTITY && act != UCOD_LORA_OUT_ACT_GELU && !(act == UCOD_LORA_OUT_ACT_SWIGLU && (out_flags & UCOD_LORA_OUT_SWIGLU))))
    return UCOD_EINVAL;
  const size_t need = out_grad_workspace_bytes(r, K, D, (out_flags & UCOD_LORA_WIDE) != 0);
  if (need == 0) return UCOD_EINVAL;
  if (dropout && (dropout->p < 0.f || dropout->p >= 1.f)) return UCOD_EINVAL;
  if (workspace_bytes < need) return UCOD_ENOMEM;
  const bool swiglu = act == UCOD_LORA_OUT_ACT_SWIGLU;
  UCOD_PROF(swiglu ? PROF_LORA_OUT_GRAD_X_SWIGLU : PROF_LORA_OUT_GRAD_X, stream);
  const Drop drop = make_drop(dropout);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = out_grad_x_blocks(rows);
  const dim3 grid(nblk, cdiv(swiglu ? K / 4 : K / 8, 128));      // (SwiGLU: a row of the interleaved [rows, 2K] buffers has K / 4 16-byte vectors)
#define GXS(w) hipLaunchKernelGGL((lora_out_grad_x_swiglu_kernel<w>), grid, dim3(128), 0, st, (const bf16_raw*)x_in, (bf16_raw*)cot_bf16, t, lora_out, r, \
                                  (float*)workspace, rows, K, drop)
#define GX(w, g) hipLaunchKernelGGL((lora_out_grad_x_kernel<w, g>), grid, dim3(128), 0, st, (const bf16_raw*)x_in, (bf16_raw*)cot_bf16, t, lora_out, r, \
                                    (float*)workspace, rows, K, drop)
  if (swiglu) {
    if (r <= 2) GXS(2);
    else GXS(8);
  } else if (act == UCOD_LORA_OUT_ACT_GELU) {
    if (r <= 2) GX(2, true);
    else GX(8, true);
  } else {
    if (r <= 2) GX(2, false);
    else GX(8, false);
  }
#undef GX
#undef GXS
  UCOD_CHECK_LAUNCH();
  hipLaunchKernelGGL(lora_out_reduce_kernel, dim3(cdiv((long)r * K, 32)), dim3(256), 0, st, (const float*)workspace, nblk, r * K, grad_out);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_lora_out_grad_x(const void* x_in, int act, void* cot_bf16, const float* t, const float* lora_out, int r, float* grad_out, void* workspace,
                                    size_t workspace_bytes, int rows, int K, int D, const ucod_lora_dropout* dropout, void* stream) {
  return ucod_lora_out_grad_x_ex(x_in, act, 0, cot_bf16, t, lora_out, r, grad_out, workspace, workspace_bytes, rows, K, D, dropout, stream);
}
