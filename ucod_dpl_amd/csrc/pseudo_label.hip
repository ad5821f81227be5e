// Pseudo-label generator on the GPU: the upstream producer of the `pseudo_label` tensors the training step
// consumes (generate_pseudo_label.py:71-94 -> data/utils/found_bkg_mask.py:4-86).
//   ucod_cls_qk         q and k projections of the CLS token of the LAST layer (the only query row the generator reads from
//                       outputs.attentions[-1], found_bkg_mask.py:23) from that layer's LN1 output, which ucod_vit_forward leaves
//                       in its workspace;
//   ucod_cls_attention  softmax over ALL keys (CLS + patches) of that query per head, patch columns kept -- from the NCHW key map
//                       the backbone pass already produced (one token-contiguous row per channel: coalesced); ucod_cls_attention_rope: the same row of a
//                       DINOv3 model, the patch keys rotated by the rotary table as they are read (the key map stays the unrotated hook output);
//   ucod_bkg_seg        CroW sparsity weights, seed = least-attended patch, cosine similarity of every patch's (weighted) key
//                       descriptor to the seed's, background mask and similarity map.  Only the seed's row of the HW x HW
//                       similarity matrix is formed (the reference builds all of it and reads one row).  One workgroup per image.
// Everything is exact f32.  up_size (the optional bilinear upsampling of found_bkg_mask.py:26,50) is not built: the generator
// calls it with up_size = grid (generate_pseudo_label.py:83-89).
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) s = fmaxf(s, red[i]);
  return s;
}

// grid (B, 1 + nreg): one block per image and leading token r (0 = CLS, 1 .. nreg = register tokens); wave per output row of [Wq ; Wk].  The CLS block writes
// q [B, D] and row 0 of k [B, 1 + nreg, D]; a register token's block its key row only (rows D .. 2D-1 of the weight: its query is never read)
__global__ __launch_bounds__(256) void cls_qk_kernel(const bf16_raw* __restrict__ h, const bf16_raw* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ q, float* __restrict__ k, int tok, int D) {
  extern __shared__ float x[];                               // LN1(x_r) as f32
  const int b = blockIdx.x, r = blockIdx.y, lead = gridDim.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bf16_raw* hr = h + ((size_t)b * tok + r) * D;
  for (int i = threadIdx.x; i < D; i += 256) x[i] = h_to_f32(hr[i]);
  __syncthreads();
  for (int n = (r == 0 ? 0 : D) + wv; n < 2 * D; n += 4) {
    const bf16_raw* wr = w + (size_t)n * D;
    float s = 0.f;
    for (int i = lane; i < D; i += 64) s += h_to_f32(wr[i]) * x[i];
    s = wave_sum(s) + bias[n];
    if (lane == 0) {
      if (n < D) q[(size_t)b * D + n] = s;
      else k[((size_t)b * lead + r) * D + n - D] = s;
    }
  }
}

// grid (B, heads); att[b][h][j] for patches j (the CLS column and the `lead - 1` register-token columns dropped after the softmax, whose maximum and
// denominator include them: kc f32 [B, lead, D] holds their keys, CLS first)
// ROPE (DINOv3): the patch keys -- and only they: not the query, not kc -- are rotated by the rows of tab f32 [hw, 64] (cos 32 | sin 32 of patch j), regrouped
// so that no rotated key is formed: score_j = scale sum_{i<32} c_j[i] (q[i] k[i] + q[i+32] k[i+32]) + s_j[i] (q[i+32] k[i] - q[i] k[i+32]) = q . rotate(k_j).
// The sum is taken key column by key column, d = 0 .. 63 as the plain kernel takes it, each column times the query turned BACK by the patch's angles
// (k[i] (c q[i] + s q[i+32]) + k[i+32] (c q[i+32] - s q[i])): one product chain of the plain kernel's length and order, and where the angles are zero (cos 1,
// sin 0: a 1 x 1 grid) the very scores, bit for bit.
// Key-map reads stay coalesced along j (kb[d hw + j] and kb[(d + 32) hw + j]).  Table reads: STRAIGHT FROM L2, a lane walking its own 256-byte row in sixteen
// 16-byte loads -- not staged through LDS.  Every block of the grid reads the same table (256 KB at hw = 1024, resident in L2 beside nothing else of size), a
// lane uses each fetched line in full within one j, and a 256-row LDS tile at a padded pitch would take 65 KB where the kernel holds (hw + 8) floats today;
// tools/cls_row_bench.py measures what the rotation costs (profiles/dinov3_cls_row_kernel.txt: 47 us against the plain kernel's 28 at B = 32, 12 heads,
// hw = 1024; 106 VGPRs, no scratch).  The ROPE = false instantiation is the kernel as it was (tab is never read).
template <bool ROPE>
__global__ __launch_bounds__(256) void cls_attention_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ key,
                                                            float* __restrict__ att, int heads, int hw, float scale, int lead, const float* __restrict__ tab) {
  extern __shared__ float sc[];                              // hw scores, then 8 floats of reduction space
  float* red = sc + hw;
  const int b = blockIdx.x, hd = blockIdx.y, D = heads * 64;
  const float* qh = q + (size_t)b * D + hd * 64;
  const float* kb = key + ((size_t)b * D + hd * 64) * hw;
  float mx = -3.0e38f;
  for (int j = threadIdx.x; j < hw; j += 256) {
    float s = 0.f;
    if constexpr (ROPE) {
      const float4* row = reinterpret_cast<const float4*>(tab + (size_t)j * 64);     // cos: row[0 .. 7], sin: row[8 .. 15]
      float qr[32];                                          // columns 32 .. 63 of the query turned back by patch j's angles, held for the second half
#pragma unroll
      for (int i = 0; i < 32; i += 4) {
        const float4 c4 = row[i >> 2], s4 = row[8 + (i >> 2)];
        const float c[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = i + e;
          const float qa = qh[d], qp = qh[d + 32];
          s = fmaf(c[e] * qa + sn[e] * qp, kb[(size_t)d * hw + j], s);
          qr[d] = c[e] * qp - sn[e] * qa;
        }
      }
#pragma unroll
      for (int d = 0; d < 32; ++d) s = fmaf(qr[d], kb[(size_t)(d + 32) * hw + j], s);
    } else {
#pragma unroll 8
      for (int d = 0; d < 64; ++d) s += qh[d] * kb[(size_t)d * hw + j];
    }
    s *= scale;
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max(mx, red);
  auto lead_score = [&](int r) {                             // (wave-uniform, recomputed for the denominator: `lead` is 1 or a handful)
    float s = 0.f;
    for (int d = 0; d < 64; ++d) s += qh[d] * kc[((size_t)b * lead + r) * D + hd * 64 + d];
    return s * scale;
  };
  for (int r = 0; r < lead; ++r) mx = fmaxf(mx, lead_score(r));
  float sum = 0.f;
  for (int j = threadIdx.x; j < hw; j += 256) {
    const float e = __expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  for (int r = 0; r < lead; ++r) sum += __expf(lead_score(r) - mx);
  const float inv = 1.0f / sum;
  float* out = att + ((size_t)b * heads + hd) * hw;
  for (int j = threadIdx.x; j < hw; j += 256) out[j] = sc[j] * inv;
}

// one block per image.  cosr[b][j] = cosine similarity to the seed patch; mask = cos > th; simr = 1 - cos (normalised by the
// batch-wide maximum in bkg_finalize_kernel, as `sim_map.max()` is over the whole batch, found_bkg_mask.py:81).
__global__ __launch_bounds__(256) void bkg_seg_kernel(const float* __restrict__ att, const float* __restrict__ key, float* __restrict__ mask,
                                                      float* __restrict__ simr, float* __restrict__ cosr, int* __restrict__ seed, float* __restrict__ beta_out,
                                                      unsigned* __restrict__ gmax, int heads, int hw, float th, float eps, int apply_w) {
  extern __shared__ float sm[];
  float* red = sm;                                           // 8
  float* beta = sm + 8;                                      // heads
  float* qn = beta + heads;                                  // heads (sparsity counts)
  const int b = blockIdx.x, D = heads * 64;
  const float* ab = att + (size_t)b * heads * hw;
  const float* kb = key + (size_t)b * D * hw;
  // threshold = mean attention of the image
  float s = 0.f;
  for (int i = threadIdx.x; i < heads * hw; i += 256) s += ab[i];
  const float thr = block_sum(s, red) / (float)(heads * hw);
  for (int h = 0; h < heads; ++h) {
    float c = 0.f;
    for (int j = threadIdx.x; j < hw; j += 256) c += ab[(size_t)h * hw + j] > thr ? 1.f : 0.f;
    c = block_sum(c, red);
    if (threadIdx.x == 0) qn[h] = c / (float)hw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int h = 0; h < heads; ++h) tot += qn[h] + eps;
    for (int h = 0; h < heads; ++h) {
      beta[h] = logf(tot / (qn[h] + eps));
      beta_out[(size_t)b * heads + h] = beta[h];
    }
  }
  __syncthreads();
  // seed: first patch with the smallest (weighted) total attention
  float best = 3.0e38f;
  int bi = 0x7fffffff;
  for (int j = threadIdx.x; j < hw; j += 256) {
    float t = 0.f;
    for (int h = 0; h < heads; ++h) t += apply_w ? ab[(size_t)h * hw + j] * beta[h] : ab[(size_t)h * hw + j];
    if (t < best) { best = t; bi = j; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  __shared__ float wb[4];
  __shared__ int wi[4];
  if ((threadIdx.x & 63) == 0) { wb[threadIdx.x >> 6] = best; wi[threadIdx.x >> 6] = bi; }
  __syncthreads();
  best = wb[0];
  bi = wi[0];
  for (int w = 1; w < 4; ++w)
    if (wb[w] < best || (wb[w] == best && wi[w] < bi)) { best = wb[w]; bi = wi[w]; }
  const int ref = bi;
  if (threadIdx.x == 0) seed[b] = ref;
  // cosine similarity of every patch descriptor to the seed's
  float lmax = 0.f;
  for (int j = threadIdx.x; j < hw; j += 256) {
    float dot = 0.f, nj = 0.f, nr = 0.f;
    for (int c = 0; c < D; ++c) {
      const float w = apply_w ? beta[c >> 6] : 1.f;
      const float vj = kb[(size_t)c * hw + j] * w, vr = kb[(size_t)c * hw + ref] * w;
      dot += vj * vr;
      nj += vj * vj;
      nr += vr * vr;
    }
    const float cs = dot / (fmaxf(sqrtf(nj), 1e-12f) * fmaxf(sqrtf(nr), 1e-12f));
    cosr[(size_t)b * hw + j] = cs;
    mask[(size_t)b * hw + j] = cs > th ? 1.f : 0.f;
    const float sv = 1.f - cs;
    simr[(size_t)b * hw + j] = sv;
    lmax = fmaxf(lmax, sv);
  }
  lmax = block_max(lmax, red);
  if (threadIdx.x == 0) atomicMax(gmax, __float_as_uint(fmaxf(lmax, 0.f)));
}

__global__ __launch_bounds__(256) void bkg_finalize_kernel(const float* __restrict__ mask, float* __restrict__ sim, const unsigned* __restrict__ gmax, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float m = __uint_as_float(*gmax);
  sim[i] = sim[i] / (m + 1e-10f) * (1.f - mask[i]);
}

}  // namespace
}  // namespace ucod

using namespace ucod;

extern "C" int ucod_cls_qk_reg(const void* h_ln1_bf16, const void* qkv_w_bf16, const float* qkv_b, float* q_cls, float* k_lead, int B, int tok, int D, int n_reg,
                               void* stream) {
  if (!h_ln1_bf16 || !qkv_w_bf16 || !qkv_b || !q_cls || !k_lead || B <= 0 || tok <= 0 || D <= 0 || n_reg < 0 || n_reg >= tok || n_reg > 1023) return UCOD_EINVAL;
  hipLaunchKernelGGL(cls_qk_kernel, dim3(B, 1 + n_reg), dim3(256), (size_t)D * sizeof(float), (hipStream_t)stream, (const bf16_raw*)h_ln1_bf16,
                     (const bf16_raw*)qkv_w_bf16, qkv_b, q_cls, k_lead, tok, D);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_cls_qk(const void* h_ln1_bf16, const void* qkv_w_bf16, const float* qkv_b, float* q_cls, float* k_cls, int B, int tok, int D,
                           void* stream) {
  return ucod_cls_qk_reg(h_ln1_bf16, qkv_w_bf16, qkv_b, q_cls, k_cls, B, tok, D, 0, stream);
}

extern "C" int ucod_cls_attention_reg(const float* q_cls, const float* k_lead, const float* key_map, float* att, int B, int heads, int hw, int n_reg, float scale,
                                      void* stream) {
  if (!q_cls || !k_lead || !key_map || !att || B <= 0 || heads <= 0 || hw <= 0 || hw > 12000 || n_reg < 0 || n_reg > 1023) return UCOD_EINVAL;
  hipLaunchKernelGGL(cls_attention_kernel<false>, dim3(B, heads), dim3(256), (size_t)(hw + 8) * sizeof(float), (hipStream_t)stream, q_cls, k_lead, key_map, att,
                     heads, hw, scale, 1 + n_reg, (const float*)nullptr);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_cls_attention_rope(const float* q_cls, const float* k_lead, const float* key_map, const float* cos_sin, float* att, int B, int heads, int hw,
                                       int n_reg, float scale, void* stream) {
  if (!q_cls || !k_lead || !key_map || !cos_sin || !att || B <= 0 || heads <= 0 || hw <= 0 || hw > 12000 || n_reg < 0 || n_reg > 1023) return UCOD_EINVAL;
  if ((uintptr_t)cos_sin & 15) return UCOD_EINVAL;           // (16-byte loads of the table's rows, as ucod_rope_qk)
  hipLaunchKernelGGL(cls_attention_kernel<true>, dim3(B, heads), dim3(256), (size_t)(hw + 8) * sizeof(float), (hipStream_t)stream, q_cls, k_lead, key_map, att,
                     heads, hw, scale, 1 + n_reg, cos_sin);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
extern "C" int ucod_cls_attention(const float* q_cls, const float* k_cls, const float* key_map, float* att, int B, int heads, int hw, float scale,
                                  void* stream) {
  return ucod_cls_attention_reg(q_cls, k_cls, key_map, att, B, heads, hw, 0, scale, stream);
}

extern "C" int ucod_bkg_seg(const float* att, const float* key_map, float th_bkg, float epsilon, int apply_weights, float* bkg_mask, float* sim_map,
                            float* cos_row, int* seed, float* beta, void* scratch4, int B, int heads, int hw, void* stream) {
  if (!att || !key_map || !bkg_mask || !sim_map || !cos_row || !seed || !beta || !scratch4 || B <= 0 || heads <= 0 || heads > 64 || hw <= 0)
    return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(scratch4, 0, 4, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bkg_seg_kernel, dim3(B), dim3(256), (size_t)(8 + 2 * heads) * sizeof(float), s, att, key_map, bkg_mask, sim_map, cos_row, seed, beta,
                     (unsigned*)scratch4, heads, hw, th_bkg, epsilon, apply_weights);
  const size_t n = (size_t)B * hw;
  hipLaunchKernelGGL(bkg_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bkg_mask, sim_map, (const unsigned*)scratch4, n);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
