// CORAL SparseRefiner, training of the window branch (HRE.CSF): the small kernels of the backward of ex_loss (models/UDLR.py:52-75 through
// models/modules/CSF.py:38-43 and the CrossAttentionBlock of models/modules/mlp.py:134-148).  The heavy parts reuse the project's GEMMs, the
// LayerNorm backward and attention96_bwd.hip; this file holds the loss gradient, the depthwise-conv + mask-head backward, the LayerNorm
// parameter gradients and the transpose that turns a weight gradient dY^T X into the GEMM's A[M,K] B[N,K]^T form.  All f32 arithmetic, every
// reduction in a fixed order (per-block partials, then one ascending sum): two runs are bit-identical.  No atomics.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace {

constexpr int DW_SLABS = 64;            // row slabs of the conv reduction (at most; a function of n * H alone)
constexpr int LNP_SLABS = 128;          // row slabs of the LayerNorm parameter reduction (at most; a function of `rows` alone)
constexpr int LNP_MAXJ = 16;            // D <= 64 * LNP_MAXJ

// ------------------------------------------------------------------ d ex_loss / d window_preds (UDLR.py:62-75)
// g[i,p] = up / (2 n H W) * (sigmoid(x) - (w_i t + (1 - w_i) l)),  w_i = clamp(1.5 iou_i, 0, 1), l = sigmoid(l_up) > 0.5: the derivative of
// w BCEWithLogits(x, t) + (1 - w) BCEWithLogits(x, l) in x; w, l and t are constants of the loss (binary_iou works on integers).
__global__ __launch_bounds__(256) void window_loss_grad_kernel(const float* __restrict__ win_preds, const float* __restrict__ h_targets,
                                                               const int* __restrict__ win_flat, const float* __restrict__ l_up,
                                                               const float* __restrict__ iou, const float* __restrict__ upstream,
                                                               float* __restrict__ g, float inv_count, int H, int W, int ws) {
  const int i = blockIdx.y, HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int flat = win_flat[i], b = flat / (ws * ws), j = flat - b * (ws * ws);
  const int wy = j / ws, wx = j - wy * ws;
  const int y = p / W, xx = p - y * W;
  const float w = fminf(fmaxf(iou[i] * 1.5f, 0.f), 1.f);
  const float up = upstream ? upstream[0] : 1.f;
  const float xv = win_preds[(size_t)i * HW + p], tv = h_targets[(size_t)flat * HW + p];
  const float lv = sigmoid_acc(l_up[((size_t)b * ws * H + (size_t)wy * H + y) * (ws * W) + (size_t)wx * W + xx]) > 0.5f ? 1.f : 0.f;
  g[(size_t)i * HW + p] = up * inv_count * (sigmoid_acc(xv) - (w * tv + (1.f - w) * lv));
}

// ------------------------------------------------------------------ depthwise 7x7 conv + mask head, backward (CSF.py:13-25,41-42)
// S[tap,c] = sum_{i,p} g[i,p] x2[i,p+tap,c] (zero padding), summed here over the input pixels q = p + tap of one slab of image rows:
// thread = channel, 49 accumulators in registers, x2 read once (coalesced), g read through the scalar path.
__global__ __launch_bounds__(256) void dwconv7_s_partial_kernel(const float* __restrict__ g, const float* __restrict__ x2, float* __restrict__ part,
                                                                int nrows /* n * H */, int rows_per_slab, int H, int W, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x, slab = blockIdx.y;
  if (c >= C) return;
  float acc[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) acc[t] = 0.f;
  const int r0 = slab * rows_per_slab, r1 = min(nrows, r0 + rows_per_slab);
  for (int r = r0; r < r1; ++r) {
    const int i = r / H, qy = r - i * H;
    const float* gi = g + (size_t)i * H * W;
    for (int qx = 0; qx < W; ++qx) {
      const float xv = x2[((size_t)r * W + qx) * C + c];
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const int py = qy - (ky - 3);
        if (py < 0 || py >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int px = qx - (kx - 3);
          if (px < 0 || px >= W) continue;
          acc[ky * 7 + kx] = fmaf(gi[py * W + px], xv, acc[ky * 7 + kx]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 49; ++t) part[((size_t)slab * 49 + t) * C + c] = acc[t];
}

// the slabs in ascending order, then every parameter gradient of the two layers (G = sum g, one fixed tree per workgroup):
//   d dw[c][tap] = w1[c] S[tap,c]    d dwb[c] = w1[c] G    d w1[c] = dwb[c] G + sum_tap dw[tap,c] S[tap,c]    d b1 = G
__global__ __launch_bounds__(256) void dwconv7_param_finish_kernel(const float* __restrict__ part, int slabs, const float* __restrict__ g, int ng,
                                                                   const float* __restrict__ dwT, const float* __restrict__ dwb,
                                                                   const float* __restrict__ w1, float* __restrict__ d_dw /* [C,49] */,
                                                                   float* __restrict__ d_dwb, float* __restrict__ d_w1, float* __restrict__ d_b1, int C) {
  __shared__ float red[16];
  float gs = 0.f;
  for (int i = threadIdx.x; i < ng; i += 256) gs += g[i];
  const float G = block_sum(gs, red);
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0) d_b1[0] = G;
  if (c >= C) return;
  const float w = w1[c];
  float aw = dwb[c] * G;
  for (int t = 0; t < 49; ++t) {
    float s = 0.f;
    for (int sl = 0; sl < slabs; ++sl) s += part[((size_t)sl * 49 + t) * C + c];
    d_dw[(size_t)c * 49 + t] = w * s;
    aw = fmaf(dwT[t * C + c], s, aw);
  }
  d_dwb[c] = w * G;
  d_w1[c] = aw;
}

// dx2[i,q,c] = w1[c] sum_tap dw[tap,c] g[i,q-tap]: one workgroup per pixel, lane = channel
__global__ __launch_bounds__(256) void dwconv7_dx_kernel(const float* __restrict__ g, const float* __restrict__ dwT, const float* __restrict__ w1,
                                                         float* __restrict__ dx, int H, int W, int C) {
  const int i = blockIdx.z, qy = blockIdx.y, qx = blockIdx.x;
  const float* gi = g + (size_t)i * H * W;
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc = 0.f;
    for (int ky = 0; ky < 7; ++ky) {
      const int py = qy - (ky - 3);
      if (py < 0 || py >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const int px = qx - (kx - 3);
        if (px < 0 || px >= W) continue;
        acc = fmaf(dwT[(ky * 7 + kx) * C + c], gi[py * W + px], acc);
      }
    }
    dx[(((size_t)i * H + qy) * W + qx) * C + c] = w1[c] * acc;
  }
}

// ------------------------------------------------------------------ LayerNorm parameter gradients (mlp.py:136-138,146: norm_q, norm_kv, norm_mlp)
// dgamma[c] = sum_r dy[r,c] xhat[r,c], dbeta[c] = sum_r dy[r,c]; xhat from the row statistics recomputed here (two-pass, f32).
// A wave owns rows w, w + 4, ... of its slab (lane = columns lane + 64 j), the four waves are added in ascending order.
template <bool DY_BF16>
__global__ __launch_bounds__(256) void ln_param_partial_kernel(const void* __restrict__ dy_, const float* __restrict__ x, float* __restrict__ part,
                                                               int rows, int rows_per_slab, int D, float eps) {
  __shared__ float sm[4][2][64 * LNP_MAXJ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slab = blockIdx.x;
  const int nj = D / 64;
  float ag[LNP_MAXJ], ab[LNP_MAXJ];
#pragma unroll
  for (int j = 0; j < LNP_MAXJ; ++j) { ag[j] = 0.f; ab[j] = 0.f; }
  const int r0 = slab * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
  for (int r = r0 + wave; r < r1; r += 4) {
    const float* xr = x + (size_t)r * D;
    float xv[LNP_MAXJ], s = 0.f;
#pragma unroll
    for (int j = 0; j < LNP_MAXJ; ++j) {
      xv[j] = j < nj ? xr[lane + 64 * j] : 0.f;
      s += xv[j];
    }
    const float mean = wave_sum(s) / (float)D;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < LNP_MAXJ; ++j)
      if (j < nj) v = fmaf(xv[j] - mean, xv[j] - mean, v);
    const float rstd = rsqrtf(wave_sum(v) / (float)D + eps);
#pragma unroll
    for (int j = 0; j < LNP_MAXJ; ++j)
      if (j < nj) {
        const size_t o = (size_t)r * D + lane + 64 * j;
        const float d = DY_BF16 ? bf16_to_f32(((const bf16_raw*)dy_)[o]) : ((const float*)dy_)[o];
        ag[j] = fmaf(d, (xv[j] - mean) * rstd, ag[j]);
        ab[j] += d;
      }
  }
#pragma unroll
  for (int j = 0; j < LNP_MAXJ; ++j)
    if (j < nj) {
      sm[wave][0][lane + 64 * j] = ag[j];
      sm[wave][1][lane + 64 * j] = ab[j];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
    part[((size_t)slab * 2 + 0) * D + c] = ((sm[0][0][c] + sm[1][0][c]) + sm[2][0][c]) + sm[3][0][c];
    part[((size_t)slab * 2 + 1) * D + c] = ((sm[0][1][c] + sm[1][1][c]) + sm[2][1][c]) + sm[3][1][c];
  }
}

__global__ __launch_bounds__(256) void ln_param_finish_kernel(const float* __restrict__ part, int slabs, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int D) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  float sg = 0.f, sb = 0.f;
  for (int s = 0; s < slabs; ++s) {
    sg += part[((size_t)s * 2 + 0) * D + c];
    sb += part[((size_t)s * 2 + 1) * D + c];
  }
  dgamma[c] = sg;
  dbeta[c] = sb;
}

// ------------------------------------------------------------------ rows [M, ld] (f32 or bf16) -> bf16 [cols, Mp], zeros in the pad
template <bool SRC_BF16>
__global__ __launch_bounds__(256) void transpose_pad_kernel(const void* __restrict__ src_, bf16_raw* __restrict__ dst, int M, int cols, int ld, int Mp) {
  __shared__ bf16_raw tile[64][66];
  const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int m = m0 + r, c = c0 + tx;
    bf16_raw v = 0;
    if (m < M && c < cols) {
      const size_t o = (size_t)m * ld + c;
      v = SRC_BF16 ? ((const bf16_raw*)src_)[o] : f32_to_bf16(((const float*)src_)[o]);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int c = c0 + r, m = m0 + tx;
    if (c < cols && m < Mp) dst[(size_t)c * Mp + m] = tile[tx][r];
  }
}

// ------------------------------------------------------------------ gated ensembler, backward (GE_pix_level.py:16-25 differentiated in l2 and the fuser)
// Per pixel: w = GE_w (the forward's saved weight, a function of preds alone), y = l1 w + l2 (1 - w), z_k = a_k y + c_k, m_k = [z_k > 0] (torch's ReLU
// subgradient).  A workgroup owns a tile of 256 pixels: thread = pixel for dl2 and for staging (G, y) in LDS, then thread t < 192 owns the sum `t >> 6`
// (0: d d_k, 1: d a_k, 2: d c_k -- wave-uniform) of channel k = t & 63 and walks the tile in pixel order with broadcast LDS reads; thread 192 sums G.
// part[block][193] = [d d | d a | d c | d bias]: no cross-lane reduction, no atomics, one fixed order.
constexpr int GEB_TILE = 256;
constexpr int GEB_SUMS = 193;

__global__ __launch_bounds__(256) void ge_bwd_partial_kernel(const float* __restrict__ l1, const float* __restrict__ l2, const float* __restrict__ gew,
                                                             const float* __restrict__ f0w, const float* __restrict__ f0b, const float* __restrict__ f2w,
                                                             const float* __restrict__ G, float* __restrict__ dl2, float* __restrict__ part, int hw) {
  __shared__ float a[64], c[64], d[64], sg[GEB_TILE], sy[GEB_TILE];
  const int t = threadIdx.x;
  if (t < 64) { a[t] = f0w[t]; c[t] = f0b[t]; d[t] = f2w[t]; }
  __syncthreads();
  const int b = blockIdx.y, p = blockIdx.x * GEB_TILE + t;
  float gv = 0.f, y = 0.f;                                          // past the image: G = 0 adds exact zeros to every sum
  if (p < hw) {
    const size_t i = (size_t)b * hw + p;
    const float wt = gew[i];
    gv = G[i];
    y = l1[i] * wt + l2[i] * (1.f - wt);
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) s += fmaf(a[k], y, c[k]) > 0.f ? d[k] * a[k] : 0.f;
    dl2[i] = gv * (1.f - wt) * s;
  }
  sg[t] = gv;
  sy[t] = y;
  __syncthreads();
  if (t > 192) return;
  const int k = t & 63, which = t >> 6;
  const float ak = a[k], ck = c[k], dk = d[k];
  float acc = 0.f;
  if (which == 0) {
    for (int j = 0; j < GEB_TILE; ++j) acc = fmaf(sg[j], fmaxf(fmaf(ak, sy[j], ck), 0.f), acc);
  } else if (which == 1) {
    for (int j = 0; j < GEB_TILE; ++j) acc += fmaf(ak, sy[j], ck) > 0.f ? sg[j] * dk * sy[j] : 0.f;
  } else if (which == 2) {
    for (int j = 0; j < GEB_TILE; ++j) acc += fmaf(ak, sy[j], ck) > 0.f ? sg[j] * dk : 0.f;
  } else {
    for (int j = 0; j < GEB_TILE; ++j) acc += sg[j];
  }
  part[((size_t)b * gridDim.x + blockIdx.x) * GEB_SUMS + t] = acc;
}

// the workgroups' partials in ascending order, in f64 (window_loss_finish_kernel's way): thread = one of the 193 sums
__global__ __launch_bounds__(256) void ge_bwd_finish_kernel(const float* __restrict__ part, int blocks, float* __restrict__ d_f0w, float* __restrict__ d_f0b,
                                                            float* __restrict__ d_f2w, float* __restrict__ d_f2b) {
  const int t = threadIdx.x;
  if (t >= GEB_SUMS) return;
  double acc = 0.0;
  for (int s = 0; s < blocks; ++s) acc += (double)part[(size_t)s * GEB_SUMS + t];
  const float v = (float)acc;
  if (t < 64) d_f2w[t] = v;
  else if (t < 128) d_f0w[t - 64] = v;
  else if (t < 192) d_f0b[t - 128] = v;
  else d_f2b[0] = v;
}

// ------------------------------------------------------------------ adjoint of the window scatter-average (HRE.py:18-39): a gather
// dwin[i,p] = dl2[win_img[i], cy H + py, cx W + px] / (1 + 1e-6) -- the windows are distinct cells, so the count the forward divides by is 1.
// ACC: added to the g ucod_window_loss_grad wrote (one g for one CSF backward).  A window whose cell lies outside the image is left alone.
template <bool ACC>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ dl2, const int* __restrict__ coords, const int* __restrict__ win_img,
                                                            float* __restrict__ g, int B, int H, int W, int ws) {
  const int i = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int cy = coords[2 * i], cx = coords[2 * i + 1], b = win_img[i];
  if (cy < 0 || cy >= ws || cx < 0 || cx >= ws || b < 0 || b >= B) return;
  const int y = p / W, x = p - y * W;
  const float v = dl2[((size_t)b * ws * H + (size_t)cy * H + y) * (ws * W) + (size_t)cx * W + x] / (1.0f + 1e-6f);
  const size_t o = (size_t)i * H * W + p;
  g[o] = ACC ? g[o] + v : v;
}

}  // namespace
}  // namespace ucod

using namespace ucod;

extern "C" int ucod_window_loss_grad(const float* window_preds, const float* h_targets, const int* win_flat, const float* l_up, const float* iou,
                                     const float* upstream, float* g, int n, int B, int H, int W, int ws, void* stream) {
  if (!window_preds || !h_targets || !win_flat || !l_up || !iou || !g || n <= 0 || B <= 0 || H <= 0 || W <= 0 || ws <= 0 || n > 65535) return UCOD_EINVAL;
  if ((long)H * W >= (1l << 31) / 4) return UCOD_EINVAL;
  hipLaunchKernelGGL(window_loss_grad_kernel, dim3(cdiv((long)H * W, 256), n), dim3(256), 0, (hipStream_t)stream, window_preds, h_targets, win_flat, l_up, iou,
                     upstream, g, (float)(1.0 / (2.0 * n * H * W)), H, W, ws);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_dwconv7_maskdec_bwd(const float* g, const float* x_tokens, const float* dw_tapmajor, const float* dw_bias, const float* w1,
                                        float* d_dw, float* d_dw_bias, float* d_w1, float* d_b1, float* dx_tokens, void* workspace,
                                        size_t workspace_bytes, int n, int H, int W, int C, void* stream) {
  if (!g || !x_tokens || !dw_tapmajor || !dw_bias || !w1 || !d_dw || !d_dw_bias || !d_w1 || !d_b1 || !dx_tokens || !workspace) return UCOD_EINVAL;
  if (n <= 0 || H <= 0 || W <= 0 || C <= 0 || n > 65535 || H > 65535) return UCOD_EINVAL;
  if ((long)n * H * W >= (1l << 31) / 4) return UCOD_EINVAL;                                   // pixel counts and g offsets stay 32-bit
  const int nrows = n * H, slabs = nrows < DW_SLABS ? nrows : DW_SLABS, rps = cdiv(nrows, slabs), used = cdiv(nrows, rps);
  if (workspace_bytes < (size_t)slabs * 49 * C * sizeof(float)) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(dwconv7_s_partial_kernel, dim3(cdiv(C, 256), used), dim3(256), 0, s, g, x_tokens, part, nrows, rps, H, W, C);
  hipLaunchKernelGGL(dwconv7_param_finish_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, part, used, g, n * H * W, dw_tapmajor, dw_bias, w1, d_dw, d_dw_bias,
                     d_w1, d_b1, C);
  hipLaunchKernelGGL(dwconv7_dx_kernel, dim3(W, H, n), dim3(256), 0, s, g, dw_tapmajor, w1, dx_tokens, H, W, C);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_layernorm_param_grad(const void* dy, int flags, const float* x, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                         int rows, int D, float eps, void* stream) {
  if (!dy || !x || !dgamma || !dbeta || !workspace || rows <= 0 || D <= 0 || (D % 64) || D > 64 * LNP_MAXJ) return UCOD_EINVAL;
  if (flags & ~UCOD_LNB_DY_BF16) return UCOD_EINVAL;
  const int want = cdiv(rows, 64), slabs = want < LNP_SLABS ? want : LNP_SLABS, rps = cdiv(rows, slabs), used = cdiv(rows, rps);
  if (workspace_bytes < (size_t)slabs * 2 * D * sizeof(float)) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (flags & UCOD_LNB_DY_BF16)
    hipLaunchKernelGGL(ln_param_partial_kernel<true>, dim3(used), dim3(256), 0, s, dy, x, part, rows, rps, D, eps);
  else
    hipLaunchKernelGGL(ln_param_partial_kernel<false>, dim3(used), dim3(256), 0, s, dy, x, part, rows, rps, D, eps);
  hipLaunchKernelGGL(ln_param_finish_kernel, dim3(cdiv(D, 256)), dim3(256), 0, s, part, used, dgamma, dbeta, D);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_transpose_pad_bf16(const void* src, int src_is_bf16, int M, int cols, int ld, void* dst_bf16, void* stream) {
  if (!src || !dst_bf16 || M <= 0 || cols <= 0 || ld < cols || (src_is_bf16 != 0 && src_is_bf16 != 1)) return UCOD_EINVAL;
  int Mp = 64 * cdiv(M, 64);
  Mp = Mp < 128 ? 128 : Mp;
  if (cdiv(cols, 64) > 65535) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (src_is_bf16)
    hipLaunchKernelGGL(transpose_pad_kernel<true>, dim3(Mp / 64, cdiv(cols, 64)), dim3(256), 0, s, src, (bf16_raw*)dst_bf16, M, cols, ld, Mp);
  else
    hipLaunchKernelGGL(transpose_pad_kernel<false>, dim3(Mp / 64, cdiv(cols, 64)), dim3(256), 0, s, src, (bf16_raw*)dst_bf16, M, cols, ld, Mp);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" size_t ucod_gated_ensemble_bwd_workspace_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)B * cdiv((long)h * w, GEB_TILE) * GEB_SUMS * sizeof(float);
}

extern "C" int ucod_gated_ensemble_bwd(const float* l1_up, const float* l2, const float* ge_w, const float* f0w, const float* f0b, const float* f2w,
                                       const float* g_out, float* dl2, float* d_f0w, float* d_f0b, float* d_f2w, float* d_f2b, void* workspace,
                                       size_t workspace_bytes, int B, int h, int w, void* stream) {
  if (!l1_up || !l2 || !ge_w || !f0w || !f0b || !f2w || !g_out || !dl2 || !d_f0w || !d_f0b || !d_f2w || !d_f2b || !workspace) return UCOD_EINVAL;
  if (B <= 0 || h <= 0 || w <= 0 || B > 65535) return UCOD_EINVAL;
  if ((long)B * h * w >= (1l << 31) / 4) return UCOD_EINVAL;
  if (workspace_bytes < ucod_gated_ensemble_bwd_workspace_bytes(B, h, w)) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = cdiv((long)h * w, GEB_TILE);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(ge_bwd_partial_kernel, dim3(tiles, B), dim3(256), 0, s, l1_up, l2, ge_w, f0w, f0b, f2w, g_out, dl2, part, h * w);
  hipLaunchKernelGGL(ge_bwd_finish_kernel, dim3(1), dim3(256), 0, s, part, tiles * B, d_f0w, d_f0b, d_f2w, d_f2b);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_window_gather(const float* dl2, const int* coords, const int* win_img, float* g, int accumulate, int n, int B, int H, int W, int ws,
                                  void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || ws <= 0 || n < 0 || n > 65535 || (accumulate != 0 && accumulate != 1)) return UCOD_EINVAL;
  if ((long)B * ws * H * ws * W >= (1l << 31) / 4) return UCOD_EINVAL;
  if (n == 0) return UCOD_OK;
  if (!dl2 || !coords || !win_img || !g) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (accumulate)
    hipLaunchKernelGGL(window_gather_kernel<true>, dim3(cdiv((long)H * W, 256), n), dim3(256), 0, s, dl2, coords, win_img, g, B, H, W, ws);
  else
    hipLaunchKernelGGL(window_gather_kernel<false>, dim3(cdiv((long)H * W, 256), n), dim3(256), 0, s, dl2, coords, win_img, g, B, H, W, ws);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
