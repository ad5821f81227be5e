// Deterministic column sums of a row-major buffer: out[n] = col_scale[n] * sum_m x[m][n], f32 accumulation, no floating-point atomics.
// What LoRA bias="lora_only" (models/modules/full_model.py:53,66) needs from the backbone backward: for y = x W^T + b the bias gradient is the column sum over
// token rows of the cotangent of y, and those cotangents (dqkv, dpre, the operand s of the residual dgrads) are live buffers of csrc/vit_train_driver.hip.
//
// Two launches, in the idiom of the _det entry points (per-workgroup partials, then an ordered sum):
//   colsum_partial_kernel  grid (column groups, slabs).  A workgroup of 256 threads = 16 row threads x 16 column vectors of 16 bytes (8 sixteen-bit or 4 f32
//                          columns): a wave instruction reads 4 rows x 256 contiguous bytes.  A thread sums rows r0 + rt, r0 + rt + 16, ... of its slab in
//                          that order (4 loads in flight), the 16 row threads of a column are added through LDS in ascending rt, and the workgroup stores
//                          part[slab][n].
//   colsum_finish_kernel   one thread per column: part[0][n] + part[1][n] + ... ascending, times col_scale[n], stored.
// ucod_colsum_det_tok (LoRA bias="all": the patch embedding's bias) is the same pair of launches over a row selection: tokens first .. tok - 1 of every image.
// The slab count depends on M alone (colsum_slabs), so the order of every addition is a function of the shape: two runs are bit-identical.  A streaming kernel:
// M x N elements are read once, the partials (slabs x N f32, at most 128 rows) are written and read once.
#include "common.h"
#include "../../include/ucod_dpl.h"
#include "colsum.h"   // the workgroup's shape, colsum_slabs and colsum_finish_kernel: shared with ucod_colsum_det_lora (csrc/vit_train.hip)

namespace {

using namespace ucod;

// TOK: the M rows are tokens first .. tok - 1 of every image of x [B * tok, ld], taken in ascending order (selected row q = image q / (tok - first), token
// first + q % (tok - first)); the additions are those of the plain form over the selected rows, so first = 0 gives its bits
template <bool F32, bool TOK = false>
__global__ __launch_bounds__(CS_THREADS) void colsum_partial_kernel(const void* __restrict__ x, float* __restrict__ part, int M, int N, size_t ld, int rows_per_slab,
                                                                    int tok = 0, int first = 0) {
  constexpr int VW = F32 ? 4 : 8;         // columns per 16-byte vector
  __shared__ float sm[CS_RT][CS_CV * VW];
  const int cv = threadIdx.x % CS_CV, rt = threadIdx.x / CS_CV;
  const int col0 = (blockIdx.x * CS_CV + cv) * VW;
  const long r0 = (long)blockIdx.y * rows_per_slab;
  const long r1 = r0 + rows_per_slab < (long)M ? r0 + rows_per_slab : (long)M;
  float acc[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) acc[j] = 0.f;
  if (col0 < N) {                         // (N % 8 == 0: a vector that starts below N ends below it)
#pragma unroll 4
    for (long rs = r0 + rt; rs < r1; rs += CS_RT) {
      long r = rs;
      if constexpr (TOK) {   // (rs < M = B (tok - first) and B tok < 2^31, checked on the host: one 32-bit divide; r stays a long, so r * ld below cannot wrap)
        const unsigned span = (unsigned)(tok - first), img = (unsigned)rs / span;
        r = (long)(img * (unsigned)tok + (unsigned)first + ((unsigned)rs - img * span));
      }
      if constexpr (F32) {
        const f32x4 v = *(const f32x4*)((const float*)x + (size_t)r * ld + col0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[j];
      } else {
        const u32x4 v = *(const u32x4*)((const h_raw*)x + (size_t)r * ld + col0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float lo, hi;
          ucod::unpack_h2(v[e], lo, hi);
          acc[2 * e] += lo;
          acc[2 * e + 1] += hi;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) sm[rt][cv * VW + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < CS_CV * VW) {
    const int n = blockIdx.x * CS_CV * VW + threadIdx.x;
    float s = sm[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < CS_RT; ++q) s += sm[q][threadIdx.x];
    if (n < N) part[(size_t)blockIdx.y * N + n] = s;
  }
}

}  // namespace

extern "C" size_t ucod_colsum_det_workspace_bytes(int M, int N) {
  if (M < 1 || N < 8 || N % 8 != 0) return 0;
  return (size_t)colsum_slabs(M) * (size_t)N * sizeof(float);
}

extern "C" int ucod_colsum_det(const void* x, int elem, int M, int N, int ld, const float* col_scale, float* out, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!x || !out || !workspace || (elem != UCOD_ROPE_ELEM_HALF && elem != UCOD_ROPE_ELEM_F32)) return UCOD_EINVAL;
  const size_t need = ucod_colsum_det_workspace_bytes(M, N);
  if (need == 0 || ld < N || workspace_bytes < need) return UCOD_EINVAL;
  if (((size_t)ld * (elem == UCOD_ROPE_ELEM_F32 ? 4 : 2)) & 15) return UCOD_EINVAL;                         // every row starts on a 16-byte boundary
  if ((((uintptr_t)x) & 15) || ((((uintptr_t)out) | ((uintptr_t)workspace) | ((uintptr_t)col_scale)) & 3)) return UCOD_EINVAL;
  UCOD_PROF(ucod::PROF_COLSUM, stream);
  const int slabs = colsum_slabs(M), rows_per_slab = (int)(((long)M + slabs - 1) / slabs);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (elem == UCOD_ROPE_ELEM_F32)
    hipLaunchKernelGGL((colsum_partial_kernel<true>), dim3(ucod::cdiv(N, CS_CV * 4), slabs), dim3(CS_THREADS), 0, s, x, part, M, N, (size_t)ld, rows_per_slab, 0, 0);
  else
    hipLaunchKernelGGL((colsum_partial_kernel<false>), dim3(ucod::cdiv(N, CS_CV * 8), slabs), dim3(CS_THREADS), 0, s, x, part, M, N, (size_t)ld, rows_per_slab, 0, 0);
  UCOD_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ucod::cdiv(N, CS_THREADS)), dim3(CS_THREADS), 0, s, part, col_scale, out, N, slabs);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

// The rows of the patch embedding's output among the tokens of x [B * tok, ld]: tokens first .. tok - 1 of each image (CLS and register rows are no conv outputs)
extern "C" size_t ucod_colsum_det_tok_workspace_bytes(int B, int tok, int first, int N) {
  if (B < 1 || tok < 1 || first < 0 || first >= tok || (long)B * tok > 0x7fffffffL) return 0;
  return ucod_colsum_det_workspace_bytes(B * (tok - first), N);
}

extern "C" int ucod_colsum_det_tok(const void* x, int elem, int B, int tok, int first, int N, int ld, const float* col_scale, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!x || !out || !workspace || (elem != UCOD_ROPE_ELEM_HALF && elem != UCOD_ROPE_ELEM_F32)) return UCOD_EINVAL;
  const size_t need = ucod_colsum_det_tok_workspace_bytes(B, tok, first, N);
  if (need == 0 || ld < N || workspace_bytes < need) return UCOD_EINVAL;
  if (((size_t)ld * (elem == UCOD_ROPE_ELEM_F32 ? 4 : 2)) & 15) return UCOD_EINVAL;
  if ((((uintptr_t)x) & 15) || ((((uintptr_t)out) | ((uintptr_t)workspace) | ((uintptr_t)col_scale)) & 3)) return UCOD_EINVAL;
  UCOD_PROF(ucod::PROF_COLSUM, stream);
  const int M = B * (tok - first), slabs = colsum_slabs(M), rows_per_slab = (int)(((long)M + slabs - 1) / slabs);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (elem == UCOD_ROPE_ELEM_F32)
    hipLaunchKernelGGL((colsum_partial_kernel<true, true>), dim3(ucod::cdiv(N, CS_CV * 4), slabs), dim3(CS_THREADS), 0, s, x, part, M, N, (size_t)ld, rows_per_slab, tok,
                       first);
  else
    hipLaunchKernelGGL((colsum_partial_kernel<false, true>), dim3(ucod::cdiv(N, CS_CV * 8), slabs), dim3(CS_THREADS), 0, s, x, part, M, N, (size_t)ld, rows_per_slab, tok,
                       first);
  UCOD_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ucod::cdiv(N, CS_THREADS)), dim3(CS_THREADS), 0, s, part, col_scale, out, N, slabs);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
