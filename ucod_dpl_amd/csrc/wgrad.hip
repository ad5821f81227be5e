// Weight gradient of a Linear layer from the token-major operands as the backward leaves them (CORAL refiner: the six products of the
// nn.MultiheadAttention / MLP block of models/modules/mlp.py:122-148 differentiated in their weights; the reference ships no second-stage
// step -- `LocalRefineTrainLoop: pass`, engine/runner/loop_CORAL.py:38-39 -- so this is the hot path of a step it never ran):
//     dW[n][k] (+)= sum_m dy[m][n] * x[m][k]          dy bf16 [M, ld_dy], x bf16 [M, ld_x], dW f32 [N, ld_dw]
// ops.weight_grad forms dy^T and x^T in global memory (two ucod_transpose_pad_bf16 passes) and runs the plain GEMM, whose 256 x 256 tiles
// walk all of M alone: nine tiles on 256 CUs at 768 x 768.  Here both operands are read where they lie and the TOKEN axis is split:
//   * rows are cut into nsplit chunks of chunk = 64 * ceil(ceil(M / nsplit) / 64) rows; a workgroup owns one 128 x 128 output tile of one chunk and
//     walks its rows in 64-row slabs; both slabs ([64][128] bf16, 256-byte rows) are staged ROW-major in LDS, as they are in memory;
//   * both MFMA operands are columns of those slabs: A[n][m] = dy[m][n], B[m][k] = x[m][k].  ds_read_b64_tr_b16 delivers them (the read of
//     attention96_bwd.hip and gemm_split.hip) from one image per operand with slot = chunk ^ (((row & 3) << 2) | ((row >> 2) & 3)): the 32 lanes of
//     a half then touch 32 different 8-byte bank pairs.  Every lane of every wave issues every read (EXEC all ones); rows past the chunk's end
//     and columns past N / K are staged as exact zeros, stores are masked instead: nothing is read or written out of bounds;
//   * the k index of a 32x32x16 product is the same row permutation for A and B (lane half h, element j -> slab row 4 h + (j & 3) + 8 (j >> 2)),
//     so each of the 16 rows is taken once;
//   * nsplit > 1: the f32 partial goes to ws[s][N][K]; wgrad_sum_kernel adds the partials in ascending s and then writes, or adds to, dW.
//     nsplit == 1: the tile is written (or added) to dW directly and no workspace is used.  No atomics: two runs are bit-identical.
// Counting, at 768 x 768 x 56 448: 36 tiles x 7 chunks = 252 workgroups on 256 CUs; every operand is read 6 times (1.04 GB through L2, a 64-row slab
// pair of 196 KiB being shared by the 36 workgroups of a chunk while it is hot); the partials are 7 x 2.25 MiB; the MFMA floor is 0.05 ms.  A 256-wide tile
// would halve the re-reads and leave 18 tiles, i.e. 14 chunks for the same fill -- and 72 tiles at 3072 x 768, where the rule below keeps the 144 tiles of
// this size at two chunks (288 workgroups, two resident per CU).  Measured (profiles/refiner_wgrad_bench.txt): ~0.4 PF/s at all five refiner shapes.
//   nsplit(M, N, K):  tiles = ceil(N / 128) * ceil(K / 128);  n = round(256 / tiles) clamped to [1, ceil(M / 64)];
//                     chunk = 64 * ceil(ceil(M / n) / 64);  nsplit = ceil(M / chunk)   (no empty chunk; chunk(nsplit) == chunk)
// bf16 in both libraries (the fp16-operand build trains nothing): explicit bf16 types, as attention96_bwd.hip.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace {

constexpr int WG_TILE = 128;            // output tile: 128 rows of dW (columns of dy) x 128 columns of dW (columns of x)
constexpr int WG_SLAB = 64;             // token rows per staged slab
constexpr int WG_ROW = 256;             // LDS row bytes: 128 bf16
constexpr int WG_IMG = WG_SLAB * WG_ROW;   // 16 KiB per operand
constexpr int WG_CUS = 256;

__device__ __forceinline__ int wg_slot(int row, int ch) { return ch ^ (((row & 3) << 2) | ((row >> 2) & 3)); }

// one operand's slab in flight: 64 rows x 32 groups of 4 columns (8 bytes: the alignment the entry point asks of row starts), 8 per thread
struct WgStage { u32x2 r[8]; };
__device__ __forceinline__ void wg_gload(WgStage& s, const bf16_raw* __restrict__ base, int ld, int row0, int row_end, int col0, int ncols, int tid) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = tid + 256 * i, row = idx >> 5, c4 = idx & 31;
    const int r = row0 + row, c = col0 + 4 * c4;
    u32x2 v = (u32x2){0u, 0u};
    if (r < row_end && c < ncols) v = *reinterpret_cast<const u32x2*>(base + (size_t)r * ld + c);
    s.r[i] = v;
  }
}
__device__ __forceinline__ void wg_lwrite(char* img, const WgStage& s, int tid) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = tid + 256 * i, row = idx >> 5, c4 = idx & 31;
    *reinterpret_cast<u32x2*>(img + row * WG_ROW + wg_slot(row, c4 >> 1) * 16 + 8 * (c4 & 1)) = s.r[i];
  }
}
// columns 32 cb + (lane & 31) of slab rows 16 ks + {4 h .. 4 h + 3, 4 h + 8 .. 4 h + 11}: off_lo / off_hi are the lane's byte offsets at ks = 0
__device__ __forceinline__ bf16x8 wg_read_tr(const char* img, int off_lo, int off_hi) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(img + off_lo));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(img + off_hi));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ int wg_tr_off(int lane, int cb, int hi) {
  const int h5 = lane >> 5, g1 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
  const int row = 4 * h5 + q + 8 * hi;
  return row * WG_ROW + wg_slot(row, 4 * cb + 2 * g1 + (p >> 1)) * 16 + 8 * (p & 1);
}

// grid (tiles_n * tiles_k, nsplit).  out: the chunk's partial ws + s * N * K with row stride K, or dW itself with row stride ld_dw when nsplit == 1
__global__ __launch_bounds__(256, 2) void wgrad_tile_kernel(const bf16_raw* __restrict__ dy, int ld_dy, const bf16_raw* __restrict__ x, int ld_x,
                                                            float* __restrict__ out, size_t split_stride, int ld_out, int M, int N, int K, int chunk,
                                                            int tiles_k, int add) {
  __shared__ __attribute__((aligned(16))) char smem[2 * WG_IMG];          // dy slab | x slab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h5 = lane >> 5, l31 = lane & 31;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x - tn * tiles_k;
  const int n0 = tn * WG_TILE, k0 = tk * WG_TILE;
  const int s = blockIdx.y;
  const long lo_row = (long)s * chunk;
  const int row_begin = lo_row < M ? (int)lo_row : M;
  const int row_end = lo_row + chunk < M ? (int)(lo_row + chunk) : M;
  const int nslab = (row_end - row_begin + WG_SLAB - 1) / WG_SLAB;
  const int wn = wave >> 1, wk = wave & 1;                                  // the wave's 64 x 64 quarter of the tile

  int offa[2][2], offb[2][2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
      offa[c][hi] = wg_tr_off(lane, 2 * wn + c, hi);
      offb[c][hi] = WG_IMG + wg_tr_off(lane, 2 * wk + c, hi);
    }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][0][i] = 0.f; acc[0][1][i] = 0.f; acc[1][0][i] = 0.f; acc[1][1][i] = 0.f; }

  WgStage sa, sb;
  if (nslab > 0) {
    wg_gload(sa, dy, ld_dy, row_begin, row_end, n0, N, tid);
    wg_gload(sb, x, ld_x, row_begin, row_end, k0, K, tid);
  }
  for (int t = 0; t < nslab; ++t) {
    __syncthreads();                                     // every wave is done with the previous slab
    wg_lwrite(smem, sa, tid);
    wg_lwrite(smem + WG_IMG, sb, tid);
    __syncthreads();
    if (t + 1 < nslab) {
      wg_gload(sa, dy, ld_dy, row_begin + (t + 1) * WG_SLAB, row_end, n0, N, tid);
      wg_gload(sb, x, ld_x, row_begin + (t + 1) * WG_SLAB, row_end, k0, K, tid);
    }
#pragma unroll
    for (int ks = 0; ks < WG_SLAB / 16; ++ks) {
      const char* base = smem + ks * 16 * WG_ROW;
      bf16x8 a[2], b[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        a[c] = wg_read_tr(base, offa[c][0], offa[c][1]);
        b[c] = wg_read_tr(base, offb[c][0], offb[c][1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  float* o = out + (size_t)s * split_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = k0 + 64 * wk + 32 * j + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n0 + 64 * wn + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h5;
        if (row < N && col < K) {
          float* p = o + (size_t)row * ld_out + col;
          *p = add ? *p + acc[i][j][r] : acc[i][j][r];
        }
      }
    }
}

// dW[n][k] = (add ? dW[n][k] : 0) + (ws[0][n][k] + ws[1][n][k] + ... ) : the partials first, in ascending s, then the one addition into dW
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int ld_dw, int N, int K, int nsplit, int add) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nk = (size_t)N * K;
  if (i >= nk) return;
  float sum = ws[i];
  for (int s = 1; s < nsplit; ++s) sum += ws[(size_t)s * nk + i];
  const size_t n = i / K, k = i - n * K;
  float* p = dw + n * ld_dw + k;
  *p = add ? *p + sum : sum;
}

bool wg_sizes_ok(int M, int N, int K) { return M >= 1 && N >= 64 && K >= 64 && (N % 64) == 0 && (K % 64) == 0; }

int wg_nsplit(int M, int N, int K, int* chunk_out) {
  const long tiles = (long)cdiv(N, WG_TILE) * cdiv(K, WG_TILE);
  const long slabs = cdiv(M, WG_SLAB);
  long n = (WG_CUS + tiles / 2) / tiles;
  n = n < 1 ? 1 : n;
  n = n > slabs ? slabs : n;
  const int chunk = WG_SLAB * cdiv(cdiv(M, n), WG_SLAB);
  if (chunk_out) *chunk_out = chunk;
  return cdiv(M, chunk);
}

}  // namespace
}  // namespace ucod

extern "C" int ucod_wgrad_bf16_det_nsplit(int M, int N, int K) {
  if (!ucod::wg_sizes_ok(M, N, K)) return 0;
  return ucod::wg_nsplit(M, N, K, nullptr);
}

extern "C" size_t ucod_wgrad_bf16_det_workspace_bytes(int M, int N, int K) {
  if (!ucod::wg_sizes_ok(M, N, K)) return 0;
  const int ns = ucod::wg_nsplit(M, N, K, nullptr);
  return ns == 1 ? 0 : (size_t)ns * N * K * sizeof(float);
}

extern "C" int ucod_wgrad_bf16_det(const void* dy, int ld_dy, const void* x, int ld_x, float* dW, int ld_dw, int M, int N, int K, int accumulate, void* ws,
                                   size_t ws_bytes, void* stream) {
  using namespace ucod;
  if (!dy || !x || !dW || !wg_sizes_ok(M, N, K)) return UCOD_EINVAL;
  if (ld_dy < N || ld_x < K || ld_dw < K) return UCOD_EINVAL;
  if ((ld_dy % 4) || (ld_x % 4) || (((uintptr_t)dy | (uintptr_t)x) & 7) || ((uintptr_t)dW & 3)) return UCOD_EINVAL;      // 8-byte row starts
  int chunk = 0;
  const int ns = wg_nsplit(M, N, K, &chunk);
  const size_t need = ns == 1 ? 0 : (size_t)ns * N * K * sizeof(float);
  if (need && (!ws || ws_bytes < need || ((uintptr_t)ws & 3))) return UCOD_EINVAL;
  const int tiles_k = cdiv(K, WG_TILE);
  const long tiles = (long)cdiv(N, WG_TILE) * tiles_k;
  if (tiles > 0x7fffffffl) return UCOD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int add = accumulate != 0;
  if (ns == 1) {
    hipLaunchKernelGGL(wgrad_tile_kernel, dim3((unsigned)tiles, 1), dim3(256), 0, s, (const bf16_raw*)dy, ld_dy, (const bf16_raw*)x, ld_x, dW, (size_t)0, ld_dw, M, N,
                       K, chunk, tiles_k, add);
  } else {
    hipLaunchKernelGGL(wgrad_tile_kernel, dim3((unsigned)tiles, ns), dim3(256), 0, s, (const bf16_raw*)dy, ld_dy, (const bf16_raw*)x, ld_x, (float*)ws,
                       (size_t)N * K, K, M, N, K, chunk, tiles_k, 0);
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3(cdiv((long)N * K, 256)), dim3(256), 0, s, (const float*)ws, dW, ld_dw, N, K, ns, add);
  }
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
