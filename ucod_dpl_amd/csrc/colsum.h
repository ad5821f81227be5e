// What the deterministic column sums share (csrc/colsum.hip: ucod_colsum_det, ucod_colsum_det_tok; csrc/vit_train.hip: ucod_colsum_det_lora): the shape of a
// workgroup, the slab rule and the second launch.  One definition, so that "the bits of ucod_colsum_det" is a property of the source and not of two files kept in
// step by hand.
#pragma once
#include "common.h"

namespace ucod {

constexpr int CS_THREADS = 256;
constexpr int CS_CV = 16;                 // 16-byte column vectors per workgroup
constexpr int CS_RT = CS_THREADS / CS_CV; // row threads per column vector
constexpr int CS_SLAB_ROWS = 64;          // rows per slab while there are fewer than CS_MAX_SLABS of them
constexpr int CS_MAX_SLABS = 128;         // (the finishing thread walks them one after the other)

static inline int colsum_slabs(int M) {
  const long s = ((long)M + CS_SLAB_ROWS - 1) / CS_SLAB_ROWS;
  return (int)(s < CS_MAX_SLABS ? s : CS_MAX_SLABS);
}

// one thread per column: part[0][n] + part[1][n] + ... ascending, times col_scale[n] (NULL: ones), stored
static __global__ __launch_bounds__(CS_THREADS) void colsum_finish_kernel(const float* __restrict__ part, const float* __restrict__ col_scale, float* __restrict__ out,
                                                                          int N, int slabs) {
  const int n = blockIdx.x * CS_THREADS + threadIdx.x;
  if (n >= N) return;
  float s = part[n];
#pragma unroll 16
  for (int q = 1; q < slabs; ++q) s += part[(size_t)q * N + n];
  out[n] = col_scale ? col_scale[n] * s : s;
}

}  // namespace ucod
