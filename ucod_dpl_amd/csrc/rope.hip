// Rotary position embedding of DINOv3 (transformers modeling_dinov3_vit.py: apply_rotary_pos_emb / rotate_half) on the Q and K thirds of the patch rows of a QKV
// buffer [B tok, 3 D], in place (include/ucod_dpl.h: ucod_rope_qk).  One kernel serves every frozen-backbone pass because the map is linear: the 16-bit engines
// run it on the QKV GEMM's 16-bit output (the softmax pre-scale already sits in the Q rows), the split passes on the f32 output in front of their split kernels
// (a power-of-two operand scale passes through exactly).
//
// A row kernel, HBM-bound: a lane owns 8 contiguous columns of a head's first half and their partners 32 columns on -- 16-byte loads and stores (two each per half
// for f32) -- and the matching 8 cosines and 8 sines of the token's table row (f32 [n, 64] = cos[0:32] | sin[0:32]; 256 KB at n = 1024: it lives in L2).  Four
// lanes cover a head, 8 * heads lanes the Q and K thirds of a token row; the V third, the CLS row and the register rows are never addressed.  No LDS; the
// grid is capped and grid-strided.
//
// ucod_rope_qk_ld is the same kernel with a row pitch and a direction, for backbone-backward mode: the transpose (the table with the sine negated) takes the
// cotangents dq / dk of the rotated operands, in the first 3 D columns of dqkv_aug [B tok, 3 D + 64], back to those of the projection outputs.  The direction is a
// template parameter: the forward instantiations compute exactly what they did.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace {

constexpr int ROPE_BLOCK = 256;
constexpr int ROPE_MAX_BLOCKS = 2048;                              // 8 blocks of 4 waves per CU on 256 CUs: every SIMD holds its 8 waves

struct Rot8 { float lo[8], hi[8]; };

// out_lo = lo cos - hi sin, out_hi = hi cos + lo sin (f32; the products of the second term are rounded, the sum is one fma); INV: the transpose, sin -> -sin
template <bool INV>
__device__ __forceinline__ void rotate8(Rot8& v, const float* __restrict__ cs) {
  const f32x4 c0 = *(const f32x4*)cs, c1 = *(const f32x4*)(cs + 4), s0 = *(const f32x4*)(cs + 32), s1 = *(const f32x4*)(cs + 36);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float c = e < 4 ? c0[e] : c1[e - 4], s0e = e < 4 ? s0[e] : s1[e - 4], s = INV ? -s0e : s0e;
    const float a = v.lo[e], b = v.hi[e];
    v.lo[e] = a * c - b * s;
    v.hi[e] = b * c + a * s;
  }
}

template <bool F32, bool INV>
__global__ __launch_bounds__(ROPE_BLOCK) void rope_qk_kernel(void* __restrict__ qkv, const float* __restrict__ cos_sin, unsigned items, int tok, int n_reg, int np, int heads,
                                                             int ld_) {
  const unsigned per_row = 8u * heads;                             // lanes per token row: (Q | K) x heads x 4 column groups of 8
  const size_t ld = (size_t)ld_;                                   // row pitch in elements, >= 3 D: columns at or beyond 2 D are never addressed
  // (items < 2^31 and the stride <= 2^19: the 32-bit index cannot wrap)
  for (unsigned i = blockIdx.x * ROPE_BLOCK + threadIdx.x; i < items; i += gridDim.x * ROPE_BLOCK) {
    const unsigned row = i / per_row, within = i - row * per_row;
    const unsigned b = row / (unsigned)np, p = row - b * (unsigned)np;
    // column of the first half: (within >> 2) walks the 2 * heads heads of the Q third and then the K third, which are contiguous
    const size_t at = ((size_t)b * tok + 1 + n_reg + p) * ld + (within >> 2) * 64 + (within & 3) * 8;
    const float* cs = cos_sin + (size_t)p * 64 + (within & 3) * 8;
    Rot8 v;
    if constexpr (F32) {
      float* q = (float*)qkv + at;
      const f32x4 l0 = *(const f32x4*)q, l1 = *(const f32x4*)(q + 4), h0 = *(const f32x4*)(q + 32), h1 = *(const f32x4*)(q + 36);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v.lo[e] = l0[e]; v.lo[4 + e] = l1[e]; v.hi[e] = h0[e]; v.hi[4 + e] = h1[e]; }
      rotate8<INV>(v, cs);
      *(f32x4*)q = (f32x4){v.lo[0], v.lo[1], v.lo[2], v.lo[3]};
      *(f32x4*)(q + 4) = (f32x4){v.lo[4], v.lo[5], v.lo[6], v.lo[7]};
      *(f32x4*)(q + 32) = (f32x4){v.hi[0], v.hi[1], v.hi[2], v.hi[3]};
      *(f32x4*)(q + 36) = (f32x4){v.hi[4], v.hi[5], v.hi[6], v.hi[7]};
    } else {
      h_raw* q = (h_raw*)qkv + at;
      const u32x4 l = *(const u32x4*)q, h = *(const u32x4*)(q + 32);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ucod::unpack_h2(l[e], v.lo[2 * e], v.lo[2 * e + 1]);
        ucod::unpack_h2(h[e], v.hi[2 * e], v.hi[2 * e + 1]);
      }
      rotate8<INV>(v, cs);
      u32x4 ol, oh;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ol[e] = ucod::pack_h2(v.lo[2 * e], v.lo[2 * e + 1]);
        oh[e] = ucod::pack_h2(v.hi[2 * e], v.hi[2 * e + 1]);
      }
      *(u32x4*)q = ol;
      *(u32x4*)(q + 32) = oh;
    }
  }
}

}  // namespace

extern "C" int ucod_rope_qk_ld(void* buf, int elem, const float* cos_sin, int B, int tok, int n_reg, int heads, int ld, int inverse, void* stream) {
  if (!buf || !cos_sin || (elem != UCOD_ROPE_ELEM_HALF && elem != UCOD_ROPE_ELEM_F32) || B <= 0 || tok <= 0 || heads <= 0 || n_reg < 0 || n_reg >= tok - 1) return UCOD_EINVAL;
  if (inverse != 0 && inverse != 1) return UCOD_EINVAL;
  if (heads > 0x7FFFFFFF / 192 || ld < 192 * heads) return UCOD_EINVAL;                                    // ld >= 3 D
  if (((size_t)ld * (elem == UCOD_ROPE_ELEM_F32 ? 4 : 2)) & 15) return UCOD_EINVAL;                          // every row starts on a 16-byte boundary
  if ((((uintptr_t)buf) | ((uintptr_t)cos_sin)) & 15) return UCOD_EINVAL;      // 16-byte loads and stores
  const int np = tok - 1 - n_reg;
  const long items = (long)B * np * heads * 8;
  if (items > 0x7FFFFFFFL) return UCOD_EINVAL;                     // (the kernel's lane index is 32 bits; element offsets are 64)
  const long blocks = (items + ROPE_BLOCK - 1) / ROPE_BLOCK;
  const dim3 grid((unsigned)(blocks < ROPE_MAX_BLOCKS ? blocks : ROPE_MAX_BLOCKS)), block(ROPE_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const unsigned n = (unsigned)items;
  if (elem == UCOD_ROPE_ELEM_F32) {
    if (inverse) hipLaunchKernelGGL((rope_qk_kernel<true, true>), grid, block, 0, s, buf, cos_sin, n, tok, n_reg, np, heads, ld);
    else hipLaunchKernelGGL((rope_qk_kernel<true, false>), grid, block, 0, s, buf, cos_sin, n, tok, n_reg, np, heads, ld);
  } else {
    if (inverse) hipLaunchKernelGGL((rope_qk_kernel<false, true>), grid, block, 0, s, buf, cos_sin, n, tok, n_reg, np, heads, ld);
    else hipLaunchKernelGGL((rope_qk_kernel<false, false>), grid, block, 0, s, buf, cos_sin, n, tok, n_reg, np, heads, ld);
  }
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_rope_qk(void* qkv, int elem, const float* cos_sin, int B, int tok, int n_reg, int heads, void* stream) {
  if (heads <= 0 || heads > 0x7FFFFFFF / 192) return UCOD_EINVAL;
  return ucod_rope_qk_ld(qkv, elem, cos_sin, B, tok, n_reg, heads, 192 * heads, 0, stream);      // ld = 3 D (a multiple of 16 bytes in either type), forward direction
}
