// Cross-attention backward, head_dim 96 (CORAL refiner: the nn.MultiheadAttention of models/modules/mlp.py:122,143 differentiated;
// 8 heads on C = 768, dropout 0, no mask).  The formulas are those of attention_bwd.hip with hd = 96 and separate query / key counts:
// with Q' = Q * 96^-0.5 * log2(e) (what the q projection's epilogue stored), L = base-2 log-sum-exp of the scaled scores,
//     P = exp2(Q'K^T - L)    dP = dO V^T    delta = rowsum(dO * O)    dS = P * (dP - delta)
//     dQ = 96^-0.5 * dS K    dK = ln(2) * dS^T Q'    dV = P^T dO                 (gradients of the UNSCALED projections)
// Plain HIP in the style of attn_cross96_kernel (attention.hip): v_mfma_f32_32x32x16_bf16, a lane owns one column of every 32x32 tile,
// the C registers are rounded to bf16 in place and reused as the B operand of the next product; LDS rows are padded to 256 B (16 slots
// of 16 B, 12 used): row-major reads use slot = chunk ^ (row & 15), ds_read_b64_tr_b16 reads use slot = chunk ^ ((row & 3) << 2).  A tile
// that is needed both ways is staged twice.  One LDS stage, two barriers per tile, the next tile's global loads in flight under the MFMAs.
// Two kernels, no atomics, every sum in a fixed order (two runs are bit-identical):
//   attn96_bwd_dq_kernel   a wave owns 32 QUERIES (lane = query) and walks the key tiles; L and delta are per-lane scalars that
//                          initialise the S^T / dP^T accumulators; also writes delta for the second kernel;
//   attn96_bwd_dkv_kernel  a wave owns 32 KEYS (lane = key) and walks the query tiles; L[q] and delta[q] vary along the accumulator
//                          ROWS there, so they ride in an unused 16-byte slot of the row-major Q' tile.
// bf16 in both libraries (the fp16-operand build trains nothing): explicit bf16 types, as attention_bwd.hip.
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace {

constexpr int HDX = 96;
constexpr int WT = 128;                 // rows (queries or keys) owned by one workgroup: 4 waves x 32
constexpr int ST = 64;                  // rows per streamed tile
constexpr int XROW = 256;               // padded LDS row bytes
constexpr int XTILE = ST * XROW;        // 16 KiB
constexpr int CHUNKS = HDX / 8;         // 12 16-byte chunks per row
constexpr int AUX_CHUNK = 12;           // the slot of the row-major Q' tile that carries (L, delta) of the row

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

__device__ __forceinline__ f32x16 mfma96(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// C registers 8*ks .. 8*ks+7 of a 32x32 tile -> bf16 B operand of the next product (k index = the C row permutation)
__device__ __forceinline__ bf16x8 pack_b(const f32x16& s, int ks) {
  u32x4_t w;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) w[jj] = pack_bf16x2(s[8 * ks + 2 * jj], s[8 * ks + 2 * jj + 1]);
  return __builtin_bit_cast(bf16x8, w);
}

// A operand X^T[32 d of block dt][16 tile rows of block (kt, ks) in the C row permutation] from a transpose-staged tile
__device__ __forceinline__ bf16x8 read_tr(const char* tile, int off) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(tile + off));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(tile + off + 8 * XROW));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// one streamed tile in flight: 64 rows x 12 chunks = 768 chunks, 3 per thread; rows past the end re-read the last row (masked later)
struct Stage { u32x4 r[3]; };
__device__ __forceinline__ void gload(Stage& s, const bf16_raw* base, int ld, int row0, int nrows, int tid) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int idx = tid + 256 * i, row = idx / CHUNKS, ch = idx - row * CHUNKS;
    int r = row0 + row;
    r = r < nrows ? r : nrows - 1;
    s.r[i] = *reinterpret_cast<const u32x4*>(base + (size_t)r * ld + ch * 8);
  }
}
__device__ __forceinline__ void lwrite_row(char* tile, const Stage& s, int tid) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int idx = tid + 256 * i, row = idx / CHUNKS, ch = idx - row * CHUNKS;
    *reinterpret_cast<u32x4*>(tile + row * XROW + (ch ^ (row & 15)) * 16) = s.r[i];
  }
}
__device__ __forceinline__ void lwrite_tr(char* tile, const Stage& s, int tid) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int idx = tid + 256 * i, row = idx / CHUNKS, ch = idx - row * CHUNKS;
    *reinterpret_cast<u32x4*>(tile + row * XROW + (ch ^ ((row & 3) << 2)) * 16) = s.r[i];
  }
}

// byte offsets of a lane's fragments inside a tile (the forward's koff / voff).  Both swizzles depend on the low bits of the tile row only, which
// the 32-row block kt and the 16-row block ks do not touch: their part of the offset is a compile-time constant (the instruction's immediate).
struct Offs {
  int row[6];         // row-major A operand: tile row l31 (+ 32 kt), columns 16*sd + 8*h5 .. +7
  int tr[3];          // transposed A operand of block (kt, ks) = (0, 0), output columns of block dt
};
__device__ __forceinline__ void make_offs(Offs& o, int lane) {
  const int h5 = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int sd = 0; sd < 6; ++sd) o.row[sd] = l31 * XROW + ((2 * sd + h5) ^ (l31 & 15)) * 16;
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int row = 4 * h5 + (i16 >> 2);
    const int dst = dt * 32 + g1 * 16 + 4 * (i16 & 3);
    o.tr[dt] = row * XROW + ((dst >> 3) ^ ((row & 3) << 2)) * 16 + (dst & 7) * 2;   // row + 8: same (row & 3) -> + 8 * XROW
  }
}
__device__ __forceinline__ constexpr int blk_row(int kt) { return kt * 32 * XROW; }
__device__ __forceinline__ constexpr int blk_tr(int kt, int ks) { return (kt * 32 + ks * 16) * XROW; }

// the wave's own 32 rows as B operands: lane (row l31, half h5) holds X[row][16 s + 8 h5 .. +7]
__device__ __forceinline__ void load_frags(bf16x8 (&f)[6], const bf16_raw* base, int ld, int row, int h5) {
  const bf16_raw* p = base + (size_t)row * ld + 8 * h5;
#pragma unroll
  for (int s = 0; s < 6; ++s) f[s] = *reinterpret_cast<const bf16x8*>(p + 16 * s);
}

// C^T accumulators (rows = 96 head columns in three blocks, column = the lane's row) -> bf16 row of length 96, scaled
__device__ __forceinline__ void store_row96(const f32x16 (&acc)[3], float scale, bf16_raw* p /* row start + 4 * h5 */) {
#pragma unroll
  for (int dt = 0; dt < 3; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 w;
      w[0] = pack_bf16x2(acc[dt][4 * g + 0] * scale, acc[dt][4 * g + 1] * scale);
      w[1] = pack_bf16x2(acc[dt][4 * g + 2] * scale, acc[dt][4 * g + 3] * scale);
      *reinterpret_cast<u32x2*>(p + dt * 32 + 8 * g) = w;
    }
}

__global__ __launch_bounds__(256, 2) void attn96_bwd_dq_kernel(const bf16_raw* __restrict__ qp, int ldq, const bf16_raw* __restrict__ kp,
                                                                const bf16_raw* __restrict__ vp, int ldkv, const bf16_raw* __restrict__ op,
                                                                const bf16_raw* __restrict__ dop, const float* __restrict__ lse,
                                                                float* __restrict__ delta, bf16_raw* __restrict__ dq, int lddq, int Nq, int Nk,
                                                                int heads) {
  __shared__ __attribute__((aligned(16))) char smem[3 * XTILE];      // K row-major | K transpose-staged | V row-major
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h5 = lane >> 5, l31 = lane & 31;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = heads * HDX;
  const int q = blockIdx.x * WT + wave * 32 + l31;
  const int qr = q < Nq ? q : Nq - 1;
  const bf16_raw* kbase = kp + (size_t)b * Nk * ldkv + head * HDX;
  const bf16_raw* vbase = vp + (size_t)b * Nk * ldkv + head * HDX;

  bf16x8 qf[6], dof[6];
  load_frags(qf, qp + (size_t)b * Nq * ldq + head * HDX, ldq, qr, h5);
  load_frags(dof, dop + (size_t)b * Nq * D + head * HDX, D, qr, h5);
  float dl;
  {
    bf16x8 of[6];
    load_frags(of, op + (size_t)b * Nq * D + head * HDX, D, qr, h5);
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) part = fmaf((float)dof[s][j], (float)of[s][j], part);
    dl = part + __shfl_xor(part, 32, 64);
  }
  const size_t stat = ((size_t)b * heads + head) * Nq + qr;
  const float L = lse[stat];
  if (h5 == 0 && q < Nq) delta[stat] = dl;

  Offs off;
  make_offs(off, lane);
  f32x16 acc[3];
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; acc[2][i] = 0.f; }

  const int nt = (Nk + ST - 1) / ST;
  Stage sk, sv;
  gload(sk, kbase, ldkv, 0, Nk, tid);
  gload(sv, vbase, ldkv, 0, Nk, tid);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();                                     // every wave is done with the previous tile
    lwrite_row(smem, sk, tid);
    lwrite_tr(smem + XTILE, sk, tid);
    lwrite_row(smem + 2 * XTILE, sv, tid);
    __syncthreads();
    if (t + 1 < nt) {
      gload(sk, kbase, ldkv, (t + 1) * ST, Nk, tid);
      gload(sv, vbase, ldkv, (t + 1) * ST, Nk, tid);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 s, dp;                                      // S^T - L and dP^T - delta: rows = keys, column = the lane's query
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = -L; dp[i] = -dl; }
#pragma unroll
      for (int sd = 0; sd < 6; ++sd) {
        s = mfma96(*reinterpret_cast<const bf16x8*>(smem + blk_row(kt) + off.row[sd]), qf[sd], s);
        dp = mfma96(*reinterpret_cast<const bf16x8*>(smem + 2 * XTILE + blk_row(kt) + off.row[sd]), dof[sd], dp);
      }
      const int key0 = t * ST + kt * 32 + 4 * h5;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = key0 + (r & 3) + 8 * (r >> 2);
        const float p = key < Nk ? __builtin_amdgcn_exp2f(s[r]) : 0.f;
        dp[r] *= p;                                      // dS^T
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 dsb = pack_b(dp, ks);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) acc[dt] = mfma96(read_tr(smem + XTILE + blk_tr(kt, ks), off.tr[dt]), dsb, acc[dt]);
      }
    }
  }
  if (q < Nq) store_row96(acc, 0.10206207261596575f /* 96^-0.5 */, dq + ((size_t)b * Nq + q) * lddq + head * HDX + 4 * h5);
}

__global__ __launch_bounds__(256, 2) void attn96_bwd_dkv_kernel(const bf16_raw* __restrict__ qp, int ldq, const bf16_raw* __restrict__ kp,
                                                                 const bf16_raw* __restrict__ vp, int ldkv, const bf16_raw* __restrict__ dop,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_raw* __restrict__ dk, bf16_raw* __restrict__ dv, int lddkv, int Nq, int Nk,
                                                                 int heads) {
  __shared__ __attribute__((aligned(16))) char smem[4 * XTILE];      // Q' row-major (+ L, delta) | Q' transpose-staged | dO row-major | dO transpose-staged
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h5 = lane >> 5, l31 = lane & 31;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = heads * HDX;
  const int key = blockIdx.x * WT + wave * 32 + l31;
  const int kr = key < Nk ? key : Nk - 1;
  const bf16_raw* qbase = qp + (size_t)b * Nq * ldq + head * HDX;
  const bf16_raw* dobase = dop + (size_t)b * Nq * D + head * HDX;
  const float* lrow = lse + ((size_t)b * heads + head) * Nq;
  const float* drow = delta + ((size_t)b * heads + head) * Nq;

  bf16x8 kf[6], vf[6];
  load_frags(kf, kp + (size_t)b * Nk * ldkv + head * HDX, ldkv, kr, h5);
  load_frags(vf, vp + (size_t)b * Nk * ldkv + head * HDX, ldkv, kr, h5);

  Offs off;
  make_offs(off, lane);
  f32x16 dka[3], dva[3];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dka[0][i] = 0.f; dka[1][i] = 0.f; dka[2][i] = 0.f; dva[0][i] = 0.f; dva[1][i] = 0.f; dva[2][i] = 0.f; }

  const int nt = (Nq + ST - 1) / ST;
  Stage sq, sd_;
  float2 aux = make_float2(0.f, 0.f);
  auto gload_aux = [&](int t) {
    if (tid < ST) {
      int r = t * ST + tid;
      r = r < Nq ? r : Nq - 1;
      aux = make_float2(lrow[r], drow[r]);
    }
  };
  gload(sq, qbase, ldq, 0, Nq, tid);
  gload(sd_, dobase, D, 0, Nq, tid);
  gload_aux(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    lwrite_row(smem, sq, tid);
    lwrite_tr(smem + XTILE, sq, tid);
    lwrite_row(smem + 2 * XTILE, sd_, tid);
    lwrite_tr(smem + 3 * XTILE, sd_, tid);
    if (tid < ST) *reinterpret_cast<float2*>(smem + tid * XROW + (AUX_CHUNK ^ (tid & 15)) * 16) = aux;
    __syncthreads();
    if (t + 1 < nt) {
      gload(sq, qbase, ldq, (t + 1) * ST, Nq, tid);
      gload(sd_, dobase, D, (t + 1) * ST, Nq, tid);
      gload_aux(t + 1);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 s, dp;                                      // S - L and dP - delta: rows = queries, column = the lane's key
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cr = (r & 3) + 8 * ((r >> 2) & 1);       // the accumulator row's low four bits are cr | 4 h5
        const float2 a = *reinterpret_cast<const float2*>(smem + (kt * 32 + (r & 3) + 8 * (r >> 2)) * XROW + h5 * (4 * XROW) + (((AUX_CHUNK ^ cr) * 16) ^ (h5 * 64)));
        s[r] = -a.x;
        dp[r] = -a.y;
      }
#pragma unroll
      for (int sd = 0; sd < 6; ++sd) {
        s = mfma96(*reinterpret_cast<const bf16x8*>(smem + blk_row(kt) + off.row[sd]), kf[sd], s);
        dp = mfma96(*reinterpret_cast<const bf16x8*>(smem + 2 * XTILE + blk_row(kt) + off.row[sd]), vf[sd], dp);
      }
      const int q0 = t * ST + kt * 32 + 4 * h5;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = q0 + (r & 3) + 8 * (r >> 2);
        const float p = q < Nq ? __builtin_amdgcn_exp2f(s[r]) : 0.f;
        s[r] = p;                                        // P
        dp[r] *= p;                                      // dS
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pb = pack_b(s, ks), dsb = pack_b(dp, ks);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          dva[dt] = mfma96(read_tr(smem + 3 * XTILE + blk_tr(kt, ks), off.tr[dt]), pb, dva[dt]);
          dka[dt] = mfma96(read_tr(smem + XTILE + blk_tr(kt, ks), off.tr[dt]), dsb, dka[dt]);
        }
      }
    }
  }
  if (key < Nk) {
    const size_t o = ((size_t)b * Nk + key) * lddkv + head * HDX + 4 * h5;
    store_row96(dka, 0.6931471805599453f /* ln 2 */, dk + o);
    store_row96(dva, 1.0f, dv + o);
  }
}

}  // namespace
}  // namespace ucod

extern "C" int ucod_cross_attention96_bwd(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* out, const void* dout,
                                          const float* lse, float* delta, void* dq, int lddq, void* dk, void* dv, int lddkv, int B, int Nq, int Nk,
                                          int heads, void* stream) {
  using namespace ucod;
  if (!q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv || B <= 0 || Nq <= 0 || Nk <= 0 || heads <= 0) return UCOD_EINVAL;
  const long D = (long)heads * HDX;
  if ((ldq % 8) || (ldkv % 8) || (lddq % 8) || (lddkv % 8) || ldq < D || ldkv < D || lddq < D || lddkv < D) return UCOD_EINVAL;
  const uintptr_t al = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv;
  if (al & 15) return UCOD_EINVAL;
  if (heads > 65535 || B > 65535 || (long)B * heads * Nq >= (1l << 31)) return UCOD_EINVAL;      // grid limits; the statistics' index
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(attn96_bwd_dq_kernel, dim3(cdiv(Nq, WT), heads, B), dim3(256), 0, s, (const bf16_raw*)q, ldq, (const bf16_raw*)k, (const bf16_raw*)v, ldkv,
                     (const bf16_raw*)out, (const bf16_raw*)dout, lse, delta, (bf16_raw*)dq, lddq, Nq, Nk, heads);
  hipLaunchKernelGGL(attn96_bwd_dkv_kernel, dim3(cdiv(Nk, WT), heads, B), dim3(256), 0, s, (const bf16_raw*)q, ldq, (const bf16_raw*)k, (const bf16_raw*)v, ldkv,
                     (const bf16_raw*)dout, lse, delta, (bf16_raw*)dk, (bf16_raw*)dv, lddkv, Nq, Nk, heads);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
