// The way out of backbone-backward (LoRA) mode: peft's merge  W <- W + (alpha / r) B A  (models/modules/full_model.py:47-72 configures the modules; peft's
// merge_and_unload applies this formula to each of them) as one pass over the weight, and the device form of the LayerNorm fold (fold.py) that turns a merged f32
// weight into the folded fp16 operands of ucod_gemm_lnfold.  Both are row kernels, one wave per output row, bound by the weight's own bytes:
//   ucod_lora_merge_f32   out[n][k] = f32( f64(w0[n][k]) + f64(scaling) * sum_{j < r, ascending} f64(B[n][j]) * f64(A[j][k]) )
//   ucod_fold_ln_linear   wf = half( f32( (f64(w) f64(gamma[k])) f64(q[n]) ) ),  colsum[n] = f32( sum_k f64(wf) ),  bias_f[n] = f32( (sum_k f64(w) f64(beta[k]) + f64(b[n])) f64(q[n]) )
// f64 on purpose: a product of two f32 values is exact there, so the sums do not depend on whether the compiler forms an FMA, and the results can be pinned bit for
// bit against a host restatement.  The one place where an FMA would change a bit -- w0 + scaling * sum -- is kept as a multiply and an add (rounded_product: the
// build's -ffp-contract=fast fuses across statements and disregards the contract pragma).
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {

// a * b rounded to f64, opaque to the optimiser so that a following add cannot absorb it into an FMA
__device__ __forceinline__ double rounded_product(double a, double b) {
  double p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// One wave per output row, four rows per block; a lane owns 4 consecutive columns of every 256-column step (16-byte loads and stores along K).  The row's B values
// are read at one address by the whole wave and the A rows of the lane's columns come from L2 (r K f32 values, <= 129 KB at r = 21, K = 1536); nothing is indexed
// dynamically in registers, so no scratch.  K % 64 == 0 makes every 4-column group whole; the step's tail (K % 256 != 0) and the last block's rows are guarded.
__global__ __launch_bounds__(256) void lora_merge_f32_kernel(const float* __restrict__ w0, const float* __restrict__ A, const float* __restrict__ B, int r,
                                                             float scaling, float* __restrict__ out, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* brow = B + (size_t)n * r;
  const double s = (double)scaling;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 w = *reinterpret_cast<const float4*>(w0 + (size_t)n * K + k);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int j = 0; j < r; ++j) {
      const double b = (double)brow[j];
      const float4 a = *reinterpret_cast<const float4*>(A + (size_t)j * K + k);
      a0 += b * (double)a.x;
      a1 += b * (double)a.y;
      a2 += b * (double)a.z;
      a3 += b * (double)a.w;
    }
    float4 o;
    o.x = (float)((double)w.x + rounded_product(s, a0));
    o.y = (float)((double)w.y + rounded_product(s, a1));
    o.z = (float)((double)w.z + rounded_product(s, a2));
    o.w = (float)((double)w.w + rounded_product(s, a3));
    *reinterpret_cast<float4*>(out + (size_t)n * K + k) = o;
  }
}

#ifdef UCOD_HALF_F16
// One wave per row: the folded fp16 row (8-byte stores), and the row's two f64 sums reduced by shuffles.  The column sum is of the ROUNDED values (fold.py).
__global__ __launch_bounds__(256) void fold_ln_linear_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ b, const float* __restrict__ row_scale, half_t* __restrict__ wf,
                                                             float* __restrict__ bias_f, float* __restrict__ colsum, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const double q = row_scale ? (double)row_scale[n] : 1.0;
  double cs = 0.0, bs = 0.0;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 wv = *reinterpret_cast<const float4*>(w + (size_t)n * K + k);
    const float4 g = *reinterpret_cast<const float4*>(gamma + k);
    const float4 be = *reinterpret_cast<const float4*>(beta + k);
    const float we[4] = {wv.x, wv.y, wv.z, wv.w}, ge[4] = {g.x, g.y, g.z, g.w}, bee[4] = {be.x, be.y, be.z, be.w};
    hx4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float f = (float)(((double)we[e] * (double)ge[e]) * q);            // both roundings, in the host's order: f64 -> f32 -> fp16 ...
      asm volatile("" : "+v"(f));                                        // ... (the compiler otherwise folds the two conversions into ONE f64 -> fp16 rounding)
      h[e] = (half_t)f;
      cs += (double)h[e];
      bs += (double)we[e] * (double)bee[e];
    }
    *reinterpret_cast<hx4*>(wf + (size_t)n * K + k) = h;
  }
  cs = wave_sum_d(cs);
  bs = wave_sum_d(bs);
  if (lane == 0) {
    colsum[n] = (float)cs;
    bias_f[n] = (float)((bs + (double)b[n]) * q);
  }
}
#endif

}  // namespace ucod

extern "C" int ucod_lora_merge_f32(const float* w0, const float* A, const float* B, int r, float scaling, float* out, int N, int K, void* stream) {
  using namespace ucod;
  if (!w0 || !A || !B || !out || r < 1 || r > UCOD_LORA_AUG / 3 || N < 1 || K < 64 || (K % 64) != 0) return UCOD_EINVAL;
  if ((((uintptr_t)w0 | (uintptr_t)A | (uintptr_t)out) & 15) != 0 || ((uintptr_t)B & 3) != 0) return UCOD_EINVAL;      // (16-byte accesses along K)
  UCOD_PROF(PROF_LORA, stream);
  hipLaunchKernelGGL(lora_merge_f32_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, w0, A, B, r, scaling, out, N, K);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_fold_ln_linear(const float* w, const float* gamma, const float* beta, const float* b, const float* row_scale_or_null, void* wf,
                                   float* bias_f, float* colsum, int N, int K, void* stream) {
#ifdef UCOD_HALF_F16
  using namespace ucod;
  if (!w || !gamma || !beta || !b || !wf || !bias_f || !colsum || N < 1 || K < 64 || (K % 64) != 0) return UCOD_EINVAL;
  if ((((uintptr_t)w | (uintptr_t)gamma | (uintptr_t)beta) & 15) != 0 || ((uintptr_t)wf & 7) != 0) return UCOD_EINVAL;  // (16-byte loads, 8-byte stores along K)
  UCOD_PROF(PROF_CAST, stream);
  hipLaunchKernelGGL(fold_ln_linear_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, w, gamma, beta, b, row_scale_or_null, (half_t*)wf, bias_f,
                     colsum, N, K);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
#else
  return UCOD_EINVAL;                                          // the fold exists in the fp16-operand build only (ucod_gemm_lnfold)
#endif
}
