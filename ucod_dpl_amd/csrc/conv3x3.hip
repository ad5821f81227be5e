// The gradient into the features of the discriminator's feature branch (backbone-backward mode with dis_use_features=True, include/ucod_dpl.h):
//   ucod_conv3x3_f32            3x3 / stride 1 / pad 1 convolution as an implicit GEMM: dba_project_kernel<false> (gemm_f32.hip) with the rows of every
//                               K-tile gathered straight from x instead of read from an unfold buffer.  Same tile (128 output channels x 64 pixels, K-tile
//                               16), same K order (c*9 + ky*3 + kx), same v_mfma_f32_32x32x2_f32 sequence on the same values: bit-identical to
//                               ucod_unfold3x3 + ucod_dba_project(zero bias).  (An accumulator that starts at +0 never becomes -0, so the zero bias that
//                               route adds changes no bit.)
//   ucod_conv3x3_dgrad_weights  W [Cout,Cin,3,3] -> Wd [Cin,Kpad]: kernel flipped on both spatial axes, channel axes exchanged; conv3x3(gy, Wd) is the
//                               data gradient of conv3x3(x, W)
//   ucod_apm_bce_gprob          d(step loss)/d(p_s, p_p): the targets of both BCEWithLogits terms depend on w(p_s, p_p), and `loss -= dis_loss` on p_s
#include "common.h"
#include "../../include/ucod_dpl.h"

namespace ucod {
namespace {

constexpr int CK = 16;    // K-tile (FK of gemm_f32.hip)
constexpr int CLD = 132;  // row length of the [k][row] weight image (LDP of gemm_f32.hip)

// 128 rows x 16 k of the K-contiguous weight matrix -> registers -> [k][row] LDS image: load_kcontig<true> / store_kcontig of gemm_f32.hip (Kpad % 16 == 0
// and the 16-byte alignment of Wmat make every float4 whole)
__device__ __forceinline__ void load_w(const float* __restrict__ Wm, int Kpad, int n0, int Nout, int k0, int tid, float4 (&r)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i, row = idx >> 2, k = k0 + 4 * (idx & 3);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n0 + row < Nout) v = *reinterpret_cast<const float4*>(Wm + (long)(n0 + row) * Kpad + k);
    r[i] = v;
  }
}
__device__ __forceinline__ void store_w(float* lds, int tid, const float4 (&r)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i, row = idx >> 2, k = 4 * (idx & 3);
    lds[(k + 0) * CLD + row] = r[i].x;
    lds[(k + 1) * CLD + row] = r[i].y;
    lds[(k + 2) * CLD + row] = r[i].z;
    lds[(k + 3) * CLD + row] = r[i].w;
  }
}

// block: 128 output channels x 64 pixels of one image; 4 waves, wave w -> channels 32w..32w+31.  Thread tid stages pixel p0 + (tid & 63) of the rows
// (tid >> 6) + 4 i (i < 4) of every K-tile.  Row k of the GEMM is input channel k / 9 shifted by tap k % 9; per THREAD: the pixel's (y, x), its nine
// in-image masks and nothing else; per TILE: (channel, tap) of the thread's four rows advance by 16 = 9 + 7 without a division.
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(const float* __restrict__ x, const float* __restrict__ Wm, float* __restrict__ y, int C, int H,
                                                         int W, int Nout, int Kpad) {
  __shared__ float Ws[2][CK * CLD];
  __shared__ float Xs[2][CK * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  const int p0 = blockIdx.x * 64, n0 = blockIdx.y * 128, b = blockIdx.z;
  const float* xb = x + (long)b * C * HW;

  const int p = p0 + lane;
  const bool live = p < HW;
  const int py = live ? p / W : 0, px = live ? p - py * W : 0;
  unsigned tapmask = 0;                                                     // bit t = ky*3 + kx: the tap's source pixel lies inside the image
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = py + t / 3 - 1, ix = px + t % 3 - 1;
    if (live && iy >= 0 && iy < H && ix >= 0 && ix < W) tapmask |= 1u << t;
  }
  int rc[4], rt[4];                                                         // (channel, tap) of the thread's four rows in the current K-tile
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = wave + 4 * i;                                             // < 16: channel 0 or 1
    rc[i] = k >= 9 ? 1 : 0;
    rt[i] = k >= 9 ? k - 9 : k;
  }

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }

  float4 rw[2];
  float rx[4];
  auto load_x = [&]() {                                                     // the tile (rc, rt) point at; then advance them to the next one
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = rc[i], t = rt[i];
      const int ky = (t * 11) >> 5;                                         // t / 3 for t < 9
      const int off = (ky - 1) * W + (t - 3 * ky - 1);
      const bool ok = ((tapmask >> t) & 1u) != 0 && c < C;                  // rows k >= 9C are zero
      const float v = xb[(long)(c < C ? c : C - 1) * HW + (ok ? p + off : 0)];   // (clamped address + select: no branch around the load)
      rx[i] = ok ? v : 0.f;
      const int t2 = t + 7;                                                 // k += 16
      rt[i] = t2 >= 9 ? t2 - 9 : t2;
      rc[i] = c + (t2 >= 9 ? 2 : 1);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) Xs[buf][(wave + 4 * i) * 64 + lane] = rx[i];
  };

  const int nt = Kpad / CK;
  load_w(Wm, Kpad, n0, Nout, 0, tid, rw);
  load_x();
  store_w(Ws[0], tid, rw);
  store_x(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    const bool more = t + 1 < nt;
    if (more) {
      load_w(Wm, Kpad, n0, Nout, (t + 1) * CK, tid, rw);
      load_x();
    }
    const float* ws = Ws[t & 1];
    const float* xs = Xs[t & 1];
#pragma unroll
    for (int kk = 0; kk < CK; kk += 2) {
      const int k = kk + (lane >> 5);
      const float a = ws[k * CLD + wave * 32 + (lane & 31)];
      const float b0 = xs[k * 64 + (lane & 31)];
      const float b1 = xs[k * 64 + 32 + (lane & 31)];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
    }
    if (more) {
      store_w(Ws[(t + 1) & 1], tid, rw);
      store_x((t + 1) & 1);
    }
  }
  // C/D map of the 32x32 accumulator: col = lane&31 (pixel), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (channel)
  float* yb = y + (long)b * Nout * HW;
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const int q = p0 + pt * 32 + (lane & 31);
    if (q >= HW) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (n < Nout) yb[(long)n * HW + q] = acc[pt][r];
    }
  }
}

__global__ __launch_bounds__(256) void conv3x3_dgrad_weights_kernel(const float* __restrict__ W, float* __restrict__ Wd, int Cout, int Cin, int Kpad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Cin * Kpad) return;
  const int ci = (int)(i / Kpad), k = (int)(i - (long)ci * Kpad);
  float v = 0.f;
  if (k < 9 * Cout) {
    const int co = k / 9, t = k - co * 9;
    v = W[((long)co * Cin + ci) * 9 + (8 - t)];
  }
  Wd[i] = v;
}

// grid (B): one workgroup per image; the HW sum is per-thread strided partials in f64, then block_sum: a fixed order.  Everything behind the sum runs in f64 on
// the f32 inputs (one thread per image: the subtraction p_s - p_p is exact there, and sin(pi |D|) near |D| = 1 keeps its relative accuracy).
__global__ __launch_bounds__(256) void apm_bce_gprob_kernel(const float* __restrict__ pl, const float* __restrict__ teacher, const float* __restrict__ fg,
                                                            const float* __restrict__ bg, const float* __restrict__ p_s, const float* __restrict__ p_p,
                                                            float epoch_frac, float gscale, int finetune, float* __restrict__ gp_s,
                                                            float* __restrict__ gp_p, int B, int HW) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  double s = 0.0;
  for (int p = threadIdx.x; p < HW; p += 256) {
    const long i = (long)b * HW + p;
    const float tb = sigmoid_acc(teacher[i]) > 0.5f ? 1.f : 0.f;            // binarised exactly as apm_bce_kernel does
    s += (double)((bg[i] - fg[i]) * (tb - pl[i]));
  }
  s = block_sum(s, red);
  if (threadIdx.x != 0) return;
  const double pi = 3.14159265358979323846;
  const double ps = p_s[b], pp = p_p[b];
  const double d = ps - pp, ad = fabs(d);
  const double u = 0.5 * (1.0 + cos(pi * ad)) + (double)epoch_frac;
  const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  const double dwd = (u >= 0.0 && u <= 1.0) ? -0.5 * pi * sin(pi * ad) * sgn : 0.0;
  const double gw = s / ((double)B * (double)HW);
  const double tgt = (double)gscale * gw * dwd;
  double dis = 0.0;
  if (!finetune) dis = (double)gscale * (ps / fmax(ps * (1.0 - ps), (double)1e-12f)) / (double)B;   // torch's BCELoss backward at target 0 (ucod_disc_bce; its floor is an f32 constant)
  gp_p[b] = (float)(-tgt);
  gp_s[b] = (float)(tgt - dis);
}

}  // namespace
}  // namespace ucod

using namespace ucod;

extern "C" int ucod_conv3x3_f32(const float* x, const float* Wmat, float* y, int B, int C, int H, int W, int Nout, int Kpad, void* stream) {
  if (!x || !Wmat || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0 || Nout <= 0 || Kpad <= 0 || (Kpad % CK) != 0 || (long)Kpad < 9L * C ||
      (((uintptr_t)Wmat) % 16) != 0)
    return UCOD_EINVAL;
  if ((long)H * W > 0x7fffffffL / 2 || B > 65535 || cdiv(Nout, 128) > 65535) return UCOD_EINVAL;     // (grid limits; pixel indices stay in int)
  dim3 grid(cdiv((long)H * W, 64), cdiv(Nout, 128), B), block(256);
  UCOD_PROF(PROF_DBA_PROJECT, stream);
  hipLaunchKernelGGL(conv3x3_kernel, grid, block, 0, (hipStream_t)stream, x, Wmat, y, C, H, W, Nout, Kpad);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_conv3x3_dgrad_weights(const float* W, float* Wd, int Cout, int Cin, int Kpad, void* stream) {
  if (!W || !Wd || Cout <= 0 || Cin <= 0 || Kpad <= 0 || (Kpad % CK) != 0 || (long)Kpad < 9L * Cout) return UCOD_EINVAL;
  hipLaunchKernelGGL(conv3x3_dgrad_weights_kernel, dim3(cdiv((long)Cin * Kpad, 256)), dim3(256), 0, (hipStream_t)stream, W, Wd, Cout, Cin, Kpad);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

extern "C" int ucod_apm_bce_gprob(const float* pl, const float* teacher, const float* fg, const float* bg, const float* p_s, const float* p_p, float epoch_frac,
                                  float gscale, int finetune, float* gp_s, float* gp_p, int B, int HW, void* stream) {
  if (!pl || !teacher || !fg || !bg || !p_s || !p_p || !gp_s || !gp_p || B <= 0 || HW <= 0) return UCOD_EINVAL;
  UCOD_PROF(PROF_APM, stream);
  hipLaunchKernelGGL(apm_bce_gprob_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pl, teacher, fg, bg, p_s, p_p, epoch_frac, gscale, finetune, gp_s, gp_p, B, HW);
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}
