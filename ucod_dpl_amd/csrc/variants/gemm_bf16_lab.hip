// LABORATORY FILE -- not part of the product library.  Built only by `make -C ucod_dpl_amd/csrc variants` into
// ../_native/libucod_dpl_variants.so (entry: ucod_gemm_bf16_lab), loaded only by tools/ and by tests marked `variants`.
// Forms of the large-tile bf16 GEMM measured in rounds 1-2 and not adopted, kept runnable for A/B runs against
// the product kernels of ../gemm_bf16.hip:
//   3 / 4   256 x 256 / 256 x 192, four barrier intervals per K-tile, wave groups in lockstep
//   5 / 6   the same with staggered wave groups
//   7 / 8   persistent form (next tile's first K-tile under the epilogue), one workgroup per CU
// Same template (gemm_bf16_tiles.h), same epilogues (gemm_bf16_epilogue.h), same plans (gemm_bf16_plan.h) as the product.
#include "../gemm_bf16_tiles.h"
#include "../gemm_bf16_plan.h"

namespace ucod {

// =====================================================================================================
// Persistent form of the large-tile kernel: one workgroup per CU walks tiles vt = blockIdx.x, +gridDim.x, ...
// What it buys: the first K-tile of the NEXT output tile (A0|A1|B, 9-11 LDS-DMAs per thread) is issued BEFORE the epilogue of
// the current tile, into the K-tile buffer the main loop has just vacated, so the ~3 us of first-tile HBM/L2 latency that every
// tile of the one-shot kernel pays up front (13 % of a K=768 tile) hides under the epilogue's stores.  The epilogue stages
// through the OTHER buffer (4 passes of 32 rows, 8 KB per wave) so the two never touch the same LDS bytes.
// Hazards on top of the one-shot kernel's:
//   * next-tile DMAs target buffer free_buf = (last K-tile's buffer)^1, last read during K-tile nt-2: dead long before;
//   * epilogue staging lives in last_buf, whose operand reads all retired before the stagger-out barrier;
//   * after the epilogue: every wave `vmcnt(0)` (its DMAs landed; also its stores) -> barrier -> only then may B(1) of the next
//     tile be DMA'd into last_buf (it overlaps other waves' staging areas) and the next main loop read free_buf.
// =====================================================================================================
template <int EPI, int NT>
__global__ __launch_bounds__(512) void gemm_bf16_pers_kernel(const GemmArgs a) {
  using Cfg = BigCfg<NT>;
  __shared__ __attribute__((aligned(16))) char smem[2 * Cfg::BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int ntiles = a.tiles_m * a.tiles_n;
  const int K = a.K, nt = K / BK;
  constexpr int WCOLS = 16 * NT;

  auto decode = [&](int vt, int& m0, int& n0) {
    const int q = ntiles >> 3, r8 = ntiles & 7, xcd = vt & 7;
    const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (vt >> 3);
    int tm, tn;
    tile_of(a, wg, tm, tn);
    m0 = tm * 256;
    n0 = tn * Cfg::BN_;
  };
  // DMA source rows as 32-bit element offsets from the tile's first A / B row (64-bit per-tile bases stay in SGPRs): the
  // persistent kernel keeps the next tile's sources live across the epilogue, and 64-bit pointers there spilled VGPRs.
  unsigned srcA[2][2], srcB[Cfg::NB];
  const bf16_raw *baseA, *baseB;
  auto set_src = [&](int m0, int n0) {
    baseA = a.A + (size_t)m0 * K;
    baseB = a.B + (size_t)n0 * K;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = (i * 8 + wave) * 8 + (lane >> 3);
        int lr = h * 128 + r;
        lr = (m0 + lr) < a.M ? lr : a.M - 1 - m0;
        srcA[h][i] = (unsigned)lr * (unsigned)K + swz(r, lane & 7) * 8;
      }
#pragma unroll
    for (int i = 0; i < Cfg::NB; ++i) {
      const int r = (i * 8 + wave) * 8 + (lane >> 3);
      int lr = (n0 + r) < a.N ? r : a.N - 1 - n0;
      srcB[i] = (unsigned)lr * (unsigned)K + swz(r, lane & 7) * 8;
    }
  };
  auto dma = [&](const bf16_raw* src, char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };
  auto stageA = [&](int t, int h, int pb) {
    char* slot = smem + ((t + pb) & 1) * Cfg::BUF + h * SLOT_A;
#pragma unroll
    for (int i = 0; i < 2; ++i) dma(baseA + t * BK + srcA[h][i], slot + (i * 8 + wave) * 1024);
  };
  auto stageB = [&](int t, int i0, int i1, int pb) {
    char* slot = smem + ((t + pb) & 1) * Cfg::BUF + 2 * SLOT_A;
#pragma unroll
    for (int i = 0; i < Cfg::NB; ++i)
      if (i >= i0 && i < i1) dma(baseB + t * BK + srcB[i], slot + (i * 8 + wave) * 1024);
  };
  constexpr int B_SPLIT = Cfg::NB >= 2 ? 2 : 1;

#ifdef UCOD_GEMM_STAMPS
  unsigned long long st_loop = 0, st_epi = 0, st_wait = 0, st_tiles = 0, t0s, t1s, t2s, t3s;
#define STAMP(v) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory")
#else
#define STAMP(v)
#endif
  int vt = blockIdx.x, pb = 0, m0, n0;
  decode(vt, m0, n0);
  float cb[NT], cs[NT];
  load_col_consts<EPI, NT>(a, n0 + wn * WCOLS + (lane & 15), cb, cs);
  set_src(m0, n0);
  stageA(0, 0, pb);
  stageA(0, 1, pb);
  stageB(0, 0, Cfg::NB, pb);
  if (nt > 1) {
    stageB(1, 0, Cfg::NB, pb);
    wait_vmcnt<Cfg::NB>();
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  while (true) {
    finish_col_consts<EPI, NT>(a, cb, cs);
    f32x4 acc[8][NT];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){cb[j], cb[j], cb[j], cb[j]};
    STAMP(t0s);
    if (wm == 1) __builtin_amdgcn_s_barrier();               // stagger in (see the one-shot kernel)

    for (int t = 0; t < nt; ++t) {
      const char* bufA = smem + ((t + pb) & 1) * Cfg::BUF + wm * SLOT_A;
      const char* bufB = smem + ((t + pb) & 1) * Cfg::BUF + 2 * SLOT_A;
      const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
      hx8 fb[NT][2];
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) {
        if (ph == 0 && more1) stageA(t + 1, 0, pb);
        if (ph == 1 && more1) stageA(t + 1, 1, pb);
        if (ph == 2 && more2) stageB(t + 2, 0, B_SPLIT, pb);
        if (ph == 3 && more2) stageB(t + 2, B_SPLIT, Cfg::NB, pb);
        if (ph == 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              const int r = wn * 16 * NT + j * 16 + (lane & 15);
              fb[j][ks] = *reinterpret_cast<const hx8*>(bufB + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
            }
        }
        hx8 fa[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int r = ph * 32 + i * 16 + (lane & 15);
            fa[i][ks] = *reinterpret_cast<const hx8*>(bufA + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
          }
        if (ph == 3) {
          if (more2) wait_vmcnt<Cfg::NB>(); else wait_vmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[ph * 2 + i][j] = UCOD_MFMA16(fa[i][ks], fb[j][ks], acc[ph * 2 + i][j]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();               // stagger out: every wave is past its last LDS operand read
    STAMP(t1s);

    const int last_buf = (nt - 1 + pb) & 1, free_buf = last_buf ^ 1;
    const int vnext = vt + gridDim.x;
    const bool has_next = vnext < ntiles;
    const int em0 = m0, en0 = n0;
    if (has_next) {                                           // first K-tile of the next tile, in flight under the epilogue
      decode(vnext, m0, n0);
      set_src(m0, n0);
      stageA(0, 0, free_buf);
      stageA(0, 1, free_buf);
      stageB(0, 0, Cfg::NB, free_buf);
    }
    big_epilogue<EPI, NT>(a, acc, cs, smem + last_buf * Cfg::BUF + wave * (32 * WCOLS * 4), em0 + wm * 128, en0 + wn * WCOLS, lane);
    if (has_next) load_col_consts<EPI, NT>(a, n0 + wn * WCOLS + (lane & 15), cb, cs);   // retired by the vmcnt(0) below, with the stores
    STAMP(t2s);
#ifdef UCOD_GEMM_STAMPS
    wait_vmcnt<0>();
    STAMP(t3s);
    st_loop += t1s - t0s; st_epi += t2s - t1s; st_wait += t3s - t2s; st_tiles += 1;
    if (!has_next) {
      if (tid == 0 && a.stamps) { a.stamps[blockIdx.x * 4 + 0] = st_loop; a.stamps[blockIdx.x * 4 + 1] = st_epi; a.stamps[blockIdx.x * 4 + 2] = st_wait; a.stamps[blockIdx.x * 4 + 3] = st_tiles; }
      break;
    }
#else
    if (!has_next) break;
    wait_vmcnt<0>();
#endif
    __builtin_amdgcn_s_barrier();
    vt = vnext;
    pb = free_buf;
    if (nt > 1) stageB(1, 0, Cfg::NB, pb);
  }
}



// =====================================================================================================
// Variant 20 (round 3, experiment): persistent 256 x 192 kernel that PARKS the finished tile.  One workgroup per CU walks tiles
// orig = blockIdx.x, + gridDim.x, ...; the K-tiles of consecutive output tiles run as ONE pipeline (the next tile's K-tile 0 / 1 are
// requested during the current tile's last two K-tiles); after the last K-tile the accumulators go through a wave-private staging area
// (48 KB beside the two 56 KB K-tile buffers = 160 KB) into 48 registers of packed bf16 per lane, in the row-major 16-byte chunks the
// stores want, and those 12 stores are issued one per K-tile of the NEXT tile's main loop.  Nothing of the drain is left in front of the
// matrix pipe except the conversion.  256-row tiles only (no tall tiles); epilogues: bias (+ column scale) -> bf16, bias + GELU -> bf16.
// =====================================================================================================
template <int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_park_kernel(const GemmArgs a) {
  constexpr int NT = 3, IT = 4, NPH = 2, SLOT = 128 * 128, NB = 3, BN_ = 192, WCOLS = 48;
  constexpr int BUF = 2 * SLOT + BN_ * 128;                      // 57 344 bytes: A0 | A1 | B of one K-tile
  constexpr int STG = 32 * WCOLS * 4;                            // 6 144 bytes of staging per wave
  constexpr unsigned DROP = 0x80000000u;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF + 8 * STG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int K = a.K, nt = K / BK;                                // (launch: nt even, >= 2)
  const int ntiles = a.tiles_m * a.tiles_n, G = gridDim.x;
  char* wstage = smem + 2 * BUF + wave * STG;

  const unsigned long bytesA = (unsigned long)a.M * K * 2ul, bytesB = (unsigned long)a.N * K * 2ul;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(a.A), 0, bytesA > 0xFFFFFFFFul ? 0xFFFFFFFFu : (unsigned)bytesA, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(a.B), 0, bytesB > 0xFFFFFFFFul ? 0xFFFFFFFFu : (unsigned)bytesB, 0x00020000);
  const auto rsO = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.out), 0, (unsigned)((unsigned long)a.M * a.N * 2ul), 0x00020000);

  auto tile_xy = [&](int orig, int& m0, int& n0) {
    const int q = ntiles >> 3, r8 = ntiles & 7, xcd = orig & 7;
    const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
    int tm, tn;
    tile_of(a, wg, tm, tn);
    m0 = tm * 256;
    n0 = tn * BN_;
  };
  unsigned offA[2][2], offB[NB];
  auto set_offsets = [&](int m0, int n0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = (i * 8 + wave) * 8 + (lane >> 3);
        offA[h][i] = ((unsigned)(m0 + h * 128 + r) * (unsigned)K + (unsigned)swz(r, lane & 7) * 8u) * 2u;
      }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int r = (i * 8 + wave) * 8 + (lane >> 3);
      offB[i] = ((unsigned)(n0 + r) * (unsigned)K + (unsigned)swz(r, lane & 7) * 8u) * 2u;
    }
  };
  auto stageA = [&](int t, int h) {
    char* slot = smem + (t & 1) * BUF + h * SLOT;
    const unsigned kt = (unsigned)t * (BK * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(slot + (i * 8 + wave) * 1024), 16, offA[h][i], kt, 0, UCOD_LD_AUX_A);
  };
  auto stageB = [&](int t) {
    char* slot = smem + (t & 1) * BUF + 2 * SLOT;
    const unsigned kt = (unsigned)t * (BK * 2);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(slot + (i * 8 + wave) * 1024), 16, offB[i], kt, 0, UCOD_LD_AUX_B);
  };

  int orig = blockIdx.x;
  int m0, n0;
  tile_xy(orig, m0, n0);
  set_offsets(m0, n0);
  float cb[NT], cs[NT];
  load_col_consts<EPI, NT>(a, n0 + wn * WCOLS + (lane & 15), cb, cs);
  stageA(0, 0);
  stageA(0, 1);
  stageB(0);
  stageB(1);
  wait_vmcnt<NB>();                                              // K-tile 0 landed, B(1) in flight
  finish_col_consts<EPI, NT>(a, cb, cs);
  f32x4 acc[8][NT];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){cb[j], cb[j], cb[j], cb[j]};
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();                     // staggered wave groups

  u32x4 park[12];                                                // the previous tile, packed bf16: chunk q = pass * 3 + it
  bool have_parked = false;
  int pm = 0, pn = 0;                                            // first row / column of the parked wave tile
  // (row, chunk) of wave instruction `it` inside a 32-row pass: 6 chunks of 8 columns per row
  auto lrow = [&](int it) { return (it * 64 + lane) / 6; };    // (recomputed: index arrays cost registers this kernel does not have)
  auto lchk = [&](int it) { return (it * 64 + lane) - lrow(it) * 6; };
  const unsigned row_bytes = (unsigned)a.N * 2u;
  auto park_store = [&](int q) {
    const int pass = q / 3, it = q - pass * 3;
    const int m = pm + pass * 32 + lrow(it), n = pn + lchk(it) * 8;
    const unsigned off = (m < a.M && n < a.N) ? (unsigned)m * row_bytes + (unsigned)n * 2u : DROP;
    __builtin_amdgcn_raw_buffer_store_b128(park[q], rsO, off, 0, UCOD_ST_AUX);
  };
  const int spk = (12 + nt - 1) / nt;                            // parked stores per K-tile

  for (;;) {
    const bool has_next = orig + G < ntiles;
    int m0n = 0, n0n = 0;
    float cbn[NT], csn[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { cbn[j] = 0.f; csn[j] = 1.f; }
    for (int t = 0; t < nt; ++t) {
      const char* bufA = smem + (t & 1) * BUF + wm * SLOT;
      const char* bufB = smem + (t & 1) * BUF + 2 * SLOT;
      const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
      hx8 fb[NT][2];
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        if (ph == 0) {
          if (have_parked) {
            for (int q = t * spk; q < (t + 1) * spk && q < 12; ++q) {
              switch (q) {                                       // (register array: compile-time indices)
#define PK(Q) case Q: park_store(Q); break;
                PK(0) PK(1) PK(2) PK(3) PK(4) PK(5) PK(6) PK(7) PK(8) PK(9) PK(10) PK(11)
#undef PK
              }
            }
          }
          if (more1) { stageA(t + 1, 0); stageA(t + 1, 1); }
          else if (has_next) { stageA(0, 0); stageA(0, 1); }     // (offsets already those of the next tile: switched at K-tile nt-2)
          if (t == nt - 2 && has_next) {                         // no DMA of this tile is left to issue: switch to the next tile's sources
            tile_xy(orig + G, m0n, n0n);
            set_offsets(m0n, n0n);
            load_col_consts<EPI, NT>(a, n0n + wn * WCOLS + (lane & 15), cbn, csn);
          }
        }
        if (ph == 1) {
          if (more2) stageB(t + 2);
          else if (has_next) stageB(t + 2 - nt);
        }
        if (ph == 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              const int r = wn * WCOLS + j * 16 + (lane & 15);
              fb[j][ks] = *reinterpret_cast<const hx8*>(bufB + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
            }
        }
        hx8 fa[IT][2];
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int r = ph * (IT * 16) + i * 16 + (lane & 15);
            fa[i][ks] = *reinterpret_cast<const hx8*>(bufA + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
          }
        if (ph == NPH - 1) {
          if (more2 || has_next) wait_vmcnt<NB>(); else wait_vmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[ph * IT + i][j] = UCOD_MFMA16(fa[i][ks], fb[j][ks], acc[ph * IT + i][j]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- conversion: accumulators -> (scale, GELU) -> packed bf16 in the row-major chunk layout, through the wave's staging area
    if (have_parked) {                                           // (only when nt * spk < 12: never for nt >= 12)
      for (int q = nt * spk; q < 12; ++q) {
        switch (q) {
#define PK(Q) case Q: park_store(Q); break;
          PK(0) PK(1) PK(2) PK(3) PK(4) PK(5) PK(6) PK(7) PK(8) PK(9) PK(10) PK(11)
#undef PK
        }
      }
    }
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          f32x4 v = acc[pass * 2 + i][j];
          if constexpr (EPI == UCOD_EPI_BIAS_BF16) v = v * cs[j];
#pragma unroll
          for (int rg = 0; rg < 4; ++rg)
            *reinterpret_cast<float*>(wstage + (i * 16 + (lane >> 4) * 4 + rg) * (WCOLS * 4) + (j * 16 + (lane & 15)) * 4) = v[rg];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < 3; ++it) {
        f32x4 v0 = *reinterpret_cast<const f32x4*>(wstage + lrow(it) * (WCOLS * 4) + lchk(it) * 32);
        f32x4 v1 = *reinterpret_cast<const f32x4*>(wstage + lrow(it) * (WCOLS * 4) + lchk(it) * 32 + 16);
        if constexpr (EPI == UCOD_EPI_BIAS_GELU_BF16) {
          const f32x2 g0 = gelu_erf2((f32x2){v0[0], v0[1]}), g1 = gelu_erf2((f32x2){v0[2], v0[3]});
          const f32x2 g2 = gelu_erf2((f32x2){v1[0], v1[1]}), g3 = gelu_erf2((f32x2){v1[2], v1[3]});
          v0 = (f32x4){g0[0], g0[1], g1[0], g1[1]};
          v1 = (f32x4){g2[0], g2[1], g3[0], g3[1]};
        }
        u32x4 w;
        w[0] = pack_h2(v0[0], v0[1]);
        w[1] = pack_h2(v0[2], v0[3]);
        w[2] = pack_h2(v1[0], v1[1]);
        w[3] = pack_h2(v1[2], v1[3]);
        park[pass * 3 + it] = w;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    pm = m0 + wm * 128;
    pn = n0 + wn * WCOLS;
    have_parked = true;
    if (!has_next) break;
    orig += G;
    m0 = m0n;
    n0 = n0n;
    finish_col_consts<EPI, NT>(a, cbn, csn);
#pragma unroll
    for (int j = 0; j < NT; ++j) { cb[j] = cbn[j]; cs[j] = csn[j]; }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){cb[j], cb[j], cb[j], cb[j]};
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int q = 0; q < 12; ++q) park_store(q);
}

// =====================================================================================================
// Variant 21 (round 4, experiment): variant 20 with the conversion IN REGISTERS.  The MFMA operands are swapped (weight fragment as A,
// activation fragment as B), so the accumulator tile is the TRANSPOSED 16 x 16 block: lane (g = lane >> 4, c = lane & 15) holds row c,
// columns 4g..4g+3 -- four consecutive output columns, 8 bytes of bf16.  Two tiles (T0, T1) make 16-byte row chunks with two
// v_permlane16_swap (odd 16-lane rows of T0's words <-> even rows of T1's): afterwards an even-g lane holds columns 4g..4g+7 of T0's row c and
// an odd-g lane columns 4(g-1)..4(g-1)+7 of T1's row c.  Per wave tile (24 tiles): 48 v_cvt_pk + 24 swaps = 72 vector instructions instead of
// 96 ds_write + 24 ds_read_b128 + waits; no staging area.  tools/probes/acc_transpose_probe.hip prices the alternative (8 x 8 transposes
// inside the untransposed tile with DPP) at 2-4 k cycles per wave tile.
// =====================================================================================================
template <int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_park2_kernel(const GemmArgs a) {
  constexpr int NT = 3, IT = 4, NPH = 2, SLOT = 128 * 128, NB = 3, BN_ = 192, WCOLS = 48;
  constexpr int BUF = 2 * SLOT + BN_ * 128;                      // 57 344 bytes: A0 | A1 | B of one K-tile
  constexpr unsigned DROP = 0x80000000u;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int K = a.K, nt = K / BK;                                // (launch: nt even, >= 2)
  const int ntiles = a.tiles_m * a.tiles_n, G = gridDim.x;

  const unsigned long bytesA = (unsigned long)a.M * K * 2ul, bytesB = (unsigned long)a.N * K * 2ul;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(a.A), 0, bytesA > 0xFFFFFFFFul ? 0xFFFFFFFFu : (unsigned)bytesA, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(a.B), 0, bytesB > 0xFFFFFFFFul ? 0xFFFFFFFFu : (unsigned)bytesB, 0x00020000);
  const auto rsO = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.out), 0, (unsigned)((unsigned long)a.M * a.N * 2ul), 0x00020000);

  auto tile_xy = [&](int orig, int& m0, int& n0) {
    const int q = ntiles >> 3, r8 = ntiles & 7, xcd = orig & 7;
    const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
    int tm, tn;
    tile_of(a, wg, tm, tn);
    m0 = tm * 256;
    n0 = tn * BN_;
  };
  unsigned offA[2][2], offB[NB];
  auto set_offsets = [&](int m0, int n0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = (i * 8 + wave) * 8 + (lane >> 3);
        offA[h][i] = ((unsigned)(m0 + h * 128 + r) * (unsigned)K + (unsigned)swz(r, lane & 7) * 8u) * 2u;
      }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int r = (i * 8 + wave) * 8 + (lane >> 3);
      offB[i] = ((unsigned)(n0 + r) * (unsigned)K + (unsigned)swz(r, lane & 7) * 8u) * 2u;
    }
  };
  auto stageA = [&](int t, int h) {
    char* slot = smem + (t & 1) * BUF + h * SLOT;
    const unsigned kt = (unsigned)t * (BK * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(slot + (i * 8 + wave) * 1024), 16, offA[h][i], kt, 0, UCOD_LD_AUX_A);
  };
  auto stageB = [&](int t) {
    char* slot = smem + (t & 1) * BUF + 2 * SLOT;
    const unsigned kt = (unsigned)t * (BK * 2);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(slot + (i * 8 + wave) * 1024), 16, offB[i], kt, 0, UCOD_LD_AUX_B);
  };

  int orig = blockIdx.x;
  int m0, n0;
  tile_xy(orig, m0, n0);
  set_offsets(m0, n0);
  // column constants of the lane's four columns per column tile (the transposed tile: columns 4g..4g+3)
  const float* biasp = a.bias;
  const float* scalep = (EPI == UCOD_EPI_BIAS_BF16 && a.scale) ? a.scale : nullptr;
  auto load_cc = [&](int ncol0, f32x4 (&b4)[NT], f32x4 (&s4)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      int n = ncol0 + j * 16;
      n = n + 4 <= a.N ? n : a.N - 4;
      b4[j] = *reinterpret_cast<const f32x4*>(biasp + n);
      if constexpr (EPI == UCOD_EPI_BIAS_BF16) s4[j] = scalep ? *reinterpret_cast<const f32x4*>(scalep + n) : (f32x4){1.f, 1.f, 1.f, 1.f};
      else s4[j] = (f32x4){1.f, 1.f, 1.f, 1.f};
    }
  };
  // (bias and scale are applied at the conversion, from loads issued there: 24 registers the main loop does not have)
  stageA(0, 0);
  stageA(0, 1);
  stageB(0);
  stageB(1);
  wait_vmcnt<NB>();                                              // K-tile 0 landed, B(1) in flight
  f32x4 acc[8][NT];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();                     // staggered wave groups

  // pair q of the wave tile's 24 transposed 16 x 16 tiles: q < 8: (row tile q, column tiles 0 | 1); q >= 8: (row tiles 2(q-8) | 2(q-8)+1, column tile 2)
  u32x4 park[12];                                                // the previous tile, packed bf16, one 16-byte row chunk per pair
  bool have_parked = false;
  int pm = 0, pn = 0;                                            // first row / column of the parked wave tile
  const unsigned row_bytes = (unsigned)a.N * 2u;
  const int godd = (lane >> 4) & 1, gcol = ((lane >> 4) & 2) * 4;   // odd-g lanes store T1's chunk; chunk column 0 or 8 inside the tile
  auto park_store = [&](int q) {
    const int i = q < 8 ? q : 2 * (q - 8) + godd, j = q < 8 ? godd : 2;
    const int m = pm + i * 16 + (lane & 15), n = pn + j * 16 + gcol;
    const unsigned off = (m < a.M && n < a.N) ? (unsigned)m * row_bytes + (unsigned)n * 2u : DROP;
    __builtin_amdgcn_raw_buffer_store_b128(park[q], rsO, off, 0, UCOD_ST_AUX);
  };
  const int spk = (12 + nt - 1) / nt;                            // parked stores per K-tile

  for (;;) {
    const bool has_next = orig + G < ntiles;
    int m0n = 0, n0n = 0;
    for (int t = 0; t < nt; ++t) {
      const char* bufA = smem + (t & 1) * BUF + wm * SLOT;
      const char* bufB = smem + (t & 1) * BUF + 2 * SLOT;
      const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
      hx8 fb[NT][2];
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        bool stored = false;
        if (ph == 0) {
          if (more1) { stageA(t + 1, 0); stageA(t + 1, 1); }
          else if (has_next) { stageA(0, 0); stageA(0, 1); }     // (offsets already those of the next tile: switched at K-tile nt-2)
          if (t == nt - 2 && has_next) {                         // no DMA of this tile is left to issue: switch to the next tile's sources
            tile_xy(orig + G, m0n, n0n);
            set_offsets(m0n, n0n);
          }
        }
        if (ph == 1) {
          if (more2) stageB(t + 2);
          else if (has_next) stageB(t + 2 - nt);
          // the parked store goes out BEHIND this K-tile's DMAs and is left outstanding by the counted wait below (vmcnt NB + 1): it has a
          // whole K-tile to be acknowledged (variant 20 issues it ahead of the DMAs, so the wait half a K-tile later includes it)
          if (have_parked && spk == 1 && t < 12) {
            switch (t) {                                         // (register array: compile-time indices)
#define PK(Q) case Q: park_store(Q); break;
              PK(0) PK(1) PK(2) PK(3) PK(4) PK(5) PK(6) PK(7) PK(8) PK(9) PK(10) PK(11)
#undef PK
            }
            stored = true;
          } else if (have_parked) {
            for (int q = t * spk; q < (t + 1) * spk && q < 12; ++q) {
              switch (q) {
#define PK(Q) case Q: park_store(Q); break;
                PK(0) PK(1) PK(2) PK(3) PK(4) PK(5) PK(6) PK(7) PK(8) PK(9) PK(10) PK(11)
#undef PK
              }
            }
          }
        }
        if (ph == 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              const int r = wn * WCOLS + j * 16 + (lane & 15);
              fb[j][ks] = *reinterpret_cast<const hx8*>(bufB + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
            }
        }
        hx8 fa[IT][2];
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int r = ph * (IT * 16) + i * 16 + (lane & 15);
            fa[i][ks] = *reinterpret_cast<const hx8*>(bufA + r * 128 + swz(r, ks * 4 + (lane >> 4)) * 16);
          }
        if (ph == NPH - 1) {
          if (!(more2 || has_next)) wait_vmcnt<0>();
          else if (stored) wait_vmcnt<NB + 1>();
          else wait_vmcnt<NB>();
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[ph * IT + i][j] = UCOD_MFMA16(fb[j][ks], fa[i][ks], acc[ph * IT + i][j]);   // transposed tile: lane = row, registers = 4 columns
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- conversion: accumulators -> (scale, GELU) -> packed bf16 row chunks, in registers
    if (have_parked) {                                           // (only when nt * spk < 12: never for nt >= 12)
      for (int q = nt * spk; q < 12; ++q) {
        switch (q) {
#define PK(Q) case Q: park_store(Q); break;
          PK(0) PK(1) PK(2) PK(3) PK(4) PK(5) PK(6) PK(7) PK(8) PK(9) PK(10) PK(11)
#undef PK
        }
      }
    }
    f32x4 cb[NT], cs[NT];
    load_cc(n0 + wn * WCOLS + (lane >> 4) * 4, cb, cs);
    auto cvt = [&](int i, int j, unsigned& w0, unsigned& w1) {
      f32x4 v = acc[i][j] + cb[j];
      if constexpr (EPI == UCOD_EPI_BIAS_BF16) v = v * cs[j];
      if constexpr (EPI == UCOD_EPI_BIAS_GELU_BF16) {
        const f32x2 g0 = gelu_erf2((f32x2){v[0], v[1]}), g1 = gelu_erf2((f32x2){v[2], v[3]});
        v = (f32x4){g0[0], g0[1], g1[0], g1[1]};
      }
      w0 = pack_h2(v[0], v[1]);
      w1 = pack_h2(v[2], v[3]);
    };
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const int i0 = q < 8 ? q : 2 * (q - 8), i1 = q < 8 ? q : 2 * (q - 8) + 1, j0 = q < 8 ? 0 : 2, j1 = q < 8 ? 1 : 2;
      unsigned a0, a1, b0, b1;
      cvt(i0, j0, a0, a1);
      cvt(i1, j1, b0, b1);
      const auto r0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);   // [0]: a0 with its odd rows <- b0's even rows; [1]: b0 with its even rows <- a0's odd rows
      const auto r1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
      park[q] = (u32x4){r0[0], r1[0], r0[1], r1[1]};
    }
    pm = m0 + wm * 128;
    pn = n0 + wn * WCOLS;
    have_parked = true;
    if (!has_next) break;
    orig += G;
    m0 = m0n;
    n0 = n0n;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int q = 0; q < 12; ++q) park_store(q);
}

// =====================================================================================================
// Variant 22 (round 4, experiment): the product's large-tile kernel (256 x 256 x 64, 8 waves, two barrier intervals per K-tile, staggered wave
// groups) on v_mfma_f32_32x32x16 instead of v_mfma_f32_16x16x32.  Why: an MFMA holds its SIMD's vector issue for 8 cycles whatever its shape
// (MI355X_MICROARCH.md, per-instruction constants) -- 8 of 16 for the 16 x 16 x 32 form, 8 of 32 for the 32 x 32 x 16 form -- and the wave
// that shares the SIMD issues its fragment reads and LDS-DMAs (~60 cycles of issue each) exactly while its partner is in its MFMA interval:
// with 16 x 16 tiles that interval leaves half the issue cycles, with 32 x 32 tiles three quarters.  Same LDS images, same DMA schedule, same
// number of fragment reads; accumulators 4 x 2 tiles of 16 registers; drain through big_epilogue_staged with a stager for the 32 x 32 C layout
// (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).
// =====================================================================================================
template <int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_big32_kernel(const GemmArgs a) {
  constexpr int NT = 4, NPH = 2, IT = 2, JT = 2;                  // per phase: 2 row tiles of 32; 2 column tiles of 32 per wave
  using Cfg = BigCfg<NT>;
  __shared__ __attribute__((aligned(16))) char smem[2 * Cfg::BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nwg = a.tiles_m * a.tiles_n;
  const int orig = blockIdx.x;
  const int q = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
  const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
  int tm, tn;
  tile_of(a, wg, tm, tn);
  const int m0 = tm * 256, n0 = tn * Cfg::BN_;
  const int K = a.K, nt = K / BK;
  const bf16_raw* srcA[2][2];
  const bf16_raw* srcB[Cfg::NB];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (i * 8 + wave) * 8 + (lane >> 3);
      int gr = m0 + h * 128 + r;
      gr = gr < a.M ? gr : a.M - 1;
      srcA[h][i] = a.A + (size_t)gr * K + swz(r, lane & 7) * 8;
    }
#pragma unroll
  for (int i = 0; i < Cfg::NB; ++i) {
    const int r = (i * 8 + wave) * 8 + (lane >> 3);
    int gr = n0 + r;
    gr = gr < a.N ? gr : a.N - 1;
    srcB[i] = a.B + (size_t)gr * K + swz(r, lane & 7) * 8;
  }
  auto dmaA = [&](const bf16_raw* src, char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, UCOD_LD_AUX_A);
  };
  auto dmaB = [&](const bf16_raw* src, char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, UCOD_LD_AUX_B);
  };
  auto stageA = [&](int t, int h) {
    char* slot = smem + (t & 1) * Cfg::BUF + h * SLOT_A;
#pragma unroll
    for (int i = 0; i < 2; ++i) dmaA(srcA[h][i] + t * BK, slot + (i * 8 + wave) * 1024);
  };
  auto stageB = [&](int t) {
    char* slot = smem + (t & 1) * Cfg::BUF + 2 * SLOT_A;
#pragma unroll
    for (int i = 0; i < Cfg::NB; ++i) dmaB(srcB[i] + t * BK, slot + (i * 8 + wave) * 1024);
  };
  // per-column constants of the lane's two columns (32-wide tiles: col = lane & 31)
  float cb[JT], cs[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    int n = n0 + wn * 64 + j * 32 + (lane & 31);
    n = n < a.N ? n : a.N - 1;
    cb[j] = a.bias ? a.bias[n] : 0.f;
    cs[j] = (EPI == UCOD_EPI_BIAS_BF16 && a.scale) ? a.scale[n] : 1.f;
  }
  stageA(0, 0);
  stageA(0, 1);
  stageB(0);
  if (nt > 1) stageB(1);
  if (nt > 1) wait_vmcnt<Cfg::NB>(); else wait_vmcnt<0>();
  f32x16 acc[4][JT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = cb[j];
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();
  const int chunk_hi = lane >> 5;                                  // which 8 of a k-step's 16 k values this lane supplies
  for (int t = 0; t < nt; ++t) {
    const char* bufA = smem + (t & 1) * Cfg::BUF + wm * SLOT_A;
    const char* bufB = smem + (t & 1) * Cfg::BUF + 2 * SLOT_A;
    const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
    hx8 fb[JT][4];
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
      if (ph == 0 && more1) { stageA(t + 1, 0); stageA(t + 1, 1); }
      if (ph == 1 && more2) stageB(t + 2);
      if (ph == 0) {
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const int r = wn * 64 + j * 32 + (lane & 31);
            fb[j][ks] = *reinterpret_cast<const hx8*>(bufB + r * 128 + swz(r, ks * 2 + chunk_hi) * 16);
          }
      }
      hx8 fa[IT][4];
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int r = ph * 64 + i * 32 + (lane & 31);
          fa[i][ks] = *reinterpret_cast<const hx8*>(bufA + r * 128 + swz(r, ks * 2 + chunk_hi) * 16);
        }
      if (ph == NPH - 1) {
        if (more2) wait_vmcnt<Cfg::NB>(); else wait_vmcnt<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
          for (int j = 0; j < JT; ++j)
            acc[ph * IT + i][j] = UCOD_MFMA32(fa[i][ks], fb[j][ks], acc[ph * IT + i][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();
  char* wbase = smem + wave * (32 * EPI_PITCH(16 * NT));
  auto stage = [&](int pass) {                                     // pass = the wave's row tile of 32
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      f32x16 v = acc[pass][j];
      if constexpr (kStageScaled<EPI>) v = v * cs[j];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        *reinterpret_cast<float*>(wbase + ((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * EPI_PITCH(16 * NT) + (j * 32 + (lane & 31)) * 4) = v[r];
    }
  };
  big_epilogue_staged<EPI, NT, 8, UCOD_ST_AUX, false>(a, stage, wbase, m0 + wm * 128, n0 + wn * 64, lane);
}


template <int EPI>
static int launch_lab(GemmArgs a, int variant, hipStream_t s) {
  if (variant == 20 || variant == 21) {                          // persistent 192-wide kernels with the parked tile (bf16 epilogues only)
    if constexpr (EPI == UCOD_EPI_BIAS_BF16 || EPI == UCOD_EPI_BIAS_GELU_BF16) {
      const int nt = a.K / BK;
      if ((a.N & 7) != 0 || nt < 2 || (nt & 1) || !a.bias || (long)a.M * a.N * 2 >= (1L << 31) || (long)a.M * a.K * 2 >= (1L << 32) || (long)a.N * a.K * 2 >= (1L << 32))
        return UCOD_EINVAL;
      a.tiles_m = cdiv(a.M, 256);
      a.tiles_n = cdiv(a.N, 192);
      a.col_fast = a.tiles_n <= 4;
      const int n_cu = device_cus(), ntiles = a.tiles_m * a.tiles_n;
      if (variant == 21) hipLaunchKernelGGL((gemm_bf16_park2_kernel<EPI>), dim3(ntiles < n_cu ? ntiles : n_cu), dim3(512), 0, s, a);
      else hipLaunchKernelGGL((gemm_bf16_park_kernel<EPI>), dim3(ntiles < n_cu ? ntiles : n_cu), dim3(512), 0, s, a);
      UCOD_CHECK_LAUNCH();
      return UCOD_OK;
    } else {
      return UCOD_EINVAL;
    }
  }
  if (variant == 22) {                                           // the plain large-tile kernel on 32 x 32 x 16 MFMAs (no patches: whole grid)
    if constexpr (EPI == UCOD_EPI_BIAS_BF16 || EPI == UCOD_EPI_BIAS_GELU_BF16 || EPI == UCOD_EPI_BIAS_SCALE_RESID_F32 || EPI == UCOD_EPI_BIAS_F32) {
      if ((a.N & 7) != 0) return UCOD_EINVAL;
      a.tiles_m = cdiv(a.M, 256);
      a.tiles_n = cdiv(a.N, 256);
      a.col_fast = a.tiles_n <= 4;
      hipLaunchKernelGGL((gemm_bf16_big32_kernel<EPI>), dim3(a.tiles_m * a.tiles_n), dim3(512), 0, s, a);
      UCOD_CHECK_LAUNCH();
      return UCOD_OK;
    } else {
      return UCOD_EINVAL;
    }
  }
  if (variant < 3 || variant > 8 || (a.N & 3) != 0) return UCOD_EINVAL;
  constexpr bool kBf16Out = (EPI == UCOD_EPI_BIAS_BF16 || EPI == UCOD_EPI_BIAS_GELU_BF16);
  if (kBf16Out && (a.N & 7) != 0) return UCOD_EINVAL;
  const bool wide = (variant == 3 || variant == 5 || variant == 7);
  a.tiles_m = cdiv(a.M, 256);
  a.tiles_n = cdiv(a.N, wide ? 256 : 192);
  a.col_fast = a.tiles_n <= 4;
  dim3 grid(a.tiles_m * a.tiles_n), block(512);
  if (variant != 7 && variant != 8) {
    const BigPlan pl = big_plan(a.M, a.N, a.K, wide ? 256 : 192, true);
    if (pl.patches) {
      a.main_tiles = pl.rounds * device_cus();
      a.patches_per_wg = cdiv((long)pl.left * pl.ppt, a.main_tiles);
      grid.x = a.main_tiles;
    }
  }
  switch (variant) {
    case 3: hipLaunchKernelGGL((gemm_bf16_big_kernel<EPI, 4, false>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((gemm_bf16_big_kernel<EPI, 3, false>), grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL((gemm_bf16_big_kernel<EPI, 4, true>), grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL((gemm_bf16_big_kernel<EPI, 3, true>), grid, block, 0, s, a); break;
    default: {                                             // 7, 8: persistent, one workgroup per CU
      const int n_cu = device_cus();
      const int ntiles = a.tiles_m * a.tiles_n;
      dim3 pgrid(ntiles < n_cu ? ntiles : n_cu);
#ifdef UCOD_GEMM_STAMPS
      if (const char* g = getenv("UCOD_PERS_GRID")) pgrid.x = atoi(g) < ntiles ? atoi(g) : ntiles;   // diagnostic: fewer active CUs
#endif
      if (variant == 7) hipLaunchKernelGGL((gemm_bf16_pers_kernel<EPI, 4>), pgrid, block, 0, s, a);
      else hipLaunchKernelGGL((gemm_bf16_pers_kernel<EPI, 3>), pgrid, block, 0, s, a);
    }
  }
  UCOD_CHECK_LAUNCH();
  return UCOD_OK;
}

}  // namespace ucod

// Same argument meaning as ucod_gemm_bf16 (include/ucod_dpl.h); epilogues 0..5 only.
extern "C" int ucod_gemm_bf16_lab(int epilogue, const void* A, const void* B, void* out, int M, int N, int K, const float* bias,
                                  const float* scale, const float* resid, const float* pos, int tokens_per_image, int variant,
                                  void* stream) {
  using namespace ucod;
  if (!A || !B || !out || M <= 0 || N <= 0 || K <= 0 || (K % BK) != 0) return UCOD_EINVAL;
  GemmArgs a;
  a.aux = nullptr;
  a.out2 = nullptr;
  a.ovf = nullptr;
  a.stamps = nullptr;
#ifdef UCOD_GEMM_STAMPS
  a.stamps = (unsigned long long*)pos;   // diagnostic build: the (otherwise unused here) `pos` argument carries the stamp buffer
#endif
  a.A = (const bf16_raw*)A;
  a.B = (const bf16_raw*)B;
  a.out = out;
  a.bias = bias;
  a.scale = scale;
  a.resid = resid;
  a.pos = pos;
  a.M = M;
  a.N = N;
  a.K = K;
  a.tok = tokens_per_image;
  a.nreg = 0;
  a.tiles_m = cdiv(M, BM);
  a.tiles_n = cdiv(N, BN);
  a.main_tiles = 0;
  a.patches_per_wg = 0;
  a.group_m = 8;
  a.col_fast = 0;
  hipStream_t s = (hipStream_t)stream;
  switch (epilogue) {
    case UCOD_EPI_BIAS_BF16: return launch_lab<UCOD_EPI_BIAS_BF16>(a, variant, s);
    case UCOD_EPI_BIAS_GELU_BF16: if (!bias) return UCOD_EINVAL; return launch_lab<UCOD_EPI_BIAS_GELU_BF16>(a, variant, s);
    case UCOD_EPI_BIAS_SCALE_RESID_F32: if (!bias || !scale || !resid) return UCOD_EINVAL; return launch_lab<UCOD_EPI_BIAS_SCALE_RESID_F32>(a, variant, s);
    case UCOD_EPI_PATCH_TOKENS_F32: if (!bias || !pos || tokens_per_image < 2) return UCOD_EINVAL; return launch_lab<UCOD_EPI_PATCH_TOKENS_F32>(a, variant, s);
    case UCOD_EPI_KEY_NCHW_F32: if (!bias || tokens_per_image < 2) return UCOD_EINVAL; return launch_lab<UCOD_EPI_KEY_NCHW_F32>(a, variant, s);
    case UCOD_EPI_BIAS_F32: return launch_lab<UCOD_EPI_BIAS_F32>(a, variant, s);
    default: return UCOD_EINVAL;
  }
}
