// The 256x256 one-wave-per-SIMD fp8 GEMM kernel (included by fp8_gemm.hip).
#pragma once
#include "fp8_epi.h"

namespace tdg {

// ---------------------------------------------------------------------------
// 256x256 tiles at ONE wave per SIMD (4 waves, 2 x 2, each 128 x 128: the
// 8 x 8 accumulator fragments live in AGPRs). Why: at 128x128 tiles the fp8
// MFMA consumes its operands twice as fast as bf16 does, so the LDS-DMA
// stream (32 KiB per 512-cycle K tile per CU, ~34 TB/s chip-wide) meets the
// L2 bandwidth and the kernel ran no faster than bf16; a 256x256 tile halves
// the bytes per FLOP.
//
// A K tile (128 bytes deep) is four 16 KiB half-tile images: A0 (rows 0..63
// of both wave rows), A1 (rows 64..127 of both), B0 / B1 likewise for the
// columns, double-buffered (128 KiB). Four phases of 16 MFMAs per wave --
// (a0,b0) (a0,b1) (a1,b1) (a1,b0) -- and every phase reads the fragments
// the NEXT phase needs behind its MFMAs:
//   P0: MFMA a0 x b0   reads B1(t)
//   P1: MFMA a0 x b1   reads A1(t)
//   P2: MFMA a1 x b1   reads A0(t+1)   (a0 registers are free after P1)
//   P3: MFMA a1 x b0   reads B0(t+1)   (per column, behind its MFMAs)
// Each phase starts with lgkmcnt(0) (last phase's reads are this phase's
// operands) + a counted vmcnt + one barrier; the LDS-DMA of tile t+2's
// halves goes into the buffers tile t's halves just vacated, one half per
// phase (A0 in P0, B0 in P1, B1 in P2, A1 in P3), so five halves (80 KiB)
// are in flight per CU in the steady state and every half has six phases to
// land.
// (f8w1::HB, f8w1::remap: fp8_impl.h)

template <int EPI, int AF = 0, int CF = 0>
__global__ __launch_bounds__(256) void gemm_fp8_w1_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, bf16_t* __restrict__ C,
    const float* __restrict__ bias, const float* __restrict__ sa, const float* __restrict__ sb,
    uint8_t* __restrict__ C8, const float* __restrict__ sc8, unsigned* __restrict__ amax_out,
    int M, int N, int K, int lda, int ldb, int ldc, int ldc8, F8Extra ex) {
  constexpr int NW = 4, TM = 8, TN = 8;
  constexpr int HB = f8w1::HB, SB = 4 * HB;  // stage: A0, A1, B0, B1
  using G = f8::Stage<128, NW>;               // 4 pieces of 1 KiB per wave per half
  static_assert(G::P == 4, "half-tile = 4 pieces per wave");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int tiles_m = cdiv(M, 256), tiles_n = cdiv(N, 256);
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  int tm, tn;
  TDG_F8_TILE_RASTER(t, tiles_m, tiles_n, tm, tn)
  const int m0 = tm * 256, n0 = tn * 256;
  const int nk = K / BK8;  // host guarantees K % 128 == 0

  G g;
  g.init(wid, lane);
  // per piece: byte offset of its 16-byte chunk (remapped image row, clamped
  // to the operand) for each half; the host guarantees 32-bit extents
  uint32_t aoff[2][4], boff[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int ra = m0 + f8w1::remap(g.row[i], h), rb = n0 + f8w1::remap(g.row[i], h);
      ra = ra < M ? ra : M - 1;
      rb = rb < N ? rb : N - 1;
      aoff[h][i] = (uint32_t)ra * (uint32_t)lda + (uint32_t)g.col[i];
      boff[h][i] = (uint32_t)rb * (uint32_t)ldb + (uint32_t)g.col[i];
    }
  // half q of tile kt: 0 = A0, 1 = B0, 2 = B1, 3 = A1 (issue order)
  auto issue = [&](int kt, int q) {
    char* st = smem + (kt & 1) * SB;
    const int k0 = kt * BK8;
    const bool isA = q == 0 || q == 3;
    const int h = (q == 0 || q == 1) ? 0 : 1;
    char* dst = st + (isA ? h : 2 + h) * HB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* src = (isA ? A + aoff[h][i] : B + boff[h][i]) + k0;
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + (wid * 4 + i) * 1024),
                                       16, 0, 0);
    }
  };

  f32x4 acc[TM][TN];
  TDG_F8_ZERO_ACC(TM, TN, acc)
  i32x8 fa[TM], fb[TN];
  const int ar = wm * 64, br = wn * 64;  // this wave's rows / columns in a half image

  auto mfma = [&](int i, int j) {
    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], AF, 0,
                                                                 0, 127, 0, 127);
  };
  TDG_F8_FOUR_PHASE_K_LOOP(f8::frag, mfma, issue)

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f8::lds_barrier();
  using Epi = F8Epi<256, 256, 2, 2, EPI, CF, false>;
  typename Epi::Pre none;
  Epi::run(smem, acc, C, bias, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex,
           none);
}

}  // namespace tdg
