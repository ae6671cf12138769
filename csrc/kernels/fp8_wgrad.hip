// fp8 weight gradients: dW[m][n] (f32, =|+= beta) = alpha * sum_t dY8[t][m] X8[t][n],
// alpha = 1 / (scale(dY8) scale(X8)), with dY8 the e5m2 gradient and X8 the
// e4m3 activation copy the forward / backward already produced, both
// TOKEN-major ([T][ld]): the reduction runs over rows, so the operand images
// are [128 tokens][m bytes] and the MFMA fragments (32 consecutive tokens of
// one m per lane) come from ds_read_b64_tr_b8, the gfx950 transposing read of
// 8-bit data (per 16-lane group: lane 2q+p addresses row q, bytes 8p..8p+7 of
// a 16-byte block; lane i receives column i of the 8 rows -- verified with
// exact data, scripts/probes/tr_b8_probe.hip). No transposed copies.
//
// Ragged launch (one per flush): up to 64 problems in up to 8 shape classes,
// 256x256 tiles at one wave per SIMD, the phase / half-tile schedule of
// gemm_fp8_w1_kernel (two 64 KiB stages of 128 tokens). Half-image rows are
// 128 bytes; 16-byte chunk c of token row t sits at chunk c ^ sw(t),
// sw(t) = ((t >> 1) & 3) | ((t >> 5) & 1) << 2, which makes every 32-lane
// half of a transposing fragment read touch all 64 banks once.
#include "tdg_api.h"
#include "fp8_impl.h"

namespace tdg {

constexpr int WF8_MAXP = 64, WF8_MAXC = 8;
struct WF8Class {
  int M, N, lda, ldb, ldc, tiles_m, tiles_n, tile_start, prob_start;
};
struct WF8Args {
  const uint8_t* A[WF8_MAXP];  // dY8 [T][lda] (e5m2)
  const uint8_t* B[WF8_MAXP];  // X8  [T][ldb] (e4m3)
  float* C[WF8_MAXP];          // dW  [M][ldc] f32
  const float* sa[WF8_MAXP];   // scale of A (one float, device)
  const float* sb[WF8_MAXP];
  WF8Class cls[WF8_MAXC];
  int ncls;
};


__global__ __launch_bounds__(256) void wgrad_fp8_kernel(const WF8Args args, int T, float beta) {
  constexpr int TM = 8, TN = 8;
  constexpr int HB = f8w1::HB, SB = 4 * HB;  // stage: A0, A1, B0, B1 (16 KiB each)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;

  const int t0 = xcd_remap(blockIdx.x, gridDim.x);
  WF8Class cl = args.cls[0];
#pragma unroll
  for (int i = 1; i < WF8_MAXC; ++i)
    if (i < args.ncls && t0 >= args.cls[i].tile_start) cl = args.cls[i];
  const int M = cl.M, N = cl.N, lda = cl.lda, ldb = cl.ldb, ldc = cl.ldc;
  const int tpp = cl.tiles_m * cl.tiles_n;
  const int lt = t0 - cl.tile_start;
  const int pr = cl.prob_start + lt / tpp;
  const int tt = lt % tpp;
  int tm, tn;
  TDG_F8_TILE_RASTER(tt, cl.tiles_m, cl.tiles_n, tm, tn)
  const uint8_t* __restrict__ A = args.A[pr];
  const uint8_t* __restrict__ B = args.B[pr];
  const int m0 = tm * 256, n0 = tn * 256;
  const int nk = T / 128;  // host guarantees T % 128 == 0

  // DMA pieces: per half image 16 pieces of 8 token rows x 128 B; wave wid
  // issues pieces 4 wid .. 4 wid + 3. Lane: token row 8 piece + lane / 8,
  // chunk position lane % 8 <- operand chunk (lane % 8) ^ sw(row)
  uint32_t aoff[2][4], boff[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (wid * 4 + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ wf8::sw(row);
      const int x = c * 16;
      int ma = m0 + f8w1::remap(x, h), nb = n0 + f8w1::remap(x, h);
      ma = ma + 16 <= M ? ma : 0;  // past the operand: never stored (M % 16 == 0)
      nb = nb + 16 <= N ? nb : 0;
      aoff[h][i] = (uint32_t)row * (uint32_t)lda + (uint32_t)ma;
      boff[h][i] = (uint32_t)row * (uint32_t)ldb + (uint32_t)nb;
    }
  // half q of tile kt: 0 = A0, 1 = B0, 2 = B1, 3 = A1 (issue order)
  auto issue = [&](int kt, int q) {
    char* st = smem + (kt & 1) * SB;
    const bool isA = q == 0 || q == 3;
    const int h = (q == 0 || q == 1) ? 0 : 1;
    char* dst = st + (isA ? h : 2 + h) * HB;
    const size_t trow = (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* src = isA ? A + trow * lda + aoff[h][i] : B + trow * ldb + boff[h][i];
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + (wid * 4 + i) * 1024),
                                       16, 0, 0);
    }
  };

  f32x4 acc[TM][TN];
  TDG_F8_ZERO_ACC(TM, TN, acc)
  i32x8 fa[TM], fb[TN];
  const int ar = wm * 64, br = wn * 64;

  // swapped operands: lane holds 4 consecutive n of one m (16-byte stores)
  auto mfma = [&](int i, int j) {
    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[i][j], 0, 1,
                                                                 0, 127, 0, 127);
  };
  TDG_F8_FOUR_PHASE_K_LOOP(wf8::frag, mfma, issue)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // epilogue: acc[i][j] lane holds dW[m = mw + 16 i + (lane & 15)][n = nw + 16 j + 4 (lane >> 4) .. +3]
  const float alpha = 1.f / (args.sa[pr][0] * args.sb[pr][0]);
  float* __restrict__ Cp = args.C[pr];
  const int mw = m0 + wm * 128, nw = n0 + wn * 128;
  const int cl16 = lane & 15, g4 = 4 * (lane >> 4);
  const bool vec = (ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(Cp) & 15) == 0;
  // write-through (sc1): the gradients are read by Adam, not by this XCD
  const WtBuf wc(Cp, ((size_t)(M - 1) * ldc + N) * sizeof(float));
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = mw + 16 * i + cl16;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nw + 16 * j + g4;
      float* c = Cp + (size_t)m * ldc + n;
      f32x4 v = acc[i][j] * alpha;
      if (vec && n + 4 <= N) {
        if (beta != 0.f) v += beta * *reinterpret_cast<const f32x4*>(c);
        wc.st16(c, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < N) c[e] = v[e] + (beta != 0.f ? beta * c[e] : 0.f);
      }
    }
  }
}

}  // namespace tdg

using namespace tdg;

// fp8 weight gradients (wgrad_fp8_kernel): P <= 64 problems sharing the token
// count T (T % 128 == 0), consecutive problems of equal shape form a class
// (<= 8 classes). shapes[5 i ..] = (M, N, lda, ldb, ldc); A[i] e5m2 [T][lda],
// B[i] e4m3 [T][ldb], C[i] f32 [M][ldc]; sa / sb: one-float scales.
extern "C" int tdg_wgrad_fp8(const void* const* A, const void* const* B, float* const* C,
                             const float* const* sa, const float* const* sb, int P,
                             const int* shapes, int T, float beta, hipStream_t st) {
  if (P < 1 || P > WF8_MAXP || T <= 0 || T % 128) return -2;
  WF8Args args{};
  int ncls = 0, tiles = 0;
  for (int i = 0; i < P; ++i) {
    const int* s = shapes + 5 * i;
    const int M = s[0], N = s[1], lda = s[2], ldb = s[3], ldc = s[4];
    if (M <= 0 || N <= 0 || M % 16 || N % 16 || lda % 16 || ldb % 16 || lda < M || ldb < N)
      return -3;
    if ((long long)T * lda >= (1LL << 31) || (long long)T * ldb >= (1LL << 31)) return -9;
    const bool same = ncls > 0 && args.cls[ncls - 1].M == M && args.cls[ncls - 1].N == N &&
                      args.cls[ncls - 1].lda == lda && args.cls[ncls - 1].ldb == ldb &&
                      args.cls[ncls - 1].ldc == ldc;
    if (!same) {
      if (ncls == WF8_MAXC) return -5;
      WF8Class& c = args.cls[ncls++];
      c.M = M; c.N = N; c.lda = lda; c.ldb = ldb; c.ldc = ldc;
      c.tiles_m = cdiv(M, 256); c.tiles_n = cdiv(N, 256);
      c.tile_start = tiles; c.prob_start = i;
    }
    tiles += cdiv(M, 256) * cdiv(N, 256);
    args.A[i] = (const uint8_t*)A[i];
    args.B[i] = (const uint8_t*)B[i];
    args.C[i] = C[i];
    args.sa[i] = sa[i];
    args.sb[i] = sb[i];
  }
  args.ncls = ncls;
  constexpr int lds = 2 * 4 * f8w1::HB;
  big_lds<wgrad_fp8_kernel>();
  hipLaunchKernelGGL(wgrad_fp8_kernel, dim3(tiles), dim3(256), lds, st, args, T, beta);
  return 0;
}
