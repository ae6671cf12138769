// The fp8 GEMM epilogue: ids and flags of tdg_gemm_fp8's `epi`, the backward
// extras, and F8Epi (dequant, bias, ReLU / ReLU backward, beta, the bf16
// output, its fp8 copy with amax, column sums).
#pragma once
#include "fp8_impl.h"

namespace tdg {

// fp8 GEMM epilogue stores write-through (sc1): see F8Epi::run_w
#ifndef TDG_F8_EPI_SC1
#define TDG_F8_EPI_SC1 1
#endif
constexpr bool F8_EPI_SC1 = TDG_F8_EPI_SC1 != 0;

enum { F8_EPI_NONE = 0, F8_EPI_BIAS = 1, F8_EPI_BIAS_RELU = 2, F8_EPI_DRELU = 3, F8_EPI_DRELU8 = 4 };
// (F8_EPI_DRELU8: the ReLU-backward mask from F8Extra::aux8, host-selected)
// flag on top of the epilogue id: C = dequant(C8) (needs C8)
constexpr int F8_EPI_CDEQ = 16;
// host-side flag of tdg_gemm_fp8's epi: B is N-contiguous ([K][ldb], e.g. a
// weight [out][in] as the B operand of its dgrad; 128x128 tile only)
constexpr int F8_B_NCONTIG = 32;
// host-side flag: leave the column-sum partials (colsum_out) in ws unfolded
// -- the caller folds them later with other deferred reductions
constexpr int F8_CS_DEFER = 64;

// Backward-GEMM extras: the ReLU mask operand (F8_EPI_DRELU: out = 0 where
// aux <= 0) and C = alpha A B^T + beta C.
struct F8Extra {
  const bf16_t* aux;
  int ldaux;
  float beta;
  int cdeq;  // C = dequant(C8) instead of the unrounded value (epi flag F8_EPI_CDEQ)
  // ReLU-backward mask from an 8-bit copy of the activation (aux8 != 0 <=> the
  // e4m3 ReLU output is positive) instead of the bf16 aux
  const uint8_t* aux8;
  // column-sum partials of the stored (bf16-rounded) output: row tm * WM + wm
  // of colsum[rows][N] per wave row of each tile (the bias gradient of the
  // layer whose output gradient this is; folded by the host launcher)
  float* colsum;
};

// Epilogue: dequant, bias, relu -> per-wave bf16 LDS image -> 16-byte
// stores (ReLU-backward mask and beta applied per 8-column chunk) + the
// optional fp8 copy (format CF) and its amax. Called after a barrier that
// ends every wave's reads of the pipeline stages.
// PRE_OK: prefetch the ReLU mask / old C of every chunk before the image is
// written (off for the 256x256 one-wave tiles: 32 chunks per lane would not
// fit in registers; those load per chunk instead)
// (wimg_at / red_at: this wave's image and the amax scratch at given LDS
// addresses instead of smem + wid * image bytes / after the images -- the
// persistent kernel places them around the stage holding the next tile's
// first K step)
template <int BM, int BN, int WM, int WN, int EPI, int CF = 0, bool PRE_OK = true>
struct F8Epi {
  static constexpr int NW = WM * WN, TM = BM / WM / 16, TN = BN / WN / 16;
  static constexpr int WTM = BM / WM, WTN = BN / WN;
  static constexpr int SROW = WTN * 2 + 16;
  static constexpr int WIMG = WTM * SROW;  // bytes of one wave's image
  static constexpr int CPR = WTN / 8;
  static constexpr int LDS = NW * WTM * SROW + 64;  // images + amax scratch
  // the ReLU mask / old C of every chunk a lane stores, loaded into registers
  // by prefetch() BEFORE the main loop (the caller issues it ahead of the
  // first LDS-DMA): loaded in the epilogue, their latency sat exposed once per
  // tile round (the ReLU-backward dgrad 8192x4096x1024: ~30 us of ~90)
  static constexpr int ITER = (WTM * CPR) / 64;
  static constexpr bool DR = EPI == F8_EPI_DRELU || EPI == F8_EPI_DRELU8;  // ReLU backward
  static constexpr bool A8 = EPI == F8_EPI_DRELU8;                          // 8-bit mask
  static constexpr bool PRE = DR && PRE_OK;
  // (the old C of a beta != 0 ReLU-backward GEMM is loaded in the epilogue:
  // kept out of the prefetch so the kernel stays at two waves per SIMD)
  // bias of the lane's TN columns (the 16x16 path, run()): loaded with the
  // other prefetches ahead of the first DMA -- read in the epilogue, its
  // vmcnt wait also waited for every younger DMA (the persistent kernel's
  // next-tile stage issued before the epilogue)
  static constexpr bool HASB = (EPI == F8_EPI_BIAS || EPI == F8_EPI_BIAS_RELU) && PRE_OK;
  struct Pre {
    int4 aux[PRE && !A8 ? ITER : 1];  // bf16 mask chunk
    uint2 aux8[PRE && A8 ? ITER : 1];  // 8 mask bytes
    float bn[HASB ? TN : 1];
  };
  static __device__ __forceinline__ bool vec_ok(int ldc, const F8Extra& ex) {
    return (ldc & 7) == 0 && (!DR || (ex.ldaux & 7) == 0);
  }
  // (the bf16 mask is prefetched at the start of the epilogue instead: 32
  // more registers across the main loop would cost the second wave per SIMD)
  template <bool LOADB = true>
  static __device__ __forceinline__ void prefetch(Pre& pre, const bf16_t* __restrict__ C, int M, int N,
                                                  int ldc, int m0, int n0, int wid, int lane,
                                                  const F8Extra& ex, const float* __restrict__ bias) {
    if constexpr (HASB && LOADB) {
      const int wn = wid % WN, cl = lane & 15;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + 16 * j + cl;
        pre.bn[j] = bias[n < N ? n : N - 1];
      }
    }
    if constexpr (PRE && A8) {
      const int wm = wid / WN, wn = wid % WN;
      const bool vok = vec_ok(ldc, ex);
#pragma unroll
      for (int tt = 0; tt < ITER; ++tt) {
        const int id = lane + 64 * tt;
        const int row = id / CPR, ch = id % CPR;
        const int m = m0 + wm * WTM + row;
        const int n = n0 + wn * WTN + ch * 8;
        if constexpr (A8) pre.aux8[tt] = uint2{0u, 0u};
        else pre.aux[tt] = int4{0, 0, 0, 0};
        if (vok && m < M && n + 8 <= N) {
          if constexpr (A8)
            pre.aux8[tt] = *reinterpret_cast<const uint2*>(ex.aux8 + (size_t)m * ex.ldaux + n);
          else
            pre.aux[tt] = *reinterpret_cast<const int4*>(ex.aux + (size_t)m * ex.ldaux + n);
        }
      }
    }
  }
  // the 16x16 MFMA accumulators (acc[i][j] of the wave's WTM x WTN tile)
  static __device__ __forceinline__ void run(char* smem, const f32x4 (&acc)[TM][TN],
                                             bf16_t* __restrict__ C, const float* __restrict__ bias,
                                             const float* __restrict__ sa,
                                             const float* __restrict__ sb, uint8_t* __restrict__ C8,
                                             const float* __restrict__ sc8,
                                             unsigned* __restrict__ amax_out, int M, int N, int ldc,
                                             int ldc8, int m0, int n0, int wid, int lane, int tid,
                                             const F8Extra& ex, const Pre& pre, float* red_at = nullptr,
                                             char* wimg_at = nullptr) {
    const int g = lane >> 4, cl = lane & 15, wn = wid % WN;
    run_w(
        [&](char* wimg, float alpha) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WTN + 16 * j + cl;
            float bn = 0.f;
            if constexpr (HASB) bn = pre.bn[j];
            else if constexpr (EPI == F8_EPI_BIAS || EPI == F8_EPI_BIAS_RELU) bn = bias[n < N ? n : N - 1];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float v = alpha * acc[i][j][r] + bn;
                if constexpr (EPI == F8_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
                *reinterpret_cast<bf16_t*>(wimg + (16 * i + 4 * g + r) * SROW + (16 * j + cl) * 2) = f2bf(v);
              }
          }
        },
        smem, C, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex, pre, red_at,
        wimg_at);
  }
  // the 32x32 MFMA accumulators (acc[i][j]: rows 32 i .., columns 32 j .. of the wave's tile)
  static __device__ __forceinline__ void run32(char* smem, const f32x16 (&acc)[WTM / 32][WTN / 32],
                                               bf16_t* __restrict__ C, const float* __restrict__ bias,
                                               const float* __restrict__ sa,
                                               const float* __restrict__ sb, uint8_t* __restrict__ C8,
                                               const float* __restrict__ sc8,
                                               unsigned* __restrict__ amax_out, int M, int N, int ldc,
                                               int ldc8, int m0, int n0, int wid, int lane, int tid,
                                               const F8Extra& ex, const Pre& pre, float* red_at = nullptr) {
    const int h = lane >> 5, cl = lane & 31, wn = wid % WN;
    run_w(
        [&](char* wimg, float alpha) {
#pragma unroll
          for (int j = 0; j < WTN / 32; ++j) {
            const int n = n0 + wn * WTN + 32 * j + cl;
            float bn = 0.f;
            if constexpr (EPI == F8_EPI_BIAS || EPI == F8_EPI_BIAS_RELU) bn = bias[n < N ? n : N - 1];
#pragma unroll
            for (int i = 0; i < WTM / 32; ++i)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                float v = alpha * acc[i][j][r] + bn;
                if constexpr (EPI == F8_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
                const int row = 32 * i + 8 * (r >> 2) + 4 * h + (r & 3);
                *reinterpret_cast<bf16_t*>(wimg + row * SROW + (32 * j + cl) * 2) = f2bf(v);
              }
          }
        },
        smem, C, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex, pre, red_at,
        nullptr);
  }
  // write_img(wimg, alpha): the wave's dequantised (bias, ReLU) bf16 tile into its image
  template <class W>
  static __device__ __forceinline__ void run_w(W&& write_img, char* smem, bf16_t* __restrict__ C,
                                               const float* __restrict__ sa,
                                               const float* __restrict__ sb, uint8_t* __restrict__ C8,
                                               const float* __restrict__ sc8,
                                               unsigned* __restrict__ amax_out, int M, int N, int ldc,
                                               int ldc8, int m0, int n0, int wid, int lane, int tid,
                                               const F8Extra& ex, const Pre& pre, float* red_at,
                                               char* wimg_at) {
    const int wm = wid / WN, wn = wid % WN;
    const float alpha = 1.f / (sa[0] * sb[0]);
    const float s8 = C8 ? sc8[0] : 0.f;
    char* wimg = wimg_at ? wimg_at : smem + wid * WIMG;
    static_assert(64 % CPR == 0, "a lane keeps its column chunk across iterations");
    short8_t pre_aux[PRE && !A8 ? ITER : 1];
    const bool vec_ok = F8Epi::vec_ok(ldc, ex);
    // write-through (sc1) output stores: nothing left dirty in the XCD's L2
    // for the kernel-end write-back (as the bf16 GEMM epilogue, tdg_gemm.h)
    const WtBuf wc(C ? (const void*)C : (const void*)C8,
                   C ? ((size_t)(M - 1) * ldc + N) * sizeof(bf16_t) : 16);
    const WtBuf wc8(C8 ? (const void*)C8 : (const void*)C, C8 ? (size_t)(M - 1) * ldc8 + N : 16);
    float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (PRE) {
#pragma unroll
      for (int tt = 0; tt < ITER; ++tt) {
        if constexpr (A8) {
          // (raw mask bytes stay in pre.aux8: applied packed, below)
        } else {
          const int id = lane + 64 * tt;
          const int row = id / CPR, ch = id % CPR;
          const int m = m0 + wm * WTM + row;
          const int n = n0 + wn * WTN + ch * 8;
          pre_aux[tt] = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
          if (vec_ok && m < M && n + 8 <= N)
            pre_aux[tt] = *reinterpret_cast<const short8_t*>(ex.aux + (size_t)m * ex.ldaux + n);
        }
      }
    }
    write_img(wimg, alpha);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float amax = 0.f;
#pragma unroll
    for (int tt = 0; tt < (WTM * CPR) / 64; ++tt) {
      const int id = lane + 64 * tt;
      const int row = id / CPR, ch = id % CPR;
      const int m = m0 + wm * WTM + row;
      const int n = n0 + wn * WTN + ch * 8;
      if (m >= M || n >= N) continue;
      short8_t v = *reinterpret_cast<const short8_t*>(wimg + row * SROW + ch * 16);
      const bool vec = n + 8 <= N && vec_ok;
      if constexpr (A8) {
        if (vec) {
          // packed 8-bit mask: each mask byte -> 0 / 0xffff over its bf16
          // half (no bf16 -> f32 -> bf16 round trip: the per-element form
          // cost this epilogue ~20 us on 8192 x 4096)
          uint2 mb;
          if constexpr (PRE) mb = pre.aux8[tt];
          else mb = *reinterpret_cast<const uint2*>(ex.aux8 + (size_t)m * ex.ldaux + n);
          uint32_t bx = mb.x, by = mb.y;
          bx |= bx >> 4; bx |= bx >> 2; bx |= bx >> 1; bx &= 0x01010101u;
          by |= by >> 4; by |= by >> 2; by |= by >> 1; by &= 0x01010101u;
          u32x4_t dw = __builtin_bit_cast(u32x4_t, v);
          dw[0] &= __builtin_amdgcn_perm(0u, bx, 0x0c010c00u) * 0xffffu;
          dw[1] &= __builtin_amdgcn_perm(0u, bx, 0x0c030c02u) * 0xffffu;
          dw[2] &= __builtin_amdgcn_perm(0u, by, 0x0c010c00u) * 0xffffu;
          dw[3] &= __builtin_amdgcn_perm(0u, by, 0x0c030c02u) * 0xffffu;
          v = __builtin_bit_cast(short8_t, dw);
        }
      }
      if ((DR && !(A8 && vec)) || ex.beta != 0.f) {
        // 16-byte mask / old-C loads for whole aligned chunks (8 scalar
        // 2-byte loads per chunk made the ReLU-backward GEMM 2.4x slower)
        short8_t mk = v, old = v;
        if (vec) {
          if constexpr (PRE && !A8) {
            mk = pre_aux[tt];
          } else if constexpr (DR && !A8) {
            mk = *reinterpret_cast<const short8_t*>(ex.aux + (size_t)m * ex.ldaux + n);
          }
          if (ex.beta != 0.f) old = *reinterpret_cast<const short8_t*>(C + (size_t)m * ldc + n);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (!vec && n + e >= N) break;
          float f = bf2f((bf16_t)v[e]);
          if constexpr (DR) {
            float a;
            if constexpr (A8) a = vec ? 1.f : (ex.aux8[(size_t)m * ex.ldaux + n + e] ? 1.f : 0.f);
            else a = vec ? bf2f((bf16_t)mk[e]) : bf2f(ex.aux[(size_t)m * ex.ldaux + n + e]);
            if (!(a > 0.f)) f = 0.f;  // (A8, vec: already masked above)
          }
          if (ex.beta != 0.f)
            f += ex.beta * (vec ? bf2f((bf16_t)old[e]) : bf2f(C[(size_t)m * ldc + n + e]));
          v[e] = (short)f2bf(f);
        }
      }
      if (ex.colsum) {
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[e] += bf2f((bf16_t)v[e]);  // (columns past N: never stored)
      }
      int lo = 0, hi = 0;
      if (C8) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          f[e] = bf2f((bf16_t)v[e]);
          amax = fmaxf(amax, fabsf(f[e]));
        }
        f8::quant8<CF>(f, s8, lo, hi);
        if (ex.cdeq) {
          // C = dequant(C8): the bf16 output carries exactly the values the
          // fp8 consumer sees (power-of-two scales: exact in bf16), so a
          // backward that reads C differentiates the forward that ran
          const float inv = 1.f / s8;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = (short)f2bf(f8::unpack_f8<CF>(lo, e) * inv);
            v[e + 4] = (short)f2bf(f8::unpack_f8<CF>(hi, e) * inv);
          }
        }
      }
      if (C) {
        if (n + 8 <= N) {
          if constexpr (F8_EPI_SC1) wc.st16(C + (size_t)m * ldc + n, v);
          else *reinterpret_cast<short8_t*>(C + (size_t)m * ldc + n) = v;
        } else {
          for (int e = 0; e < 8 && n + e < N; ++e) C[(size_t)m * ldc + n + e] = (bf16_t)v[e];
        }
      }
      if (C8) {
        if (n + 8 <= N) {
          if constexpr (F8_EPI_SC1) wc8.st8(C8 + (size_t)m * ldc8 + n, make_int2(lo, hi));
          else *reinterpret_cast<int2*>(C8 + (size_t)m * ldc8 + n) = make_int2(lo, hi);
        } else {
          for (int e = 0; e < 8 && n + e < N; ++e)
            C8[(size_t)m * ldc8 + n + e] = f8::quant8_byte(lo, hi, e);
        }
      }
    }
    if (ex.colsum) {  // lanes with equal lane % CPR hold the same columns
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[e] += __shfl_xor(csum[e], o, 64);
      const int n = n0 + wn * WTN + (lane % CPR) * 8;
      float* prow = ex.colsum + (size_t)((m0 / BM) * WM + wm) * N;
      if (lane < CPR) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (n + e < N) prow[n + e] = csum[e];
      }
    }
    if (C8 && amax_out) {  // one atomic per workgroup, spread over AMAX_SPREAD words
      amax = wave_max(amax);
      float* red = red_at ? red_at : reinterpret_cast<float*>(smem + NW * WTM * SROW);
      if (lane == 0) red[wid] = amax;
      __syncthreads();
      if (tid == 0) {
        float m = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) m = fmaxf(m, red[w]);
        f8::atomic_amax(amax_word(amax_out, blockIdx.x), m);
      }
    }
  }
};

}  // namespace tdg
