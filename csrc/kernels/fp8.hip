// FP8 (OCP e4m3) forward GEMM and quantization for gfx950.
//
//   C[m,n] = act( (sum_k A8[m,k] * B8[n,k]) / (sa * sb) + bias[n] )      (bf16 out)
//   optional C8 = e4m3(C * sc8), amax(C) -> amax_out   (fp8 copy for the next GEMM)
//
// A8 = e4m3(A * sa) and B8 = e4m3(B * sb) are per-tensor scaled copies of the
// bf16 activations / weights; the scales live in device memory (delayed
// scaling: each producer records the amax of what it quantised, and
// fp8_scale_update turns last step's amax into this step's scale), so a
// captured HIP graph stays valid across steps.
//
// MFMA: v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 block scales -- the
// per-tensor scales are applied in the epilogue. Lane l holds
// A[row l&15][k 32(l>>4) .. +31] and B[k 32(l>>4) .. +31][col l&15] (verified
// with exact integer data: scripts/probes/fp8_mfma_layout.hip); C/D layout as
// every 16x16 MFMA on gfx950 (col l&15, row 4(l>>4)+r). One instruction per
// 128-deep K tile = twice the bf16 16x16x32 rate per clock, and half the bytes
// staged through LDS.
//
// Staging is the bf16 kernel's (csrc/kernels/gemm.hip): LDS-DMA
// (global_load_lds_dwordx4) into 128-byte-row images with the same 32-byte
// XOR swizzle, STAGES tiles in flight, counted vmcnt + raw s_barrier.
//
// Replaces (in the fp8 configuration, BASELINE config 5) the forward Dense
// MatMuls of the reference (distributed_training_transformer/
// transformer_model.py:119-122, 165, 172-174); backward stays bf16.
#include "tdg_api.h"
#include "tdg_common.h"
#include "tdg_reduce.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace tdg {

typedef int i32x8 __attribute__((ext_vector_type(8)));
// E4M3_MAX, AMAX_SPREAD, pack2_e4m3, atomic_amax: tdg_common.h (each amax slot
// is AMAX_SPREAD words; producers pick one by block id so the atomics of a
// large grid do not serialise on one address)
constexpr int BK8 = 128;  // K elements (= bytes) per tile row
// fp8 GEMM epilogue stores write-through (sc1): see F8Epi::run_w
#ifndef TDG_F8_EPI_SC1
#define TDG_F8_EPI_SC1 1
#endif
constexpr bool F8_EPI_SC1 = TDG_F8_EPI_SC1 != 0;

namespace f8 {

__device__ __forceinline__ int lds_off(int row, int byte) {
  const int seg = (byte >> 5) ^ ((row >> 1) & 3);
  return row * BK8 + (seg << 5) + (byte & 31);
}

// global -> LDS staging of an R x 128-byte K-contiguous tile (as Glds<KC> in gemm.hip)
template <int R, int NW>
struct Stage {
  static constexpr int BYTES = R * BK8;
  static constexpr int P = BYTES / (NW * 1024);
  static_assert(BYTES % (NW * 1024) == 0, "tile must split into 1 KiB pieces per wave");
  int row[P], col[P];
  __device__ __forceinline__ void init(int wid, int lane) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int j = wid * P + i;
      const int r = j * 8 + lane / 8;
      const int pc = lane % 8;
      const int c = (((pc >> 1) ^ ((r >> 1) & 3)) << 1) | (pc & 1);
      row[i] = r;
      col[i] = c * 16;
    }
  }
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ X, int ld, int len, int mn0,
                                        int k0, char* lds, int wid) const {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      int mn = mn0 + row[i];
      mn = mn < len ? mn : len - 1;
      const long long off = (long long)mn * ld + k0 + col[i];
      __builtin_amdgcn_global_load_lds(
          (const void*)(X + off),
          (__attribute__((address_space(3))) void*)(lds + (wid * P + i) * 1024), 16, 0, 0);
    }
  }
};

// 32-byte operand fragment: row base + (lane&15), bytes 32(lane>>4) .. +31
__device__ __forceinline__ i32x8 frag(const char* lds, int base, int lane) {
  const int row = base + (lane & 15);
  const int g = lane >> 4;
  // untracked reads (tdg_common.h): a tracked LDS read after an LDS-DMA issue
  // gets an s_waitcnt vmcnt(0) that drains the next tile's prefetch
  const int4 lo = __builtin_bit_cast(int4, tdg::lds_read_b128_async(lds + lds_off(row, 32 * g)));
  const int4 hi = __builtin_bit_cast(int4, tdg::lds_read_b128_async(lds + lds_off(row, 32 * g + 16)));
  return i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

using tdg::atomic_amax;
using tdg::pack2_e4m3;

// OCP e5m2 (gfx950 bf8): the gradient format of the fp8 backward
constexpr float E5M2_MAX = 57344.f;
template <bool HI>
__device__ __forceinline__ int pack2_e5m2(float a, float b, int old) {
  a = fminf(fmaxf(a, -E5M2_MAX), E5M2_MAX);
  b = fminf(fmaxf(b, -E5M2_MAX), E5M2_MAX);
  return __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
}
// byte `sel` (0..3) of a packed word, decoded (FMT 0: e4m3, 1: e5m2)
template <int FMT>
__device__ __forceinline__ float unpack_f8(int w, int sel) {
  if constexpr (FMT == 0) {
    switch (sel) {
      case 0: return __builtin_amdgcn_cvt_f32_fp8(w, 0);
      case 1: return __builtin_amdgcn_cvt_f32_fp8(w, 1);
      case 2: return __builtin_amdgcn_cvt_f32_fp8(w, 2);
      default: return __builtin_amdgcn_cvt_f32_fp8(w, 3);
    }
  } else {
    switch (sel) {
      case 0: return __builtin_amdgcn_cvt_f32_bf8(w, 0);
      case 1: return __builtin_amdgcn_cvt_f32_bf8(w, 1);
      case 2: return __builtin_amdgcn_cvt_f32_bf8(w, 2);
      default: return __builtin_amdgcn_cvt_f32_bf8(w, 3);
    }
  }
}
// FMT 0: e4m3, 1: e5m2
template <int FMT, bool HI>
__device__ __forceinline__ int pack2_f8(float a, float b, int old) {
  if constexpr (FMT == 0) return pack2_e4m3<HI>(a, b, old);
  else return pack2_e5m2<HI>(a, b, old);
}

}  // namespace f8

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
        lo = f8::pack2_f8<CF, false>(f[0] * s8, f[1] * s8, 0);
        lo = f8::pack2_f8<CF, true>(f[2] * s8, f[3] * s8, lo);
        hi = f8::pack2_f8<CF, false>(f[4] * s8, f[5] * s8, 0);
        hi = f8::pack2_f8<CF, true>(f[6] * s8, f[7] * s8, hi);
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
          // (bytes by shifts: taking &lo / &hi put them in scratch memory)
          for (int e = 0; e < 8 && n + e < N; ++e)
            C8[(size_t)m * ldc8 + n + e] = (uint8_t)((uint32_t)(e < 4 ? lo : hi) >> (8 * (e & 3)));
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

// AF: format of A (0 e4m3, 1 e5m2: the gradient operand of a dgrad), B is
// e4m3; CF: format of the optional C8 copy.
namespace wf8 {
__device__ __forceinline__ int sw(int t) { return ((t >> 1) & 3) | (((t >> 5) & 1) << 2); }
// byte offset of (token row t, image column x) in a [128][128 B] half image
__device__ __forceinline__ int off(int t, int x) { return t * 128 + ((((x >> 4) ^ sw(t)) & 7) << 4) + (x & 15); }
// transposing 8-byte read (untracked: the caller waits with lgkmcnt)
__device__ __forceinline__ uint64_t tr8(const void* p) {
  uint64_t r;
  const uint32_t a = (uint32_t)(uintptr_t)p;
  asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(r) : "v"(a) : "memory");
  return r;
}
// MFMA fragment of image columns base..base+15 (one per lane & 15), tokens
// 32 (lane >> 4) .. +31: four transposing reads of 8 tokens
__device__ __forceinline__ i32x8 frag(const char* img, int base, int lane) {
  const int g = lane >> 4, w = lane & 15, q = w >> 1, p = w & 1;
  uint64_t r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = 32 * g + 8 * j + q;
    r[j] = tr8(img + off(t, base + 8 * p));
  }
  return i32x8{(int)r[0], (int)(r[0] >> 32), (int)r[1], (int)(r[1] >> 32),
               (int)r[2], (int)(r[2] >> 32), (int)r[3], (int)(r[3] >> 32)};
}
}  // namespace wf8

// global -> LDS staging of a 128 (K) x 128-byte (N) tile of an N-CONTIGUOUS
// operand ([K][ld]: a weight [out][in] read as the B operand of its dgrad,
// B(n, k) = W[k][n]) into the wf8 image (16-byte chunk c of row t at chunk
// c ^ wf8::sw(t)); fragments come from wf8::frag (ds_read_b64_tr_b8), so the
// dgrad needs no transposed weight copy. NW = 4 waves, 4 pieces of 8 rows
// x 128 B each.
template <int NW>
struct StageT {
  static constexpr int P = 16 / NW;
  static_assert(P * NW == 16, "16 pieces of 1 KiB per 16 KiB image");
  uint32_t off[P];
  __device__ __forceinline__ void init(int wid, int lane, int n0, int N, int ld) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int row = (wid * P + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ wf8::sw(row);
      int n = n0 + 16 * c;
      n = n + 16 <= N ? n : 0;  // past the operand: never stored (N % 16 == 0)
      off[i] = (uint32_t)row * (uint32_t)ld + (uint32_t)n;
    }
  }
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ X, int ld, int k0, char* lds,
                                        int wid) const {
#pragma unroll
    for (int i = 0; i < P; ++i)
      __builtin_amdgcn_global_load_lds(
          (const void*)(X + (size_t)k0 * ld + off[i]),
          (__attribute__((address_space(3))) void*)(lds + (wid * P + i) * 1024), 16, 0, 0);
  }
};

template <int BM, int BN, int WM, int WN, int STAGES, int EPI, int AF = 0, int CF = 0,
          bool BT = false>
__global__ __launch_bounds__(WM* WN * 64) void gemm_fp8_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, bf16_t* __restrict__ C,
    const float* __restrict__ bias, const float* __restrict__ sa, const float* __restrict__ sb,
    uint8_t* __restrict__ C8, const float* __restrict__ sc8, unsigned* __restrict__ amax_out,
    int M, int N, int K, int lda, int ldb, int ldc, int ldc8, F8Extra ex) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int A_BYTES = BM * BK8, B_BYTES = BN * BK8, SB = A_BYTES + B_BYTES;
  using GA = f8::Stage<BM, NW>;
  // BT: B is N-contiguous ([K][ldb], StageT + transposing fragment reads)
  static_assert(!BT || (BN == 128 && NW == 4), "N-contiguous B: 128-column tiles on 4 waves");
  using GB = typename std::conditional<BT, StageT<NW>, f8::Stage<BN, NW>>::type;
  constexpr int PT = GA::P + GB::P;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int tiles_m = cdiv(M, BM), tiles_n = cdiv(N, BN);
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  int tm, tn;
  if (tiles_n <= tiles_m) {
    tn = t % tiles_n;
    tm = t / tiles_n;
  } else {
    tm = t % tiles_m;
    tn = t / tiles_m;
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = K / BK8;  // host guarantees K % 128 == 0

  using Epi = F8Epi<BM, BN, WM, WN, EPI, CF>;
  typename Epi::Pre pre;
  Epi::prefetch(pre, C, M, N, ldc, m0, n0, wid, lane, ex, bias);  // (older than every DMA)
  GA ga;
  GB gb;
  ga.init(wid, lane);
  if constexpr (BT) gb.init(wid, lane, n0, N, ldb);
  else gb.init(wid, lane);
  auto issue_b = [&](int k0, char* dst) {
    if constexpr (BT) gb.issue(B, ldb, k0, dst, wid);
    else gb.issue(B, ldb, N, n0, k0, dst, wid);
  };
  auto frag_b = [&](const char* img, int base) {
    if constexpr (BT) return wf8::frag(img, base, lane);
    else return f8::frag(img, base, lane);
  };
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < STAGES; ++s)
    if (s < nk) {
      ga.issue(A, lda, M, m0, s * BK8, smem + s * SB, wid);
      issue_b(s * BK8, smem + s * SB + A_BYTES);
    }
  if (nk >= STAGES) f8::wait_vmcnt<(STAGES - 1) * PT>();
  else f8::wait_vmcnt<0>();
  f8::lds_barrier();
  const int abase = wm * (BM / WM), bbase = wn * (BN / WN);
  i32x8 fa[TM], fb[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) fa[i] = f8::frag(smem, abase + 16 * i, lane);
#pragma unroll
  for (int j = 0; j < TN; ++j) fb[j] = frag_b(smem + A_BYTES, bbase + 16 * j);

  // MODE 2: tile kt + STAGES exists (steady, branch-free); 1: kt + 1 exists
  // (tail: drain, no issue); 0: the last tile. With the tail's branches
  // inside one loop body the compiler sank the MFMAs past the wait, barrier,
  // DMA issue and fragment reads into the latch (scripts/isa_loops.py).
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    tdg::lgkm_wait<0>();
#pragma unroll
    for (int i = 0; i < TM; ++i) tdg::tie(fa[i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) tdg::tie(fb[j]);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], AF,
                                                                     0, 0, 127, 0, 127);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MODE >= 1) {
      if constexpr (MODE == 2) f8::wait_vmcnt<(STAGES - 2) * PT>();
      else f8::wait_vmcnt<0>();
      f8::lds_barrier();
      if constexpr (MODE == 2) {
        char* ns = smem + (kt % STAGES) * SB;
        ga.issue(A, lda, M, m0, (kt + STAGES) * BK8, ns, wid);
        issue_b((kt + STAGES) * BK8, ns + A_BYTES);
      }
      const char* nx = smem + ((kt + 1) % STAGES) * SB;
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = f8::frag(nx, abase + 16 * i, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = frag_b(nx + A_BYTES, bbase + 16 * j);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  int kt = 0;
  for (; kt + STAGES < nk; ++kt) kstep(kt, std::integral_constant<int, 2>{});
#pragma unroll
  for (int d = 0; d < STAGES - 1; ++d)
    if (kt + 1 < nk) kstep(kt++, std::integral_constant<int, 1>{});
  kstep(kt, std::integral_constant<int, 0>{});

  f8::lds_barrier();
  Epi::run(smem, acc, C, bias, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex,
           pre);
}

// ---------------------------------------------------------------------------
// Persistent form of the 128x128 / 2x2-wave / 2-stage tile above: two
// workgroups per CU walk the tiles (dispatch positions blockIdx.x, + gridDim.x,
// ...; each position's tile -- and so its XCD -- as in the one-shot grid). At
// K = 1024 a tile round of the one-shot kernel is ~40 % fixed cost: the first
// stage's fill latency and the epilogue, with the MFMAs idle
// (scripts/fp8_ksweep.py: 5.5-7 us per round against 1.08 us per 128-deep K
// step). Here the next tile's K step 0 is issued into the stage the
// last-but-one K step vacated, the epilogue writes its swizzled, unpadded
// images into the stage the last K step
// vacated (waves 0-2; wave 3's image in a 9 KiB region past the stages: the
// padded images are 36 KiB), and the next tile's K step 1 goes there once
// the images are stored: the next tile's fill runs under this tile's epilogue.
template <int EPI, int AF = 0, int CF = 0, bool BT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void gemm_fp8_pk_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, bf16_t* __restrict__ C,
    const float* __restrict__ bias, const float* __restrict__ sa, const float* __restrict__ sb,
    uint8_t* __restrict__ C8, const float* __restrict__ sc8, unsigned* __restrict__ amax_out,
    int M, int N, int K, int lda, int ldb, int ldc, int ldc8, F8Extra ex) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2, NW = 4, TM = 4, TN = 4;
  constexpr int A_BYTES = BM * BK8, B_BYTES = BN * BK8, SB = A_BYTES + B_BYTES;
  using GA = f8::Stage<BM, NW>;
  using GB = typename std::conditional<BT, StageT<NW>, f8::Stage<BN, NW>>::type;
  constexpr int PT = GA::P + GB::P;
  using Epi = F8Epi<BM, BN, WM, WN, EPI, CF>;
  static_assert(3 * Epi::WIMG <= SB, "three wave images fit in a stage");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem + 2 * SB + Epi::WIMG);  // amax scratch

  const int tid = threadIdx.x;
  int lane = tid & 63;  // (re-defined opaquely per tile: see the loop head)
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int tiles_m = cdiv(M, BM), tiles_n = cdiv(N, BN), tiles = tiles_m * tiles_n;
  const int nk = K / BK8;  // host: K % 128 == 0, nk >= 2
  auto coords = [&](int pos, int& m0_, int& n0_) {
    const int t = xcd_remap(pos, tiles);
    int tm, tn;
    if (tiles_n <= tiles_m) {
      tn = t % tiles_n;
      tm = t / tiles_n;
    } else {
      tm = t % tiles_m;
      tn = t / tiles_m;
    }
    m0_ = tm * BM;
    n0_ = tn * BN;
  };
  int pos = blockIdx.x;
  int m0, n0;
  coords(pos, m0, n0);
  GA ga;
  ga.init(wid, lane);
  GB gb, gbn;  // (BT: the B offsets carry n0 -- the next tile's set in gbn)
  if constexpr (BT) gb.init(wid, lane, n0, N, ldb);
  else gb.init(wid, lane);
  auto issue = [&](const GB& g_, int m0_, int n0_, int k, char* dst) {
    ga.issue(A, lda, M, m0_, k * BK8, dst, wid);
    if constexpr (BT) g_.issue(B, ldb, k * BK8, dst + A_BYTES, wid);
    else g_.issue(B, ldb, N, n0_, k * BK8, dst + A_BYTES, wid);
  };
  auto frag_b = [&](const char* img, int base) {
    if constexpr (BT) return wf8::frag(img, base, lane);
    else return f8::frag(img, base, lane);
  };
  const int abase = wm * (BM / WM), bbase = wn * (BN / WN);

  typename Epi::Pre pre;
  Epi::prefetch(pre, C, M, N, ldc, m0, n0, wid, lane, ex, bias);  // (older than every DMA)
  issue(gb, m0, n0, 0, smem);
  issue(gb, m0, n0, 1, smem + SB);
  int sl0 = 0;  // stage of the current tile's K step 0
  for (;;) {
    // lane-derived addresses (epilogue image / store offsets, fragment
    // reads) are recomputed per tile: hoisted out of the tile loop they held
    // ~150 more registers across it and cost the second workgroup per CU
    asm volatile("" : "+v"(lane));
    const int posn = pos + (int)gridDim.x;
    const bool more = posn < tiles;  // (workgroup-uniform)
    int m0n = 0, n0n = 0;
    if (more) {
      coords(posn, m0n, n0n);
      if constexpr (BT) gbn.init(wid, lane, n0n, N, ldb);
      else gbn = gb;
    }
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K step 0 landed (younger: K step 1 -- and nothing else outstanding
    // is younger than step 0 but the epilogue stores / prefetch, waited too)
    f8::wait_vmcnt<PT>();
    f8::lds_barrier();
    i32x8 fa[TM], fb[TN];
    {
      const char* st0 = smem + sl0 * SB;
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = f8::frag(st0, abase + 16 * i, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = frag_b(st0 + A_BYTES, bbase + 16 * j);
    }
    // MODE 2: step kt + 2 exists (issue it into the vacated stage); 1: the
    // last-but-one step (issue the next tile's step 0 there); 0: the last
    auto kstep = [&](int kt, auto modec) {
      constexpr int MODE = decltype(modec)::value;
      tdg::lgkm_wait<0>();
#pragma unroll
      for (int i = 0; i < TM; ++i) tdg::tie(fa[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) tdg::tie(fb[j]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], AF,
                                                                       0, 0, 127, 0, 127);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (MODE >= 1) {
        f8::wait_vmcnt<0>();
        f8::lds_barrier();
        char* cur = smem + ((kt + sl0) & 1) * SB;
        if constexpr (MODE == 2) issue(gb, m0, n0, kt + 2, cur);
        else if (more) issue(gbn, m0n, n0n, 0, cur);
        const char* nx = smem + ((kt + 1 + sl0) & 1) * SB;
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = f8::frag(nx, abase + 16 * i, lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = frag_b(nx + A_BYTES, bbase + 16 * j);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    int kt = 0;
    for (; kt + 2 < nk; ++kt) kstep(kt, std::integral_constant<int, 2>{});
    kstep(kt++, std::integral_constant<int, 1>{});
    kstep(kt, std::integral_constant<int, 0>{});

    // epilogue images in the stage of the last K step (every wave's reads of
    // it completed before its last MFMAs; the barrier makes that all waves)
    char* img = smem + ((nk - 1 + sl0) & 1) * SB;
    f8::lds_barrier();
    Epi::run(img, acc, C, bias, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex,
             pre, red, wid < 3 ? img + wid * Epi::WIMG : smem + 2 * SB);
    if (!more) break;
    f8::lds_barrier();  // every wave's image reads done
    Epi::prefetch(pre, C, M, N, ldc, m0n, n0n, wid, lane, ex, bias);
    issue(gbn, m0n, n0n, 1, img);
    sl0 = (nk + sl0) & 1;
    pos = posn;
    m0 = m0n;
    n0 = n0n;
    gb = gbn;
  }
}

// ---------------------------------------------------------------------------
// 128x128 tile on 4 waves (64x64 each) on the 32x32x64 block-scaled MFMA, so
// one K step is 64 bytes: a ring of FIVE 16 KiB stages (an 8 KiB A image
// [128 rows][64 B] + an 8 KiB B image) per workgroup, two workgroups per CU
// (80 KiB each). Step j: wait for stage j, one barrier (stage j landed for
// every wave; stage j - 1 read by every wave), issue stage j + 4 into stage
// j - 1's slot, read the fragments, 4 MFMAs per wave. Every stage is issued
// FOUR steps (two 128-byte K steps) before it is read: 64 KiB per workgroup
// in flight across the load latency, against 32 KiB in gemm_fp8_kernel's
// 2-stage 128-byte loop, whose stage is read one step after its issue. The
// loop is bound by bytes in flight per CU (docs/PERF.md "Round 4").
// K-contiguous stage image: row R, 16-byte chunk c at chunk c ^ ((R >> 2) & 3):
// the four ds_read_b128 lane groups of a 32-row fragment read (rows R..R+31
// by lane & 31, chunk pair 2 (lane >> 5)) hit 16 distinct 16-byte slots each.
namespace f8r {
constexpr int IMG = 128 * 64;  // bytes of one operand stage image
constexpr int NS = 5;          // ring slots (each: A image + B image)
constexpr int SLOT = 2 * IMG;
__device__ __forceinline__ int off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }
// LDS-DMA of a [128 rows][64 B] K-slice of a K-contiguous operand: 8 pieces of
// 16 rows; wave wid issues pieces 2 wid, 2 wid + 1 (lane: row 16 piece +
// lane / 4, chunk position lane % 4 <- operand chunk (lane % 4) ^ ((row >> 2) & 3))
struct StageK {
  uint32_t off[2];
  __device__ __forceinline__ void init(int wid, int lane, int mn0, int len, int ld) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 16 + (lane >> 2);
      const int c = (lane & 3) ^ ((row >> 2) & 3);
      int mn = mn0 + row;
      mn = mn < len ? mn : len - 1;
      off[i] = (uint32_t)mn * (uint32_t)ld + (uint32_t)(c * 16);
    }
  }
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ X, int k0, char* lds, int wid) const {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(X + off[i] + k0),
                                       (__attribute__((address_space(3))) void*)(lds + (wid * 2 + i) * 1024),
                                       16, 0, 0);
  }
};
// N-contiguous stage image ([64 k-rows][128 n-bytes]): row t, 16-byte chunk c
// at chunk c ^ (2 ((t >> 1) & 3)): a transposing fragment read's 32-lane half
// (rows 8 j + q, q < 8; 32 columns: chunks c0, c0 + 1 with c0 even) lands
// on 32 distinct 8-byte slots
__device__ __forceinline__ int swn(int t) { return ((t >> 1) & 3) << 1; }
__device__ __forceinline__ int offn(int t, int x) { return t * 128 + ((((x >> 4) ^ swn(t)) & 7) << 4) + (x & 15); }
struct StageN {
  uint32_t off[2];
  __device__ __forceinline__ void init(int wid, int lane, int n0, int N, int ld) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swn(row);
      int n = n0 + 16 * c;
      n = n + 16 <= N ? n : 0;  // past the operand: never stored (N % 16 == 0)
      off[i] = (uint32_t)row * (uint32_t)ld + (uint32_t)n;
    }
  }
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ X, int ld, int k0, char* lds,
                                        int wid) const {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(X + (size_t)k0 * ld + off[i]),
                                       (__attribute__((address_space(3))) void*)(lds + (wid * 2 + i) * 1024),
                                       16, 0, 0);
  }
};
// 32x32x64 operand fragment of a K-contiguous image: row base + (lane & 31),
// K bytes 32 (lane >> 5) .. +31
__device__ __forceinline__ i32x8 frag(const char* img, int base, int lane) {
  const int row = base + (lane & 31), c = 2 * (lane >> 5);
  const int4 lo = __builtin_bit_cast(int4, tdg::lds_read_b128_async(img + off(row, c)));
  const int4 hi = __builtin_bit_cast(int4, tdg::lds_read_b128_async(img + off(row, c + 1)));
  return i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}
// ... of an N-contiguous image: column base + (lane & 31), K rows
// 32 (lane >> 5) .. +31 by four transposing reads of 8 rows (a 16-lane group
// reads 8 rows x 16 columns; lane w of it gets column w)
__device__ __forceinline__ i32x8 frag_t(const char* img, int base, int lane) {
  const int h = lane >> 5, cb = base + 16 * ((lane >> 4) & 1), w = lane & 15, q = w >> 1, p = w & 1;
  uint64_t r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = wf8::tr8(img + offn(32 * h + 8 * j + q, cb + 8 * p));
  return i32x8{(int)r[0], (int)(r[0] >> 32), (int)r[1], (int)(r[1] >> 32),
               (int)r[2], (int)(r[2] >> 32), (int)r[3], (int)(r[3] >> 32)};
}
}  // namespace f8r

template <int EPI, int AF = 0, int CF = 0, bool BT = false>
__global__ __launch_bounds__(256) void gemm_fp8_ring_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, bf16_t* __restrict__ C,
    const float* __restrict__ bias, const float* __restrict__ sa, const float* __restrict__ sb,
    uint8_t* __restrict__ C8, const float* __restrict__ sc8, unsigned* __restrict__ amax_out,
    int M, int N, int K, int lda, int ldb, int ldc, int ldc8, F8Extra ex) {
  constexpr int P = 4;  // LDS-DMA pieces per wave per stage (A 2 + B 2)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int tiles_m = cdiv(M, 128), tiles_n = cdiv(N, 128);
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  int tm, tn;
  if (tiles_n <= tiles_m) {
    tn = t % tiles_n;
    tm = t / tiles_n;
  } else {
    tm = t % tiles_m;
    tn = t / tiles_m;
  }
  const int m0 = tm * 128, n0 = tn * 128;
  const int ns = K / 64;  // 64-byte K steps (host: K % 128 == 0, so ns >= 2)

  using Epi = F8Epi<128, 128, 2, 2, EPI, CF>;
  typename Epi::Pre pre;
  // (run32 reads the bias itself)
  Epi::template prefetch<false>(pre, C, M, N, ldc, m0, n0, wid, lane, ex, bias);  // (older than every DMA)
  f8r::StageK ga;
  ga.init(wid, lane, m0, M, lda);
  f8r::StageK gbk;
  f8r::StageN gbn;
  if constexpr (BT) gbn.init(wid, lane, n0, N, ldb);
  else gbk.init(wid, lane, n0, N, ldb);
  auto issue = [&](int j) {
    char* slot = smem + (j % f8r::NS) * f8r::SLOT;
    ga.issue(A, 64 * j, slot, wid);
    if constexpr (BT) gbn.issue(B, ldb, 64 * j, slot + f8r::IMG, wid);
    else gbk.issue(B, 64 * j, slot + f8r::IMG, wid);
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int abase = wm * 64, bbase = wn * 64;

  // prologue: stages 0..3 (ns >= 2); step j waits for stage j with the
  // stages issued after it (up to j + 3) still in flight
  issue(0);
  issue(1);
  if (ns > 2) issue(2);
  if (ns > 3) issue(3);
  // W: stages younger than j in flight at step j's wait; ISS: issue stage j + 4
  auto kstep = [&](int j, auto wc, auto ic) {
    constexpr int W = decltype(wc)::value;
    constexpr bool ISS = decltype(ic)::value != 0;
    f8::wait_vmcnt<W * P>();
    f8::lds_barrier();
    if constexpr (ISS) issue(j + 4);
    const char* st = smem + (j % f8r::NS) * f8r::SLOT;
    i32x8 fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = f8r::frag(st, abase + 32 * i, lane);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      if constexpr (BT) fb[jj] = f8r::frag_t(st + f8r::IMG, bbase + 32 * jj, lane);
      else fb[jj] = f8r::frag(st + f8r::IMG, bbase + 32 * jj, lane);
    }
    tdg::lgkm_wait<0>();
#pragma unroll
    for (int i = 0; i < 2; ++i) tdg::tie(fa[i]);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) tdg::tie(fb[jj]);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        acc[i][jj] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[jj], acc[i][jj], AF, 0,
                                                                     0, 127, 0, 127);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  int j = 0;
  for (; j + 4 < ns; ++j) kstep(j, I3{}, I1{});  // stages j+1..j+3 in flight; issue j + 4
  // tail: no more issues; the stages younger than j in flight: ns - 1 - j
  if (ns - j == 4) kstep(j++, I3{}, I0{});
  if (ns - j == 3) kstep(j++, I2{}, I0{});
  kstep(j++, I1{}, I0{});
  kstep(j, I0{}, I0{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f8::lds_barrier();
  Epi::run32(smem, acc, C, bias, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid,
             ex, pre);
}

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
namespace f8w1 {
constexpr int HB = 128 * BK8;  // bytes of a half-tile image
// image row x (0..127) of half h -> tile row / column
__device__ __forceinline__ int remap(int x, int h) { return (x >> 6) * 128 + h * 64 + (x & 63); }
}  // namespace f8w1

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
  if (tiles_n <= tiles_m) {
    tn = t % tiles_n;
    tm = t / tiles_n;
  } else {
    tm = t % tiles_m;
    tn = t / tiles_m;
  }
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
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  i32x8 fa[TM], fb[TN];
  const int ar = wm * 64, br = wn * 64;  // this wave's rows / columns in a half image

  // prologue: tiles 0 and 1 in flight; A0(0), B0(0) landed and read
#pragma unroll
  for (int q = 0; q < 4; ++q) issue(0, q);
  if (nk > 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) issue(1, q);
    f8::wait_vmcnt<24>();
  } else {
    f8::wait_vmcnt<8>();
  }
  f8::lds_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) fa[i] = f8::frag(smem + 0 * HB, ar + 16 * i, lane);
#pragma unroll
  for (int j = 0; j < 4; ++j) fb[j] = f8::frag(smem + 2 * HB, br + 16 * j, lane);

  auto mfma = [&](int i, int j) {
    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], AF, 0,
                                                                 0, 127, 0, 127);
  };
  // branch-free steady step + tail instantiations (see wgrad_fp8_kernel)
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    constexpr bool more1 = MODE >= 1, more2 = MODE == 2;
    const char* st = smem + (kt & 1) * SB;
    const char* nx = smem + ((kt + 1) & 1) * SB;
    // ---- P0: a0 x b0; read B1(kt); issue A0(kt+2)
    // B1(kt) landed: younger issues A1(kt), A0/B0/B1/A1(kt+1) -- or fewer at the tail
    if constexpr (more1) f8::wait_vmcnt<20>();
    else f8::wait_vmcnt<4>();
    f8::lds_barrier();  // (lgkmcnt(0): last phase's fragment reads)
#pragma unroll
    for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) tdg::tie(fb[j]);
    if constexpr (more2) issue(kt + 2, 0);
#pragma unroll
    for (int j = 4; j < 8; ++j) fb[j] = f8::frag(st + 3 * HB, br + 16 * (j - 4), lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P1: a0 x b1; read A1(kt); issue B0(kt+2)
    // A1(kt) landed: younger A0/B0/B1/A1(kt+1), A0(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<16>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
#pragma unroll
    for (int j = 4; j < 8; ++j) tdg::tie(fb[j]);
    if constexpr (more2) issue(kt + 2, 1);
#pragma unroll
    for (int i = 4; i < 8; ++i) fa[i] = f8::frag(st + 1 * HB, ar + 16 * (i - 4), lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 4; j < 8; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P2: a1 x b1; read A0(kt+1); issue B1(kt+2)
    // A0(kt+1) landed: younger B0/B1/A1(kt+1), A0/B0(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<12>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
#pragma unroll
    for (int i = 4; i < 8; ++i) tdg::tie(fa[i]);
    if constexpr (more2) issue(kt + 2, 2);
    if constexpr (more1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = f8::frag(nx + 0 * HB, ar + 16 * i, lane);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 4; i < 8; ++i)
#pragma unroll
      for (int j = 4; j < 8; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P3: a1 x b0; read B0(kt+1) per column behind its MFMAs; issue A1(kt+2)
    // B0(kt+1) landed: younger B1/A1(kt+1), A0/B0/B1(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<8>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
    if constexpr (more1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);
    }
    if constexpr (more2) issue(kt + 2, 3);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 4; i < 8; ++i) mfma(i, j);
      __builtin_amdgcn_s_setprio(0);
      if constexpr (more1) fb[j] = f8::frag(nx + 2 * HB, br + 16 * j, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  int kt = 0;
  for (; kt + 2 < nk; ++kt) kstep(kt, std::integral_constant<int, 2>{});
  if (kt + 1 < nk) kstep(kt++, std::integral_constant<int, 1>{});
  kstep(kt, std::integral_constant<int, 0>{});

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f8::lds_barrier();
  using Epi = F8Epi<256, 256, 2, 2, EPI, CF, false>;
  typename Epi::Pre none;
  Epi::run(smem, acc, C, bias, sa, sb, C8, sc8, amax_out, M, N, ldc, ldc8, m0, n0, wid, lane, tid, ex,
           none);
}

// ---------------------------------------------------------------------------
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
  if (cl.tiles_n <= cl.tiles_m) {
    tn = tt % cl.tiles_n;
    tm = tt / cl.tiles_n;
  } else {
    tm = tt % cl.tiles_m;
    tn = tt / cl.tiles_m;
  }
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
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  i32x8 fa[TM], fb[TN];
  const int ar = wm * 64, br = wn * 64;

#pragma unroll
  for (int q = 0; q < 4; ++q) issue(0, q);
  if (nk > 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) issue(1, q);
    f8::wait_vmcnt<24>();
  } else {
    f8::wait_vmcnt<8>();
  }
  f8::lds_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) fa[i] = wf8::frag(smem + 0 * HB, ar + 16 * i, lane);
#pragma unroll
  for (int j = 0; j < 4; ++j) fb[j] = wf8::frag(smem + 2 * HB, br + 16 * j, lane);

  // swapped operands: lane holds 4 consecutive n of one m (16-byte stores)
  auto mfma = [&](int i, int j) {
    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[i][j], 0, 1,
                                                                 0, 127, 0, 127);
  };
  // One K-step (128 tokens) in four phases. MODE 2: tiles kt+1 and kt+2
  // exist; 1: only kt+1; 0: the last tile. The steady loop is branch-free
  // (the tail steps are separate instantiations): with `if (more2)` branches
  // inside the body the compiler sank all 64 MFMAs of a step out of their
  // phases into the loop latch, behind every wait and barrier (measured ISA,
  // scripts/isa_loops.py), which serialised the DMA / LDS work and the MFMAs.
  // sched_barrier(0) pins each phase's boundary.
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    constexpr bool more1 = MODE >= 1, more2 = MODE == 2;
    const char* st = smem + (kt & 1) * SB;
    const char* nx = smem + ((kt + 1) & 1) * SB;
    // ---- P0: a0 x b0; read B1(kt); issue A0(kt+2)
    if constexpr (more1) f8::wait_vmcnt<20>();
    else f8::wait_vmcnt<4>();
    f8::lds_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) tdg::tie(fb[j]);
    if constexpr (more2) issue(kt + 2, 0);
#pragma unroll
    for (int j = 4; j < 8; ++j) fb[j] = wf8::frag(st + 3 * HB, br + 16 * (j - 4), lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P1: a0 x b1; read A1(kt); issue B0(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<16>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
#pragma unroll
    for (int j = 4; j < 8; ++j) tdg::tie(fb[j]);
    if constexpr (more2) issue(kt + 2, 1);
#pragma unroll
    for (int i = 4; i < 8; ++i) fa[i] = wf8::frag(st + 1 * HB, ar + 16 * (i - 4), lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 4; j < 8; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P2: a1 x b1; read A0(kt+1); issue B1(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<12>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
#pragma unroll
    for (int i = 4; i < 8; ++i) tdg::tie(fa[i]);
    if constexpr (more2) issue(kt + 2, 2);
    if constexpr (more1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = wf8::frag(nx + 0 * HB, ar + 16 * i, lane);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 4; i < 8; ++i)
#pragma unroll
      for (int j = 4; j < 8; ++j) mfma(i, j);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- P3: a1 x b0; read B0(kt+1) per column behind its MFMAs; issue A1(kt+2)
    if constexpr (more2) f8::wait_vmcnt<20>();
    else if constexpr (more1) f8::wait_vmcnt<8>();
    else f8::wait_vmcnt<0>();
    f8::lds_barrier();
    if constexpr (more1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);
    }
    if constexpr (more2) issue(kt + 2, 3);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 4; i < 8; ++i) mfma(i, j);
      __builtin_amdgcn_s_setprio(0);
      if constexpr (more1) fb[j] = wf8::frag(nx + 2 * HB, br + 16 * j, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  int kt = 0;
  for (; kt + 2 < nk; ++kt) kstep(kt, std::integral_constant<int, 2>{});
  if (kt + 1 < nk) kstep(kt++, std::integral_constant<int, 1>{});
  kstep(kt, std::integral_constant<int, 0>{});
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

// Quantise a [M, N] bf16 gradient (row stride ld) to fp8 (FMT) AND write the
// per-row-block column sums of the bf16 values (part[blockIdx.y][N], folded
// later: the bias gradient of the layer whose output gradient this is) in
// one pass. Block: 256 columns (32 lanes x 8) x 8 row lanes, QC_ROWS rows.
constexpr int QC_ROWS = 256;
template <int FMT>
__global__ __launch_bounds__(256) void fp8_quant_colsum_kernel(const bf16_t* __restrict__ x, int ld,
                                                               uint8_t* __restrict__ y8, int M,
                                                               int N, const float* __restrict__ scale,
                                                               unsigned* __restrict__ amax_out,
                                                               float* __restrict__ part) {
  __shared__ float red[8][256 + 4];
  __shared__ float redm[4];
  const float s = scale[0];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int n = blockIdx.x * 256 + cl * 8;
  const int r0 = blockIdx.y * QC_ROWS;
  const int r1 = min(M, r0 + QC_ROWS);
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float amax = 0.f;
  if (n < N) {  // (host: N % 8 == 0, ld % 8 == 0)
    for (int r = r0 + rl; r < r1; r += 8) {
      const short8_t v = *reinterpret_cast<const short8_t*>(x + (size_t)r * ld + n);
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = bf2f((bf16_t)v[e]);
        cs[e] += f[e];
        amax = fmaxf(amax, fabsf(f[e]));
      }
      int lo = f8::pack2_f8<FMT, false>(f[0] * s, f[1] * s, 0);
      lo = f8::pack2_f8<FMT, true>(f[2] * s, f[3] * s, lo);
      int hi = f8::pack2_f8<FMT, false>(f[4] * s, f[5] * s, 0);
      hi = f8::pack2_f8<FMT, true>(f[6] * s, f[7] * s, hi);
      *reinterpret_cast<int2*>(y8 + (size_t)r * N + n) = make_int2(lo, hi);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cl * 8 + e] = cs[e];
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = amax;
  __syncthreads();
  const int c = threadIdx.x;  // one column per thread
  if (blockIdx.x * 256 + c < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][c];
    part[(size_t)blockIdx.y * N + blockIdx.x * 256 + c] = t;
  }
  if (threadIdx.x == 0 && amax_out)
    f8::atomic_amax(amax_word(amax_out, blockIdx.y * gridDim.x + blockIdx.x),
                    fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3])));
}

// Transposing e4m3 quantisation of same-shape weights: dst[g] [C][R] =
// e4m3(src[g] [R][C]^T * scale[slot[g]]), amax into amax[slot[g]] -- the
// transposed weight copies of the fp8 dgrads straight from the bf16 compute
// copy (no bf16 transposed copy). 64 x 64 tiles through LDS.
constexpr int QT_MAXG = 64;
struct QuantTGroup {
  const bf16_t* src[QT_MAXG];
  uint8_t* dst[QT_MAXG];
  int slot[QT_MAXG];
};
__global__ __launch_bounds__(256) void fp8_quant_t_kernel(QuantTGroup grp, int R, int C,
                                                          const float* __restrict__ scale,
                                                          unsigned* __restrict__ amax) {
  __shared__ float tile[64][65];
  __shared__ float redm[4];
  const bf16_t* __restrict__ src = grp.src[blockIdx.y];
  uint8_t* __restrict__ dst = grp.dst[blockIdx.y];
  const int slot = grp.slot[blockIdx.y];
  const float s = scale[slot];
  const int tiles_c = (C + 63) / 64;
  const int r0 = (blockIdx.x / tiles_c) * 64, c0 = (blockIdx.x % tiles_c) * 64;
  const int tid = threadIdx.x;
  float am = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = tid + 256 * k;
    const int r = id >> 3, c = (id & 7) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = r0 + r < R && c0 + c + e < C;
      const float f = in ? bf2f(src[(size_t)(r0 + r) * C + c0 + c + e]) : 0.f;
      tile[r][c + e] = f;
      am = fmaxf(am, fabsf(f));
    }
  }
  __syncthreads();
  // dst row = source column (c0 + c), 8 consecutive source rows per thread
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = tid + 256 * k;
    const int c = id >> 3, r = (id & 7) * 8;
    if (c0 + c >= C) continue;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = tile[r + e][c] * s;
    int lo = f8::pack2_f8<0, false>(f[0], f[1], 0);
    lo = f8::pack2_f8<0, true>(f[2], f[3], lo);
    int hi = f8::pack2_f8<0, false>(f[4], f[5], 0);
    hi = f8::pack2_f8<0, true>(f[6], f[7], hi);
    uint8_t* d = dst + (size_t)(c0 + c) * R + r0 + r;
    if (r0 + r + 8 <= R && (R % 8) == 0) {
      *reinterpret_cast<int2*>(d) = make_int2(lo, hi);
    } else {
      for (int e = 0; e < 8 && r0 + r + e < R; ++e)
        d[e] = (uint8_t)(((e < 4 ? lo : hi) >> (8 * (e & 3))) & 0xff);
    }
  }
  am = wave_max(am);
  if ((tid & 63) == 0) redm[tid >> 6] = am;
  __syncthreads();
  if (tid == 0)
    f8::atomic_amax(amax_word(amax + (size_t)slot * AMAX_WORDS, blockIdx.x),
                    fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3])));
}

// y8 = e4m3(x * scale[0]); amax_out = max|x| (both optional sides)
template <int FMT>
__global__ __launch_bounds__(256) void fp8_quant_kernel(const bf16_t* __restrict__ x,
                                                        uint8_t* __restrict__ y8, long long n,
                                                        const float* __restrict__ scale,
                                                        unsigned* __restrict__ amax_out) {
  const float s = scale[0];
  float amax = 0.f;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n;
       i += (long long)gridDim.x * blockDim.x * 8) {
    if (i + 8 <= n) {
      const short8_t v = *reinterpret_cast<const short8_t*>(x + i);
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = bf2f((bf16_t)v[e]);
        amax = fmaxf(amax, fabsf(f[e]));
      }
      int lo = f8::pack2_f8<FMT, false>(f[0] * s, f[1] * s, 0);
      lo = f8::pack2_f8<FMT, true>(f[2] * s, f[3] * s, lo);
      int hi = f8::pack2_f8<FMT, false>(f[4] * s, f[5] * s, 0);
      hi = f8::pack2_f8<FMT, true>(f[6] * s, f[7] * s, hi);
      *reinterpret_cast<int2*>(y8 + i) = make_int2(lo, hi);
    } else {
      for (long long e = i; e < n; ++e) {
        const float f = bf2f(x[e]);
        amax = fmaxf(amax, fabsf(f));
        const int w = f8::pack2_f8<FMT, false>(f * s, 0.f, 0);
        y8[e] = (uint8_t)(w & 0xff);
      }
    }
  }
  // one atomic per block: thousands of same-address atomics serialise in L2
  __shared__ float red[4];
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0 && amax_out)
    f8::atomic_amax(amax_word(amax_out, blockIdx.x),
                    fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// Many tensors in one launch (the weight refresh after every optimizer step:
// 43 weight matrices of Transformer-big, 43 launches of ~8 us before): block
// ranges per segment from a host prefix sum, each segment its own scale and
// amax slot.
constexpr int QMAX = 64;
struct QuantSegs {
  const bf16_t* x[QMAX];
  uint8_t* y[QMAX];
  long long n[QMAX];
  int slot[QMAX];
  int blk0[QMAX + 1];
};

__global__ __launch_bounds__(256) void fp8_quant_multi_kernel(const QuantSegs segs, int nseg,
                                                              const float* __restrict__ scale,
                                                              unsigned* __restrict__ amax_out) {
  int sg = 0;
  for (int i = 1; i < nseg; ++i)
    if ((int)blockIdx.x >= segs.blk0[i]) sg = i;
  const bf16_t* __restrict__ x = segs.x[sg];
  uint8_t* __restrict__ y8 = segs.y[sg];
  const long long n = segs.n[sg];
  const int b = blockIdx.x - segs.blk0[sg], nb = segs.blk0[sg + 1] - segs.blk0[sg];
  const float s = scale[segs.slot[sg]];
  float amax = 0.f;
  for (long long i = ((long long)b * blockDim.x + threadIdx.x) * 8; i < n;
       i += (long long)nb * blockDim.x * 8) {
    if (i + 8 <= n) {
      const short8_t v = *reinterpret_cast<const short8_t*>(x + i);
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = bf2f((bf16_t)v[e]);
        amax = fmaxf(amax, fabsf(f[e]));
      }
      int lo = f8::pack2_e4m3<false>(f[0] * s, f[1] * s, 0);
      lo = f8::pack2_e4m3<true>(f[2] * s, f[3] * s, lo);
      int hi = f8::pack2_e4m3<false>(f[4] * s, f[5] * s, 0);
      hi = f8::pack2_e4m3<true>(f[6] * s, f[7] * s, hi);
      *reinterpret_cast<int2*>(y8 + i) = make_int2(lo, hi);
    } else {
      for (long long e = i; e < n; ++e) {
        const float f = bf2f(x[e]);
        amax = fmaxf(amax, fabsf(f));
        y8[e] = (uint8_t)(f8::pack2_e4m3<false>(f * s, 0.f, 0) & 0xff);
      }
    }
  }
  __shared__ float red[4];
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0 && amax_out)
    f8::atomic_amax(amax_word(amax_out + (long long)segs.slot[sg] * AMAX_WORDS, b),
                    fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// Delayed scaling: scale[i] = 448 / (amax[i] * 2^margin) from last step's
// amax (kept when nothing was recorded), then amax[i] = 0.
// One wave per slot, lane j reads (and clears) word j of the slot's spread.
__global__ __launch_bounds__(256) void fp8_scale_update_kernel(float* __restrict__ scale,
                                                               unsigned* __restrict__ amax, int n,
                                                               float margin_pow2, float fmax) {
  static_assert(AMAX_SPREAD == 64, "one lane per spread word");
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  unsigned* w = amax + (long long)i * AMAX_WORDS + lane * AMAX_STRIDE;
  unsigned m = *w;
  *w = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  const float a = __uint_as_float(m);
  // power-of-two scales: dequantisation (x8 / scale) is exact in bf16 / f32,
  // so an fp8 operand and its bf16 dequantised copy carry the same values
  if (lane == 0 && a > 0.f && isfinite(a)) {
    int e;
    frexpf(fmax / (a * margin_pow2), &e);  // ratio = f * 2^e, f in [0.5, 1)
    scale[i] = ldexpf(1.f, e - 1);         // largest 2^k <= ratio
  }
}

// e4m3 -> f32 (tests / debugging)
__global__ void fp8_dequant_kernel(const uint8_t* __restrict__ x8, float* __restrict__ y,
                                   long long n, float inv_scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = __builtin_amdgcn_cvt_f32_fp8((int)x8[i], 0) * inv_scale;
}

}  // namespace tdg

using namespace tdg;

namespace {
// compute units of the current device (cached per process)
int cu_count() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}
// persistent 128x128 fp8 GEMM (gemm_fp8_pk_kernel) per epilogue id: a bit
// mask over F8_EPI_* (TDG_FP8_PERSIST: 0 = off, "all", or a comma list of
// epilogue ids; default: the ReLU forward and the 8-bit-mask ReLU backward,
// the two measured faster in the step); tdg_fp8_set_persist overrides (tests
// compare both forms in one process)
int g_fp8_persist = -1;
int fp8_persist_mask() {
  if (g_fp8_persist < 0) {
    const char* e = getenv("TDG_FP8_PERSIST");
    int m = (1 << F8_EPI_BIAS_RELU) | (1 << F8_EPI_DRELU8);
    if (e && *e) {
      if (e[0] == 'a') {
        m = 0xff;
      } else {  // "0": off; "2,4": those epilogue ids
        m = 0;
        for (const char* c = e; *c; ++c)
          if (*c >= '1' && *c <= '7' && (c == e || c[-1] == ',')) m |= 1 << (*c - '0');
      }
    }
    g_fp8_persist = m;
  }
  return g_fp8_persist;
}
bool fp8_persist(int epi) { return (fp8_persist_mask() >> epi) & 1; }
template <int BM, int BN, int WM, int WN, int ST, int EPI, int AF = 0, int CF = 0, bool BT = false>
int launch_f8(const void* A, const void* B, void* C, const float* bias, const float* sa,
              const float* sb, void* C8, const float* sc8, unsigned* amax, int M, int N, int K,
              int lda, int ldb, int ldc, int ldc8, const F8Extra& ex, hipStream_t st) {
  constexpr int img = WM * WN * (BM / WM) * ((BN / WN) * 2 + 16) + 64;  // + amax scratch
  constexpr int lds = std::max(ST * (BM + BN) * BK8, img);
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)gemm_fp8_kernel<BM, BN, WM, WN, ST, EPI, AF, CF, BT>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const int tiles = cdiv(M, BM) * cdiv(N, BN);
  // persistent walk when there is more than one round of tiles (K >= 256;
  // not the bf16-mask ReLU backward, whose epilogue would spill in the loop)
  if constexpr (BM == 128 && BN == 128 && WM == 2 && WN == 2 && ST == 2 && EPI != F8_EPI_DRELU) {
    const int grid = 2 * cu_count();
    if (fp8_persist(EPI) && K >= 2 * BK8 && tiles > grid) {
      constexpr int plds = 2 * (BM + BN) * BK8 + (BM / 2) * (BN + 16) + 64;  // stages, wave-3 image, scratch
      static bool pattr = false;
      if (!pattr) {
        hipFuncSetAttribute((const void*)gemm_fp8_pk_kernel<EPI, AF, CF, BT>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        pattr = true;
      }
      hipLaunchKernelGGL((gemm_fp8_pk_kernel<EPI, AF, CF, BT>), dim3(grid), dim3(256), plds, st,
                         (const uint8_t*)A, (const uint8_t*)B, (bf16_t*)C, bias, sa, sb,
                         (uint8_t*)C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex);
      return 0;
    }
  }
  hipLaunchKernelGGL((gemm_fp8_kernel<BM, BN, WM, WN, ST, EPI, AF, CF, BT>), dim3(tiles),
                     dim3(WM * WN * 64), lds, st, (const uint8_t*)A, (const uint8_t*)B, (bf16_t*)C,
                     bias, sa, sb, (uint8_t*)C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex);
  return 0;
}

template <int EPI, int AF = 0, int CF = 0>
int launch_f8_w1(const void* A, const void* B, void* C, const float* bias, const float* sa,
                 const float* sb, void* C8, const float* sc8, unsigned* amax, int M, int N, int K,
                 int lda, int ldb, int ldc, int ldc8, const F8Extra& ex, hipStream_t st) {
  constexpr int img = 4 * 128 * (128 * 2 + 16) + 64;  // epilogue images + amax scratch
  constexpr int lds = std::max(2 * 4 * f8w1::HB, img);
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)gemm_fp8_w1_kernel<EPI, AF, CF>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const int tiles = cdiv(M, 256) * cdiv(N, 256);
  hipLaunchKernelGGL((gemm_fp8_w1_kernel<EPI, AF, CF>), dim3(tiles), dim3(256), lds, st,
                     (const uint8_t*)A, (const uint8_t*)B, (bf16_t*)C, bias, sa, sb, (uint8_t*)C8,
                     sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex);
  return 0;
}

template <int EPI, int AF = 0, int CF = 0, bool BT = false>
int launch_f8r(const void* A, const void* B, void* C, const float* bias, const float* sa,
               const float* sb, void* C8, const float* sc8, unsigned* amax, int M, int N, int K,
               int lda, int ldb, int ldc, int ldc8, const F8Extra& ex, hipStream_t st) {
  if ((long long)M * lda >= (1LL << 32) || (!BT && (long long)N * ldb >= (1LL << 32))) return -3;
  constexpr int img = 4 * 64 * (64 * 2 + 16) + 64;
  constexpr int lds = std::max(f8r::NS * f8r::SLOT, img);
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)gemm_fp8_ring_kernel<EPI, AF, CF, BT>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const int tiles = cdiv(M, 128) * cdiv(N, 128);
  hipLaunchKernelGGL((gemm_fp8_ring_kernel<EPI, AF, CF, BT>), dim3(tiles), dim3(256), lds, st,
                     (const uint8_t*)A, (const uint8_t*)B, (bf16_t*)C, bias, sa, sb, (uint8_t*)C8,
                     sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex);
  return 0;
}

template <int EPI>
int tiles_f8(int cfg, const void* A, const void* B, void* C, const float* bias, const float* sa,
             const float* sb, void* C8, const float* sc8, unsigned* amax, int M, int N, int K,
             int lda, int ldb, int ldc, int ldc8, const F8Extra& ex, hipStream_t st) {
#define TDG_F8(ID, BM_, BN_, WM_, WN_, ST_) \
  case ID:                                 \
    return launch_f8<BM_, BN_, WM_, WN_, ST_, EPI>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
  switch (cfg) {
    TDG_F8(0, 128, 128, 2, 2, 2)
    TDG_F8(1, 128, 64, 2, 2, 3)
    TDG_F8(2, 64, 128, 2, 2, 3)
    TDG_F8(3, 256, 128, 4, 2, 2)
    TDG_F8(4, 128, 128, 2, 4, 3)
    TDG_F8(8, 256, 128, 4, 2, 3)
    case 9:  // 256x256, one wave per SIMD (gemm_fp8_w1_kernel)
      if ((long long)M * lda >= (1LL << 32) || (long long)N * ldb >= (1LL << 32)) return -3;
      return launch_f8_w1<EPI>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    case 10:  // 128x128, ring of 64-byte K half-stages (gemm_fp8_ring_kernel)
      return launch_f8r<EPI>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    default:
      TDG_F8(5, 64, 128, 2, 2, 2)
  }
#undef TDG_F8
}
}  // namespace

// afmt / cfmt: formats of A and of the C8 copy (0 e4m3, 1 e5m2). The e5m2-A
// backward GEMMs (ReLU-backward dgrad with an e5m2 copy of its output; the
// plain dgrad accumulating into C) run on the 128x128 tile only.
static int tdg_gemm_fp8_body(const void* A, const void* B, void* C, const float* bias,
                             const float* sa, const float* sb, void* C8, const float* sc8,
                             unsigned* amax, int M, int N, int K, int lda, int ldb, int ldc,
                             int ldc8, int epi, int cfg, int afmt, int cfmt, const F8Extra& ex,
                             hipStream_t st, bool bt);

// aux8: the ReLU-backward mask as 8-bit activations (instead of bf16 aux);
// colsum_out: also colsum_out[N] (=|+= colsum_beta) the column sums of the
// stored output (bias gradient), via partials in ws (>= rows * N floats,
// rows = ceil(M / BM) * WM of the tile config; the 128x128 tile: M / 64).
// C may be null (then only C8 and / or the column sums are produced).
extern "C" int tdg_gemm_fp8(const void* A, const void* B, void* C, const float* bias,
                            const float* sa, const float* sb, void* C8, const float* sc8,
                            unsigned* amax, int M, int N, int K, int lda, int ldb, int ldc,
                            int ldc8, int epi, int cfg, int afmt, int cfmt, const void* aux,
                            int ldaux, float beta, const void* aux8, float* colsum_out,
                            float colsum_beta, float* ws, hipStream_t st) {
  if (K % BK8 != 0 || lda % 16 != 0 || ldb % 16 != 0) return -2;
  const int cdeq = (epi & F8_EPI_CDEQ) != 0;
  const bool bt = (epi & F8_B_NCONTIG) != 0;
  const bool csdefer = (epi & F8_CS_DEFER) != 0;
  epi &= ~(F8_EPI_CDEQ | F8_B_NCONTIG | F8_CS_DEFER);
  if (bt && ((cfg != 0 && cfg != 10) || N % 16 != 0 || ldb < N || afmt != 1 || cfmt != 1)) return -6;
  if (cdeq && !C8) return -2;
  if (!C && (beta != 0.f || cdeq)) return -2;
  if (colsum_out && (!ws || (cfg != 0 && cfg != 10))) return -2;  // (partials: 128x128 / 2x2 tiles)
  const F8Extra ex{(const bf16_t*)aux, ldaux, beta, cdeq, (const uint8_t*)aux8,
                   colsum_out ? ws : nullptr};
  if (colsum_out) {
    const int rc = tdg_gemm_fp8_body(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc,
                                     ldc8, epi, cfg, afmt, cfmt, ex, st, bt);
    if (rc) return rc;
    if (!csdefer) launch_reduce_partials(ws, colsum_out, N, cdiv(M, 128) * 2, colsum_beta, st);
    return 0;
  }
  return tdg_gemm_fp8_body(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, epi,
                           cfg, afmt, cfmt, ex, st, bt);
}

static int tdg_gemm_fp8_body(const void* A, const void* B, void* C, const float* bias,
                             const float* sa, const float* sb, void* C8, const float* sc8,
                             unsigned* amax, int M, int N, int K, int lda, int ldb, int ldc,
                             int ldc8, int epi, int cfg, int afmt, int cfmt, const F8Extra& ex,
                             hipStream_t st, bool bt) {
  if (bt && cfg == 10) {
    if (epi == F8_EPI_DRELU && ex.aux8)
      return launch_f8r<F8_EPI_DRELU8, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    if (epi == F8_EPI_DRELU)
      return launch_f8r<F8_EPI_DRELU, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    if (epi == F8_EPI_NONE)
      return launch_f8r<F8_EPI_NONE, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    return -1;
  }
  if (bt) {  // e5m2 x N-contiguous e4m3 (validated by the caller: cfg 0 or 10)
    if (epi == F8_EPI_DRELU && ex.aux8)
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_DRELU8, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    if (epi == F8_EPI_DRELU)
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_DRELU, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    if (epi == F8_EPI_NONE)
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_NONE, 1, 1, true>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    return -1;
  }
  if (afmt == 0 && cfmt == 0) {
    switch (epi) {
      case F8_EPI_NONE: return tiles_f8<F8_EPI_NONE>(cfg, A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      case F8_EPI_BIAS: return tiles_f8<F8_EPI_BIAS>(cfg, A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      case F8_EPI_BIAS_RELU: return tiles_f8<F8_EPI_BIAS_RELU>(cfg, A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      default: return -1;
    }
  }
  if (afmt == 1 && cfmt == 1) {
    if (cfg == 10) {
      if (epi == F8_EPI_DRELU && ex.aux8)
        return launch_f8r<F8_EPI_DRELU8, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      if (epi == F8_EPI_DRELU)
        return launch_f8r<F8_EPI_DRELU, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      if (epi == F8_EPI_NONE)
        return launch_f8r<F8_EPI_NONE, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      return -1;
    }
    if (epi == F8_EPI_DRELU && ex.aux8) {
      if (cfg == 9 && (long long)M * lda < (1LL << 32) && (long long)N * ldb < (1LL << 32))
        return launch_f8_w1<F8_EPI_DRELU8, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_DRELU8, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    }
    if (cfg == 9 && (long long)M * lda < (1LL << 32) && (long long)N * ldb < (1LL << 32)) {
      if (epi == F8_EPI_DRELU)
        return launch_f8_w1<F8_EPI_DRELU, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
      if (epi == F8_EPI_NONE)
        return launch_f8_w1<F8_EPI_NONE, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    }
    if (epi == F8_EPI_DRELU)
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_DRELU, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
    if (epi == F8_EPI_NONE)
      return launch_f8<128, 128, 2, 2, 2, F8_EPI_NONE, 1, 1>(A, B, C, bias, sa, sb, C8, sc8, amax, M, N, K, lda, ldb, ldc, ldc8, ex, st);
  }
  return -1;
}

// on: an F8_EPI_* bit mask (0 off, 0xff all); < 0 queries. Returns the old mask.
extern "C" int tdg_fp8_set_persist(int on) {
  const int old = fp8_persist_mask();
  if (on >= 0) g_fp8_persist = on;
  return old;
}

extern "C" int tdg_fp8_quant(const void* x, void* y8, long long n, const float* scale,
                             unsigned* amax, int fmt, hipStream_t st) {
  const int blocks = (int)std::min<long long>(1024, (n / 8 + 255) / 256 + 1);
  if (fmt == 1)
    hipLaunchKernelGGL(fp8_quant_kernel<1>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x,
                       (uint8_t*)y8, n, scale, amax);
  else
    hipLaunchKernelGGL(fp8_quant_kernel<0>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x,
                       (uint8_t*)y8, n, scale, amax);
  return 0;
}

// segments: x[i] (bf16, n[i] elements) -> y[i] with scale[slot[i]], amax into
// amax[slot[i]] (AMAX_SPREAD words each); blocks split by size
extern "C" int tdg_fp8_quant_multi(const void* const* x, void* const* y, const long long* n,
                                   const int* slot, int nseg, const float* scale, unsigned* amax,
                                   hipStream_t st) {
  if (nseg <= 0 || nseg > QMAX) return -2;
  QuantSegs q{};
  long long total = 0;
  for (int i = 0; i < nseg; ++i) total += n[i];
  int blk = 0;
  for (int i = 0; i < nseg; ++i) {
    q.x[i] = (const bf16_t*)x[i];
    q.y[i] = (uint8_t*)y[i];
    q.n[i] = n[i];
    q.slot[i] = slot[i];
    q.blk0[i] = blk;
    // ~4096 blocks over all segments, at least one each
    blk += (int)std::max<long long>(1, (n[i] * 4096 + total - 1) / std::max<long long>(total, 1));
  }
  q.blk0[nseg] = blk;
  hipLaunchKernelGGL(fp8_quant_multi_kernel, dim3(blk), dim3(256), 0, st, q, nseg, scale, amax);
  return 0;
}

extern "C" int tdg_fp8_scale_update(float* scale, unsigned* amax, int n, float margin_pow2,
                                    float fmax, hipStream_t st) {
  hipLaunchKernelGGL(fp8_scale_update_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, scale, amax, n,
                     margin_pow2, fmax);
  return 0;
}

extern "C" int tdg_fp8_dequant(const void* x8, float* y, long long n, float inv_scale,
                               hipStream_t st) {
  hipLaunchKernelGGL(fp8_dequant_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (const uint8_t*)x8, y, n, inv_scale);
  return 0;
}

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
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)wgrad_fp8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                        160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(wgrad_fp8_kernel, dim3(tiles), dim3(256), lds, st, args, T, beta);
  return 0;
}

// y8 [M, N] (contiguous) = fp8(x * scale) of x [M, N] (row stride ld), amax
// recorded, and part[ceil(M / 256)][N] = per-row-block column sums of x.
extern "C" int tdg_fp8_quant_colsum(const void* x, int ld, void* y8, int M, int N,
                                    const float* scale, unsigned* amax, float* part, int fmt,
                                    hipStream_t st) {
  if (N % 8 || ld % 8 || M <= 0) return -2;
  const dim3 grid(cdiv(N, 256), cdiv(M, QC_ROWS));
  if (fmt == 1)
    hipLaunchKernelGGL(fp8_quant_colsum_kernel<1>, grid, dim3(256), 0, st, (const bf16_t*)x, ld,
                       (uint8_t*)y8, M, N, scale, amax, part);
  else
    hipLaunchKernelGGL(fp8_quant_colsum_kernel<0>, grid, dim3(256), 0, st, (const bf16_t*)x, ld,
                       (uint8_t*)y8, M, N, scale, amax, part);
  return 0;
}

extern "C" int tdg_fp8_quant_t(const void* const* src, void* const* dst, const int* slot, int G,
                               int R, int C, const float* scale, unsigned* amax, hipStream_t st) {
  if (G < 1 || G > QT_MAXG || R < 1 || C < 1) return -2;
  QuantTGroup g{};
  for (int i = 0; i < G; ++i) {
    g.src[i] = (const bf16_t*)src[i];
    g.dst[i] = (uint8_t*)dst[i];
    g.slot[i] = slot[i];
  }
  const int tiles = cdiv(R, 64) * cdiv(C, 64);
  hipLaunchKernelGGL(fp8_quant_t_kernel, dim3(tiles, G), dim3(256), 0, st, g, R, C, scale, amax);
  return 0;
}
