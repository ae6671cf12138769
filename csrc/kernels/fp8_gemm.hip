// FP8 (OCP e4m3) forward GEMM, and the e5m2-gradient backward GEMMs, for gfx950.
//
//   C[m,n] = act( (sum_k A8[m,k] * B8[n,k]) / (sa * sb) + bias[n] )      (bf16 out)
//   optional C8 = e4m3(C * sc8), amax(C) -> amax_out   (fp8 copy for the next GEMM)
//
// A8 = e4m3(A * sa) and B8 = e4m3(B * sb) are per-tensor scaled copies of the
// bf16 activations / weights; the scales live in device memory (delayed
// scaling, fp8_quant.hip), so a captured HIP graph stays valid across steps.
//
// MFMA: v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 block scales -- the
// per-tensor scales are applied in the epilogue. Lane l holds
// A[row l&15][k 32(l>>4) .. +31] and B[k 32(l>>4) .. +31][col l&15] (verified
// with exact integer data: scripts/probes/fp8_mfma_layout.hip); C/D layout as
// every 16x16 MFMA on gfx950 (col l&15, row 4(l>>4)+r). One instruction per
// 128-deep K tile = twice the bf16 16x16x32 rate per clock, and half the bytes
// staged through LDS.
//
// Staging is the bf16 kernels' (tdg_gemm.h Glds, gemm_pipe.h): LDS-DMA
// (global_load_lds_dwordx4) into 128-byte-row images with the same 32-byte
// XOR swizzle, STAGES tiles in flight, counted vmcnt + raw s_barrier.
//
// Replaces (in the fp8 configuration, BASELINE config 5) the forward Dense
// MatMuls of the reference (distributed_training_transformer/
// transformer_model.py:119-122, 165, 172-174); backward stays bf16.
//
// One unit: fp8_impl.h (shared device pieces), fp8_epi.h (epilogue), and one
// header per kernel.
#include "tdg_api.h"
#include "tdg_reduce.h"
#include "fp8_gemm_tile.h"
#include "fp8_gemm_ring.h"
#include "fp8_gemm_w1.h"

#include <algorithm>
#include <cstdlib>

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

// The operands of one GEMM, as every kernel takes them (tdg_gemm_fp8's
// arguments after validation)
struct F8Args {
  const uint8_t *A, *B;
  bf16_t* C;
  const float *bias, *sa, *sb;
  uint8_t* C8;
  const float* sc8;
  unsigned* amax;
  int M, N, K, lda, ldb, ldc, ldc8;
  F8Extra ex;
  hipStream_t st;
  // A (and a K-contiguous B) addressed with 32-bit offsets
  bool fits32(bool b_too) const {
    return (long long)M * lda < (1LL << 32) && (!b_too || (long long)N * ldb < (1LL << 32));
  }
};
// Kernel over `grid` workgroups of `block` threads with `lds` bytes
template <auto Kernel>
int launch(const F8Args& a, int grid, int block, int lds) {
  big_lds<Kernel>();
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, a.st, a.A, a.B, a.C, a.bias, a.sa, a.sb,
                     a.C8, a.sc8, a.amax, a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.ldc8, a.ex);
  return 0;
}

template <int BM, int BN, int WM, int WN, int ST, int EPI, int AF = 0, int CF = 0, bool BT = false>
int launch_f8(const F8Args& a) {
  constexpr int img = WM * WN * (BM / WM) * ((BN / WN) * 2 + 16) + 64;  // + amax scratch
  constexpr int lds = std::max(ST * (BM + BN) * BK8, img);
  const int tiles = cdiv(a.M, BM) * cdiv(a.N, BN);
  // persistent walk when there is more than one round of tiles (K >= 256;
  // not the bf16-mask ReLU backward, whose epilogue would spill in the loop)
  if constexpr (BM == 128 && BN == 128 && WM == 2 && WN == 2 && ST == 2 && EPI != F8_EPI_DRELU) {
    const int grid = 2 * cu_count();
    if (fp8_persist(EPI) && a.K >= 2 * BK8 && tiles > grid) {
      constexpr int plds = 2 * (BM + BN) * BK8 + (BM / 2) * (BN + 16) + 64;  // stages, wave-3 image, scratch
      return launch<gemm_fp8_pk_kernel<EPI, AF, CF, BT>>(a, grid, 256, plds);
    }
  }
  return launch<gemm_fp8_kernel<BM, BN, WM, WN, ST, EPI, AF, CF, BT>>(a, tiles, WM * WN * 64, lds);
}

template <int EPI, int AF = 0, int CF = 0>
int launch_f8_w1(const F8Args& a) {
  constexpr int img = 4 * 128 * (128 * 2 + 16) + 64;  // epilogue images + amax scratch
  constexpr int lds = std::max(2 * 4 * f8w1::HB, img);
  return launch<gemm_fp8_w1_kernel<EPI, AF, CF>>(a, cdiv(a.M, 256) * cdiv(a.N, 256), 256, lds);
}

template <int EPI, int AF = 0, int CF = 0, bool BT = false>
int launch_f8r(const F8Args& a) {
  if (!a.fits32(!BT)) return -3;
  constexpr int img = 4 * 64 * (64 * 2 + 16) + 64;
  constexpr int lds = std::max(f8r::NS * f8r::SLOT, img);
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  return launch<gemm_fp8_ring_kernel<EPI, AF, CF, BT>>(a, cdiv(a.M, 128) * cdiv(a.N, 128), 256, lds);
}

// the forward tile table (e4m3 A, e4m3 C8)
template <int EPI>
int tiles_f8(int cfg, const F8Args& a) {
#define TDG_F8(ID, BM_, BN_, WM_, WN_, ST_) \
  case ID:                                 \
    return launch_f8<BM_, BN_, WM_, WN_, ST_, EPI>(a);
  switch (cfg) {
    TDG_F8(0, 128, 128, 2, 2, 2)
    TDG_F8(1, 128, 64, 2, 2, 3)
    TDG_F8(2, 64, 128, 2, 2, 3)
    TDG_F8(3, 256, 128, 4, 2, 2)
    TDG_F8(4, 128, 128, 2, 4, 3)
    TDG_F8(8, 256, 128, 4, 2, 3)
    case 9:  // 256x256, one wave per SIMD (gemm_fp8_w1_kernel)
      if (!a.fits32(true)) return -3;
      return launch_f8_w1<EPI>(a);
    case 10:  // 128x128, ring of 64-byte K half-stages (gemm_fp8_ring_kernel)
      return launch_f8r<EPI>(a);
    default:
      TDG_F8(5, 64, 128, 2, 2, 2)
  }
#undef TDG_F8
}

template <int E>
using EpiC = std::integral_constant<int, E>;

// afmt / cfmt: formats of A and of the C8 copy (0 e4m3, 1 e5m2). The e5m2-A
// backward GEMMs (ReLU-backward dgrad with an e5m2 copy of its output; the
// plain dgrad accumulating into C) run on the 128x128 tile, the ring (cfg 10)
// or, with a K-contiguous B of 32-bit extent, the 256x256 tile (cfg 9; larger
// operands fall back to 128x128).
int gemm_fp8_dispatch(const F8Args& a, int epi, int cfg, int afmt, int cfmt, bool bt) {
  if (afmt == 0 && cfmt == 0) {  // (bt: validated by the caller -- both e5m2, cfg 0 or 10)
    switch (epi) {
      case F8_EPI_NONE: return tiles_f8<F8_EPI_NONE>(cfg, a);
      case F8_EPI_BIAS: return tiles_f8<F8_EPI_BIAS>(cfg, a);
      case F8_EPI_BIAS_RELU: return tiles_f8<F8_EPI_BIAS_RELU>(cfg, a);
      default: return -1;
    }
  }
  if (afmt != 1 || cfmt != 1) return -1;
  // the epilogue of a backward GEMM, applied to a launcher: ReLU backward with
  // the 8-bit or the bf16 mask, or none
  auto with_epi = [&](auto launcher) {
    if (epi == F8_EPI_DRELU && a.ex.aux8) return launcher(EpiC<F8_EPI_DRELU8>{});
    if (epi == F8_EPI_DRELU) return launcher(EpiC<F8_EPI_DRELU>{});
    if (epi == F8_EPI_NONE) return launcher(EpiC<F8_EPI_NONE>{});
    return -1;
  };
  if (bt && cfg == 10)
    return with_epi([&](auto e) { return launch_f8r<decltype(e)::value, 1, 1, true>(a); });
  if (bt)  // e5m2 x N-contiguous e4m3
    return with_epi([&](auto e) { return launch_f8<128, 128, 2, 2, 2, decltype(e)::value, 1, 1, true>(a); });
  if (cfg == 10) return with_epi([&](auto e) { return launch_f8r<decltype(e)::value, 1, 1>(a); });
  if (cfg == 9 && a.fits32(true))
    return with_epi([&](auto e) { return launch_f8_w1<decltype(e)::value, 1, 1>(a); });
  return with_epi([&](auto e) { return launch_f8<128, 128, 2, 2, 2, decltype(e)::value, 1, 1>(a); });
}
}  // namespace

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
  const F8Args a{(const uint8_t*)A, (const uint8_t*)B, (bf16_t*)C, bias, sa, sb, (uint8_t*)C8, sc8,
                 amax, M, N, K, lda, ldb, ldc, ldc8,
                 F8Extra{(const bf16_t*)aux, ldaux, beta, cdeq, (const uint8_t*)aux8,
                         colsum_out ? ws : nullptr},
                 st};
  const int rc = gemm_fp8_dispatch(a, epi, cfg, afmt, cfmt, bt);
  if (rc == 0 && colsum_out && !csdefer)
    launch_reduce_partials(ws, colsum_out, N, cdiv(M, 128) * 2, colsum_beta, st);
  return rc;
}

// on: an F8_EPI_* bit mask (0 off, 0xff all); < 0 queries. Returns the old mask.
extern "C" int tdg_fp8_set_persist(int on) {
  const int old = fp8_persist_mask();
  if (on >= 0) g_fp8_persist = on;
  return old;
}
