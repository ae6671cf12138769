// Device pieces shared by the fp8 kernel families (fp8_gemm.hip,
// fp8_wgrad.hip, fp8_quant.hip): the 128-byte-row LDS images and their
// fragment reads, the pack / unpack helpers, and the steps more than one
// kernel runs (tile raster, MFMA block, the four-phase 256x256 K loop,
// quantise-eight, workgroup amax).
//
// Only the straight-line value helpers (quant8, quant1, quant8_byte,
// amax_record) are functions; every other shared step is a statement macro,
// because as an inlined function it changed some kernel's machine code
// (docs/KERNELS.md "Refactoring a kernel file").
#pragma once
#include "tdg_common.h"

#include <type_traits>

namespace tdg {

typedef int i32x8 __attribute__((ext_vector_type(8)));
// E4M3_MAX, AMAX_SPREAD, pack2_e4m3, atomic_amax: tdg_common.h (each amax slot
// is AMAX_SPREAD words; producers pick one by block id so the atomics of a
// large grid do not serialise on one address)
constexpr int BK8 = 128;  // K elements (= bytes) per tile row

namespace f8 {

__device__ __forceinline__ int lds_off(int row, int byte) {
  const int seg = (byte >> 5) ^ ((row >> 1) & 3);
  return row * BK8 + (seg << 5) + (byte & 31);
}

// global -> LDS staging of an R x 128-byte K-contiguous tile (as Glds<KC> in tdg_gemm.h)
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

// Quantise eight values: (lo, hi) = the eight fp8 bytes of f[0..7] * s, in order
template <int FMT>
__device__ __forceinline__ void quant8(const float (&f)[8], float s, int& lo, int& hi) {
  lo = pack2_f8<FMT, false>(f[0] * s, f[1] * s, 0);
  lo = pack2_f8<FMT, true>(f[2] * s, f[3] * s, lo);
  hi = pack2_f8<FMT, false>(f[4] * s, f[5] * s, 0);
  hi = pack2_f8<FMT, true>(f[6] * s, f[7] * s, hi);
}
// ... and one value (the scalar tails)
template <int FMT>
__device__ __forceinline__ uint8_t quant1(float f, float s) {
  return (uint8_t)(pack2_f8<FMT, false>(f * s, 0.f, 0) & 0xff);
}
// byte e (0..7) of quant8's (lo, hi), for ragged tails (bytes by shifts:
// taking &lo / &hi put them in scratch memory)
__device__ __forceinline__ uint8_t quant8_byte(int lo, int hi, int e) {
  return (uint8_t)((uint32_t)(e < 4 ? lo : hi) >> (8 * (e & 3)));
}

// Workgroup amax of a 256-thread block, in two halves around the caller's
// __syncthreads(): every wave leaves its max in red[4] (tid: threadIdx.x as
// the kernel holds it; a macro: as a function it changed the transposing
// quantise kernel's code), then ONE thread records the block's (one atomic
// per block: thousands of same-address atomics serialise in L2)
#define TDG_F8_AMAX_STAGE(red, amax, tid) \
  amax = wave_max(amax);                  \
  if (((tid) & 63) == 0) red[(tid) >> 6] = amax;
__device__ __forceinline__ void amax_record(const float (&red)[4], unsigned* word) {
  atomic_amax(word, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

}  // namespace f8

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

// the 256x256 one-wave-per-SIMD tiles (gemm_fp8_w1_kernel, wgrad_fp8_kernel)
namespace f8w1 {
constexpr int HB = 128 * BK8;  // bytes of a half-tile image
// image row x (0..127) of half h -> tile row / column
__device__ __forceinline__ int remap(int x, int h) { return (x >> 6) * 128 + h * 64 + (x & 63); }
}  // namespace f8w1

// Tile raster: (tm, tn) of tile t of a tiles_m x tiles_n grid (t already
// through xcd_remap), walking the shorter dimension fastest. (As functions,
// this and the zeroing below changed the kernels' code.)
#define TDG_F8_TILE_RASTER(t, tiles_m, tiles_n, tm, tn) \
  if ((tiles_n) <= (tiles_m)) {                         \
    tn = (t) % (tiles_n);                               \
    tm = (t) / (tiles_n);                               \
  } else {                                              \
    tm = (t) % (tiles_m);                               \
    tn = (t) / (tiles_m);                               \
  }

// Accumulator zeroing: acc[TM_][TN_] of f32 vectors (f32x4 of the 16x16
// MFMAs, f32x16 of the 32x32)
#define TDG_F8_ZERO_ACC(TM_, TN_, acc)                                                 \
  _Pragma("unroll") for (int i_ = 0; i_ < TM_; ++i_)                                   \
      _Pragma("unroll") for (int j_ = 0; j_ < TN_; ++j_)                               \
          _Pragma("unroll") for (int r_ = 0; r_ < (int)(sizeof(acc[0][0]) / sizeof(float)); ++r_) \
              acc[i_][j_][r_] = 0.f;

// MFMA block of one K step: the TM_ x TN_ grid acc[i][j] = MFMA_(fa[i], fb[j],
// acc[i][j]) of a block-scaled MFMA with unit scales (A format AF_, B e4m3)
// on fragments read untracked -- wait for them, tie them (orders the MFMAs
// after the wait), raised priority across the grid, and a scheduling fence.
#define TDG_F8_MFMA_BLOCK(TM_, TN_, MFMA_, AF_, acc, fa, fb)                           \
  {                                                                                    \
    tdg::lgkm_wait<0>();                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < TM_; ++i_) tdg::tie(fa[i_]);               \
    _Pragma("unroll") for (int j_ = 0; j_ < TN_; ++j_) tdg::tie(fb[j_]);               \
    __builtin_amdgcn_s_setprio(1);                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < TM_; ++i_)                                 \
        _Pragma("unroll") for (int j_ = 0; j_ < TN_; ++j_) acc[i_][j_] =               \
            MFMA_(fa[i_], fb[j_], acc[i_][j_], AF_, 0, 0, 127, 0, 127);                \
    __builtin_amdgcn_s_setprio(0);                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  }

// The K loop of a 256x256 tile at one wave per SIMD (gemm_fp8_w1_kernel's
// block comment has the schedule): prologue (tiles 0 and 1 in flight; A0(0),
// B0(0) landed and read), then one K step (128 deep) in four phases per
// tile. FRAG_(image, base, lane) reads a fragment, mfma(i, j) is the kernel's
// MFMA on fa[i], fb[j]; issue(kt, q) stages half q of tile kt (0 = A0,
// 1 = B0, 2 = B1, 3 = A1: the issue order). Uses the kernel's smem, HB, SB,
// nk, lane, ar / br (the wave's rows / columns in a half image), fa, fb.
//
// MODE 2: tiles kt+1 and kt+2 exist; 1: only kt+1; 0: the last tile. The
// steady loop is branch-free (the tail steps are separate instantiations):
// with `if (more2)` branches inside the body the compiler sank all 64 MFMAs
// of a step out of their phases into the loop latch, behind every wait and
// barrier (measured ISA, scripts/isa_loops.py), which serialised the DMA /
// LDS work and the MFMAs. sched_barrier(0) pins each phase's boundary.
#define TDG_F8_PHASE_MFMAS(i0, j0)                                                     \
  __builtin_amdgcn_s_setprio(1);                                                       \
  _Pragma("unroll") for (int i = i0; i < i0 + 4; ++i)                                  \
      _Pragma("unroll") for (int j = j0; j < j0 + 4; ++j) mfma(i, j);                  \
  __builtin_amdgcn_s_setprio(0);                                                       \
  __builtin_amdgcn_sched_barrier(0);
#define TDG_F8_FOUR_PHASE_K_LOOP(FRAG_, mfma, issue)                                   \
  _Pragma("unroll") for (int q = 0; q < 4; ++q) issue(0, q);                           \
  if (nk > 1) {                                                                        \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) issue(1, q);                         \
    f8::wait_vmcnt<24>();                                                              \
  } else {                                                                             \
    f8::wait_vmcnt<8>();                                                               \
  }                                                                                    \
  f8::lds_barrier();                                                                   \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) fa[i] = FRAG_(smem + 0 * HB, ar + 16 * i, lane); \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) fb[j] = FRAG_(smem + 2 * HB, br + 16 * j, lane); \
  auto kstep = [&](int kt, auto modec) {                                               \
    constexpr int MODE = decltype(modec)::value;                                       \
    constexpr bool more1 = MODE >= 1, more2 = MODE == 2;                               \
    const char* st = smem + (kt & 1) * SB;                                             \
    const char* nx = smem + ((kt + 1) & 1) * SB;                                       \
    /* ---- P0: a0 x b0; read B1(kt); issue A0(kt+2) */                                \
    /* B1(kt) landed: younger issues A1(kt), A0/B0/B1/A1(kt+1) -- or fewer at the tail */ \
    if constexpr (more1) f8::wait_vmcnt<20>();                                         \
    else f8::wait_vmcnt<4>();                                                          \
    f8::lds_barrier(); /* (lgkmcnt(0): last phase's fragment reads) */                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) tdg::tie(fb[j]);                     \
    if constexpr (more2) issue(kt + 2, 0);                                             \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) fb[j] = FRAG_(st + 3 * HB, br + 16 * (j - 4), lane); \
    TDG_F8_PHASE_MFMAS(0, 0)                                                           \
    /* ---- P1: a0 x b1; read A1(kt); issue B0(kt+2) */                                \
    /* A1(kt) landed: younger A0/B0/B1/A1(kt+1), A0(kt+2) */                           \
    if constexpr (more2) f8::wait_vmcnt<20>();                                         \
    else if constexpr (more1) f8::wait_vmcnt<16>();                                    \
    else f8::wait_vmcnt<0>();                                                          \
    f8::lds_barrier();                                                                 \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) tdg::tie(fb[j]);                     \
    if constexpr (more2) issue(kt + 2, 1);                                             \
    _Pragma("unroll") for (int i = 4; i < 8; ++i) fa[i] = FRAG_(st + 1 * HB, ar + 16 * (i - 4), lane); \
    TDG_F8_PHASE_MFMAS(0, 4)                                                           \
    /* ---- P2: a1 x b1; read A0(kt+1); issue B1(kt+2) */                              \
    /* A0(kt+1) landed: younger B0/B1/A1(kt+1), A0/B0(kt+2) */                         \
    if constexpr (more2) f8::wait_vmcnt<20>();                                         \
    else if constexpr (more1) f8::wait_vmcnt<12>();                                    \
    else f8::wait_vmcnt<0>();                                                          \
    f8::lds_barrier();                                                                 \
    _Pragma("unroll") for (int i = 4; i < 8; ++i) tdg::tie(fa[i]);                     \
    if constexpr (more2) issue(kt + 2, 2);                                             \
    if constexpr (more1) {                                                             \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) fa[i] = FRAG_(nx + 0 * HB, ar + 16 * i, lane); \
    }                                                                                  \
    TDG_F8_PHASE_MFMAS(4, 4)                                                           \
    /* ---- P3: a1 x b0; read B0(kt+1) per column behind its MFMAs; issue A1(kt+2) */  \
    /* B0(kt+1) landed: younger B1/A1(kt+1), A0/B0/B1(kt+2) */                         \
    if constexpr (more2) f8::wait_vmcnt<20>();                                         \
    else if constexpr (more1) f8::wait_vmcnt<8>();                                     \
    else f8::wait_vmcnt<0>();                                                          \
    f8::lds_barrier();                                                                 \
    if constexpr (more1) {                                                             \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) tdg::tie(fa[i]);                   \
    }                                                                                  \
    if constexpr (more2) issue(kt + 2, 3);                                             \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                    \
      __builtin_amdgcn_s_setprio(1);                                                   \
      _Pragma("unroll") for (int i = 4; i < 8; ++i) mfma(i, j);                        \
      __builtin_amdgcn_s_setprio(0);                                                   \
      if constexpr (more1) fb[j] = FRAG_(nx + 2 * HB, br + 16 * j, lane);              \
    }                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  };                                                                                   \
  {                                                                                    \
    int kt = 0;                                                                        \
    for (; kt + 2 < nk; ++kt) kstep(kt, std::integral_constant<int, 2>{});             \
    if (kt + 1 < nk) kstep(kt++, std::integral_constant<int, 1>{});                    \
    kstep(kt, std::integral_constant<int, 0>{});                                       \
  }

}  // namespace tdg
