// The half-stage ring fp8 GEMM kernel (included by fp8_gemm.hip).
#pragma once
#include "fp8_epi.h"

namespace tdg {

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
  TDG_F8_TILE_RASTER(t, tiles_m, tiles_n, tm, tn)
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
  TDG_F8_ZERO_ACC(2, 2, acc)
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
    TDG_F8_MFMA_BLOCK(2, 2, __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4, AF, acc, fa, fb)
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

}  // namespace tdg
