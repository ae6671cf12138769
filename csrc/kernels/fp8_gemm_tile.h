// The 128-byte-K-step fp8 GEMM tile kernel and its persistent form (included
// by fp8_gemm.hip).
#pragma once
#include "fp8_epi.h"

namespace tdg {

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

// The wave's TM A and TN B fragments of the stage at img (the A image, then
// the B image; the kernel's frag_b reads K- or N-contiguous B)
#define TDG_F8_LOAD_FRAGS(img)                                                                       \
  _Pragma("unroll") for (int i_ = 0; i_ < TM; ++i_) fa[i_] = f8::frag(img, abase + 16 * i_, lane);   \
  _Pragma("unroll") for (int j_ = 0; j_ < TN; ++j_) fb[j_] = frag_b((img) + A_BYTES, bbase + 16 * j_);

// AF: format of A (0 e4m3, 1 e5m2: the gradient operand of a dgrad), B is
// e4m3; CF: format of the optional C8 copy.
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
  TDG_F8_TILE_RASTER(t, tiles_m, tiles_n, tm, tn)
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
  TDG_F8_ZERO_ACC(TM, TN, acc)

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
  TDG_F8_LOAD_FRAGS(smem)

  // MODE 2: tile kt + STAGES exists (steady, branch-free); 1: kt + 1 exists
  // (tail: drain, no issue); 0: the last tile. With the tail's branches
  // inside one loop body the compiler sank the MFMAs past the wait, barrier,
  // DMA issue and fragment reads into the latch (scripts/isa_loops.py).
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    TDG_F8_MFMA_BLOCK(TM, TN, __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4, AF, acc, fa, fb)
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
      TDG_F8_LOAD_FRAGS(nx)
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
    TDG_F8_TILE_RASTER(t, tiles_m, tiles_n, tm, tn)
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
    TDG_F8_ZERO_ACC(TM, TN, acc)
    // K step 0 landed (younger: K step 1 -- and nothing else outstanding
    // is younger than step 0 but the epilogue stores / prefetch, waited too)
    f8::wait_vmcnt<PT>();
    f8::lds_barrier();
    i32x8 fa[TM], fb[TN];
    {
      const char* st0 = smem + sl0 * SB;
      TDG_F8_LOAD_FRAGS(st0)
    }
    // MODE 2: step kt + 2 exists (issue it into the vacated stage); 1: the
    // last-but-one step (issue the next tile's step 0 there); 0: the last
    auto kstep = [&](int kt, auto modec) {
      constexpr int MODE = decltype(modec)::value;
      TDG_F8_MFMA_BLOCK(TM, TN, __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4, AF, acc, fa, fb)
      if constexpr (MODE >= 1) {
        f8::wait_vmcnt<0>();
        f8::lds_barrier();
        char* cur = smem + ((kt + sl0) & 1) * SB;
        if constexpr (MODE == 2) issue(gb, m0, n0, kt + 2, cur);
        else if (more) issue(gbn, m0n, n0n, 0, cur);
        const char* nx = smem + ((kt + 1 + sl0) & 1) * SB;
        TDG_F8_LOAD_FRAGS(nx)
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

}  // namespace tdg
