// Attention forward, bf16: the short and the pipelined kernel, the
// probabilities kernel and their launchers (design: attn_impl.h). Holds
// definitions: include it from one translation unit only.
#pragma once
#include "attn_impl.h"

namespace tdg {

// ============================================================================ forward
// NWV waves per workgroup, U 16-query subtiles per wave (16 U NWV queries per
// workgroup; 8 x 1 covers a whole <= 128-query sequence, so K/V are read from
// HBM once per (batch, head)). Each K / V fragment read from LDS feeds U
// MFMAs: with U = 1 the fragment reads alone saturate the LDS at the MFMA
// rate (1 KiB per 16-cycle MFMA per wave), U = 2 halves them.
// KT keys per LDS tile (64 or 128: one load phase and one barrier pair for a
// whole <= 128-key sequence).
template <int HD, int NWV, int KT, int U>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn_fwd_kernel(AttnArgs a) {
  using T = ATile<HD>;
  constexpr int QBW = 16 * NWV * U;
  constexpr int NT16 = KT / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsK = smem;
  char* ldsV = smem + (KT / 64) * T::BYTES;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, cl = lane & 15;
  int xb, h, b;
  attn_coords(a, xb, h, b);
  const int q0 = xb * QBW;
  int qrow[U];
#pragma unroll
  for (int u = 0; u < U; ++u) qrow[u] = q0 + 16 * (U * w + u) + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, q0 + QBW);

  TDG_STAMP(0);
  short8_t qf[U][T::KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bf16_t* qp = a.q + b * a.q_sb + (long long)min(qrow[u], a.Lq - 1) * a.q_sl + h * a.q_sh;
    TDG_LOAD_ROW_FRAGS(HD, lane, qrow[u] < a.Lq, qf[u], qp)
  }

  const bf16_t* kb = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + h * a.v_sh;
  const float c = scl * LOG2E;
  constexpr int KTILE = KT;
  const int wq0 = q0 + 16 * U * w;

  f32x4 oacc[U][T::DT];
  float m[U], l[U];
  TDG_ZERO(U, T::DT, oacc)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
  }

  // K / V tiles staged global -> registers -> LDS; the NEXT tile's loads are
  // issued right after the current one is in LDS, so they are in flight
  // during this tile's MFMAs (every load of a tile in flight before the
  // first LDS write, one memory latency per tile at most)
  typename T::template Chunks<NWV * 64> ck[KT / 64], cv[KT / 64];
  auto fetch_kv = [&](int kk0) {
#pragma unroll
    for (int h64 = 0; h64 < KT / 64; ++h64) {
      T::template fetch<NWV * 64>(ck[h64], kb, a.k_sl, kk0 + 64 * h64, a.Lk, tid);
      T::template fetch<NWV * 64>(cv[h64], vb, a.v_sl, kk0 + 64 * h64, a.Lk, tid);
    }
  };
  if (klim > 0) fetch_kv(0);
  for (int k0 = 0; k0 < klim; k0 += KT) {
#pragma unroll
    for (int h64 = 0; h64 < KT / 64; ++h64) {
      T::template put<NWV * 64>(ldsK + h64 * T::BYTES, ck[h64], tid);
      T::template put<NWV * 64>(ldsV + h64 * T::BYTES, cv[h64], tid);
    }
    __syncthreads();
    if (k0 == 0) TDG_STAMP(1);
    if (k0 + KT < klim) fetch_kv(k0 + KT);
    f32x4 s[U][NT16];
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
#pragma unroll
      for (int u = 0; u < U; ++u) s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
        const short8_t kfr = T::frag_row(ldsK, 16 * t, ks, lane);
#pragma unroll
        for (int u = 0; u < U; ++u) s[u][t] = mfma16(kfr, qf[u][ks], s[u][t]);
      }
    }
    short8_t pf[U][NT16 / 2];
#pragma unroll
    for (int u = 0; u < U; ++u)
      softmax_tile<NT16, T::DT>(s[u], m[u], l[u], oacc[u], pf[u], tile_masked(k0, KTILE, klim, causal, wq0),
                                k0, klim, causal, qrow[u], g, c);
#pragma unroll
    for (int s2 = 0; s2 < NT16 / 2; ++s2) {
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        const short8_t vfr = T::frag_tr(ldsV, s2, dt, lane);
#pragma unroll
        for (int u = 0; u < U; ++u) oacc[u][dt] = mfma16(vfr, pf[u][s2], oacc[u][dt]);
      }
    }
    __syncthreads();
  }
  TDG_STAMP(2);
#pragma unroll
  for (int u = 0; u < U; ++u) TDG_FWD_FINISH(T::DT, a, b, h, qrow[u], oacc[u], m[u], l[u], g)
#ifdef TDG_STAMPS
  TDG_STAMP(3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TDG_STAMP(4);
#endif
}

// ============================================================================ forward, long sequences
// hd = 64, Lq > 128. The K / V tiles (64 keys) stream through an NS-slot LDS
// ring by LDS-DMA (Glds: the ATile<64> image is the GEMM's K-contiguous
// 64-row image), NS-1 tiles in flight and one barrier per tile -- instead of
// global -> register -> LDS with one tile of register prefetch, which left
// the 512-key sequences latency-bound (0.31 PF/s). NWV waves x U 16-query
// subtiles per wave; the K / V fragment reads are shared by the U subtiles.
template <int NWV, int U, int NS>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn_fwd_pipe_kernel(AttnArgs a) {
  constexpr int HD = 64;
  using T = ATile<HD>;
  using G = Glds<true, 64, NWV>;  // 64 rows x 64 head-dim elements
  constexpr int QBW = 16 * NWV * U;
  constexpr int NT16 = 4;             // 16-key tiles per 64-key tile
  constexpr int SLOT = 2 * T::BYTES;  // K image, V image
  constexpr int PT = 2 * G::P;        // LDS-DMA per wave per tile
  static_assert(NS >= 3, "ring: refilled, being read, landed");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, h, b;
  attn_coords(a, xb, h, b);
  const int q0 = xb * QBW;
  int qrow[U];
#pragma unroll
  for (int u = 0; u < U; ++u) qrow[u] = q0 + 16 * (U * w + u) + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, q0 + QBW);
  const int nkt = (klim + 63) / 64;

  short8_t qf[U][T::KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bf16_t* qp = a.q + b * a.q_sb + (long long)min(qrow[u], a.Lq - 1) * a.q_sl + h * a.q_sh;
    TDG_LOAD_ROW_FRAGS(HD, lane, qrow[u] < a.Lq, qf[u], qp)
  }
  const bf16_t* kb = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + h * a.v_sh;
  G gs;
  gs.init(w, lane);
  auto issue = [&](int kt) {
    char* slot = smem + (kt % NS) * SLOT;
    gs.issue(kb, (int)a.k_sl, a.Lk, HD, 64 * kt, 0, slot, w);
    gs.issue(vb, (int)a.v_sl, a.Lk, HD, 64 * kt, 0, slot + T::BYTES, w);
  };
  // prologue tiles issued unconditionally (clamped rows past the sequence,
  // never read) so the DMA count behind the Q loads is a constant
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue(s);
  wait_vmcnt_known<(NS - 1) * PT>();  // Q fragments in registers

  const float c = scl * LOG2E;
  constexpr int KTILE = 64;
  const int wq0 = q0 + 16 * U * w;
  f32x4 oacc[U][T::DT];
  float m[U], l[U];
  TDG_ZERO(U, T::DT, oacc)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
  }
  for (int kt = 0; kt < nkt; ++kt) {
    // tile kt landed (this wave's DMA, then everyone's); every wave is past
    // its reads of tile kt-1, whose slot takes tile kt+NS-1
    wait_tiles<PT, NS - 2>(min(NS - 2, nkt - 1 - kt));
    lds_barrier();
    if (kt + NS - 1 < nkt) issue(kt + NS - 1);
    const char* ldsK = smem + (kt % NS) * SLOT;
    const char* ldsV = ldsK + T::BYTES;
    const int k0 = 64 * kt;
    // all LDS reads of the tile untracked (a tracked read would get a
    // vmcnt(0) for the DMA in flight), with counted waits: K fragments in
    // two halves, V fragments issued between the softmax's max and exp parts
    short8_t kfr[NT16][T::KS];
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) kfr[t][ks] = T::frag_row_async(ldsK, 16 * t, ks, lane);
    f32x4 s[U][NT16];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half == 0) lgkm_wait<NT16 * T::KS / 2>();
      else lgkm_wait<0>();
#pragma unroll
      for (int t = half * NT16 / 2; t < (half + 1) * NT16 / 2; ++t) {
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) tie(kfr[t][ks]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < T::KS; ++ks) s[u][t] = mfma16(kfr[t][ks], qf[u][ks], s[u][t]);
        }
      }
    }
    const bool msk = tile_masked(k0, KTILE, klim, causal, wq0);
#pragma unroll
    for (int u = 0; u < U; ++u)
      softmax_max<NT16, T::DT>(s[u], m[u], l[u], oacc[u], msk, k0, klim, causal, qrow[u], g, c);
    short4_t vlo[NT16 / 2][T::DT], vhi[NT16 / 2][T::DT];
#pragma unroll
    for (int s2 = 0; s2 < NT16 / 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) T::frag_tr_async(ldsV, s2, dt, lane, vlo[s2][dt], vhi[s2][dt]);
    short8_t pf[U][NT16 / 2];
#pragma unroll
    for (int u = 0; u < U; ++u) softmax_exp<NT16>(s[u], m[u], l[u], pf[u], msk ? 1.f : c);
#pragma unroll
    for (int s2 = 0; s2 < NT16 / 2; ++s2) {
      if (s2 == 0) lgkm_wait<2 * T::DT>();
      else lgkm_wait<0>();
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        tie(vlo[s2][dt]);
        tie(vhi[s2][dt]);
        const short8_t vfr = cat4(vlo[s2][dt], vhi[s2][dt]);
#pragma unroll
        for (int u = 0; u < U; ++u) oacc[u][dt] = mfma16(vfr, pf[u][s2], oacc[u][dt]);
      }
    }
  }
  wait_vmcnt<0>();  // (nothing in flight on the exit paths; keeps the grid drained)
#pragma unroll
  for (int u = 0; u < U; ++u) TDG_FWD_FINISH(T::DT, a, b, h, qrow[u], oacc[u], m[u], l[u], g)
}

// ============================================================================ probabilities (inference maps)
// One wave per (b, h, q) row: emits the full softmax row [Lk] in f32, the
// attention_weights the reference returns (transformer_model.py:104-109,
// tester.py:51-53). Not on the training path.
template <int HD>
__global__ void attn_probs_kernel(AttnArgs a, float* __restrict__ probs) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const long long total = (long long)a.B * a.H * a.Lq;
  if (row >= total) return;
  const int q = (int)(row % a.Lq);
  const int h = (int)((row / a.Lq) % a.H);
  const int b = (int)(row / ((long long)a.Lq * a.H));
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, q + 1);
  const bf16_t* qp = a.q + b * a.q_sb + (long long)q * a.q_sl + h * a.q_sh;
  float qv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) qv[d] = bf2f(qp[d]);
  float* out = probs + row * a.Lk;
  float mx = -INFINITY;
  for (int k = lane; k < klim; k += 64) {
    const bf16_t* kp = a.k + b * a.k_sb + (long long)k * a.k_sl + h * a.k_sh;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s += qv[d] * bf2f(kp[d]);
    s *= scl;
    out[k] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < klim; k += 64) {
    const float e = __expf(out[k] - mx);
    out[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  for (int k = lane; k < a.Lk; k += 64) out[k] = k < klim ? out[k] * inv : 0.f;
}

}  // namespace tdg

using namespace tdg;

namespace {
template <int HD>
int fwd_hd(const AttnArgs& a, hipStream_t st) {
  // (64 queries per workgroup for Lq > 64 -- twice the workgroups, K / V
  // staged by both halves -- measured 17.2 vs 12.2 us at B 64, H 8, L 128:
  // csrc/lab/attn_lab.cpp, profiles/attn_lab/)
  // hd 64, > 128 queries: LDS-DMA pipelined kernel, 8 waves x 16 queries,
  // 3-slot ring (seq 512: 40.5 us vs 41-45 for 4 slots or 32 queries per
  // wave, 47 for the register-staged kernel; profiles/r3/attn_seq512_*)
  if constexpr (HD == 64) {
    if (a.Lq > 128) {
      constexpr int NWV = 8, U = 1, NS = 3;
      big_lds<attn_fwd_pipe_kernel<NWV, U, NS>>();
      attn_plan_record(ATTN_FWD_PIPE, HD, (long long)cdiv(a.Lq, 16 * NWV * U) * a.H * a.B, NWV * 64);
      hipLaunchKernelGGL((attn_fwd_pipe_kernel<NWV, U, NS>), dim3(cdiv(a.Lq, 16 * NWV * U), a.H, a.B),
                         dim3(NWV * 64), NS * 2 * ATile<64>::BYTES, st, a);
      return 0;
    }
  }
  if (a.Lq > 64) {
    dim3 grid(cdiv(a.Lq, 128), a.H, a.B);
    // 4 waves x 2 query subtiles (each K / V fragment read from LDS feeds two
    // MFMAs; 225 VGPRs, two 4-wave workgroups per CU): 9.6 vs 10.3 us (causal
    // 10.3 vs 11.7) for 8 waves x 1 subtile, whose 142 VGPRs fit only one
    // 8-wave workgroup per CU -- the 512 (batch, head) items ran in two
    // rounds (profiles/r3s2/attn_short_fwd_variants.txt); headline step
    // 5.04-5.06 vs 5.07-5.08 ms A/B (profiles/r3s2/attn_short_fwd_ab.txt)
    // (hd 128: 8 waves x 1 subtile, two subtiles per wave would spill)
    attn_plan_record(HD <= 64 ? ATTN_FWD128 : ATTN_FWD128W8, HD, (long long)grid.x * grid.y * grid.z,
                     HD <= 64 ? 256 : 512);
    if constexpr (HD <= 64)
      hipLaunchKernelGGL((attn_fwd_kernel<HD, 4, 128, 2>), grid, dim3(256), 4 * ATile<HD>::BYTES, st, a);
    else
      hipLaunchKernelGGL((attn_fwd_kernel<HD, 8, 128, 1>), grid, dim3(512), 4 * ATile<HD>::BYTES, st, a);
  } else {
    dim3 grid(cdiv(a.Lq, 64), a.H, a.B);
    attn_plan_record(ATTN_FWD64, HD, (long long)grid.x * grid.y * grid.z, 256);
    hipLaunchKernelGGL((attn_fwd_kernel<HD, 4, 64, 1>), grid, dim3(256), 2 * ATile<HD>::BYTES, st, a);
  }
  return 0;
}
template <int HD>
int probs_hd(const AttnArgs& a, float* probs, hipStream_t st) {
  const long long rows = (long long)a.B * a.H * a.Lq;
  attn_plan_record(ATTN_PROBS, HD, (rows + 3) / 4, 256);
  hipLaunchKernelGGL(attn_probs_kernel<HD>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a,
                     probs);
  return 0;
}
}  // namespace

// (the record every bf16 attention launcher writes: attn_impl.h attn_plan_record)
extern "C" void tdg_attn_last_plan(int out[5]) {
  const int* p = attn_plan_slot();
  for (int i = 0; i < 5; ++i) out[i] = p[i];
}
extern "C" int tdg_attn_fwd(const AttnArgs* a, int hd, hipStream_t st) {
  TDG_HD_CASES(fwd_hd, *a, st)
}
extern "C" int tdg_attn_probs(const AttnArgs* a, int hd, float* probs, hipStream_t st) {
  TDG_HD_CASES(probs_hd, *a, probs, st)
}
