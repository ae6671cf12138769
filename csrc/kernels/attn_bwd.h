// Attention backward, bf16: the dQ and dK/dV pairs (register-staged and
// pipelined), the fused short-sequence backward and their launchers (design:
// attn_impl.h). Holds definitions: include it from one translation unit only.
#pragma once
#include "attn_impl.h"

namespace tdg {

// Does query q attend to key `key`? The mask of every P / dS recompute below:
// inside the key window, a real query row, at or below the causal diagonal
// (no short circuit: no branches; macros for the reason given in attn_impl.h)
#define TDG_ATTENDS(key, q, klim, Lq, causal) \
  (((key) < (klim)) & ((q) < (Lq)) & (!(causal) | ((key) <= (q))))
// P and dS = P (dP - delta) of one 16 x 16 tile, recomputed from the raw
// logits sv, the forward's lse and dpv = dP, with the KEY on the lane (key[u],
// U subtiles): element r is query q4 + r, its lse / delta lse[r] / del[r].
// full (wave-uniform): every (query, key) of the tile valid, no per-element mask.
#define TDG_PDS_KEY_LANE(U_, full, sv, dpv, lse, del, c, key, q4, klim, Lq, causal, p, ds)   \
  if (full) {                                                                                \
    _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_)                                         \
    _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_) {                                      \
      const float pv_ = fast_exp2((sv)[u_][r_] * (c) - (lse)[r_]);                           \
      (p)[u_][r_] = pv_;                                                                     \
      (ds)[u_][r_] = pv_ * ((dpv)[u_][r_] - (del)[r_]);                                      \
    }                                                                                        \
  } else {                                                                                   \
    _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                       \
      const int q_ = (q4) + r_;                                                              \
      _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_) {                                    \
        const bool ok_ = TDG_ATTENDS((key)[u_], q_, klim, Lq, causal);                       \
        const float pv_ = masked_exp2((sv)[u_][r_] * (c) - (lse)[r_], ok_);                  \
        (p)[u_][r_] = pv_;                                                                   \
        (ds)[u_][r_] = pv_ * ((dpv)[u_][r_] - (del)[r_]);                                    \
      }                                                                                      \
    }                                                                                        \
  }
// The same with the QUERY on the lane (qrow[u], lse / delta L[u] / D[u]):
// element r is key k4 + r; only dS is needed
#define TDG_DS_QUERY_LANE(U_, full, sv, dpv, L, D, c, qrow, k4, klim, Lq, causal, ds)        \
  if (full) {                                                                                \
    _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_)                                         \
    _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_)                                        \
      (ds)[u_][r_] = fast_exp2((sv)[u_][r_] * (c) - (L)[u_]) * ((dpv)[u_][r_] - (D)[u_]);    \
  } else {                                                                                   \
    _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                       \
      const int key_ = (k4) + r_;                                                            \
      _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_) {                                    \
        const bool ok_ = TDG_ATTENDS(key_, (qrow)[u_], klim, Lq, causal);                    \
        const float pv_ = masked_exp2((sv)[u_][r_] * (c) - (L)[u_], ok_);                    \
        (ds)[u_][r_] = pv_ * ((dpv)[u_][r_] - (D)[u_]);                                      \
      }                                                                                      \
    }                                                                                        \
  }

// ============================================================================ dK, dV
// 4 waves, U 16-key subtiles per wave (64 U keys per workgroup): every Q / dO
// fragment read from LDS feeds U MFMAs.
template <int HD, int U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_bwd_dkdv_kernel(AttnArgs a) {
  using T = ATile<HD>;
  constexpr int KBW = 64 * U;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsQ = smem;
  char* ldsO = smem + T::BYTES;  // dO tile
  float* ldsL = reinterpret_cast<float*>(smem + 2 * T::BYTES);
  float* ldsD = ldsL + QB;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: scalar branches)
  int xb, h, b;
  attn_coords(a, xb, h, b);
  const int k0 = xb * KBW;
  int key[U];
#pragma unroll
  for (int u = 0; u < U; ++u) key[u] = k0 + 16 * (U * w + u) + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  const float c = scl * LOG2E;

  f32x4 dk[U][T::DT], dv[U][T::DT];
  TDG_ZERO2(U, T::DT, dk, dv)

  if (k0 < klim) {
    short8_t kf[U][T::KS], vf[U][T::KS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int krow = min(key[u], a.Lk - 1);
      const bf16_t* kp = a.k + b * a.k_sb + (long long)krow * a.k_sl + h * a.k_sh;
      const bf16_t* vp = a.v + b * a.v_sb + (long long)krow * a.v_sl + h * a.v_sh;
      TDG_LOAD_ROW_FRAGS2(HD, lane, key[u] < a.Lk, kf[u], kp, vf[u], vp)
    }
    const bf16_t* qb = a.q + b * a.q_sb + h * a.q_sh;
    const bf16_t* ob = a.dout + b * a.do_sb + h * a.do_sh;
    const float* lse = a.lse + ((long long)b * a.H + h) * a.Lq;
    const float* del = a.delta + ((long long)b * a.H + h) * a.Lq;
    const int qstart = causal ? (k0 / QB) * QB : 0;
    // Q / dO / lse / delta of query block q0+QB are loaded into registers
    // while block q0 is computed (register prefetch, single LDS buffer)
    typename T::template Chunks<256> cq, co;
    float lv = INFINITY, dlv = 0.f;
    auto fetch_q = [&](int qq0) {
      T::template fetch<256>(cq, qb, a.q_sl, qq0, a.Lq, tid);
      T::template fetch<256>(co, ob, a.do_sl, qq0, a.Lq, tid);
      if (tid < QB) {
        const int q = qq0 + tid;
        lv = q < a.Lq ? lse[q] : INFINITY;
        dlv = q < a.Lq ? del[q] : 0.f;
      }
    };
    if (qstart < a.Lq) fetch_q(qstart);
    for (int q0 = qstart; q0 < a.Lq; q0 += QB) {
      T::template put<256>(ldsQ, cq, tid);
      T::template put<256>(ldsO, co, tid);
      if (tid < QB) {
        ldsL[tid] = lv;
        ldsD[tid] = dlv;
      }
      __syncthreads();
      if (q0 + QB < a.Lq) fetch_q(q0 + QB);
      // S[q][key] and dP[q][key]: rows q = q0 + 16t + 4g + r, col key (lane)
      short8_t pf[U][2], dsf[U][2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        f32x4 p[2][U], ds[2][U];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int t = 2 * s2 + tt;
          f32x4 sv[U], dpv[U];
#pragma unroll
          for (int u = 0; u < U; ++u) sv[u] = dpv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < T::KS; ++ks) {
            const short8_t qfr = T::frag_row(ldsQ, 16 * t, ks, lane);
            const short8_t ofr = T::frag_row(ldsO, 16 * t, ks, lane);
#pragma unroll
            for (int u = 0; u < U; ++u) {
              sv[u] = mfma16(qfr, kf[u][ks], sv[u]);
              dpv[u] = mfma16(ofr, vf[u][ks], dpv[u]);
            }
          }
          // (TDG_PDS_KEY_LANE's masked branch written out: lse / delta are read
          // per query here, and as the macro those LDS reads are merged otherwise)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = 16 * t + 4 * g + r;
            const int q = q0 + ql;
            const float lq = ldsL[ql], dq = ldsD[ql];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const bool ok = TDG_ATTENDS(key[u], q, klim, a.Lq, causal);
              const float pv = masked_exp2(sv[u][r] * c - lq, ok);
              p[tt][u][r] = pv;
              ds[tt][u][r] = pv * (dpv[u][r] - dq);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pf[u][s2] = pack8(p[0][u], p[1][u]);
          dsf[u][s2] = pack8(ds[0][u], ds[1][u]);
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int dt = 0; dt < T::DT; ++dt) {
          const short8_t ot = T::frag_tr(ldsO, s2, dt, lane);
          const short8_t qt = T::frag_tr(ldsQ, s2, dt, lane);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            dv[u][dt] = mfma16(ot, pf[u][s2], dv[u][dt]);
            dk[u][dt] = mfma16(qt, dsf[u][s2], dk[u][dt]);
          }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = key[u] < a.Lk;
    bf16_t* dkp = a.dk + b * a.dk_sb + (long long)key[u] * a.dk_sl + h * a.dk_sh;
    bf16_t* dvp = a.dv + b * a.dv_sb + (long long)key[u] * a.dv_sl + h * a.dv_sh;
    uint32_t lo[T::DT], hi[T::DT];
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dkp, dk[u], a.scale, g, ok)
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dvp, dv[u], 1.f, g, ok)
  }
}

// ============================================================================ dQ
// 4 waves, U 16-query subtiles per wave (64 U queries per workgroup): every
// K / V fragment read from LDS feeds U MFMAs.
template <int HD, int U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_bwd_dq_kernel(AttnArgs a) {
  using T = ATile<HD>;
  constexpr int QBW = 64 * U;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsK = smem;
  char* ldsV = smem + T::BYTES;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: scalar branches)
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
  const float c = scl * LOG2E;
  short8_t qf[U][T::KS], of[U][T::KS];
  float L[U], D[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool qvalid = qrow[u] < a.Lq;
    const int qr = min(qrow[u], a.Lq - 1);
    const bf16_t* qp = a.q + b * a.q_sb + (long long)qr * a.q_sl + h * a.q_sh;
    const bf16_t* dop = a.dout + b * a.do_sb + (long long)qr * a.do_sl + h * a.do_sh;
    TDG_LOAD_ROW_FRAGS2(HD, lane, qvalid, qf[u], qp, of[u], dop)
    const long long bh = ((long long)b * a.H + h) * a.Lq + qr;
    L[u] = a.lse[bh];
    // delta = rowsum(dO * O) of this lane's query row, from the dO fragments
    // already in registers and the matching O fragments (the 4 lane groups g
    // hold disjoint head-dim slices); written for the dK/dV kernel, which runs
    // after this one -- no separate delta pass over O and dO
    // (row_delta written out: with an O fragment array this kernel's loads are reordered)
    float d = 0.f;
    const bf16_t* opr = a.o + b * a.o_sb + (long long)qr * a.o_sl + h * a.o_sh;
#pragma unroll
    for (int s = 0; s < T::KS; ++s) {
      const short8_t ov = gfrag<HD>(opr, qvalid, s, lane);
#pragma unroll
      for (int e = 0; e < 8; ++e) d += bf2f((bf16_t)of[u][s][e]) * bf2f((bf16_t)ov[e]);
    }
    d = rows_sum(d);
    if (qvalid && g == 0) a.delta[bh] = d;
    D[u] = d;
  }
  const bf16_t* kb = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + h * a.v_sh;
  f32x4 dq[U][T::DT];
  TDG_ZERO(U, T::DT, dq)

  // K / V of key block k0+KB in registers while block k0 is computed
  typename T::template Chunks<256> ck, cv;
  if (klim > 0) {
    T::template fetch<256>(ck, kb, a.k_sl, 0, a.Lk, tid);
    T::template fetch<256>(cv, vb, a.v_sl, 0, a.Lk, tid);
  }
  for (int k0 = 0; k0 < klim; k0 += KB) {
    T::template put<256>(ldsK, ck, tid);
    T::template put<256>(ldsV, cv, tid);
    __syncthreads();
    if (k0 + KB < klim) {
      T::template fetch<256>(ck, kb, a.k_sl, k0 + KB, a.Lk, tid);
      T::template fetch<256>(cv, vb, a.v_sl, k0 + KB, a.Lk, tid);
    }
    short8_t dsf[U][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      f32x4 ds[2][U];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * s2 + tt;
        f32x4 sv[U], dpv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sv[u] = dpv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) {
          const short8_t kfr = T::frag_row(ldsK, 16 * t, ks, lane);
          const short8_t vfr = T::frag_row(ldsV, 16 * t, ks, lane);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            sv[u] = mfma16(kfr, qf[u][ks], sv[u]);
            dpv[u] = mfma16(vfr, of[u][ks], dpv[u]);
          }
        }
        // (every tile takes the masked branch)
        TDG_DS_QUERY_LANE(U, false, sv, dpv, L, D, c, qrow, k0 + 16 * t + 4 * g, klim, a.Lq, causal, ds[tt])
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        dsf[u][s2] = pack8(ds[0][u], ds[1][u]);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        const short8_t kt = T::frag_tr(ldsK, s2, dt, lane);
#pragma unroll
        for (int u = 0; u < U; ++u) dq[u][dt] = mfma16(kt, dsf[u][s2], dq[u][dt]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    TDG_STORE_GRAD_ROW(T::DT, a.dq, a.dq_sb, a.dq_sl, a.dq_sh, b, h, qrow[u], a.Lq, dq[u], a.scale, g)
  }
}

// ============================================================================ backward, long sequences, pipelined
// hd = 64, the dQ / dK,dV kernels above with their streamed operand tiles in
// an NS-slot LDS-DMA ring (as attn_fwd_pipe_kernel): dK/dV streams Q, dO and
// the tile's lse / delta (one 4-byte-per-lane DMA per wave: wave 0 lse, wave 1
// delta, the others a scratch copy so every wave's DMA count is the same),
// dQ streams K and V.
// e5m2 copy of a 4-wave workgroup's gradient tile (the hd-64 pipelined
// backward kernels): lane (g, cl) of wave w holds rows rows[u] (u < U),
// columns 16 dt + 4 g .. +3 of one head. Writes the e5m2 values of the
// bf16-rounded x * sc, records their |max| (one atomic per wave) and, when
// part != null, the columns' sums over the workgroup's valid rows into
// part[0..63] (shuffles over the 16 rows of a lane group, then the 4 waves
// through `red`, 1 KiB of LDS). Every thread of the workgroup must call it.
template <int U>
__device__ __forceinline__ void attn_emit_g8(const f32x4 (&x)[U][4], float sc, const int (&rows)[U],
                                             int nrows, uint8_t* base8, long long sl, float s8,
                                             unsigned* amax, float* part, float* red, int lane,
                                             int w) {
  const int g = lane >> 4;
  float cs[4][4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[dt][r] = 0.f;
  float am = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = rows[u] < nrows;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = ok ? bf2f(f2bf(x[u][dt][r] * sc)) : 0.f;
        cs[dt][r] += v[r];
        am = fmaxf(am, fabsf(v[r]));
      }
      int w8 = pack2_e5m2c<false>(v[0] * s8, v[1] * s8, 0);
      w8 = pack2_e5m2c<true>(v[2] * s8, v[3] * s8, w8);
      if (ok) *reinterpret_cast<int*>(base8 + (long long)rows[u] * sl + 16 * dt + 4 * g) = w8;
    }
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) am = fmaxf(am, __shfl_xor(am, sh, 64));
  if (lane == 0) atomic_amax(amax_word(amax, blockIdx.x + 5 * blockIdx.y + 11 * blockIdx.z + w), am);
  if (!part) return;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int sh = 1; sh < 16; sh <<= 1) cs[dt][r] += __shfl_xor(cs[dt][r], sh, 64);
  __syncthreads();  // (the caller's LDS reads are done)
  if ((lane & 15) == 0) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w * 64 + 16 * dt + 4 * g + r] = cs[dt][r];
  }
  __syncthreads();
  if (threadIdx.x < 64)
    part[threadIdx.x] = red[threadIdx.x] + red[64 + threadIdx.x] + red[128 + threadIdx.x] +
                        red[192 + threadIdx.x];
  __syncthreads();
}

template <int U, int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_bwd_dkdv_pipe_kernel(AttnArgs a) {
  constexpr int HD = 64;
  using T = ATile<HD>;
  using G = Glds<true, 64, 4>;
  constexpr int KBW = 64 * U;
  constexpr int SLOT = 2 * T::BYTES + 3 * 256;  // Q, dO images, lse, delta, scratch
  constexpr int PT = 2 * G::P + 1;
  static_assert(NS >= 3, "ring: refilled, being read, landed");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, h, b;
  attn_coords(a, xb, h, b);
  const int k0 = xb * KBW;
  int key[U];
#pragma unroll
  for (int u = 0; u < U; ++u) key[u] = k0 + 16 * (U * w + u) + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  const float c = scl * LOG2E;
  const int kmaxw = k0 + 16 * U * (w + 1) - 1;  // the wave's last key

  f32x4 dk[U][T::DT], dv[U][T::DT];
  TDG_ZERO2(U, T::DT, dk, dv)

  const int qstart = causal ? (k0 / 64) * 64 : 0;
  const int nqt = k0 < klim && qstart < a.Lq ? (a.Lq - qstart + 63) / 64 : 0;
  short8_t kf[U][T::KS], vf[U][T::KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int krow = min(key[u], a.Lk - 1);
    const bf16_t* kp = a.k + b * a.k_sb + (long long)krow * a.k_sl + h * a.k_sh;
    const bf16_t* vp = a.v + b * a.v_sb + (long long)krow * a.v_sl + h * a.v_sh;
    TDG_LOAD_ROW_FRAGS2(HD, lane, key[u] < a.Lk, kf[u], kp, vf[u], vp)
  }
  const bf16_t* qb = a.q + b * a.q_sb + h * a.q_sh;
  const bf16_t* ob = a.dout + b * a.do_sb + h * a.do_sh;
  const float* vecs = (w == 1 ? a.delta : a.lse) + ((long long)b * a.H + h) * a.Lq;
  const int voff = 2 * T::BYTES + 256 * min(w, 2);
  G gs;
  gs.init(w, lane);
  auto issue = [&](int it) {
    const int q0 = qstart + 64 * it;
    char* slot = smem + (it % NS) * SLOT;
    gs.issue(qb, (int)a.q_sl, a.Lq, HD, q0, 0, slot, w);
    gs.issue(ob, (int)a.do_sl, a.Lq, HD, q0, 0, slot + T::BYTES, w);
    __builtin_amdgcn_global_load_lds((const void*)(vecs + min(q0 + lane, a.Lq - 1)),
                                     (__attribute__((address_space(3))) void*)(slot + voff), 4, 0, 0);
  };
  // prologue tiles issued unconditionally (clamped rows, never read) so the
  // DMA count behind the K / V fragment loads is a constant
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue(s);
  wait_vmcnt_known<(NS - 1) * PT>();

  uint32_t roff[T::KS], troff[T::DT];  // lane parts of the fragment addresses
#pragma unroll
  for (int ks = 0; ks < T::KS; ++ks) roff[ks] = T::row_off(ks, lane);
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) troff[dt] = T::tr_off(dt, lane);
  for (int it = 0; it < nqt; ++it) {
    wait_tiles<PT, NS - 2>(min(NS - 2, nqt - 1 - it));
    lds_barrier();
    if (it + NS - 1 < nqt) issue(it + NS - 1);
    const uint32_t slotQ = (uint32_t)(uintptr_t)smem + (uint32_t)((it % NS) * SLOT);
    const uint32_t slotO = slotQ + T::BYTES;
    const char* ldsL = smem + (it % NS) * SLOT + 2 * T::BYTES;  // lse, then delta (64 floats each)
    const int q0 = qstart + 64 * it;
    // untracked LDS reads with counted waits (a tracked read would get a
    // vmcnt(0) for the DMA in flight); the next 16-query tile's Q / dO
    // fragments and lse / delta are requested before this one is used; row
    // bases in the DS offset field
    uint32_t qra[T::KS], ora[T::KS];
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      qra[ks] = slotQ + roff[ks];
      ora[ks] = slotO + roff[ks];
    }
    const uint32_t lda4 = (uint32_t)(uintptr_t)ldsL + 16 * g;
    short8_t pf[U][2], dsf[U][2];
    short8_t qfr[2][T::KS], ofr[2][T::KS];
    f32x4 l4[2], d4[2];
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      qfr[0][ks] = T::template frag_row_at<0>(qra[ks]);
      ofr[0][ks] = T::template frag_row_at<0>(ora[ks]);
    }
    l4[0] = __builtin_bit_cast(f32x4, lds_read_b128_at<0>(lda4));
    d4[0] = __builtin_bit_cast(f32x4, lds_read_b128_at<256>(lda4));
    constexpr int RPT = 2 * T::KS + 2;  // LDS reads per 16-query tile
    f32x4 p[2][U], ds[2][U];
    static_for<4>([&](auto tc) {
      constexpr int t = decltype(tc)::value, tt = t & 1, s2 = t >> 1, cb = t & 1, nb = cb ^ 1;
      if constexpr (t < 3) {
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) {
          qfr[nb][ks] = T::template frag_row_at<16 * (t + 1)>(qra[ks]);
          ofr[nb][ks] = T::template frag_row_at<16 * (t + 1)>(ora[ks]);
        }
        l4[nb] = __builtin_bit_cast(f32x4, lds_read_b128_at<64 * (t + 1)>(lda4));
        d4[nb] = __builtin_bit_cast(f32x4, lds_read_b128_at<256 + 64 * (t + 1)>(lda4));
        lgkm_wait<RPT>();
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
        tie(qfr[cb][ks]);
        tie(ofr[cb][ks]);
      }
      tie(l4[cb]);
      tie(d4[cb]);
      f32x4 sv[U], dpv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) sv[u] = dpv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          sv[u] = mfma16(qfr[cb][ks], kf[u][ks], sv[u]);
          dpv[u] = mfma16(ofr[cb][ks], vf[u][ks], dpv[u]);
        }
      }
      // the whole 16-query subtile valid for every key of the wave (a
      // wave-uniform test): no per-element masking
      const int qs0 = q0 + 16 * t;
      const bool full = kmaxw < klim && qs0 + 15 < a.Lq && (!causal || kmaxw <= qs0);
      TDG_PDS_KEY_LANE(U, full, sv, dpv, l4[cb], d4[cb], c, key, qs0 + 4 * g, klim, a.Lq, causal, p[tt],
                       ds[tt])
      if constexpr (tt == 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pf[u][s2] = pack8(p[0][u], p[1][u]);
          dsf[u][s2] = pack8(ds[0][u], ds[1][u]);
        }
      }
    });
    // dV^T += dO^T P, dK^T += Q^T dS: transposed fragments, next requested
    // before this one is used
    uint32_t otra[T::DT], qtra[T::DT];
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) {
      otra[dt] = slotO + troff[dt];
      qtra[dt] = slotQ + troff[dt];
    }
    short4_t olo[2], ohi[2], qlo[2], qhi[2];
    T::template frag_tr_at<0>(otra[0], olo[0], ohi[0]);
    T::template frag_tr_at<0>(qtra[0], qlo[0], qhi[0]);
    static_for<2 * T::DT>([&](auto ic) {
      constexpr int i = decltype(ic)::value, s2 = i / T::DT, dt = i % T::DT, cb = i & 1, nb = cb ^ 1;
      if constexpr (i + 1 < 2 * T::DT) {
        T::template frag_tr_at<(i + 1) / T::DT>(otra[(i + 1) % T::DT], olo[nb], ohi[nb]);
        T::template frag_tr_at<(i + 1) / T::DT>(qtra[(i + 1) % T::DT], qlo[nb], qhi[nb]);
        lgkm_wait<4>();
      } else {
        lgkm_wait<0>();
      }
      tie(olo[cb]);
      tie(ohi[cb]);
      tie(qlo[cb]);
      tie(qhi[cb]);
      const short8_t ot = cat4(olo[cb], ohi[cb]);
      const short8_t qt = cat4(qlo[cb], qhi[cb]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        dv[u][dt] = mfma16(ot, pf[u][s2], dv[u][dt]);
        dk[u][dt] = mfma16(qt, dsf[u][s2], dk[u][dt]);
      }
    });
  }
  wait_vmcnt<0>();
  if (!a.skip_bf16) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = key[u] < a.Lk;
    bf16_t* dkp = a.dk + b * a.dk_sb + (long long)key[u] * a.dk_sl + h * a.dk_sh;
    bf16_t* dvp = a.dv + b * a.dv_sb + (long long)key[u] * a.dv_sl + h * a.dv_sh;
    uint32_t lo[T::DT], hi[T::DT];
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dkp, dk[u], a.scale, g, ok)
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dvp, dv[u], 1.f, g, ok)
  }
  }
  if (a.dk8) {  // e5m2 dK / dV (+ amax, + bias-gradient partials)
    const float s8 = a.sg8[0];
    float* red = reinterpret_cast<float*>(smem);
    float* prow = a.cs_part ? a.cs_part + ((long long)b * a.cs_np + xb) * a.cs_ld + h * 64 : nullptr;
    attn_emit_g8<U>(dk, a.scale, key, a.Lk, a.dk8 + b * a.dk_sb + h * a.dk_sh, a.dk_sl, s8, a.amaxg8,
                    prow ? prow + a.cs_k : nullptr, red, lane, w);
    attn_emit_g8<U>(dv, 1.f, key, a.Lk, a.dv8 + b * a.dv_sb + h * a.dv_sh, a.dv_sl, s8, a.amaxg8,
                    prow ? prow + a.cs_v : nullptr, red, lane, w);
  }
}

template <int U, int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_bwd_dq_pipe_kernel(AttnArgs a) {
  constexpr int HD = 64;
  using T = ATile<HD>;
  using G = Glds<true, 64, 4>;
  constexpr int QBW = 64 * U;
  constexpr int SLOT = 2 * T::BYTES;
  constexpr int PT = 2 * G::P;
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
  const int qminw = q0 + 16 * U * w;  // the wave's first query
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, q0 + QBW);
  const float c = scl * LOG2E;
  const int nkt = (klim + 63) / 64;
  const bf16_t* kb = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + h * a.v_sh;
  short8_t qf[U][T::KS], of[U][T::KS];
  float L[U], D[U];
  short8_t ov[U][T::KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool qvalid = qrow[u] < a.Lq;
    const int qr = min(qrow[u], a.Lq - 1);
    const bf16_t* qp = a.q + b * a.q_sb + (long long)qr * a.q_sl + h * a.q_sh;
    const bf16_t* dop = a.dout + b * a.do_sb + (long long)qr * a.do_sl + h * a.do_sh;
    TDG_LOAD_ROW_FRAGS2(HD, lane, qvalid, qf[u], qp, of[u], dop)
    const long long bh = ((long long)b * a.H + h) * a.Lq + qr;
    L[u] = a.lse[bh];
    const bf16_t* opr = a.o + b * a.o_sb + (long long)qr * a.o_sl + h * a.o_sh;
    TDG_LOAD_ROW_FRAGS(HD, lane, qvalid, ov[u], opr)
  }
  G gs;
  gs.init(w, lane);
  auto issue = [&](int kt) {
    char* slot = smem + (kt % NS) * SLOT;
    gs.issue(kb, (int)a.k_sl, a.Lk, HD, 64 * kt, 0, slot, w);
    gs.issue(vb, (int)a.v_sl, a.Lk, HD, 64 * kt, 0, slot + T::BYTES, w);
  };
  // prologue tiles issued unconditionally (clamped rows, never read) so the
  // DMA count behind the Q / dO / O / lse loads is a constant
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue(s);
  wait_vmcnt_known<(NS - 1) * PT>();
  // delta = rowsum(dO * O) of the lane's query row (the 4 lane groups hold
  // disjoint head-dim slices), written for the dK/dV kernel, which runs after
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float d = row_delta(of[u], ov[u]);
    if (qrow[u] < a.Lq && g == 0) a.delta[((long long)b * a.H + h) * a.Lq + qrow[u]] = d;
    D[u] = d;
  }
  f32x4 dq[U][T::DT];
  TDG_ZERO(U, T::DT, dq)
  uint32_t roff[T::KS], troff[T::DT];  // lane parts of the fragment addresses
#pragma unroll
  for (int ks = 0; ks < T::KS; ++ks) roff[ks] = T::row_off(ks, lane);
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) troff[dt] = T::tr_off(dt, lane);

  for (int kt = 0; kt < nkt; ++kt) {
    wait_tiles<PT, NS - 2>(min(NS - 2, nkt - 1 - kt));
    lds_barrier();
    if (kt + NS - 1 < nkt) issue(kt + NS - 1);
    const uint32_t slotK = (uint32_t)(uintptr_t)smem + (uint32_t)((kt % NS) * SLOT);
    const uint32_t slotV = slotK + T::BYTES;
    const int k0 = 64 * kt;
    // untracked LDS reads with counted waits, next 16-key tile requested
    // before this one is used; row bases in the DS offset field
    uint32_t kra[T::KS], vra[T::KS];
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      kra[ks] = slotK + roff[ks];
      vra[ks] = slotV + roff[ks];
    }
    short8_t dsf[U][2];
    short8_t kfr[2][T::KS], vfr[2][T::KS];
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      kfr[0][ks] = T::template frag_row_at<0>(kra[ks]);
      vfr[0][ks] = T::template frag_row_at<0>(vra[ks]);
    }
    constexpr int RPT = 2 * T::KS;
    f32x4 ds[2][U];
    static_for<4>([&](auto tc) {
      constexpr int t = decltype(tc)::value, tt = t & 1, s2 = t >> 1, cb = t & 1, nb = cb ^ 1;
      if constexpr (t < 3) {
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) {
          kfr[nb][ks] = T::template frag_row_at<16 * (t + 1)>(kra[ks]);
          vfr[nb][ks] = T::template frag_row_at<16 * (t + 1)>(vra[ks]);
        }
        lgkm_wait<RPT>();
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
        tie(kfr[cb][ks]);
        tie(vfr[cb][ks]);
      }
      f32x4 sv[U], dpv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) sv[u] = dpv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          sv[u] = mfma16(kfr[cb][ks], qf[u][ks], sv[u]);
          dpv[u] = mfma16(vfr[cb][ks], of[u][ks], dpv[u]);
        }
      }
      // the whole 16-key subtile valid for every query of the wave (a
      // wave-uniform test): no per-element masking
      const int ks0 = k0 + 16 * t;
      const bool full = qminw + 16 * U <= a.Lq && ks0 + 15 < klim && (!causal || ks0 + 15 <= qminw);
      TDG_DS_QUERY_LANE(U, full, sv, dpv, L, D, c, qrow, ks0 + 4 * g, klim, a.Lq, causal, ds[tt])
      if constexpr (tt == 1) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          dsf[u][s2] = pack8(ds[0][u], ds[1][u]);
      }
    });
    uint32_t ktra[T::DT];
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) ktra[dt] = slotK + troff[dt];
    short4_t klo[2], khi[2];
    T::template frag_tr_at<0>(ktra[0], klo[0], khi[0]);
    static_for<2 * T::DT>([&](auto ic) {
      constexpr int i = decltype(ic)::value, s2 = i / T::DT, dt = i % T::DT, cb = i & 1, nb = cb ^ 1;
      if constexpr (i + 1 < 2 * T::DT) {
        T::template frag_tr_at<(i + 1) / T::DT>(ktra[(i + 1) % T::DT], klo[nb], khi[nb]);
        lgkm_wait<2>();
      } else {
        lgkm_wait<0>();
      }
      tie(klo[cb]);
      tie(khi[cb]);
      const short8_t kt2 = cat4(klo[cb], khi[cb]);
#pragma unroll
      for (int u = 0; u < U; ++u) dq[u][dt] = mfma16(kt2, dsf[u][s2], dq[u][dt]);
    });
  }
  wait_vmcnt<0>();
  if (!a.skip_bf16) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    TDG_STORE_GRAD_ROW(T::DT, a.dq, a.dq_sb, a.dq_sl, a.dq_sh, b, h, qrow[u], a.Lq, dq[u], a.scale, g)
  }
  }
  if (a.dq8) {  // e5m2 dQ (+ amax, + bias-gradient partials)
    float* prow = a.cs_part ? a.cs_part + ((long long)b * a.cs_np + xb) * a.cs_ld + h * 64 + a.cs_q
                            : nullptr;
    attn_emit_g8<U>(dq, a.scale, qrow, a.Lq, a.dq8 + b * a.dq_sb + h * a.dq_sh, a.dq_sl, a.sg8[0],
                    a.amaxg8, prow, reinterpret_cast<float*>(smem), lane, w);
  }
}

// ============================================================================ fused backward, short sequences
// Lq, Lk <= 128: one workgroup (8 waves) per (batch, head) computes dQ, dK
// and dV together, with delta = rowsum(dO*O) computed in the prologue.
// Phase 1 (key rows on lanes, wave w owns keys 16w..16w+15): S^T and dP^T
// from the Q / dO tiles in LDS and the wave's K / V fragments in registers,
// P recomputed from the forward log-sum-exp, dS = P (dP - delta); dV^T and
// dK^T accumulate over all queries. dS is then written as bf16 into the LDS
// the Q / dO tiles used: a [key][query] image whose transposing read is
// exactly the B-operand layout of phase 2. Phase 2 (query rows on lanes,
// wave w owns queries 16w..16w+15): dQ^T = K^T dS^T.
// Versus the three-kernel path (delta, dK/dV, dQ): every tile is read from
// HBM once and there is one launch instead of three.
// U: 16-key (phase 1) / 16-query (phase 2) subtiles per wave, 8 / U waves.
// U = 2 reads every Q / dO / K fragment from LDS once for two MFMAs (the
// U = 1 loops issue one LDS read per MFMA).
// dS^T image of the fused backward: 128 key rows x 128 queries (bf16, 256-B
// rows). ATile<128>'s 32-byte segment swizzle (segment ^ row & 7) keeps the
// transposing dQ-phase reads conflict-free, but the key-row-per-lane 8-byte
// stores of a 16-lane group (one row each, the same column) then land on only
// 4 bank positions (a 256-B row is 0 mod 32 banks): 4-way conflicts. Rows with
// bit 3 set also swap the 16-byte halves of each segment: 2-way for the stores,
// the reads (8 consecutive rows per 32-lane half, bit 3 constant) unchanged.
struct DsImg {
  static constexpr int RB = 256;
  __device__ static __forceinline__ int off(int row, int byte) {
    const int seg = (byte >> 5) ^ (row & 7);
    return row * RB + (seg << 5) + ((byte & 31) ^ (((row >> 3) & 1) << 4));
  }
  // ATile<128>::frag_tr with this image's offsets
  __device__ static __forceinline__ short8_t frag_tr(const char* lds, int s2, int dt, int lane) {
    const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
    const int r1 = 32 * s2 + 4 * g + q;
    const int byte = (16 * dt + 4 * p) * 2;
    return cat4(lds_read_tr(lds + off(r1, byte)), lds_read_tr(lds + off(r1 + 16, byte)));
  }
};

// dO tile of the fused backward with the output-projection dgrad (FDO):
// dO_bh [128 x 64] = dY_b [128 rows, d] @ Wo[:, 64 h .. 64 h + 63], K = d,
// on 8 waves as 4 x 2 of 32 x 32 -- the main loop of gemm_impl.h's
// gemm_kernel (3 LDS-DMA stages of 64-deep K tiles, swapped-operand MFMAs,
// the same k order per element as the standalone NN dgrad, so the bf16 dO is
// bitwise that kernel's). Uses smem[0, 3 * 24 KiB); returns the accumulators.
constexpr int FDO_STAGES = 3, FDO_SB = (128 + 64) * BK * 2;
__device__ __forceinline__ void fdo_tile(const AttnArgs& a, int b, int h, char* smem, int wid,
                                         int lane, f32x4 (&acc)[2][2]) {
  constexpr int NW = 8, BM = 128, BN = 64, WN = 2, TM = 2, TN = 2, STAGES = FDO_STAGES;
  constexpr int A_BYTES = BM * BK * 2, SB = FDO_SB;
  using GA = Glds<true, BM, NW>;
  using GB = Glds<false, BN, NW>;
  constexpr int PT = GA::P + GB::P;
  const int wm = wid / WN, wn = wid % WN;
  const int K = a.fdo_d;
  const bf16_t* Y = reinterpret_cast<const bf16_t*>(a.fdo_dy) + (size_t)b * a.Lq * a.fdo_ldy;
  const bf16_t* W = reinterpret_cast<const bf16_t*>(a.fdo_w) + 64 * h;
  GA ga;
  GB gb;
  ga.init(wid, lane);
  gb.init(wid, lane);
  const int nk = K / BK;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < STAGES; ++st) {
    if (st < nk) {
      ga.issue(Y, a.fdo_ldy, a.Lq, K, 0, st * BK, smem + st * SB, wid);
      gb.issue(W, a.fdo_ldw, BN, K, 0, st * BK, smem + st * SB + A_BYTES, wid);
    }
  }
  const int abase = wm * (BM / 4), bbase = wn * (BN / WN);
  short8_t fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  if (nk >= STAGES)
    wait_vmcnt<(STAGES - 1) * PT>();
  else
    wait_vmcnt<0>();
  lds_barrier();
#pragma unroll
  for (int i = 0; i < TM; ++i) fa0[i] = frag<true, BM>(smem, abase + 16 * i, 0, lane);
#pragma unroll
  for (int j = 0; j < TN; ++j) fb0[j] = frag<false, BN>(smem + A_BYTES, bbase + 16 * j, 0, lane);
  constexpr int STEP_OPS = TM * frag_ops<true>() + TN * frag_ops<false>();
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    const char* st = smem + (kt % STAGES) * SB;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa1[i] = frag<true, BM>(st, abase + 16 * i, 1, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb1[j] = frag<false, BN>(st + A_BYTES, bbase + 16 * j, 1, lane);
    lgkm_wait<STEP_OPS>();
    tie_all(fa0);
    tie_all(fb0);
    prio_hi();
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(fb0[j], fa0[i], acc[i][j]);
    prio_lo();
    if constexpr (MODE >= 1) {
      if constexpr (MODE >= 2) wait_vmcnt<(STAGES - 2) * PT>();
      else wait_vmcnt<0>();
      lds_barrier();
      const char* nx = smem + ((kt + 1) % STAGES) * SB;
      if constexpr (MODE == 3) {
        char* ns = smem + (kt % STAGES) * SB;
        ga.issue(Y, a.fdo_ldy, a.Lq, K, 0, (kt + STAGES) * BK, ns, wid);
        gb.issue(W, a.fdo_ldw, BN, K, 0, (kt + STAGES) * BK, ns + A_BYTES, wid);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) fa0[i] = frag<true, BM>(nx, abase + 16 * i, 0, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb0[j] = frag<false, BN>(nx + A_BYTES, bbase + 16 * j, 0, lane);
    } else {
      lgkm_wait<0>();
    }
    tie_all(fa1);
    tie_all(fb1);
    prio_hi();
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(fb1[j], fa1[i], acc[i][j]);
    prio_lo();
  };
  int kt = 0;
  for (; kt + STAGES < nk; ++kt) kstep(kt, std::integral_constant<int, 3>{});
  if (kt + STAGES - 1 < nk && kt + 1 < nk) kstep(kt++, std::integral_constant<int, 2>{});
  for (; kt + 1 < nk; ++kt) kstep(kt, std::integral_constant<int, 1>{});
  if (kt < nk) kstep(kt, std::integral_constant<int, 0>{});
  lds_barrier();  // the stages are free for the attention's images
}

template <int HD, int U, bool FDO = false>
__global__ __launch_bounds__(512 / U) __attribute__((amdgpu_waves_per_eu(U == 1 ? (HD <= 64 ? 4 : 2) : 2))) void attn_bwd_fused_kernel(AttnArgs a) {
  static_assert(!FDO || (HD == 64 && U == 1), "in-kernel dO: hd 64, 8 waves");
  using T = ATile<HD>;
  using TS = DsImg;  // dS image: 128 key rows x 128 queries (bf16)
  constexpr int R = 128;
  constexpr int NT = 512 / U;  // threads
  constexpr int TB = R * T::RB;  // bytes of one 128-row tile image
  constexpr int SB = R * TS::RB;  // dS image bytes (32 KiB)
  constexpr int ALIAS = 2 * TB >= SB;  // dS fits over Q + dO
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsQ = smem;
  char* ldsO = smem + TB;
  char* ldsK = smem + 2 * TB;
  char* ldsS = ALIAS ? smem : smem + 3 * TB;
  float* ldsL = reinterpret_cast<float*>(smem + (ALIAS ? 3 * TB : 3 * TB + SB));
  float* ldsD = ldsL + R;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: scalar branches)
  const int bh = a.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int b = bh / a.H, h = bh % a.H;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  const float c = scl * LOG2E;

  // ---- prologue. Every global load is issued before any is used (one
  // memory latency): this wave's K / V register fragments for phase 1, the
  // Q / dO / K tile chunks, O chunks for delta, and lse.
  TDG_STAMP(0);
  const bf16_t* qb = a.q + b * a.q_sb + h * a.q_sh;
  const bf16_t* ob = a.dout + b * a.do_sb + h * a.do_sh;
  const bf16_t* kbp = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* obo = a.o + b * a.o_sb + h * a.o_sh;
  int key[U];
#pragma unroll
  for (int u = 0; u < U; ++u) key[u] = 16 * (U * w + u) + cl;
  short8_t kf[U][T::KS], vf[U][T::KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int krow = min(key[u], a.Lk - 1);
    const bf16_t* kp = kbp + (long long)krow * a.k_sl;
    const bf16_t* vp = a.v + b * a.v_sb + (long long)krow * a.v_sl + h * a.v_sh;
    TDG_LOAD_ROW_FRAGS2(HD, lane, key[u] < a.Lk, kf[u], kp, vf[u], vp)
  }
  {
    constexpr int CPR = HD / 8;  // 16-byte chunks per row
    constexpr int TOTAL = R * CPR;
    constexpr int NI = (TOTAL + NT - 1) / NT;
    short8_t vq[NI], vo[NI], vk[NI], vx[NI];
    const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int id = tid + i * NT;
      const int row = id / CPR, cc = id % CPR;
      vq[i] = vo[i] = vk[i] = vx[i] = z;
      if constexpr (TOTAL % NT == 0) {  // (clamped rows, zeroed: no branch per load)
        const int rq = min(row, a.Lq - 1), rk = min(row, a.Lk - 1);
        vq[i] = ld8_or0(qb + (long long)rq * a.q_sl + cc * 8, row < a.Lq);
        if constexpr (!FDO) vo[i] = ld8_or0(ob + (long long)rq * a.do_sl + cc * 8, row < a.Lq);
        vx[i] = ld8_or0(obo + (long long)rq * a.o_sl + cc * 8, row < a.Lq);
        vk[i] = ld8_or0(kbp + (long long)rk * a.k_sl + cc * 8, row < a.Lk);
      } else {
        if (id < TOTAL && row < a.Lq) {
          vq[i] = *reinterpret_cast<const short8_t*>(qb + (long long)row * a.q_sl + cc * 8);
          if constexpr (!FDO) vo[i] = *reinterpret_cast<const short8_t*>(ob + (long long)row * a.do_sl + cc * 8);
          vx[i] = *reinterpret_cast<const short8_t*>(obo + (long long)row * a.o_sl + cc * 8);
        }
        if (id < TOTAL && row < a.Lk)
          vk[i] = *reinterpret_cast<const short8_t*>(kbp + (long long)row * a.k_sl + cc * 8);
      }
    }
    const float lse_v = (tid < R && tid < a.Lq) ? a.lse[((long long)b * a.H + h) * a.Lq + tid] : INFINITY;
    if constexpr (FDO) {
      // dO from the in-kernel output-projection dgrad (rows >= Lq zero, as
      // the loads above give them), into its image; then read back in the
      // chunk layout for delta
      f32x4 acc[2][2];
      fdo_tile(a, b, h, smem, w, lane, acc);
      const int wm = w / 2, wn = w % 2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int m = 32 * wm + 16 * i + cl, n = 32 * wn + 16 * j + 4 * g;
          short4_t o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = m < a.Lq ? (short)f2bf(acc[i][j][r]) : (short)0;
          *reinterpret_cast<short4_t*>(ldsO + T::off(m, n * 2)) = o;
        }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int id = tid + i * NT;
        const int row = id / CPR, cc = id % CPR;
        if (id < TOTAL) vo[i] = *reinterpret_cast<const short8_t*>(ldsO + T::off(row, cc * 16));
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int id = tid + i * NT;
      const int row = id / CPR, cc = id % CPR;
      if (id < TOTAL) {
        *reinterpret_cast<short8_t*>(ldsQ + T::off(row, cc * 16)) = vq[i];
        if constexpr (!FDO) *reinterpret_cast<short8_t*>(ldsO + T::off(row, cc * 16)) = vo[i];
        *reinterpret_cast<short8_t*>(ldsK + T::off(row, cc * 16)) = vk[i];
      }
      // delta[row] = sum_d dO * O: partial over this chunk, then over the
      // CPR consecutive lanes holding the row (xor shuffles)
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d += bf2f((bf16_t)vo[i][e]) * bf2f((bf16_t)vx[i][e]);
#pragma unroll
      for (int o = 1; o < CPR; o <<= 1) d += __shfl_xor(d, o, 64);
      if (id < TOTAL && cc == 0) ldsD[row] = row < a.Lq ? d : 0.f;
    }
    if (tid < R) ldsL[tid] = lse_v;
  }
  __syncthreads();
  TDG_STAMP(1);

  // ---- phase 1: this wave's U x 16 keys against all queries
  f32x4 dk[U][T::DT], dv[U][T::DT];
  TDG_ZERO2(U, T::DT, dk, dv)
  // P and dS of [q = 16t + 4g + r][key], packed to bf16 pairs as produced
  uint32_t pk[U][8][2], dk2[U][8][2];
  const bool active = 16 * U * w < klim;  // wave-uniform
  if (active) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const bool live = 16 * t < a.Lq && (!causal || 16 * t + 15 >= 16 * U * w);  // uniform
      if (!live) {  // (no query of the tile attends to the wave's keys: P = dS = 0)
#pragma unroll
        for (int u = 0; u < U; ++u) pk[u][t][0] = pk[u][t][1] = dk2[u][t][0] = dk2[u][t][1] = 0u;
        continue;
      }
      f32x4 sv[U], dpv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) sv[u] = dpv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
        const short8_t qfr = T::frag_row(ldsQ, 16 * t, ks, lane);
        const short8_t ofr = T::frag_row(ldsO, 16 * t, ks, lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          sv[u] = mfma16(qfr, kf[u][ks], sv[u]);
          dpv[u] = mfma16(ofr, vf[u][ks], dpv[u]);
        }
      }
      // lse / delta of queries 16t + 4g .. +3: one 16-byte LDS read each
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(ldsL + 16 * t + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(ldsD + 16 * t + 4 * g);
      // every (query, key) of this 16-query tile valid for the wave's keys
      // (wave-uniform): no per-element masks
      const int kmaxw = 16 * U * (w + 1) - 1;
      const bool full = kmaxw < klim && 16 * t + 15 < a.Lq && (!causal || kmaxw <= 16 * t);
      // (TDG_PDS_KEY_LANE written out per subtile: as the macro, with the branch
      // outside the subtile loop, this kernel's control flow changes)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float pv[4], dv4[4];
        if (full) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[r] = fast_exp2(sv[u][r] * c - l4[r]);
            dv4[r] = pv[r] * (dpv[u][r] - d4[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 16 * t + 4 * g + r;
            const bool ok = TDG_ATTENDS(key[u], q, klim, a.Lq, causal);
            pv[r] = masked_exp2(sv[u][r] * c - l4[r], ok);
            dv4[r] = pv[r] * (dpv[u][r] - d4[r]);
          }
        }
        pk[u][t][0] = pack2bf(pv[0], pv[1]);
        pk[u][t][1] = pack2bf(pv[2], pv[3]);
        dk2[u][t][0] = pack2bf(dv4[0], dv4[1]);
        dk2[u][t][1] = pack2bf(dv4[2], dv4[3]);
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      if (32 * s2 >= a.Lq) break;
      short8_t pf[U], dsf[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pf[u] = __builtin_bit_cast(short8_t, make_uint4(pk[u][2 * s2][0], pk[u][2 * s2][1],
                                                        pk[u][2 * s2 + 1][0], pk[u][2 * s2 + 1][1]));
        dsf[u] = __builtin_bit_cast(short8_t, make_uint4(dk2[u][2 * s2][0], dk2[u][2 * s2][1],
                                                         dk2[u][2 * s2 + 1][0], dk2[u][2 * s2 + 1][1]));
      }
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        const short8_t otr = T::frag_tr(ldsO, s2, dt, lane);
        const short8_t qtr = T::frag_tr(ldsQ, s2, dt, lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          dv[u][dt] = mfma16(otr, pf[u], dv[u][dt]);
          dk[u][dt] = mfma16(qtr, dsf[u], dk[u][dt]);
        }
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < 8; ++t) dk2[u][t][0] = dk2[u][t][1] = 0u;
  }
  TDG_STAMP(2);
  __syncthreads();  // everyone done with Q / dO (the dS image aliases them)
  // dS^T image: row = key, bytes (16t + 4g) * 2 .. +8 = queries 16t+4g .. +3
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < 8; ++t)
      *reinterpret_cast<uint2*>(ldsS + TS::off(key[u], (16 * t + 4 * g) * 2)) = make_uint2(dk2[u][t][0], dk2[u][t][1]);
  // dK, dV out (key rows on lanes)
  const float sc = a.scale;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = key[u] < a.Lk;
    bf16_t* dkp = a.dk + b * a.dk_sb + (long long)key[u] * a.dk_sl + h * a.dk_sh;
    bf16_t* dvp = a.dv + b * a.dv_sb + (long long)key[u] * a.dv_sl + h * a.dv_sh;
    uint32_t lo[T::DT], hi[T::DT];
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dkp, dk[u], sc, g, ok)
    TDG_PACK_STORE_ROW(T::DT, lo, hi, dvp, dv[u], 1.f, g, ok)
  }
  __syncthreads();

  // ---- phase 2: dQ for queries 16 (U w + u) .. +15 (query on lanes)
  if (16 * U * w >= a.Lq) return;
  f32x4 dq[U][T::DT];
  TDG_ZERO(U, T::DT, dq)
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    if (32 * s2 >= klim) break;
    short8_t dsf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) dsf[u] = TS::frag_tr(ldsS, s2, U * w + u, lane);
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) {
      const short8_t ktr = T::frag_tr(ldsK, s2, dt, lane);
#pragma unroll
      for (int u = 0; u < U; ++u) dq[u][dt] = mfma16(ktr, dsf[u], dq[u][dt]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int qrow = 16 * (U * w + u) + cl;
    TDG_STORE_GRAD_ROW(T::DT, a.dq, a.dq_sb, a.dq_sl, a.dq_sh, b, h, qrow, a.Lq, dq[u], sc, g)
  }
#ifdef TDG_STAMPS
  TDG_STAMP(3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TDG_STAMP(4);
#endif
}

#undef TDG_ATTENDS
#undef TDG_PDS_KEY_LANE
#undef TDG_DS_QUERY_LANE

}  // namespace tdg

using namespace tdg;

namespace {
template <int HD>
constexpr int fused_bwd_lds() {
  constexpr int TB = 128 * HD * 2, SB = 128 * 256;
  return (2 * TB >= SB ? 3 * TB : 3 * TB + SB) + 2 * 128 * 4;
}
}  // namespace

// Fused backward with the output-projection dgrad in-kernel (FDO): Lq, Lk <=
// 128, hd 64, d = 64 H. Returns -1 when not covered.
extern "C" int tdg_attn_bwd_fdo(const AttnArgs* ap, hipStream_t st) {
  const AttnArgs& a = *ap;
  if (a.Lq > 128 || a.Lk > 128 || a.fdo_d != 64 * a.H || a.fdo_d % BK || a.fdo_ldy % 8 ||
      a.fdo_ldw % 8 || !a.fdo_dy || !a.fdo_w)
    return -1;
  constexpr int lds = fused_bwd_lds<64>() > FDO_STAGES * FDO_SB ? fused_bwd_lds<64>() : FDO_STAGES * FDO_SB;
  big_lds<attn_bwd_fused_kernel<64, 1, true>>();
  attn_plan_record(ATTN_BWD_FDO, 64, (long long)a.B * a.H, 512);
  hipLaunchKernelGGL((attn_bwd_fused_kernel<64, 1, true>), dim3(a.B * a.H), dim3(512), lds, st, a);
  return 0;
}

namespace {
template <int HD>
int bwd_hd(const AttnArgs& a, hipStream_t st) {
  if (a.Lq <= 128 && a.Lk <= 128) {
    constexpr int lds = fused_bwd_lds<HD>();
    // U = 1: 8 waves, 16 keys / queries each. U = 2 (4 waves, every fragment
    // read feeding two MFMAs, 231 VGPRs) measured slower: 22.7 vs 21.7 us per
    // call, step 5.15 vs 5.13 ms (profiles/r3s2/attn_bwd_u2.txt)
    constexpr int U = 1;
    big_lds<attn_bwd_fused_kernel<HD, U>>();
    attn_plan_record(ATTN_BWD_FUSED, HD, (long long)a.B * a.H, 512 / U);
    hipLaunchKernelGGL((attn_bwd_fused_kernel<HD, U>), dim3(a.B * a.H), dim3(512 / U), lds, st, a);
    return 0;
  }
  // dQ first: it also writes delta = rowsum(dO * O), which dK/dV reads
  // hd 64: LDS-DMA pipelined kernels, 32 queries / keys per wave (seq 512:
  // 121 us vs 132-136 with 16 per wave in either, 147 register-staged)
  if constexpr (HD == 64) {
    constexpr int U = 2, NS = 4;
    constexpr int lds_dq = NS * 2 * ATile<64>::BYTES;
    constexpr int lds_kv = NS * (2 * ATile<64>::BYTES + 768);
    big_lds<attn_bwd_dq_pipe_kernel<U, NS>>();
    big_lds<attn_bwd_dkdv_pipe_kernel<U, NS>>();
    attn_plan_record(ATTN_BWD_PIPE, HD, (long long)cdiv(a.Lq, 64 * U) * a.H * a.B, 256,
                     (long long)cdiv(a.Lk, 64 * U) * a.H * a.B);
    hipLaunchKernelGGL((attn_bwd_dq_pipe_kernel<U, NS>), dim3(cdiv(a.Lq, 64 * U), a.H, a.B),
                       dim3(256), lds_dq, st, a);
    hipLaunchKernelGGL((attn_bwd_dkdv_pipe_kernel<U, NS>), dim3(cdiv(a.Lk, 64 * U), a.H, a.B),
                       dim3(256), lds_kv, st, a);
    return 0;
  }
  attn_plan_record(ATTN_BWD_SPLIT, HD, (long long)cdiv(a.Lq, QB) * a.H * a.B, 256,
                   (long long)cdiv(a.Lk, KB) * a.H * a.B);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, 1>), dim3(cdiv(a.Lq, QB), a.H, a.B), dim3(256),
                     2 * ATile<HD>::BYTES, st, a);
  hipLaunchKernelGGL((attn_bwd_dkdv_kernel<HD, 1>), dim3(cdiv(a.Lk, KB), a.H, a.B), dim3(256),
                     2 * ATile<HD>::BYTES + 2 * QB * 4, st, a);
  return 0;
}
}  // namespace

extern "C" int tdg_attn_bwd(const AttnArgs* a, int hd, hipStream_t st) {
  TDG_HD_CASES(bwd_hd, *a, st)
}
