// fp8 attention: the e4m3 forward, the e4m3 / e5m2 backward and their
// launchers (design: attn_impl.h). Definitions: one translation unit only.
#pragma once
#include "attn_impl.h"

namespace tdg {

// ============================================================================ forward, e4m3
// BASELINE config 5's fp8 attention: Q, K, V are the e4m3 copies the fp8
// input projections emit (per-tensor scales sq, sk, sv), S^T = K Q^T and
// O^T = V^T P^T on v_mfma_f32_16x16x32_fp8_fp8, P quantised as e4m3(P * 448)
// (P <= 1 against the running max), softmax in f32. hd = 64, > 128 queries;
// the structure of attn_fwd_pipe_kernel: 8 waves x 16 queries, K / V tiles of
// 64 keys (64-byte rows, 4 KiB each) in an NS-slot LDS-DMA ring, waves 0-3
// staging K and 4-7 V (one 1 KiB piece per wave per tile), untracked counted
// LDS reads. Images: 8-byte chunk c of row r stored at c ^ 2 ((r >> 2) & 3)
// (the K row reads and the V transposing reads both conflict-free). The PV
// product needs each lane group's 8 keys consecutive (ds_read_b64_tr_b8 gives
// 8 consecutive V rows): the K image is filled in a permuted key order so
// that the S accumulator (t, g, r) is key 32 (t >> 1) + 8 g + 4 (t & 1) + r,
// which makes the P registers the PV B operand as they stand. The backward
// stays bf16 (it recomputes P from the bf16 Q, K and this LSE).
template <int NS, int U>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(U == 2 ? 4 : 2))) void attn_fwd_fp8_kernel(AttnArgs a) {
  // U 16-query subtiles per wave (16 U queries): every K / V fragment feeds U
  // MFMAs and each wave carries U independent softmax chains (U = 2: one
  // round of 4 waves per SIMD at seq 512 instead of 1.33 rounds of 6)
  constexpr int NWV = 8, HD = 64, RB = 64, TB = 64 * RB, SLOT = 2 * TB, QBW = 16 * U * NWV;
  constexpr int NT16 = 4, DT = 4;
  static_assert(NS >= 3, "ring: refilled, being read, landed");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint8_t* q8 = reinterpret_cast<const uint8_t*>(a.q);
  const uint8_t* k8 = reinterpret_cast<const uint8_t*>(a.k);
  const uint8_t* v8 = reinterpret_cast<const uint8_t*>(a.v);
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, h, b;
  attn_coords(a, xb, h, b);
  const int q0 = xb * QBW;
  const int wq0 = q0 + 16 * U * w;
  int qrow[U];
#pragma unroll
  for (int u = 0; u < U; ++u) qrow[u] = wq0 + 16 * u + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, q0 + QBW);
  const int nkt = (klim + 63) / 64;
  // (causal: the wave's last key tile; later tiles are staged for the other
  // waves but skipped here)
  const int wkt = causal ? min(nkt, (wq0 + 16 * U + 63) / 64) : nkt;

  // Q fragments (B operand of S^T): lane (g, q) holds Q[q][32 ks + 8 g .. +7]
  long qf[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint8_t* qp = q8 + b * a.q_sb + (long long)min(qrow[u], a.Lq - 1) * a.q_sl + h * a.q_sh;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[u][ks] = qrow[u] < a.Lq ? *reinterpret_cast<const long*>(qp + 32 * ks + 8 * g) : 0;
  }
  // staging: wave w < 4 fills K image rows 16w.., w >= 4 V image rows 16(w-4)..
  const bool isv = w >= 4;
  const int rho = 16 * (w & 3) + (lane >> 2);
  // K image row rho = 16 t + 4 g + r holds key 32 t1 + 8 g + 4 t0 + r
  const int kin = isv ? rho : ((rho & 0x23) | ((rho & 0x0C) << 1) | ((rho & 0x10) >> 2));
  const int chunk = (lane & 3) ^ ((rho >> 2) & 3);  // 16-byte source chunk of the swizzled row
  const uint8_t* src0 = (isv ? v8 + b * a.v_sb + h * a.v_sh : k8 + b * a.k_sb + h * a.k_sh) + 16 * chunk;
  const long long sl = isv ? a.v_sl : a.k_sl;
  char* dst0 = smem + (isv ? TB : 0) + (w & 3) * 1024;
  // DMA source: a 32-bit byte offset stepped by 64 rows per tile (no 64-bit
  // multiply per issue); only the tiles that reach past Lk clamp their row
  const uint8_t* srcb = src0 + (long long)kin * sl;
  const uint32_t step = (uint32_t)(64 * sl);
  const int klast = a.Lk - 1 - kin;  // (64 kt > klast: this lane's row is clamped)
  auto issue = [&](int kt, auto slc) {
    constexpr int SL = decltype(slc)::value;
    const uint8_t* sp = 64 * kt <= klast ? srcb + (uint32_t)kt * step : src0 + (long long)(a.Lk - 1) * sl;
    __builtin_amdgcn_global_load_lds((const void*)sp,
                                     (__attribute__((address_space(3))) void*)(dst0 + SL * SLOT), 16, 0, 0);
  };
  // prologue tiles issued unconditionally (clamped rows, never read) so the
  // DMA count behind the Q loads is a constant
  static_for<NS - 1>([&](auto sc) { issue(decltype(sc)::value, sc); });
  wait_vmcnt_known<NS - 1>();

  // lane parts of the fragment addresses (the swizzle term (row >> 2) & 3 is
  // the same for every 16-row K tile t and both 32-row V halves s2); the ring
  // slot and the tile rows are immediate offsets (the tile loop is unrolled
  // by NS, so tile kt's slot kt % NS is a constant)
  const uint32_t sbase = (uint32_t)(uintptr_t)smem;
  uint32_t ka[2], va[DT];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) ka[ks] = sbase + cl * RB + 8 * ((4 * ks + g) ^ (((cl >> 2) & 3) << 1));
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int row = 8 * g + (cl >> 1);
    va[dt] = sbase + TB + row * RB + 8 * ((2 * dt + (cl & 1)) ^ (((row >> 2) & 3) << 1));
  }
  const float inv_qk = 1.f / (a.sq8[0] * a.sk8[0]);
  const float c = scl * LOG2E * inv_qk;
  f32x4 oacc[U][DT];
  float m[U], l[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
#pragma unroll
    for (int i = 0; i < DT; ++i) oacc[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto tile = [&](int kt, auto slc) {
    constexpr int SL = decltype(slc)::value;
    wait_tiles<1, NS - 2>(min(NS - 2, nkt - 1 - kt));
    lds_barrier();
    if (kt + NS - 1 < nkt) issue(kt + NS - 1, std::integral_constant<int, (SL + NS - 1) % NS>{});
    if (kt >= wkt) return;  // (wave-uniform)
    const int k0 = 64 * kt;
    // S^T: K rows 16 t + cl, hd bytes 32 ks + 8 g (8-byte chunk 4 ks + g);
    // lane part of the address ka[ks], slot and 16 t rows immediate offsets
    long kfr[NT16][2];
    static_for<NT16>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      kfr[t][0] = lds_read_b64_at<SL * SLOT + 16 * t * RB>(ka[0]);
      kfr[t][1] = lds_read_b64_at<SL * SLOT + 16 * t * RB>(ka[1]);
    });
    f32x4 s[U][NT16];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half == 0) lgkm_wait<NT16>();
      else lgkm_wait<0>();
#pragma unroll
      for (int t = half * 2; t < half * 2 + 2; ++t) {
        tie(kfr[t][0]);
        tie(kfr[t][1]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            s[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kfr[t][ks], qf[u][ks], s[u][t], 0, 0, 0);
        }
      }
    }
    const bool msk = tile_masked(k0, 64, klim, causal, wq0);
#pragma unroll
    for (int u = 0; u < U; ++u)
      softmax_max<NT16, DT, true>(s[u], m[u], l[u], oacc[u], msk, k0, klim, causal, qrow[u], g, c);
    // V^T fragments: lane pair (2 r8 + hh) of group g passes V row 32 s2 + 8 g + r8,
    // 8-byte chunk 2 dt + hh; lane i receives hd column 16 dt + i, keys 8 g .. +7
    long vfr[2][DT];
    static_for<DT>([&](auto dc) {
      constexpr int dt = decltype(dc)::value;
      vfr[0][dt] = lds_read_tr8_at<SL * SLOT>(va[dt]);
      vfr[1][dt] = lds_read_tr8_at<SL * SLOT + 32 * RB>(va[dt]);
    });
    // P448 = 448 exp2(c S - m) = exp2(c S - m + log2 448) (f32 row sum l of
    // P448), then e4m3(P448) in PV operand order: P <= 1 against the running
    // max, so P448 <= 448 needs no clamp and the 448 costs no multiply
    const float cs = msk ? 1.f : c;
    long pf[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float nm = (m[u] == -INFINITY ? 0.f : -m[u]) + LOG2_448;
#pragma unroll
      for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[u][t][r] = fast_exp2(fmaf(s[u][t][r], cs, nm));
      float rs = s[u][0][0];
#pragma unroll
      for (int i = 1; i < 4 * NT16; ++i) rs += s[u][i / 4][i % 4];
      l[u] += rs;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        // (the first convert of each word writes its low half: its old value
        // is any register, the high half is written next -- no zeroing move)
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(s[u][2 * s2][0], s[u][2 * s2][1],
                                                 __builtin_bit_cast(int, s[u][2 * s2][0]), false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(s[u][2 * s2][2], s[u][2 * s2][3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(s[u][2 * s2 + 1][0], s[u][2 * s2 + 1][1],
                                                 __builtin_bit_cast(int, s[u][2 * s2 + 1][0]), false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(s[u][2 * s2 + 1][2], s[u][2 * s2 + 1][3], hi, true);
        pf[u][s2] = (long)(uint32_t)lo | ((long)hi << 32);
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (s2 == 0) lgkm_wait<DT>();
      else lgkm_wait<0>();
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        tie(vfr[s2][dt]);
#pragma unroll
        for (int u = 0; u < U; ++u)
          oacc[u][dt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(vfr[s2][dt], pf[u][s2], oacc[u][dt], 0, 0, 0);
      }
    }
  };
  int kt = 0;
  for (; kt + NS <= nkt; kt += NS) static_for<NS>([&](auto sc) { tile(kt + decltype(sc)::value, sc); });
  static_for<NS - 1>([&](auto sc) {
    if (kt + decltype(sc)::value < nkt) tile(kt + decltype(sc)::value, sc);
  });
  wait_vmcnt<0>();
  // e4m3 copy of O for the e4m3 output projection: from the bf16-rounded
  // values (what quantising the bf16 O gives), wave amax -> one atomic
  const float so = a.out8 ? a.so8[0] : 0.f;
  float am = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float lu = l[u];
    lu = rows_sum(lu);
    const bool valid = qrow[u] < a.Lq;
    // (softmax_inv / softmax_lse's conventions with LOG2_448 folded in: lu is the row sum of P448)
    const float inv = lu > 0.f ? 1.f / (lu * a.sv8[0]) : 0.f;
    const long long ooff = b * a.o_sb + (long long)qrow[u] * a.o_sl + h * a.o_sh;
    bf16_t* op = a.out + ooff;
    // (8-byte stores: the 16-byte form of store_row16 measured 4 % slower here,
    // 739 vs 708 us per step over 18 calls, profiles/r4/ab_grouped_tiles_fp8_kstats.txt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      bf16_t e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = f2bf(oacc[u][dt][r] * inv);
      if (valid) {
        const uint32_t lo = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
        const uint32_t hi = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
        *reinterpret_cast<uint2*>(op + 16 * dt + 4 * g) = make_uint2(lo, hi);
      }
      if (a.out8) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = bf2f(e[r]);
          am = fmaxf(am, valid ? fabsf(v[r]) : 0.f);
        }
        int w8 = pack2_e4m3<false>(v[0] * so, v[1] * so, 0);
        w8 = pack2_e4m3<true>(v[2] * so, v[3] * so, w8);
        if (valid) *reinterpret_cast<int*>(a.out8 + ooff + 16 * dt + 4 * g) = w8;
      }
    }
    if (valid && g == 0)
      a.lse[((long long)b * a.H + h) * a.Lq + qrow[u]] = lu > 0.f ? m[u] + (log2f(lu) - LOG2_448) : INFINITY;
  }
  if (a.out8) {
    am = wave_max(am);
    if (lane == 0) atomic_amax(amax_word(a.amax8, blockIdx.x + 7 * blockIdx.y + 13 * blockIdx.z), am);
  }
}

// ============================================================================ backward, e4m3 / e5m2
// BASELINE config 5's fp8 attention backward (reference: the autograd of
// transformer_model.py:73-109). Operands: the e4m3 Q / K / V the forward ran
// on (scales sq, sk, sv), the e5m2 dO (sdo8), P as e4m3(448 P) and dS as
// e5m2(dS * sds8) -- five products on v_mfma_f32_16x16x32_{fp8,bf8}_{fp8,bf8}:
//   S^T = K Q^T, dP^T = V dO^T, dV^T += dO^T P, dK^T += Q^T dS, dQ = dS K,
// softmax recomputed in f32 from the forward's log2-domain LSE.
// One workgroup per (batch, head) holds ALL of its <= 512 keys -- the e4m3
// K image is 32 KiB and a wave's K / V fragments 32 registers, half the bf16
// footprint -- so P and dS are computed once (the bf16 path recomputes them
// in a dQ kernel and a dK/dV kernel) and dQ needs no sum across workgroups.
// NW waves; wave w owns the 16-key subtiles s = w + NW u (u < U = 32 / NW:
// interleaved, so causal work stays balanced) with their dK^T / dV^T in
// accumulators. Per step of 32 queries (Q / dO tiles register-prefetched into
// a 2-slot LDS ring):
//  * S^T, dP^T with the key on the lane: lane cl of query half j reads the
//    Q / dO image row 8 (cl >> 2) + 4 j + (cl & 3), so accumulator register r
//    of lane group g is query 8 g + 4 j + r and the two halves' P / dS pack
//    into the e4m3 / e5m2 B operand of dV^T / dK^T as they stand (queries
//    8 g .. 8 g + 7 of the lane); dO^T / Q^T A operands by ds_read_b64_tr_b8;
//  * dS^T goes to a [key][32 queries] e5m2 image (double-buffered), and the
//    next step computes this step's dQ = dS K from it and the K image (both
//    operands transposing reads): one barrier per step.
// delta = rowsum(dO O) from the e5m2 dO actually used and the bf16 O
// (consistent with dP) in the prologue, with lse, for all queries in LDS.
// Swizzles (8-byte chunk c of row r): K image c ^ 2 ((r >> 2) & 3); Q / dO
// images c ^ 2 (((r >> 2) ^ (r >> 4)) & 3) (conflict-free for both the
// permuted row reads and the transposing reads); dS image c ^ 2 ((r >> 3) & 1).
__device__ __forceinline__ int f8k_off(int r, int c) { return r * 64 + 8 * (c ^ (2 * ((r >> 2) & 3))); }
__device__ __forceinline__ int f8q_off(int r, int c) {
  return r * 64 + 8 * (c ^ (2 * (((r >> 2) ^ (r >> 4)) & 3)));
}
__device__ __forceinline__ int f8s_off(int r, int c) { return r * 32 + 8 * (c ^ (2 * ((r >> 3) & 1))); }

template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_bwd_f8_kernel(AttnArgs a) {
  constexpr int LMAX = 512, QT = 32, U = 32 / NW, NT = NW * 64;
  constexpr int KIMG = LMAX * 64, QIMG = QT * 64, SIMG = LMAX * QT;
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsK = smem;
  char* ldsV = smem + KIMG;          // (the same layout; its row fragments only)
  char* ldsQ = ldsV + KIMG;          // slot i: Q at 2 i QIMG, dO at (2 i + 1) QIMG
  char* ldsS = ldsQ + 4 * QIMG;      // dS^T images, 2 x SIMG
  float* ldsL = reinterpret_cast<float*>(ldsS + 2 * SIMG);  // lse - log2(448)
  float* ldsD = ldsL + LMAX;                                 // delta * sds / 448
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, h, b;
  attn_coords(a, xb, h, b);
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  const uint8_t* qb = reinterpret_cast<const uint8_t*>(a.q) + b * a.q_sb + h * a.q_sh;
  const uint8_t* kb = reinterpret_cast<const uint8_t*>(a.k) + b * a.k_sb + h * a.k_sh;
  const uint8_t* vb = reinterpret_cast<const uint8_t*>(a.v) + b * a.v_sb + h * a.v_sh;
  const uint8_t* db = reinterpret_cast<const uint8_t*>(a.dout) + b * a.do_sb + h * a.do_sh;
  const bf16_t* ob = a.o + b * a.o_sb + h * a.o_sh;
  const float sq = a.sq8[0], sk = a.sk8[0], sv = a.sv8[0], sdo = a.sdo8[0], sds = a.sds8[0];
  const float c8 = scl * LOG2E / (sq * sk);     // log2-domain logit per raw S product
  const float k1 = sds / 448.f;                 // e5m2 dS = P448 (dP - delta) * k1
  const float cdp = k1 / (sdo * sv);            // raw dP product -> dP * k1
  const int nq = (a.Lq + QT - 1) / QT;

  // ---- prologue: K image, Q / dO tile 0, lse / delta of every query, V fragments
#pragma unroll
  for (int i = 0; i < 2 * KIMG / 16 / NT; ++i) {  // K, then V
    const int id = tid + i * NT, r = (id >> 2) & (LMAX - 1), p = id & 3;
    const bool isv = id >= KIMG / 16;
    const uint8_t* src = (isv ? vb + (long long)min(r, a.Lk - 1) * a.v_sl
                              : kb + (long long)min(r, a.Lk - 1) * a.k_sl) + 16 * p;
    uint4 v = *reinterpret_cast<const uint4*>(src);
    if (r >= a.Lk) v = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>((isv ? ldsV : ldsK) + r * 64 + 16 * (p ^ ((r >> 2) & 3))) = v;
  }
  // Q / dO tile t, piece tid (< 256): tensor tid >> 7, row (tid >> 2) & 31, 16-byte piece tid & 3
  const int pr = (tid >> 2) & 31, pp = tid & 3;
  const bool pdo = (tid >> 7) & 1;
  // (the load's zero-select is applied at the LDS write, so that the
  // prefetch of the next tile is not waited for where it is issued)
  auto tile_load = [&](int t) {
    const int q = min(t * QT + pr, a.Lq - 1);
    const uint8_t* src = (pdo ? db + (long long)q * a.do_sl : qb + (long long)q * a.q_sl) + 16 * pp;
    return *reinterpret_cast<const uint4*>(src);
  };
  auto tile_put = [&](int t, uint4 v) {
    if (t * QT + pr >= a.Lq) v = make_uint4(0u, 0u, 0u, 0u);
    char* dst = ldsQ + (2 * (t & 1) + (pdo ? 1 : 0)) * QIMG;
    *reinterpret_cast<uint4*>(dst + pr * 64 + 16 * (pp ^ (((pr >> 2) ^ (pr >> 4)) & 3))) = v;
  };
  if (tid < 256) tile_put(0, tile_load(0));
  for (int q = tid; q < LMAX; q += NT) {
    float l = INFINITY, d = 0.f;
    if (q < a.Lq) {
      l = a.lse[((long long)b * a.H + h) * a.Lq + q] - LOG2_448;
      const uint8_t* dr = db + (long long)q * a.do_sl;
      const bf16_t* orow = ob + (long long)q * a.o_sl;
#pragma unroll
      for (int c = 0; c < 8; ++c) {  // 8 elements per chunk
        const uint2 d8 = *reinterpret_cast<const uint2*>(dr + 8 * c);
        const short8_t o8 = *reinterpret_cast<const short8_t*>(orow + 8 * c);
        const auto x0 = __builtin_amdgcn_cvt_pk_f32_bf8(d8.x, false);
        const auto x1 = __builtin_amdgcn_cvt_pk_f32_bf8(d8.x, true);
        const auto x2 = __builtin_amdgcn_cvt_pk_f32_bf8(d8.y, false);
        const auto x3 = __builtin_amdgcn_cvt_pk_f32_bf8(d8.y, true);
        const float dv8[8] = {x0[0], x0[1], x1[0], x1[1], x2[0], x2[1], x3[0], x3[1]};
#pragma unroll
        for (int e = 0; e < 8; ++e) d += dv8[e] * bf2f((bf16_t)o8[e]);
      }
      d *= k1 / sdo;
    }
    ldsL[q] = l;
    ldsD[q] = d;
  }
  __syncthreads();

  f32x4 dk[U][4], dv[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int i = 0; i < 4; ++i) dk[u][i] = dv[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float amx = 0.f;  // max |dS| * sds
  // LDS addresses: every image row base below is a multiple of 16 (32 for the
  // dS image), so each swizzle term is the lane's own and a fragment address
  // is a per-lane offset plus a wave-uniform base plus a compile-time
  // immediate (no address arithmetic per read; all reads are the untracked
  // asm forms, waited for by count -- the compiler had merged tracked K / V
  // and Q / dO reads into ds_read2st64, whose 32-bank rule made them conflict)
  const uint32_t lK = (uint32_t)(uintptr_t)ldsK, lQ = (uint32_t)(uintptr_t)ldsQ;
  const uint32_t lS = (uint32_t)(uintptr_t)ldsS, lL = (uint32_t)(uintptr_t)ldsL;
  // K / V row fragments of subtile u: lK + 1024 w + kvo[ks] + 8192 u (+ KIMG for V)
  const uint32_t kvb0 = lK + 1024 * w + cl * 64 + 8 * ((0 + g) ^ (2 * ((cl >> 2) & 3)));
  const uint32_t kvb1 = lK + 1024 * w + cl * 64 + 8 * ((4 + g) ^ (2 * ((cl >> 2) & 3)));
  // Q / dO row fragments (row 8 (cl >> 2) + 4 j + (cl & 3)) and transposed ones
  uint32_t qo[2][2], to[4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qo[j][ks] = f8q_off(8 * (cl >> 2) + 4 * j + (cl & 3), 4 * ks + g);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) to[dt] = f8q_off(8 * g + (cl >> 1), 2 * dt + (cl & 1));
  // dS^T image row of subtile u: lS + 512 w + so + 4096 u (+ SIMG for odd steps)
  const uint32_t sob = lS + 512 * w + f8s_off(cl, g);
  // lse / delta of the lane's queries q0 + 8 g .. +7
  const uint32_t lgb = lL + 32 * g;

  // dQ: 8 output blocks of 16 queries x 16 head dims per step, blocks w + NW i;
  // the column sums of the bf16-rounded dQ (bias gradient) over every step
  const float gq = a.scale / (sds * sk), s8 = a.sg8 ? a.sg8[0] : 0.f;
  float csq[4] = {0.f, 0.f, 0.f, 0.f}, amq = 0.f;
  const long long dq_base = b * a.dq_sb + h * a.dq_sh;
  const int drow = 8 * g + (cl >> 1);
  auto dq_step = [&](int t) {
    const int q0 = t * QT;
    const int nkc = min(causal ? t + 1 : LMAX / 32, (klim + 31) / 32);
#pragma unroll
    for (int i = 0; i < 8 / NW; ++i) {
      const int blk = w + NW * i, qbk = blk >> 2, dt = blk & 3;
      // chunk kc: K^T at lK + dko + 2048 kc, dS at the step's image + dso + 1024 kc
      uint32_t ka = lK + f8k_off(drow, 2 * dt + (cl & 1));
      uint32_t sa = lS + (t & 1) * SIMG + f8s_off(drow, 2 * qbk + (cl & 1));
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      // batches of 4 chunks; a partial last batch reads clamped chunks and
      // zeroes their dS operand
      for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
        long kt[4], st[4];
        static_for<4>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          kt[c] = lds_read_tr8_at<2048 * c>(ka);
          st[c] = lds_read_tr8_at<1024 * c>(sa);
        });
        lgkm_wait<0>();
        const int nv = nkc - kc0;  // valid chunks of this batch (wave-uniform)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          tie(kt[c]);
          tie(st[c]);
          if (c > 0 && nv <= c) st[c] = 0;
          acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(kt[c], st[c], acc, 0, 0, 0);
        }
        ka += 4 * 2048;
        sa += 4 * 1024;
      }
      const int q = q0 + 16 * qbk + cl;
      const bool ok = q < a.Lq;
      // (uniform base + 32-bit lane offset: a 64-bit per-lane address kept
      // across the loop was spilled)
      const long long off = dq_base + (q * (int)a.dq_sl + 16 * dt + 4 * g);
      float v[4];
      bf16_t e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = f2bf(acc[r] * gq);
        v[r] = ok ? bf2f(e[r]) : 0.f;
        csq[r] += v[r];
        amq = fmaxf(amq, fabsf(v[r]));
      }
      if (ok && a.dq)
        *reinterpret_cast<uint2*>(a.dq + off) = make_uint2((uint32_t)e[0] | ((uint32_t)e[1] << 16),
                                                           (uint32_t)e[2] | ((uint32_t)e[3] << 16));
      if (ok && a.dq8) {
        int w8 = pack2_e5m2c<false>(v[0] * s8, v[1] * s8, 0);
        w8 = pack2_e5m2c<true>(v[2] * s8, v[3] * s8, w8);
        *reinterpret_cast<int*>(a.dq8 + off) = w8;
      }
    }
  };
  // Q / dO tile t by LDS-DMA (waves 0-3, one 1 KiB piece each: wave wq
  // fills tensor wq >> 1, rows 16 (wq & 1) .. +15, lane l the 16-byte
  // position l & 3 of row l >> 2 -- the source piece is swizzled instead of
  // the destination). Rows past Lq repeat row Lq - 1 (finite; their P and dS
  // are masked to 0). No destination registers: nothing for a later register
  // reuse to wait on.
  auto tile_dma = [&](int t) {
    if (w < 4) {
      const int r = 16 * (w & 1) + (lane >> 2);
      const int q = min(t * QT + r, a.Lq - 1);
      const int pc = (lane & 3) ^ (((r >> 2) ^ (r >> 4)) & 3);
      const uint8_t* src = ((w >> 1) ? db + (long long)q * a.do_sl : qb + (long long)q * a.q_sl) + 16 * pc;
      char* dst = ldsQ + (2 * (t & 1) + (w >> 1)) * QIMG + 16 * (w & 1) * 64;
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)dst,
                                       16, 0, 0);
    }
  };
  for (int it = 0; it < nq; ++it) {
    if (it > 0) {
      if (w < 4) wait_vmcnt<0>();  // this tile's DMA (issued a whole step ago by waves 0-3)
      lds_barrier();
    }
    const int q0 = it * QT;
    // dQ of the previous tile first, then the next tile's DMA
    if (it > 0) dq_step(it - 1);
    if (it + 1 < nq) tile_dma(it + 1);
    const uint32_t sQa = lQ + 2 * (it & 1) * QIMG;
    long qf[2][2], of[2][2], qT[4], oT[4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        qf[j][ks] = lds_read_b64_at<0>(sQa + qo[j][ks]);
        of[j][ks] = lds_read_b64_at<QIMG>(sQa + qo[j][ks]);
      }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      qT[dt] = lds_read_tr8_at<0>(sQa + to[dt]);
      oT[dt] = lds_read_tr8_at<QIMG>(sQa + to[dt]);
    }
    lgkm_wait<0>();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        tie(qf[j][ks]);
        tie(of[j][ks]);
      }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      tie(qT[dt]);
      tie(oT[dt]);
    }
    const uint32_t sw0 = sob + (it & 1) * SIMG;
    const uint32_t lgq = lgb + 4 * q0;
    // subtile u: S^T / dP^T, P and dS (e4m3 / e5m2 packed as they stand), the
    // dV^T / dK^T updates and dS^T into the image. (A branch-free copy of this
    // body for the all-active, unmasked case made the compiler spill 262
    // registers: one uniform branch per subtile instead.)
    static_for<U>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int s16 = 16 * (w + NW * u);  // the subtile's first key (wave-uniform)
      const bool act = s16 < klim && (!causal || s16 <= q0 + QT - 1);
      long pS = 0;
      if (act) {
        // the subtile's K / V row fragments (key on the lane) and the lse /
        // delta of the lane's 8 queries
        long kf[2], vf[2];
        kf[0] = lds_read_b64_at<8192 * u>(kvb0);
        kf[1] = lds_read_b64_at<8192 * u>(kvb1);
        vf[0] = lds_read_b64_at<KIMG + 8192 * u>(kvb0);
        vf[1] = lds_read_b64_at<KIMG + 8192 * u>(kvb1);
        f32x4 L4[2], D4[2];
        L4[0] = __builtin_bit_cast(f32x4, lds_read_b128_at<0>(lgq));
        L4[1] = __builtin_bit_cast(f32x4, lds_read_b128_at<16>(lgq));
        D4[0] = __builtin_bit_cast(f32x4, lds_read_b128_at<4 * LMAX>(lgq));
        D4[1] = __builtin_bit_cast(f32x4, lds_read_b128_at<4 * LMAX + 16>(lgq));
        lgkm_wait<4>();
        tie(kf[0]);
        tie(kf[1]);
        tie(vf[0]);
        tie(vf[1]);
        f32x4 s[2], dp[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(qf[j][0], kf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(qf[j][1], kf[1], s[j], 0, 0, 0);
          dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(of[j][0], vf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(of[j][1], vf[1], dp[j], 0, 0, 0);
        }
        lgkm_wait<0>();
        tie(L4[0]);
        tie(L4[1]);
        tie(D4[0]);
        tie(D4[1]);
        const bool full = s16 + 15 < klim && q0 + QT <= a.Lq && (!causal || s16 + 15 <= q0);
        float x[2][4];
        if (full) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) x[j][r] = fmaf(s[j][r], c8, -L4[j][r]);
        } else {
          const int key = s16 + cl;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int q = q0 + 8 * g + 4 * j + r;
              const bool ok = (key < klim) & (q < a.Lq) & (!causal | (key <= q));  // (no short circuit)
              const float xv = fmaf(s[j][r], c8, -L4[j][r]);
              x[j][r] = ok ? xv : -INFINITY;
            }
        }
        int pw[2], sw[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // 448 P = exp2(x): x <= 0 up to rounding (the forward's LSE over the
          // same e4m3 products), so 448 P rounds to at most e4m3's 448
          float p[4], ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            p[r] = fast_exp2(x[j][r]);
            ds[r] = p[r] * fmaf(dp[j][r], cdp, -D4[j][r]);
          }
          amx = fmaxf(amx, fmaxf(fmaxf(fabsf(ds[0]), fabsf(ds[1])), fmaxf(fabsf(ds[2]), fabsf(ds[3]))));
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[r] = __builtin_amdgcn_fmed3f(ds[r], -E5M2_MAX_F, E5M2_MAX_F);
          // (the first convert's old operand: any register -- the second one
          // overwrites its other half)
          const int pv = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], __float_as_int(p[2]), false);
          pw[j] = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], pv, true);
          const int sv2 = __builtin_amdgcn_cvt_pk_bf8_f32(ds[0], ds[1], __float_as_int(ds[2]), false);
          sw[j] = __builtin_amdgcn_cvt_pk_bf8_f32(ds[2], ds[3], sv2, true);
        }
        const long pP = (long)(uint32_t)pw[0] | ((long)pw[1] << 32);
        pS = (long)(uint32_t)sw[0] | ((long)sw[1] << 32);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[u][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(oT[dt], pP, dv[u][dt], 0, 0, 0);
          dk[u][dt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(qT[dt], pS, dk[u][dt], 0, 0, 0);
        }
      }
      lds_write_b64_at<4096 * u>(sw0, pS);
    });
  }
  wait_vmcnt<0>();
  lds_barrier();
  dq_step(nq - 1);

  // ---- epilogue: dK / dV (key rows on lanes) bf16 and / or e5m2, amax and
  // the bias-gradient column sums (dQ's, dK's, dV's) of this (b, h)
  const float gk = a.scale / (sds * sq), gv = 1.f / (448.f * sdo);
  const float s8kv = a.sgkv8 ? a.sgkv8[0] : s8;  // dK / dV e5m2 scale
  float csk[4][4], csv[4][4], amk = 0.f;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) csk[dt][r] = csv[dt][r] = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int key = 16 * (w + NW * u) + cl;
    const bool ok = key < a.Lk;
    const long long offk = b * a.dk_sb + (long long)key * a.dk_sl + h * a.dk_sh;
    const long long offv = b * a.dv_sb + (long long)key * a.dv_sl + h * a.dv_sh;
    uint32_t klo[4], khi[4], vlo[4], vhi[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      pack_acc(dk[u][dt], gk, klo[dt], khi[dt]);
      pack_acc(dv[u][dt], gv, vlo[dt], vhi[dt]);
    }
    if (a.dk) store_row16<4>(a.dk + offk, klo, khi, g, ok);
    if (a.dv) store_row16<4>(a.dv + offv, vlo, vhi, g, ok);
    if (a.dk8) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const float k4[4] = {__uint_as_float(klo[dt] << 16), __uint_as_float(klo[dt] & 0xffff0000u),
                             __uint_as_float(khi[dt] << 16), __uint_as_float(khi[dt] & 0xffff0000u)};
        const float v4[4] = {__uint_as_float(vlo[dt] << 16), __uint_as_float(vlo[dt] & 0xffff0000u),
                             __uint_as_float(vhi[dt] << 16), __uint_as_float(vhi[dt] & 0xffff0000u)};
        int wk = pack2_e5m2c<false>(k4[0] * s8kv, k4[1] * s8kv, 0);
        wk = pack2_e5m2c<true>(k4[2] * s8kv, k4[3] * s8kv, wk);
        int wv = pack2_e5m2c<false>(v4[0] * s8kv, v4[1] * s8kv, 0);
        wv = pack2_e5m2c<true>(v4[2] * s8kv, v4[3] * s8kv, wv);
        if (ok) {
          *reinterpret_cast<int*>(a.dk8 + offk + 16 * dt + 4 * g) = wk;
          *reinterpret_cast<int*>(a.dv8 + offv + 16 * dt + 4 * g) = wv;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          csk[dt][r] += ok ? k4[r] : 0.f;
          csv[dt][r] += ok ? v4[r] : 0.f;
          amk = fmaxf(amk, ok ? fmaxf(fabsf(k4[r]), fabsf(v4[r])) : 0.f);
        }
      }
    }
  }
  // amax: dS (its own slot), the gradients (the projection's e5m2 slot)
  amx = wave_max(amx);
  if (lane == 0 && a.amaxds8) atomic_amax(amax_word(a.amaxds8, b * 7 + h * 13 + w), amx / sds);
  if (a.amaxgkv8) {  // dK / dV in their own slot
    const float amq_w = wave_max(amq), amk_w = wave_max(amk);
    if (lane == 0 && a.amaxg8 && a.dq8) atomic_amax(amax_word(a.amaxg8, b * 5 + h * 11 + w), amq_w);
    if (lane == 0 && a.dk8) atomic_amax(amax_word(a.amaxgkv8, b * 5 + h * 11 + w), amk_w);
  } else {
    const float amg = wave_max(fmaxf(amq, amk));
    if (lane == 0 && a.amaxg8 && (a.dq8 || a.dk8)) atomic_amax(amax_word(a.amaxg8, b * 5 + h * 11 + w), amg);
  }
  if (!a.cs_part) return;
  // column sums: over the wave's 16 rows per lane group (shuffles), then the
  // waves through LDS (the Q / dO ring is free: every read of it is behind the
  // last barrier)
  float* red = reinterpret_cast<float*>(ldsQ);  // [3][NW][64]
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) csq[r] += __shfl_xor(csq[r], sh, 64);
  if (a.dk8) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) {
          csk[dt][r] += __shfl_xor(csk[dt][r], sh, 64);
          csv[dt][r] += __shfl_xor(csv[dt][r], sh, 64);
        }
  }
  if (cl == 0) {
    const int dtq = w & 3;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * dt + 4 * g + r;
        red[w * 64 + col] = dt == dtq ? csq[r] : 0.f;
        red[(NW + w) * 64 + col] = csk[dt][r];
        red[(2 * NW + w) * 64 + col] = csv[dt][r];
      }
  }
  __syncthreads();
  float* prow = a.cs_part + ((long long)b * a.cs_np) * a.cs_ld + h * 64;
  float* prow2 = a.cs_part2 ? a.cs_part2 + (long long)b * a.cs_ld2 + h * 64 : prow;
  if (tid < 64 * (a.dk8 ? 3 : 1)) {
    const int m = tid >> 6, col = tid & 63;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) sum += red[(m * NW + i) * 64 + col];
    if (m == 0) prow[a.cs_q + col] = sum;
    else prow2[(m == 1 ? a.cs_k : a.cs_v) + col] = sum;
  }
}

}  // namespace tdg

using namespace tdg;

namespace {
template <int NS, int U>
int fwd_fp8_u(const AttnArgs& a, hipStream_t st) {
  big_lds<attn_fwd_fp8_kernel<NS, U>>();
  hipLaunchKernelGGL((attn_fwd_fp8_kernel<NS, U>), dim3(cdiv(a.Lq, 128 * U), a.H, a.B), dim3(512),
                     NS * 2 * 64 * 64, st, a);
  return 0;
}
int fwd_fp8_ns() {
  static const int v = [] {
    const char* e = getenv("TDG_ATTN_FWD8_NS");
    return e ? atoi(e) : 3;
  }();
  return v;
}
}  // namespace
// ring depth NS from TDG_ATTN_FWD8_NS (3, 4 or 6: measured equal, 3 kept).
// (32 queries per wave, U = 2, measured 3-5 % slower at seq 512 and is not
// instantiated: profiles/r5/attn_fwd8_u_rows.txt)
extern "C" int tdg_attn_fwd_fp8(const AttnArgs* a, int hd, hipStream_t st) {
  if (hd != 64) return -1;
  switch (fwd_fp8_ns()) {
    case 4: return fwd_fp8_u<4, 1>(*a, st);
    case 6: return fwd_fp8_u<6, 1>(*a, st);
    default: return fwd_fp8_u<3, 1>(*a, st);
  }
}
namespace {
template <int NW>
int bwd_f8_nw(const AttnArgs& a, hipStream_t st) {
  constexpr int lds = 2 * 512 * 64 + 4 * 32 * 64 + 2 * 512 * 32 + 2 * 512 * 4;  // 108 KiB
  big_lds<attn_bwd_f8_kernel<NW>>(lds);
  hipLaunchKernelGGL(attn_bwd_f8_kernel<NW>, dim3(1, a.H, a.B), dim3(NW * 64), lds, st, a);
  return 0;
}
}  // namespace
// hd 64, Lq, Lk <= 512: one 8-wave workgroup per (batch, head) (4 waves of
// 8 subtiles each -- one wave per SIMD -- spilled 155 registers at -O3)
extern "C" int tdg_attn_bwd_f8(const AttnArgs* a, int hd, hipStream_t st) {
  if (hd != 64 || a->Lq < 1 || a->Lk < 1 || a->Lq > 512 || a->Lk > 512) return -1;
  return bwd_f8_nw<8>(*a, st);
}
