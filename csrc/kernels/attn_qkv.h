// Fused Q|K|V projection + attention forward and its launcher (design:
// attn_impl.h). Holds definitions: include it from one translation unit only.
#pragma once
#include "attn_impl.h"

namespace tdg {

// ============================================================================ fused Q|K|V projection + attention forward
// Self-attention of sequences of <= 128 tokens at head dim 64: one workgroup
// per (batch, head) computes the head's Q|K|V = X_b W_h^T + b_h (128 x 192,
// K = d_model; the GEMM main loop of gemm_impl.h: LDS-DMA K tiles, 8 waves as
// 2 x 4 of 64 x 48, MFMAs with swapped operands) and keeps them in LDS as the
// attention's K / V images and Q rows, writes them to the [M, 3d] projection
// output (the backward reads it), and runs the attention forward of
// attn_fwd_kernel on them (8 waves x 16 queries, one 128-key tile). The
// separate projection launch, its Q|K|V write and the attention's re-read of
// them (the attention forward at L = 128 is a load burst + a short compute
// phase) become one launch whose attention phase reads LDS.
// (reference: transformer_model.py:112-166 -- the Q / K / V Dense layers and
// scaled_dot_product_attention of MultiHeadAttention)
// CROSS (cross-attention): the GEMM is the head's Q projection only (128 x
// 64, 8 waves as 4 x 2 of 32 x 32) and K / V come from the batched K|V
// projection in memory (a.k / a.v), their loads issued before the GEMM.
// SB1: single-buffered fragments and a two-barrier K loop (the register
// budget of two workgroups per CU), STAGES = 2.
template <int STAGES, bool CROSS, bool SB1 = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(SB1 ? 4 : 2))) void qkv_attn_fwd_kernel(
    const QkvAttnArgs qa) {
  constexpr int NW = 8, WM = CROSS ? 4 : 2, WN = CROSS ? 2 : 4, BM = 128, BN = CROSS ? 64 : 192;
  constexpr int NPART = BN / 64;                      // projection parts computed here
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;  // 4 x 3 (2 x 2) subtiles per wave
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, SB = A_BYTES + B_BYTES;
  using GA = Glds<true, BM, NW>;
  using GB = Glds<true, BN, NW>;
  constexpr int PT = GA::P + GB::P;
  using T = ATile<64>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AttnArgs& a = qa.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  // (head, batch): each XCD a contiguous run of batch elements, so a batch
  // element's X panel is read into one XCD's L2 for its heads
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int h = t % a.H, b = t / a.H;
  const int L = qa.L, d = qa.d, K = d;
  const bf16_t* X = reinterpret_cast<const bf16_t*>(qa.x) + (size_t)b * L * qa.ldx;
  // cross-attention K / V (128 keys each, two 64-row tiles): global loads now,
  // LDS after the GEMM
  using Ch = typename ATile<64>::template Chunks<512>;
  Ch ck[2], cv[2];
  if constexpr (CROSS) {
    const bf16_t* kb = a.k + b * a.k_sb + h * a.k_sh;
    const bf16_t* vb = a.v + b * a.v_sb + h * a.v_sh;
#pragma unroll
    for (int h64 = 0; h64 < 2; ++h64) {
      ATile<64>::template fetch<512>(ck[h64], kb, a.k_sl, 64 * h64, a.Lk, tid);
      ATile<64>::template fetch<512>(cv[h64], vb, a.v_sl, 64 * h64, a.Lk, tid);
    }
  }

  // ------------------------------------------------ Q|K|V GEMM (K = d_model)
  GA ga;
  GB gb;
  ga.init(wid, lane);
  gb.init(wid, lane);
  // B rows r of the tile: W row (r / 64) * d + 64 h + r % 64 (a 1 KiB piece
  // covers 8 rows of one 64-row block)
  int wrow[GB::P];
#pragma unroll
  for (int i = 0; i < GB::P; ++i) wrow[i] = (gb.row[i] >> 6) * d + 64 * h + (gb.row[i] & 63);
  auto issue_b = [&](int k0, char* lds) {
#pragma unroll
    for (int i = 0; i < GB::P; ++i) {
      const long long off = (long long)wrow[i] * qa.ldw + k0 + gb.col[i];
      __builtin_amdgcn_global_load_lds((const void*)(reinterpret_cast<const bf16_t*>(qa.w) + off),
                                       (__attribute__((address_space(3))) void*)(lds + (wid * GB::P + i) * 1024),
                                       16, 0, 0);
    }
  };
  const int nk = K / BK;
  f32x4 acc[TM][TN];
  TDG_ZERO(TM, TN, acc)
#pragma unroll
  for (int st = 0; st < STAGES; ++st) {
    if (st < nk) {
      ga.issue(X, qa.ldx, L, K, 0, st * BK, smem + st * SB, wid);
      issue_b(st * BK, smem + st * SB + A_BYTES);
    }
  }
  const int abase = wm * (BM / WM), bbase = wn * (BN / WN);
  if constexpr (SB1) {
    short8_t fa[TM], fb[TN];
    for (int kt = 0; kt < nk; ++kt) {
      // tile kt landed (the younger tile, if any, stays in flight)
      if (kt + 1 < nk) wait_vmcnt<PT>();
      else wait_vmcnt<0>();
      lds_barrier();
      const char* st = smem + (kt % STAGES) * SB;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = frag<true, BM>(st, abase + 16 * i, s2, lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = frag<true, BN>(st + A_BYTES, bbase + 16 * j, s2, lane);
        lgkm_wait<0>();
        tie_all(fa);
        tie_all(fb);
        prio_hi();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(fb[j], fa[i], acc[i][j]);
        prio_lo();
      }
      lds_barrier();  // everyone done with the stage: refill it
      if (kt + STAGES < nk) {
        char* ns = smem + (kt % STAGES) * SB;
        ga.issue(X, qa.ldx, L, K, 0, (kt + STAGES) * BK, ns, wid);
        issue_b((kt + STAGES) * BK, ns + A_BYTES);
      }
    }
  } else {
  short8_t fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  if (nk >= STAGES)
    wait_vmcnt<(STAGES - 1) * PT>();
  else
    wait_vmcnt<0>();
  lds_barrier();
#pragma unroll
  for (int i = 0; i < TM; ++i) fa0[i] = frag<true, BM>(smem, abase + 16 * i, 0, lane);
#pragma unroll
  for (int j = 0; j < TN; ++j) fb0[j] = frag<true, BN>(smem + A_BYTES, bbase + 16 * j, 0, lane);
  constexpr int STEP_OPS = TM + TN;
  auto kstep = [&](int kt, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    const char* st = smem + (kt % STAGES) * SB;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa1[i] = frag<true, BM>(st, abase + 16 * i, 1, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb1[j] = frag<true, BN>(st + A_BYTES, bbase + 16 * j, 1, lane);
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
        ga.issue(X, qa.ldx, L, K, 0, (kt + STAGES) * BK, ns, wid);
        issue_b((kt + STAGES) * BK, ns + A_BYTES);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) fa0[i] = frag<true, BM>(nx, abase + 16 * i, 0, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb0[j] = frag<true, BN>(nx + A_BYTES, bbase + 16 * j, 0, lane);
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
  {
    int kt = 0;
    for (; kt + STAGES < nk; ++kt) kstep(kt, std::integral_constant<int, 3>{});
    if (kt + STAGES - 1 < nk && kt + 1 < nk) kstep(kt++, std::integral_constant<int, 2>{});
    for (; kt + 1 < nk; ++kt) kstep(kt, std::integral_constant<int, 1>{});
    if (kt < nk) kstep(kt, std::integral_constant<int, 0>{});
  }
  }
  lds_barrier();  // the pipeline stages become the Q / K / V images

  // ------------------------------------------------ bias, bf16, LDS images
  // image p (0 Q, 1 K, 2 V): 128 rows x 64 head dims in the attention's
  // K-image layout (T::off over 128 rows = two 64-row tiles)
  char* img = smem;
  constexpr int IMG = 2 * T::BYTES;
  const int g = lane >> 4, cl = lane & 15;
  if constexpr (CROSS) {
#pragma unroll
    for (int h64 = 0; h64 < 2; ++h64) {
      ATile<64>::template put<512>(img + IMG + h64 * T::BYTES, ck[h64], tid);
      ATile<64>::template put<512>(img + 2 * IMG + h64 * T::BYTES, cv[h64], tid);
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = bbase + 16 * j + 4 * g;  // 4 consecutive columns of one image
    const int part = n >> 6, hc = n & 63;
    const f32x4 bn = *reinterpret_cast<const f32x4*>(qa.bias + part * d + 64 * h + hc);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = abase + 16 * i + cl;
      short4_t o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(acc[i][j][r] + bn[r]);
      *reinterpret_cast<short4_t*>(img + part * IMG + T::off(m, hc * 2)) = o;
    }
  }
  __syncthreads();
  // the projection output for the backward ([M, NPART d]): rows < L,
  // 16-byte chunks
  {
    const WtBuf wt(qa.qkv, ((size_t)(b + 1) * L * NPART * d) * sizeof(bf16_t));
#pragma unroll
    for (int pass = 0; pass < NPART * 128 * 8 / 512; ++pass) {
      const int id = tid + 512 * pass;
      const int part = id >> 10, row = (id >> 3) & 127, c = id & 7;
      const short8_t v = *reinterpret_cast<const short8_t*>(img + part * IMG + T::off(row, c * 16));
      if (row < L)
        wt.st16(reinterpret_cast<bf16_t*>(qa.qkv) + ((size_t)b * L + row) * NPART * d + part * d + 64 * h + c * 8,
                v);
    }
  }

  // ------------------------------------------------ attention (attn_fwd_kernel, 8 x 16 queries)
  const char* ldsQ = img;
  const char* ldsK = img + IMG;
  const char* ldsV = img + 2 * IMG;
  const int w = wid;
  const int qrow = 16 * w + cl;
  int klim;
  float scl;
  bool causal;
  key_window(a, b, klim, scl, causal);
  if (causal) klim = min(klim, 128);
  const float c = scl * LOG2E;
  const int wq0 = 16 * w;
  short8_t qf[T::KS];
#pragma unroll
  for (int s2 = 0; s2 < T::KS; ++s2) qf[s2] = T::frag_row(ldsQ, 16 * w, s2, lane);
  f32x4 oacc[T::DT];
  TDG_ZERO1(T::DT, oacc)
  float m = -INFINITY, l = 0.f;
  constexpr int NT16 = 8;
  if (klim > 0) {
    f32x4 sc[NT16];
#pragma unroll
    for (int tt = 0; tt < NT16; ++tt) {
      sc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) sc[tt] = mfma16(T::frag_row(ldsK, 16 * tt, ks, lane), qf[ks], sc[tt]);
    }
    short8_t pf[NT16 / 2];
    softmax_tile<NT16, T::DT>(sc, m, l, oacc, pf, tile_masked(0, 128, klim, causal, wq0), 0, klim, causal,
                              qrow, g, c);
#pragma unroll
    for (int s2 = 0; s2 < NT16 / 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) oacc[dt] = mfma16(T::frag_tr(ldsV, s2, dt, lane), pf[s2], oacc[dt]);
  }
  TDG_FWD_FINISH(T::DT, a, b, h, qrow, oacc, m, l, g)
}

}  // namespace tdg

using namespace tdg;

// Fused Q|K|V projection + attention forward (qkv_attn_fwd_kernel): L <= 128,
// hd 64, d % 64 == 0. Self-attention: 2 stages, single-buffered fragments,
// two workgroups per CU (116 VGPRs): 21.5 us per call at B 64, L 128, H 8
// against 25.7 for 3 stages with double-buffered fragments at one workgroup
// per CU (144 VGPRs; with 2 stages and double buffering it spilled, 32.1 us;
// profiles/r6/attn_fused_projections.txt). qa->cross:
// the cross-attention form (Q projection only, K / V from a.k / a.v, Lk <=
// 128). Returns -1 when the shape is not covered.
namespace {
template <int STAGES, bool CROSS, bool SB1>
void qkv_attn_launch(const QkvAttnArgs& qa, hipStream_t st) {
  constexpr int SB = (128 + (CROSS ? 64 : 192)) * BK * 2;
  big_lds<qkv_attn_fwd_kernel<STAGES, CROSS, SB1>>();
  attn_plan_record(CROSS ? ATTN_QKV_CROSS : ATTN_QKV_SELF, 64, (long long)qa.a.B * qa.a.H, 512);
  hipLaunchKernelGGL((qkv_attn_fwd_kernel<STAGES, CROSS, SB1>), dim3(qa.a.B * qa.a.H), dim3(512),
                     STAGES * SB, st, qa);
}

}  // namespace
extern "C" int tdg_qkv_attn_fwd(const QkvAttnArgs* qa, hipStream_t st) {
  const AttnArgs& a = qa->a;
  if (qa->L > 128 || qa->L <= 0 || a.Lq != qa->L || a.Lk > 128 || a.Lk <= 0 || qa->d % 64 ||
      qa->d != 64 * a.H || qa->ldx % 8 || qa->ldw % 8 || (!qa->cross && a.Lk != qa->L))
    return -1;
  if (qa->cross)
    qkv_attn_launch<3, true, false>(*qa, st);
  else
    qkv_attn_launch<2, false, true>(*qa, st);
  return 0;
}
