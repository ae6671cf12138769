// Flash-style fused multi-head attention for gfx950 (forward + backward).
//
// Replaces the reference's scaled_dot_product_attention
// (reference: distributed_training_transformer/transformer_model.py:73-109):
//   softmax(Q K^T / sqrt(dk) + mask*-1e9) V
// with the [B,h,Lq,Lk] score tensor never materialised. Padding masks are
// per-batch key lengths (right-padded PAD=0 tokens, transformer_model.py:56-62)
// and the look-ahead mask (transformer_model.py:65-70) is causal tile skipping
// plus an in-tile compare; masked logits contribute exactly 0 probability, as
// exp(-1e9) does in the reference.
//
// Design (CDNA4): one workgroup = 4 waves = 64 query rows (forward / dQ) or
// 64 key rows (dK/dV) of one (batch, head). MFMA v_mfma_f32_16x16x32_bf16.
// Forward computes S^T = K Q^T so that every lane owns one query row (lane&15)
// and 4 key positions per 16-key tile: the row softmax is register-local plus
// two cross-lane xors, and the P accumulators feed the P^T operand of
// O^T = V^T P^T directly (keys permuted consistently on both operands), the V
// operand coming from the transposing ds_read_b64_tr_b16. K/V tiles are staged
// through one XOR-swizzled LDS image that is conflict-free both for the
// 16-byte row reads and for the transposed reads (docs/KERNELS.md).
// Backward: two kernels (dK/dV with key rows on lanes, dQ with query rows on
// lanes), each recomputing P from the forward's log-sum-exp; no atomics, so
// gradients are bitwise deterministic.
#pragma once
#include "tdg_api.h"
#include "tdg_common.h"
#include "tdg_attn.h"

#include <cstdlib>
#include "tdg_gemm.h"

namespace tdg {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LOG2_448 = 8.807354922057604f;  // log2(448): the e4m3 P scale

// v_exp_f32 as is: libm's exp2f wraps it in a denormal-range fix-up (compare,
// select, ldexp: 4 more VALU per element); softmax weights below 2^-126
// flushed to zero change nothing at bf16 P.
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// ok ? exp2(x) : 0 as a select: exp2 computed for every lane (x is finite or
// -inf on the masked side, never NaN). Written as the conditional expression,
// the compiler branched around each element's exp (exec-mask save / restore,
// ~10 instructions per element on every masked tile).
__device__ __forceinline__ float masked_exp2(float x, bool ok) {
  float e = fast_exp2(x);
  asm volatile("" : "+v"(e));
  return ok ? e : 0.f;
}

// Row-per-lane store of a 16x16-MFMA output row: lane (g, cl) holds columns
// 16 dt + 4 g .. +3 (dt < DT) of its row as packed bf16 pairs lo[dt] / hi[dt].
// For each dt pair, v_permlane16_swap exchanges the odd 16-lane groups' dt
// half with the even groups' dt + 1 half, after which every lane holds 16
// contiguous bytes -- columns 16 (dt + (g & 1)) + 8 (g >> 1) .. +7 -- and
// writes them with one dwordx4: half the store instructions of the 8-byte
// form, whose tail was store-issue-bound (the guide's T21). Every lane of
// the wave must call it (the swaps); `store` masks the lane's row.
template <int DT>
__device__ __forceinline__ void store_row16(bf16_t* __restrict__ row, const uint32_t (&lo)[DT],
                                            const uint32_t (&hi)[DT], int g, bool store) {
  if constexpr (DT % 2 == 0) {
#pragma unroll
    for (int d = 0; d < DT; d += 2) {
      const auto r0 = __builtin_amdgcn_permlane16_swap(lo[d], lo[d + 1], false, false);
      const auto r1 = __builtin_amdgcn_permlane16_swap(hi[d], hi[d + 1], false, false);
      if (store)
        *reinterpret_cast<uint4*>(row + 16 * (d + (g & 1)) + 8 * (g >> 1)) =
            make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
  } else {
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (store) *reinterpret_cast<uint2*>(row + 16 * d + 4 * g) = make_uint2(lo[d], hi[d]);
  }
}
// (the packing of an accumulator: 4 values, times sc)
__device__ __forceinline__ void pack_acc(const f32x4& v, float sc, uint32_t& lo, uint32_t& hi) {
  lo = pack2bf(v[0] * sc, v[1] * sc);
  hi = pack2bf(v[2] * sc, v[3] * sc);
}
// two accumulators as one 8-element bf16 MFMA operand
__device__ __forceinline__ short8_t pack8(const f32x4& x, const f32x4& y) {
  return pack8(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]);
}
// accumulator arrays to zero: x[N], x[U][N], and x[U][N] together with y[U][N]
#define TDG_ZERO1(N_, x) _Pragma("unroll") for (int i_ = 0; i_ < N_; ++i_) (x)[i_] = f32x4{0.f, 0.f, 0.f, 0.f};
#define TDG_ZERO(U_, N_, x) \
  _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_) TDG_ZERO1(N_, (x)[u_])
#define TDG_ZERO2(U_, N_, x, y)                                                                   \
  _Pragma("unroll") for (int u_ = 0; u_ < U_; ++u_) _Pragma("unroll") for (int i_ = 0; i_ < N_; ++i_) \
      (x)[u_][i_] = (y)[u_][i_] = f32x4{0.f, 0.f, 0.f, 0.f};

// 16-byte global load from an always-valid (clamped) address, zero where
// !ok: a select instead of an exec-mask branch around every prologue load
__device__ __forceinline__ short8_t ld8_or0(const bf16_t* p, bool ok) {
  const short8_t v = *reinterpret_cast<const short8_t*>(p);
  const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? v : z;
}

// Key window and logit scale of batch row b. A row with NO valid key
// (kv_len == 0: an all-PAD sequence) gets the reference's numerics: its
// padding mask adds -1e9 to every logit, which in fp32 leaves them all equal
// (transformer_model.py:101-105), so the softmax is uniform over ALL Lk keys
// (padding included) -- reproduced by attending to all Lk keys with a zero
// logit scale for P. The backward is TF's autograd of that graph: dS =
// P (dP - delta) with the uniform P, and dQ / dK keep the real scale (the
// mask add passes the gradient through). In causal attention such a row's
// look-ahead mask is covered by the padding mask too (the reference combines
// them with a maximum, transformer_model.py:361-362): all keys, causal off.
__device__ __forceinline__ void key_window(const AttnArgs& a, int b, int& klim, float& scale,
                                           bool& causal) {
  klim = a.Lk;
  scale = a.scale;
  causal = a.causal != 0;
  if (a.kv_len) {
    const int n = a.kv_len[b];
    if (n > 0) {
      klim = min(klim, n);
    } else {
      scale = 0.f;
      causal = false;
    }
  }
}
// (block, head, batch) of this workgroup over a (blocks, H, B) grid; with
// a.xcd the linear order is xcd_remap'd (tdg_common.h), so the XCD that ran
// the projection GEMM tiles of a batch element's rows (their run of tile ids
// covers whole row bands) also runs that element's attention workgroups
__device__ __forceinline__ void attn_coords(const AttnArgs& a, int& xb, int& h, int& b) {
  const int gx = gridDim.x, gy = gridDim.y;
  int t = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  if (a.xcd) t = xcd_remap(t, gx * gy * gridDim.z);
  xb = t % gx;
  h = (t / gx) % gy;
  b = t / (gx * gy);
}
constexpr int QB = 64;  // rows per workgroup
constexpr int KB = 64;  // keys per tile

template <int HD>
struct ATile {
  static constexpr int RB = HD * 2;                       // bytes per row
  static constexpr int SEGS = HD / 16 > 0 ? HD / 16 : 1;  // 32-byte segments per row
  static constexpr int RPB = 128 / HD;                    // rows per 256-B bank row
  static constexpr int BYTES = 64 * RB;
  static constexpr int KS = HD >= 32 ? HD / 32 : 1;       // 32-deep MFMA steps over head dim
  static constexpr int DT = HD / 16;                      // 16-wide tiles over head dim
  __device__ static __forceinline__ int off(int row, int byte) {
    const int seg = (byte >> 5) ^ ((row / RPB) & (SEGS - 1));
    return row * RB + (seg << 5) + (byte & 31);
  }
  // Stage 64 rows (row0..row0+63, rows >= nrows zero) of a [L, ...] tensor,
  // in two halves so that callers can issue the global loads of several
  // tiles before the first LDS write (one memory latency, not one per tile).
  template <int NT = 256>
  struct Chunks {
    static constexpr int CPR = HD / 8;
    static constexpr int TOTAL = 64 * CPR;
    static constexpr int NI = (TOTAL + NT - 1) / NT;
    short8_t v[NI];
  };
  template <int NT = 256>
  __device__ static __forceinline__ void fetch(Chunks<NT>& c, const bf16_t* __restrict__ base,
                                               long long sl, int row0, int nrows, int tid) {
    using C = Chunks<NT>;
#pragma unroll
    for (int i = 0; i < C::NI; ++i) {
      const int id = tid + i * NT;
      const int row = id / C::CPR, cc = id % C::CPR;
      if constexpr (C::TOTAL % NT == 0) {  // (rows past nrows: clamped load, zeroed)
        const int r = min(row0 + row, nrows - 1);
        c.v[i] = ld8_or0(base + (long long)r * sl + cc * 8, row0 + row < nrows);
      } else {
        c.v[i] = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (id < C::TOTAL && row0 + row < nrows)
          c.v[i] = *reinterpret_cast<const short8_t*>(base + (long long)(row0 + row) * sl + cc * 8);
      }
    }
  }
  template <int NT = 256>
  __device__ static __forceinline__ void put(char* lds, const Chunks<NT>& c, int tid) {
    using C = Chunks<NT>;
#pragma unroll
    for (int i = 0; i < C::NI; ++i) {
      const int id = tid + i * NT;
      if (C::TOTAL % NT != 0 && id >= C::TOTAL) break;
      const int row = id / C::CPR, cc = id % C::CPR;
      *reinterpret_cast<short8_t*>(lds + off(row, cc * 16)) = c.v[i];
    }
  }
  template <int NT = 256>
  __device__ static __forceinline__ void load(char* lds, const bf16_t* __restrict__ base,
                                              long long sl, int row0, int nrows, int tid) {
    Chunks<NT> c;
    fetch<NT>(c, base, sl, row0, nrows, tid);
    put<NT>(lds, c, tid);
  }
  // Row fragment: lane holds X[rbase + (lane&15)][32s + 8(lane>>4) + j]
  __device__ static __forceinline__ short8_t frag_row(const char* lds, int rbase, int s, int lane) {
    const int row = rbase + (lane & 15);
    const int c = 4 * s + (lane >> 4);
    if constexpr (HD < 32) {
      const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
      const short8_t v =
          *reinterpret_cast<const short8_t*>(lds + off(row, (c & (HD / 8 - 1)) * 16));
      return c < HD / 8 ? v : z;
    } else {
      return *reinterpret_cast<const short8_t*>(lds + off(row, c * 16));
    }
  }
  // The same row fragment read untracked (tdg_common.h lds_read_b128_async):
  // for loops with LDS-DMA in flight, where the compiler would put a
  // vmcnt(0) before a tracked read; the caller waits (lgkm_wait) and ties.
  __device__ static __forceinline__ short8_t frag_row_async(const char* lds, int rbase, int s, int lane) {
    static_assert(HD >= 32, "untracked row fragments: hd >= 32");
    const int row = rbase + (lane & 15);
    const int c = 4 * s + (lane >> 4);
    return lds_read_b128_async(lds + off(row, c * 16));
  }
  // Offset-immediate forms (tdg_common.h lds_read_*_at): the lane part of
  // the address once per tile, the row base in the DS offset field.
  // row_off: frag_row_async's lane part for row bases that are multiples of
  // 8 (the swizzle term is then the lane's own); frag_row_at<RBASE>(tile
  // address + row_off(s, lane)) == frag_row_async(tile, RBASE, s, lane).
  __device__ static __forceinline__ uint32_t row_off(int s, int lane) {
    return (uint32_t)off(lane & 15, (4 * s + (lane >> 4)) * 16);
  }
  template <int RBASE>
  __device__ static __forceinline__ short8_t frag_row_at(uint32_t a) {
    static_assert(RBASE % 8 == 0, "row base: multiple of 8");
    return lds_read_b128_at<RBASE * RB>(a);
  }
  // tr_off: frag_tr_async's lane part (rows 4 g + q of k-step 0: the swizzle
  // term is the same at + 16 and + 32 s2 rows)
  __device__ static __forceinline__ uint32_t tr_off(int dt, int lane) {
    const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
    return (uint32_t)off(4 * g + q, (16 * dt + 4 * p) * 2);
  }
  template <int S2>
  __device__ static __forceinline__ void frag_tr_at(uint32_t a, short4_t& lo, short4_t& hi) {
    lo = lds_read_tr16_at<32 * S2 * RB>(a);
    hi = lds_read_tr16_at<(32 * S2 + 16) * RB>(a);
  }
  // Transposed fragment, untracked, as its two 8-byte halves (tie both
  // after the wait, then cat4)
  __device__ static __forceinline__ void frag_tr_async(const char* lds, int s2, int dt, int lane,
                                                       short4_t& lo, short4_t& hi) {
    const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
    const int r1 = 32 * s2 + 4 * g + q;
    const int byte = (16 * dt + 4 * p) * 2;
    lo = lds_read_tr_async(lds + off(r1, byte));
    hi = lds_read_tr_async(lds + off(r1 + 16, byte));
  }
  // Transposed fragment over 32 rows (k-step s2 of a 64-row tile), head-dim
  // columns 16dt..16dt+15. Element j of lane group g is row
  // 32s2 + (j<4 ? 4g+j : 16+4g+j-4) (the key/query permutation that matches
  // the accumulator layout of a 16x16 MFMA output), column 16dt + (lane&15).
  __device__ static __forceinline__ short8_t frag_tr(const char* lds, int s2, int dt, int lane) {
    const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
    const int r1 = 32 * s2 + 4 * g + q;
    const int byte = (16 * dt + 4 * p) * 2;
    return cat4(lds_read_tr(lds + off(r1, byte)), lds_read_tr(lds + off(r1 + 16, byte)));
  }
};

// Load a head-row fragment straight from global: X[row][32s + 8g + j]
template <int HD>
__device__ __forceinline__ short8_t gfrag(const bf16_t* __restrict__ rowp, bool valid, int s,
                                          int lane) {
  const int c = 4 * s + (lane >> 4);
  if constexpr (HD >= 64) {  // (c < HD / 8 always; rowp is a clamped, valid row)
    return ld8_or0(rowp + c * 8, valid);
  } else {
    short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (valid && c < HD / 8) v = *reinterpret_cast<const short8_t*>(rowp + c * 8);
    return v;
  }
}


// One key tile of the online softmax for the lane's query row (swapped
// QK^T: s[t][r] = S[key = k0 + 16t + 4g + r][row], raw logits). m is the
// running max in the scaled log2 domain (max of c*S), l the running sum.
// Per element: a max, one FMA, one exp2, one add (and the mask compare only
// on tiles that need it: the key-window edge, the causal diagonal); the
// O rescale runs only when some lane's max grew (exact: alpha = 1 otherwise).
// Writes the tile's P as bf16 MFMA operands (pairs of 16-key tiles).
// Does the key tile [k0, k0 + kt) need the per-element mask for a wave whose
// first query row is wq0 (wave-uniform)?
__device__ __forceinline__ bool tile_masked(int k0, int kt, int klim, bool causal, int wq0) {
  return k0 + kt > klim || (causal && k0 + kt - 1 > wq0);
}

// (split in two so that LDS reads can be issued between them: the max part
// has the cross-lane shuffles, the exp part no LDS access)
// (a masked tile is scaled while masking -- masked logits -inf, the others
// c*S -- so that c = 0, the zero logit scale of a kv_len = 0 row, never meets
// an infinity in a product; unmasked tiles keep raw logits and fold c into
// the exp's FMA)
// (KPERM: the e4m3 kernel's key order, accumulator (t, g, r) = key
// 32 (t >> 1) + 8 g + 4 (t & 1) + r -- see attn_fwd_fp8_kernel)
template <int NT16, int DT, bool KPERM = false>
__device__ __forceinline__ void softmax_max(f32x4 (&s)[NT16], float& m, float& l, f32x4 (&oacc)[DT],
                                            bool masked, int k0, int klim, bool causal, int qrow,
                                            int g, float c) {
  if (masked) {
    // key = lane base + a constant per (t, r): valid iff the constant <= the
    // lane's limit (last valid key, the causal diagonal) minus the base --
    // one compare against an inline constant per element
    const int kb = k0 + (KPERM ? 8 * g : 4 * g);
    const int lim = (causal ? min(klim - 1, qrow) : klim - 1) - kb;
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int off = KPERM ? 32 * (t >> 1) + 4 * (t & 1) + r : 16 * t + r;
        s[t][r] = off <= lim ? s[t][r] * c : -INFINITY;
      }
  }
  // (asm max3 chain: no canonicalising moves on the MFMA results)
  float tmax = vmax3(s[0][0], s[0][1], s[0][2]);
  tmax = vmax(tmax, s[0][3]);
#pragma unroll
  for (int t = 1; t < NT16; ++t) {
    tmax = vmax3(tmax, s[t][0], s[t][1]);
    tmax = vmax3(tmax, s[t][2], s[t][3]);
  }
  tmax = rows_max(tmax);
  const float mn = vmax(m, masked ? tmax : tmax * c);
  if (__ballot(mn > m)) {  // wave-uniform: rescale only when a row max grew
    const float alpha = fast_exp2(m - mn);  // m = -inf (nothing yet): 0, and O, l are 0
#pragma unroll
    for (int i = 0; i < DT; ++i) oacc[i] *= alpha;
    l *= alpha;
    m = mn;
  }
}
// cs: c for a raw (unmasked) tile, 1 for a masked (already scaled) one
template <int NT16>
__device__ __forceinline__ void softmax_exp(f32x4 (&s)[NT16], float m, float& l,
                                            short8_t (&pf)[NT16 / 2], float cs) {
  const float nm = m == -INFINITY ? 0.f : -m;  // all masked so far: exp2(-inf) = 0, no NaN
  float rs = 0.f;
#pragma unroll
  for (int t = 0; t < NT16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = fast_exp2(fmaf(s[t][r], cs, nm));
      s[t][r] = p;
      rs += p;
    }
  l += rs;
#pragma unroll
  for (int s2 = 0; s2 < NT16 / 2; ++s2)
    pf[s2] = pack8(s[2 * s2], s[2 * s2 + 1]);
}
template <int NT16, int DT>
__device__ __forceinline__ void softmax_tile(f32x4 (&s)[NT16], float& m, float& l,
                                             f32x4 (&oacc)[DT], short8_t (&pf)[NT16 / 2],
                                             bool masked, int k0, int klim, bool causal, int qrow,
                                             int g, float c) {
  softmax_max<NT16, DT>(s, m, l, oacc, masked, k0, klim, causal, qrow, g, c);
  softmax_exp<NT16>(s, m, l, pf, masked ? 1.f : c);
}

// ============================================================================ conventions shared by the kernels
// Value conventions are functions. The steps with a loop over outputs, a
// branch or a store are statement macros (TDG_*; the P / dS recompute ones in
// attn_bwd.h): as an inlined function such a step is optimised on its own
// before it is inlined, and that changed the generated code of most kernels.

// Forward tail conventions of a query row with softmax denominator l (the
// rows_sum over the lane groups) and running max m, both in the log2 domain:
// O = oacc * softmax_inv(l), lse = softmax_lse(m, l). A row with no key at
// all (l == 0: Lk == 0) gets O = 0 and lse = +inf, which makes the backward's
// recomputed P = exp2(S c - lse) exactly 0.
__device__ __forceinline__ float softmax_inv(float l) { return l > 0.f ? 1.f / l : 0.f; }
__device__ __forceinline__ float softmax_lse(float m, float l) {
  return l > 0.f ? m + log2f(l) : INFINITY;
}

// One row of a 16x16-MFMA output, acc * scale as bf16 (every lane of the wave
// must run it: store_row16's swaps; ok masks the lane's row)
#define TDG_PACK_STORE_ROW(DT_, lo, hi, rowp, acc, scale, g, ok)                               \
  {                                                                                            \
    _Pragma("unroll") for (int dt_ = 0; dt_ < DT_; ++dt_)                                      \
        pack_acc((acc)[dt_], scale, lo[dt_], hi[dt_]); /* columns 16dt + 4g + r */             \
    store_row16<DT_>(rowp, lo, hi, g, ok);                                                     \
  }
#define TDG_STORE_ROW(DT_, rowp, acc, scale, g, ok)                                            \
  {                                                                                            \
    bf16_t* rowp_ = rowp;                                                                      \
    uint32_t lo_[DT_], hi_[DT_];                                                               \
    TDG_PACK_STORE_ROW(DT_, lo_, hi_, rowp_, acc, scale, g, ok)                                \
  }
// Gradient row `row` of head h of a [B, L, H, hd] tensor (rows >= nrows masked)
#define TDG_STORE_GRAD_ROW(DT_, base, sb, sl, sh, b, h, row, nrows, acc, scale, g)             \
  TDG_STORE_ROW(DT_, (base) + (b) * (sb) + (long long)(row) * (sl) + (h) * (sh), acc, scale, g, \
                (row) < (nrows))
// The forward tail of query row qrow: normalise, store the output row and lse
#define TDG_FWD_FINISH(DT_, a, b, h, qrow, oacc, m, l, g)                                      \
  {                                                                                            \
    float lu_ = l;                                                                             \
    lu_ = rows_sum(lu_);                                                                       \
    const bool ok_ = (qrow) < (a).Lq;                                                          \
    const float inv_ = softmax_inv(lu_);                                                       \
    bf16_t* op_ = (a).out + (b) * (a).o_sb + (long long)(qrow) * (a).o_sl + (h) * (a).o_sh;    \
    TDG_STORE_ROW(DT_, op_, oacc, inv_, g, ok_)                                                \
    if (ok_ && (g) == 0)                                                                       \
      (a).lse[((long long)(b) * (a).H + (h)) * (a).Lq + (qrow)] = softmax_lse(m, lu_);         \
  }

// The KS register fragments of one head row (or of two rows, interleaved): rowp
// is a clamped, always-valid row, the fragments zero where !valid
#define TDG_LOAD_ROW_FRAGS(HD_, lane, valid, f, rowp) \
  _Pragma("unroll") for (int s_ = 0; s_ < ATile<HD_>::KS; ++s_) (f)[s_] = gfrag<HD_>(rowp, valid, s_, lane);
#define TDG_LOAD_ROW_FRAGS2(HD_, lane, valid, f1, rowp1, f2, rowp2)    \
  _Pragma("unroll") for (int s_ = 0; s_ < ATile<HD_>::KS; ++s_) {      \
    (f1)[s_] = gfrag<HD_>(rowp1, valid, s_, lane);                     \
    (f2)[s_] = gfrag<HD_>(rowp2, valid, s_, lane);                     \
  }

// delta = rowsum(dO * O) of the lane's query row from its dO and O fragments
// (the 4 lane groups g hold disjoint head-dim slices)
template <int KS>
__device__ __forceinline__ float row_delta(const short8_t (&of)[KS], const short8_t (&ov)[KS]) {
  float d = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) d += bf2f((bf16_t)of[s][e]) * bf2f((bf16_t)ov[s][e]);
  return rows_sum(d);
}

// The launch about to be made, for tdg_attn_last_plan (tdg_api.h): kernel
// family, head dim, workgroups and threads per workgroup of the (first)
// launch, workgroups of the second launch (the split / pipelined backward's
// dK/dV kernel; 0 otherwise). One thread-local record, written by the
// launcher that launches: nothing here predicts a dispatch. Host only.
enum AttnPlanFamily : int {
  ATTN_FWD64 = 0,     // attn_fwd_kernel<HD, 4, 64, 1>
  ATTN_FWD128 = 1,    // attn_fwd_kernel<HD, 4, 128, 2>
  ATTN_FWD128W8 = 2,  // attn_fwd_kernel<128, 8, 128, 1>
  ATTN_FWD_PIPE = 3,
  ATTN_PROBS = 4,
  ATTN_BWD_FUSED = 5,
  ATTN_BWD_FDO = 6,
  ATTN_BWD_SPLIT = 7,
  ATTN_BWD_PIPE = 8,
  ATTN_QKV_SELF = 9,
  ATTN_QKV_CROSS = 10,
};
inline int* attn_plan_slot() {
  static thread_local int plan[5] = {-1, 0, 0, 0, 0};
  return plan;
}
inline void attn_plan_record(int family, int hd, long long wgs, int threads, long long wgs2 = 0) {
  int* p = attn_plan_slot();
  p[0] = family; p[1] = hd; p[2] = (int)wgs; p[3] = threads; p[4] = (int)wgs2;
}

}  // namespace tdg

// (big_lds<Kernel>(): tdg_common.h)

#define TDG_HD_CASES(F, ...)           \
  switch (hd) {                        \
    case 16: return F<16>(__VA_ARGS__);   \
    case 32: return F<32>(__VA_ARGS__);   \
    case 64: return F<64>(__VA_ARGS__);   \
    case 128: return F<128>(__VA_ARGS__); \
    default: return -1;                \
  }
