// Word alignment from cross-attention: the head-mean attention distribution
//
//   A[i, j] = (1 / H) sum_h softmax_j(scale q_h[i] . k_h[j])     (j < kv_len[b])
//
// of every query row, its arg-max over a narrowed key range and, on request,
// the distribution itself -- one launch, bf16 operands, nothing of size
// B H Lq Lk in memory (attn_probs + mean + max in torch writes and re-reads
// that tensor three times).
//
// Why two passes. A flash kernel may rescale its running output when a row
// max grows because the output is a sum over keys of ONE head. Here the
// accumulator is a sum over HEADS of normalised probabilities: exp2(S - m_h) /
// l_h needs the final (m_h, l_h) of head h before the first key can be added,
// and those differ from head to head, so there is no common factor to fix up
// afterwards. Pass 1 finds (m_h, l_h) of every head, pass 2 recomputes S (the
// same MFMAs on the same operands: bitwise the same logits, so every exponent
// is <= 0) and accumulates.
//
// Work split. One workgroup of 4 waves per (batch element, 16-query tile), in
// the XCD-grouped batch order of the other attention kernels. The waves split
// the 16-key blocks, block kb to wave kb mod 4, not the heads: a wave's
// accumulators then cover disjoint keys, all heads add into the same
// registers in ascending order, and no cross-wave sum of A exists at all.
// S^T = K Q^T on v_mfma_f32_16x16x32_bf16 (hd 16: the upper half of the
// 32-deep step is zero, as in the forward kernel), so lane (g, cl) owns query
// row cl and keys 4 g .. 4 g + 3 of each of its blocks: NKB blocks x f32x4 per
// wave, NKB = Lk / 64 rounded up to a power of two (64 VGPRs at Lk 1024; the
// kernel is instantiated per NKB so that they are registers).
//
// Data movement. Q of the 16 rows, all heads, is staged once in LDS (16 H hd
// bf16, chunk-swizzled) and read as B operands by both passes. K goes from
// global memory straight into the A-operand registers (a lane's 16 bytes are
// contiguous in a key row); no wave shares a key block with another, so LDS
// would buy nothing within a pass. K is therefore read TWICE FROM L2, once per
// pass: a batch element's K (Lk H hd bf16, 1 MB at 1024 x 8 x 64) does not fit
// in LDS at the long end, where the second read costs most, and at the short
// end it is a few tens of KB that stay in L2 between the passes. The blocks
// are taken four at a time: 4 KS loads in flight per lane before the first
// MFMA, and groups past kv_len are skipped (wave-uniform).
//
// Reductions, all in a fixed order (no atomics; bitwise reproducible):
//   pass 1: per lane max / sum over its keys, the four lane groups by
//           permlane swaps, the four waves' (m, l)[16] per head through LDS,
//           combined in wave order by every wave alike;
//   arg-max: per lane over ascending keys (strict >), then the 16 (wave, lane
//           group) candidates of a row through LDS by value, then lower index.
// soft rows leave as one 16-byte store per lane and block.
#include "attn_impl.h"

namespace tdg {

constexpr int ALIGN_MAX_NKB = 16;  // key blocks per wave: Lk <= 64 * 16

// LDS: Q image | (m, l) partials [H][4 waves][16 rows] | arg-max [4][4][16]
__host__ __device__ inline int align_q_bytes(int H, int hd) { return 16 * H * hd * 2; }
__host__ __device__ inline int align_lds_bytes(int H, int hd) {
  return align_q_bytes(H, hd) + H * 4 * 16 * 8 + 4 * 4 * 16 * 8;
}

template <int HD, int NKB>
__global__ __launch_bounds__(256) void attn_align_kernel(AttnAlignArgs a) {
  using T = ATile<HD>;
  constexpr int CPR = HD / 8;              // 16-byte chunks per head row
  constexpr int GRP = NKB < 4 ? NKB : 4;   // key blocks per load group
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, cl = lane & 15;
  const int nqt = cdiv(a.Lq, 16);
  int t = blockIdx.x;
  if (a.xcd) t = xcd_remap(t, gridDim.x);
  const int b = t / nqt, q0 = (t % nqt) * 16;
  const int H = a.H;
  const int klim = min(max(a.kv_len[b], 0), a.Lk);
  const int nq = a.q_len ? min(max(a.q_len[b], 0), a.Lq) : a.Lq;
  const int row = q0 + cl;

  char* ldsQ = smem;
  float2* ldsML = reinterpret_cast<float2*>(smem + align_q_bytes(H, HD));
  int2* ldsBest = reinterpret_cast<int2*>(ldsML + H * 64);

  f32x4 acc[NKB];
  TDG_ZERO1(NKB, acc)

  // (b only and the tile: uniform over the workgroup, so are the barriers inside)
  if (klim > 0 && q0 < nq) {
    // ---- Q of the tile's rows, every head: chunk c of (head, row) at c ^ (row mod CPR)
    const bf16_t* qb = a.q + b * a.q_sb;
    for (int id = tid; id < 16 * H * CPR; id += 256) {
      const int c = id % CPR, h = (id / CPR) % H, r = id / (CPR * H);
      const int qr = q0 + r;
      const short8_t v = ld8_or0(qb + (long long)min(qr, a.Lq - 1) * a.q_sl + h * a.q_sh + c * 8, qr < a.Lq);
      *reinterpret_cast<short8_t*>(ldsQ + (h * 16 + r) * (HD * 2) + ((c ^ (r & (CPR - 1))) << 4)) = v;
    }
    __syncthreads();

    const float c2 = a.scale * LOG2E;
    const bf16_t* kb = a.k + b * a.k_sb;
    // S of the wave's blocks i0 .. i0 + GRP - 1 for head h, scaled to the log2
    // domain, keys >= klim at -inf: x[j][r] = key 16 (w + 4 (i0 + j)) + 4 g + r
    auto logits = [&](int h, int i0, const short8_t (&qf)[T::KS], f32x4 (&x)[GRP]) {
      short8_t kf[GRP][T::KS];
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        const int key = 16 * (w + 4 * (i0 + j)) + cl;
        const bf16_t* kp = kb + (long long)min(key, klim - 1) * a.k_sl + h * a.k_sh;
        TDG_LOAD_ROW_FRAGS(HD, lane, key < klim, kf[j], kp)
      }
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) s = mfma16(kf[j][ks], qf[ks], s);
        const int lim = klim - (16 * (w + 4 * (i0 + j)) + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[j][r] = r < lim ? s[r] * c2 : -INFINITY;
      }
    };
    auto q_frags = [&](int h, short8_t (&qf)[T::KS]) {
#pragma unroll
      for (int ks = 0; ks < T::KS; ++ks) {
        const int c = 4 * ks + g;
        const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
        const short8_t v = *reinterpret_cast<const short8_t*>(
            ldsQ + (h * 16 + cl) * (HD * 2) + (((c & (CPR - 1)) ^ (cl & (CPR - 1))) << 4));
        qf[ks] = c < CPR ? v : z;
      }
    };

    // ---- pass 1: (m, l) of the wave's keys, per head and row
    for (int h = 0; h < H; ++h) {
      short8_t qf[T::KS];
      q_frags(h, qf);
      f32x4 x[NKB];
#pragma unroll
      for (int i = 0; i < NKB; ++i) x[i] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int i0 = 0; i0 < NKB; i0 += GRP) {
        if (16 * (w + 4 * i0) >= klim) break;
        f32x4 xg[GRP];
        logits(h, i0, qf, xg);
#pragma unroll
        for (int j = 0; j < GRP; ++j) x[i0 + j] = xg[j];
      }
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < NKB; ++i) m = fmaxf(fmaxf(m, fmaxf(x[i][0], x[i][1])), fmaxf(x[i][2], x[i][3]));
      m = rows_max(m);
      const float nm = m == -INFINITY ? 0.f : m;  // (a wave with no key: l = 0, no NaN)
      float l = 0.f;
#pragma unroll
      for (int i = 0; i < NKB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) l += fast_exp2(x[i][r] - nm);
      l = rows_sum(l);
      if (g == 0) ldsML[(h * 4 + w) * 16 + cl] = make_float2(m, l);
    }
    __syncthreads();

    // ---- pass 2: heads in ascending order into the wave's accumulators
    const float invH = 1.f / (float)H;
    for (int h = 0; h < H; ++h) {
      float2 ml[4];
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) ml[ww] = ldsML[(h * 4 + ww) * 16 + cl];
      const float m = fmaxf(fmaxf(ml[0].x, ml[1].x), fmaxf(ml[2].x, ml[3].x));  // finite: klim > 0
      float l = 0.f;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) l += ml[ww].y * fast_exp2(ml[ww].x - m);
      const float rinv = invH / l;  // l >= 1: the row max contributes exp2(0)
      short8_t qf[T::KS];
      q_frags(h, qf);
#pragma unroll
      for (int i0 = 0; i0 < NKB; i0 += GRP) {
        if (16 * (w + 4 * i0) >= klim) break;
        f32x4 xg[GRP];
        logits(h, i0, qf, xg);
#pragma unroll
        for (int j = 0; j < GRP; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i0 + j][r] += fast_exp2(xg[j][r] - m) * rinv;
      }
    }
  }

  // ---- outputs. Rows at or beyond q_len: zeros / -1 (acc is 0 when the tile
  // was skipped; a live tile's rows past nq are zeroed here)
  const bool rowok = row < nq;
  if (!rowok) TDG_ZERO1(NKB, acc)
  float best = -1.f;  // A >= 0: the first key in range always wins over this
  int bidx = -1;
  const int lo = a.k_lo, hi = klim - a.k_trim;
  if (rowok) {
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * (w + 4 * i) + 4 * g + r;  // ascending in (i, r)
        if (key >= lo && key < hi && acc[i][r] > best) {
          best = acc[i][r];
          bidx = key;
        }
      }
  }
  ldsBest[(w * 4 + g) * 16 + cl] = make_int2(__float_as_int(best), bidx);
  if (a.soft && row < a.Lq) {
    float* sp = a.soft + ((long long)b * a.Lq + row) * a.ldk;
#pragma unroll
    for (int i = 0; i < NKB; ++i) {
      const int key0 = 16 * (w + 4 * i) + 4 * g;  // a multiple of 4, ldk of 8: whole or none
      if (key0 < a.ldk) *reinterpret_cast<f32x4*>(sp + key0) = acc[i];
    }
  }
  __syncthreads();
  if (tid < 16 && q0 + tid < a.Lq) {
    float bv = -1.f;
    int bi = -1;
    for (int c = 0; c < 16; ++c) {
      const int2 e = ldsBest[c * 16 + tid];
      const float ev = __int_as_float(e.x);
      if (ev > bv || (ev == bv && e.y < bi)) {
        bv = ev;
        bi = e.y;
      }
    }
    const long long o = (long long)b * a.Lq + q0 + tid;
    a.hard[o] = bi;
    a.conf[o] = bi >= 0 ? bv : 0.f;
  }
}

}  // namespace tdg

using namespace tdg;

namespace {
template <int HD, int NKB>
int align_launch(const AttnAlignArgs& a, hipStream_t st) {
  const long long wgs = (long long)a.B * cdiv(a.Lq, 16);
  hipLaunchKernelGGL((attn_align_kernel<HD, NKB>), dim3((unsigned)wgs), dim3(256),
                     align_lds_bytes(a.H, HD), st, a);
  return 0;
}
template <int HD>
int align_hd(const AttnAlignArgs& a, hipStream_t st) {
  const int nkb = cdiv(a.Lk, 64);
  if (nkb <= 1) return align_launch<HD, 1>(a, st);
  if (nkb <= 2) return align_launch<HD, 2>(a, st);
  if (nkb <= 4) return align_launch<HD, 4>(a, st);
  if (nkb <= 8) return align_launch<HD, 8>(a, st);
  return align_launch<HD, 16>(a, st);
}
}  // namespace

// -1: hd not in {16, 32, 64, 128}; -2: Lk > 1024 (the accumulators of a row
// are registers); -3: the Q image of a tile over 64 KiB of LDS, or more
// workgroups than a grid holds; nothing launched. (No attn_plan_record: the
// record's families are the forward / backward kernels'.)
extern "C" int tdg_attn_align(const AttnAlignArgs* a, int hd, hipStream_t st) {
  if (a->B <= 0 || a->Lq <= 0 || a->Lk <= 0 || a->H <= 0) return 0;
  if (a->Lk > 64 * ALIGN_MAX_NKB) return -2;
  if (align_lds_bytes(a->H, hd) > 64 * 1024 || (long long)a->B * cdiv(a->Lq, 16) > 0x7fffffffLL) return -3;
  TDG_HD_CASES(align_hd, *a, st)
}
