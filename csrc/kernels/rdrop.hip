// R-Drop consistency loss (Liang et al., NeurIPS 2021, "R-Drop: Regularized
// Dropout for Neural Networks"), forward and backward in one launch over both
// copies' logits (gfx950).
//
// The batch of B pairs is duplicated to 2B rows, copy 2 after copy 1, and runs
// through one ordinary forward. M is the number of label positions of one copy
// (B x T). Logits row i (copy 1) and row i + M (copy 2) form a pair with the
// same label y. With xa, xb the pair's bf16 logits over the first V columns,
// p = softmax(xa), r = softmax(xb), s the label smoothing, ntok the label count
// of the doubled batch and workers as in tdg_xent:
//   row_label[a] = (1 - s)(lse_a - xa[y]) + s (lse_a - mean xa)     (tdg_xent's row_loss; same for b)
//   d[v]         = (xa[v] - lse_a) - (xb[v] - lse_b)                 (= log p - log r)
//   KLab = sum_v p[v] d[v]          KLba = -sum_v r[v] d[v]
//   row_loss[a]  = row_label[a] + (alpha / 2) KLab
//   row_loss[b]  = row_label[b] + (alpha / 2) KLba
//   row_correct[.] = first-index argmax of the row == y               (each copy on its own)
//   dlogits[a] = ( p - target  +  (alpha / 2) ( p (d - KLab) + p - r ) ) / (max(ntok, 1) workers)
//   dlogits[b] = ( r - target  +  (alpha / 2) ( r (-d - KLba) + r - p ) ) / (max(ntok, 1) workers)
//   target     = (1 - s) onehot(y) + s / V
// Summed and divided by ntok * workers this is the paper's objective, NLL_1 +
// NLL_2 + (alpha / 2)(KL(p||r) + KL(r||p)) per token. The gradient is written
// in place over both rows, in bf16; the columns [V, ldl) are written as zero.
// A PAD pair (label 0) gives 0 everywhere and two zero gradient rows. Logits
// are finite: they come from the projection, a -inf column is not supported.
//
// Arithmetic. Every term is a difference of logits taken before an exp; no
// log of a rounded probability is formed:
//   d = (xa - xb) - ((max_a - max_b) + (log S_a - log S_b)),  S = sum exp(x - max)
//   p = exp(xa - max_a) / S_a,  r likewise
// (xa - xb) and (x - max) are differences of two bf16 values. Both rows go
// through the same statements in the same order; S is a sum of exponentials
// with no product in it and p a rounded product (__fmul_rn), so that no
// contraction into a fused multiply-add, which the compiler may choose for
// one row and not for the other, reaches them. A pair whose rows are
// bitwise equal has max, S and every p equal to the other row's: d is exactly
// 0, both KL sums are exactly 0, p - r is exactly 0 and the two gradient rows
// are the plain cross-entropy gradient, bit for bit the same.
//
// Design. One 256-thread workgroup per pair; a PAD pair leaves before it loads
// anything (in a padded batch that is a large share of the rows). The steps
// are tdg_vocab_row.h's (chunk loads, first-index argmax, fixed-order four-wave
// folds, label_loss, write-through stores), so sums and ties are ordered as in
// xent.hip and distill.hip; the pairing is this file's.
//   Register arm (ldl % 8 == 0, ldl <= 8192, 16-byte aligned rows): thread t
//   holds chunk t + 256 k of BOTH rows, 2 x NCH short8_t, loaded once. There is
//   no f32 copy of a row and no row in LDS. Three rounds, each reducing both
//   rows behind ONE barrier (a row's four partials are 16 bytes of LDS, each
//   round has its own slots, so no barrier guards a reuse):
//     1. max, first argmax, sum of logits of a and b;
//     2. e = exp(x - max), kept in registers (2 x 8 NCH f32), and S_a, S_b;
//     3. p = e / S over e, and the two KL sums, which need both S.
//   The gradient then comes from the registers: 2 exp per column pair in all
//   (xent_reg_kernel spends 4 on two rows), each logit read once and written
//   once, 3 barriers per pair, 160 bytes of LDS.
//   Generic arm (V up to 65536, any stride, any 2-byte alignment): the same
//   rounds streamed over the L2-resident rows, each row read four times (max,
//   sum, KL, gradient); 3 barriers per pair.
// No atomics; a pair's result does not depend on the grid.
#include <cmath>

#include "tdg_api.h"
#include "tdg_common.h"
#include "tdg_vocab_row.h"

namespace tdg {

// Every column c0 + e < V of the pair's chunks, ascending: the statements see
// the two logits `va`, `vb` (ra, rb: the kernel's short8_t chunks).
#define RDROP_PAIR_COLUMNS(...)                          \
  _Pragma("unroll")                                      \
  for (int k = 0; k < NCH; ++k) {                        \
    const int c0 = 8 * (tid + 256 * k);                  \
    _Pragma("unroll")                                    \
    for (int e = 0; e < 8; ++e)                          \
      if (c0 + e < V) {                                  \
        const float va = bf2f((bf16_t)ra[k][e]);         \
        const float vb = bf2f((bf16_t)rb[k][e]);         \
        __VA_ARGS__                                      \
      }                                                  \
  }
// (m, bi, sumx) over the wave, as TDG_REG_MAX_SUMX reduces them
#define RDROP_WAVE_MAX_SUMX(m, bi, sumx)                 \
  _Pragma("unroll")                                      \
  for (int o = 32; o > 0; o >>= 1) {                     \
    const float m2 = __shfl_xor(m, o, 64);               \
    const int i2 = __shfl_xor(bi, o, 64);                \
    TDG_ARGMAX_TAKE(m, bi, m2, i2)                       \
    sumx += __shfl_xor(sumx, o, 64);                     \
  }
// ... and over the four waves' slots
#define RDROP_FOLD_MAX_SUMX(m, bi, sumx, rm, ri, rx)     \
  m = rm[0]; bi = ri[0]; sumx = rx[0];                   \
  _Pragma("unroll")                                      \
  for (int k = 1; k < 4; ++k) {                          \
    TDG_ARGMAX_TAKE(m, bi, rm[k], ri[k])                 \
    sumx += rx[k];                                       \
  }
// The per-row outputs of a pair (thread 0) from the reduced statistics.
__device__ __forceinline__ void rdrop_outputs(const RdropArgs& a, int pair, int lab, float lsea,
                                              float lseb, float xla, float xlb, float sxa, float sxb,
                                              int ia, int ib, float klab, float klba) {
  const float ha = 0.5f * a.alpha;
  const float la = label_loss(lsea, xla, sxa, a.V, a.smoothing);
  const float lb = label_loss(lseb, xlb, sxb, a.V, a.smoothing);
  const int ra = pair, rb = pair + a.M;
  a.row_loss[ra] = la + ha * klab;
  a.row_loss[rb] = lb + ha * klba;
  if (a.row_label) {
    a.row_label[ra] = la;
    a.row_label[rb] = lb;
  }
  a.row_correct[ra] = ia == lab ? 1.f : 0.f;
  a.row_correct[rb] = ib == lab ? 1.f : 0.f;
}
__device__ __forceinline__ void rdrop_pad_outputs(const RdropArgs& a, int pair) {
  const int ra = pair, rb = pair + a.M;
  a.row_loss[ra] = a.row_loss[rb] = 0.f;
  if (a.row_label) a.row_label[ra] = a.row_label[rb] = 0.f;
  a.row_correct[ra] = a.row_correct[rb] = 0.f;
}

// Both gradients of one column: p, r the two probabilities, d = log p - log r,
// t the label target of the column.
#define RDROP_GRADS(fa, fb, p, r, d, t)                                  \
  fa = ((p - t) + ha * (p * (d - klab) + (p - r))) * scale;              \
  fb = ((r - t) + ha * (r * (-d - klba) + (r - p))) * scale;

template <typename LabT, int NCH>
__global__ __launch_bounds__(256) void rdrop_reg_kernel(const RdropArgs a) {
  __shared__ float r_m[2][4], r_x[2][4], r_s[2][4], r_k[2][4];
  __shared__ int r_i[2][4];
  const int pair = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ldl = a.ldl, nch = ldl >> 3;
  bf16_t* xa = a.x + (size_t)pair * ldl;
  bf16_t* xb = a.x + ((size_t)pair + a.M) * ldl;
  const int lab = (int)static_cast<const LabT*>(a.labels)[pair];
  const WtBuf wt(a.x, (size_t)2 * a.M * ldl * sizeof(bf16_t));
  if (lab == 0) {  // the same in every thread of the pair
    if (tid == 0) rdrop_pad_outputs(a, pair);
    if (!a.write_grad) return;
    short8_t z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int ch = tid + 256 * k;
      if (ch >= nch) continue;
      wt.st16(xa + 8 * ch, z);
      wt.st16(xb + 8 * ch, z);
    }
    return;
  }
  short8_t ra[NCH], rb[NCH];
  TDG_REG_LOAD(ra, xa, nch)
  TDG_REG_LOAD(rb, xb, nch)
  const int li = min(max(lab, 0), V - 1);
  const float xla = bf2f(xa[li]), xlb = bf2f(xb[li]);  // read before any thread overwrites the rows

  // round 1: max + first argmax + sum of logits of both rows
  float ma = -INFINITY, mb = -INFINITY, sxa = 0.f, sxb = 0.f;
  int ia = NO_CAND, ib = NO_CAND;
  RDROP_PAIR_COLUMNS(sxa += va;
                     if (va > ma) { ma = va; ia = c0 + e; }
                     sxb += vb;
                     if (vb > mb) { mb = vb; ib = c0 + e; })
  RDROP_WAVE_MAX_SUMX(ma, ia, sxa)
  RDROP_WAVE_MAX_SUMX(mb, ib, sxb)
  if (lane == 0) {
    r_m[0][w] = ma; r_i[0][w] = ia; r_x[0][w] = sxa;
    r_m[1][w] = mb; r_i[1][w] = ib; r_x[1][w] = sxb;
  }
  __syncthreads();
  RDROP_FOLD_MAX_SUMX(ma, ia, sxa, r_m[0], r_i[0], r_x[0])
  RDROP_FOLD_MAX_SUMX(mb, ib, sxb, r_m[1], r_i[1], r_x[1])

  // round 2: e = exp(x - max) into registers, and the two sums
  float ea[NCH][8], eb[NCH][8];
  float sa = 0.f, sb = 0.f;
  RDROP_PAIR_COLUMNS(ea[k][e] = __expf(va - ma); sa += ea[k][e];
                     eb[k][e] = __expf(vb - mb); sb += eb[k][e];)
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if (lane == 0) { r_s[0][w] = sa; r_s[1][w] = sb; }
  __syncthreads();
  sa = r_s[0][0] + r_s[0][1] + r_s[0][2] + r_s[0][3];
  sb = r_s[1][0] + r_s[1][1] + r_s[1][2] + r_s[1][3];
  const float lsra = __logf(sa), lsrb = __logf(sb);
  const float dl = (ma - mb) + (lsra - lsrb);  // lse_a - lse_b
  const float inva = 1.f / sa, invb = 1.f / sb;

  // round 3: the probabilities over e, and the two KL sums
  float ka = 0.f, kb = 0.f;
  RDROP_PAIR_COLUMNS(const float d = (va - vb) - dl;
                     ea[k][e] = __fmul_rn(ea[k][e], inva); eb[k][e] = __fmul_rn(eb[k][e], invb);
                     ka += ea[k][e] * d; kb += eb[k][e] * d;)
  ka = wave_sum(ka);
  kb = wave_sum(kb);
  if (lane == 0) { r_k[0][w] = ka; r_k[1][w] = kb; }
  __syncthreads();
  const float klab = (r_k[0][0] + r_k[0][1]) + (r_k[0][2] + r_k[0][3]);
  const float klba = -((r_k[1][0] + r_k[1][1]) + (r_k[1][2] + r_k[1][3]));
  if (tid == 0)
    rdrop_outputs(a, pair, lab, ma + lsra, mb + lsrb, xla, xlb, sxa, sxb, ia, ib, klab, klba);
  if (!a.write_grad) return;

  const float scale = 1.f / (fmaxf(a.ntok[0], 1.f) * a.workers);
  const float off = a.smoothing / (float)V, hit = 1.f - a.smoothing, ha = 0.5f * a.alpha;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int ch = tid + 256 * k;
    if (ch >= nch) continue;
    const int c0 = 8 * ch;
    short8_t ga, gb;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      float fa = 0.f, fb = 0.f;
      if (c < V) {
        const float d = (bf2f((bf16_t)ra[k][e]) - bf2f((bf16_t)rb[k][e])) - dl;
        const float p = ea[k][e], r = eb[k][e];
        const float t = off + (c == lab ? hit : 0.f);
        RDROP_GRADS(fa, fb, p, r, d, t)
      }
      ga[e] = pack_bf(fa);
      gb[e] = pack_bf(fb);
    }
    wt.st16(xa + c0, ga);  // write-through: 2 x 115 MB of dlogits at Transformer-base
    wt.st16(xb + c0, gb);
  }
}

template <typename LabT>
__global__ __launch_bounds__(256) void rdrop_kernel(const RdropArgs a) {
  __shared__ float sm[2][4], ss[2][4], sx[2][4], sk[2][4];
  __shared__ int si[2][4];
  const int pair = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ldl = a.ldl;
  bf16_t* xa = a.x + (size_t)pair * ldl;
  bf16_t* xb = a.x + ((size_t)pair + a.M) * ldl;
  const int lab = (int)static_cast<const LabT*>(a.labels)[pair];
  if (lab == 0) {  // the same in every thread of the pair
    if (tid == 0) rdrop_pad_outputs(a, pair);
    if (!a.write_grad) return;
    for (int c = tid; c < ldl; c += 256) xa[c] = xb[c] = f2bf(0.f);
    return;
  }
  const int li = min(max(lab, 0), V - 1);
  const float xla = bf2f(xa[li]), xlb = bf2f(xb[li]);  // read before any thread overwrites the rows

  // phase 1: max + first argmax + sum of logits of both rows, then the two
  // sums of exp(x - max): additions only, as in the register arm (an online
  // softmax sum has products the compiler contracted for one row and not for
  // the other: equal rows then got sums one ulp apart)
  float ma = -INFINITY, mb = -INFINITY, sxa = 0.f, sxb = 0.f;
  int ia = NO_CAND, ib = NO_CAND;
  for (int c = tid; c < V; c += 256) {
    const float va = bf2f(xa[c]), vb = bf2f(xb[c]);
    sxa += va;
    if (va > ma) { ma = va; ia = c; }
    sxb += vb;
    if (vb > mb) { mb = vb; ib = c; }
  }
  RDROP_WAVE_MAX_SUMX(ma, ia, sxa)
  RDROP_WAVE_MAX_SUMX(mb, ib, sxb)
  if (lane == 0) {
    sm[0][w] = ma; si[0][w] = ia; sx[0][w] = sxa;
    sm[1][w] = mb; si[1][w] = ib; sx[1][w] = sxb;
  }
  __syncthreads();  // every read of x[lab] above is done; the partials are visible
  RDROP_FOLD_MAX_SUMX(ma, ia, sxa, sm[0], si[0], sx[0])
  RDROP_FOLD_MAX_SUMX(mb, ib, sxb, sm[1], si[1], sx[1])
  float sa = 0.f, sb = 0.f;
  for (int c = tid; c < V; c += 256) {
    sa += __expf(bf2f(xa[c]) - ma);
    sb += __expf(bf2f(xb[c]) - mb);
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if (lane == 0) { ss[0][w] = sa; ss[1][w] = sb; }
  __syncthreads();
  sa = ss[0][0] + ss[0][1] + ss[0][2] + ss[0][3];
  sb = ss[1][0] + ss[1][1] + ss[1][2] + ss[1][3];
  const float lsra = __logf(sa), lsrb = __logf(sb);
  const float dl = (ma - mb) + (lsra - lsrb);  // lse_a - lse_b
  const float inva = 1.f / sa, invb = 1.f / sb;

  // phase 2: the two KL sums
  float ka = 0.f, kb = 0.f;
  for (int c = tid; c < V; c += 256) {
    const float va = bf2f(xa[c]), vb = bf2f(xb[c]);
    const float d = (va - vb) - dl;
    ka += __fmul_rn(__expf(va - ma), inva) * d;
    kb += __fmul_rn(__expf(vb - mb), invb) * d;
  }
  ka = wave_sum(ka);
  kb = wave_sum(kb);
  if (lane == 0) { sk[0][w] = ka; sk[1][w] = kb; }
  __syncthreads();  // every read of the rows by another thread's columns is done
  const float klab = (sk[0][0] + sk[0][1]) + (sk[0][2] + sk[0][3]);
  const float klba = -((sk[1][0] + sk[1][1]) + (sk[1][2] + sk[1][3]));
  if (tid == 0)
    rdrop_outputs(a, pair, lab, ma + lsra, mb + lsrb, xla, xlb, sxa, sxb, ia, ib, klab, klba);
  if (!a.write_grad) return;

  const float scale = 1.f / (fmaxf(a.ntok[0], 1.f) * a.workers);
  const float off = a.smoothing / (float)V, hit = 1.f - a.smoothing, ha = 0.5f * a.alpha;
  for (int c = tid; c < ldl; c += 256) {  // a thread reads and writes its own columns only
    float fa = 0.f, fb = 0.f;
    if (c < V) {
      const float va = bf2f(xa[c]), vb = bf2f(xb[c]);
      const float d = (va - vb) - dl;
      const float p = __fmul_rn(__expf(va - ma), inva), r = __fmul_rn(__expf(vb - mb), invb);
      const float t = off + (c == lab ? hit : 0.f);
      RDROP_GRADS(fa, fb, p, r, d, t)
    }
    xa[c] = f2bf(fa);
    xb[c] = f2bf(fb);
  }
}

}  // namespace tdg

// The R-Drop loss of M pairs (tdg_rdrop.h RdropArgs; the formulas are at the
// head of this file). Register arm: ldl % 8 == 0, ldl <= 8192 and a 16-byte
// aligned buffer (row i + M then is aligned too); the generic arm otherwise.
// -1: V outside [1, 65536], alpha negative or not finite, M < 0; -2: a row
// shorter than V or a null operand; nothing launched. M == 0: nothing to do.
extern "C" int tdg_xent_rdrop(const tdg::RdropArgs* a, hipStream_t st) {
  if (a->V < 1 || a->V > 65536 || !(a->alpha >= 0.f) || !std::isfinite(a->alpha) || a->M < 0) return -1;
  if (a->ldl < a->V) return -2;
  if (a->M == 0) return 0;  // (empty operands may be null)
  if (!a->x || !a->labels || !a->ntok || !a->row_loss || !a->row_correct) return -2;
  const bool reg = a->ldl % 8 == 0 && a->ldl <= 256 * 8 * 4 && (reinterpret_cast<uintptr_t>(a->x) & 15) == 0;
  tdg::dispatch_labels(a->lab64, [&](auto l) {
    using LabT = decltype(l);
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(a->M), dim3(256), 0, st, *a); };
    if (reg)
      tdg::dispatch_upto<4>(tdg::cdiv(a->ldl / 8, 256),
                            [&](auto n) { launch(tdg::rdrop_reg_kernel<LabT, decltype(n)::value>); });
    else
      launch(tdg::rdrop_kernel<LabT>);
  });
  return 0;
}
