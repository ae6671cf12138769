// Steps of the vocabulary-row kernels (xent.hip, distill.hip, decode.hip): one
// 256-thread workgroup streams one bf16 row, reduces it over its four waves in
// a fixed order and writes a few scalars or the row. One copy of each step, so
// that every kernel orders its sums and breaks its ties the same way.
//
// Straight-line value helpers are functions. A step with a loop, a branch, a
// barrier or a store is a statement macro: an inlined function is optimised on
// its own first, and as functions these steps changed the code of the kernels
// around them (docs/KERNELS.md, "Refactoring a kernel file"). The macros name
// their operands; besides those they use the kernel's `tid`, `lane` (tid & 63),
// `w` (tid >> 6), `V` and, in the register arms, `NCH`.
#pragma once
#include <type_traits>

#include "tdg_common.h"

namespace tdg {

// ---------------------------------------------------------------- values
// (m, s) <- the softmax partial of both: s = sum exp(x - m) over what was seen
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}
// (m, s) of the whole wave in every lane
__device__ __forceinline__ void wave_merge(float& m, float& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    merge(m, s, m2, s2);
  }
}

// candidate order: higher value first, equal values by the lower index. The
// relation is a macro because TDG_ARGMAX_TAKE below, written through the
// function, changed the code of all ten cross-entropy kernels.
#define TDG_BETTER(av, ai, bv, bi) ((av) > (bv) || ((av) == (bv) && (ai) < (bi)))
constexpr int NO_CAND = 0x7fffffff;
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) {
  return TDG_BETTER(av, ai, bv, bi);
}

// the four waves' values in the fixed order (r0 + r1) + (r2 + r3); `red` is
// free again on return
__device__ __forceinline__ float block_max(float v, float* red) {
  const float w = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  const float w = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// 8 bf16 of one 16-byte load -> f32, and back (round to nearest even)
__device__ __forceinline__ void unpack8(const uint4& w, float* f) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(u[i] << 16);
    f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8bf(float f0, float f1, float f2, float f3, float f4, float f5,
                                         float f6, float f7) {
  uint4 w;
  w.x = pack2bf(f0, f1);
  w.y = pack2bf(f2, f3);
  w.z = pack2bf(f4, f5);
  w.w = pack2bf(f6, f7);
  return w;
}

// the label part of a row's loss: cross entropy against (1 - s) onehot + s / V
__device__ __forceinline__ float label_loss(float lse, float xl, float sumx, int V, float smoothing) {
  return (1.f - smoothing) * (lse - xl) + smoothing * (lse - sumx / (float)V);
}

// ---------------------------------------------------------------- host: dispatch
// f(std::integral_constant<int, n>) with n clamped into [1, N]: the template
// parameter of a kernel (beam, members, chunks per thread) from a run-time count
template <int N, class F>
void dispatch_upto(int n, F f) {
  if constexpr (N > 1) {
    if (n < N) return dispatch_upto<N - 1>(n, f);
  }
  f(std::integral_constant<int, N>{});
}
// f(LabT()) for int or long long labels
template <class F>
void dispatch_labels(int lab64, F f) {
  if (lab64)
    f((long long)0);
  else
    f((int)0);
}

}  // namespace tdg

// ---------------------------------------------------------------- arg-best
// (bv, bi) <- the better of the two candidates
#define TDG_ARGMAX_TAKE(bv, bi, bv2, bi2) \
  if (TDG_BETTER(bv2, bi2, bv, bi)) { (bv) = (bv2); (bi) = (bi2); }

// The workgroup's best candidate: every wave's, through LDS, past the barrier;
// then TDG_ARGBEST_FOLD takes waves 1..3 into (bv, bi), which holds wave 0's.
#define TDG_ARGBEST_WAVES(bv, bi, red, redi)   \
  _Pragma("unroll")                            \
  for (int o = 1; o < 64; o <<= 1) {           \
    const float ov = __shfl_xor(bv, o);        \
    const int oi = __shfl_xor(bi, o);          \
    if (better(ov, oi, bv, bi)) {              \
      bv = ov;                                 \
      bi = oi;                                 \
    }                                          \
  }                                            \
  if ((tid & 63) == 0) {                       \
    red[tid >> 6] = bv;                        \
    redi[tid >> 6] = bi;                       \
  }                                            \
  __syncthreads();
#define TDG_ARGBEST_FOLD(bv, bi, red, redi)     \
  _Pragma("unroll")                             \
  for (int wv = 1; wv < 4; ++wv)                \
    if (better(red[wv], redi[wv], bv, bi)) {    \
      bv = red[wv];                             \
      bi = redi[wv];                            \
    }

// ---------------------------------------------------------------- register arms
// A padded row of nch = ldl / 8 chunks of 8 columns, NCH per thread: chunk
// tid + 256 k, once into raw[k] (short8_t).
#define TDG_REG_LOAD(raw, x, nch)                                          \
  _Pragma("unroll")                                                        \
  for (int k = 0; k < NCH; ++k) {                                          \
    const int ch = tid + 256 * k;                                          \
    if (ch < nch) raw[k] = *reinterpret_cast<const short8_t*>(x + 8 * ch); \
  }
// Every column c0 + e < V of raw, ascending: the statements see its value `v`.
#define TDG_REG_COLUMNS(raw, ...)                     \
  _Pragma("unroll")                                   \
  for (int k = 0; k < NCH; ++k) {                     \
    const int c0 = 8 * (tid + 256 * k);               \
    _Pragma("unroll")                                 \
    for (int e = 0; e < 8; ++e)                       \
      if (c0 + e < V) {                               \
        const float v = bf2f((bf16_t)(raw)[k][e]);    \
        __VA_ARGS__                                   \
      }                                               \
  }
// m, bi, sumx (-inf, NO_CAND, 0 on entry) <- the row's max, its first index
// and the sum of the logits, in every thread; r_m, r_i, r_x: 4 LDS words each.
#define TDG_REG_MAX_SUMX(raw, m, bi, sumx, r_m, r_i, r_x)        \
  TDG_REG_COLUMNS(raw, sumx += v;                                \
                  if (v > m) { m = v; bi = c0 + e; })            \
  _Pragma("unroll")                                              \
  for (int o = 32; o > 0; o >>= 1) {                             \
    const float m2 = __shfl_xor(m, o, 64);                       \
    const int i2 = __shfl_xor(bi, o, 64);                        \
    TDG_ARGMAX_TAKE(m, bi, m2, i2)                               \
    sumx += __shfl_xor(sumx, o, 64);                             \
  }                                                              \
  if (lane == 0) { r_m[w] = m; r_i[w] = bi; r_x[w] = sumx; }     \
  __syncthreads();                                               \
  m = r_m[0]; bi = r_i[0]; sumx = r_x[0];                        \
  _Pragma("unroll")                                              \
  for (int k = 1; k < 4; ++k) {                                  \
    TDG_ARGMAX_TAKE(m, bi, r_m[k], r_i[k])                       \
    sumx += r_x[k];                                              \
  }

// The row's gradient, 16 bytes per chunk through wt (WtBuf): GRAD, which sees
// the column c and its logit v, where c < V on a row with a label; else 0.
#define TDG_REG_STORE_GRAD(raw, x, nch, wt, valid, GRAD)                  \
  _Pragma("unroll")                                                       \
  for (int k = 0; k < NCH; ++k) {                                         \
    const int ch = tid + 256 * k;                                         \
    if (ch >= nch) continue;                                              \
    const int c0 = 8 * ch;                                                \
    short8_t g;                                                           \
    _Pragma("unroll")                                                     \
    for (int e = 0; e < 8; ++e) {                                         \
      const int c = c0 + e;                                               \
      float gv = 0.f;                                                     \
      if (c < V && valid) {                                               \
        const float v = bf2f((bf16_t)raw[k][e]);                          \
        gv = GRAD;                                                        \
      }                                                                   \
      g[e] = pack_bf(gv);                                                 \
    }                                                                     \
    wt.st16(x + c0, g);                                                   \
  }

// ---------------------------------------------------------------- generic arms
// The online statistics of a row, (m, s) the softmax partial, (bv, bi) the
// first max, sumx the sum: over the wave, then (past the caller's barrier,
// lane 0 of wave w having stored sm[w] ..) over the four waves.
#define TDG_ROW_WAVE_REDUCE(m, s, bv, bi, sumx)                            \
  _Pragma("unroll")                                                        \
  for (int o = 32; o > 0; o >>= 1) {                                       \
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);      \
    merge(m, s, m2, s2);                                                   \
    sumx += __shfl_xor(sumx, o, 64);                                       \
    const float bv2 = __shfl_xor(bv, o, 64);                               \
    const int bi2 = __shfl_xor(bi, o, 64);                                 \
    TDG_ARGMAX_TAKE(bv, bi, bv2, bi2)                                      \
  }
#define TDG_ROW_BLOCK_FOLD(m, s, bv, bi, sumx, sm, ss, sv, si, sx)         \
  m = sm[0]; s = ss[0]; bv = sv[0]; bi = si[0]; sumx = sx[0];              \
  _Pragma("unroll")                                                        \
  for (int k = 1; k < 4; ++k) {                                            \
    merge(m, s, sm[k], ss[k]);                                             \
    sumx += sx[k];                                                         \
    TDG_ARGMAX_TAKE(bv, bi, sv[k], si[k])                                  \
  }

// ---------------------------------------------------------------- mixture
// am[m][i] <- x_m[c + i] + off[m], the log of member m's weighted probability
// of column c + i; -inf for padding and for a logit of probability 0
#define TDG_MIX_LOAD(am, x, off, c)                                                        \
  _Pragma("unroll")                                                                        \
  for (int m = 0; m < M; ++m) {                                                            \
    unpack8(*reinterpret_cast<const uint4*>(x[m] + c), am[m]);                             \
    _Pragma("unroll")                                                                      \
    for (int i = 0; i < 8; ++i)                                                            \
      am[m][i] = (c + i < V && am[m][i] > -INFINITY) ? am[m][i] + off[m] : -INFINITY;      \
  }
