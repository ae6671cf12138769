// Clipped n-gram match counts between pairs of token rows (n = 1 .. 4): the
// count behind BLEU, and the pairwise utility of minimum-Bayes-risk selection.
//
// For rows x and y, m_n = sum over the distinct n-grams g of x of
// min(count_x(g), count_y(g)). Position by position: with r_n(i) = the number
// of earlier positions i' < i of x that hold the n-gram at i, and c_n(i) = the
// number of positions of y that hold it, the k-th occurrence of g in x (k =
// r_n + 1) is matched exactly when k <= count_y(g), so
//
//   m_n = sum_i [ r_n(i) < c_n(i) ]      over the n-grams of x (i + n <= |x|).
//
// One wave per pair. Both rows are staged in LDS (zero beyond their length:
// what lies there in memory is never read). The lanes take the positions of x
// in chunks of 64 and keep x[i .. i + 3] in registers; a loop over the
// positions j of the other row reads one new token per step from LDS at a
// wave-uniform address (a broadcast) and slides a 4-token window, so "same
// n-gram at (i, j)" is a chain of four compares AND-ed, counted per lane. The
// ranks r_n are the same loop of x against itself, restricted to j < i: either
// inside the pair kernel, or once per row in a pre-pass that stores them
// (NgramArgs::ranks) for the pair kernel to read. Integers only, no atomics,
// no in-band sentinel: validity is decided by positions, never by token values.
#include "tdg_api.h"
#include "tdg_common.h"

namespace tdg {

constexpr int NG_WAVES = 4;  // pairs (rows in the pre-pass) per workgroup

// LDS words per staged row: whole 64-position chunks plus the 3 tokens the
// last lane's window reaches past its own position
__host__ __device__ __forceinline__ int ng_row_words(int L) { return cdiv(L, WAVE) * WAVE + 4; }

__device__ __forceinline__ int ng_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int ng_len(const int* length, long long row, int L) {
  return ng_uniform(min(max(length[row], 0), L));
}

// s[0, words) = the row's first `len` tokens, then zeros
__device__ __forceinline__ void ng_stage(int* s, const int* row, int len, int words, int lane) {
  for (int k = lane; k < words; k += WAVE) s[k] = k < len ? row[k] : 0;
}

// c[n - 1] += the positions j in [j0, j1) of the staged row s whose n-gram
// equals the lane's x[0 .. n); BELOW: only those with j < i. Reads s up to
// j1 + 2: the caller keeps every n-gram it counts inside the row, or masks
// the lanes it does not (a window that runs into the zero padding).
template <bool BELOW>
__device__ __forceinline__ void ng_count(const int* s, int j0, int j1, const int (&x)[4], int i,
                                         int (&c)[4]) {
  if (j0 >= j1) return;
  int y0 = s[j0], y1 = s[j0 + 1], y2 = s[j0 + 2];
  // (the loop vectoriser would turn the per-lane counters into short vectors
  // of partial sums: ten times the code for nothing)
#pragma clang loop vectorize(disable) unroll_count(4)
  for (int j = j0; j < j1; ++j) {
    const int y3 = s[j + 3];
    bool e = x[0] == y0;
    if (BELOW) e &= j < i;
    c[0] += e;
    e &= x[1] == y1;
    c[1] += e;
    e &= x[2] == y2;
    c[2] += e;
    e &= x[3] == y3;
    c[3] += e;
    y0 = y1, y1 = y2, y2 = y3;
  }
}

// r[n - 1] = the positions j < i of the staged row sx that hold the n-gram at
// i, for the lane's position i of chunk `ch`. Every j < ch * 64 lies below
// every lane of the chunk; the chunk's own positions need the lane compare.
// An n-gram at j < i is inside the row whenever the one at i is, and the lanes
// whose own n-gram is not are masked by the caller.
__device__ __forceinline__ void ng_ranks(const int* sx, int lenx, int ch, const int (&x)[4], int i,
                                         int (&r)[4]) {
  ng_count<false>(sx, 0, ch * WAVE, x, i, r);
  ng_count<true>(sx, ch * WAVE, min(ch * WAVE + WAVE - 1, lenx), x, i, r);
}

// ranks[row, i, :] for i < length[row] (later positions are not written and
// never read); one wave per row
__global__ __launch_bounds__(NG_WAVES * WAVE) void ngram_ranks_kernel(const NgramArgs a) {
  extern __shared__ int ng_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = ng_uniform(threadIdx.x / WAVE);
  const int words = ng_row_words(a.L);
  int* sx = ng_lds + w * words;
  const long long row = (long long)blockIdx.x * NG_WAVES + w;
  const bool live = row < a.N;  // wave-uniform
  int lenx = 0;
  if (live) {
    lenx = ng_len(a.length, row, a.L);
    ng_stage(sx, a.tok + row * a.ld, lenx, words, lane);
  }
  __syncthreads();
  if (!live) return;
  for (int ch = 0; ch * WAVE < lenx; ++ch) {
    const int i = ch * WAVE + lane;
    const int x[4] = {sx[i], sx[i + 1], sx[i + 2], sx[i + 3]};
    int r[4] = {0, 0, 0, 0};
    ng_ranks(sx, lenx, ch, x, i, r);
    if (i < lenx) {
      const short4_t v = {(short)r[0], (short)r[1], (short)r[2], (short)r[3]};
      *reinterpret_cast<short4_t*>(a.ranks + (row * a.L + i) * 4) = v;
    }
  }
}

// PRE: the ranks of x come from the pre-pass
template <bool PRE>
__global__ __launch_bounds__(NG_WAVES * WAVE) void ngram_matches_kernel(const NgramArgs a) {
  extern __shared__ int ng_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = ng_uniform(threadIdx.x / WAVE);
  const int words = ng_row_words(a.L);
  int* sx = ng_lds + (2 * w) * words;
  int* sy = sx + words;
  const long long p = (long long)blockIdx.x * NG_WAVES + w;
  // every branch below is wave-uniform
  const bool live = p < a.P;
  int ra = -1, rb = -1;
  if (live) ra = ng_uniform(a.pair_a[p]), rb = ng_uniform(a.pair_b[p]);
  const bool ok = ra >= 0 && ra < a.N && rb >= 0 && rb < a.N;
  int lenx = 0, leny = 0;
  if (ok) {
    lenx = ng_len(a.length, ra, a.L);
    leny = ng_len(a.length, rb, a.L);
    ng_stage(sx, a.tok + (long long)ra * a.ld, lenx, words, lane);
    ng_stage(sy, a.tok + (long long)rb * a.ld, leny, words, lane);
  }
  __syncthreads();
  if (!live) return;
  if (!ok) {  // a bad index: no row was read
    if (lane < NGRAM_ORDERS) a.out[p * NGRAM_ORDERS + lane] = -1;
    return;
  }
  int m[4] = {0, 0, 0, 0};  // per lane, over its positions
  for (int ch = 0; ch * WAVE < lenx; ++ch) {
    const int i = ch * WAVE + lane;
    const int x[4] = {sx[i], sx[i + 1], sx[i + 2], sx[i + 3]};
    int c[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    // positions of y with all four n-grams inside the row, then its last
    // three, whose longer n-grams do not exist
    ng_count<false>(sy, 0, leny - 3, x, i, c);
#pragma clang loop vectorize(disable)
    for (int j = max(leny - 3, 0); j < leny; ++j) {
      const int nv = leny - j;  // 1 .. 3
      bool e = x[0] == sy[j];
      c[0] += e;
      if (nv >= 2) {
        e &= x[1] == sy[j + 1];
        c[1] += e;
      }
      if (nv >= 3) {
        e &= x[2] == sy[j + 2];
        c[2] += e;
      }
    }
    if (PRE) {
      if (i < lenx) {
        const short4_t v =
            *reinterpret_cast<const short4_t*>(a.ranks + ((long long)ra * a.L + i) * 4);
        r[0] = v[0], r[1] = v[1], r[2] = v[2], r[3] = v[3];
      }
    } else {
      ng_ranks(sx, lenx, ch, x, i, r);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) m[n] += (i + n + 1 <= lenx && r[n] < c[n]) ? 1 : 0;
  }
  // at most 512 in all: exact in f32
  int tot[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) tot[n] = (int)wave_sum((float)m[n]);
  if (lane < NGRAM_ORDERS)
    a.out[p * NGRAM_ORDERS + lane] = lane == 0 ? tot[0] : lane == 1 ? tot[1] : lane == 2 ? tot[2] : tot[3];
}

}  // namespace tdg

extern "C" {

// Clipped n-gram match counts of P row pairs (tdg_overlap.h NgramArgs), a wave
// per pair. Only positions below a row's length (clamped into [0, L]) count;
// every int32 is a token. A pair with an index outside [0, N) gets -1 in all
// four columns and reads no row. With a->ranks a pre-pass over the N rows runs
// first on the same stream. -1: L outside [1, 512], N or P negative, ld < L;
// -2: a null operand; nothing launched. P == 0 launches nothing.
int tdg_ngram_matches(const tdg::NgramArgs* a, hipStream_t st) {
  if (a->L < 1 || a->L > tdg::NGRAM_MAX_L || a->N < 0 || a->P < 0 || a->ld < a->L) return -1;
  if (a->P == 0) return 0;
  if (((!a->tok || !a->length) && a->N > 0) || !a->pair_a || !a->pair_b || !a->out) return -2;
  const int row_bytes = tdg::ng_row_words(a->L) * (int)sizeof(int);
  const dim3 block(tdg::NG_WAVES * tdg::WAVE);
  const auto blocks = [](int n) { return (unsigned)((n + (long long)tdg::NG_WAVES - 1) / tdg::NG_WAVES); };
  if (a->ranks) {
    if (a->N > 0)
      hipLaunchKernelGGL(tdg::ngram_ranks_kernel, dim3(blocks(a->N)), block,
                         tdg::NG_WAVES * row_bytes, st, *a);
    hipLaunchKernelGGL(tdg::ngram_matches_kernel<true>, dim3(blocks(a->P)), block,
                       2 * tdg::NG_WAVES * row_bytes, st, *a);
  } else {
    hipLaunchKernelGGL(tdg::ngram_matches_kernel<false>, dim3(blocks(a->P)), block,
                       2 * tdg::NG_WAVES * row_bytes, st, *a);
  }
  return 0;
}

}  // extern "C"
