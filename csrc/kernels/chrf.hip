// Clipped character n-gram match counts between pairs of rows of code points
// (n = 1 .. 6): the count behind chrF, and the pairwise utility of
// minimum-Bayes-risk selection among sampled translations.
//
// The identity is overlap.hip's: with r_n(i) = the number of earlier
// occurrences in x of the n-gram at i and c_n(i) = its occurrences in y,
//
//   m_n = sum_i [ r_n(i) < c_n(i) ]      over the n-grams of x (i + n <= |x|).
//
// overlap.hip finds r and c by comparing every position with every position,
// which is right for rows of a hundred words and four orders. A row of
// characters is five times longer and chrF wants six orders, so here a row is
// SORTED once and a pair SEARCHES:
//
// Key. Position i of a row gets six 21-bit fields, field k = chr[i + k] + 1, or
// 0 where i + k is past the row's end; the first character is the top field.
// Fields 0-2 are one 64-bit word (hi), fields 3-5 a second (lo), bit 63 of
// both is clear. Keys compare as (hi, lo), which is the lexicographic order of
// the six characters, so in a sorted row the positions that hold one n-gram are
// adjacent FOR EVERY n AT ONCE: they are the run of keys with the same first n
// fields. An n-gram lies inside its row exactly when field n - 1 is not 0.
//
// Row pre-pass (chrf_sort_kernel), a workgroup per row: the keys are built in
// LDS, padded to a power of two with all-ones keys (no real key has bit 63
// set), sorted by a bitonic network, and every sorted position then finds the
// start of its six runs by searching the sorted row itself: r_n = position -
// start. Keys and ranks go to scratch, 16 bytes each per position.
//
// Pair kernel (chrf_pairs_kernel), a wave per pair: only y's sorted keys are
// staged in LDS (hi words, then lo words). The lanes take x's SORTED positions
// in chunks of 64 and read key and ranks straight from scratch into registers,
// the next chunk's while this one is searched. c_n is upper bound minus lower
// bound of the n-prefix in y, and each order searches inside the range of the
// order before, so orders 1-3 compare hi words only, orders 4-6 (inside a run
// of equal hi) lo words only, and the ranges collapse after two or three
// orders of ordinary text. Both bounds advance in one branch-free loop whose
// trip count depends on the range's size alone. Neighbouring lanes hold
// neighbouring keys, so their probes mostly hit the same LDS words (a
// broadcast). Integers only, no atomics: a pair's result depends on its two
// rows and nothing else.
#include "tdg_api.h"
#include "tdg_common.h"

namespace tdg {

typedef unsigned long long u64;
typedef u64 u64x2_t __attribute__((ext_vector_type(2)));

constexpr int CHRF_SORT_THREADS = 256;
constexpr int CHRF_PAIR_WAVES = 4;             // pairs per workgroup, at most
constexpr int CHRF_PAIR_LDS = 64 * 1024;       // what a workgroup of the pair kernel may stage
constexpr int CHRF_BITS = 21;                  // a field
constexpr u64 CHRF_FIELD = (1ull << CHRF_BITS) - 1;

__host__ __device__ __forceinline__ int chrf_pow2(int n) {
  int s = 1;
  while (s < n) s <<= 1;
  return s;
}

// pairs per workgroup at row length L: 16 L bytes of LDS each
__host__ __device__ __forceinline__ int chrf_pair_waves(int L) {
  const int fit = CHRF_PAIR_LDS / (L * 16);
  return fit < 1 ? 1 : fit > CHRF_PAIR_WAVES ? CHRF_PAIR_WAVES : fit;
}

__device__ __forceinline__ int chrf_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int chrf_len(const int* length, long long row, int L) {
  return chrf_uniform(min(max(length[row], 0), L));
}

// field value of a character: 1 .. 0x1FFFFF
__device__ __forceinline__ u64 chrf_field(int c) {
  return (u64)min((unsigned)c & (unsigned)CHRF_FIELD, (unsigned)CHRF_FIELD - 1u) + 1u;
}

// [a, b) -> the positions of the sorted words y[a, b) that lie in [kl, ku]:
// lower bound of kl and upper bound of ku, both by the branch-free halving
// search (the probes stay inside [a, b); an empty range stays empty)
__device__ __forceinline__ void chrf_range(const u64* y, int& a, int& b, u64 kl, u64 ku) {
  int n = b - a, lb = a, ub = a;
  while (n > 1) {
    const int h = n >> 1;
    const u64 vl = y[lb + h - 1], vu = y[ub + h - 1];
    lb += vl < kl ? h : 0;
    ub += vu <= ku ? h : 0;
    n -= h;
  }
  if (n == 1) {
    lb += y[lb] < kl ? 1 : 0;
    ub += y[ub] <= ku ? 1 : 0;
  }
  a = lb, b = ub;
}

// The six nested ranges of the key (xh, xl) in the sorted row (yh, yl) of
// `len` keys; live: this lane has a key. f(n - 1, start, count) per order; an
// n-gram that is not inside its own row finds nothing, nor does any longer one.
template <class F>
__device__ __forceinline__ void chrf_orders(const u64* yh, const u64* yl, int len, u64 xh, u64 xl,
                                            bool live, F&& f) {
  int a = 0, b = live ? len : 0;
#pragma unroll
  for (int n = 0; n < CHRF_ORDERS; ++n) {
    const int sh = CHRF_BITS * (2 - n % 3);
    const u64 w = n < 3 ? xh : xl, low = (1ull << sh) - 1;
    if (((w >> sh) & CHRF_FIELD) == 0) b = a;
    chrf_range(n < 3 ? yh : yl, a, b, w & ~low, w | low);
    f(n, a, b - a);
  }
}

// keys[row] = the row's sorted keys, ranks[row] = their ranks, for the
// positions below length[row] (later ones are not written and never read)
__global__ __launch_bounds__(CHRF_SORT_THREADS) void chrf_sort_kernel(const ChrfArgs a) {
  extern __shared__ u64 chrf_lds[];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  const int len = chrf_len(a.length, row, a.L);
  const int S = chrf_pow2(len);
  u64* kh = chrf_lds;
  u64* kl = chrf_lds + chrf_pow2(a.L);
  const int* x = a.chr + row * a.ld;
  for (int i = tid; i < S; i += CHRF_SORT_THREADS) {
    u64 f[CHRF_ORDERS];
#pragma unroll
    for (int k = 0; k < CHRF_ORDERS; ++k) f[k] = i + k < len ? chrf_field(x[i + k]) : 0;
    const bool in = i < len;
    kh[i] = in ? f[0] << 2 * CHRF_BITS | f[1] << CHRF_BITS | f[2] : ~0ull;
    kl[i] = in ? f[3] << 2 * CHRF_BITS | f[4] << CHRF_BITS | f[5] : ~0ull;
  }
  __syncthreads();
  // bitonic network, ascending: compare-exchange t pairs position i (bit j
  // clear) with i | j
  for (int k = 2; k <= S; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < S / 2; t += CHRF_SORT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const u64 h0 = kh[i], l0 = kl[i], h1 = kh[p], l1 = kl[p];
        const bool gt = h0 > h1 || (h0 == h1 && l0 > l1);
        if (gt == ((i & k) == 0)) {
          kh[i] = h1, kl[i] = l1;
          kh[p] = h0, kl[p] = l0;
        }
      }
      __syncthreads();
    }
  }
  u64x2_t* keys = reinterpret_cast<u64x2_t*>(a.keys) + row * a.L;
  short8_t* ranks = reinterpret_cast<short8_t*>(a.ranks) + row * a.L;
  for (int s0 = 0; s0 < len; s0 += CHRF_SORT_THREADS) {
    const int s = s0 + tid;
    const bool live = s < len;
    const u64 xh = live ? kh[s] : 0, xl = live ? kl[s] : 0;
    short8_t r = {0, 0, 0, 0, 0, 0, 0, 0};
    chrf_orders(kh, kl, len, xh, xl, live, [&](int n, int start, int count) {
      r[n] = (short)(count > 0 ? s - start : 0);
    });
    if (live) {
      keys[s] = u64x2_t{xh, xl};
      ranks[s] = r;
    }
  }
}

__global__ __launch_bounds__(CHRF_PAIR_WAVES * WAVE) void chrf_pairs_kernel(const ChrfArgs a) {
  extern __shared__ u64 chrf_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = chrf_uniform(threadIdx.x / WAVE);
  u64* yh = chrf_lds + (size_t)w * 2 * a.L;
  u64* yl = yh + a.L;
  const long long p = (long long)blockIdx.x * (blockDim.x / WAVE) + w;
  // every branch below is wave-uniform
  const bool live = p < a.P;
  int ra = -1, rb = -1;
  if (live) ra = chrf_uniform(a.pair_a[p]), rb = chrf_uniform(a.pair_b[p]);
  const bool ok = ra >= 0 && ra < a.N && rb >= 0 && rb < a.N;
  int lenx = 0, leny = 0;
  const u64x2_t* kx = nullptr;
  const short8_t* rx = nullptr;
  if (ok) {
    lenx = chrf_len(a.length, ra, a.L);
    leny = chrf_len(a.length, rb, a.L);
    kx = reinterpret_cast<const u64x2_t*>(a.keys) + (long long)ra * a.L;
    rx = reinterpret_cast<const short8_t*>(a.ranks) + (long long)ra * a.L;
    const u64x2_t* ky = reinterpret_cast<const u64x2_t*>(a.keys) + (long long)rb * a.L;
    for (int k = lane; k < leny; k += WAVE) {
      const u64x2_t v = ky[k];
      yh[k] = v[0], yl[k] = v[1];
    }
  }
  __syncthreads();
  if (!live) return;
  if (!ok) {  // a bad index: no row was read
    if (lane < CHRF_ORDERS) a.out[p * CHRF_ORDERS + lane] = -1;
    return;
  }
  int m[CHRF_ORDERS] = {0, 0, 0, 0, 0, 0};  // per lane, over its positions
  u64x2_t key = {0, 0};
  short8_t rank = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane < lenx) key = kx[lane], rank = rx[lane];
  for (int s0 = 0; s0 < lenx; s0 += WAVE) {
    const u64x2_t k = key;
    const short8_t r = rank;
    const int nxt = s0 + WAVE + lane;
    if (nxt < lenx) key = kx[nxt], rank = rx[nxt];
    chrf_orders(yh, yl, leny, k[0], k[1], s0 + lane < lenx,
                [&](int n, int, int count) { m[n] += r[n] < count ? 1 : 0; });
  }
  // at most 2048 in all: exact in f32
  int tot[CHRF_ORDERS];
#pragma unroll
  for (int n = 0; n < CHRF_ORDERS; ++n) tot[n] = (int)wave_sum((float)m[n]);
  if (lane < CHRF_ORDERS)
    a.out[p * CHRF_ORDERS + lane] = lane == 0   ? tot[0]
                                    : lane == 1 ? tot[1]
                                    : lane == 2 ? tot[2]
                                    : lane == 3 ? tot[3]
                                    : lane == 4 ? tot[4]
                                                : tot[5];
}

}  // namespace tdg

extern "C" {

// Clipped character n-gram match counts of P row pairs (tdg_chrf.h ChrfArgs):
// the row pre-pass over all N rows, then a wave per pair, on one stream. Only
// positions below a row's length (clamped into [0, L]) count. A pair with an
// index outside [0, N) gets -1 in all six columns and reads no row. -1: L
// outside [1, 2048], N or P negative, ld < L; -2: a null operand; nothing
// launched. P == 0 launches nothing.
int tdg_char_ngram_matches(const tdg::ChrfArgs* a, hipStream_t st) {
  if (a->L < 1 || a->L > tdg::CHRF_MAX_L || a->N < 0 || a->P < 0 || a->ld < a->L) return -1;
  if (a->P == 0) return 0;
  if (((!a->chr || !a->length || !a->keys || !a->ranks) && a->N > 0) || !a->pair_a || !a->pair_b ||
      !a->out)
    return -2;
  if (a->N > 0)
    hipLaunchKernelGGL(tdg::chrf_sort_kernel, dim3((unsigned)a->N), dim3(tdg::CHRF_SORT_THREADS),
                       tdg::chrf_pow2(a->L) * 16, st, *a);
  const int waves = tdg::chrf_pair_waves(a->L);
  hipLaunchKernelGGL(tdg::chrf_pairs_kernel, dim3((unsigned)((a->P + (long long)waves - 1) / waves)),
                     dim3(waves * tdg::WAVE), waves * a->L * 16, st, *a);
  return 0;
}

}  // extern "C"
