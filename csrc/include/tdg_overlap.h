// Argument block of the n-gram overlap kernel (overlap.hip), host <-> device.
#pragma once
#include <stdint.h>

namespace tdg {

constexpr int NGRAM_MAX_L = 512;  // longest row
constexpr int NGRAM_ORDERS = 4;   // n = 1 .. 4

// Clipped n-gram match counts (BLEU's) between pairs of token rows:
// out[p, n - 1] = sum over the distinct n-grams g of x of min(count_x(g),
// count_y(g)), x = tok[pair_a[p], :length[pair_a[p]]], y likewise of pair_b.
struct NgramArgs {
  const int* tok;      // [N, ld], the first L columns of a row may count
  const int* length;   // [N], clamped into [0, L]
  const int* pair_a;   // [P]
  const int* pair_b;   // [P]
  int* out;            // [P, 4] contiguous; -1 x 4 for a pair with an index outside [0, N)
  // Scratch int16 [N, L, 4], 8-byte aligned, or null. Given: a pre-pass writes
  // every row's ranks once and the pair kernel reads them; null: the pair
  // kernel computes the ranks of x itself.
  int16_t* ranks;
  long long ld;        // row stride of tok, >= L
  int N, L, P;
};

}  // namespace tdg
