// Argument block of the character n-gram kernels (chrf.hip), host <-> device.
#pragma once
#include <stdint.h>

namespace tdg {

constexpr int CHRF_MAX_L = 2048;  // longest row
constexpr int CHRF_ORDERS = 6;    // n = 1 .. 6

// Clipped character n-gram match counts (chrF's) between pairs of rows of code
// points: out[p, n - 1] = sum over the distinct n-grams g of x of
// min(count_x(g), count_y(g)), x = chr[pair_a[p], :length[pair_a[p]]], y
// likewise of pair_b. A character is its low 21 bits (0 .. 0x10FFFF is a code
// point; 0x1FFFFF, which is none, counts as 0x1FFFFE).
struct ChrfArgs {
  const int* chr;      // [N, ld], the first L columns of a row may count
  const int* length;   // [N], clamped into [0, L]
  const int* pair_a;   // [P]
  const int* pair_b;   // [P]
  int* out;            // [P, 6] contiguous; -1 x 6 for a pair with an index outside [0, N)
  // Scratch, both 16-byte aligned, written by the row pre-pass and read by the
  // pair kernel; what they hold on entry does not matter.
  unsigned long long* keys;  // int64 [N, L, 2]: a row's sorted 126-bit n-gram keys
  int16_t* ranks;            // int16 [N, L, 8]: per sorted position r_1 .. r_6, two slots spare
  long long ld;        // row stride of chr, >= L
  int N, L, P;
};

}  // namespace tdg
