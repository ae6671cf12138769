// A bf16 vocabulary row held by one 256-thread workgroup and searched by
// bisection: the 16-bit order-preserving key of a logit and the row's columns
// in registers or re-read from L2. Shared by sample_token (decode.hip) and the
// wide beam selection (beam_wide.hip).
#pragma once
#include "tdg_vocab_row.h"

namespace tdg {

// The order-preserving 16-bit key of a bf16 logit: a > b <=> okey(a) > okey(b)
// for finite values (-0 counts as +0). -inf and NaN get 0, below every kept
// value: the smallest finite bf16 has key KEY_MIN.
constexpr uint32_t KEY_MIN = 0x0080u;
__device__ __forceinline__ uint32_t okey(float f) {
  if (!(f > -INFINITY)) return 0u;
  uint32_t b = __float_as_uint(f) >> 16;
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
// the bf16 value (as f32) of a key >= KEY_MIN; -0 comes back as +0
__device__ __forceinline__ float unkey(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}

// This thread's columns of a row: 8 at c = 8 tid + 2048 j. NCH > 0: the row
// has at most NCH such chunks and is read once, into registers; NCH == 0: a row
// of any length, re-read (from L2) by every pass.
template <int NCH>
struct RowRegs {
  uint4 w[NCH > 0 ? NCH : 1];
  __device__ __forceinline__ void load(const uint16_t* x, int V) {
    if constexpr (NCH > 0) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int c = threadIdx.x * 8 + j * 2048;
        w[j] = c < V ? *reinterpret_cast<const uint4*>(x + c) : make_uint4(0, 0, 0, 0);
      }
    }
  }
  // g(c, e, j): the values e[0..8) of columns c .. c + 7, chunk j (0 if NCH == 0)
  template <class G>
  __device__ __forceinline__ void chunks(const uint16_t* x, int V, G g) const {
    if constexpr (NCH > 0) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int c = threadIdx.x * 8 + j * 2048;
        if (c < V) {
          float e[8];
          unpack8(w[j], e);
          g(c, e, j);
        }
      }
    } else {
      for (int c = threadIdx.x * 8; c < V; c += 2048) {
        float e[8];
        unpack8(*reinterpret_cast<const uint4*>(x + c), e);
        g(c, e, 0);
      }
    }
  }
  // f(x[v], slot) for the columns v < V, ascending; slot = 8 j + i names the
  // column among this thread's (NCH > 0)
  template <class F>
  __device__ __forceinline__ void scan(const uint16_t* x, int V, F f) const {
    chunks(x, V, [&](int c, const float* e, int j) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c + i < V) f(e[i], 8 * j + i);
    });
  }
};

}  // namespace tdg
