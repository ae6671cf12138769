// Exponential moving average of the weights over (a range of) the flat f32
// master buffer (gfx950), the average evaluation and decoding may run on:
//   e += (p - e) * (1 - d_eff)
//   d_eff = decay, or with warm-up min(decay, (1 + count) / (10 + count))
// where count, the number of updates applied so far, lives in device memory,
// so the update needs no host sync and is captured in the step's HIP graph.
// The first update (count == 0) copies p into e and reads nothing of e. A
// step the gradient-norm pass marked as skipped (adam.hip GNS_SKIP) leaves
// both the average and the count alone, like the Adam kernels leave the
// weights.
#include "tdg_api.h"
#include "tdg_common.h"

namespace tdg {

// word of the gradient-norm device state that holds the skip flag (adam.hip
// GNS_SKIP, ops/kernels/optimizer.py NORM_SKIP)
constexpr int EMA_GNS_SKIP = 3;

__device__ __forceinline__ void ema4(float4& ee, const float4& pp, float omd) {
  float* E = &ee.x;
  const float* P = &pp.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) E[k] += (P[k] - E[k]) * omd;
}

// Streaming: 8 B/param read (p, e) + 4 B written; two float4 groups per
// thread per iteration with all four 16-byte loads issued before any math, as
// in adam_kernel. Plain stores and 64-bit indexing: one launch covers any n.
__global__ __launch_bounds__(256) void ema_kernel(const float* __restrict__ p, float* __restrict__ e,
                                                  long long n, const long long* __restrict__ count,
                                                  float decay, int warmup,
                                                  const float* __restrict__ gstate) {
  if (gstate && gstate[EMA_GNS_SKIP] != 0.f) return;
  const long long cnt = count[0];
  const long long n4 = n >> 2;
  const float4* P4 = reinterpret_cast<const float4*>(p);
  float4* E4 = reinterpret_cast<float4*>(e);
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cnt == 0) {  // first update: e = p bitwise (e may hold anything, NaN included)
    for (; i + stride < n4; i += 2 * stride) {
      const long long j = i + stride;
      const float4 pa = P4[i], pb = P4[j];
      E4[i] = pa;
      E4[j] = pb;
    }
    if (i < n4) E4[i] = P4[i];
    return;
  }
  float d = decay;
  if (warmup) {
    const float c = (float)cnt;
    d = fminf(decay, (1.f + c) / (10.f + c));
  }
  const float omd = 1.f - d;
  for (; i + stride < n4; i += 2 * stride) {
    const long long j = i + stride;
    const float4 pa = P4[i], pb = P4[j];
    float4 ea = E4[i], eb = E4[j];
    ema4(ea, pa, omd);
    ema4(eb, pb, omd);
    E4[i] = ea;
    E4[j] = eb;
  }
  if (i < n4) {
    const float4 pa = P4[i];
    float4 ea = E4[i];
    ema4(ea, pa, omd);
    E4[i] = ea;
  }
}

// (a skipped step is no update: the warm-up ramp does not advance either)
__global__ void ema_count_inc_kernel(long long* count, const float* __restrict__ gstate) {
  if (gstate && gstate[EMA_GNS_SKIP] != 0.f) return;
  count[0] += 1;
}

}  // namespace tdg

using namespace tdg;

// One update of e[0, n) from p[0, n). Every range of a step reads the same
// count; exactly one call per step (the last) passes inc_count, which
// advances it in a one-thread tail launch.
extern "C" int tdg_ema(const float* p, float* e, long long n, long long* count, float decay,
                       int warmup, int inc_count, const float* gstate, hipStream_t st) {
  if (n <= 0 || n % 4 != 0 || !(decay >= 0.f && decay < 1.f)) return -1;
  const long long n4 = n / 4;
  const int blocks = (int)std::min<long long>(8192, (n4 + 255) / 256);
  hipLaunchKernelGGL(ema_kernel, dim3(blocks), dim3(256), 0, st, p, e, n, count, decay, warmup,
                     gstate);
  if (inc_count) hipLaunchKernelGGL(ema_count_inc_kernel, dim3(1), dim3(1), 0, st, count, gstate);
  return 0;
}
