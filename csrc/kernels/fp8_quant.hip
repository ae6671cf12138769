// fp8 quantisation and delayed scaling for gfx950.
//
// x8 = fp8(x * scale) of bf16 activations / weights / gradients (e4m3, or
// e5m2 for gradients) with per-tensor scales that live in device memory
// (delayed scaling: each producer records the amax of what it quantised, and
// fp8_scale_update turns last step's amax into this step's scale), so a
// captured HIP graph stays valid across steps.
#include "tdg_api.h"
#include "fp8_impl.h"

#include <algorithm>

namespace tdg {

// Quantise a [M, N] bf16 gradient (row stride ld) to fp8 (FMT) AND write the
// per-row-block column sums of the bf16 values (part[blockIdx.y][N], folded
// later: the bias gradient of the layer whose output gradient this is) in
// one pass. Block: 256 columns (32 lanes x 8) x 8 row lanes, QC_ROWS rows.
constexpr int QC_ROWS = 256;
template <int FMT>
__global__ __launch_bounds__(256) void fp8_quant_colsum_kernel(const bf16_t* __restrict__ x, int ld,
                                                               uint8_t* __restrict__ y8, int M,
                                                               int N, const float* __restrict__ scale,
                                                               unsigned* __restrict__ amax_out,
                                                               float* __restrict__ part) {
  __shared__ float red[8][256 + 4];
  __shared__ float redm[4];
  const float s = scale[0];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int n = blockIdx.x * 256 + cl * 8;
  const int r0 = blockIdx.y * QC_ROWS;
  const int r1 = min(M, r0 + QC_ROWS);
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float amax = 0.f;
  if (n < N) {  // (host: N % 8 == 0, ld % 8 == 0)
    for (int r = r0 + rl; r < r1; r += 8) {
      const short8_t v = *reinterpret_cast<const short8_t*>(x + (size_t)r * ld + n);
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = bf2f((bf16_t)v[e]);
        cs[e] += f[e];
        amax = fmaxf(amax, fabsf(f[e]));
      }
      int lo, hi;
      f8::quant8<FMT>(f, s, lo, hi);
      *reinterpret_cast<int2*>(y8 + (size_t)r * N + n) = make_int2(lo, hi);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cl * 8 + e] = cs[e];
  TDG_F8_AMAX_STAGE(redm, amax, threadIdx.x)
  __syncthreads();
  const int c = threadIdx.x;  // one column per thread
  if (blockIdx.x * 256 + c < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][c];
    part[(size_t)blockIdx.y * N + blockIdx.x * 256 + c] = t;
  }
  if (threadIdx.x == 0 && amax_out)
    f8::amax_record(redm, amax_word(amax_out, blockIdx.y * gridDim.x + blockIdx.x));
}

// Transposing e4m3 quantisation of same-shape weights: dst[g] [C][R] =
// e4m3(src[g] [R][C]^T * scale[slot[g]]), amax into amax[slot[g]] -- the
// transposed weight copies of the fp8 dgrads straight from the bf16 compute
// copy (no bf16 transposed copy). 64 x 64 tiles through LDS.
constexpr int QT_MAXG = 64;
struct QuantTGroup {
  const bf16_t* src[QT_MAXG];
  uint8_t* dst[QT_MAXG];
  int slot[QT_MAXG];
};
__global__ __launch_bounds__(256) void fp8_quant_t_kernel(QuantTGroup grp, int R, int C,
                                                          const float* __restrict__ scale,
                                                          unsigned* __restrict__ amax) {
  __shared__ float tile[64][65];
  __shared__ float redm[4];
  const bf16_t* __restrict__ src = grp.src[blockIdx.y];
  uint8_t* __restrict__ dst = grp.dst[blockIdx.y];
  const int slot = grp.slot[blockIdx.y];
  const float s = scale[slot];
  const int tiles_c = (C + 63) / 64;
  const int r0 = (blockIdx.x / tiles_c) * 64, c0 = (blockIdx.x % tiles_c) * 64;
  const int tid = threadIdx.x;
  float am = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = tid + 256 * k;
    const int r = id >> 3, c = (id & 7) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = r0 + r < R && c0 + c + e < C;
      const float f = in ? bf2f(src[(size_t)(r0 + r) * C + c0 + c + e]) : 0.f;
      tile[r][c + e] = f;
      am = fmaxf(am, fabsf(f));
    }
  }
  __syncthreads();
  // dst row = source column (c0 + c), 8 consecutive source rows per thread
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = tid + 256 * k;
    const int c = id >> 3, r = (id & 7) * 8;
    if (c0 + c >= C) continue;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = tile[r + e][c] * s;
    int lo, hi;
    // (scaled as they are read: scaling inside quant8 schedules the LDS reads
    // and the converts differently)
    f8::quant8<0>(f, 1.f, lo, hi);
    uint8_t* d = dst + (size_t)(c0 + c) * R + r0 + r;
    if (r0 + r + 8 <= R && (R % 8) == 0) {
      *reinterpret_cast<int2*>(d) = make_int2(lo, hi);
    } else {
      for (int e = 0; e < 8 && r0 + r + e < R; ++e) d[e] = f8::quant8_byte(lo, hi, e);
    }
  }
  TDG_F8_AMAX_STAGE(redm, am, tid)
  __syncthreads();
  if (tid == 0) f8::amax_record(redm, amax_word(amax + (size_t)slot * AMAX_WORDS, blockIdx.x));
}

// Blocks b of nb quantise the span x[0 .. n) (8 elements per thread and
// pass, a scalar tail) with scale s and record its amax at
// amax_word(AMAX_SLOT_, b) if AMAX_ON_: the body of the two kernels below
#define TDG_F8_QUANT_SPAN(FMT_, x, y8, n, s, b, nb, AMAX_ON_, AMAX_SLOT_)                \
  float amax = 0.f;                                                                      \
  for (long long i = ((long long)(b) * blockDim.x + threadIdx.x) * 8; i < n;             \
       i += (long long)(nb) * blockDim.x * 8) {                                          \
    if (i + 8 <= n) {                                                                    \
      const short8_t v = *reinterpret_cast<const short8_t*>(x + i);                      \
      float f[8];                                                                        \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                    \
        f[e] = bf2f((bf16_t)v[e]);                                                       \
        amax = fmaxf(amax, fabsf(f[e]));                                                 \
      }                                                                                  \
      int lo, hi;                                                                        \
      f8::quant8<FMT_>(f, s, lo, hi);                                                    \
      *reinterpret_cast<int2*>(y8 + i) = make_int2(lo, hi);                              \
    } else {                                                                             \
      for (long long e = i; e < n; ++e) {                                                \
        const float f = bf2f(x[e]);                                                      \
        amax = fmaxf(amax, fabsf(f));                                                    \
        y8[e] = f8::quant1<FMT_>(f, s);                                                  \
      }                                                                                  \
    }                                                                                    \
  }                                                                                      \
  __shared__ float red[4];                                                               \
  TDG_F8_AMAX_STAGE(red, amax, threadIdx.x)                                              \
  __syncthreads();                                                                       \
  if (threadIdx.x == 0 && (AMAX_ON_)) f8::amax_record(red, amax_word(AMAX_SLOT_, b));

// y8 = e4m3(x * scale[0]); amax_out = max|x| (both optional sides)
template <int FMT>
__global__ __launch_bounds__(256) void fp8_quant_kernel(const bf16_t* __restrict__ x,
                                                        uint8_t* __restrict__ y8, long long n,
                                                        const float* __restrict__ scale,
                                                        unsigned* __restrict__ amax_out) {
  const float s = scale[0];
  TDG_F8_QUANT_SPAN(FMT, x, y8, n, s, blockIdx.x, gridDim.x, amax_out, amax_out)
}

// Many tensors in one launch (the weight refresh after every optimizer step:
// 43 weight matrices of Transformer-big, 43 launches of ~8 us before): block
// ranges per segment from a host prefix sum, each segment its own scale and
// amax slot.
constexpr int QMAX = 64;
struct QuantSegs {
  const bf16_t* x[QMAX];
  uint8_t* y[QMAX];
  long long n[QMAX];
  int slot[QMAX];
  int blk0[QMAX + 1];
};

__global__ __launch_bounds__(256) void fp8_quant_multi_kernel(const QuantSegs segs, int nseg,
                                                              const float* __restrict__ scale,
                                                              unsigned* __restrict__ amax_out) {
  int sg = 0;
  for (int i = 1; i < nseg; ++i)
    if ((int)blockIdx.x >= segs.blk0[i]) sg = i;
  const bf16_t* __restrict__ x = segs.x[sg];
  uint8_t* __restrict__ y8 = segs.y[sg];
  const long long n = segs.n[sg];
  const int b = blockIdx.x - segs.blk0[sg], nb = segs.blk0[sg + 1] - segs.blk0[sg];
  const float s = scale[segs.slot[sg]];
  TDG_F8_QUANT_SPAN(0, x, y8, n, s, b, nb, amax_out, amax_out + (long long)segs.slot[sg] * AMAX_WORDS)
}

// Delayed scaling: scale[i] = 448 / (amax[i] * 2^margin) from last step's
// amax (kept when nothing was recorded), then amax[i] = 0.
// One wave per slot, lane j reads (and clears) word j of the slot's spread.
__global__ __launch_bounds__(256) void fp8_scale_update_kernel(float* __restrict__ scale,
                                                               unsigned* __restrict__ amax, int n,
                                                               float margin_pow2, float fmax) {
  static_assert(AMAX_SPREAD == 64, "one lane per spread word");
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  unsigned* w = amax + (long long)i * AMAX_WORDS + lane * AMAX_STRIDE;
  unsigned m = *w;
  *w = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  const float a = __uint_as_float(m);
  // power-of-two scales: dequantisation (x8 / scale) is exact in bf16 / f32,
  // so an fp8 operand and its bf16 dequantised copy carry the same values
  if (lane == 0 && a > 0.f && isfinite(a)) {
    int e;
    frexpf(fmax / (a * margin_pow2), &e);  // ratio = f * 2^e, f in [0.5, 1)
    scale[i] = ldexpf(1.f, e - 1);         // largest 2^k <= ratio
  }
}

// e4m3 -> f32 (tests / debugging)
__global__ void fp8_dequant_kernel(const uint8_t* __restrict__ x8, float* __restrict__ y,
                                   long long n, float inv_scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = __builtin_amdgcn_cvt_f32_fp8((int)x8[i], 0) * inv_scale;
}

}  // namespace tdg

using namespace tdg;

extern "C" int tdg_fp8_quant(const void* x, void* y8, long long n, const float* scale,
                             unsigned* amax, int fmt, hipStream_t st) {
  const int blocks = (int)std::min<long long>(1024, (n / 8 + 255) / 256 + 1);
  if (fmt == 1)
    hipLaunchKernelGGL(fp8_quant_kernel<1>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x,
                       (uint8_t*)y8, n, scale, amax);
  else
    hipLaunchKernelGGL(fp8_quant_kernel<0>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x,
                       (uint8_t*)y8, n, scale, amax);
  return 0;
}

// segments: x[i] (bf16, n[i] elements) -> y[i] with scale[slot[i]], amax into
// amax[slot[i]] (AMAX_SPREAD words each); blocks split by size
extern "C" int tdg_fp8_quant_multi(const void* const* x, void* const* y, const long long* n,
                                   const int* slot, int nseg, const float* scale, unsigned* amax,
                                   hipStream_t st) {
  if (nseg <= 0 || nseg > QMAX) return -2;
  QuantSegs q{};
  long long total = 0;
  for (int i = 0; i < nseg; ++i) total += n[i];
  int blk = 0;
  for (int i = 0; i < nseg; ++i) {
    q.x[i] = (const bf16_t*)x[i];
    q.y[i] = (uint8_t*)y[i];
    q.n[i] = n[i];
    q.slot[i] = slot[i];
    q.blk0[i] = blk;
    // ~4096 blocks over all segments, at least one each
    blk += (int)std::max<long long>(1, (n[i] * 4096 + total - 1) / std::max<long long>(total, 1));
  }
  q.blk0[nseg] = blk;
  hipLaunchKernelGGL(fp8_quant_multi_kernel, dim3(blk), dim3(256), 0, st, q, nseg, scale, amax);
  return 0;
}

extern "C" int tdg_fp8_scale_update(float* scale, unsigned* amax, int n, float margin_pow2,
                                    float fmax, hipStream_t st) {
  hipLaunchKernelGGL(fp8_scale_update_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, scale, amax, n,
                     margin_pow2, fmax);
  return 0;
}

extern "C" int tdg_fp8_dequant(const void* x8, float* y, long long n, float inv_scale,
                               hipStream_t st) {
  hipLaunchKernelGGL(fp8_dequant_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (const uint8_t*)x8, y, n, inv_scale);
  return 0;
}

// y8 [M, N] (contiguous) = fp8(x * scale) of x [M, N] (row stride ld), amax
// recorded, and part[ceil(M / 256)][N] = per-row-block column sums of x.
extern "C" int tdg_fp8_quant_colsum(const void* x, int ld, void* y8, int M, int N,
                                    const float* scale, unsigned* amax, float* part, int fmt,
                                    hipStream_t st) {
  if (N % 8 || ld % 8 || M <= 0) return -2;
  const dim3 grid(cdiv(N, 256), cdiv(M, QC_ROWS));
  if (fmt == 1)
    hipLaunchKernelGGL(fp8_quant_colsum_kernel<1>, grid, dim3(256), 0, st, (const bf16_t*)x, ld,
                       (uint8_t*)y8, M, N, scale, amax, part);
  else
    hipLaunchKernelGGL(fp8_quant_colsum_kernel<0>, grid, dim3(256), 0, st, (const bf16_t*)x, ld,
                       (uint8_t*)y8, M, N, scale, amax, part);
  return 0;
}

extern "C" int tdg_fp8_quant_t(const void* const* src, void* const* dst, const int* slot, int G,
                               int R, int C, const float* scale, unsigned* amax, hipStream_t st) {
  if (G < 1 || G > QT_MAXG || R < 1 || C < 1) return -2;
  QuantTGroup g{};
  for (int i = 0; i < G; ++i) {
    g.src[i] = (const bf16_t*)src[i];
    g.dst[i] = (uint8_t*)dst[i];
    g.slot[i] = slot[i];
  }
  const int tiles = cdiv(R, 64) * cdiv(C, 64);
  hipLaunchKernelGGL(fp8_quant_t_kernel, dim3(tiles, G), dim3(256), 0, st, g, R, C, scale, amax);
  return 0;
}
