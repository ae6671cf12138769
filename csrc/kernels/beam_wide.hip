// Beam selection for widths up to 64 (gfx950), used by infer/beam.py through
// ops.kernels.beam_topk: decode.hip's beam_topk keeps a sorted list of `beam`
// candidates per thread and runs one workgroup per sentence, which fits a
// width of 8 and no more. Here the step is two launches on one stream.
//
// beam_rows: a workgroup per row, all B * beam at once. The row's k-th largest
// candidate by sample_token's bisection on the 16-bit key of a bf16 logit
// (decode_row.h; a row of up to 8192 columns stays in registers, a longer one
// is re-read from L2), then one pass that keeps what lies above it and the
// lowest-indexed ties: at most `beam` survivors per row, into the workspace.
//
// beam_merge: a workgroup per sentence holds the <= beam^2 survivors in
// registers and extracts `beam` in order with the arg-best rounds of
// beam_topk, writes the slots and advances the ancestry table as it does.
//
// The candidate values, their order and the dead slots are beam_topk's bit
// for bit: the logsumexp takes the same tdg_vocab_row.h steps in the same
// order. No atomics in global memory; the one LDS counter hands out slots
// whose order does not matter. This file is compiled without packed f32
// instructions (_build.py HIP_EXTRA_FLAGS).
#include "decode_row.h"
#include "tdg_api.h"
#include "tdg_vocab_row.h"

namespace tdg {

// Stage 1 of the wide selection, one workgroup per row: the row's best
// q = min(beam, candidates) candidates into its workspace slots, unordered.
// cv = score + (x - lse) does not decrease with x, so the q-th largest cv is
// that of the q-th largest logit: its key by bisection (16 counting passes
// over the row, in registers for NCH > 0), theta from it by cv's own
// expression. Kept: every cv > theta and, of the cv == theta (logits below the
// q-th can round to it), the lowest columns that fill the quota -- their last
// column by a second bisection, only where more tie than fit.
template <int NCH>
__global__ __launch_bounds__(256) void beam_rows_kernel(const BeamWideArgs w) {
  __shared__ float red[4];
  __shared__ int s_slot;
  const BeamTopkArgs& a = w.k;
  const int tid = threadIdx.x, r = blockIdx.x, V = a.V, beam = a.beam;
  const int base = (r % beam) * V;  // flat index of the row's column 0
  float* const ov = w.ws_val + (long long)r * beam;
  int* const oi = w.ws_idx + (long long)r * beam;
  if (tid == 0) s_slot = 0;
  const float sc = a.score[r];
  // every branch below is workgroup-uniform
  if (!(sc > -INFINITY)) {  // a dead slot (or NaN) offers nothing
    if (tid == 0) w.ws_cnt[r] = 0;
    return;
  }
  if (a.fin[r]) {  // ended: itself, once, score unchanged
    if (tid == 0) {
      ov[0] = sc;
      oi[0] = base + a.pad_id;
      w.ws_cnt[r] = 1;
    }
    return;
  }
  const uint16_t* x = a.logits + (long long)r * a.ldl;
  RowRegs<NCH> row;
  row.load(x, V);
  // the logsumexp of beam_topk_kernel: the same terms in the same order
  float mx = -INFINITY;
  row.scan(x, V, [&](float f, int) { mx = fmaxf(mx, f); });
  mx = block_max(mx, red);
  if (!(mx > -INFINITY)) {  // no finite logit
    if (tid == 0) w.ws_cnt[r] = 0;
    return;
  }
  float sum = 0.f;
  row.scan(x, V, [&](float f, int) { sum += __expf(f - mx); });
  const float lse = mx + logf(block_sum(sum, red));

  // |{v < V: pred(cv[v], x[v], v)}|, exact in f32 (V <= 65536)
  auto count = [&](auto pred) {
    float n = 0.f;
    row.chunks(x, V, [&](int c, const float* e, int) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c + i < V && pred(sc + (e[i] - lse), e[i], c + i)) n += 1.f;
    });
    return (int)block_sum(n, red);
  };
  const int ncand = count([](float cv, float, int) { return cv > -INFINITY; });
  const int q = min(beam, ncand);
  float theta = -INFINITY;  // q == ncand: every candidate
  int last = -1;            // the last column taken of those with cv == theta
  if (q < ncand) {
    uint32_t t = 0;  // the largest key with |{candidates of key >= t}| >= q
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = t | (1u << bit);
      if (count([=](float cv, float f, int) { return cv > -INFINITY && okey(f) >= cand; }) >= q)
        t = cand;
    }
    theta = sc + (unkey(t) - lse);
    const int above = count([=](float cv, float, int) { return cv > theta; });  // < q
    const int ties = count([=](float cv, float, int) { return cv == theta; });  // >= q - above
    const int need = q - above;
    last = V;
    if (ties > need) {
      int l = 0;  // the largest column with fewer than `need` ties before it
      for (int bit = 15; bit >= 0; --bit) {
        const int cand = l | (1 << bit);
        if (count([=](float cv, float, int v) { return cv == theta && v < cand; }) < need) l = cand;
      }
      last = l;
    }
  }
  row.chunks(x, V, [&](int c, const float* e, int) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float cv = sc + (e[i] - lse);
      if (c + i < V && (cv > theta || (cv == theta && c + i <= last))) {
        const int s = atomicAdd(&s_slot, 1);  // LDS; the slots' order is free
        if (s < beam) {
          ov[s] = cv;
          oi[s] = base + c + i;
        }
      }
    }
  });
  __syncthreads();
  if (tid == 0) w.ws_cnt[r] = min(s_slot, beam);
}

// Stage 2, one workgroup per sentence: its rows' candidates (at most beam^2,
// NK per thread, in registers) and `beam` rounds of the workgroup arg-best
// over the threads' best; the winner's owner drops it and looks again. Slots,
// dead slots and the ancestry update as in beam_topk_kernel.
template <int NK>
__global__ __launch_bounds__(256) void beam_merge_kernel(const BeamWideArgs w) {
  __shared__ float red[4];
  __shared__ int redi[4];
  __shared__ int s_parent[BEAM_WIDE_MAX];
  const BeamTopkArgs& a = w.k;
  const int tid = threadIdx.x, V = a.V, beam = a.beam;
  const int r0 = blockIdx.x * beam;

  float lv[NK];
  int li[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int e = tid + 256 * k, row = e / beam;
    lv[k] = -INFINITY;
    li[k] = NO_CAND;
    if (e < beam * beam && e - row * beam < w.ws_cnt[r0 + row]) {
      lv[k] = w.ws_val[(long long)r0 * beam + e];
      li[k] = w.ws_idx[(long long)r0 * beam + e];
    }
  }
  float mv;  // this thread's best
  int mi;
  auto look = [&]() {
    mv = lv[0];
    mi = li[0];
#pragma unroll
    for (int k = 1; k < NK; ++k)
      if (better(lv[k], li[k], mv, mi)) {
        mv = lv[k];
        mi = li[k];
      }
  };
  look();

  for (int k = 0; k < beam; ++k) {
    float bv = mv;
    int bi = mi;
    TDG_ARGBEST_WAVES(bv, bi, red, redi)
    bv = red[0];
    bi = redi[0];
    TDG_ARGBEST_FOLD(bv, bi, red, redi)
    __syncthreads();
    if (bi != NO_CAND && mi == bi) {  // the winner's owner moves on
#pragma unroll
      for (int j = 0; j < NK; ++j)
        if (li[j] == bi) {
          lv[j] = -INFINITY;
          li[j] = NO_CAND;
        }
      look();
    }
    if (tid == 0) {
      const int r = r0 + k;
      if (bi == NO_CAND) {  // fewer candidates than slots: a dead slot
        a.score_out[r] = -INFINITY;
        a.parent[r] = r0;
        a.token[r] = a.pad_id;
        a.fin_out[r] = 1;
        s_parent[k] = r0;
      } else {
        const int b = bi / V, tok = bi - b * V;
        a.score_out[r] = bv;
        a.parent[r] = r0 + b;
        a.token[r] = tok;
        a.fin_out[r] = (a.fin[r0 + b] != 0 || tok == a.end_id) ? 1 : 0;
        s_parent[k] = r0 + b;
      }
    }
  }
  if (a.anc_out == nullptr) return;
  __syncthreads();
  const int wd = a.t + 2;
  for (int i = tid; i < beam * wd; i += 256) {
    const int b = i / wd, j = i - b * wd;
    a.anc_out[(long long)(r0 + b) * a.ld_anc + j] =
        j <= a.t ? a.anc_in[(long long)s_parent[b] * a.ld_anc + j] : r0 + b;
  }
}

}  // namespace tdg

extern "C" {

// One beam-search step as tdg_beam_topk defines it, with the same result bit
// for bit, for 1 <= beam <= 64 (tdg_decode.h BeamWideArgs): beam_rows on
// B * beam workgroups, then beam_merge on B. The workspace need not be cleared.
int tdg_beam_topk_wide(const tdg::BeamWideArgs* w, hipStream_t st) {
  const tdg::BeamTopkArgs* a = &w->k;
  if (a->beam < 1 || a->beam > tdg::BEAM_WIDE_MAX || a->V < 1 || a->V > 65536) return -1;
  if (w->ws_val == nullptr || w->ws_idx == nullptr || w->ws_cnt == nullptr) return -2;
  if (a->B <= 0) return 0;
  const dim3 rows(a->B * a->beam), block(256);
  if (a->V <= 2048)  // the row in registers, as in sample_token
    hipLaunchKernelGGL(tdg::beam_rows_kernel<1>, rows, block, 0, st, *w);
  else if (a->V <= 8192)
    hipLaunchKernelGGL(tdg::beam_rows_kernel<4>, rows, block, 0, st, *w);
  else
    hipLaunchKernelGGL(tdg::beam_rows_kernel<0>, rows, block, 0, st, *w);
  if (a->beam <= 16)  // beam^2 candidates, 256 NK of them in registers
    hipLaunchKernelGGL(tdg::beam_merge_kernel<1>, dim3(a->B), block, 0, st, *w);
  else if (a->beam <= 32)
    hipLaunchKernelGGL(tdg::beam_merge_kernel<4>, dim3(a->B), block, 0, st, *w);
  else
    hipLaunchKernelGGL(tdg::beam_merge_kernel<16>, dim3(a->B), block, 0, st, *w);
  return 0;
}

}  // extern "C"
