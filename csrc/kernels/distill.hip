// Word-level knowledge distillation loss (Kim & Rush 2016), forward and
// backward in one launch over the student's logits (gfx950).
//
// Per non-PAD row r (one 256-thread workgroup), with p = softmax(x[r, :V]),
// lse = logsumexp(x[r, :V]) and T teachers z_m of weights w_m (sum 1):
//   q      = sum_m w_m softmax(z_m[r, :V])      (the mean the ensemble decodes with)
//   target = (1 - alpha) ((1 - s) onehot(label) + s / V) + alpha q
//   row_label   = (1 - s)(lse - x_label) + s (lse - mean x)        (tdg_xent's row_loss)
//   row_loss    = (1 - alpha) row_label + alpha (lse - sum_v q[v] x[v])
//   row_correct = first-index argmax of x == label
//   dlogits     = (p - target) / (max(ntok, 1) workers)            (in place over x, bf16)
// PAD rows (label 0) give 0, 0, 0 and a zero gradient row; the columns
// [V, ldl) of the student are written as zero; teacher columns >= V never
// reach a result. A teacher's softmax is formed as exp((z - max) - (log sum -
// log w)): the difference of two bf16 logits is exact in f32, so q keeps the
// relative accuracy of exp where it is not negligible. The student's own
// probability is formed the same way, exp((x - max) - log sum), where xent.hip
// forms exp(x - lse): the two kernels share their steps (tdg_vocab_row.h), not
// their arithmetic, and stay two kernels.
#include "tdg_api.h"
#include "tdg_common.h"
#include "tdg_vocab_row.h"

namespace tdg {

// Register arm: padded rows of <= 256 * 8 * NCH columns, every row of the
// student and of the teachers on a 16-byte boundary. The student's NCH chunks
// per thread are loaded once and stay in registers; each teacher's row is
// loaded once, reduced to (max, log sum-exp) with one block reduction, and
// added into the f32 mixture q, which stays in registers too (8 * NCH per
// thread). Loss, argmax and gradient then come from registers: the student
// row is read once and written once (write-through), a teacher row read once.
template <typename LabT, int NCH>
__global__ __launch_bounds__(256) void distill_reg_kernel(const DistillArgs a) {
  __shared__ float t_m[DISTILL_MAX][4], t_s[DISTILL_MAX][4];
  __shared__ float r_m[4], r_x[4], r_s[4], r_q[4];
  __shared__ int r_i[4];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ldl = a.ldl, nch = ldl >> 3;
  bf16_t* x = a.x + (size_t)row * ldl;
  const int lab = (int)static_cast<const LabT*>(a.labels)[row];
  const bool valid = lab != 0;
  const float alpha = a.alpha, smoothing = a.smoothing;
  const bool mix = valid && alpha > 0.f;  // the same in every thread of the row
  short8_t raw[NCH];
  TDG_REG_LOAD(raw, x, nch)
  const float xl = bf2f(x[min(max(lab, 0), V - 1)]);  // read before any thread overwrites the row

  float q[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) q[k][e] = 0.f;
  if (mix) {
    for (int t = 0; t < a.T; ++t) {
      const bf16_t* z = a.t.x[t] + (size_t)row * a.t.ld[t];
      short8_t tr[NCH];
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c0 = 8 * (tid + 256 * k);  // c0 < V: the chunk ends inside the row (ldt % 8 == 0, ldt >= V)
        if (c0 < V) tr[k] = *reinterpret_cast<const short8_t*>(z + c0);
      }
      float tm = -INFINITY, ts = 0.f;
      TDG_REG_COLUMNS(tr, tm = fmaxf(tm, v);)
      TDG_REG_COLUMNS(tr, ts += __expf(v - tm);)
      wave_merge(tm, ts);
      if (lane == 0) { t_m[t][w] = tm; t_s[t][w] = ts; }
      __syncthreads();  // slots of teacher t are written once: no second barrier
      tm = t_m[t][0]; ts = t_s[t][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) merge(tm, ts, t_m[t][k], t_s[t][k]);
      const float off = __logf(ts) - a.t.logw[t];
      TDG_REG_COLUMNS(tr, q[k][e] += __expf((v - tm) - off);)
    }
  }

  // student: max + first argmax + sum of logits, then sum-exp and sum q x
  float m = -INFINITY, sumx = 0.f;
  int bi = NO_CAND;
  TDG_REG_MAX_SUMX(raw, m, bi, sumx, r_m, r_i, r_x)
  float se = 0.f, qx = 0.f;
  TDG_REG_COLUMNS(raw, se += __expf(v - m); qx += q[k][e] * v;)
  se = wave_sum(se);
  qx = wave_sum(qx);
  if (lane == 0) { r_s[w] = se; r_q[w] = qx; }
  __syncthreads();
  // p = exp((x - max) - lsr): like the teachers' terms, not exp(x - lse)
  const float lsr = __logf(r_s[0] + r_s[1] + r_s[2] + r_s[3]);
  const float lse = m + lsr;
  if (tid == 0) {
    float lab_loss = 0.f, loss = 0.f;
    if (valid) {
      lab_loss = label_loss(lse, xl, sumx, V, smoothing);
      loss = lab_loss;
      if (mix) loss = (1.f - alpha) * lab_loss + alpha * (lse - ((r_q[0] + r_q[1]) + (r_q[2] + r_q[3])));
    }
    a.row_loss[row] = loss;
    if (a.row_label) a.row_label[row] = lab_loss;
    a.row_correct[row] = (valid && bi == lab) ? 1.f : 0.f;
  }
  if (!a.write_grad) return;
  const float scale = valid ? 1.f / (fmaxf(a.ntok[0], 1.f) * a.workers) : 0.f;
  const float oma = 1.f - alpha;
  const float off = smoothing / (float)V;
  const WtBuf wt(a.x, (size_t)gridDim.x * ldl * sizeof(bf16_t));  // one row per block
  TDG_REG_STORE_GRAD(raw, x, nch, wt, valid,
                     (__expf((v - m) - lsr) - oma * (off + (c == lab ? 1.f - smoothing : 0.f)) -
                      alpha * q[k][e]) * scale)
}

// Generic arm: any row stride and any (2-byte) alignment of the student and
// of the teachers, rows of any length; element-wise passes over the
// L2-resident rows: the student's online softmax statistics, each teacher's,
// sum q x, and the gradient (which forms q a second time).
template <typename LabT>
__global__ __launch_bounds__(256) void distill_kernel(const DistillArgs a) {
  __shared__ float sm[4], ss[4], sv[4], sx[4], sq[4];
  __shared__ int si[4];
  __shared__ float t_m[DISTILL_MAX][4], t_s[DISTILL_MAX][4], t_max[DISTILL_MAX], t_off[DISTILL_MAX];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, ldl = a.ldl, T = a.T;
  bf16_t* x = a.x + (size_t)row * ldl;
  const int lab = (int)static_cast<const LabT*>(a.labels)[row];
  const bool valid = lab != 0;
  const float alpha = a.alpha, smoothing = a.smoothing;
  const bool mix = valid && alpha > 0.f;  // the same in every thread of the row
  const float xl = bf2f(x[min(max(lab, 0), V - 1)]);  // read before any thread overwrites the row

  float m = -INFINITY, s = 0.f, bv = -INFINITY, sumx = 0.f;
  int bi = NO_CAND;
  for (int c = tid; c < V; c += 256) {
    const float v = bf2f(x[c]);
    if (v > m) {
      s *= __expf(m - v);
      m = v;
    }
    s += __expf(v - m);
    sumx += v;
    if (v > bv) { bv = v; bi = c; }
  }
  TDG_ROW_WAVE_REDUCE(m, s, bv, bi, sumx)
  if (lane == 0) { sm[w] = m; ss[w] = s; sv[w] = bv; si[w] = bi; sx[w] = sumx; }
  if (mix) {
    for (int t = 0; t < T; ++t) {
      const bf16_t* z = a.t.x[t] + (size_t)row * a.t.ld[t];
      float tm = -INFINITY, ts = 0.f;
      for (int c = tid; c < V; c += 256) {
        const float v = bf2f(z[c]);
        if (v > tm) {
          ts *= __expf(tm - v);
          tm = v;
        }
        ts += __expf(v - tm);
      }
      wave_merge(tm, ts);
      if (lane == 0) { t_m[t][w] = tm; t_s[t][w] = ts; }
    }
  }
  __syncthreads();  // every read of x above is done; the partials are visible
  TDG_ROW_BLOCK_FOLD(m, s, bv, bi, sumx, sm, ss, sv, si, sx)
  const float lsr = __logf(s);
  const float lse = m + lsr;
  float qsum = 0.f;
  if (mix) {
    if (tid < T) {
      float tm = t_m[tid][0], ts = t_s[tid][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) merge(tm, ts, t_m[tid][k], t_s[tid][k]);
      t_max[tid] = tm;
      t_off[tid] = __logf(ts) - a.t.logw[tid];
    }
    __syncthreads();
    float qx = 0.f;
    for (int c = tid; c < V; c += 256) {
      float qv = 0.f;
      for (int t = 0; t < T; ++t)
        qv += __expf((bf2f(a.t.x[t][(size_t)row * a.t.ld[t] + c]) - t_max[t]) - t_off[t]);
      qx += qv * bf2f(x[c]);
    }
    qx = wave_sum(qx);
    if (lane == 0) sq[w] = qx;
    __syncthreads();  // every read of x is done
    qsum = (sq[0] + sq[1]) + (sq[2] + sq[3]);
  }
  if (tid == 0) {
    float lab_loss = 0.f, loss = 0.f;
    if (valid) {
      lab_loss = label_loss(lse, xl, sumx, V, smoothing);
      loss = mix ? (1.f - alpha) * lab_loss + alpha * (lse - qsum) : lab_loss;
    }
    a.row_loss[row] = loss;
    if (a.row_label) a.row_label[row] = lab_loss;
    a.row_correct[row] = (valid && bi == lab) ? 1.f : 0.f;
  }
  if (!a.write_grad) return;
  const float scale = valid ? 1.f / (fmaxf(a.ntok[0], 1.f) * a.workers) : 0.f;
  const float oma = 1.f - alpha;
  const float off = smoothing / (float)V;
  for (int c = tid; c < ldl; c += 256) {  // a thread reads and writes its own columns only
    float g = 0.f;
    if (c < V && valid) {
      float qv = 0.f;
      if (mix)
        for (int t = 0; t < T; ++t)
          qv += __expf((bf2f(a.t.x[t][(size_t)row * a.t.ld[t] + c]) - t_max[t]) - t_off[t]);
      g = (__expf((bf2f(x[c]) - m) - lsr) - oma * (off + (c == lab ? 1.f - smoothing : 0.f)) - alpha * qv) *
          scale;
    }
    x[c] = f2bf(g);
  }
}

}  // namespace tdg

// The distillation loss of M rows (tdg_distill.h DistillArgs; the formulas
// are at the head of this file). Register arm: ldl % 8 == 0, ldl <= 8192, a
// 16-byte aligned student, and every teacher 16-byte aligned with
// ldt % 8 == 0; the generic arm otherwise. alpha == 0 reads no teacher.
// -1: T outside [1, 8], V outside [1, 65536] or alpha outside [0, 1];
// -2: a row shorter than V; nothing launched.
extern "C" int tdg_xent_distill(const tdg::DistillArgs* a, hipStream_t st) {
  if (a->T < 1 || a->T > tdg::DISTILL_MAX || a->V < 1 || a->V > 65536 ||
      !(a->alpha >= 0.f && a->alpha <= 1.f))
    return -1;
  if (a->ldl < a->V) return -2;
  bool reg = a->ldl % 8 == 0 && a->ldl <= 256 * 8 * 4 && (reinterpret_cast<uintptr_t>(a->x) & 15) == 0;
  for (int t = 0; t < a->T; ++t) {
    if (a->t.ld[t] < a->V || !a->t.x[t]) return -2;
    reg = reg && a->t.ld[t] % 8 == 0 && (reinterpret_cast<uintptr_t>(a->t.x[t]) & 15) == 0;
  }
  if (a->M <= 0) return 0;
  tdg::dispatch_labels(a->lab64, [&](auto l) {
    using LabT = decltype(l);
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(a->M), dim3(256), 0, st, *a); };
    if (reg)
      tdg::dispatch_upto<4>(tdg::cdiv(a->ldl / 8, 256),
                            [&](auto n) { launch(tdg::distill_reg_kernel<LabT, decltype(n)::value>); });
    else
      launch(tdg::distill_kernel<LabT>);
  });
  return 0;
}
