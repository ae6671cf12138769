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
// relative accuracy of exp where it is not negligible.
#include "tdg_api.h"
#include "tdg_common.h"
#include "tdg_rowloss.h"

namespace tdg {

// (m, s) of the whole wave in every lane
__device__ __forceinline__ void wave_merge(float& m, float& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    merge(m, s, m2, s2);
  }
}

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
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int ch = tid + 256 * k;
    if (ch < nch) raw[k] = *reinterpret_cast<const short8_t*>(x + 8 * ch);
  }
  const float xl = bf2f(x[min(max(lab, 0), V - 1)]);  // read before any thread overwrites the row

  float q[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) q[k][e] = 0.f;
  if (mix) {
    for (int t = 0; t < a.T; ++t) {
      const bf16_t* z = a.t[t] + (size_t)row * a.ldt[t];
      short8_t tr[NCH];
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c0 = 8 * (tid + 256 * k);  // c0 < V: the chunk ends inside the row (ldt % 8 == 0, ldt >= V)
        if (c0 < V) tr[k] = *reinterpret_cast<const short8_t*>(z + c0);
      }
      float tm = -INFINITY, ts = 0.f;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c0 = 8 * (tid + 256 * k);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c0 + e < V) tm = fmaxf(tm, bf2f((bf16_t)tr[k][e]));
      }
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c0 = 8 * (tid + 256 * k);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c0 + e < V) ts += __expf(bf2f((bf16_t)tr[k][e]) - tm);
      }
      wave_merge(tm, ts);
      if (lane == 0) { t_m[t][w] = tm; t_s[t][w] = ts; }
      __syncthreads();  // slots of teacher t are written once: no second barrier
      tm = t_m[t][0]; ts = t_s[t][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) merge(tm, ts, t_m[t][k], t_s[t][k]);
      const float off = __logf(ts) - a.logw[t];
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c0 = 8 * (tid + 256 * k);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c0 + e < V) q[k][e] += __expf((bf2f((bf16_t)tr[k][e]) - tm) - off);
      }
    }
  }

  // student: max + first argmax + sum of logits, then sum-exp and sum q x
  float m = -INFINITY, sumx = 0.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c0 = 8 * (tid + 256 * k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (c0 + e < V) {
        const float v = bf2f((bf16_t)raw[k][e]);
        sumx += v;
        if (v > m) { m = v; bi = c0 + e; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    TDG_ARGMAX_TAKE(m, bi, m2, i2)
    sumx += __shfl_xor(sumx, o, 64);
  }
  if (lane == 0) { r_m[w] = m; r_i[w] = bi; r_x[w] = sumx; }
  __syncthreads();
  m = r_m[0]; bi = r_i[0]; sumx = r_x[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    TDG_ARGMAX_TAKE(m, bi, r_m[k], r_i[k])
    sumx += r_x[k];
  }
  float se = 0.f, qx = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c0 = 8 * (tid + 256 * k);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (c0 + e < V) {
        const float v = bf2f((bf16_t)raw[k][e]);
        se += __expf(v - m);
        qx += q[k][e] * v;
      }
  }
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
      lab_loss = (1.f - smoothing) * (lse - xl) + smoothing * (lse - sumx / (float)V);
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
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int ch = tid + 256 * k;
    if (ch >= nch) continue;
    const int c0 = 8 * ch;
    short8_t g;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      float gv = 0.f;
      if (c < V && valid)
        gv = (__expf((bf2f((bf16_t)raw[k][e]) - m) - lsr) -
              oma * (off + (c == lab ? 1.f - smoothing : 0.f)) - alpha * q[k][e]) * scale;
      g[e] = pack_bf(gv);
    }
    wt.st16(x + c0, g);
  }
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
  int bi = 0x7fffffff;
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
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    merge(m, s, m2, s2);
    sumx += __shfl_xor(sumx, o, 64);
    const float bv2 = __shfl_xor(bv, o, 64);
    const int bi2 = __shfl_xor(bi, o, 64);
    TDG_ARGMAX_TAKE(bv, bi, bv2, bi2)
  }
  if (lane == 0) { sm[w] = m; ss[w] = s; sv[w] = bv; si[w] = bi; sx[w] = sumx; }
  if (mix) {
    for (int t = 0; t < T; ++t) {
      const bf16_t* z = a.t[t] + (size_t)row * a.ldt[t];
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
  m = sm[0]; s = ss[0]; bv = sv[0]; bi = si[0]; sumx = sx[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    merge(m, s, sm[k], ss[k]);
    sumx += sx[k];
    TDG_ARGMAX_TAKE(bv, bi, sv[k], si[k])
  }
  const float lsr = __logf(s);
  const float lse = m + lsr;
  float qsum = 0.f;
  if (mix) {
    if (tid < T) {
      float tm = t_m[tid][0], ts = t_s[tid][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) merge(tm, ts, t_m[tid][k], t_s[tid][k]);
      t_max[tid] = tm;
      t_off[tid] = __logf(ts) - a.logw[tid];
    }
    __syncthreads();
    float qx = 0.f;
    for (int c = tid; c < V; c += 256) {
      float qv = 0.f;
      for (int t = 0; t < T; ++t)
        qv += __expf((bf2f(a.t[t][(size_t)row * a.ldt[t] + c]) - t_max[t]) - t_off[t]);
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
      lab_loss = (1.f - smoothing) * (lse - xl) + smoothing * (lse - sumx / (float)V);
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
          qv += __expf((bf2f(a.t[t][(size_t)row * a.ldt[t] + c]) - t_max[t]) - t_off[t]);
      g = (__expf((bf2f(x[c]) - m) - lsr) - oma * (off + (c == lab ? 1.f - smoothing : 0.f)) - alpha * qv) *
          scale;
    }
    x[c] = f2bf(g);
  }
}

template <typename LabT>
static void launch_distill(const DistillArgs& a, bool reg, hipStream_t st) {
  const dim3 grid(a.M), block(256);
  if (reg) {
    const int nch = cdiv(a.ldl / 8, 256);
    if (nch <= 1)
      hipLaunchKernelGGL((distill_reg_kernel<LabT, 1>), grid, block, 0, st, a);
    else if (nch == 2)
      hipLaunchKernelGGL((distill_reg_kernel<LabT, 2>), grid, block, 0, st, a);
    else if (nch == 3)
      hipLaunchKernelGGL((distill_reg_kernel<LabT, 3>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((distill_reg_kernel<LabT, 4>), grid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL(distill_kernel<LabT>, grid, block, 0, st, a);
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
    if (a->ldt[t] < a->V || !a->t[t]) return -2;
    reg = reg && a->ldt[t] % 8 == 0 && (reinterpret_cast<uintptr_t>(a->t[t]) & 15) == 0;
  }
  if (a->M <= 0) return 0;
  if (a->lab64)
    tdg::launch_distill<long long>(*a, reg, st);
  else
    tdg::launch_distill<int>(*a, reg, st);
  return 0;
}
