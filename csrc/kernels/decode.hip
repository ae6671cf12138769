// Decoding kernels (gfx950): single-query attention over an indexed K/V cache
// the beam-search selection step, the sampling step, the ensemble's
// probability average and teacher-forced scoring under it. Used by
// infer/step.py, infer/beam.py, infer/sample.py and infer/score.py.
//
// decode_attn: M = 1 per (row, head), so there is no matrix to feed the MFMA
// units: the kernel is a stream over the keys. One wave per (row, head), four
// per workgroup, no LDS. hd / 8 lanes share a key (one 16-byte load of K and
// one of V each), so a wave covers 64 / (hd / 8) keys per pass. Every lane
// group keeps its own online softmax (running max, sum and f32 accumulator of
// its keys; P is never rounded); the groups are merged once at the end.
// Which cache row holds key j of row r comes from the ancestry table
// (anc[r][j]) or, without one, from row_map[r]: beams never reorder a cache,
// and the encoder K/V exist once per sentence.
//
// beam_topk: one workgroup per sentence. Per live row the f32 logsumexp of the
// logits, then every thread keeps the best `beam` of the candidates it scans
// (score[r] + logp[r, v], ordered by value, ties to the lower flat index
// r_local * V + v) and the workgroup merges the lists with `beam` arg-max
// rounds. The same launch advances the ancestry table.
//
// sample_token: one workgroup per row. The thresholds of top-k and top-p are
// found by bisection on the 16-bit order-preserving key of a bf16 value (16
// passes each of a workgroup-wide count or mass of {key >= mid}; a row of up
// to 8192 columns stays in registers, a longer one, at most 128 KiB, is
// re-read from L2), the draw is a Gumbel-max over the kept set: no sort, no
// prefix sums, every reduction in a fixed order.
//
// ensemble_logprobs: one workgroup per row. Pass 1 streams the row of every
// member once, each thread keeping an online (max, sum) pair per member; the
// pairs are reduced over the workgroup in a fixed order (no atomics). Pass 2
// re-reads the rows (at most 8 x 128 KiB, from L2) and stores the log of the
// weighted mean probability, 16 bytes at a time. The members' pointers ride
// in the argument block: nothing to upload before a launch.
//
// score_tokens: the same stream without the V-wide store. Pass 1 is
// ensemble_logprobs' own (one function, member_offsets); one thread then forms
// the label's mixture value from M scalar loads. The row's largest mixture
// value, where asked for, is max - lse for one member and for more a second
// pass from L2 that keeps a per-thread max, reduced in a fixed order. The
// label's column and every other go through one expression (mix_column), so
// tok_lp >= top_lp is exact. A row whose label is pad_id leaves before its
// first load.
//
// The block reductions, the candidate order and its workgroup arg-best, the
// 8-value bf16 unpack / pack and the mixture's column load are
// tdg_vocab_row.h's, shared with xent.hip and distill.hip.
#include "tdg_api.h"
#include "tdg_vocab_row.h"

namespace tdg {

// ---------------------------------------------------------------- decode_attn
template <int HD>
__global__ __launch_bounds__(256) void decode_attn_kernel(const DecodeAttnArgs a) {
  constexpr int LPK = HD / 8;    // lanes per key (8 bf16 = 16 bytes each)
  constexpr int KPW = 64 / LPK;  // keys per wave pass
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= a.R * a.H) return;  // whole waves leave
  const int r = pair / a.H, h = pair - r * a.H;
  const int g = lane / LPK, e0 = (lane % LPK) * 8;
  uint16_t* const orow = a.out + (long long)r * a.o_sr + h * a.o_sh + e0;
  const int n = min(a.kv_len[r], a.Lk);
  if (n < 1) {  // outside the precondition: defined as zeros, nothing read
    if (lane < LPK) *reinterpret_cast<uint4*>(orow) = make_uint4(0, 0, 0, 0);
    return;
  }
  float q[8];
  {
    const uint4 w = *reinterpret_cast<const uint4*>(a.q + (long long)r * a.q_sr + h * a.q_sh + e0);
    unpack8(w, q);
    const float sc = a.scale * 1.44269504088896f;  // softmax in base 2
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] *= sc;
  }
  const bool fused = a.k_new != nullptr;
  const int t = n - 1;
  int own = r;
  if (a.anc == nullptr && a.row_map != nullptr) own = a.row_map[r];
  own = min(max(own, 0), a.n_src - 1);
  const int* const anc = a.anc ? a.anc + (long long)r * a.ld_anc : nullptr;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  for (int j0 = 0; j0 < n; j0 += KPW) {
    const int j = j0 + g;
    const bool valid = j < n;
    uint4 kw = make_uint4(0, 0, 0, 0), vw = kw;
    if (valid) {
      if (fused && j == t) {
        // the new key: from the projection's output, and into the cache
        kw = *reinterpret_cast<const uint4*>(a.k_new + (long long)r * a.kn_sr + h * a.kn_sh + e0);
        vw = *reinterpret_cast<const uint4*>(a.v_new + (long long)r * a.vn_sr + h * a.vn_sh + e0);
        *reinterpret_cast<uint4*>(a.k + r * a.k_sr + t * a.k_sk + h * a.k_sh + e0) = kw;
        *reinterpret_cast<uint4*>(a.v + r * a.v_sr + t * a.v_sk + h * a.v_sh + e0) = vw;
      } else {
        int src = own;
        if (anc) src = min(max(anc[j], 0), a.n_src - 1);
        kw = *reinterpret_cast<const uint4*>(a.k + src * a.k_sr + j * a.k_sk + h * a.k_sh + e0);
        vw = *reinterpret_cast<const uint4*>(a.v + src * a.v_sr + j * a.v_sk + h * a.v_sh + e0);
      }
    }
    float kf[8], s = 0.f;
    unpack8(kw, kf);
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(q[i], kf[i], s);
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o);
    if (valid) {
      float vf[8];
      unpack8(vw, vf);
      const float mn = fmaxf(m, s);
      const float alpha = exp2f(m - mn), p = exp2f(s - mn);
      m = mn;
      l = l * alpha + p;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = acc[i] * alpha + p * vf[i];
    }
  }
  // merge the lane groups: rescale to the wave's max, then sum lanes of equal
  // slice across the groups (m = -inf, a group without keys, scales to 0)
  const float f = exp2f(m - wave_max(m));
  l *= f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] *= f;
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    l += __shfl_xor(l, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], o);
  }
  if (lane < LPK) {
    const float inv = 1.f / l;
    *reinterpret_cast<uint4*>(orow) = pack8bf(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv,
                                              acc[4] * inv, acc[5] * inv, acc[6] * inv, acc[7] * inv);
  }
}

// ---------------------------------------------------------------- beam_topk
template <int BEAM>
__global__ __launch_bounds__(256) void beam_topk_kernel(const BeamTopkArgs a) {
  __shared__ float red[4];
  __shared__ int redi[4];
  __shared__ int s_parent[BEAM];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * BEAM;
  const int V = a.V;

  float lv[BEAM];  // this thread's best candidates, best first
  int li[BEAM];
#pragma unroll
  for (int i = 0; i < BEAM; ++i) {
    lv[i] = -INFINITY;
    li[i] = NO_CAND;
  }
  auto offer = [&](float cv, int ci) {
    if (!better(cv, ci, lv[BEAM - 1], li[BEAM - 1])) return;
#pragma unroll
    for (int i = 0; i < BEAM; ++i) {
      if (better(cv, ci, lv[i], li[i])) {
        const float tv = lv[i];
        const int ti = li[i];
        lv[i] = cv;
        li[i] = ci;
        cv = tv;
        ci = ti;
      }
    }
  };

  for (int b = 0; b < BEAM; ++b) {  // every branch below is workgroup-uniform
    const int r = r0 + b;
    const float sc = a.score[r];
    if (!(sc > -INFINITY)) continue;  // a dead slot (or NaN) offers nothing
    if (a.fin[r]) {                   // ended: itself, once, score unchanged
      if (tid == 0) offer(sc, b * V + a.pad_id);
      continue;
    }
    const uint16_t* x = a.logits + (long long)r * a.ldl;
    float mx = -INFINITY;
    for (int c = tid * 8; c < V; c += 2048) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + c), f);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c + i < V) mx = fmaxf(mx, f[i]);
    }
    mx = block_max(mx, red);
    if (!(mx > -INFINITY)) continue;  // no finite logit
    float sum = 0.f;
    for (int c = tid * 8; c < V; c += 2048) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + c), f);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c + i < V) sum += __expf(f[i] - mx);
    }
    const float lse = mx + logf(block_sum(sum, red));
    for (int c = tid * 8; c < V; c += 2048) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + c), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float cv = sc + (f[i] - lse);
        if (c + i < V && cv > -INFINITY) offer(cv, b * V + c + i);
      }
    }
  }

  // merge: BEAM rounds of workgroup arg-max over the lists' heads
  for (int k = 0; k < BEAM; ++k) {
    float bv = lv[0];
    int bi = li[0];
    TDG_ARGBEST_WAVES(bv, bi, red, redi)
    bv = red[0];
    bi = redi[0];
    TDG_ARGBEST_FOLD(bv, bi, red, redi)
    __syncthreads();
    if (bi != NO_CAND && li[0] == bi) {  // the winner's owner moves on
#pragma unroll
      for (int i = 0; i + 1 < BEAM; ++i) {
        lv[i] = lv[i + 1];
        li[i] = li[i + 1];
      }
      lv[BEAM - 1] = -INFINITY;
      li[BEAM - 1] = NO_CAND;
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
  const int w = a.t + 2;
  for (int i = tid; i < BEAM * w; i += 256) {
    const int b = i / w, j = i - b * w;
    a.anc_out[(long long)(r0 + b) * a.ld_anc + j] =
        j <= a.t ? a.anc_in[(long long)s_parent[b] * a.ld_anc + j] : r0 + b;
  }
}

// ---------------------------------------------------------------- sample_token
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

template <int NCH>
__global__ __launch_bounds__(256) void sample_token_kernel(const SampleArgs a) {
  __shared__ float red[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
  const float sc = a.score[r];
  auto put = [&](int tok, float s, int fin) {
    if (tid == 0) {
      a.token[r] = tok;
      a.score_out[r] = s;
      a.fin_out[r] = fin;
    }
  };
  // every branch below is workgroup-uniform
  if (a.fin[r]) return put(a.pad_id, sc, 1);
  const uint16_t* x = a.logits + (long long)r * a.ldl;
  RowRegs<NCH> row;
  row.load(x, V);
  float mx = -INFINITY, cnt = 0.f;
  row.scan(x, V, [&](float f, int) {
    if (f > -INFINITY) {
      mx = fmaxf(mx, f);
      cnt += 1.f;
    }
  });
  mx = block_max(mx, red);
  if (!(sc > -INFINITY) || !(mx > -INFINITY)) return put(a.pad_id, -INFINITY, 1);
  const int nfin = (int)block_sum(cnt, red);  // counts are exact in f32
  float sum = 0.f;
  row.scan(x, V, [&](float f, int) {
    if (f > -INFINITY) sum += __expf(f - mx);
  });
  const float lse = mx + logf(block_sum(sum, red));

  // tau_k: the largest key t with |{key >= t}| >= top_k, a bit per pass
  uint32_t tk = KEY_MIN;
  if (a.top_k > 0 && a.top_k < nfin) {
    const float need = (float)a.top_k;
    uint32_t t = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = t | (1u << bit);
      float c = 0.f;
      row.scan(x, V, [&](float f, int) { c += okey(f) >= cand ? 1.f : 0.f; });
      if (block_sum(c, red) >= need) t = cand;
    }
    tk = t;
  }
  // tau_p: the largest key t whose mass inside K reaches top_p of K's. While
  // cand <= tk a pass sums the very set of the total, in the same order. A row
  // in registers keeps its weights there too (0 outside K).
  const float T = a.temperature;
  uint32_t ts = tk;
  if (a.top_p < 1.f) {
    float wt[NCH > 0 ? 8 * NCH : 1];
    if constexpr (NCH > 0)
      row.scan(x, V, [&](float f, int slot) { wt[slot] = okey(f) >= tk ? expf((f - mx) / T) : 0.f; });
    auto mass = [&](uint32_t lo) {  // of {key >= lo}, lo >= tk
      float m = 0.f;
      row.scan(x, V, [&](float f, int slot) {
        if (okey(f) >= lo) {
          if constexpr (NCH > 0)
            m += wt[slot];
          else
            m += expf((f - mx) / T);
        }
      });
      return block_sum(m, red);
    };
    const float need = a.top_p * mass(tk);
    uint32_t t = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = t | (1u << bit);
      if (mass(max(cand, tk)) >= need) t = cand;
    }
    ts = max(t, tk);
  }

  // Gumbel-max over S = {key >= ts}: one Philox call per four columns
  const uint32_t rid = a.row_id ? (uint32_t)a.row_id[r] : (uint32_t)r;
  float bv = -INFINITY;
  int bi = NO_CAND;
  row.chunks(x, V, [&](int c, const float* e, int) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bool any = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) any |= c + 4 * h + i < V && okey(e[4 * h + i]) >= ts;
      if (!any) continue;
      uint32_t w[4];
      Philox::gen(a.seed, a.step, ((uint64_t)rid << 32) | (uint32_t)((c >> 2) + h), w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = c + 4 * h + i;
        const float f = e[4 * h + i];
        if (v < V && okey(f) >= ts) {
          const float u = ((float)(w[i] >> 9) + 0.5f) * 0x1p-23f;  // exact, in (0, 1)
          const float key = f / T - logf(-logf(u));
          if (better(key, v, bv, bi)) {
            bv = key;
            bi = v;
          }
        }
      }
    }
  });
  TDG_ARGBEST_WAVES(bv, bi, red, redi)
  if (tid == 0) {
    TDG_ARGBEST_FOLD(bv, bi, red, redi)
    if (bi == NO_CAND) {  // no comparable key (NaN logits or temperature): a dead row
      put(a.pad_id, -INFINITY, 1);
    } else {
      const float xt = __uint_as_float((uint32_t)x[bi] << 16);
      put(bi, sc + (xt - lse), bi == a.end_id ? 1 : 0);
    }
  }
}

// ---------------------------------------------------------------- ensemble_logprobs, score_tokens
// Pass 1 of both kernels: per member the row's logsumexp over its finite
// logits, an online (max, sum) pair per thread and member reduced over the
// workgroup in a fixed order. gm[m]: the row's largest finite logit (-inf: none);
// off[m] = log w_m - lse_m, -inf for a member without a finite logit in the
// row. Ends past its last barrier: `red` is free again after one more.
template <int M>
__device__ __forceinline__ void member_offsets(const uint16_t* (&x)[M],
                                               const float (&logw)[ENSEMBLE_MAX], int V,
                                               float (&red)[ENSEMBLE_MAX][4], float (&gm)[M],
                                               float (&off)[M]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mx[M], sum[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    mx[m] = -INFINITY;
    sum[m] = 0.f;
  }
  for (int c = tid * 8; c < V; c += 2048) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x[m] + c), f);
      float cm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!(c + i < V && f[i] > -INFINITY)) f[i] = -INFINITY;  // padding, -inf, NaN: probability 0
        cm = fmaxf(cm, f[i]);
      }
      if (cm > mx[m]) {  // one rescale per chunk of 8
        sum[m] *= __expf(mx[m] - cm);
        mx[m] = cm;
      }
      if (mx[m] > -INFINITY) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sum[m] += __expf(f[i] - mx[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float w = wave_max(mx[m]);
    if (lane == 0) red[m][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) gm[m] = fmaxf(fmaxf(red[m][0], red[m][1]), fmaxf(red[m][2], red[m][3]));
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float w = wave_sum(mx[m] > -INFINITY ? sum[m] * __expf(mx[m] - gm[m]) : 0.f);
    if (lane == 0) red[m][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float tot = (red[m][0] + red[m][1]) + (red[m][2] + red[m][3]);
    off[m] = gm[m] > -INFINITY ? logw[m] - (gm[m] + logf(tot)) : -INFINITY;
  }
}

// One column of the mixture: log sum_m exp(am(m)), am(m) = x_m + off_m or -inf
// for a logit of probability 0; -inf where every member has none.
template <int M, class A>
__device__ __forceinline__ float mix_column(A am) {
  float top = am(0);
#pragma unroll
  for (int m = 1; m < M; ++m) top = fmaxf(top, am(m));
  float s = 0.f;
  if (top > -INFINITY) {
#pragma unroll
    for (int m = 0; m < M; ++m) s += __expf(am(m) - top);
  }
  return top > -INFINITY ? top + logf(s) : -INFINITY;
}

template <int M>
__global__ __launch_bounds__(256) void ensemble_logprobs_kernel(const EnsembleArgs a) {
  __shared__ float red[ENSEMBLE_MAX][4];
  const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
  const uint16_t* x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = a.mem.x[m] + (long long)r * a.mem.ld[m];

  float gm[M], off[M];
  member_offsets<M>(x, a.mem.logw, V, red, gm, off);

  // pass 2: out = log sum_m exp(x_m + off_m); the columns [V, No) get -inf
  uint16_t* const orow = a.out + (long long)r * a.ldo;
  for (int c = tid * 8; c < a.No; c += 2048) {
    float am[M][8], o[8];
    if (c < V) {
      TDG_MIX_LOAD(am, x, off, c)
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = mix_column<M>([&](int m) { return am[m][i]; });
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = -INFINITY;
    }
    *reinterpret_cast<uint4*>(orow + c) = pack8bf(o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
  }
}

template <int M>
__global__ __launch_bounds__(256) void score_tokens_kernel(const ScoreArgs a) {
  __shared__ float red[ENSEMBLE_MAX][4];
  const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
  // every branch below is workgroup-uniform
  const long long lab = a.lab64 ? static_cast<const long long*>(a.labels)[r]
                                : static_cast<const int*>(a.labels)[r];
  if (lab == a.pad_id) {  // an ignored row: no logit is read
    if (tid == 0) {
      a.tok_lp[r] = 0.f;
      if (a.top_lp) a.top_lp[r] = 0.f;
    }
    return;
  }
  const uint16_t* x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = a.mem.x[m] + (long long)r * a.mem.ld[m];

  float gm[M], off[M];
  member_offsets<M>(x, a.mem.logw, V, red, gm, off);

  if (tid == 0) {  // the label's column: M scalar loads
    float t = -INFINITY;
    if (lab >= 0 && lab < V) {
      float am[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float f = __uint_as_float((uint32_t)x[m][lab] << 16);
        am[m] = f > -INFINITY ? f + off[m] : -INFINITY;
      }
      t = mix_column<M>([&](int m) { return am[m]; });
    }
    a.tok_lp[r] = t;
  }
  if (a.top_lp == nullptr) return;
  if constexpr (M == 1) {
    // x + off grows with x: the largest column is the largest logit's
    if (tid == 0) {
      const float am = gm[0] > -INFINITY ? gm[0] + off[0] : -INFINITY;
      a.top_lp[r] = mix_column<1>([&](int) { return am; });
    }
  } else {
    // pass 2 (rows from L2): the largest mixture value, nothing stored
    float best = -INFINITY;
    for (int c = tid * 8; c < V; c += 2048) {
      float am[M][8];
      TDG_MIX_LOAD(am, x, off, c)
#pragma unroll
      for (int i = 0; i < 8; ++i) best = fmaxf(best, mix_column<M>([&](int m) { return am[m][i]; }));
    }
    __syncthreads();  // member_offsets' last reads of red
    best = block_max(best, red[0]);
    if (tid == 0) a.top_lp[r] = best;
  }
}

}  // namespace tdg

extern "C" {

// out[r, h, :] = softmax(scale * q[r, h] . K[row(r, j), j, h] for j < kv_len[r]) @ V,
// row(r, j) = anc[r][j], else row_map[r], else r; with k_new / v_new the new
// key is stored to cache position kv_len[r] - 1 of row r and used from
// registers. kv_len[r] >= 1 (a row with none gets zeros). hd 16 or 64.
int tdg_decode_attn(const tdg::DecodeAttnArgs* a, int hd, hipStream_t st) {
  if (hd != 16 && hd != 64) return -1;
  if (a->R <= 0 || a->H <= 0) return 0;
  const dim3 grid(tdg::cdiv(a->R * a->H, 4)), block(256);
  if (hd == 64)
    hipLaunchKernelGGL(tdg::decode_attn_kernel<64>, grid, block, 0, st, *a);
  else
    hipLaunchKernelGGL(tdg::decode_attn_kernel<16>, grid, block, 0, st, *a);
  return 0;
}

// One beam-search step (tdg_decode.h BeamTopkArgs): per sentence the best
// `beam` of the candidates (r, v) -> score[r] + log_softmax(logits[r])[v];
// an ended row offers only (r, pad_id) with its score, a row of score -inf
// nothing. Slots come out by descending score, ties by the lower flat index;
// a slot with no candidate left gets score -inf, token pad_id, fin 1, parent
// = the sentence's first row. ldl % 8 == 0, 16-byte aligned logits.
int tdg_beam_topk(const tdg::BeamTopkArgs* a, hipStream_t st) {
  if (a->beam < 1 || a->beam > 8 || a->V < 1 || a->V > 65536) return -1;
  if (a->B <= 0) return 0;
  tdg::dispatch_upto<8>(a->beam, [&](auto n) {
    hipLaunchKernelGGL(tdg::beam_topk_kernel<decltype(n)::value>, dim3(a->B), dim3(256), 0, st, *a);
  });
  return 0;
}

// One sampling step (tdg_decode.h SampleArgs), a workgroup per row: keep the
// top_k largest logits (ties at the threshold all kept), of those the smallest
// top set whose softmax(x / T) mass reaches top_p, and draw by Gumbel-max with
// uniforms from Philox(seed, step, (row_id, v / 4)). score += the unfiltered
// log-softmax of the drawn token at T = 1. An ended row gives pad_id, its
// score and fin 1; a row of score -inf / NaN or without a finite logit
// pad_id, -inf, fin 1. ldl % 8 == 0, 16-byte aligned logits.
int tdg_sample_token(const tdg::SampleArgs* a, hipStream_t st) {
  if (a->V < 1 || a->V > 65536) return -1;
  if (a->R <= 0) return 0;
  const dim3 grid(a->R), block(256);
  if (a->V <= 2048)  // the row in registers: 1 or 4 chunks of 8 columns per thread
    hipLaunchKernelGGL(tdg::sample_token_kernel<1>, grid, block, 0, st, *a);
  else if (a->V <= 8192)
    hipLaunchKernelGGL(tdg::sample_token_kernel<4>, grid, block, 0, st, *a);
  else
    hipLaunchKernelGGL(tdg::sample_token_kernel<0>, grid, block, 0, st, *a);
  return 0;
}

// The log of the weighted mean of M members' next-token probabilities
// (tdg_decode.h EnsembleArgs), a workgroup per row: out[r, v] = log sum_m
// w_m softmax(x_m[r])[v] in f32, rounded to bf16; a NaN or -inf logit has
// probability 0, a member's row without a finite logit none at all, a row no
// member has a finite logit in is all -inf, as are the columns [V, No).
// ldl % 8 == 0, ldo % 8 == 0, No % 8 == 0, 16-byte aligned rows.
int tdg_ensemble_logprobs(const tdg::EnsembleArgs* a, hipStream_t st) {
  if (a->M < 1 || a->M > tdg::ENSEMBLE_MAX || a->V < 1 || a->V > 65536) return -1;
  if (a->R <= 0) return 0;
  tdg::dispatch_upto<tdg::ENSEMBLE_MAX>(a->M, [&](auto n) {
    hipLaunchKernelGGL(tdg::ensemble_logprobs_kernel<decltype(n)::value>, dim3(a->R), dim3(256), 0, st, *a);
  });
  return 0;
}

// Teacher-forced scores under that mixture (tdg_decode.h ScoreArgs), a
// workgroup per row: tok_lp[r] = mix[r, labels[r]] and, where wanted,
// top_lp[r] = max_v mix[r, v], both f32 and never rounded; nothing V-wide is
// stored. A row whose label is pad_id gets 0 for both without a logit read, a
// label outside [0, V) tok_lp -inf, a row no member has a finite logit in
// -inf for both. ldl % 8 == 0, 16-byte aligned rows.
int tdg_score_tokens(const tdg::ScoreArgs* a, hipStream_t st) {
  if (a->M < 1 || a->M > tdg::ENSEMBLE_MAX || a->V < 1 || a->V > 65536) return -1;
  if (a->R <= 0) return 0;
  tdg::dispatch_upto<tdg::ENSEMBLE_MAX>(a->M, [&](auto n) {
    hipLaunchKernelGGL(tdg::score_tokens_kernel<decltype(n)::value>, dim3(a->R), dim3(256), 0, st, *a);
  });
  return 0;
}

}  // extern "C"
