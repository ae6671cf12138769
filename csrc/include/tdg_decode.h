// Argument blocks of the decoding kernels (decode.hip), host <-> device.
#pragma once
#include <stdint.h>

namespace tdg {

// Single-query attention: one query per (row, head), keys reached through an
// index. All strides are in bf16 elements; every 8-element slice of a row
// lies on a 16-byte boundary.
struct DecodeAttnArgs {
  const uint16_t* q;  // [R, H, hd]
  uint16_t* out;      // [R, H, hd]
  uint16_t* k;        // [n_src, Lk, H, hd] (written only by the fused append)
  uint16_t* v;
  // fused append (both or neither): [R, H, hd], stored to cache position
  // kv_len[r] - 1 of row r and used as that key
  const uint16_t* k_new;
  const uint16_t* v_new;
  const int* kv_len;   // [R], keys j < kv_len[r] are used; >= 1
  const int* anc;      // [R, ld_anc] cache row of key j of row r, or null
  const int* row_map;  // [R] cache row of every key of row r (anc null), or null = r
  long long k_sr, k_sk, v_sr, v_sk;  // cache row / key strides
  int k_sh, v_sh;                    // head strides
  int q_sr, q_sh, o_sr, o_sh, kn_sr, kn_sh, vn_sr, vn_sh;
  int ld_anc;
  int R, H, Lk;
  int n_src;  // cache rows: anc / row_map entries are clamped into [0, n_src)
  float scale;
};

// One beam-search selection step, B sentences x beam hypotheses (rows
// r = sentence * beam + slot).
struct BeamTopkArgs {
  const uint16_t* logits;  // bf16 [R, ldl], the first V columns count
  const float* score;      // [R]
  const int* fin;          // [R] 1 = hypothesis has ended
  float* score_out;        // [R] per new slot, descending
  int* parent;             // [R] global row the slot continues
  int* token;              // [R]
  int* fin_out;            // [R]
  // ancestry update (both or neither): anc_out[r][:t+1] = anc_in[parent[r]][:t+1],
  // anc_out[r][t+1] = r
  const int* anc_in;
  int* anc_out;
  int B, beam, V, ldl, end_id, pad_id, ld_anc, t;
};

// One sampling step (temperature, then top-k, then top-p, then a Gumbel-max
// draw), one row per hypothesis. Row r draws from the Philox stream of
// (seed, step, row_id[r]), wherever it sits in the batch.
struct SampleArgs {
  const uint16_t* logits;  // bf16 [R, ldl], the first V columns count
  const float* score;      // [R] running sum of model log-probabilities
  const int* fin;          // [R] 1 = row has ended
  const int* row_id;       // [R] identity in the random stream, or null = r
  float* score_out;        // [R]
  int* token;              // [R]
  int* fin_out;            // [R]
  unsigned long long seed, step;
  float temperature, top_p;  // T > 0; 0 < top_p <= 1 (1 = off)
  int top_k;                 // 0 = off
  int R, V, ldl, end_id, pad_id;
};

// The members of a mixture of distributions over the vocabulary (an ensemble's
// models, a student's teachers). They ride in the argument block by value: no
// pointer table on the device, nothing to upload before a launch.
constexpr int MEMBERS_MAX = 8;
struct MemberRows {
  const uint16_t* x[MEMBERS_MAX];  // member m: bf16 [R, ld[m]], the first V columns count
  float logw[MEMBERS_MAX];         // log of the weights (> 0, sum 1)
  int ld[MEMBERS_MAX];             // row strides, in elements
};

// The ensemble's combine step: M members' logits -> the log of the weighted
// mean of their probabilities, one row per hypothesis.
constexpr int ENSEMBLE_MAX = MEMBERS_MAX;
struct EnsembleArgs {
  MemberRows mem;
  uint16_t* out;  // bf16 [R, ldo]: columns [0, V) written, [V, No) set to -inf
  int M, R, V, ldo, No;
};

// Teacher-forced scoring: the same mixture as EnsembleArgs, of which only the
// label's column and (optionally) the row's largest value are kept.
struct ScoreArgs {
  MemberRows mem;
  const void* labels;  // [R] int32, or int64 with lab64
  float* tok_lp;       // [R] mix[r, labels[r]]; 0 on a pad_id row, -inf outside [0, V)
  float* top_lp;       // [R] max_v mix[r, v]; 0 on a pad_id row; null = not wanted
  int M, R, V, lab64, pad_id;
};

}  // namespace tdg
