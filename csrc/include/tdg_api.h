// The C launcher ABI of the gfx950 kernels: every tdg_* entry point, declared
// once. The .hip file that defines a launcher and the bindings that call it
// both include this header, so a definition that disagrees with its
// declaration does not compile ("conflicting types" for a C-linkage
// function). What each launcher computes is documented at its definition.
// Launchers return 0 on success and a negative code for an unsupported
// configuration (nothing launched) unless noted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdg_attn.h"
#include "tdg_decode.h"
#include "tdg_distill.h"
#include "tdg_overlap.h"

extern "C" {

// ---------------------------------------------------------------- gemm.hip
// a_kc / b_kc: operand is K-contiguous; epi: tdg::Epi (0..3); ws: split-K slabs.
// relu_bits (or null): the ReLU mask as a bitmap [M][ldbits] bytes, bit e of
// byte c = column 8c + e -- written by epi 2 (bits = output > 0), read by
// epi 3 instead of aux. Needs N % 8 == 0, ldc % 8 == 0, a 16-byte aligned
// bf16 C and no split-K (-11 / -12 otherwise).
int tdg_gemm(const void* A, const void* B, void* C, const float* bias, const void* aux, int M,
             int N, int K, int lda, int ldb, int ldc, int ldaux, int a_kc, int b_kc, int epi,
             int out_f32, float alpha, float beta, int tile_cfg, int splits, float* ws,
             hipStream_t st, void* relu_bits, int ldbits);
int tdg_gemm_grouped(const void* const* A, const void* const* B, void* const* C, int G, int M,
                     int N, int K, int lda, int ldb, int ldc, int a_kc, int b_kc, int out_f32,
                     float alpha, float beta, int tile_cfg, hipStream_t st);
// shapes[7 * i ..] = (M, N, lda, ldb, ldc, t_first, t_count) of problem i
int tdg_gemm_ragged(const void* const* A, const void* const* B, void* const* C, int P,
                    const int* shapes, int K, int a_kc, int b_kc, int out_f32, float alpha,
                    float beta, float* const* bias_out, hipStream_t st);
// The GEMM launch this thread made last, as its launcher recorded it: family
// (0 lock-step tiles, 1 256x256 ragged kernel, 2 pipelined kernel), BM, BN,
// pipeline depth, effective split-K count. family -1: none yet. Host only.
void tdg_gemm_last_plan(int out[5]);
void tdg_colsum(const void* X, float* out, float* part, int M, int N, int ld, int rows_per_block,
                float beta, hipStream_t st);
int tdg_colsum_grouped(const void* const* X, float* const* out, int G, float* part, int M, int N,
                       int ld, int rows_per_block, float beta, hipStream_t st);

// ---------------------------------------------------------------- attention.hip (attn_{fwd,bwd,f8,qkv}.h)
// -1 from tdg_qkv_attn_fwd / tdg_attn_bwd_fdo: shape not covered, nothing launched
int tdg_attn_fwd(const tdg::AttnArgs* a, int hd, hipStream_t st);
int tdg_qkv_attn_fwd(const tdg::QkvAttnArgs* qa, hipStream_t st);
int tdg_attn_bwd(const tdg::AttnArgs* a, int hd, hipStream_t st);
int tdg_attn_bwd_fdo(const tdg::AttnArgs* a, hipStream_t st);
int tdg_attn_probs(const tdg::AttnArgs* a, int hd, float* probs, hipStream_t st);
int tdg_attn_fwd_fp8(const tdg::AttnArgs* a, int hd, hipStream_t st);
int tdg_attn_bwd_f8(const tdg::AttnArgs* a, int hd, hipStream_t st);
// The bf16 attention launch this thread made last, as its launcher recorded
// it: kernel family (attn_impl.h AttnPlanFamily), head dim, workgroups and
// threads per workgroup, workgroups of the backward's second (dK/dV) launch
// or 0. family -1: none yet. The fp8 launchers do not record. Host only.
void tdg_attn_last_plan(int out[5]);

// ---------------------------------------------------------------- decode.hip
// -1: hd not 16 / 64 (decode_attn), beam outside [1, 8] or V outside
// [1, 65536] (beam_topk, sample_token, ensemble_logprobs, score_tokens), M
// outside [1, 8] (ensemble_logprobs, score_tokens); nothing launched
int tdg_decode_attn(const tdg::DecodeAttnArgs* a, int hd, hipStream_t st);
int tdg_beam_topk(const tdg::BeamTopkArgs* a, hipStream_t st);
int tdg_sample_token(const tdg::SampleArgs* a, hipStream_t st);
int tdg_ensemble_logprobs(const tdg::EnsembleArgs* a, hipStream_t st);
int tdg_score_tokens(const tdg::ScoreArgs* a, hipStream_t st);

// --------------------------------------------------------------- overlap.hip
// -1: L outside [1, 512], N or P negative, ld < L; -2: a null operand; nothing
// launched
int tdg_ngram_matches(const tdg::NgramArgs* a, hipStream_t st);

// ---------------------------------------------------------------- norm.hip
// ctr: device RNG step counter (or null); site: dropout site id; y8 / s8 /
// amax8: optional e4m3 copy of y, its scale and amax slot; kbits: keep bitmap
int tdg_ln_fwd(const void* x, const void* s, const float* gamma, const float* beta, void* y,
               void* hsave, float* mean, float* rstd, int M, int D, float p, uint64_t seed,
               const long long* ctr, uint64_t site, float eps, void* y8, const float* s8,
               unsigned* amax8, void* kbits, hipStream_t st);
// rpb: rows per block of the dgamma / dbeta partials in ws; ds8: e5m2 copy of ds
int tdg_ln_bwd(const void* dy, const void* hsave, const float* mean, const float* rstd,
               const float* gamma, void* dh, void* ds, const void* dres, float* dgamma,
               float* dbeta, float* dbias, float* ws, int M, int D, float p, uint64_t seed,
               const long long* ctr, uint64_t site, int accumulate, int skip_reduce, int rpb,
               void* ds8, const float* s8, unsigned* amax8, const void* kbits, hipStream_t st);
int tdg_reduce_partials_multi(const float* const* parts, float* const* outs, const int* nparts,
                              int G, int N, float beta, hipStream_t st);

// ---------------------------------------------------------------- embed.hip
int tdg_embed_fwd(const void* tok, int tok64, const void* table, const float* pe, void* out, int M,
                  int L, int D, float scale, float p, uint64_t seed, const long long* ctr,
                  uint64_t site, void* kbits, hipStream_t st);
int tdg_embed_bwd(const void* tok, int tok64, const void* dout, float* dtable, int M, int D,
                  float scale, float p, uint64_t seed, const long long* ctr, uint64_t site,
                  hipStream_t st);
// acc: all-zero int64 [V, D] scratch, left all-zero
int tdg_embed_bwd_det(const void* tok, int tok64, const void* dout, float* dtable, long long* acc,
                      int M, int D, long long V, float scale, float p, uint64_t seed,
                      const long long* ctr, uint64_t site, float beta, hipStream_t st);
// workspace words (int32, int64) of the CSR backward
void tdg_embed_csr_ws(int M, int V, int D, long long* n32, long long* n64);
int tdg_embed_csr_ok(int M, int V);  // 1 when the sort covers the shape
int tdg_embed_csr_sort(int ntab, const void* const* tok, const int* tok64, const int* M,
                       const int* V, int* const* ws32, long long* stamps, hipStream_t st);
int tdg_embed_csr_apply(const void* dout, const void* kbits, float* dtable, int* ws32,
                        long long* ws64, int M, int D, int V, float scale, float p, uint64_t seed,
                        const long long* ctr, uint64_t site, float beta, hipStream_t st);

// ---------------------------------------------------------------- xent.hip
int tdg_count_tokens(const void* labels, int lab64, int M, float* out, hipStream_t st);
// row_lab [B], ticket (zero on entry), bad_rows: int32 scratch words
int tdg_prep_batch(const void* src, int S, const void* tgt, int T1, int B, int lab64, void* tgt_in,
                   void* labels, int* src_len, int* tgt_len, float* ntok, long long* ctr,
                   int* row_lab, unsigned* ticket, int* bad_rows, hipStream_t st);
// up to 32 target batches [B[i], T1[i]] (host arrays of device pointers and
// sizes): total[0] = labels (tgt[b, t] != 0, t >= 1) of all of them, as f32;
// counts (or null): int32 per entry. -1: n outside [1, 32]; -2: a bad entry
int tdg_count_labels_multi(const void* const* tgt, const int* B, const int* T1, const int* tok64,
                           int n, float* total, int* counts, hipStream_t st);
int tdg_xent(void* logits, int M, int V, int ldl, const void* labels, int lab64, const float* ntok,
             float workers, float smoothing, float* row_loss, float* row_correct, int write_grad,
             hipStream_t st);
int tdg_xent_stats(const float* row_loss, const float* row_correct, int M, const float* ntok,
                   float workers, float* step_out, float* accum, hipStream_t st);

// ---------------------------------------------------------------- distill.hip
// -1: T outside [1, 8], V outside [1, 65536] or alpha outside [0, 1]; -2: a
// student or teacher row shorter than V, a null teacher; nothing launched
int tdg_xent_distill(const tdg::DistillArgs* a, hipStream_t st);

// ---------------------------------------------------------------- adam.hip
// gstate: device state of the gradient-norm pass (clip factor, skip flag) or null
int tdg_adam(float* p, float* g, float* m, float* v, void* shadow, long long n, long long* step,
             float beta1, float beta2, float eps, float lr_const, float d_model, float warmup,
             float grad_scale, float weight_decay, int sched, int zero_grad, int inc_step,
             const float* gstate, hipStream_t st);
// chunks: [nchunks, 4] int64 (start, n, fp8 slot or -1, e4m3 address or 0)
int tdg_adam_chunks(float* p, float* g, float* m, float* v, void* shadow, long long n,
                    const void* chunks, int nchunks, long long* step, float beta1, float beta2,
                    float eps, float lr_const, float d_model, float warmup, float grad_scale,
                    float weight_decay, int sched, int zero_grad, int inc_step,
                    const float* scale8, unsigned* amax8, const float* gstate, hipStream_t st);
int tdg_adam_step_inc(long long* step, const float* gstate, hipStream_t st);
// returns the number of partials written
long long tdg_grad_sumsq(const float* g, const void* chunks, long long nchunks, long long n,
                         float* partials, hipStream_t st);
int tdg_grad_norm_finalize(const float* partials, long long nparts, float* state,
                           unsigned* counters, float clip, int skip_on, float grad_scale,
                           hipStream_t st);
int tdg_to_bf16(const float* p, void* o, long long n, hipStream_t st);
int tdg_transpose_grouped(const void* const* src, void* const* dst, int G, int R, int C,
                          hipStream_t st);

// ----------------------------------------------------------------- ema.hip
// e[0, n) += (p - e) * (1 - d_eff), d_eff from decay, warmup and the device
// update count (count == 0: e = p); gstate as in tdg_adam (skipped step: no
// write, no advance); inc_count: the last range of a step advances the count
int tdg_ema(const float* p, float* e, long long n, long long* count, float decay, int warmup,
            int inc_count, const float* gstate, hipStream_t st);

// --------------------------------------------------------------- batch.hip
// out0 [B, L0] (nsides == 2: and out1 [B, L1]) = store rows idx[0, B), cut at
// L and right-padded with 0; a side's store: int32 tokens (ntok words) and
// int64 offsets [nrows + 1]; out64: int64 outputs, else int32; bad (or null):
// counter of cut / out-of-range rows. -1: nsides outside [1, 2]; -2: B < 1;
// -3: an L < 1; -4: an nrows < 0
int tdg_gather_rows(int nsides, const int* idx, int B, int out64, const int* tok0,
                    const long long* off0, int nrows0, long long ntok0, void* out0, int L0,
                    const int* tok1, const long long* off1, int nrows1, long long ntok1,
                    void* out1, int L1, unsigned* bad, hipStream_t st);

// ------------------------------------ fp8_gemm.hip, fp8_wgrad.hip, fp8_quant.hip
// afmt / cfmt / fmt: 0 e4m3, 1 e5m2; amax: a 2048-word slot (or slot table)
int tdg_gemm_fp8(const void* A, const void* B, void* C, const float* bias, const float* sa,
                 const float* sb, void* C8, const float* sc8, unsigned* amax, int M, int N, int K,
                 int lda, int ldb, int ldc, int ldc8, int epi, int cfg, int afmt, int cfmt,
                 const void* aux, int ldaux, float beta, const void* aux8, float* colsum_out,
                 float colsum_beta, float* ws, hipStream_t st);
// shapes[5 * i ..] = (M, N, lda, ldb, ldc) of problem i; T: shared token count
int tdg_wgrad_fp8(const void* const* A, const void* const* B, float* const* C,
                  const float* const* sa, const float* const* sb, int P, const int* shapes, int T,
                  float beta, hipStream_t st);
// on: bit mask over the F8_EPI_* epilogue ids (fp8_epi.h) that take the
// persistent 128x128 kernel (0 off, 0xff all); < 0 queries. Returns the old mask.
int tdg_fp8_set_persist(int on);
int tdg_fp8_quant(const void* x, void* y8, long long n, const float* scale, unsigned* amax,
                  int fmt, hipStream_t st);
int tdg_fp8_quant_multi(const void* const* x, void* const* y, const long long* n, const int* slot,
                        int nseg, const float* scale, unsigned* amax, hipStream_t st);
int tdg_fp8_quant_colsum(const void* x, int ld, void* y8, int M, int N, const float* scale,
                         unsigned* amax, float* part, int fmt, hipStream_t st);
int tdg_fp8_quant_t(const void* const* src, void* const* dst, const int* slot, int G, int R, int C,
                    const float* scale, unsigned* amax, hipStream_t st);
int tdg_fp8_scale_update(float* scale, unsigned* amax, int n, float margin_pow2, float fmax,
                         hipStream_t st);
int tdg_fp8_dequant(const void* x8, float* y, long long n, float inv_scale, hipStream_t st);

// ---------------------------------------------------------------- signal.hip
// host: pinned word the CPU polls; dhost: its device address; cnt: device counter
int tdg_signal_create(unsigned long long** host, unsigned long long** dhost,
                      unsigned long long** cnt);
int tdg_signal_emit(unsigned long long* cnt, unsigned long long* dhost, hipStream_t st);

}  // extern "C"
