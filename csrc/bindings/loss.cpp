// Loss bindings: batch preparation, token counts, the fused label-smoothed
// cross entropy (loss + in-place gradient) and its statistics.
#include "common.h"

namespace {

void count_tokens(const Tensor& labels, const Tensor& out) {
  TORCH_CHECK(labels.is_contiguous() && labels.is_cuda(), "labels");
  const bool l64 = labels.scalar_type() == at::kLong;
  check_f32(out, "out");
  c10::DeviceGuard g(labels.device());
  check_err(tdg_count_tokens(labels.data_ptr(), l64, (int)labels.numel(), out.data_ptr<float>(),
                             stream_of(labels)),
            "tdg count_tokens");
}

// tgts: the target batches [B, T1] of one optimizer update; total f32 [1];
// counts (optional) int32 [>= len(tgts)]
void count_labels_multi(const std::vector<Tensor>& tgts, const Tensor& total,
                        const optional<Tensor>& counts) {
  const int n = (int)tgts.size();
  TORCH_CHECK(n >= 1, "count_labels_multi: no entries");
  check_f32(total, "total");
  TORCH_CHECK(total.numel() >= 1, "count_labels_multi: total");
  if (counts.has_value())
    TORCH_CHECK(counts->is_cuda() && counts->scalar_type() == at::kInt && counts->is_contiguous() &&
                    counts->numel() >= n, "count_labels_multi: counts must be int32 [n]");
  std::vector<const void*> p(n);
  std::vector<int> B(n), T1(n), t64(n);
  for (int i = 0; i < n; ++i) {
    const Tensor& t = tgts[i];
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.is_contiguous() && t.device() == total.device(),
                "count_labels_multi: entries must be contiguous [B, T1] tensors on one GPU");
    const auto dt = t.scalar_type();
    TORCH_CHECK(dt == at::kLong || dt == at::kInt, "count_labels_multi: tokens must be int64 or int32");
    TORCH_CHECK(t.numel() <= 0x7fffffffLL, "count_labels_multi: entry too large");
    p[i] = t.data_ptr();
    B[i] = (int)t.size(0);
    T1[i] = (int)t.size(1);
    t64[i] = dt == at::kLong;
  }
  c10::DeviceGuard g(total.device());
  check_err(tdg_count_labels_multi(p.data(), B.data(), T1.data(), t64.data(), n,
                                   total.data_ptr<float>(),
                                   counts.has_value() ? counts->data_ptr<int>() : nullptr,
                                   stream_of(total)),
            "tdg count_labels_multi");
}

// tgt_in, labels [B, T] (token dtype), src_len, tgt_len [B] int32, ntok [1] f32,
// ctr (optional int64 [1], += 1)
void prep_batch(const Tensor& src, const Tensor& tgt, const Tensor& tgt_in, const Tensor& labels,
                const Tensor& src_len, const Tensor& tgt_len, const Tensor& ntok,
                const c10::optional<Tensor>& ctr, const Tensor& scratch) {
  TORCH_CHECK(src.is_cuda() && src.dim() == 2 && src.is_contiguous(), "prep_batch: src");
  TORCH_CHECK(tgt.is_cuda() && tgt.dim() == 2 && tgt.is_contiguous() && tgt.size(0) == src.size(0),
              "prep_batch: tgt");
  const auto dt = src.scalar_type();
  TORCH_CHECK((dt == at::kLong || dt == at::kInt) && tgt.scalar_type() == dt,
              "prep_batch: tokens must be int64 or int32 (both)");
  const int64_t B = src.size(0), S = src.size(1), T1 = tgt.size(1);
  TORCH_CHECK(T1 >= 2, "prep_batch: target needs >= 2 tokens");
  for (const Tensor* t : {&tgt_in, &labels})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == dt &&
                    t->numel() == B * (T1 - 1), "prep_batch: tgt_in / labels");
  for (const Tensor* t : {&src_len, &tgt_len})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->numel() == B, "prep_batch: lengths");
  check_f32(ntok, "ntok");
  // scratch: int32 [B + 2] -- per-row label counts, a zero-initialised
  // ticket, and a sticky count of rows with a PAD before a non-PAD token
  TORCH_CHECK(scratch.is_cuda() && scratch.scalar_type() == at::kInt && scratch.numel() >= B + 2,
              "prep_batch: scratch must be int32 [B + 2], ticket word zero");
  long long* c = nullptr;
  if (ctr.has_value()) {
    TORCH_CHECK(ctr->is_cuda() && ctr->scalar_type() == at::kLong, "prep_batch: ctr");
    c = reinterpret_cast<long long*>(ctr->data_ptr<int64_t>());
  }
  c10::DeviceGuard g(src.device());
  check_err(tdg_prep_batch(src.data_ptr(), (int)S, tgt.data_ptr(), (int)T1, (int)B, dt == at::kLong,
                           tgt_in.data_ptr(), labels.data_ptr(), src_len.data_ptr<int>(),
                           tgt_len.data_ptr<int>(), ntok.data_ptr<float>(), c,
                           scratch.data_ptr<int>(),
                           reinterpret_cast<unsigned*>(scratch.data_ptr<int>() + B),
                           scratch.data_ptr<int>() + B + 1, stream_of(src)),
            "tdg prep_batch");
}

void xent(const Tensor& logits, int64_t V, const Tensor& labels, const Tensor& ntok,
          double workers, double smoothing, const Tensor& row_loss, const Tensor& row_correct,
          bool write_grad) {
  check_bf16(logits, "logits");
  check_contig(logits, "logits");
  const int64_t ldl = logits.size(-1), M = logits.numel() / ldl;
  TORCH_CHECK(ldl % 2 == 0 && V <= ldl && V > 0, "xent: logits row must be even-padded >= V");
  TORCH_CHECK(labels.numel() == M && labels.is_contiguous(), "xent: labels");
  const bool l64 = labels.scalar_type() == at::kLong;
  TORCH_CHECK(l64 || labels.scalar_type() == at::kInt, "labels int32/int64");
  check_f32(ntok, "ntok");
  check_f32(row_loss, "row_loss");
  check_f32(row_correct, "row_correct");
  TORCH_CHECK(row_loss.numel() == M && row_correct.numel() == M, "xent: row outputs");
  c10::DeviceGuard g(logits.device());
  check_err(tdg_xent(logits.data_ptr(), (int)M, (int)V, (int)ldl, labels.data_ptr(), l64,
                     ntok.data_ptr<float>(), (float)workers, (float)smoothing,
                     row_loss.data_ptr<float>(), row_correct.data_ptr<float>(), write_grad,
                     stream_of(logits)),
            "tdg xent");
}

void xent_stats(const Tensor& row_loss, const Tensor& row_correct, const Tensor& ntok,
                double workers, const optional<Tensor>& step_out,
                const optional<Tensor>& accum) {
  check_f32(row_loss, "row_loss");
  check_f32(row_correct, "row_correct");
  if (step_out.has_value()) check_f32(*step_out, "step_out");
  if (accum.has_value()) {
    check_f32(*accum, "accum");
    TORCH_CHECK(accum->numel() >= 4, "accum needs 4 slots");
  }
  c10::DeviceGuard g(row_loss.device());
  check_err(tdg_xent_stats(row_loss.data_ptr<float>(), row_correct.data_ptr<float>(),
                           (int)row_loss.numel(), ntok.data_ptr<float>(), (float)workers,
                           opt_f32(step_out), opt_f32(accum), stream_of(row_loss)),
            "tdg xent_stats");
}

}  // namespace

void def_loss(py::module_& m) {
  m.def("count_tokens", &count_tokens);
  m.def("count_labels_multi", &count_labels_multi);
  m.def("prep_batch", &prep_batch);
  m.def("xent", &xent);
  m.def("xent_stats", &xent_stats);
}
