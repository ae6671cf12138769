// Distillation loss binding: the student's cross entropy against a mixture of
// label and teacher distributions (loss + in-place gradient), one launch.
#include "common.h"

namespace {

// logits: the student, bf16 [M, ldl] (row stride ldl, any element offset);
// teachers: bf16 [M, ldt] each; logw: log of the normalised weights, one per
// teacher. The teacher count and alpha are passed on as given: the launcher
// refuses what it does not cover (rc -1).
void xent_distill(const Tensor& logits, const std::vector<Tensor>& teachers, int64_t V,
                  const Tensor& labels, const Tensor& ntok, double workers, double smoothing,
                  double alpha, const std::vector<double>& logw, const Tensor& row_loss,
                  const Tensor& row_correct, const optional<Tensor>& row_label, bool write_grad) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
              "xent_distill: logits must be contiguous [M, ldl] (the row padding is written)");
  const int64_t M = logits.size(0), ldl = logits.size(1);
  TORCH_CHECK(V > 0 && V <= ldl, "xent_distill: logits row must be >= V");
  TORCH_CHECK(M < (1LL << 31) && ldl < (1LL << 31), "xent_distill: logits too large");
  TORCH_CHECK(labels.numel() == M && labels.is_contiguous() && labels.is_cuda(), "xent_distill: labels");
  const bool l64 = labels.scalar_type() == at::kLong;
  TORCH_CHECK(l64 || labels.scalar_type() == at::kInt, "labels int32/int64");
  check_f32(ntok, "ntok");
  check_f32(row_loss, "row_loss");
  check_f32(row_correct, "row_correct");
  TORCH_CHECK(row_loss.numel() == M && row_correct.numel() == M && row_loss.is_contiguous() &&
                  row_correct.is_contiguous(), "xent_distill: row outputs");
  if (row_label.has_value()) {
    check_f32(*row_label, "row_label");
    TORCH_CHECK(row_label->numel() == M && row_label->is_contiguous(), "xent_distill: row_label");
  }
  tdg::DistillArgs a{};
  a.T = (int)teachers.size();
  check_members(teachers, V, logw, true, M, logits.device(), "xent_distill", "teacher", false, &a.t);
  a.x = static_cast<uint16_t*>(logits.data_ptr());
  a.labels = labels.data_ptr();
  a.lab64 = l64;
  a.ntok = ntok.data_ptr<float>();
  a.row_loss = row_loss.data_ptr<float>();
  a.row_label = opt_f32(row_label);
  a.row_correct = row_correct.data_ptr<float>();
  a.workers = (float)workers;
  a.smoothing = (float)smoothing;
  a.alpha = (float)alpha;
  a.write_grad = write_grad;
  a.M = (int)M;
  a.V = (int)V;
  a.ldl = (int)ldl;
  c10::DeviceGuard g(logits.device());
  check_err(tdg_xent_distill(&a, stream_of(logits)), "tdg xent_distill");
}

}  // namespace

void def_distill(py::module_& m) {
  m.def("xent_distill", &xent_distill, py::arg("logits"), py::arg("teachers"), py::arg("V"),
        py::arg("labels"), py::arg("ntok"), py::arg("workers"), py::arg("smoothing"),
        py::arg("alpha"), py::arg("logw"), py::arg("row_loss"), py::arg("row_correct"),
        py::arg("row_label") = py::none(), py::arg("write_grad") = true);
}
