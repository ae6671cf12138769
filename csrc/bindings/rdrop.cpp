// R-Drop loss binding: label cross entropy plus the symmetric KL between the
// two copies of every row (loss + in-place gradient of both), one launch.
#include "common.h"

namespace {

// logits2: bf16 [2 M, ldl] (row stride ldl, any element offset), copy 2 after
// copy 1; labels and the row outputs have 2 M entries. V, ldl and alpha are
// passed on as given: the launcher refuses what it does not cover (rc -1 / -2).
void xent_rdrop(const Tensor& logits2, int64_t V, const Tensor& labels, const Tensor& ntok,
                double workers, double smoothing, double alpha, const Tensor& row_loss,
                const Tensor& row_correct, const optional<Tensor>& row_label, bool write_grad) {
  check_bf16(logits2, "logits2");
  TORCH_CHECK(logits2.dim() == 2 && logits2.is_contiguous() && logits2.size(0) % 2 == 0,
              "xent_rdrop: logits2 must be contiguous [2 M, ldl] (the row padding is written)");
  const int64_t R = logits2.size(0), ldl = logits2.size(1);
  TORCH_CHECK(R < (1LL << 31) && ldl < (1LL << 31) && V < (1LL << 31), "xent_rdrop: logits too large");
  TORCH_CHECK(labels.numel() == R && labels.is_contiguous() && labels.is_cuda(), "xent_rdrop: labels");
  const bool l64 = labels.scalar_type() == at::kLong;
  TORCH_CHECK(l64 || labels.scalar_type() == at::kInt, "labels int32/int64");
  check_f32(ntok, "ntok");
  check_f32(row_loss, "row_loss");
  check_f32(row_correct, "row_correct");
  TORCH_CHECK(ntok.numel() >= 1 && row_loss.numel() == R && row_correct.numel() == R &&
                  row_loss.is_contiguous() && row_correct.is_contiguous(), "xent_rdrop: row outputs");
  if (row_label.has_value()) {
    check_f32(*row_label, "row_label");
    TORCH_CHECK(row_label->numel() == R && row_label->is_contiguous(), "xent_rdrop: row_label");
  }
  tdg::RdropArgs a{};
  a.x = static_cast<uint16_t*>(logits2.data_ptr());
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
  a.M = (int)(R / 2);
  a.V = (int)V;
  a.ldl = (int)ldl;
  c10::DeviceGuard g(logits2.device());
  check_err(tdg_xent_rdrop(&a, stream_of(logits2)), "tdg xent_rdrop");
}

}  // namespace

void def_rdrop(py::module_& m) {
  m.def("xent_rdrop", &xent_rdrop, py::arg("logits2"), py::arg("V"), py::arg("labels"), py::arg("ntok"),
        py::arg("workers"), py::arg("smoothing"), py::arg("alpha"), py::arg("row_loss"),
        py::arg("row_correct"), py::arg("row_label") = py::none(), py::arg("write_grad") = true);
}
