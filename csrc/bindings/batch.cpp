// Batch-assembly binding (batch.hip): gather rows of a device-resident token
// store into right-padded [B, L] token tensors, one or two sides per launch.
#include "common.h"

namespace {

// outs[i] [B, L_i] = rows idx[0, B) of side i's store (tokens[i]: flat int32;
// offsets[i]: int64 [n_rows_i + 1]), cut at L_i and right-padded with 0.
// outs share one dtype, int64 or int32. bad: int32 device counter of cut /
// out-of-range rows, or none. The side count, B and L are the launcher's to
// refuse (rc < 0, nothing launched, outputs untouched).
void gather_rows(const Tensor& idx, const std::vector<Tensor>& tokens,
                 const std::vector<Tensor>& offsets, const std::vector<Tensor>& outs,
                 const optional<Tensor>& bad) {
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kInt && idx.is_contiguous() &&
                  idx.dim() == 1,
              "gather_rows: idx must be a contiguous int32 [B] GPU tensor");
  const size_t n = outs.size();
  TORCH_CHECK(tokens.size() == n && offsets.size() == n, "gather_rows: one store per output");
  const int64_t B = idx.numel();
  TORCH_CHECK(B <= INT32_MAX, "gather_rows: B past int32");
  const int* tp[2] = {nullptr, nullptr};
  const long long* op[2] = {nullptr, nullptr};
  void* outp[2] = {nullptr, nullptr};
  int nrows[2] = {0, 0}, L[2] = {0, 0};
  long long ntok[2] = {0, 0};
  bool o64 = true;
  for (size_t i = 0; i < n && i < 2; ++i) {
    const Tensor &t = tokens[i], &o = offsets[i], &out = outs[i];
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() &&
                    t.device() == idx.device(),
                "gather_rows: tokens must be contiguous int32 on idx's GPU");
    TORCH_CHECK(o.is_cuda() && o.scalar_type() == at::kLong && o.is_contiguous() &&
                    o.numel() >= 1 && o.numel() - 1 <= INT32_MAX && o.device() == idx.device(),
                "gather_rows: offsets must be contiguous int64 [n_rows + 1] on idx's GPU");
    const bool is64 = out.scalar_type() == at::kLong;
    TORCH_CHECK(out.is_cuda() && (is64 || out.scalar_type() == at::kInt) && out.is_contiguous() &&
                    out.dim() == 2 && out.size(0) == B && out.size(1) <= INT32_MAX &&
                    out.device() == idx.device(),
                "gather_rows: out must be a contiguous int64 / int32 [B, L] on idx's GPU");
    TORCH_CHECK(i == 0 || is64 == o64, "gather_rows: outputs of one dtype");
    o64 = is64;
    tp[i] = t.data_ptr<int>();
    op[i] = reinterpret_cast<const long long*>(o.data_ptr<int64_t>());
    outp[i] = out.data_ptr();
    nrows[i] = (int)(o.numel() - 1);
    ntok[i] = t.numel();
    L[i] = (int)out.size(1);
  }
  unsigned* bp = nullptr;
  if (bad.has_value()) {
    TORCH_CHECK(bad->is_cuda() && bad->scalar_type() == at::kInt && bad->numel() >= 1 &&
                    bad->device() == idx.device(),
                "gather_rows: bad must be an int32 tensor on idx's GPU");
    bp = reinterpret_cast<unsigned*>(bad->data_ptr<int>());
  }
  c10::DeviceGuard g(idx.device());
  check_err(tdg_gather_rows((int)n, idx.data_ptr<int>(), (int)B, o64, tp[0], op[0], nrows[0],
                            ntok[0], outp[0], L[0], tp[1], op[1], nrows[1], ntok[1], outp[1], L[1],
                            bp, stream_of(idx)),
            "tdg gather_rows");
}

}  // namespace

void def_batch(py::module_& m) { m.def("gather_rows", &gather_rows); }
