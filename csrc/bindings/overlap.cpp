// N-gram overlap binding: clipped match counts between pairs of token rows
// (overlap.hip).
#include <cstdint>

#include "common.h"

namespace {

// int32 [R], contiguous, on dev
const int* i32_vec(const Tensor& t, int64_t R, const c10::Device& dev, const char* n) {
  TORCH_CHECK(t.scalar_type() == at::kInt, n, " must be int32");
  TORCH_CHECK(t.is_cuda() && t.device() == dev, n, " must be a GPU tensor on tok's device");
  TORCH_CHECK(t.dim() == 1 && t.numel() == R && t.is_contiguous(), n, " must be int32 [", R,
              "], contiguous");
  return t.data_ptr<int>();
}

// tok int32 [N, L] (rows contiguous, any row stride >= L), length int32 [N],
// pair_a / pair_b int32 [P], out int32 [P, 4] contiguous; ranks: optional
// int16 [N, L, 4] scratch (given: the ranks come from a per-row pre-pass)
void ngram_matches(const Tensor& tok, const Tensor& length, const Tensor& pair_a,
                   const Tensor& pair_b, const Tensor& out, const optional<Tensor>& ranks) {
  TORCH_CHECK(tok.scalar_type() == at::kInt, "tok must be int32");
  TORCH_CHECK(tok.is_cuda(), "tok must be a GPU tensor");
  TORCH_CHECK(tok.dim() == 2, "tok must be [N, L]");
  const int64_t N = tok.size(0), L = tok.size(1);
  TORCH_CHECK(L >= 1 && L <= tdg::NGRAM_MAX_L, "ngram_matches: L must be in [1, ",
              tdg::NGRAM_MAX_L, "], got ", L);
  TORCH_CHECK(N < (1LL << 31), "ngram_matches: too many rows");
  TORCH_CHECK(tok.stride(1) == 1 && (tok.stride(0) >= L || N <= 1),
              "tok: rows must be contiguous, with a row stride >= L");
  check_extent(tok, N, tok.stride(0), L, "tok");
  const c10::Device dev = tok.device();
  TORCH_CHECK(pair_a.dim() == 1, "pair_a must be int32 [P]");
  const int64_t P = pair_a.numel();
  TORCH_CHECK(P < (1LL << 31), "ngram_matches: too many pairs");
  tdg::NgramArgs a{};
  a.tok = tok.data_ptr<int>();
  a.length = i32_vec(length, N, dev, "length");
  a.pair_a = i32_vec(pair_a, P, dev, "pair_a");
  a.pair_b = i32_vec(pair_b, P, dev, "pair_b");
  TORCH_CHECK(out.scalar_type() == at::kInt, "out must be int32");
  TORCH_CHECK(out.is_cuda() && out.device() == dev, "out must be a GPU tensor on tok's device");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == P && out.size(1) == tdg::NGRAM_ORDERS &&
                  out.is_contiguous(),
              "out must be int32 [", P, ", 4], contiguous");
  a.out = out.data_ptr<int>();
  if (ranks.has_value()) {
    TORCH_CHECK(ranks->scalar_type() == at::kShort && ranks->is_cuda() && ranks->device() == dev,
                "ranks must be an int16 GPU tensor on tok's device");
    TORCH_CHECK(ranks->dim() == 3 && ranks->size(0) == N && ranks->size(1) == L &&
                    ranks->size(2) == tdg::NGRAM_ORDERS && ranks->is_contiguous(),
                "ranks must be int16 [N, L, 4], contiguous");
    check_aligned(*ranks, 8, "ranks");
    a.ranks = ranks->data_ptr<int16_t>();
  }
  a.ld = N > 1 ? tok.stride(0) : L;
  a.N = (int)N;
  a.L = (int)L;
  a.P = (int)P;
  c10::DeviceGuard g(dev);
  check_err(tdg_ngram_matches(&a, stream_of(tok)), "tdg ngram_matches");
}

}  // namespace

void def_overlap(py::module_& m) {
  namespace py = pybind11;
  m.def("ngram_matches", &ngram_matches, py::arg("tok"), py::arg("length"), py::arg("pair_a"),
        py::arg("pair_b"), py::arg("out"), py::arg("ranks") = py::none());
}
