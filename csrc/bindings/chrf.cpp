// Character n-gram binding: clipped match counts between pairs of rows of code
// points (chrf.hip).
#include <cstdint>

#include "common.h"

namespace {

// int32 [R], contiguous, on dev
const int* i32_vec(const Tensor& t, int64_t R, const c10::Device& dev, const char* n) {
  TORCH_CHECK(t.scalar_type() == at::kInt, n, " must be int32");
  TORCH_CHECK(t.is_cuda() && t.device() == dev, n, " must be a GPU tensor on chr's device");
  TORCH_CHECK(t.dim() == 1 && t.numel() == R && t.is_contiguous(), n, " must be int32 [", R,
              "], contiguous");
  return t.data_ptr<int>();
}

// scratch of `dtype` [N, L, last], contiguous, 16-byte aligned, on dev
void* scratch(const Tensor& t, at::ScalarType dtype, int64_t N, int64_t L, int64_t last,
              const c10::Device& dev, const char* n) {
  TORCH_CHECK(t.scalar_type() == dtype && t.is_cuda() && t.device() == dev, n, " must be a ", dtype,
              " GPU tensor on chr's device");
  TORCH_CHECK(t.dim() == 3 && t.size(0) == N && t.size(1) == L && t.size(2) == last &&
                  t.is_contiguous(),
              n, " must be [N, L, ", last, "], contiguous");
  check_aligned(t, 16, n);
  return t.data_ptr();
}

// chr int32 [N, L] (rows contiguous, any row stride >= L), length int32 [N],
// pair_a / pair_b int32 [P], out int32 [P, 6] contiguous; scratch the row
// pre-pass fills: keys int64 [N, L, 2], ranks int16 [N, L, 8]
void char_ngram_matches(const Tensor& chr, const Tensor& length, const Tensor& pair_a,
                        const Tensor& pair_b, const Tensor& out, const Tensor& keys,
                        const Tensor& ranks) {
  TORCH_CHECK(chr.scalar_type() == at::kInt, "chr must be int32");
  TORCH_CHECK(chr.is_cuda(), "chr must be a GPU tensor");
  TORCH_CHECK(chr.dim() == 2, "chr must be [N, L]");
  const int64_t N = chr.size(0), L = chr.size(1);
  TORCH_CHECK(L >= 1 && L <= tdg::CHRF_MAX_L, "char_ngram_matches: L must be in [1, ",
              tdg::CHRF_MAX_L, "], got ", L);
  TORCH_CHECK(N < (1LL << 31), "char_ngram_matches: too many rows");
  TORCH_CHECK(chr.stride(1) == 1 && (chr.stride(0) >= L || N <= 1),
              "chr: rows must be contiguous, with a row stride >= L");
  check_extent(chr, N, chr.stride(0), L, "chr");
  const c10::Device dev = chr.device();
  TORCH_CHECK(pair_a.dim() == 1, "pair_a must be int32 [P]");
  const int64_t P = pair_a.numel();
  TORCH_CHECK(P < (1LL << 31) / tdg::CHRF_ORDERS, "char_ngram_matches: too many pairs");
  tdg::ChrfArgs a{};
  a.chr = chr.data_ptr<int>();
  a.length = i32_vec(length, N, dev, "length");
  a.pair_a = i32_vec(pair_a, P, dev, "pair_a");
  a.pair_b = i32_vec(pair_b, P, dev, "pair_b");
  TORCH_CHECK(out.scalar_type() == at::kInt, "out must be int32");
  TORCH_CHECK(out.is_cuda() && out.device() == dev, "out must be a GPU tensor on chr's device");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == P && out.size(1) == tdg::CHRF_ORDERS &&
                  out.is_contiguous(),
              "out must be int32 [", P, ", 6], contiguous");
  a.out = out.data_ptr<int>();
  a.keys = static_cast<unsigned long long*>(scratch(keys, at::kLong, N, L, 2, dev, "keys"));
  a.ranks = static_cast<int16_t*>(scratch(ranks, at::kShort, N, L, 8, dev, "ranks"));
  a.ld = N > 1 ? chr.stride(0) : L;
  a.N = (int)N;
  a.L = (int)L;
  a.P = (int)P;
  c10::DeviceGuard g(dev);
  check_err(tdg_char_ngram_matches(&a, stream_of(chr)), "tdg char_ngram_matches");
}

}  // namespace

void def_chrf(py::module_& m) {
  namespace py = pybind11;
  m.def("char_ngram_matches", &char_ngram_matches, py::arg("chr"), py::arg("length"),
        py::arg("pair_a"), py::arg("pair_b"), py::arg("out"), py::arg("keys"), py::arg("ranks"));
}
