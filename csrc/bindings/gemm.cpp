// bf16 GEMM bindings: plain, grouped, ragged, and the bias-gradient column sums.
#include "common.h"

namespace {

// A(m,k) / B(n,k): bf16, 16-byte aligned, K-contiguous [mn][ld] or
// MN-contiguous [K][ld]. The kernels read whole 16-byte chunks, so the
// contiguous dimension must be readable up to a multiple of 8.
void check_operand(const Tensor& t, bool kc, int64_t mn, int64_t K, int64_t ld, const char* n) {
  check_bf16(t, n);
  check_aligned(t, 16, n);
  if (kc) check_extent(t, mn, ld, round8(K), n);
  else check_extent(t, K, ld, round8(mn), n);
}
// C of a grouped launch: every problem's output has the first one's dtype.
void check_group_c(const Tensor& C, bool f32, int64_t M, int64_t N, int64_t ldc) {
  TORCH_CHECK(C.is_cuda() && (C.scalar_type() == at::kFloat) == f32 &&
                  (f32 || C.scalar_type() == at::kBFloat16),
              "grouped gemm: C dtypes must match (f32 or bf16)");
  check_extent(C, M, ldc, N, "C");
}

void gemm(const Tensor& A, const Tensor& B, const Tensor& C, const optional<Tensor>& bias,
          const optional<Tensor>& aux, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
          int64_t ldc, int64_t ldaux, bool a_kc, bool b_kc, int64_t epi, double alpha,
          double beta, int64_t tile_cfg, int64_t splits, const optional<Tensor>& ws,
          const optional<Tensor>& relu_bits, int64_t ldbits) {
  TORCH_CHECK(C.is_cuda(), "C must be a GPU tensor");
  const bool f32 = C.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || C.scalar_type() == at::kBFloat16, "C must be f32 or bf16");
  TORCH_CHECK(M > 0 && N > 0 && K > 0, "gemm: empty problem");
  TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0, "gemm: lda/ldb must be multiples of 8");
  TORCH_CHECK(lda >= round8(a_kc ? K : M), "gemm: lda < round8(", a_kc ? "K)" : "M)");
  TORCH_CHECK(ldb >= round8(b_kc ? K : N), "gemm: ldb < round8(", b_kc ? "K)" : "N)");
  check_operand(A, a_kc, M, K, lda, "A");
  check_operand(B, b_kc, N, K, ldb, "B");
  TORCH_CHECK(ldc >= N, "gemm: ldc < N");
  check_extent(C, M, ldc, N, "C");
  const float* bptr = nullptr;
  if (epi == 1 || epi == 2) {
    TORCH_CHECK(bias.has_value(), "gemm: bias epilogue needs bias");
    check_f32(*bias, "bias");
    TORCH_CHECK(bias->numel() >= N, "gemm: bias too short");
    bptr = bias->data_ptr<float>();
  }
  const void* xptr = nullptr;
  // ReLU mask as a bitmap [M][ldbits] (uint8, bit e of byte c = column 8c + e):
  // written by the bias+ReLU epilogue, read by the ReLU-backward one instead of aux
  void* bits = nullptr;
  if (relu_bits.has_value()) {
    TORCH_CHECK(epi == 2 || epi == 3, "gemm: relu_bits needs the bias+ReLU or ReLU-backward epilogue");
    TORCH_CHECK(relu_bits->is_cuda() && relu_bits->scalar_type() == at::kByte,
                "relu_bits must be a uint8 GPU tensor");
    TORCH_CHECK(N % 8 == 0, "gemm: relu_bits needs N % 8 == 0");
    TORCH_CHECK(ldbits >= N / 8, "gemm: ldbits < N / 8");
    check_extent(*relu_bits, M, ldbits, N / 8, "relu_bits");
    bits = relu_bits->data_ptr();
  }
  if (epi == 3 && bits == nullptr) {
    TORCH_CHECK(aux.has_value(), "gemm: DRELU epilogue needs aux");
    check_bf16(*aux, "aux");
    check_extent(*aux, M, ldaux, N, "aux");
    xptr = aux->data_ptr();
  }
  float* wptr = nullptr;
  if (splits > 1) {
    TORCH_CHECK(ws.has_value(), "gemm: split-K needs a workspace");
    check_f32(*ws, "ws");
    TORCH_CHECK(ws->numel() >= splits * M * ldc, "gemm: workspace too small");
    wptr = ws->data_ptr<float>();
  }
  c10::DeviceGuard g(A.device());
  const int rc = tdg_gemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), bptr, xptr, (int)M, (int)N,
                          (int)K, (int)lda, (int)ldb, (int)ldc, (int)ldaux, a_kc, b_kc, (int)epi,
                          f32, (float)alpha, (float)beta, (int)tile_cfg, (int)splits, wptr,
                          stream_of(A), bits, (int)ldbits);
  check_err(rc, "tdg gemm");
}

void gemm_grouped(const std::vector<Tensor>& As, const std::vector<Tensor>& Bs,
                  const std::vector<Tensor>& Cs, int64_t M, int64_t N, int64_t K, int64_t lda,
                  int64_t ldb, int64_t ldc, bool a_kc, bool b_kc, double alpha, double beta,
                  int64_t tile_cfg) {
  const size_t G = As.size();
  TORCH_CHECK(G >= 1 && G <= 32 && Bs.size() == G && Cs.size() == G, "gemm_grouped: 1..32 problems");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc >= N, "gemm_grouped: shape");
  const bool f32 = Cs[0].scalar_type() == at::kFloat;
  std::vector<const void*> a(G), b(G);
  std::vector<void*> c(G);
  for (size_t i = 0; i < G; ++i) {
    check_operand(As[i], a_kc, M, K, lda, "A");
    check_operand(Bs[i], b_kc, N, K, ldb, "B");
    check_group_c(Cs[i], f32, M, N, ldc);
    a[i] = As[i].data_ptr();
    b[i] = Bs[i].data_ptr();
    c[i] = Cs[i].data_ptr();
  }
  c10::DeviceGuard g(As[0].device());
  const int rc = tdg_gemm_grouped(a.data(), b.data(), c.data(), (int)G, (int)M, (int)N, (int)K,
                                  (int)lda, (int)ldb, (int)ldc, a_kc, b_kc, f32, (float)alpha,
                                  (float)beta, (int)tile_cfg, stream_of(As[0]));
  check_err(rc, "tdg gemm_grouped");
}

// Ragged grouped GEMM (256x256 tiles): problems i = (As[i], Bs[i], Cs[i]) with
// shapes[i] = (M, N, lda, ldb, ldc, t_first, t_count), sharing K and the
// operand layouts.
void gemm_ragged(const std::vector<Tensor>& As, const std::vector<Tensor>& Bs,
                 const std::vector<Tensor>& Cs, const std::vector<int64_t>& shapes, int64_t K,
                 bool a_kc, bool b_kc, double alpha, double beta,
                 const std::vector<c10::optional<Tensor>>& bias_out) {
  const size_t P = As.size();
  TORCH_CHECK(P >= 1 && P <= 64 && Bs.size() == P && Cs.size() == P && shapes.size() == 7 * P,
              "gemm_ragged: 1..64 problems, 7 shape values each (M, N, lda, ldb, ldc, t_first, "
              "t_count)");
  TORCH_CHECK(K > 0 && K % 64 == 0, "gemm_ragged: K must be a multiple of 64");
  const bool f32 = Cs[0].scalar_type() == at::kFloat;
  std::vector<const void*> a(P), b(P);
  std::vector<void*> c(P);
  std::vector<int> sh(7 * P);
  for (size_t i = 0; i < P; ++i) {
    const int64_t M = shapes[7 * i], N = shapes[7 * i + 1], lda = shapes[7 * i + 2],
                  ldb = shapes[7 * i + 3], ldc = shapes[7 * i + 4];
    TORCH_CHECK(M > 0 && N > 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc >= N, "gemm_ragged: shape");
    check_operand(As[i], a_kc, M, K, lda, "A");
    check_operand(Bs[i], b_kc, N, K, ldb, "B");
    check_group_c(Cs[i], f32, M, N, ldc);
    a[i] = As[i].data_ptr();
    b[i] = Bs[i].data_ptr();
    c[i] = Cs[i].data_ptr();
    for (int j = 0; j < 7; ++j) sh[7 * i + j] = (int)shapes[7 * i + j];
  }
  // optional fused bias gradients: bias_out[i][M_i] = alpha * row sums of A_i (+ beta * old)
  TORCH_CHECK(bias_out.empty() || bias_out.size() == P, "gemm_ragged: bias_out must be empty or P long");
  std::vector<float*> bo(P, nullptr);
  bool any_bias = false;
  for (size_t i = 0; i < bias_out.size(); ++i) {
    if (!bias_out[i].has_value()) continue;
    const Tensor& t = *bias_out[i];
    TORCH_CHECK(!a_kc, "gemm_ragged: fused bias sums need an MN-contiguous A");
    check_f32(t, "bias_out");
    TORCH_CHECK(t.is_contiguous() && t.numel() == shapes[7 * i], "gemm_ragged: bias_out[", i,
                "] must hold M floats");
    bo[i] = t.data_ptr<float>();
    any_bias = true;
  }
  c10::DeviceGuard g(As[0].device());
  const int rc = tdg_gemm_ragged(a.data(), b.data(), c.data(), (int)P, sh.data(), (int)K, a_kc,
                                 b_kc, f32, (float)alpha, (float)beta,
                                 any_bias ? bo.data() : nullptr, stream_of(As[0]));
  check_err(rc, "tdg gemm_ragged");
}

void colsum(const Tensor& X, const Tensor& out, const Tensor& part, int64_t M, int64_t N,
            int64_t ld, int64_t rows_per_block, double beta) {
  check_bf16(X, "X");
  check_f32(out, "out");
  check_f32(part, "part");
  check_extent(X, M, ld, N, "X");
  TORCH_CHECK(out.numel() >= N, "colsum: out too short");
  TORCH_CHECK(part.numel() >= ((M + rows_per_block - 1) / rows_per_block) * N,
              "colsum: partial buffer too small");
  c10::DeviceGuard g(X.device());
  tdg_colsum(X.data_ptr(), out.data_ptr<float>(), part.data_ptr<float>(), (int)M, (int)N, (int)ld,
             (int)rows_per_block, (float)beta, stream_of(X));
  check_err(0, "tdg colsum");
}

void colsum_grouped(const std::vector<Tensor>& Xs, const std::vector<Tensor>& outs,
                    const Tensor& part, int64_t M, int64_t N, int64_t ld, int64_t rows_per_block,
                    double beta) {
  const size_t G = Xs.size();
  TORCH_CHECK(G >= 1 && G <= 32 && outs.size() == G, "colsum_grouped: 1..32 problems");
  check_f32(part, "part");
  const int64_t nparts = (M + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK(part.numel() >= (int64_t)G * nparts * N, "colsum_grouped: partials too small");
  std::vector<const void*> x(G);
  std::vector<float*> o(G);
  for (size_t i = 0; i < G; ++i) {
    check_bf16(Xs[i], "X");
    check_extent(Xs[i], M, ld, N, "X");
    check_f32(outs[i], "out");
    TORCH_CHECK(outs[i].numel() >= N, "colsum_grouped: out too short");
    x[i] = Xs[i].data_ptr();
    o[i] = outs[i].data_ptr<float>();
  }
  c10::DeviceGuard g(Xs[0].device());
  check_err(tdg_colsum_grouped(x.data(), o.data(), (int)G, part.data_ptr<float>(), (int)M, (int)N,
                               (int)ld, (int)rows_per_block, (float)beta, stream_of(Xs[0])),
            "tdg colsum_grouped");
}

// (family, BM, BN, depth, splits) of this thread's last GEMM launch
std::vector<int64_t> gemm_last_plan() {
  int p[5];
  tdg_gemm_last_plan(p);
  return {p[0], p[1], p[2], p[3], p[4]};
}

}  // namespace

void def_gemm(py::module_& m) {
  m.def("gemm", &gemm, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"), py::arg("aux"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"),
        py::arg("ldaux"), py::arg("a_kc"), py::arg("b_kc"), py::arg("epi"), py::arg("alpha"),
        py::arg("beta"), py::arg("tile_cfg"), py::arg("splits"), py::arg("ws"),
        py::arg("relu_bits") = optional<Tensor>(), py::arg("ldbits") = 0);
  m.def("gemm_grouped", &gemm_grouped);
  m.def("gemm_ragged", &gemm_ragged, py::arg("As"), py::arg("Bs"), py::arg("Cs"), py::arg("shapes"),
        py::arg("K"), py::arg("a_kc"), py::arg("b_kc"), py::arg("alpha"), py::arg("beta"),
        py::arg("bias_out") = std::vector<c10::optional<Tensor>>{});
  m.def("gemm_last_plan", &gemm_last_plan);
  m.def("colsum", &colsum);
  m.def("colsum_grouped", &colsum_grouped);
}
