// fp8 bindings: the e4m3 / e5m2 GEMM and weight gradients, quantisation
// (plain, multi-tensor, transposing, with column sums), delayed-scaling
// update and dequantisation.
#include "common.h"

namespace {

void gemm_fp8(const Tensor& A, const Tensor& B, const optional<Tensor>& C, const optional<Tensor>& bias,
              const Tensor& sa, const Tensor& sb, const optional<Tensor>& C8,
              const optional<Tensor>& sc8, const optional<Tensor>& amax, int64_t M, int64_t N,
              int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldc8, int64_t epi,
              int64_t cfg, int64_t afmt, int64_t cfmt, const optional<Tensor>& aux, int64_t ldaux,
              double beta, const optional<Tensor>& aux8, const optional<Tensor>& colsum_out,
              double colsum_beta, const optional<Tensor>& ws) {
  check_f8_fmt(A, afmt, "A8");
  check_f8_fmt(B, 0, "B8");
  TORCH_CHECK(C.has_value() || C8.has_value() || colsum_out.has_value(), "gemm_fp8: no output");
  if (C.has_value()) {
    check_bf16(*C, "C");
    TORCH_CHECK(C->numel() >= (M - 1) * ldc + N && ldc % 8 == 0, "gemm_fp8: C extent / ldc");
  } else {
    TORCH_CHECK(beta == 0.0 && !(epi & 16), "gemm_fp8: beta / C = dequant(C8) need C");
  }
  check_f32(sa, "sa");
  check_f32(sb, "sb");
  TORCH_CHECK(K % 128 == 0 && lda % 16 == 0 && ldb % 16 == 0, "gemm_fp8: K % 128, ld % 16");
  // flag 32: B is N-contiguous [K][ldb] (a plain weight as its dgrad's B operand)
  const bool bt = (epi & 32) != 0;
  TORCH_CHECK(A.numel() >= (M - 1) * lda + K &&
                  (bt ? B.numel() >= (K - 1) * ldb + N && ldb >= N && N % 16 == 0
                      : B.numel() >= (N - 1) * ldb + K),
              "gemm_fp8: A/B extent");
  TORCH_CHECK(!bt || ((cfg == 0 || cfg == 10) && afmt == 1 && cfmt == 1),
              "gemm_fp8: N-contiguous B runs the e5m2 backward 128x128 configs (cfg 0, 10) only");
  if (bias.has_value()) check_f32(*bias, "bias");
  const int64_t epi_id = epi & 15;  // (flag 16: C = dequant(C8))
  // (flag 64: the column-sum partials stay in ws, folded by the caller)
  TORCH_CHECK((epi & ~int64_t(127)) == 0 && epi_id <= 3, "gemm_fp8: epilogue id");
  TORCH_CHECK(!(epi & 64) || colsum_out.has_value(), "gemm_fp8: deferred column sums need colsum_out");
  TORCH_CHECK(!(epi & 16) || C8.has_value(), "gemm_fp8: C = dequant(C8) needs C8");
  TORCH_CHECK(epi_id == 0 || epi_id == 3 || bias.has_value(), "gemm_fp8: epilogue needs bias");
  TORCH_CHECK(epi_id != 3 || aux.has_value() != aux8.has_value(),
              "gemm_fp8: the ReLU-backward epilogue needs exactly one of aux (bf16) / aux8 (e4m3)");
  if (aux.has_value()) {
    check_bf16(*aux, "aux");
    TORCH_CHECK(aux->numel() >= (M - 1) * ldaux + N, "gemm_fp8: aux extent");
  }
  if (aux8.has_value()) {
    check_f8_fmt(*aux8, 0, "aux8");
    TORCH_CHECK(aux8->numel() >= (M - 1) * ldaux + N && ldaux % 8 == 0, "gemm_fp8: aux8 extent");
  }
  TORCH_CHECK((afmt == 0 || afmt == 1) && (cfmt == 0 || cfmt == 1), "gemm_fp8: formats are 0 / 1");
  if (C8.has_value()) {
    check_f8_fmt(*C8, cfmt, "C8");
    TORCH_CHECK(sc8.has_value() && C8->numel() >= (M - 1) * ldc8 + N && ldc8 % 8 == 0, "gemm_fp8: C8");
  }
  if (colsum_out.has_value()) {
    check_f32(*colsum_out, "colsum_out");
    TORCH_CHECK(colsum_out->is_contiguous() && colsum_out->numel() == N && (cfg == 0 || cfg == 10),
                "gemm_fp8: colsum_out is [N] f32 (128x128 tile configs 0, 10)");
    TORCH_CHECK(ws.has_value() && ws->scalar_type() == at::kFloat &&
                    ws->numel() >= ((M + 127) / 128) * 2 * N,
                "gemm_fp8: colsum workspace [ceil(M/128)*2, N] f32");
  }
  c10::DeviceGuard g(A.device());
  const int rc = tdg_gemm_fp8(A.data_ptr(), B.data_ptr(), opt_ptr(C), opt_f32(bias),
                              sa.data_ptr<float>(), sb.data_ptr<float>(), opt_ptr(C8),
                              opt_f32(sc8), amax_ptr(amax), (int)M, (int)N, (int)K, (int)lda,
                              (int)ldb, (int)ldc, (int)ldc8, (int)epi, (int)cfg, (int)afmt,
                              (int)cfmt, opt_ptr(aux), (int)ldaux, (float)beta, opt_ptr(aux8),
                              opt_f32(colsum_out), (float)colsum_beta, opt_f32(ws), stream_of(A));
  check_err(rc, "tdg gemm_fp8");
}

// fp8 weight gradients: Cs[i][M,N] (f32, =|+= beta) = dequant(As[i][T,M]^T (e5m2)
// @ Bs[i][T,N] (e4m3)), token-major operands, one ragged launch.
void wgrad_fp8(const std::vector<Tensor>& As, const std::vector<Tensor>& Bs,
               const std::vector<Tensor>& Cs, const std::vector<Tensor>& sas,
               const std::vector<Tensor>& sbs, double beta) {
  const size_t P = As.size();
  TORCH_CHECK(P >= 1 && P <= 64 && Bs.size() == P && Cs.size() == P && sas.size() == P &&
                  sbs.size() == P,
              "wgrad_fp8: 1..64 problems");
  const int64_t T = As[0].size(0);
  std::vector<const void*> a(P), b(P);
  std::vector<float*> c(P);
  std::vector<const float*> sa(P), sb(P);
  std::vector<int> sh(5 * P);
  for (size_t i = 0; i < P; ++i) {
    check_f8_fmt(As[i], 1, "A8 (e5m2 gradient)");
    check_f8_fmt(Bs[i], 0, "B8 (e4m3 activation)");
    check_f32(Cs[i], "C");
    check_f32(sas[i], "sa");
    check_f32(sbs[i], "sb");
    TORCH_CHECK(As[i].dim() == 2 && Bs[i].dim() == 2 && Cs[i].dim() == 2, "wgrad_fp8: 2-D tensors");
    TORCH_CHECK(As[i].size(0) == T && Bs[i].size(0) == T, "wgrad_fp8: one token count");
    TORCH_CHECK(As[i].stride(1) == 1 && Bs[i].stride(1) == 1 && Cs[i].stride(1) == 1,
                "wgrad_fp8: unit inner stride");
    const int64_t M = Cs[i].size(0), N = Cs[i].size(1);
    TORCH_CHECK(As[i].size(1) == M && Bs[i].size(1) == N, "wgrad_fp8: shapes");
    check_aligned(As[i], 16, "wgrad_fp8: A8");
    check_aligned(Bs[i], 16, "wgrad_fp8: B8");
    a[i] = As[i].data_ptr();
    b[i] = Bs[i].data_ptr();
    c[i] = Cs[i].data_ptr<float>();
    sa[i] = sas[i].data_ptr<float>();
    sb[i] = sbs[i].data_ptr<float>();
    sh[5 * i] = (int)M;
    sh[5 * i + 1] = (int)N;
    sh[5 * i + 2] = (int)As[i].stride(0);
    sh[5 * i + 3] = (int)Bs[i].stride(0);
    sh[5 * i + 4] = (int)Cs[i].stride(0);
  }
  c10::DeviceGuard g(As[0].device());
  check_err(tdg_wgrad_fp8(a.data(), b.data(), c.data(), sa.data(), sb.data(), (int)P, sh.data(),
                          (int)T, (float)beta, stream_of(As[0])),
            "tdg wgrad_fp8");
}

void fp8_quant(const Tensor& x, const Tensor& y8, const Tensor& scale,
               const optional<Tensor>& amax, int64_t fmt) {
  check_bf16(x, "x");
  check_contig(x, "x");
  check_f8_fmt(y8, fmt, "y8");
  TORCH_CHECK(fmt == 0 || fmt == 1, "fp8_quant: format is 0 / 1");
  TORCH_CHECK(y8.numel() >= x.numel() && y8.is_contiguous(), "fp8_quant: y8");
  check_f32(scale, "scale");
  c10::DeviceGuard g(x.device());
  check_err(tdg_fp8_quant(x.data_ptr(), y8.data_ptr(), x.numel(), scale.data_ptr<float>(),
                          amax_ptr(amax), (int)fmt, stream_of(x)), "tdg fp8_quant");
}

// y8 = fp8(x) (amax recorded) + per-256-row-block column sums of x into part
void fp8_quant_colsum(const Tensor& x, const Tensor& y8, const Tensor& scale, const Tensor& amax,
                      const Tensor& part, int64_t fmt) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "fp8_quant_colsum: x [M, N], unit inner stride");
  const int64_t M = x.size(0), N = x.size(1);
  check_f8_fmt(y8, fmt, "y8");
  TORCH_CHECK(y8.is_contiguous() && y8.numel() == M * N, "fp8_quant_colsum: y8 [M, N]");
  check_f32(scale, "scale");
  check_f32(part, "part");
  TORCH_CHECK(part.numel() >= ((M + 255) / 256) * N, "fp8_quant_colsum: part [ceil(M/256), N]");
  TORCH_CHECK(N % 8 == 0 && x.stride(0) % 8 == 0, "fp8_quant_colsum: N, ld % 8");
  c10::DeviceGuard g(x.device());
  check_err(tdg_fp8_quant_colsum(x.data_ptr(), (int)x.stride(0), y8.data_ptr(), (int)M, (int)N,
                                 scale.data_ptr<float>(), amax_ptr(amax), part.data_ptr<float>(),
                                 (int)fmt, stream_of(x)),
            "tdg fp8_quant_colsum");
}

// The slot tables of a multi-tensor quantisation: scale f32 [slots], amax [slots, 2048].
void check_slots(const Tensor& scale, const Tensor& amax, const char* what) {
  check_f32(scale, "scale");
  TORCH_CHECK(amax.numel() == 2048 * scale.numel(), what, ": amax is [slots, 2048]");
}

// dsts[g] [C, R] e4m3 = transposed, quantised srcs[g] [R, C] bf16 (slot scales / amax)
void fp8_quant_t(const std::vector<Tensor>& srcs, const std::vector<Tensor>& dsts,
                 const std::vector<int64_t>& slots, const Tensor& scale, const Tensor& amax) {
  const int n = (int)srcs.size();
  TORCH_CHECK(n >= 1 && n <= 64 && (int)dsts.size() == n && (int)slots.size() == n,
              "fp8_quant_t: 1..64 weights");
  check_slots(scale, amax, "fp8_quant_t");
  const int64_t R = srcs[0].size(0), C = srcs[0].size(1);
  std::vector<const void*> sp(n);
  std::vector<void*> dp(n);
  std::vector<int> sl(n);
  for (int i = 0; i < n; ++i) {
    check_bf16(srcs[i], "src");
    check_contig(srcs[i], "src");
    check_f8_fmt(dsts[i], 0, "dst");
    TORCH_CHECK(srcs[i].dim() == 2 && srcs[i].size(0) == R && srcs[i].size(1) == C &&
                    dsts[i].is_contiguous() && dsts[i].numel() == R * C,
                "fp8_quant_t: same-shape [R, C] sources, [C, R] destinations");
    TORCH_CHECK(slots[i] >= 0 && slots[i] < scale.numel(), "fp8_quant_t: slot range");
    sp[i] = srcs[i].data_ptr();
    dp[i] = dsts[i].data_ptr();
    sl[i] = (int)slots[i];
  }
  c10::DeviceGuard g(scale.device());
  check_err(tdg_fp8_quant_t(sp.data(), dp.data(), sl.data(), n, (int)R, (int)C,
                            scale.data_ptr<float>(), amax_ptr(amax), stream_of(scale)),
            "tdg fp8_quant_t");
}

void fp8_quant_multi(const std::vector<Tensor>& xs, const std::vector<Tensor>& ys,
                     const std::vector<int64_t>& slots, const Tensor& scale, const Tensor& amax) {
  const int n = (int)xs.size();
  TORCH_CHECK(n >= 1 && n <= 64 && (int)ys.size() == n && (int)slots.size() == n,
              "fp8_quant_multi: 1..64 tensors, one output and slot each");
  check_slots(scale, amax, "fp8_quant_multi");
  std::vector<const void*> xp(n);
  std::vector<void*> yp(n);
  std::vector<long long> ne(n);
  std::vector<int> sl(n);
  for (int i = 0; i < n; ++i) {
    check_bf16(xs[i], "x");
    check_contig(xs[i], "x");
    check_f8_fmt(ys[i], 0, "y8");
    TORCH_CHECK(ys[i].numel() >= xs[i].numel() && ys[i].is_contiguous(), "fp8_quant_multi: y8");
    TORCH_CHECK(xs[i].device() == scale.device() && ys[i].device() == scale.device(),
                "fp8_quant_multi: one device");
    TORCH_CHECK(slots[i] >= 0 && slots[i] < scale.numel(), "fp8_quant_multi: slot range");
    xp[i] = xs[i].data_ptr();
    yp[i] = ys[i].data_ptr();
    ne[i] = xs[i].numel();
    sl[i] = (int)slots[i];
  }
  c10::DeviceGuard g(scale.device());
  check_err(tdg_fp8_quant_multi(xp.data(), yp.data(), ne.data(), sl.data(), n,
                                scale.data_ptr<float>(), amax_ptr(amax), stream_of(scale)),
            "tdg fp8_quant_multi");
}

void fp8_scale_update(const Tensor& scale, const Tensor& amax, double margin_pow2, double fmax) {
  check_slots(scale, amax, "fp8_scale_update");
  c10::DeviceGuard g(scale.device());
  check_err(tdg_fp8_scale_update(scale.data_ptr<float>(), amax_ptr(amax), (int)scale.numel(),
                                 (float)margin_pow2, (float)fmax, stream_of(scale)), "tdg fp8_scale_update");
}

void fp8_dequant(const Tensor& x8, const Tensor& y, double inv_scale) {
  check_f8_fmt(x8, 0, "x8");
  check_f32(y, "y");
  TORCH_CHECK(y.numel() == x8.numel(), "fp8_dequant: sizes");
  c10::DeviceGuard g(x8.device());
  check_err(tdg_fp8_dequant(x8.data_ptr(), y.data_ptr<float>(), x8.numel(), (float)inv_scale,
                            stream_of(x8)), "tdg fp8_dequant");
}

}  // namespace

void def_fp8(py::module_& m) {
  m.def("gemm_fp8", &gemm_fp8, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"),
        py::arg("sa"), py::arg("sb"), py::arg("C8"), py::arg("sc8"), py::arg("amax"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("ldc8"),
        py::arg("epi"), py::arg("cfg"), py::arg("afmt"), py::arg("cfmt"), py::arg("aux"),
        py::arg("ldaux"), py::arg("beta"), py::arg("aux8") = py::none(),
        py::arg("colsum_out") = py::none(), py::arg("colsum_beta") = 0.0, py::arg("ws") = py::none());
  m.def("wgrad_fp8", &wgrad_fp8);
  m.def("fp8_quant", &fp8_quant);
  m.def("fp8_quant_multi", &fp8_quant_multi);
  m.def("fp8_quant_colsum", &fp8_quant_colsum);
  m.def("fp8_quant_t", &fp8_quant_t);
  m.def("fp8_scale_update", &fp8_scale_update);
  m.def("fp8_dequant", &fp8_dequant);
  m.def("fp8_set_persist", [](int64_t on) { return (int64_t)tdg_fp8_set_persist((int)on); },
        "persistent 128x128 fp8 GEMM on (1) / off (0) / query (-1); returns the previous state");
}
