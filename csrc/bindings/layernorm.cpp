// LayerNorm bindings: fused (dropout + residual +) LayerNorm forward /
// backward and the deferred fold of its dgamma / dbeta partials.
#include "common.h"

namespace {

// A contiguous tensor with as many elements as `like`.
void check_same_numel(const Tensor& t, const Tensor& like, const char* n) {
  TORCH_CHECK(t.numel() == like.numel() && t.is_contiguous(), "ln: ", n, " shape");
}
// dropout keep-bit bitmap of a [M, D] LayerNorm: uint8 [M, D / 8], D >= 512
void check_ln_kbits(const optional<Tensor>& kbits, int64_t M, int64_t D) {
  if (!kbits.has_value()) return;
  TORCH_CHECK(kbits->is_cuda() && kbits->scalar_type() == at::kByte && kbits->is_contiguous() &&
                  kbits->numel() == M * D / 8 && D >= 512,
              "ln: kbits uint8 [M, D / 8] (D >= 512)");
}

void ln_fwd(const Tensor& x, const optional<Tensor>& s, const Tensor& gamma, const Tensor& beta,
            const Tensor& y, const optional<Tensor>& hsave, const optional<Tensor>& mean,
            const optional<Tensor>& rstd, double p, int64_t seed, const optional<Tensor>& ctr,
            int64_t site, double eps, const optional<Tensor>& y8, const optional<Tensor>& s8,
            const optional<Tensor>& amax8, const optional<Tensor>& kbits) {
  check_bf16(x, "x");
  check_contig(x, "x");
  const int64_t D = x.size(-1), M = x.numel() / D;
  check_bf16(y, "y");
  check_same_numel(y, x, "y");
  if (s.has_value()) {
    check_bf16(*s, "s");
    check_same_numel(*s, x, "s");
  }
  check_f32(gamma, "gamma");
  check_f32(beta, "beta");
  TORCH_CHECK(gamma.numel() == D && beta.numel() == D, "ln: gamma/beta shape");
  if (hsave.has_value()) {
    check_bf16(*hsave, "hsave");
    check_same_numel(*hsave, x, "hsave");
  }
  for (auto* t : {&mean, &rstd})
    if (t->has_value()) {
      check_f32(**t, "mean/rstd");
      TORCH_CHECK((*t)->numel() == M, "ln: mean/rstd shape");
    }
  if (y8.has_value()) {
    check_f8_fmt(*y8, 0, "y8");
    check_same_numel(*y8, x, "y8");
    TORCH_CHECK(s8.has_value(), "ln: y8 needs s8");
    check_f32(*s8, "s8");
  }
  check_ln_kbits(kbits, M, D);
  TORCH_CHECK(!kbits.has_value() || s.has_value(), "ln: kbits are the dropout on s");
  c10::DeviceGuard g(x.device());
  const int rc = tdg_ln_fwd(x.data_ptr(), opt_ptr(s), gamma.data_ptr<float>(),
                            beta.data_ptr<float>(), y.data_ptr(), opt_ptr(hsave), opt_f32(mean),
                            opt_f32(rstd), (int)M, (int)D, (float)p, (uint64_t)seed, ctr_ptr(ctr),
                            (uint64_t)site, (float)eps, opt_ptr(y8), opt_f32(s8), amax_ptr(amax8),
                            opt_ptr(kbits), stream_of(x));
  check_err(rc, "tdg ln_fwd");
}

void ln_bwd(const Tensor& dy, const Tensor& hsave, const Tensor& mean, const Tensor& rstd,
            const Tensor& gamma, const Tensor& dh, const optional<Tensor>& ds,
            const optional<Tensor>& dres, const Tensor& dgamma, const Tensor& dbeta,
            const optional<Tensor>& dbias, const Tensor& ws, double p, int64_t seed,
            const optional<Tensor>& ctr, int64_t site, bool accumulate, bool skip_reduce,
            int64_t rpb, const optional<Tensor>& ds8, const optional<Tensor>& s8,
            const optional<Tensor>& amax8, const optional<Tensor>& kbits) {
  check_bf16(dy, "dy");
  check_contig(dy, "dy");
  const int64_t D = dy.size(-1), M = dy.numel() / D;
  for (auto* t : {&hsave, &dh}) {
    check_bf16(*t, "hsave/dh");
    check_same_numel(*t, dy, "hsave/dh");
  }
  for (auto* t : {&ds, &dres})
    if (t->has_value()) {
      check_bf16(**t, "ds/dres");
      check_same_numel(**t, dy, "ds/dres");
    }
  check_f32(mean, "mean");
  check_f32(rstd, "rstd");
  check_f32(gamma, "gamma");
  check_f32(dgamma, "dgamma");
  check_f32(dbeta, "dbeta");
  TORCH_CHECK(mean.numel() == M && rstd.numel() == M, "ln_bwd: mean/rstd shape");
  TORCH_CHECK(gamma.numel() == D && dgamma.numel() == D && dbeta.numel() == D, "ln_bwd: D");
  if (dbias.has_value()) {
    check_f32(*dbias, "dbias");
    TORCH_CHECK(dbias->numel() == D && (ds.has_value() || ds8.has_value()), "ln_bwd: dbias needs ds");
  }
  if (ds8.has_value()) {
    check_f8_fmt(*ds8, 1, "ds8 (e5m2)");
    check_same_numel(*ds8, dy, "ds8");
    TORCH_CHECK(s8.has_value(), "ln_bwd: ds8 needs s8");
    check_f32(*s8, "s8");
  }
  check_f32(ws, "ws");
  TORCH_CHECK(rpb == 16 || rpb == 32 || rpb == 64, "ln_bwd: rows per block 16 / 32 / 64");
  TORCH_CHECK(ws.numel() >= 3 * ((M + rpb - 1) / rpb) * D, "ln_bwd: workspace too small");
  check_ln_kbits(kbits, M, D);
  c10::DeviceGuard g(dy.device());
  const int rc = tdg_ln_bwd(
      dy.data_ptr(), hsave.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
      gamma.data_ptr<float>(), dh.data_ptr(), opt_ptr(ds), opt_ptr(dres), dgamma.data_ptr<float>(),
      dbeta.data_ptr<float>(), opt_f32(dbias), ws.data_ptr<float>(), (int)M, (int)D, (float)p,
      (uint64_t)seed, ctr_ptr(ctr), (uint64_t)site, accumulate, skip_reduce, (int)rpb,
      opt_ptr(ds8), opt_f32(s8), amax_ptr(amax8), opt_ptr(kbits), stream_of(dy));
  check_err(rc, "tdg ln_bwd");
}

// Deferred LayerNorm partial folds: outs[g] (=|+=) column sums of parts[g]
// ([nparts[g], N] f32 each), one launch.
void reduce_partials_multi(const std::vector<Tensor>& parts, const std::vector<Tensor>& outs,
                           const std::vector<int64_t>& nparts, int64_t N, double beta) {
  const size_t G = parts.size();
  TORCH_CHECK(G >= 1 && G <= 96 && outs.size() == G && nparts.size() == G,
              "reduce_partials_multi: 1..96 problems");
  std::vector<const float*> pp(G);
  std::vector<float*> oo(G);
  std::vector<int> np(G);
  for (size_t i = 0; i < G; ++i) {
    check_f32(parts[i], "parts");
    check_f32(outs[i], "outs");
    check_contig(parts[i], "parts");
    TORCH_CHECK(outs[i].numel() == N && outs[i].is_contiguous(), "reduce_partials_multi: out");
    TORCH_CHECK(parts[i].numel() >= nparts[i] * N, "reduce_partials_multi: partials too small");
    TORCH_CHECK(parts[i].device() == parts[0].device() && outs[i].device() == parts[0].device(),
                "reduce_partials_multi: one device");
    pp[i] = parts[i].data_ptr<float>();
    oo[i] = outs[i].data_ptr<float>();
    np[i] = (int)nparts[i];
  }
  c10::DeviceGuard g(parts[0].device());
  check_err(tdg_reduce_partials_multi(pp.data(), oo.data(), np.data(), (int)G, (int)N, (float)beta,
                                      stream_of(parts[0])),
            "tdg reduce_partials_multi");
}

}  // namespace

void def_layernorm(py::module_& m) {
  m.def("ln_fwd", &ln_fwd);
  m.def("ln_bwd", &ln_bwd);
  m.def("reduce_partials_multi", &reduce_partials_multi);
}
