// Decoding bindings: single-query attention over an indexed K/V cache and the
// beam-search selection and sampling steps, the ensemble's probability
// average and teacher-forced scoring (decode.hip).
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

void check_i32(const Tensor& t, const char* n) {
  TORCH_CHECK(t.scalar_type() == at::kInt, n, " must be int32");
  TORCH_CHECK(t.is_cuda(), n, " must be a GPU tensor");
}
// int32 [R], contiguous
const int* i32_rows(const Tensor& t, int64_t R, const char* n) {
  check_i32(t, n);
  TORCH_CHECK(t.dim() == 1 && t.numel() == R && t.is_contiguous(), n, " must be int32 [R]");
  return t.data_ptr<int>();
}
// bf16 [R, H, hd] view, hd contiguous, every row slice on a 16-byte boundary
void check_rhd(const Tensor& t, int64_t R, int64_t H, int64_t hd, const char* n) {
  check_bf16(t, n);
  TORCH_CHECK(t.dim() == 3 && t.size(0) == R && t.size(1) == H && t.size(2) == hd &&
                  t.stride(2) == 1,
              n, " must be [R, H, hd] with hd contiguous");
  check_aligned(t, 16, n);
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0, n, ": rows must be 16-byte aligned");
  TORCH_CHECK(t.stride(0) < (1LL << 31) && t.stride(1) < (1LL << 31), n, ": stride too large");
}
// bf16 [n_src, Lk, H, hd] cache view
void check_cache(const Tensor& t, const Tensor& like, int64_t H, int64_t hd, const char* n) {
  check_bf16(t, n);
  TORCH_CHECK(t.dim() == 4 && t.size(2) == H && t.size(3) == hd && t.stride(3) == 1 &&
                  t.size(0) >= 1 && t.size(1) >= 1,
              n, " must be [rows, Lk, H, hd] with hd contiguous");
  TORCH_CHECK(t.size(0) == like.size(0) && t.size(1) == like.size(1), "k / v shape mismatch");
  check_aligned(t, 16, n);
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 && t.stride(2) % 8 == 0, n,
              ": rows must be 16-byte aligned");
  TORCH_CHECK(t.stride(2) < (1LL << 31) && t.size(0) < (1LL << 31) && t.size(1) < (1LL << 31), n,
              ": too large");
}

void decode_attn(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out,
                 const Tensor& kv_len, double scale, const optional<Tensor>& anc,
                 const optional<Tensor>& row_map, const optional<Tensor>& k_new,
                 const optional<Tensor>& v_new) {
  TORCH_CHECK(q.dim() == 3, "q must be [R, H, hd]");
  const int64_t R = q.size(0), H = q.size(1), hd = q.size(2);
  TORCH_CHECK(hd == 16 || hd == 64, "decode_attn: head dim must be 16 or 64, got ", hd);
  check_rhd(q, R, H, hd, "q");
  check_rhd(out, R, H, hd, "out");
  check_cache(k, k, H, hd, "k");
  check_cache(v, k, H, hd, "v");
  tdg::DecodeAttnArgs a{};
  a.kv_len = i32_rows(kv_len, R, "kv_len");
  a.R = (int)R;
  a.H = (int)H;
  a.Lk = (int)k.size(1);
  a.n_src = (int)k.size(0);
  a.scale = (float)scale;
  a.q = (const uint16_t*)q.data_ptr();
  a.out = (uint16_t*)out.data_ptr();
  a.k = (uint16_t*)k.data_ptr();
  a.v = (uint16_t*)v.data_ptr();
  a.q_sr = (int)q.stride(0), a.q_sh = (int)q.stride(1);
  a.o_sr = (int)out.stride(0), a.o_sh = (int)out.stride(1);
  a.k_sr = k.stride(0), a.k_sk = k.stride(1), a.k_sh = (int)k.stride(2);
  a.v_sr = v.stride(0), a.v_sk = v.stride(1), a.v_sh = (int)v.stride(2);
  if (anc.has_value()) {
    check_i32(*anc, "anc");
    TORCH_CHECK(anc->dim() == 2 && anc->size(0) == R && anc->size(1) >= a.Lk &&
                    anc->stride(1) == 1 && anc->stride(0) >= anc->size(1),
                "anc must be int32 [R, >= Lk], rows contiguous");
    a.anc = anc->data_ptr<int>();
    a.ld_anc = (int)anc->stride(0);
  } else if (row_map.has_value()) {
    a.row_map = i32_rows(*row_map, R, "row_map");
  } else {
    TORCH_CHECK(a.n_src >= R, "decode_attn: k / v hold ", a.n_src, " rows, q ", R);
  }
  TORCH_CHECK(k_new.has_value() == v_new.has_value(), "decode_attn: k_new and v_new together");
  if (k_new.has_value()) {
    check_rhd(*k_new, R, H, hd, "k_new");
    check_rhd(*v_new, R, H, hd, "v_new");
    TORCH_CHECK(a.n_src >= R, "decode_attn: fused append needs a cache row per query row");
    a.k_new = (const uint16_t*)k_new->data_ptr();
    a.v_new = (const uint16_t*)v_new->data_ptr();
    a.kn_sr = (int)k_new->stride(0), a.kn_sh = (int)k_new->stride(1);
    a.vn_sr = (int)v_new->stride(0), a.vn_sh = (int)v_new->stride(1);
  }
  c10::DeviceGuard g(q.device());
  check_err(tdg_decode_attn(&a, (int)hd, stream_of(q)), "tdg decode_attn");
}

void beam_topk(const Tensor& logits, int64_t V, const Tensor& score, const Tensor& fin,
               int64_t beam, int64_t end_id, int64_t pad_id, const Tensor& score_out,
               const Tensor& parent, const Tensor& token, const Tensor& fin_out,
               const optional<Tensor>& anc_in, const optional<Tensor>& anc_out, int64_t t) {
  TORCH_CHECK(beam >= 1 && beam <= 8, "beam_topk: beam must be in [1, 8], got ", beam);
  TORCH_CHECK(V >= 1 && V <= 65536, "beam_topk: V must be in [1, 65536], got ", V);
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(1) >= V,
              "logits must be [R, >= V], rows contiguous");
  const int64_t R = logits.size(0), ldl = logits.stride(0);
  TORCH_CHECK(R % beam == 0, "beam_topk: rows ", R, " not a multiple of beam ", beam);
  TORCH_CHECK(ldl % 8 == 0 && ldl >= round8(V), "beam_topk: logits row stride must be a multiple of 8");
  check_aligned(logits, 16, "logits");
  check_extent(logits, R, ldl, round8(V), "logits");
  TORCH_CHECK(pad_id >= 0 && pad_id < V && end_id >= 0 && end_id < V, "beam_topk: pad / end id");
  check_f32(score, "score");
  check_f32(score_out, "score_out");
  TORCH_CHECK(score.numel() == R && score.is_contiguous() && score_out.numel() == R &&
                  score_out.is_contiguous(),
              "score / score_out must be f32 [R]");
  tdg::BeamTopkArgs a{};
  a.logits = (const uint16_t*)logits.data_ptr();
  a.score = score.data_ptr<float>();
  a.score_out = score_out.data_ptr<float>();
  a.fin = i32_rows(fin, R, "fin");
  a.parent = (int*)i32_rows(parent, R, "parent");
  a.token = (int*)i32_rows(token, R, "token");
  a.fin_out = (int*)i32_rows(fin_out, R, "fin_out");
  a.B = (int)(R / beam);
  a.beam = (int)beam;
  a.V = (int)V;
  a.ldl = (int)ldl;
  a.end_id = (int)end_id;
  a.pad_id = (int)pad_id;
  TORCH_CHECK(anc_in.has_value() == anc_out.has_value(), "beam_topk: anc_in and anc_out together");
  if (anc_in.has_value()) {
    for (const Tensor* x : {&*anc_in, &*anc_out}) {
      check_i32(*x, "anc");
      TORCH_CHECK(x->dim() == 2 && x->size(0) == R && x->stride(1) == 1 && t >= 0 &&
                      t + 1 < x->size(1) && x->stride(0) == anc_in->stride(0) &&
                      x->stride(0) >= x->size(1),
                  "anc_in / anc_out must be int32 [R, > t + 1] with equal row strides");
    }
    TORCH_CHECK(anc_in->data_ptr() != anc_out->data_ptr(), "beam_topk: anc_out must not alias anc_in");
    a.anc_in = anc_in->data_ptr<int>();
    a.anc_out = anc_out->data_ptr<int>();
    a.ld_anc = (int)anc_in->stride(0);
    a.t = (int)t;
  }
  c10::DeviceGuard g(logits.device());
  check_err(tdg_beam_topk(&a, stream_of(logits)), "tdg beam_topk");
}

void sample_token(const Tensor& logits, int64_t V, const Tensor& score, const Tensor& fin,
                  int64_t end_id, int64_t pad_id, double temperature, int64_t top_k, double top_p,
                  int64_t seed, int64_t step, const optional<Tensor>& row_id,
                  const Tensor& score_out, const Tensor& token, const Tensor& fin_out) {
  TORCH_CHECK(V >= 1 && V <= 65536, "sample_token: V must be in [1, 65536], got ", V);
  TORCH_CHECK(std::isfinite(temperature) && temperature > 0 && (float)temperature > 0.f,
              "sample_token: temperature must be finite and > 0, got ", temperature);
  TORCH_CHECK(top_p > 0 && top_p <= 1 && (float)top_p > 0.f,
              "sample_token: top_p must be in (0, 1], got ", top_p);
  TORCH_CHECK(top_k >= 0, "sample_token: top_k must be >= 0, got ", top_k);
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(1) >= V,
              "logits must be [R, >= V], rows contiguous");
  const int64_t R = logits.size(0), ldl = logits.stride(0);
  TORCH_CHECK(R < (1LL << 31) && ldl < (1LL << 31), "sample_token: logits too large");
  TORCH_CHECK(ldl % 8 == 0 && ldl >= round8(V),
              "sample_token: logits row stride must be a multiple of 8");
  check_aligned(logits, 16, "logits");
  check_extent(logits, R, ldl, round8(V), "logits");
  TORCH_CHECK(pad_id >= 0 && pad_id < V && end_id >= 0 && end_id < V, "sample_token: pad / end id");
  check_f32(score, "score");
  check_f32(score_out, "score_out");
  TORCH_CHECK(score.numel() == R && score.is_contiguous() && score_out.numel() == R &&
                  score_out.is_contiguous(),
              "score / score_out must be f32 [R]");
  tdg::SampleArgs a{};
  a.logits = (const uint16_t*)logits.data_ptr();
  a.score = score.data_ptr<float>();
  a.score_out = score_out.data_ptr<float>();
  a.fin = i32_rows(fin, R, "fin");
  a.row_id = row_id.has_value() ? i32_rows(*row_id, R, "row_id") : nullptr;
  a.token = (int*)i32_rows(token, R, "token");
  a.fin_out = (int*)i32_rows(fin_out, R, "fin_out");
  a.seed = (unsigned long long)seed;
  a.step = (unsigned long long)step;
  a.temperature = (float)temperature;
  a.top_p = (float)top_p;
  a.top_k = (int)std::min<int64_t>(top_k, 1 << 30);  // beyond V: off
  a.R = (int)R;
  a.V = (int)V;
  a.ldl = (int)ldl;
  a.end_id = (int)end_id;
  a.pad_id = (int)pad_id;
  c10::DeviceGuard g(logits.device());
  check_err(tdg_sample_token(&a, stream_of(logits)), "tdg sample_token");
}

void ensemble_logprobs(const std::vector<Tensor>& logits, int64_t V,
                       const std::vector<double>& weights, const Tensor& out) {
  const int64_t M = (int64_t)logits.size();
  TORCH_CHECK(M >= 1 && M <= tdg::ENSEMBLE_MAX, "ensemble_logprobs: 1 to ", tdg::ENSEMBLE_MAX,
              " members, got ", M);
  TORCH_CHECK(V >= 1 && V <= 65536, "ensemble_logprobs: V must be in [1, 65536], got ", V);
  check_bf16(out, "out");
  TORCH_CHECK(out.dim() == 2 && out.stride(1) == 1 && out.size(1) >= V && out.size(1) % 8 == 0,
              "out must be [R, >= V] with a multiple of 8 columns, rows contiguous");
  const int64_t R = out.size(0), No = out.size(1), ldo = out.stride(0);
  TORCH_CHECK(R < (1LL << 31) && ldo < (1LL << 31), "ensemble_logprobs: out too large");
  TORCH_CHECK(ldo % 8 == 0 && (ldo >= No || R <= 1),
              "ensemble_logprobs: out row stride must be a multiple of 8");
  check_aligned(out, 16, "out");
  check_extent(out, R, ldo, No, "out");
  tdg::EnsembleArgs a{};
  check_members(logits, V, weights, false, R, out.device(), "ensemble_logprobs", "logits", true, &a.mem);
  a.out = (uint16_t*)out.data_ptr();
  a.M = (int)M;
  a.R = (int)R;
  a.V = (int)V;
  a.ldo = (int)ldo;
  a.No = (int)No;
  c10::DeviceGuard g(out.device());
  check_err(tdg_ensemble_logprobs(&a, stream_of(out)), "tdg ensemble_logprobs");
}

// labels: int32 or int64 [R]; tok_lp and (optional) top_lp: f32 [R]; all on
// the members' device, R the members' row count
void score_tokens(const std::vector<Tensor>& logits, int64_t V, const std::vector<double>& weights,
                  const Tensor& labels, int64_t pad_id, const Tensor& tok_lp,
                  const optional<Tensor>& top_lp) {
  const int64_t M = (int64_t)logits.size();
  TORCH_CHECK(M >= 1 && M <= tdg::ENSEMBLE_MAX, "score_tokens: 1 to ", tdg::ENSEMBLE_MAX,
              " members, got ", M);
  TORCH_CHECK(V >= 1 && V <= 65536, "score_tokens: V must be in [1, 65536], got ", V);
  TORCH_CHECK(logits[0].dim() == 2, "every member's logits must be [R, >= V], rows contiguous");
  const int64_t R = logits[0].size(0);
  TORCH_CHECK(R < (1LL << 31), "score_tokens: too many rows");
  TORCH_CHECK(logits[0].is_cuda(), "logits must be a GPU tensor");
  const c10::Device dev = logits[0].device();
  const auto lt = labels.scalar_type();
  TORCH_CHECK(lt == at::kInt || lt == at::kLong, "labels must be int32 or int64");
  TORCH_CHECK(labels.device() == dev && labels.dim() == 1 && labels.numel() == R &&
                  labels.is_contiguous(),
              "labels must be [R] on the members' device");
  TORCH_CHECK(pad_id >= INT32_MIN && pad_id <= INT32_MAX, "score_tokens: pad_id");
  for (const Tensor* o : {&tok_lp, top_lp.has_value() ? &*top_lp : &tok_lp}) {
    check_f32(*o, "tok_lp / top_lp");
    TORCH_CHECK(o->device() == dev && o->dim() == 1 && o->numel() == R && o->is_contiguous(),
                "tok_lp / top_lp must be f32 [R] on the members' device");
  }
  tdg::ScoreArgs a{};
  check_members(logits, V, weights, false, R, dev, "score_tokens", "logits", true, &a.mem);
  a.labels = labels.data_ptr();
  a.lab64 = lt == at::kLong ? 1 : 0;
  a.tok_lp = tok_lp.data_ptr<float>();
  a.top_lp = opt_f32(top_lp);
  a.M = (int)M;
  a.R = (int)R;
  a.V = (int)V;
  a.pad_id = (int)pad_id;
  c10::DeviceGuard g(dev);
  check_err(tdg_score_tokens(&a, stream_of(tok_lp)), "tdg score_tokens");
}

}  // namespace

void def_decode(py::module_& m) {
  namespace py = pybind11;
  m.def("decode_attn", &decode_attn, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"),
        py::arg("kv_len"), py::arg("scale"), py::arg("anc") = py::none(),
        py::arg("row_map") = py::none(), py::arg("k_new") = py::none(),
        py::arg("v_new") = py::none());
  m.def("beam_topk", &beam_topk, py::arg("logits"), py::arg("V"), py::arg("score"), py::arg("fin"),
        py::arg("beam"), py::arg("end_id"), py::arg("pad_id"), py::arg("score_out"),
        py::arg("parent"), py::arg("token"), py::arg("fin_out"), py::arg("anc_in") = py::none(),
        py::arg("anc_out") = py::none(), py::arg("t") = 0);
  m.def("sample_token", &sample_token, py::arg("logits"), py::arg("V"), py::arg("score"),
        py::arg("fin"), py::arg("end_id"), py::arg("pad_id"), py::arg("temperature"),
        py::arg("top_k"), py::arg("top_p"), py::arg("seed"), py::arg("step"), py::arg("row_id"),
        py::arg("score_out"), py::arg("token"), py::arg("fin_out"));
  m.def("ensemble_logprobs", &ensemble_logprobs, py::arg("logits"), py::arg("V"),
        py::arg("weights"), py::arg("out"));
  m.def("score_tokens", &score_tokens, py::arg("logits"), py::arg("V"), py::arg("weights"),
        py::arg("labels"), py::arg("pad_id"), py::arg("tok_lp"), py::arg("top_lp") = py::none());
}
