// Optimizer bindings (adam.hip): Adam over the flat parameter buffer, the
// global gradient norm for clipping / step skipping, and the bf16 shadow and
// transposed weight copies.
#include "common.h"

namespace {

// The device state of the gradient-norm pass (grad_norm_finalize), or null.
const float* norm_state_ptr(const optional<Tensor>& gstate, const Tensor& like) {
  if (!gstate.has_value()) return nullptr;
  check_f32(*gstate, "norm state");
  TORCH_CHECK(gstate->is_cuda() && gstate->device() == like.device() && gstate->is_contiguous() &&
                  gstate->numel() >= 4,
              "norm state: >= 4 contiguous f32 on the gradient's GPU");
  return gstate->data_ptr<float>();
}
// p / g / m / v: contiguous f32 flat buffers of one size
void check_adam_buffers(const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v) {
  for (auto* t : {&p, &g, &m, &v}) {
    check_f32(*t, "adam buffers");
    check_contig(*t, "adam buffers");
    TORCH_CHECK(t->numel() == p.numel(), "adam: buffer sizes differ");
  }
}
long long* step_ptr(const Tensor& step) {
  TORCH_CHECK(step.scalar_type() == at::kLong && step.is_cuda(), "adam: step int64 GPU");
  return reinterpret_cast<long long*>(step.data_ptr<int64_t>());
}
// A chunk table [n, 4] int64 (start, n, fp8 slot or -1, e4m3 address or 0)
// over a flat buffer of `numel` elements. Its CONTENTS (start + n <= numel,
// n <= 4096, n % 4 == 0, slot < scale8.numel(), live e4m3 addresses) are
// validated on the host where it is built (ops/fp8.py validate_chunk_table:
// Fp8Weights.adam_chunks and Adam.apply_range) -- reading it back here would
// be a device sync inside the captured step. Here: its size against the buffer.
void check_chunk_table(const Tensor& chunks, int64_t numel, const char* what) {
  TORCH_CHECK(chunks.is_cuda() && chunks.scalar_type() == at::kLong && chunks.dim() == 2 &&
                  chunks.size(1) == 4 && chunks.is_contiguous(),
              what, ": chunk table [n, 4] int64 on the GPU");
  TORCH_CHECK(chunks.size(0) >= 1 && chunks.size(0) <= (numel + 3) / 4, what,
              ": chunk count out of range for the flat buffer");
}

void adam(const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v,
          const optional<Tensor>& shadow, const Tensor& step, double beta1, double beta2,
          double eps, double lr_const, double d_model, double warmup, double grad_scale,
          double weight_decay, int64_t sched, bool zero_grad, bool inc_step,
          const optional<Tensor>& gstate) {
  check_adam_buffers(p, g, m, v);
  TORCH_CHECK(p.numel() % 4 == 0, "adam: flat buffer must be a multiple of 4");
  if (shadow.has_value()) {
    check_bf16(*shadow, "shadow");
    TORCH_CHECK(shadow->numel() == p.numel(), "adam: shadow size");
  }
  long long* sp = step_ptr(step);
  c10::DeviceGuard gd(p.device());
  check_err(tdg_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), opt_ptr(shadow), p.numel(), sp, (float)beta1,
                     (float)beta2, (float)eps, (float)lr_const, (float)d_model, (float)warmup,
                     (float)grad_scale, (float)weight_decay, (int)sched, zero_grad, inc_step,
                     norm_state_ptr(gstate, p), stream_of(p)),
            "tdg adam");
}

// Adam over a chunk table built by ops/fp8.py Fp8Weights.adam_chunks: the
// weights with e4m3 copies get them refreshed in the same pass.
void adam_chunks(const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v,
                 const Tensor& shadow, const Tensor& chunks, const Tensor& step, double beta1,
                 double beta2, double eps, double lr_const, double d_model, double warmup,
                 double grad_scale, double weight_decay, int64_t sched, bool zero_grad,
                 bool inc_step, const Tensor& scale8, const Tensor& amax8,
                 const optional<Tensor>& gstate) {
  check_adam_buffers(p, g, m, v);
  check_bf16(shadow, "shadow");
  TORCH_CHECK(shadow.numel() == p.numel() && p.numel() % 4 == 0 && p.numel() < (1LL << 28),
              "adam_chunks: shadow size / flat size");
  check_chunk_table(chunks, p.numel(), "adam_chunks");
  long long* sp = step_ptr(step);
  check_f32(scale8, "scale8");
  TORCH_CHECK(amax8.numel() >= 2048, "adam_chunks: amax slot table");
  c10::DeviceGuard gd(p.device());
  check_err(tdg_adam_chunks(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                            v.data_ptr<float>(), shadow.data_ptr(), p.numel(), chunks.data_ptr(),
                            (int)chunks.size(0), sp, (float)beta1, (float)beta2, (float)eps,
                            (float)lr_const, (float)d_model, (float)warmup, (float)grad_scale,
                            (float)weight_decay, (int)sched, zero_grad, inc_step,
                            scale8.data_ptr<float>(),
                            reinterpret_cast<unsigned*>(amax8.data_ptr()),
                            norm_state_ptr(gstate, p), stream_of(p)),
            "tdg adam_chunks");
}

void adam_step_inc(const Tensor& step, const optional<Tensor>& gstate) {
  long long* sp = step_ptr(step);
  c10::DeviceGuard gd(step.device());
  check_err(tdg_adam_step_inc(sp, norm_state_ptr(gstate, step), stream_of(step)),
            "tdg adam_step_inc");
}

// partials[base ..) = one squared sum per <= 4096-element chunk of g: the
// chunks of an Adam chunk table, or without a table the consecutive
// 4096-element pieces of g (numel % 4 == 0). Returns how many partials were
// written.
int64_t grad_sumsq(const Tensor& g, const optional<Tensor>& chunks, const Tensor& partials,
                   int64_t base) {
  check_f32(g, "grad_sumsq gradient");
  check_contig(g, "grad_sumsq gradient");
  check_f32(partials, "grad_sumsq partials");
  check_contig(partials, "grad_sumsq partials");
  TORCH_CHECK(g.is_cuda() && partials.device() == g.device(), "grad_sumsq: GPU tensors");
  check_aligned(g, 16, "grad_sumsq: gradient range start");
  int64_t nch;
  const void* tab = nullptr;
  if (chunks.has_value()) {
    check_chunk_table(*chunks, g.numel(), "grad_sumsq");
    nch = chunks->size(0);
    tab = chunks->data_ptr();
  } else {
    TORCH_CHECK(g.numel() > 0 && g.numel() % 4 == 0, "grad_sumsq: length must be a multiple of 4");
    nch = (g.numel() + 4095) / 4096;
  }
  TORCH_CHECK(base >= 0 && base + nch <= partials.numel(), "grad_sumsq: partials buffer too small");
  c10::DeviceGuard gd(g.device());
  const long long r = tdg_grad_sumsq(g.data_ptr<float>(), tab, nch, g.numel(),
                                     partials.data_ptr<float>() + base, stream_of(g));
  TORCH_CHECK(r == nch, "tdg grad_sumsq failed");
  return nch;
}

// state (f32 [>= 4]: squared sum, norm, clip factor, skip flag) and counters
// (int32 [>= 4]: steps clipped, steps skipped, bits of the largest finite
// norm) from partials[0 .. nparts).
void grad_norm_finalize(const Tensor& partials, int64_t nparts, const Tensor& state,
                        const Tensor& counters, double clip, bool skip_on, double grad_scale) {
  check_f32(partials, "grad_norm_finalize partials");
  check_contig(partials, "grad_norm_finalize partials");
  TORCH_CHECK(nparts >= 0 && nparts <= partials.numel(), "grad_norm_finalize: partial count");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.is_contiguous() &&
                  counters.numel() >= 4 && counters.device() == partials.device(),
              "grad_norm_finalize: counters int32 [>= 4] on the GPU");
  const optional<Tensor> st(state);
  float* sp = const_cast<float*>(norm_state_ptr(st, partials));
  c10::DeviceGuard gd(partials.device());
  check_err(tdg_grad_norm_finalize(partials.data_ptr<float>(), nparts, sp,
                                   reinterpret_cast<unsigned*>(counters.data_ptr<int>()),
                                   (float)clip, skip_on, (float)grad_scale, stream_of(partials)),
            "tdg grad_norm_finalize");
}

// dsts[g] [C, R] = srcs[g] [R, C]^T (bf16, same shape, <= 64 matrices, one launch)
void transpose_grouped(const std::vector<Tensor>& srcs, const std::vector<Tensor>& dsts) {
  const size_t G = srcs.size();
  TORCH_CHECK(G >= 1 && G <= 64 && dsts.size() == G, "transpose_grouped: 1..64 matrices");
  const int64_t R = srcs[0].size(0), C = srcs[0].size(1);
  TORCH_CHECK(R % 8 == 0 && C % 8 == 0, "transpose_grouped: rows and columns multiples of 8");
  std::vector<const void*> s(G);
  std::vector<void*> d(G);
  for (size_t i = 0; i < G; ++i) {
    check_bf16(srcs[i], "src");
    check_bf16(dsts[i], "dst");
    TORCH_CHECK(srcs[i].dim() == 2 && srcs[i].size(0) == R && srcs[i].size(1) == C &&
                    srcs[i].is_contiguous(), "transpose_grouped: same-shape contiguous sources");
    TORCH_CHECK(dsts[i].dim() == 2 && dsts[i].size(0) == C && dsts[i].size(1) == R &&
                    dsts[i].is_contiguous(), "transpose_grouped: dst must be [C, R]");
    check_aligned(srcs[i], 16, "transpose_grouped: src");
    check_aligned(dsts[i], 16, "transpose_grouped: dst");
    s[i] = srcs[i].data_ptr();
    d[i] = dsts[i].data_ptr();
  }
  c10::DeviceGuard g(srcs[0].device());
  check_err(tdg_transpose_grouped(s.data(), d.data(), (int)G, (int)R, (int)C, stream_of(srcs[0])),
            "tdg transpose_grouped");
}

// o = bf16(p): the bf16 shadow of an f32 parameter range (same element count)
void to_bf16(const Tensor& p, const Tensor& o) {
  check_f32(p, "p");
  check_bf16(o, "o");
  TORCH_CHECK(p.numel() == o.numel() && p.is_contiguous() && o.is_contiguous(), "to_bf16 shape");
  c10::DeviceGuard g(p.device());
  check_err(tdg_to_bf16(p.data_ptr<float>(), o.data_ptr(), p.numel(), stream_of(p)),
            "tdg to_bf16");
}

}  // namespace

void def_optimizer(py::module_& m) {
  m.def("adam", &adam);
  m.def("adam_chunks", &adam_chunks);
  m.def("adam_step_inc", &adam_step_inc);
  m.def("grad_sumsq", &grad_sumsq);
  m.def("grad_norm_finalize", &grad_norm_finalize);
  m.def("transpose_grouped", &transpose_grouped);
  m.def("to_bf16", &to_bf16);
}
