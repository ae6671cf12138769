// Weight-EMA binding (ema.hip): one update of (a range of) the averaged copy
// of the flat f32 master buffer.
#include "common.h"

namespace {

// e += (p - e) * (1 - d_eff) over two same-size contiguous f32 ranges; count:
// the device-resident int64 update count; gstate: the gradient-norm pass's
// device state, or none. The length and the decay are the launcher's to
// refuse (rc -1, nothing launched).
void ema(const Tensor& p, const Tensor& e, const Tensor& count, double decay, bool warmup,
         bool inc_count, const optional<Tensor>& gstate) {
  check_f32(p, "ema weights");
  check_f32(e, "ema average");
  check_contig(p, "ema weights");
  check_contig(e, "ema average");
  TORCH_CHECK(e.numel() == p.numel() && e.device() == p.device(), "ema: buffer sizes / devices differ");
  check_aligned(p, 16, "ema: weight range start");
  check_aligned(e, 16, "ema: average range start");
  TORCH_CHECK(count.scalar_type() == at::kLong && count.is_cuda() && count.numel() >= 1 &&
                  count.device() == p.device(),
              "ema: count int64 on the weights' GPU");
  const float* gs = nullptr;
  if (gstate.has_value()) {
    check_f32(*gstate, "norm state");
    TORCH_CHECK(gstate->device() == p.device() && gstate->is_contiguous() && gstate->numel() >= 4,
                "norm state: >= 4 contiguous f32 on the weights' GPU");
    gs = gstate->data_ptr<float>();
  }
  c10::DeviceGuard gd(p.device());
  check_err(tdg_ema(p.data_ptr<float>(), e.data_ptr<float>(), p.numel(),
                    reinterpret_cast<long long*>(count.data_ptr<int64_t>()), (float)decay, warmup,
                    inc_count, gs, stream_of(p)),
            "tdg ema");
}

}  // namespace

void def_ema(py::module_& m) { m.def("ema", &ema); }
