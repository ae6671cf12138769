// Shared pieces of the Python bindings (module `_C`): the launcher ABI, the
// host-side validation helpers and each kernel family's registration hook.
// Every op launches on the current HIP stream of the tensors' device, takes
// caller-allocated outputs (no allocation inside an op: HIP-graph capturable)
// and validates dtypes / shapes / strides on the host before launching, so a
// kernel never sees operands its grid does not assume.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <cmath>
#include <vector>

#include "tdg_api.h"

using at::Tensor;
using c10::optional;

// One per kernel family (<family>.cpp): its m.def lines, next to the wrappers
// they name. module.cpp calls them all.
void def_gemm(py::module_& m);
void def_attention(py::module_& m);
void def_decode(py::module_& m);
void def_overlap(py::module_& m);
void def_layernorm(py::module_& m);
void def_embedding(py::module_& m);
void def_batch(py::module_& m);
void def_fp8(py::module_& m);
void def_loss(py::module_& m);
void def_distill(py::module_& m);
void def_optimizer(py::module_& m);
void def_ema(py::module_& m);
void def_signal(py::module_& m);

inline hipStream_t stream_of(const Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "tdg op: tensor must be on the GPU");
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}
inline void check_err(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, ": unsupported configuration (rc=", rc, ")");
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, what, ": launch failed: ", hipGetErrorString(e));
}

inline void check_bf16(const Tensor& t, const char* n) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, n, " must be bfloat16");
  TORCH_CHECK(t.is_cuda(), n, " must be a GPU tensor");
}
inline void check_f32(const Tensor& t, const char* n) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, n, " must be float32");
  TORCH_CHECK(t.is_cuda(), n, " must be a GPU tensor");
}
// fmt 0: e4m3 (float8_e4m3fn), 1: e5m2 (float8_e5m2); raw uint8 buffers are
// accepted as untyped storage, a float8 dtype of the other format is not
inline void check_f8_fmt(const Tensor& t, int64_t fmt, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.element_size() == 1, n, " must be a 1-byte (fp8) GPU tensor");
  const auto st = t.scalar_type();
  TORCH_CHECK(st == at::kByte || st == (fmt ? at::kFloat8_e5m2 : at::kFloat8_e4m3fn), n,
              " has dtype ", st, " but the format argument says ", fmt ? "e5m2" : "e4m3");
}
inline void check_contig(const Tensor& t, const char* n) {
  TORCH_CHECK(t.is_contiguous(), n, " must be contiguous");
}
// The data pointer lies on a `bytes` boundary.
inline void check_aligned(const Tensor& t, int bytes, const char* n) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0, n, " must be ", bytes,
              "-byte aligned");
}
// The extent [0, rows*ld) (minus trailing) must lie inside the storage.
inline void check_extent(const Tensor& t, long long rows, long long ld, long long cols,
                         const char* n) {
  const long long need = rows > 0 ? (rows - 1) * ld + cols : 0;
  const long long have = (long long)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
  TORCH_CHECK(need <= have, n, ": operand extent ", need, " exceeds storage ", have);
}
inline int64_t round8(int64_t v) { return (v + 7) / 8 * 8; }

// The members of a mixture (tdg_decode.h MemberRows): bf16 tensors [R, >= V] on
// `dev`, rows contiguous, each with its own row stride, and one number per
// member: its weight, > 0 (the Python wrapper normalises them to sum 1), or,
// with `logs`, the logarithm of that; the kernel gets the logarithms. vec: the
// kernel loads 16 bytes at a time, so every row lies on a 16-byte boundary, the
// strides are multiples of 8 and the columns up to round8(V) lie inside the
// storage; without it any rows of V columns do. `op` and `what` name the call
// and a member in the messages. Members past MEMBERS_MAX are checked but not
// stored: the launcher refuses their count.
inline void check_members(const std::vector<Tensor>& members, int64_t V, const std::vector<double>& w,
                          bool logs, int64_t R, const c10::Device& dev, const char* op,
                          const char* what, bool vec, tdg::MemberRows* out) {
  TORCH_CHECK(w.size() == members.size(), op, ": ", w.size(), " weights for ", members.size(), " ",
              what, " tensors");
  for (size_t m = 0; m < members.size(); ++m) {
    const Tensor& t = members[m];
    check_bf16(t, what);
    TORCH_CHECK(t.device() == dev, op, ": every ", what, " and the other operands on one device");
    TORCH_CHECK(t.dim() == 2 && t.size(0) == R && t.stride(1) == 1 && t.size(1) >= V, op, ": every ",
                what, " must be [R, >= V], rows contiguous");
    const int64_t ld = t.stride(0);
    TORCH_CHECK(ld < (1LL << 31) && (R <= 1 || ld >= (vec ? round8(V) : t.size(1))) &&
                    (!vec || ld % 8 == 0),
                op, ": ", what, " row stride ", ld, vec ? " must be a multiple of 8" : " too small");
    if (vec) check_aligned(t, 16, what);
    check_extent(t, R, ld, vec ? round8(V) : V, what);
    const double lw = logs ? w[m] : std::log(w[m]);
    TORCH_CHECK(std::isfinite(w[m]) && (logs || w[m] > 0) && std::isfinite(lw), op,
                ": weights must be finite and > 0, got ", logs ? std::exp(lw) : w[m]);
    if (m < (size_t)tdg::MEMBERS_MAX) {
      out->x[m] = static_cast<const uint16_t*>(t.data_ptr());
      out->ld[m] = (int)(R > 1 ? ld : t.size(1));  // one row: its stride is never used
      out->logw[m] = (float)lw;
    }
  }
}

// One fp8 amax slot (64 words, 32 apart), or null.
inline unsigned* amax_ptr(const optional<Tensor>& t) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->element_size() == 4 && t->numel() >= 2048,
              "amax must be a 2048-word GPU tensor (one fp8 slot: 64 words, 32 apart)");
  return reinterpret_cast<unsigned*>(t->data_ptr());
}
// The device RNG step counter of the dropout sites, or null.
inline const long long* ctr_ptr(const optional<Tensor>& c) {
  if (!c.has_value()) return nullptr;
  TORCH_CHECK(c->scalar_type() == at::kLong && c->numel() >= 1 && c->is_cuda(),
              "rng counter must be an int64 GPU tensor");
  return reinterpret_cast<const long long*>(c->data_ptr<int64_t>());
}
// Per-batch valid key counts of the attention kernels (int32 [B]), or null.
inline const int* kv_len_ptr(const optional<Tensor>& kv_len, int B) {
  if (!kv_len.has_value()) return nullptr;
  TORCH_CHECK(kv_len->scalar_type() == at::kInt && kv_len->numel() == B, "kv_len: int32 [B]");
  return kv_len->data_ptr<int>();
}
// Data pointer of an optional tensor, or null.
inline void* opt_ptr(const optional<Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }
inline float* opt_f32(const optional<Tensor>& t) {
  return t.has_value() ? t->data_ptr<float>() : nullptr;
}
