// Embedding bindings: lookup + positional encoding + dropout forward, and the
// atomic, fixed-point and sorted (CSR) table-gradient backwards.
#include "common.h"

namespace {

// Token ids of any shape: contiguous int32 / int64 on the GPU. Returns whether int64.
bool check_tok(const Tensor& tok) {
  TORCH_CHECK(tok.is_contiguous() && tok.is_cuda(), "tok must be a contiguous GPU tensor");
  const bool t64 = tok.scalar_type() == at::kLong;
  TORCH_CHECK(t64 || tok.scalar_type() == at::kInt, "tok must be int32/int64");
  return t64;
}
// The backward's operands: dout bf16 [M, D], dtable f32 [V, D], both contiguous.
void check_grads(const Tensor& dout, const Tensor& dtable, int64_t M) {
  check_bf16(dout, "dout");
  check_contig(dout, "dout");
  check_f32(dtable, "dtable");
  check_contig(dtable, "dtable");
  TORCH_CHECK(dout.numel() == M * dtable.size(1), "dout shape");
}
// dropout keep-bit bitmap of [M, D] activations: uint8 [M, D / 8]
void check_kbits(const optional<Tensor>& kbits, int64_t M, int64_t D) {
  if (!kbits.has_value()) return;
  TORCH_CHECK(kbits->is_cuda() && kbits->scalar_type() == at::kByte && kbits->is_contiguous() &&
                  kbits->numel() == M * D / 8,
              "kbits: uint8 [M, D / 8]");
  check_aligned(*kbits, 4, "kbits");
}

void embed_fwd(const Tensor& tok, const Tensor& table, const Tensor& pe, const Tensor& out,
               double scale, double p, int64_t seed, const optional<Tensor>& ctr, int64_t site,
               const optional<Tensor>& kbits) {
  TORCH_CHECK(tok.dim() == 2, "tok must be [B,L]");
  const bool t64 = check_tok(tok);
  check_bf16(table, "table");
  check_contig(table, "table");
  check_f32(pe, "pe");
  check_contig(pe, "pe");
  check_bf16(out, "out");
  check_contig(out, "out");
  const int64_t D = table.size(1), L = tok.size(1), M = tok.numel();
  TORCH_CHECK(pe.dim() == 2 && pe.size(1) == D && pe.size(0) >= L, "pe table too short");
  TORCH_CHECK(out.numel() == M * D, "out shape");
  check_kbits(kbits, M, D);
  c10::DeviceGuard g(tok.device());
  const int rc = tdg_embed_fwd(tok.data_ptr(), t64, table.data_ptr(), pe.data_ptr<float>(),
                               out.data_ptr(), (int)M, (int)L, (int)D, (float)scale, (float)p,
                               (uint64_t)seed, ctr_ptr(ctr), (uint64_t)site, opt_ptr(kbits),
                               stream_of(tok));
  check_err(rc, "tdg embed_fwd");
}

void embed_bwd(const Tensor& tok, const Tensor& dout, const Tensor& dtable, double scale,
               double p, int64_t seed, const optional<Tensor>& ctr, int64_t site) {
  const bool t64 = check_tok(tok);
  const int64_t D = dtable.size(1), M = tok.numel();
  check_grads(dout, dtable, M);
  c10::DeviceGuard g(tok.device());
  const int rc = tdg_embed_bwd(tok.data_ptr(), t64, dout.data_ptr(), dtable.data_ptr<float>(),
                               (int)M, (int)D, (float)scale, (float)p, (uint64_t)seed,
                               ctr_ptr(ctr), (uint64_t)site, stream_of(tok));
  check_err(rc, "tdg embed_bwd");
}

// Deterministic: acc is an all-zero int64 [V, D] scratch (left all-zero).
void embed_bwd_det(const Tensor& tok, const Tensor& dout, const Tensor& dtable, const Tensor& acc,
                   double scale, double p, int64_t seed, const optional<Tensor>& ctr, int64_t site,
                   bool accumulate) {
  const bool t64 = check_tok(tok);
  const int64_t D = dtable.size(1), M = tok.numel(), V = dtable.size(0);
  check_grads(dout, dtable, M);
  TORCH_CHECK(acc.scalar_type() == at::kLong && acc.is_cuda() && acc.is_contiguous(), "acc int64");
  TORCH_CHECK(acc.numel() >= dtable.numel(), "acc too small");
  c10::DeviceGuard g(tok.device());
  const int rc = tdg_embed_bwd_det(tok.data_ptr(), t64, dout.data_ptr(), dtable.data_ptr<float>(),
                                   reinterpret_cast<long long*>(acc.data_ptr<int64_t>()), (int)M,
                                   (int)D, (long long)V, (float)scale, (float)p, (uint64_t)seed,
                                   ctr_ptr(ctr), (uint64_t)site, accumulate ? 1.f : 0.f,
                                   stream_of(tok));
  check_err(rc, "tdg embed_bwd_det");
}

// (int32 words, int64 words) of the CSR embedding backward's workspace
std::vector<int64_t> embed_csr_ws(int64_t M, int64_t V, int64_t D) {
  long long n32 = 0, n64 = 0;
  tdg_embed_csr_ws((int)M, (int)V, (int)D, &n32, &n64);
  return {n32, n64};
}

bool embed_csr_ok(int64_t M, int64_t V) { return tdg_embed_csr_ok((int)M, (int)V) != 0; }

void check_csr_ws(const Tensor& ws32, int64_t M, int64_t V, int64_t D, const char* n) {
  const int64_t n32 = embed_csr_ws(M, V, D)[0];
  TORCH_CHECK(ws32.scalar_type() == at::kInt && ws32.is_cuda() && ws32.is_contiguous() &&
                  ws32.numel() >= n32,
              n, ": int32 workspace of ", n32, " words");
  check_aligned(ws32, 16, n);
}

// Token sort of the CSR embedding backward for one or two tables (one
// launch): toks[i] (int32/int64, any shape) over vocabularies V[i] into the
// int32 workspaces ws32[i] (embed_csr_ws words).
void embed_csr_sort(const std::vector<Tensor>& toks, const std::vector<int64_t>& V,
                    const std::vector<Tensor>& ws32, const optional<Tensor>& stamps) {
  const int n = (int)toks.size();
  TORCH_CHECK(n >= 1 && n <= 2 && (int)V.size() == n && (int)ws32.size() == n, "embed_csr_sort: 1-2 tables");
  const void* tp[2];
  int t64[2], M[2], VV[2];
  int* wp[2];
  for (int i = 0; i < n; ++i) {
    const Tensor& t = toks[i];
    t64[i] = check_tok(t);
    TORCH_CHECK(tdg_embed_csr_ok((int)t.numel(), (int)V[i]), "embed_csr_sort: shape past the sort");
    check_csr_ws(ws32[i], t.numel(), V[i], 128, "embed_csr_sort");
    tp[i] = t.data_ptr();
    M[i] = (int)t.numel();
    VV[i] = (int)V[i];
    wp[i] = ws32[i].data_ptr<int>();
  }
  c10::DeviceGuard g(toks[0].device());
  long long* sp = nullptr;
  if (stamps.has_value()) {  // lab: int64 [2 * 8 * 64]
    TORCH_CHECK(stamps->scalar_type() == at::kLong && stamps->is_cuda() && stamps->numel() >= 1024,
                "stamps");
    sp = reinterpret_cast<long long*>(stamps->data_ptr<int64_t>());
  }
  check_err(tdg_embed_csr_sort(n, tp, t64, M, VV, wp, sp, stream_of(toks[0])), "tdg embed_csr_sort");
}

// The embedding gradient from a sorted workspace (deterministic; bitwise the
// fixed-point atomic path's): dtable = beta * dtable + scatter of drop(dout) *
// scale; kbits: the forward's keep bits.
void embed_csr_apply(const Tensor& dout, const Tensor& dtable, const Tensor& ws32,
                     const Tensor& ws64, int64_t M, double scale, double p, int64_t seed,
                     const optional<Tensor>& ctr, int64_t site, bool accumulate,
                     const optional<Tensor>& kbits) {
  check_grads(dout, dtable, M);
  check_aligned(dtable, 16, "dtable");
  const int64_t D = dtable.size(1), V = dtable.size(0);
  TORCH_CHECK(tdg_embed_csr_ok((int)M, (int)V), "embed_csr_apply: shape past the sort");
  check_kbits(kbits, M, D);
  check_csr_ws(ws32, M, V, D, "embed_csr_apply");
  const int64_t n64 = embed_csr_ws(M, V, D)[1];
  TORCH_CHECK(ws64.scalar_type() == at::kLong && ws64.is_cuda() && ws64.is_contiguous() &&
                  ws64.numel() >= n64,
              "embed_csr_apply: int64 workspace of ", n64, " words");
  c10::DeviceGuard g(dout.device());
  check_err(tdg_embed_csr_apply(dout.data_ptr(), opt_ptr(kbits), dtable.data_ptr<float>(),
                                ws32.data_ptr<int>(),
                                reinterpret_cast<long long*>(ws64.data_ptr<int64_t>()), (int)M,
                                (int)D, (int)V, (float)scale, (float)p, (uint64_t)seed,
                                ctr_ptr(ctr), (uint64_t)site, accumulate ? 1.f : 0.f,
                                stream_of(dout)),
            "tdg embed_csr_apply");
}

}  // namespace

void def_embedding(py::module_& m) {
  m.def("embed_fwd", &embed_fwd);
  m.def("embed_bwd", &embed_bwd);
  m.def("embed_bwd_det", &embed_bwd_det);
  m.def("embed_csr_ws", &embed_csr_ws);
  m.def("embed_csr_ok", &embed_csr_ok);
  m.def("embed_csr_sort", &embed_csr_sort);
  m.def("embed_csr_apply", &embed_csr_apply);
}
