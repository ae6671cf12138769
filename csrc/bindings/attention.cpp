// Attention bindings: bf16 and fp8 forward / backward, the fused projection
// forms and the probability dump. q/k/v/o/do/dq/dk/dv are 4-D [B, L, H, hd]
// views (any strides, hd contiguous).
#include "common.h"

namespace {

// XCD-grouped workgroup order of the attention kernels (tdg_attn.h xcd):
// TDG_ATTN_XCD=0 restores the plain grid order
int attn_xcd() {
  static const int v = [] {
    const char* e = getenv("TDG_ATTN_XCD");
    return (e && e[0] == '0') ? 0 : 1;
  }();
  return v;
}

// Every row of a 4-D view starts on a `bytes` boundary: the pointer and the
// three outer strides.
void check_rows_aligned(const Tensor& t, int bytes, const char* n) {
  check_aligned(t, bytes, n);
  const int64_t e = bytes / t.element_size();
  TORCH_CHECK(t.stride(0) % e == 0 && t.stride(1) % e == 0 && t.stride(2) % e == 0, n,
              ": rows must be ", bytes, "-byte aligned");
}
// One (pointer, batch / row / head stride) quadruple of AttnArgs from a view.
template <typename P>
void set_view(P*& ptr, long long& sb, long long& sl, int& sh, const Tensor& t) {
  ptr = (P*)t.data_ptr();
  sb = t.stride(0);
  sl = t.stride(1);
  sh = (int)t.stride(2);
}

using DtypeCheck = void (*)(const Tensor&, const char*);
void check_e4m3_or_raw(const Tensor& t, const char* n) { check_f8_fmt(t, 0, n); }

// Shapes and the q / k / v quadruples of `a`. check: the operands' element
// type; q_align / kv_align: byte alignment of their rows (16 for the bf16
// kernels' 16-byte row chunks and the LDS-DMA staging of fp8 K / V).
void fill_qkv(tdg::AttnArgs& a, const Tensor& q, const Tensor& k, const Tensor& v,
              DtypeCheck check = check_bf16, int q_align = 16, int kv_align = 16) {
  for (auto* t : {&q, &k, &v}) {
    check(*t, "q/k/v");
    TORCH_CHECK(t->dim() == 4 && t->stride(3) == 1, "q/k/v must be [B,L,H,hd] with hd contiguous");
  }
  a.B = (int)q.size(0);
  a.Lq = (int)q.size(1);
  a.H = (int)q.size(2);
  a.Lk = (int)k.size(1);
  TORCH_CHECK(k.size(0) == a.B && v.size(0) == a.B && k.size(2) == a.H && v.size(2) == a.H &&
                  v.size(1) == a.Lk && k.size(3) == q.size(3) && v.size(3) == q.size(3),
              "attention: q/k/v shape mismatch");
  set_view(a.q, a.q_sb, a.q_sl, a.q_sh, q);
  set_view(a.k, a.k_sb, a.k_sl, a.k_sh, k);
  set_view(a.v, a.v_sb, a.v_sl, a.v_sh, v);
  check_rows_aligned(q, q_align, "attention q");
  check_rows_aligned(k, kv_align, "attention k");
  check_rows_aligned(v, kv_align, "attention v");
}
// A bf16 [B, L, H, hd] operand shaped like q (L = Lq) or k (L = Lk); 16-byte
// rows: the kernels store whole 16-byte row chunks (attn_impl.h store_row16)
void check_like(const Tensor& t, const tdg::AttnArgs& a, int L, const char* n) {
  check_bf16(t, n);
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1 && t.size(0) == a.B && t.size(1) == L &&
                  t.size(2) == a.H,
              n, ": bad shape/stride");
  check_rows_aligned(t, 16, n);
}
// lse / delta: f32 [B, H, Lq]
void check_rowstat(const Tensor& t, const tdg::AttnArgs& a, const char* n) {
  check_f32(t, n);
  TORCH_CHECK(t.numel() == (int64_t)a.B * a.H * a.Lq, n, " must be [B,H,Lq]");
}
// The forward's outputs and mask / scale arguments (B, H, Lq set before).
void fill_fwd(tdg::AttnArgs& a, const Tensor& out, const Tensor& lse,
              const optional<Tensor>& kv_len, double scale, bool causal) {
  check_like(out, a, a.Lq, "out");
  check_rowstat(lse, a, "lse");
  check_contig(lse, "lse");
  set_view(a.out, a.o_sb, a.o_sl, a.o_sh, out);
  a.lse = lse.data_ptr<float>();
  a.kv_len = kv_len_ptr(kv_len, a.B);
  a.scale = (float)scale;
  a.causal = causal;
}

void attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out,
              const Tensor& lse, const optional<Tensor>& kv_len, double scale, bool causal) {
  tdg::AttnArgs a{};
  a.xcd = attn_xcd();
  fill_qkv(a, q, k, v);
  fill_fwd(a, out, lse, kv_len, scale, causal);
  c10::DeviceGuard g(q.device());
  check_err(tdg_attn_fwd(&a, (int)q.size(3), stream_of(q)), "tdg attn_fwd");
}

// Fused self-attention input projection + attention forward (L <= 128, hd
// 64): qkv[M, 3d] = x2 @ w^T + bias (written for the backward) and out / lse
// of the attention over it, in one launch. Returns false (nothing launched)
// when the shape is not covered.
bool qkv_attn_fwd(const Tensor& x2, const Tensor& w, const Tensor& bias, const Tensor& qkv,
                  const Tensor& out, const Tensor& lse, const optional<Tensor>& kv_len,
                  double scale, bool causal, int64_t B, int64_t heads,
                  const optional<Tensor>& k, const optional<Tensor>& v) {
  // k / v given: the cross-attention form (w / bias / qkv = the Q
  // projection's; k / v the [B, Lk, H, 64] views of the batched K|V)
  const bool cross = k.has_value();
  TORCH_CHECK(cross == v.has_value(), "qkv_attn_fwd: k and v together");
  const int np = cross ? 1 : 3;
  check_bf16(x2, "x2");
  check_bf16(w, "w");
  check_bf16(qkv, "qkv");
  check_contig(qkv, "qkv");
  check_f32(bias, "bias");
  TORCH_CHECK(x2.dim() == 2 && w.dim() == 2 && x2.stride(1) == 1 && w.stride(1) == 1, "x2 / w rows");
  const int64_t M = x2.size(0), d = x2.size(1);
  TORCH_CHECK(M % B == 0 && w.size(0) == np * d && w.size(1) == d && bias.numel() >= np * d &&
                  qkv.numel() == M * np * d,
              "qkv_attn_fwd: shapes");
  const int64_t L = M / B;
  if (L > 128 || d != 64 * heads || d % 64 || x2.stride(0) % 8 || w.stride(0) % 8) return false;
  check_aligned(x2, 16, "qkv_attn_fwd: x2");
  check_aligned(w, 16, "qkv_attn_fwd: w");
  check_aligned(qkv, 16, "qkv_attn_fwd: qkv");
  check_aligned(bias, 16, "qkv_attn_fwd: bias");
  tdg::QkvAttnArgs qa{};
  tdg::AttnArgs& a = qa.a;
  a.B = (int)B;
  a.H = (int)heads;
  a.Lk = (int)L;
  if (cross) {
    for (const Tensor* t : {&*k, &*v}) {
      check_bf16(*t, "k/v");
      TORCH_CHECK(t->dim() == 4 && t->stride(3) == 1 && t->size(0) == B && t->size(2) == heads &&
                      t->size(3) == 64 && t->size(1) == k->size(1),
                  "qkv_attn_fwd: k / v [B, Lk, H, 64], head dim contiguous");
      check_rows_aligned(*t, 16, "qkv_attn_fwd: k / v");
    }
    a.Lk = (int)k->size(1);
    set_view(a.k, a.k_sb, a.k_sl, a.k_sh, *k);
    set_view(a.v, a.v_sb, a.v_sl, a.v_sh, *v);
    if (a.Lk > 128) return false;
  }
  a.xcd = 0;
  a.Lq = (int)L;
  fill_fwd(a, out, lse, kv_len, scale, causal);
  qa.x = (const uint16_t*)x2.data_ptr();
  qa.w = (const uint16_t*)w.data_ptr();
  qa.bias = bias.data_ptr<float>();
  qa.qkv = (uint16_t*)qkv.data_ptr();
  qa.d = (int)d;
  qa.ldx = (int)x2.stride(0);
  qa.ldw = (int)w.stride(0);
  qa.L = (int)L;
  qa.cross = cross;
  c10::DeviceGuard g(x2.device());
  const int rc = tdg_qkv_attn_fwd(&qa, stream_of(x2));
  if (rc == -1) return false;
  check_err(rc, "tdg qkv_attn_fwd");
  return true;
}

// e4m3 forward: q8/k8/v8 are [B, L, H, 64] float8_e4m3fn views (hd
// contiguous; K / V rows 16-byte aligned for the LDS-DMA staging, Q rows
// 8-byte), with per-tensor scales (x8 = e4m3(x * s), one-element f32 device
// tensors)
void attn_fwd_fp8(const Tensor& q8, const Tensor& k8, const Tensor& v8, const Tensor& out,
                  const Tensor& lse, const optional<Tensor>& kv_len, const Tensor& sq,
                  const Tensor& sk, const Tensor& sv, double scale, bool causal,
                  const optional<Tensor>& out8, const optional<Tensor>& so8,
                  const optional<Tensor>& amax8) {
  tdg::AttnArgs a{};
  a.xcd = attn_xcd();
  fill_qkv(a, q8, k8, v8,
           [](const Tensor& t, const char*) {
             TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat8_e4m3fn,
                         "attn_fwd_fp8: e4m3 q/k/v");
           },
           8, 16);
  TORCH_CHECK(q8.size(3) == 64, "attn_fwd_fp8: [B,L,H,64] with hd contiguous");
  fill_fwd(a, out, lse, kv_len, scale, causal);
  for (auto* t : {&sq, &sk, &sv}) check_f32(*t, "fp8 scale");
  if (out8.has_value()) {
    check_f8_fmt(*out8, 0, "out8");
    TORCH_CHECK(out8->sizes() == out.sizes() && out8->strides() == out.strides() && so8.has_value() &&
                    amax8.has_value(),
                "attn_fwd_fp8: out8 has out's shape / strides, with so8 and amax8");
    check_f32(*so8, "so8");
    a.out8 = (uint8_t*)out8->data_ptr();
    a.so8 = so8->data_ptr<float>();
    a.amax8 = amax_ptr(amax8);
  }
  a.sq8 = sq.data_ptr<float>();
  a.sk8 = sk.data_ptr<float>();
  a.sv8 = sv.data_ptr<float>();
  c10::DeviceGuard g(q8.device());
  check_err(tdg_attn_fwd_fp8(&a, 64, stream_of(q8)), "tdg attn_fwd_fp8");
}

tdg::AttnArgs attn_bwd_args(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                            const Tensor& dout, const Tensor& lse, const Tensor& delta,
                            const Tensor& dq, const Tensor& dk, const Tensor& dv,
                            const optional<Tensor>& kv_len, double scale, bool causal) {
  tdg::AttnArgs a{};
  a.xcd = attn_xcd();
  fill_qkv(a, q, k, v);
  check_like(o, a, a.Lq, "o");
  check_like(dout, a, a.Lq, "dout");
  check_like(dq, a, a.Lq, "dq");
  check_like(dk, a, a.Lk, "dk");
  check_like(dv, a, a.Lk, "dv");
  check_rowstat(lse, a, "lse");
  check_rowstat(delta, a, "delta");
  set_view(a.o, a.o_sb, a.o_sl, a.o_sh, o);
  set_view(a.dout, a.do_sb, a.do_sl, a.do_sh, dout);
  set_view(a.dq, a.dq_sb, a.dq_sl, a.dq_sh, dq);
  set_view(a.dk, a.dk_sb, a.dk_sl, a.dk_sh, dk);
  set_view(a.dv, a.dv_sb, a.dv_sl, a.dv_sh, dv);
  a.lse = lse.data_ptr<float>();
  a.delta = delta.data_ptr<float>();
  a.kv_len = kv_len_ptr(kv_len, a.B);
  a.scale = (float)scale;
  a.causal = causal;
  return a;
}

void attn_bwd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
              const Tensor& dout, const Tensor& lse, const Tensor& delta, const Tensor& dq,
              const Tensor& dk, const Tensor& dv, const optional<Tensor>& kv_len, double scale,
              bool causal) {
  tdg::AttnArgs a = attn_bwd_args(q, k, v, o, dout, lse, delta, dq, dk, dv, kv_len, scale, causal);
  c10::DeviceGuard g(q.device());
  check_err(tdg_attn_bwd(&a, (int)q.size(3), stream_of(q)), "tdg attn_bwd");
}

// attn_bwd with the output-projection dgrad in-kernel: dO = dy2 @ wo[:, head
// columns] per (batch, head) (dy2 [B * Lq, d], wo [d, d] bf16), never
// written to memory. Returns false (nothing launched) when not covered
// (Lq / Lk > 128, hd != 64).
bool attn_bwd_fdo(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                  const Tensor& dy2, const Tensor& wo, const Tensor& lse, const Tensor& delta,
                  const Tensor& dq, const Tensor& dk, const Tensor& dv,
                  const optional<Tensor>& kv_len, double scale, bool causal) {
  // (o stands in for dout in the checks: the kernel computes dO itself)
  tdg::AttnArgs a = attn_bwd_args(q, k, v, o, o, lse, delta, dq, dk, dv, kv_len, scale, causal);
  a.dout = nullptr;
  check_bf16(dy2, "dy2");
  check_bf16(wo, "wo");
  const int64_t d = wo.size(1);
  TORCH_CHECK(dy2.dim() == 2 && wo.dim() == 2 && dy2.stride(1) == 1 && wo.stride(1) == 1 &&
                  dy2.size(0) == (int64_t)a.B * a.Lq && dy2.size(1) == d && wo.size(0) == d,
              "attn_bwd_fdo: dy2 [B * Lq, d], wo [d, d]");
  check_aligned(dy2, 16, "attn_bwd_fdo: dy2");
  check_aligned(wo, 16, "attn_bwd_fdo: wo");
  if (q.size(3) != 64 || a.Lq > 128 || a.Lk > 128 || d != 64 * a.H) return false;
  a.fdo_dy = (const uint16_t*)dy2.data_ptr();
  a.fdo_w = (const uint16_t*)wo.data_ptr();
  a.fdo_d = (int)d;
  a.fdo_ldy = (int)dy2.stride(0);
  a.fdo_ldw = (int)wo.stride(0);
  c10::DeviceGuard g(q.device());
  const int rc = tdg_attn_bwd_fdo(&a, stream_of(q));
  if (rc == -1) return false;
  check_err(rc, "tdg attn_bwd_fdo");
  return true;
}

// attn_bwd that also emits e5m2 copies of dQ (and of dK / dV when given),
// their amax, and the bias-gradient column-sum partials (tdg_attn.h); the
// hd-64 pipelined kernels (Lq or Lk > 128) only.
void attn_bwd_g8(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                 const Tensor& dout, const Tensor& lse, const Tensor& delta, const Tensor& dq,
                 const Tensor& dk, const Tensor& dv, const optional<Tensor>& kv_len, double scale,
                 bool causal, const Tensor& dq8, const optional<Tensor>& dk8,
                 const optional<Tensor>& dv8, const Tensor& sg8, const optional<Tensor>& amax8,
                 const optional<Tensor>& cs_part, int64_t cs_np, int64_t cs_ld, int64_t cs_q,
                 int64_t cs_k, int64_t cs_v, bool skip_bf16) {
  tdg::AttnArgs a = attn_bwd_args(q, k, v, o, dout, lse, delta, dq, dk, dv, kv_len, scale, causal);
  TORCH_CHECK(q.size(3) == 64 && (a.Lq > 128 || a.Lk > 128),
              "attn_bwd_g8: the pipelined hd-64 kernels (Lq or Lk > 128) only");
  TORCH_CHECK(dk8.has_value() == dv8.has_value(), "attn_bwd_g8: dk8 and dv8 together");
  // skip_bf16 leaves the bf16 dK / dV unwritten: only legal when their e5m2
  // copies are the output (else the gradients would stay uninitialised)
  TORCH_CHECK(!skip_bf16 || dk8.has_value(), "attn_bwd_g8: skip_bf16 needs dk8/dv8");
  auto same = [](const Tensor& x8, const Tensor& x, const char* n) {
    check_f8_fmt(x8, 1, n);
    TORCH_CHECK(x8.sizes() == x.sizes() && x8.strides() == x.strides(), n,
                " must have the bf16 gradient's shape and strides");
  };
  same(dq8, dq, "dq8");
  a.dq8 = (uint8_t*)dq8.data_ptr();
  if (dk8.has_value()) {
    same(*dk8, dk, "dk8");
    same(*dv8, dv, "dv8");
    a.dk8 = (uint8_t*)dk8->data_ptr();
    a.dv8 = (uint8_t*)dv8->data_ptr();
  }
  check_f32(sg8, "sg8");
  a.sg8 = sg8.data_ptr<float>();
  a.amaxg8 = amax_ptr(amax8);
  TORCH_CHECK(a.amaxg8 != nullptr, "attn_bwd_g8: amax8 slot");
  if (cs_part.has_value()) {
    check_f32(*cs_part, "cs_part");
    const int64_t nqb = (a.Lq + 127) / 128, nkb = (a.Lk + 127) / 128;
    TORCH_CHECK(cs_np == nqb && (!dk8.has_value() || nkb == nqb),
                "attn_bwd_g8: cs_np must equal the query (and key) 128-row block count");
    TORCH_CHECK(cs_part->numel() >= (int64_t)a.B * cs_np * cs_ld &&
                    cs_q + a.H * 64 <= cs_ld && (!dk8.has_value() || (cs_k + a.H * 64 <= cs_ld &&
                                                                       cs_v + a.H * 64 <= cs_ld)),
                "attn_bwd_g8: column-sum partial extent");
    a.cs_part = cs_part->data_ptr<float>();
    a.cs_np = (int)cs_np;
    a.cs_ld = (int)cs_ld;
    a.cs_q = (int)cs_q;
    a.cs_k = (int)cs_k;
    a.cs_v = (int)cs_v;
  }
  a.skip_bf16 = skip_bf16 ? 1 : 0;
  c10::DeviceGuard g(q.device());
  check_err(tdg_attn_bwd(&a, 64, stream_of(q)), "tdg attn_bwd_g8");
}

// fp8 attention backward (attn_f8.h attn_bwd_f8_kernel): e4m3 q8/k8/v8
// (the forward's operands, scales sq/sk/sv), e5m2 do8 (scale sdo), bf16 o,
// the forward's lse; dS quantised with sds (amax into amaxds). Outputs, each
// written when given: bf16 dq/dk/dv, e5m2 dq8/dk8/dv8 (scale sg8, amax into
// amaxg8), and one row per batch of bias-gradient column sums of the e5m2
// outputs in cs_part[b * cs_ld + cs_{q,k,v} + h * 64 + col] (cs_np = 1).
void attn_bwd_f8(const Tensor& q8, const Tensor& k8, const Tensor& v8, const Tensor& sq,
                 const Tensor& sk, const Tensor& sv, const Tensor& o, const Tensor& do8,
                 const Tensor& sdo, const Tensor& lse, const optional<Tensor>& kv_len, double scale,
                 bool causal, const Tensor& sds, const Tensor& amaxds, const optional<Tensor>& dq,
                 const optional<Tensor>& dk, const optional<Tensor>& dv, const optional<Tensor>& dq8,
                 const optional<Tensor>& dk8, const optional<Tensor>& dv8,
                 const optional<Tensor>& sg8, const optional<Tensor>& amaxg8,
                 const optional<Tensor>& cs_part, int64_t cs_ld, int64_t cs_q, int64_t cs_k,
                 int64_t cs_v, const optional<Tensor>& sgkv8, const optional<Tensor>& amaxgkv8,
                 const optional<Tensor>& cs_part2, int64_t cs_ld2) {
  tdg::AttnArgs a{};
  a.xcd = attn_xcd();
  fill_qkv(a, q8, k8, v8, check_e4m3_or_raw, 16, 16);
  check_f8_fmt(do8, 1, "attn_bwd_f8 do8");
  TORCH_CHECK(q8.size(3) == 64 && do8.dim() == 4 && do8.stride(3) == 1 && do8.sizes() == q8.sizes(),
              "attn_bwd_f8: q/k/v/do [B,L,H,64] with hd contiguous");
  check_rows_aligned(do8, 16, "attn_bwd_f8 do8");
  TORCH_CHECK(a.Lq <= 512 && a.Lk <= 512, "attn_bwd_f8: Lq, Lk <= 512 (all keys in one workgroup)");
  set_view(a.dout, a.do_sb, a.do_sl, a.do_sh, do8);
  check_like(o, a, a.Lq, "o");
  set_view(a.o, a.o_sb, a.o_sl, a.o_sh, o);
  check_rowstat(lse, a, "lse");
  check_contig(lse, "lse");
  a.lse = lse.data_ptr<float>();
  for (auto* t : {&sq, &sk, &sv, &sdo, &sds}) check_f32(*t, "fp8 scale");
  a.sq8 = sq.data_ptr<float>();
  a.sk8 = sk.data_ptr<float>();
  a.sv8 = sv.data_ptr<float>();
  a.sdo8 = sdo.data_ptr<float>();
  a.sds8 = sds.data_ptr<float>();
  a.amaxds8 = amax_ptr(amaxds);
  a.kv_len = kv_len_ptr(kv_len, a.B);
  a.scale = (float)scale;
  a.causal = causal;
  // outputs: a bf16 / e5m2 pair shares its strides (one set per gradient)
  auto out = [&](const optional<Tensor>& x, const optional<Tensor>& x8, int L, const char* n,
                 uint16_t*& p, uint8_t*& p8, long long& sb, long long& sl, int& sh) {
    TORCH_CHECK(x.has_value() || x8.has_value(), "attn_bwd_f8: no output for ", n);
    if (x8.has_value()) {
      check_f8_fmt(*x8, 1, n);
      TORCH_CHECK(x8->dim() == 4 && x8->size(0) == a.B && x8->size(1) == L && x8->size(2) == a.H &&
                      x8->size(3) == 64 && x8->stride(3) == 1,
                  n, ": e5m2 copy [B,L,H,64]");
      check_rows_aligned(*x8, 4, n);
      TORCH_CHECK(!x.has_value() || x8->strides() == x->strides(), n, ": bf16 and e5m2 strides differ");
      set_view(p8, sb, sl, sh, *x8);
    }
    if (x.has_value()) {
      check_like(*x, a, L, n);
      set_view(p, sb, sl, sh, *x);
    }
  };
  out(dq, dq8, a.Lq, "dq", a.dq, a.dq8, a.dq_sb, a.dq_sl, a.dq_sh);
  out(dk, dk8, a.Lk, "dk", a.dk, a.dk8, a.dk_sb, a.dk_sl, a.dk_sh);
  out(dv, dv8, a.Lk, "dv", a.dv, a.dv8, a.dv_sb, a.dv_sl, a.dv_sh);
  TORCH_CHECK(dk8.has_value() == dv8.has_value(), "attn_bwd_f8: dk8 and dv8 together");
  TORCH_CHECK(!dk8.has_value() || dq8.has_value(), "attn_bwd_f8: dk8 / dv8 need dq8");
  if (dq8.has_value()) {
    TORCH_CHECK(sg8.has_value() && amaxg8.has_value(), "attn_bwd_f8: e5m2 outputs need sg8 and amaxg8");
    check_f32(*sg8, "sg8");
    a.sg8 = sg8->data_ptr<float>();
    a.amaxg8 = amax_ptr(amaxg8);
  }
  // dK / dV e5m2 in a slot of their own (scale + amax together)
  TORCH_CHECK(sgkv8.has_value() == amaxgkv8.has_value(), "attn_bwd_f8: sgkv8 with amaxgkv8");
  if (sgkv8.has_value()) {
    TORCH_CHECK(dk8.has_value(), "attn_bwd_f8: sgkv8 needs dk8 / dv8");
    check_f32(*sgkv8, "sgkv8");
    a.sgkv8 = sgkv8->data_ptr<float>();
    a.amaxgkv8 = amax_ptr(amaxgkv8);
  }
  const int64_t ld2 = cs_part2.has_value() ? cs_ld2 : cs_ld;
  if (cs_part2.has_value()) {
    TORCH_CHECK(cs_part.has_value() && dk8.has_value(), "attn_bwd_f8: cs_part2 needs cs_part and dk8");
    check_f32(*cs_part2, "cs_part2");
    TORCH_CHECK(cs_part2->numel() >= (int64_t)a.B * cs_ld2, "attn_bwd_f8: cs_part2 extent");
    a.cs_part2 = cs_part2->data_ptr<float>();
    a.cs_ld2 = (int)cs_ld2;
  }
  if (cs_part.has_value()) {
    TORCH_CHECK(dq8.has_value(), "attn_bwd_f8: column sums come with the e5m2 outputs");
    check_f32(*cs_part, "cs_part");
    TORCH_CHECK(cs_part->numel() >= (int64_t)a.B * cs_ld && cs_q >= 0 && cs_q + a.H * 64 <= cs_ld &&
                    (!dk8.has_value() || (cs_k >= 0 && cs_v >= 0 && cs_k + a.H * 64 <= ld2 &&
                                          cs_v + a.H * 64 <= ld2)),
                "attn_bwd_f8: column-sum partial extent");
    a.cs_part = cs_part->data_ptr<float>();
    a.cs_np = 1;
    a.cs_ld = (int)cs_ld;
    a.cs_q = (int)cs_q;
    a.cs_k = (int)cs_k;
    a.cs_v = (int)cs_v;
  }
  c10::DeviceGuard g(q8.device());
  check_err(tdg_attn_bwd_f8(&a, 64, stream_of(q8)), "tdg attn_bwd_f8");
}

void attn_probs(const Tensor& q, const Tensor& k, const Tensor& probs,
                const optional<Tensor>& kv_len, double scale, bool causal) {
  tdg::AttnArgs a{};
  a.xcd = attn_xcd();
  fill_qkv(a, q, k, k);
  check_f32(probs, "probs");
  check_contig(probs, "probs");
  TORCH_CHECK(probs.numel() == (int64_t)a.B * a.H * a.Lq * a.Lk, "probs must be [B,H,Lq,Lk]");
  a.kv_len = kv_len_ptr(kv_len, a.B);
  a.scale = (float)scale;
  a.causal = causal;
  c10::DeviceGuard g(q.device());
  check_err(tdg_attn_probs(&a, (int)q.size(3), probs.data_ptr<float>(), stream_of(q)),
            "tdg attn_probs");
}

std::vector<int64_t> attn_last_plan() {
  int p[5];
  tdg_attn_last_plan(p);
  return std::vector<int64_t>(p, p + 5);
}

}  // namespace

void def_attention(py::module_& m) {
  m.def("attn_fwd", &attn_fwd);
  m.def("qkv_attn_fwd", &qkv_attn_fwd);
  m.def("attn_fwd_fp8", &attn_fwd_fp8);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_bwd_fdo", &attn_bwd_fdo);
  m.def("attn_bwd_g8", &attn_bwd_g8);
  m.def("attn_bwd_f8", &attn_bwd_f8);
  m.def("attn_probs", &attn_probs);
  m.def("attn_last_plan", &attn_last_plan);
}
