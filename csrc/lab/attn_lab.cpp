// Attention lab: standalone timing + per-workgroup phase stamps of the fused
// attention forward / backward on the Transformer-base shapes (B 64, H 8,
// head dim 64, L 128; self, causal self, cross).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DTDG_STAMPS -Icsrc/include \
//         -x hip csrc/lab/attn_lab.cpp -o lab_bin/attn_lab
#include "../kernels/attn_fwd.h"
#include "../kernels/attn_bwd.h"
#include "lab_common.h"

int main() {
  const int B = 64, H = 8, D = 64, L = 128;
  hipStream_t st;
  CK(hipStreamCreate(&st));
  lab::Stamps stamps;
  stamps.init(HIP_SYMBOL(tdg::tdg_stamps), (size_t)B * H * 4);
  std::mt19937 rng(3);
  const size_t n = (size_t)B * L * H * D;
  std::vector<uint16_t> hq, hk, hv;
  uint16_t* q = lab::rand_bf16(n, rng, 1.f, &hq);
  uint16_t* k = lab::rand_bf16(n, rng, 1.f, &hk);
  uint16_t* v = lab::rand_bf16(n, rng, 1.f, &hv);
  uint16_t* dout = lab::rand_bf16(n, rng, 0.1f);
  uint16_t *o, *dq, *dk, *dv;
  float *lse, *delta;
  CK(hipMalloc(&o, n * 2));
  CK(hipMalloc(&dq, n * 2));
  CK(hipMalloc(&dk, n * 2));
  CK(hipMalloc(&dv, n * 2));
  CK(hipMalloc(&lse, (size_t)B * H * L * 4));
  CK(hipMalloc(&delta, (size_t)B * H * L * 4));
  for (int causal = 0; causal < 2; ++causal) {
    AttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.out = o; a.lse = lse; a.delta = delta;
    a.dq = dq; a.dk = dk; a.dv = dv; a.kv_len = nullptr;
    const long long sb = (long long)L * H * D, sl = H * D;
    a.q_sb = a.k_sb = a.v_sb = a.o_sb = a.dq_sb = a.dk_sb = a.dv_sb = a.do_sb = sb;
    a.q_sl = a.k_sl = a.v_sl = a.o_sl = a.dq_sl = a.dk_sl = a.dv_sl = a.do_sl = sl;
    a.q_sh = a.k_sh = a.v_sh = a.o_sh = a.dq_sh = a.dk_sh = a.dv_sh = a.do_sh = D;
    a.B = B; a.H = H; a.Lq = L; a.Lk = L; a.scale = 0.125f; a.causal = causal;
    // forward: check one (b, h) against the host
    CK((hipError_t)tdg_attn_fwd(&a, D, st));
    CK(hipStreamSynchronize(st));
    std::vector<uint16_t> ho(n);
    CK(hipMemcpy(ho.data(), o, n * 2, hipMemcpyDeviceToHost));
    double err = 0, ref2 = 0;
    const int bb = 5, hh = 3;
    for (int i = 0; i < L; ++i) {
      std::vector<double> s(L);
      double mx = -1e300;
      for (int j = 0; j < L; ++j) {
        double acc = 0;
        for (int d = 0; d < D; ++d)
          acc += lab::host_f(hq[((size_t)bb * L + i) * H * D + hh * D + d]) *
                 lab::host_f(hk[((size_t)bb * L + j) * H * D + hh * D + d]);
        s[j] = (causal && j > i) ? -1e300 : acc * 0.125;
        mx = std::max(mx, s[j]);
      }
      double den = 0;
      for (int j = 0; j < L; ++j) den += (s[j] > -1e299) ? std::exp(s[j] - mx) : 0.0;
      for (int d = 0; d < D; ++d) {
        double r = 0;
        for (int j = 0; j < L; ++j)
          if (s[j] > -1e299)
            r += std::exp(s[j] - mx) / den * lab::host_f(hv[((size_t)bb * L + j) * H * D + hh * D + d]);
        const double g = lab::host_f(ho[((size_t)bb * L + i) * H * D + hh * D + d]);
        err += (g - r) * (g - r);
        ref2 += r * r;
      }
    }
    const char* fn[4] = {"load", "compute", "epi-issue", "drain"};
    stamps.clear(st);
    CK((hipError_t)tdg_attn_fwd(&a, D, st));
    CK(hipStreamSynchronize(st));
    const std::string sf = stamps.summary((size_t)B * H * 2, fn);
    const float tf = lab::graph_us(st, [&] { tdg_attn_fwd(&a, D, st); });
    std::printf("fwd causal=%d %8.2f us rel %.1e | %s\n", causal, tf, std::sqrt(err / ref2), sf.c_str());
    const char* bn[4] = {"load", "phase1", "phase2+stores", "drain"};
    stamps.clear(st);
    CK((hipError_t)tdg_attn_bwd(&a, D, st));
    CK(hipStreamSynchronize(st));
    const std::string sbw = stamps.summary((size_t)B * H, bn);
    const float tb = lab::graph_us(st, [&] { tdg_attn_bwd(&a, D, st); });
    std::printf("bwd causal=%d %8.2f us | %s\n", causal, tb, sbw.c_str());
    std::fflush(stdout);
    // backward with the output-projection dgrad in-kernel (FDO), as the
    // training step runs it: operands and outputs rotate over NSET buffer
    // sets (64 MiB each, together past the 256 MiB last-level cache), so
    // every launch reads from HBM
    constexpr int NSET = 6;
    static uint16_t* set[NSET][8];  // q k v o dy dq dk dv
    static uint16_t* wo = nullptr;
    const int d = H * D;
    if (!wo) {
      wo = lab::rand_bf16((size_t)d * d, rng, 0.05f);
      uint16_t* dy0 = lab::rand_bf16(n, rng, 0.1f);
      const uint16_t* src[5] = {q, k, v, o, dy0};
      for (int s = 0; s < NSET; ++s)
        for (int i = 0; i < 8; ++i) {
          CK(hipMalloc(&set[s][i], n * 2));
          if (i < 5) CK(hipMemcpy(set[s][i], src[i], n * 2, hipMemcpyDeviceToDevice));
        }
    }
    int turn = 0;
    auto fdo = [&] {
      uint16_t** p = set[turn++ % NSET];
      AttnArgs f = a;
      f.q = p[0]; f.k = p[1]; f.v = p[2]; f.o = p[3]; f.dout = nullptr;
      f.fdo_dy = p[4]; f.fdo_w = wo; f.fdo_d = d; f.fdo_ldy = d; f.fdo_ldw = d;
      f.dq = p[5]; f.dk = p[6]; f.dv = p[7];
      f.xcd = 1;
      CK((hipError_t)tdg_attn_bwd_fdo(&f, st));
    };
    for (int i = 0; i < NSET; ++i) fdo();
    CK(hipStreamSynchronize(st));
    stamps.clear(st);
    fdo();
    CK(hipStreamSynchronize(st));
    const char* on[6] = {"dO-gemm", "dO+delta+tiles", "phase1", "dS+dKdV-out", "phase2+dQ-out", "drain"};
    const int oo[7] = {0, 5, 1, 2, 6, 3, 4};
    const std::string sfo = stamps.summary((size_t)B * H, on, oo, 7);
    const float tfo = lab::graph_us(st, fdo);
    std::printf("bwd-fdo causal=%d %8.2f us (HBM-cold rotation) | %s\n", causal, tfo, sfo.c_str());
    std::fflush(stdout);
  }
  return 0;
}
