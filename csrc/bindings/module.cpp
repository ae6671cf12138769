// Python module `_C`: one registration call per kernel family.
#include "common.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 (MI355X) HIP kernels for tensorflow_distributed_on_gke_amd";
  def_gemm(m);
  def_attention(m);
  def_decode(m);
  def_overlap(m);
  def_layernorm(m);
  def_embedding(m);
  def_batch(m);
  def_fp8(m);
  def_loss(m);
  def_distill(m);
  def_optimizer(m);
  def_ema(m);
  def_signal(m);
  m.attr("ARCH") = "gfx950";
}
