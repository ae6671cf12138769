"""Thin, shape-checked launch wrappers over the gfx950 HIP kernels (`_C`),
one module per kernel family; this package re-exports their functions, classes
and constants, so callers write `from ...ops import kernels as K; K.gemm(...)`.

All GPU compute of the model goes through here. Outputs are allocated from
the PyTorch caching allocator (stream-ordered, graph-capture safe); scratch
buffers (split-K slabs, column-sum partials) come from a grow-only per-device
workspace so a captured HIP graph sees stable addresses.

Switches and mutable tables (LN_BWD_RPB, EMBED_CSR, QKV_ATTN, _TUNED, ...) are
not re-exported: a name rebound here would not be seen by the module that
reads it, so they are set on their owning module (the timed tile search's
AUTOTUNE on `ops.tuning`). `gemm` and `workspace` name the functions here; the
modules of those names are reached with `importlib.import_module`.

The re-exported surface is the one the single-file module had and
tests/test_kernels_surface_cpu.py pins; a wrapper added since is imported from
its family module (`from ...ops.kernels.decode import score_tokens`).
"""
from .workspace import NUM_CU, reset_workspace, workspace
from .gemm import (EPI_BIAS, EPI_BIAS_RELU, EPI_DRELU, EPI_NONE, RAGGED_MAX_PROBLEMS,
                   RAGGED_MAX_SHAPES, choose_gemm, colsum, colsum_grouped, gemm, linear_dgrad,
                   linear_dgrad_t, linear_fwd, linear_wgrad, load_tuned, pack_relu_bits, save_tuned,
                   set_gemm_config, transpose_grouped, tuned_table, wgrad_grouped, wgrad_ragged)
from .attention import (attn_bwd, attn_bwd_f8, attn_bwd_f8_ok, attn_bwd_fdo, attn_bwd_g8,
                        attn_bwd_g8_ok, attn_fwd, attn_fwd_fp8, attn_fwd_fp8_ok, attn_probs,
                        qkv_attn_fwd)
from .decode import (ENSEMBLE_MAX, beam_topk, decode_attn, ensemble_logprobs, sample_token,
                     sample_uniforms)
from .layernorm import ln_bwd, ln_bwd_nparts, ln_bwd_rpb, ln_fwd, reduce_partials_multi
from .embedding import EmbCsr, embed_bwd, embed_csr_apply, embed_csr_ok, embed_csr_sort, embed_fwd
from .batch import (COUNT_MAX_ENTRIES, check_gather_rows, check_trailing_padding, count_labels_multi,
                    count_tokens, gather_bad_counter, gather_bad_rows, gather_rows,
                    interior_pad_rows, label_total, prep_batch)
from .loss import DISTILL_MAX, distill_target, distill_weights, xent, xent_distill, xent_stats
from .optimizer import (NORM_CLIPPED, NORM_FACTOR, NORM_MAX, NORM_NORM, NORM_SKIP, NORM_SKIPPED,
                        NORM_SUMSQ, adam, adam_chunks, adam_step_inc, ema_update, grad_norm_finalize,
                        grad_sumsq)
from .signal import StreamSignal
