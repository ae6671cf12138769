"""The surface and the layering of `ops.kernels`, the package of launch
wrappers: what it re-exports, what it must not, and what `ops` may import."""
import ast
import importlib
import os
import types

import pytest

import tensorflow_distributed_on_gke_amd as pkg
from tensorflow_distributed_on_gke_amd.ops import kernels as K

PKG = pkg.__name__
OPS_DIR = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "ops")
FAMILIES = ["workspace", "gemm", "attention", "decode", "layernorm", "embedding", "batch", "loss",
            "optimizer", "signal"]

# sorted(n for n in vars(K) if not n.startswith("_")) of the single-file ops/kernels.py this package
# replaced, without what it had imported (math, os, torch, Dict, List, Optional, Tuple, annotations)
# and without the switches below
PUBLIC = [
    "COUNT_MAX_ENTRIES", "DISTILL_MAX", "ENSEMBLE_MAX", "EPI_BIAS", "EPI_BIAS_RELU", "EPI_DRELU",
    "EPI_NONE", "EmbCsr", "NORM_CLIPPED", "NORM_FACTOR", "NORM_MAX", "NORM_NORM", "NORM_SKIP",
    "NORM_SKIPPED", "NORM_SUMSQ", "NUM_CU", "RAGGED_MAX_PROBLEMS", "RAGGED_MAX_SHAPES", "StreamSignal",
    "adam", "adam_chunks", "adam_step_inc", "attn_bwd", "attn_bwd_f8", "attn_bwd_f8_ok", "attn_bwd_fdo",
    "attn_bwd_g8", "attn_bwd_g8_ok", "attn_fwd", "attn_fwd_fp8", "attn_fwd_fp8_ok", "attn_probs",
    "beam_topk", "check_gather_rows", "check_trailing_padding", "choose_gemm", "colsum",
    "colsum_grouped", "count_labels_multi", "count_tokens", "decode_attn", "distill_target",
    "distill_weights", "ema_update", "embed_bwd", "embed_csr_apply", "embed_csr_ok", "embed_csr_sort",
    "embed_fwd", "ensemble_logprobs", "gather_bad_counter", "gather_bad_rows", "gather_rows", "gemm",
    "grad_norm_finalize", "grad_sumsq", "interior_pad_rows", "label_total", "linear_dgrad",
    "linear_dgrad_t", "linear_fwd", "linear_wgrad", "ln_bwd", "ln_bwd_nparts", "ln_bwd_rpb", "ln_fwd",
    "load_tuned", "pack_relu_bits", "prep_batch", "qkv_attn_fwd", "reduce_partials_multi",
    "reset_workspace", "sample_token", "sample_uniforms", "save_tuned", "set_gemm_config",
    "transpose_grouped", "tuned_table", "wgrad_grouped", "wgrad_ragged", "workspace", "xent",
    "xent_distill", "xent_stats",
]
# switches and mutable tables: set on the module that reads them, never reachable through the package
# (a name rebound on the package would not be seen by that module)
OWNED = ["AUTOTUNE", "QKV_ATTN", "ATTN_BWD_FDO", "LN_BWD_RPB", "DETERMINISTIC_EMBED", "EMBED_CSR",
         "TUNED_FILE", "_TUNED", "_CFG_OVERRIDE", "_GROUP_TUNED", "_WS", "_WS_RETIRED", "C"]
# family module -> sibling family modules it may import besides workspace (calls that cross families)
CROSS = {"decode": {"attention"}}  # decode_attn's CPU arm runs attention._ref_attn_fwd


def _family(name):
    """The module ops.kernels.<name> (the package attributes `gemm` and
    `workspace` are the functions of those names)."""
    return importlib.import_module(f"{K.__name__}.{name}")


def test_public_names():
    got = sorted(n for n, v in vars(K).items()
                 if not n.startswith("_") and not isinstance(v, types.ModuleType))
    assert got == sorted(PUBLIC)


def test_switches_and_tables_not_reexported():
    for n in OWNED:
        assert not hasattr(K, n), n
    # each has an owner
    from tensorflow_distributed_on_gke_amd.ops import tuning
    owners = {"AUTOTUNE": tuning, "QKV_ATTN": _family("attention"), "ATTN_BWD_FDO": _family("attention"),
              "LN_BWD_RPB": _family("layernorm"), "DETERMINISTIC_EMBED": _family("embedding"),
              "EMBED_CSR": _family("embedding"), "TUNED_FILE": _family("gemm"), "_TUNED": _family("gemm"),
              "_CFG_OVERRIDE": _family("gemm"), "_GROUP_TUNED": _family("gemm"),
              "_WS": _family("workspace"), "_WS_RETIRED": _family("workspace")}
    for n, m in owners.items():
        assert hasattr(m, n), f"{m.__name__}.{n}"
    assert sorted(owners) == sorted(n for n in OWNED if n != "C")


def test_reexports_are_the_family_objects():
    mods = {f: _family(f) for f in FAMILIES}
    for n in PUBLIC:
        homes = [f for f, m in mods.items() if n in vars(m)]
        assert homes, f"{n}: in no family module"
        for f in homes:
            assert getattr(K, n) is vars(mods[f])[n], f"{n}: ops.kernels.{n} is not ops.kernels.{f}.{n}"


def _imports(path, modname, is_pkg):
    """Absolute names of everything `path` imports, at any depth."""
    with open(path) as f:
        tree = ast.parse(f.read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            out += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            if node.level:
                base = modname.split(".")
                base = base[:len(base) - node.level + (1 if is_pkg else 0)]
                mod = ".".join(base + ([node.module] if node.module else []))
            else:
                mod = node.module
            out += [mod] + [f"{mod}.{a.name}" for a in node.names]
    return out


def _ops_files():
    for dp, _, files in os.walk(OPS_DIR):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(dp, f)
                rel = os.path.relpath(path, os.path.dirname(OPS_DIR))[:-3].split(os.sep)
                is_pkg = rel[-1] == "__init__"
                yield path, ".".join([PKG] + (rel[:-1] if is_pkg else rel)), is_pkg


def test_ops_imports_no_layer_above():
    above = tuple(f"{PKG}.{layer}" for layer in ("models", "train", "infer", "parallel", "data"))
    seen = 0
    for path, modname, is_pkg in _ops_files():
        seen += 1
        for name in _imports(path, modname, is_pkg):
            assert not any(name == a or name.startswith(a + ".") for a in above), f"{path} imports {name}"
    assert seen >= 5 + len(FAMILIES)  # the walk found ops/ and ops/kernels/


def test_family_modules_import_no_sibling():
    prefix = f"{K.__name__}."
    for fam in FAMILIES:
        path = os.path.join(OPS_DIR, "kernels", fam + ".py")
        allowed = {"workspace"} | CROSS.get(fam, set())
        for name in _imports(path, prefix + fam, False):
            assert name != K.__name__, f"{fam} imports the package"
            if name.startswith(prefix):
                assert name[len(prefix):].split(".")[0] in allowed, f"{fam} imports {name}"


@pytest.mark.parametrize("fam", sorted(CROSS))
def test_cross_family_allow_list_is_used(fam):
    path = os.path.join(OPS_DIR, "kernels", fam + ".py")
    names = _imports(path, f"{K.__name__}.{fam}", False)
    for sib in CROSS[fam]:
        assert f"{K.__name__}.{sib}" in names
