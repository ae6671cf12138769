"""Run configuration.

The YAML file keeps the reference's four keys
(reference: configuration/settings.yaml:1-4, read at distributed_training_transformer/__main__.py:20-25):
`local_batch_size`, `worker_count`, `cloud_storage_bucket_name`,
`cloud_storage_upload_folder`. Everything the reference hard-codes
(__main__.py:39-43, 56-73, 89, 139-169) becomes an optional key with the
reference value as default, and any key can be overridden on the command line
with `--set key=value`.

Divergence (fixes a reference bug): the data-parallel world
size comes from the runtime (WORLD_SIZE / the cluster), not from
`worker_count`; `worker_count` is only the expected size, checked at start-up.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import yaml


@dataclass
class Settings:
    # --- the reference's four keys
    local_batch_size: int = 64
    worker_count: int = 1
    cloud_storage_bucket_name: str = "kubernetes-transformer-training"
    cloud_storage_upload_folder: str = "training-snapshots"
    # --- model (reference __main__.py:39-43 -> preset "reference")
    preset: str = "reference"
    layers: Optional[int] = None
    d_model: Optional[int] = None
    heads: Optional[int] = None
    d_ff: Optional[int] = None
    dropout: float = 0.1
    label_smoothing: float = 0.0
    src_vocab: int = 7765
    tgt_vocab: int = 7010
    max_len: int = 1000
    # --- optimisation (reference __main__.py:56-73)
    warmup_steps: int = 4000
    beta1: float = 0.9
    beta2: float = 0.98
    epsilon: float = 1e-9
    learning_rate: Optional[float] = None  # None -> Noam schedule
    # extensions, off by default (the reference sets neither): Keras Adam's
    # global_clipnorm (tf.clip_by_global_norm over the whole all-reduced
    # gradient; 0: off) and skipping of steps whose gradient norm is inf / NaN
    # (weights, moments and `iterations` untouched)
    global_clipnorm: float = 0.0
    skip_nonfinite: bool = False
    # extension, off by default: an exponential moving average of the weights
    # (Keras Adam use_ema; train/ema.py), updated after every completed step.
    # ema_decay in [0, 1), 0: off; ema_warmup: the decay ramps up as
    # min(ema_decay, (1 + updates) / (10 + updates)); ema_eval: a second
    # validation pass per epoch on the averaged weights. With it on, weight
    # snapshots gain a `model_weights_ema` bundle (`test --ema` decodes from it)
    ema_decay: float = 0.0
    ema_warmup: bool = False
    ema_eval: bool = True
    # --- loop (reference __main__.py:89, 149-180)
    epochs: int = 20
    steps_per_epoch: int = 200
    validation_steps: int = 20
    log_every: int = 50
    snapshot_every_epochs: int = 5
    # --- data: "synthetic" token pairs, or "text": TSV source<TAB>target files
    # (data/text.py, the reference's TED pipeline on local files; an epoch is
    # one pass over train_file, steps_per_epoch / validation_steps ignored)
    data: str = "synthetic"
    train_file: Optional[str] = None
    validation_file: Optional[str] = None
    src_tokenizer: Optional[str] = None  # WordPiece JSON; None: trained on train_file
    tgt_tokenizer: Optional[str] = None
    shuffle_buffer: int = 20000
    src_len: int = 40
    tgt_len: int = 40
    min_len: int = 4
    copy_task: bool = True
    seed: int = 0
    # --- checkpoint / storage (reference checkpoint.py, __main__.py:30,139-147)
    storage_backend: str = "local"
    storage_root: str = "snapshots"
    google_cloud_access_key_path: str = "configuration/gcp-access-key.json"
    temporary_directory: str = "temporary"
    warm_start: Optional[str] = None  # reference always loads saved_weights/2/model_weights
    resume: bool = True  # extension: resume from the newest local snapshot
    # --- runtime
    dtype: str = "bf16"
    bucket_mb: float = 64.0
    grad_comm_dtype: str = "fp32"  # fp32 | bf16 (gradient all-reduce payload)
    hip_graph: bool = False
    # variable-length (text) batches under hip_graph: each batch's source and
    # target-input lengths are padded up to a multiple of graph_bucket (capped
    # at max_len; semantically neutral -- attention, loss and LayerNorm are
    # length-masked) and one captured step per (source, target) bucket is kept,
    # at most graph_cache of them (least recently used evicted)
    graph_bucket: int = 32
    graph_cache: int = 64
    idle_after_train: bool = False  # reference __main__.py:183-186 keeps the pod alive
    check_replicas_every: int = 0  # debug: assert bitwise-identical replicas every N steps
    metrics_file: Optional[str] = None  # JSONL metrics sink (rank 0)
    profile_dir: Optional[str] = None  # torch.profiler (roctracer) Chrome trace of the first steps
    profile_steps: int = 5  # active profiled steps (after 1 wait + 1 warm-up step)
    kill_at_step: int = -1  # fault injection (tests): global step at which to exit
    kill_rank: int = -1  # rank that exits (-1: the last rank)
    # "step": exit after the step; "backward": exit in the middle of that
    # step's backward, once half of the gradients are final (peers are then
    # blocked inside a gradient all-reduce; eager steps only -- a captured
    # step runs no Python callbacks)
    kill_point: str = "step"
    # "replica_mean": the reference's per-replica token mean / workers
    # (transformer_model.py:11-17); "global_mean": sum of all replicas' token
    # losses / all replicas' label count (equal to the single-process loss on
    # the global batch, whatever the per-replica token counts)
    loss_mode: str = "replica_mean"
    # extension, off at 1: gradient accumulation. One optimizer update consumes
    # accum_steps consecutive local batches per rank (micro-batches), each
    # treated as one more replica: the update is that of world * accum_steps
    # replicas with one batch each (train/step.py TrainStep.update). An integer
    # in [1, 32]; not with dtype=fp8
    accum_steps: int = 1
    # extension, off at 0: token-budget batches of data=text (data/text.py
    # plan_token_batches). batch_tokens = N > 0 is the per-rank budget of
    # processed positions per batch, rows_per_rank * (S + T - 1) with S the
    # padded source and T - 1 the padded decoder-input length: the pairs are
    # sorted by length and cut into batches of varying row count, each padded
    # to a multiple of length_bucket (>= 1; graph_bucket and local_batch_size
    # are not used in this mode). Label counts then differ a lot between
    # batches, so loss_mode=global_mean is the sensible companion.
    # corpus_on_device (with batch_tokens > 0 on a GPU): the tokenised corpus
    # lives on the device and a batch is one gather launch
    # (data/corpus.py); false assembles the same batches on the host
    batch_tokens: int = 0
    length_bucket: int = 8
    corpus_on_device: bool = True
    # extension, off without distill_teacher: word-level knowledge distillation
    # (train/distill.py). distill_teacher: comma-separated weight prefixes (or
    # snapshot directories, as warm_start) of 1 to 8 frozen teachers with the
    # student's vocabularies; distill_weights: one positive number per teacher
    # (default uniform); distill_alpha in (0, 1]: the teachers' share of the
    # target, 0.5 when a teacher is given and it is left unset;
    # distill_preset: the teachers' model preset (default: the student's
    # configuration). Not with dtype=fp8. Validation stays the label cross
    # entropy without a teacher
    distill_teacher: Optional[str] = None
    distill_weights: Optional[str] = None
    distill_alpha: Optional[float] = None
    distill_preset: Optional[str] = None

    def global_batch(self, world: int) -> int:
        return self.local_batch_size * world


def _coerce(cur: Any, value: str, ftype) -> Any:
    if value in ("None", "null") and "Optional" in str(ftype):
        return None
    if isinstance(cur, bool) or ftype in (bool, "bool", Optional[bool]):
        return str(value).lower() in ("1", "true", "yes", "on")
    for t in (int, float):
        if isinstance(cur, t) and not isinstance(cur, bool):
            return t(value)
    if value in ("None", "null", ""):
        return None
    try:
        return int(value)
    except ValueError:
        try:
            return float(value)
        except ValueError:
            return value


def load_settings(path: Optional[str] = None, overrides: Optional[List[str]] = None) -> Settings:
    s = Settings()
    names = {f.name: f for f in dataclasses.fields(Settings)}
    if path:
        with open(path) as f:
            data: Dict[str, Any] = yaml.safe_load(f) or {}
        unknown = set(data) - set(names)
        if unknown:
            raise KeyError(f"unknown settings keys: {sorted(unknown)}")
        for k, v in data.items():
            setattr(s, k, v)
    for ov in overrides or []:
        if "=" not in ov:
            raise ValueError(f"--set expects key=value, got {ov!r}")
        k, v = ov.split("=", 1)
        if k not in names:
            raise KeyError(f"unknown setting {k!r}")
        setattr(s, k, _coerce(getattr(s, k), v, names[k].type))
    if not (isinstance(s.ema_decay, (int, float)) and 0.0 <= float(s.ema_decay) < 1.0):
        raise ValueError(f"ema_decay must lie in [0, 1) (0: off), got {s.ema_decay!r}")
    check_accum_steps(s.accum_steps, s.dtype)
    check_batch_tokens(s.batch_tokens, s.data, s.length_bucket)
    check_distill(s.distill_teacher, s.distill_weights, s.distill_alpha, s.dtype)
    return s


ACCUM_STEPS_MAX = 32


def check_accum_steps(n: Any, dtype: str = "bf16") -> int:
    """accum_steps is an integer in [1, 32], and 1 with dtype=fp8 (delayed
    scaling across micro-batches is not designed yet); ValueError otherwise."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= ACCUM_STEPS_MAX:
        raise ValueError(f"accum_steps must be an integer in [1, {ACCUM_STEPS_MAX}], got {n!r}")
    if n > 1 and dtype == "fp8":
        raise ValueError(f"accum_steps={n} with dtype=fp8 is not supported: the fp8 delayed scaling "
                         "assumes one forward/backward per optimizer update (use dtype=bf16)")
    return n


def check_batch_tokens(n: Any, data: str = "text", length_bucket: Any = 8) -> int:
    """batch_tokens is an integer >= 0 (0: fixed local_batch_size batches) and
    non-zero only with data=text; length_bucket is an integer >= 1;
    ValueError otherwise."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"batch_tokens must be an integer >= 0 (0: off), got {n!r}")
    if isinstance(length_bucket, bool) or not isinstance(length_bucket, int) or length_bucket < 1:
        raise ValueError(f"length_bucket must be an integer >= 1, got {length_bucket!r}")
    if n > 0 and data != "text":
        raise ValueError(f"batch_tokens={n} needs data=text (token-budget batches are cut from a "
                         f"text corpus), got data={data!r}")
    return n


DISTILL_TEACHERS_MAX = 8
DISTILL_ALPHA_DEFAULT = 0.5


def check_distill(teacher: Any, weights: Any = None, alpha: Any = None, dtype: str = "bf16"):
    """The distillation settings as (prefixes, weights or None, alpha): ([],
    None, 0.0) when off. distill_teacher names 1 to 8 comma-separated weight
    prefixes; distill_weights one finite positive number per teacher;
    distill_alpha lies in (0, 1] (default 0.5 with a teacher); weights or
    alpha without a teacher, and a teacher with dtype=fp8, are refused.
    ValueError otherwise."""
    prefixes = [p.strip() for p in str(teacher).split(",") if p.strip()] if teacher else []
    if isinstance(weights, (int, float)) and not isinstance(weights, bool):
        weights = str(weights)  # (a single number given as a setting)
    if not prefixes:
        if teacher:
            raise ValueError(f"distill_teacher names no weights prefix: {teacher!r}")
        if weights:
            raise ValueError(f"distill_weights={weights!r} without distill_teacher")
        if alpha is not None:
            raise ValueError(f"distill_alpha={alpha!r} without distill_teacher")
        return [], None, 0.0
    if len(prefixes) > DISTILL_TEACHERS_MAX:
        raise ValueError(f"distill_teacher: at most {DISTILL_TEACHERS_MAX} teachers, got {len(prefixes)}")
    if dtype == "fp8":
        raise ValueError("distill_teacher with dtype=fp8 is not supported: the distillation step "
                         "trains in bf16 (use dtype=bf16)")
    w = None
    if weights:
        try:
            w = [float(x) for x in str(weights).split(",") if x.strip()]
        except ValueError:
            raise ValueError(f"distill_weights must be comma-separated numbers, got {weights!r}") from None
        if len(w) != len(prefixes):
            raise ValueError(f"distill_weights has {len(w)} values for {len(prefixes)} teachers")
        if not all(0.0 < x < float("inf") for x in w):
            raise ValueError(f"distill_weights must be finite and > 0, got {weights!r}")
    if alpha is None:
        alpha = DISTILL_ALPHA_DEFAULT
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"distill_alpha must lie in (0, 1], got {alpha!r}")
    return prefixes, w, float(alpha)
