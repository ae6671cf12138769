"""Batch preparation (csrc/kernels/batch.hip): label counts, the
teacher-forcing split, the device-corpus gather and their device counters."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C


def count_tokens(labels, out):
    C().count_tokens(labels, out)


COUNT_MAX_ENTRIES = 32
_LABEL_TOTAL: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}


def label_total(device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The static (f32 [1] total, int32 [32] per-entry) outputs of
    count_labels_multi on `device`: captured steps bake the total's address in
    as their cross entropy's `ntok`."""
    dev = torch.device(device)
    if dev.index is None:  # "cuda" and "cuda:<current>" are one device
        dev = torch.device(dev.type, torch.cuda.current_device())
    t = _LABEL_TOTAL.get(dev)
    if t is None:
        t = _LABEL_TOTAL[dev] = (torch.empty(1, dtype=torch.float32, device=dev),
                                 torch.empty(COUNT_MAX_ENTRIES, dtype=torch.int32, device=dev))
    return t


def count_labels_multi(tgts, total=None, counts=None) -> torch.Tensor:
    """One launch: the non-PAD label count (tgt[:, 1:] != 0) of up to 32
    target batches [B, T1] (int32 / int64, mixed), as f32 [1] in `total`
    (default: the device's static scalar, label_total) and per entry in
    `counts`. More than 32 entries raise and launch nothing."""
    tgts = [t.contiguous() for t in tgts]
    if total is None:
        total, counts = label_total(tgts[0].device)
    C().count_labels_multi(tgts, total, counts)
    return total


_PREP_SCRATCH: Dict[tuple, torch.Tensor] = {}


def prep_batch(src, tgt, ctr=None):
    """One launch: (tgt_in, labels, src_len, tgt_len, ntok) of a teacher-forced
    batch -- tgt[:, :-1], tgt[:, 1:], int32 non-PAD lengths, f32 [1] non-PAD
    label count -- and ctr += 1 when given (the dropout RNG step)."""
    src = src.contiguous()
    tgt = tgt.contiguous()
    B, T1 = tgt.shape
    tgt_in = torch.empty(B, T1 - 1, dtype=tgt.dtype, device=tgt.device)
    labels = torch.empty(B, T1 - 1, dtype=tgt.dtype, device=tgt.device)
    lens = torch.empty(2, B, dtype=torch.int32, device=tgt.device)
    ntok = torch.empty(1, dtype=torch.float32, device=tgt.device)
    key = (tgt.device, B)
    scratch = _PREP_SCRATCH.get(key)
    if scratch is None:  # [B] label counts, ticket (zero; the kernel re-arms it), bad-row count
        scratch = _PREP_SCRATCH[key] = torch.zeros(B + 2, dtype=torch.int32, device=tgt.device)
    C().prep_batch(src, tgt, tgt_in, labels, lens[0], lens[1], ntok, ctr, scratch)
    return tgt_in, labels, lens[0], lens[1], ntok


def interior_pad_rows(reset: bool = False) -> int:
    """Rows seen by prep_batch (since the last reset) with a PAD token before
    a non-PAD one. Attention masks keys by length, i.e. assumes trailing
    padding; the reference masks each PAD position individually
    (transformer_model.py:56-62), so callers reject batches where this is
    non-zero. Reads a device counter (a host sync): call at log points."""
    n = 0
    for scratch in _PREP_SCRATCH.values():
        n += int(scratch[-1].item())
        if reset:
            scratch[-1].zero_()
    return n


def check_trailing_padding() -> None:
    """Raise if any batch prepared on the GPU had interior PAD tokens."""
    n = interior_pad_rows(reset=True)
    if n:
        raise ValueError(f"{n} batch rows had a PAD (id 0) token before a non-PAD token; sequences "
                         "must be right-padded (attention masks keys by length)")


def gather_rows(idx, tokens, offsets, outs, bad=None) -> None:
    """One launch (batch.hip): outs[i] [B, L_i] (int64 or int32, one dtype) =
    rows idx (int32 [B]) of side i's flat store -- tokens[i] int32, offsets[i]
    int64 [n_rows + 1] -- cut at L_i and right-padded with PAD, for one or two
    sides. A cut row or an id outside the store (written all-PAD) bumps `bad`
    (int32 device word, or None). No allocation, no sync. An empty idx, an
    L < 1 or another side count raise and launch nothing."""
    C().gather_rows(idx, list(tokens), list(offsets), list(outs), bad)


_GATHER_BAD: Dict[torch.device, torch.Tensor] = {}


def gather_bad_counter(device) -> torch.Tensor:
    """The device's bad-row counter word of gather_rows (int32 [1], zeroed)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    t = _GATHER_BAD.get(dev)
    if t is None:
        t = _GATHER_BAD[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def gather_bad_rows(reset: bool = False) -> int:
    """Rows gather_rows cut or found outside the store since the last reset.
    Reads the device counters (a host sync): call at log points."""
    n = 0
    for t in _GATHER_BAD.values():
        n += int(t.item())
        if reset:
            t.zero_()
    return n


def check_gather_rows() -> None:
    """Raise if a batch gathered on the GPU asked for a row outside the corpus
    or for fewer columns than a row holds (a batch-plan bug)."""
    n = gather_bad_rows(reset=True)
    if n:
        raise ValueError(f"{n} gathered batch rows were longer than the batch's padded length or had "
                         "an id outside the device corpus; the batch plan and the corpus disagree")
