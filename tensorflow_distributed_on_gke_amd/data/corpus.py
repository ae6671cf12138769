"""A tokenised parallel corpus resident on the training device.

Per side (source, target) the tokens of all rows lie back to back in one
int32 tensor, with an int64 [n_rows + 1] offset array (a corpus may exceed
2^31 tokens; row ids are int32). Both sides are uploaded once, at
construction; an epoch's laid-out row-id list is uploaded once per epoch
(`upload_ids`), and a batch is `gather(view of that list, S, T)`: on a GPU one
launch of the gather kernel (csrc/kernels/batch.hip) that fills the [B, S]
source and the [B, T] target tensor, so assembling a batch moves nothing
between host and device. On the CPU the same gather is done with torch
indexing -- also the reference the kernel is tested against. Either way the
result is bitwise what data/text.py pad_rows builds from the same rows.

The kernel cuts a row longer than the requested length and writes an id
outside the store as an all-PAD row, counting both in a device word that
`ops.kernels.check_gather_rows` reads at log points: the batch plan keeps it
at zero, and a plan bug becomes an error message, not a fault.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from tensorflow_distributed_on_gke_amd.data.text import PAD


def flatten_rows(rows: Sequence[Sequence[int]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(int32 tokens of all rows back to back, int64 [n + 1] offsets), on the host."""
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    off = torch.zeros(len(rows) + 1, dtype=torch.int64)
    torch.cumsum(lens, 0, out=off[1:])
    flat = torch.tensor([t for r in rows for t in r], dtype=torch.int32)
    return flat, off


def gather_reference(tokens: torch.Tensor, offsets: torch.Tensor, idx: torch.Tensor, L: int,
                     dtype=torch.int64) -> torch.Tensor:
    """[B, L] = the first min(len, L) tokens of store rows idx, then PAD; an
    id outside [0, n_rows) gives an all-PAD row. Torch indexing, any device."""
    n_rows = offsets.numel() - 1
    idx = idx.to(torch.int64)
    ok = (idx >= 0) & (idx < n_rows)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    start = offsets[safe]
    length = torch.where(ok, offsets[safe + 1] - start, torch.zeros_like(start))
    col = torch.arange(L, dtype=torch.int64, device=tokens.device)
    live = col[None, :] < length[:, None]
    pos = torch.where(live, start[:, None] + col[None, :], torch.zeros_like(live, dtype=torch.int64))
    if tokens.numel() == 0:
        return torch.full((idx.numel(), L), PAD, dtype=dtype, device=tokens.device)
    return torch.where(live, tokens[pos].to(dtype), torch.full((), PAD, dtype=dtype, device=tokens.device))


class DeviceCorpus:
    """Source and target rows of a corpus on `device`; see the module text."""

    def __init__(self, src_rows: Sequence[Sequence[int]], tgt_rows: Sequence[Sequence[int]], device):
        if len(src_rows) != len(tgt_rows):
            raise ValueError("DeviceCorpus: one target row per source row")
        if len(src_rows) >= 2 ** 31:
            raise ValueError("DeviceCorpus: row ids are int32")
        self.device = torch.device(device)
        self.n_rows = len(src_rows)
        sides = [flatten_rows(src_rows), flatten_rows(tgt_rows)]
        self.tokens = [t.to(self.device) for t, _ in sides]
        self.offsets = [o.to(self.device) for _, o in sides]

    @property
    def on_gpu(self) -> bool:
        return self.device.type == "cuda"

    def upload_ids(self, ids: Sequence[int]) -> torch.Tensor:
        """An epoch's laid-out row ids as int32 on the device (one copy)."""
        return torch.tensor(list(ids), dtype=torch.int32).to(self.device)

    def gather(self, idx: torch.Tensor, S: int, T: Optional[int] = None,
               dtype=torch.int64) -> Tuple[torch.Tensor, ...]:
        """(src [B, S], tgt [B, T]) of rows idx (int32, on the device); with
        T None the source side alone, as a 1-tuple."""
        Ls = [S] if T is None else [S, T]
        if not self.on_gpu:
            return tuple(gather_reference(self.tokens[i], self.offsets[i], idx, L, dtype)
                         for i, L in enumerate(Ls))
        from tensorflow_distributed_on_gke_amd.ops import kernels as K
        outs = [torch.empty(idx.numel(), L, dtype=dtype, device=self.device) for L in Ls]
        K.gather_rows(idx, self.tokens[:len(Ls)], self.offsets[:len(Ls)], outs,
                      bad=K.gather_bad_counter(self.device))
        return tuple(outs)
