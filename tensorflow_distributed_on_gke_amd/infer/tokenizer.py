"""Reversible byte-level tokenizer (stand-in for the reference's TF-Text
subword converters `ted_hrlr_translate_pt_en_converter`, loaded at
english_portugese_dataset.py:9-18, which need TensorFlow and a download).

ids: 0 PAD, 1 UNK, 2 [START], 3 [END], 4 + byte. Any object with the same
`tokenize` / `detokenize` / `lookup` / `start_end` methods can be used by the
Tester instead (e.g. a `tokenizers` wrapper around a trained vocabulary).
"""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

PAD, UNK, START, END = 0, 1, 2, 3
OFFSET = 4


def after_first_end(tokens: torch.Tensor, end: int) -> torch.Tensor:
    """bool, of tokens' shape [..., L]: the positions strictly after the first `end` along the
    last dimension. Decoding, scoring and MBR all cut their rows by it."""
    is_end = (tokens == end).long()
    return is_end.cumsum(dim=-1) - is_end > 0


def word_ids(pieces: Sequence[str], byte_level: bool = False) -> List[int]:
    """The word index of every piece of a tokenised text (infer/align.py's
    projection to words), -1 for a piece that is part of no word. WordPiece
    names: a `##` continuation piece belongs to the word before it, every other
    piece starts one. byte_level (ByteTokenizer.lookup names): a word is a run
    of non-whitespace bytes, whitespace is part of none."""
    out, w, inside = [], -1, False
    for p in pieces:
        if byte_level:
            if p in (" ", "\t", "\n", "\r", "\x0b", "\x0c"):  # (ASCII: a UTF-8 tail byte is never one)
                inside = False
                out.append(-1)
                continue
            w += 0 if inside else 1
            inside = True
        elif not (p.startswith("##") and w >= 0):
            w += 1
        out.append(w)
    return out


class ByteTokenizer:
    def __init__(self, vocab_size: int = 260):
        if vocab_size < OFFSET + 256:
            raise ValueError("ByteTokenizer needs a vocabulary of at least 260 ids")
        self.vocab_size = vocab_size

    def start_end(self):
        return START, END

    def encode(self, text: str, add_start_end: bool = True) -> List[int]:
        ids = [OFFSET + b for b in text.encode("utf-8")]
        return [START] + ids + [END] if add_start_end else ids

    def tokenize(self, texts: Union[str, Sequence[str]]) -> torch.Tensor:
        """Right-padded int64 [B, L] with [START] ... [END]."""
        if isinstance(texts, str):
            texts = [texts]
        rows = [self.encode(t) for t in texts]
        L = max(len(r) for r in rows)
        out = torch.zeros(len(rows), L, dtype=torch.int64)
        for i, r in enumerate(rows):
            out[i, : len(r)] = torch.tensor(r, dtype=torch.int64)
        return out

    def lookup(self, ids: Sequence[int]) -> List[str]:
        names = {PAD: "[PAD]", UNK: "[UNK]", START: "[START]", END: "[END]"}
        out = []
        for i in ids:
            i = int(i)
            if i in names:
                out.append(names[i])
            elif OFFSET <= i < OFFSET + 256:
                out.append(bytes([i - OFFSET]).decode("latin-1"))
            else:
                out.append(f"<{i}>")
        return out

    def detokenize(self, ids: Sequence[int]) -> str:
        bs = bytes(int(i) - OFFSET for i in ids if OFFSET <= int(i) < OFFSET + 256)
        return bs.decode("utf-8", errors="replace")
