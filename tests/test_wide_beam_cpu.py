"""Beam search above width 8 on the CPU f32 path: every hypothesis' score is
its teacher-forced sum, and the width stops at 64."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config

SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]


def test_beam12_scores_are_teacher_forced_sums():
    m = Transformer(model_config("tiny", src_vocab=300, tgt_vocab=300)).build("cpu", seed=23)
    tester = Tester(ByteTokenizer(300), m)
    src = tester.src_tok.tokenize(SENTS)
    _, _, all_tokens, all_scores = beam_search(m, src, START, END, beam=12, max_length=12)
    assert all_scores.shape == (3, 12) and torch.isfinite(all_scores).any(dim=1).all()
    for i in range(12):
        want = tester.score(src, all_tokens[:, i])
        for b in range(3):
            if all_scores[b, i] > float("-inf"):
                # f32 logsumexp and <= 12 additions against the re-forwarded sum (test_beam_cpu.py)
                assert abs(float(all_scores[b, i]) - float(want[b])) <= 1e-4 * max(1.0, abs(float(want[b])))
    with pytest.raises(ValueError):
        beam_search(m, src, START, END, beam=65, max_length=12)
