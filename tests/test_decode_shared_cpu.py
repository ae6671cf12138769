"""What the decoding modes share on the host: the first-[END] mask
(infer/tokenizer.py) with what its users derive from it, and the rules between
the modes (infer/greedy.py `check_mode`) through every caller."""
import re

import pytest
import torch

from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester, check_mode
from tensorflow_distributed_on_gke_amd.infer.mbr import candidate_rows
from tensorflow_distributed_on_gke_amd.infer.score import mask_after_end
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, ByteTokenizer, after_first_end
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

ROWS = [[5, 6, 7, 8, 9],        # no [END]
        [END, 5, 6, 7, 8],      # [END] first
        [5, 6, 7, 8, END],      # [END] last
        [5, END, 6, END, 7],    # two
        [5, 6, END, PAD_ID, PAD_ID]]


def _after(row):
    """Plain loop: is position i strictly after the row's first [END]?"""
    out, seen = [], False
    for t in row:
        out.append(seen)
        seen = seen or t == END
    return out


def test_after_first_end_is_the_loop():
    tokens = torch.tensor(ROWS, dtype=torch.int64)
    want = torch.tensor([_after(r) for r in ROWS])
    got = after_first_end(tokens, END)
    assert got.dtype == torch.bool and torch.equal(got, want)
    # a 3-d input: along the last dimension, every leading index on its own
    cube = torch.stack([tokens, tokens.flip(0)])
    assert torch.equal(after_first_end(cube, END), torch.stack([want, want.flip(0)]))
    # what the users derive: the labels scoring keeps, and MBR's content length
    kept = [[t if not a else PAD_ID for t, a in zip(r, _after(r))] for r in ROWS]
    assert torch.equal(mask_after_end(tokens, END), torch.tensor(kept))
    with_start = torch.cat([torch.full((len(ROWS), 1), 2), tokens], dim=1).view(1, len(ROWS), -1)
    length = candidate_rows(with_start, END, PAD_ID)[1]
    assert length.tolist() == [5, 0, 4, 1, 2]  # up to, and excluding, the first [END]


RULES = [  # decode's arguments, the library's message, the command line's flags
    (dict(sample=-1), "sample must be >= 0, got -1", ["--sample", "-1"]),
    (dict(sample=2, beam=3), "beam > 1 and sample > 0 exclude each other", ["--sample", "2", "--beam", "3"]),
    (dict(n_best=True), "n_best lists the hypotheses of a beam search: it needs beam > 1", ["--n-best"]),
    (dict(mbr=True, beam=3, n_best=True), "mbr keeps one hypothesis per sentence: it does not go with n_best",
     ["--mbr", "--beam", "3", "--n-best"]),
    (dict(mbr=True, sample=1), "mbr selects among candidates: it needs sample >= 2 or beam >= 2",
     ["--mbr", "--sample", "1"]),
]


@pytest.fixture(scope="module")
def tester():
    cfg = model_config("tiny", src_vocab=300, tgt_vocab=300)
    return Tester(ByteTokenizer(300), Transformer(cfg).build("cpu", seed=4))


@pytest.mark.parametrize("mode,message,flags", RULES, ids=["negative_sample", "beam_and_sample", "n_best_without_beam", "mbr_and_n_best", "mbr_of_one"])
def test_mode_rules_through_every_caller(tester, tmp_path, capsys, mode, message, flags):
    text = re.escape(message) + "$"
    src = tester.src_tok.tokenize(["olá"])
    with pytest.raises(ValueError, match=text):
        check_mode(**mode)
    with pytest.raises(ValueError, match=text):
        tester.decode(src, 4, **mode)
    with pytest.raises(ValueError, match=text):
        tester.translate_lines(["olá"], max_length=4, **mode)
    if "n_best" not in mode:  # decode_mbr has no such argument
        with pytest.raises(ValueError, match=text):
            tester.decode_mbr(src, 4, **{k: v for k, v in mode.items() if k != "mbr"})
    inp, out = tmp_path / "in.txt", tmp_path / "out.tsv"
    inp.write_text("olá\n", encoding="utf-8")
    with pytest.raises(SystemExit) as e:
        main(["test", "--device", "cpu", "--config", "none.yaml", "--input", str(inp), "--output", str(out)]
             + flags)
    assert e.value.code == 2 and not out.exists()
    assert f"test: {message}\n" in capsys.readouterr().err
    check_mode(beam=4, n_best=True, alpha=0.6, temperature=1.0)  # a valid mode; other arguments pass
