"""MBR selection (infer/mbr.py), corpus BLEU (infer/bleu.py) and their command
line on the CPU, against the Python references of ref_overlap.py."""
import os
import random

import pytest
import torch

import ref_overlap as R
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.infer.bleu import corpus_bleu, format_bleu
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.mbr import mbr_select, select_text, sentence_bleu
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, OFFSET, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # the utility lies in [0, 1]: about ten f64 operations on exact integers
CANDS = ["the cat sat on the mat", "the cat sat on a mat", "a cat sat on the mat", "a dog"]
HYPS = ["the cat sat on the mat", "a dog barked"]
REFS = ["the cat sat on a mat", "the dog barked loudly"]
BLEU_LINE = "BLEU = 44.15 77.8/57.1/40.0/33.3 (BP = 0.895 ratio = 0.900 hyp_len = 9 ref_len = 10)"


def _tokens(groups, T, tail=None):
    """groups of token lists -> int64 [B, n, 1 + T]: [START], the tokens,
    [END] where there is room, then PAD (or `tail`, which must be ignored)."""
    B, n = len(groups), len(groups[0])
    t = torch.full((B, n, 1 + T), PAD_ID, dtype=torch.int64)
    t[:, :, 0] = START
    for b, g in enumerate(groups):
        for i, c in enumerate(g):
            t[b, i, 1:1 + len(c)] = torch.tensor(c, dtype=torch.int64)
            if len(c) < T:
                t[b, i, 1 + len(c)] = END
                if tail is not None:
                    t[b, i, 2 + len(c):] = torch.tensor(tail(T - 1 - len(c)), dtype=torch.int64)
    return t


def _check(groups, T, valid=None, tail=None):
    tokens = _tokens(groups, T, tail)
    v = None if valid is None else torch.tensor(valid)
    best, expected = mbr_select(tokens, END, PAD_ID, v)
    assert best.dtype == torch.int64 and expected.dtype == torch.float64
    assert best.shape == (len(groups),) and expected.shape == tokens.shape[:2]
    for b, g in enumerate(groups):
        want_best, want = R.mbr_ref(g, None if valid is None else valid[b])
        for i, w in enumerate(want):
            got = float(expected[b, i])
            assert got == w if w == float("-inf") else abs(got - w) <= TOL, (b, i, got, w)
        top = sorted((w for w in want if w > float("-inf")), reverse=True)
        if len(top) < 2 or top[0] - top[1] > 1e-9 or want.count(top[0]) > 1:
            assert int(best[b]) == want_best, (b, want)
    return best, expected


def test_worked_example():
    ids = {}
    group = [[ids.setdefault(w, 10 + len(ids)) for w in c.split()] for c in CANDS]
    best, expected = _check([group], T=8)
    assert int(best[0]) == 2
    for got, want in zip(expected[0].tolist(), (0.610593, 0.576216, 0.617337, 0.297848)):
        assert abs(got - want) < 1e-6
    m = torch.tensor(R.matches_ref(group[3], group[1]))
    assert abs(float(sentence_bleu(m, torch.tensor(2), torch.tensor(6))) - 0.095696) < 1e-6
    assert abs(float(sentence_bleu(m, torch.tensor(6), torch.tensor(2))) - 0.193049) < 1e-6


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [2, 5, 8])
def test_random_groups(B, n):
    rng = random.Random(10 * B + n)
    for vocab in ([10, 11], list(range(10, 40))):
        groups = [[[rng.choice(vocab) for _ in range(rng.randint(1, 12))] for _ in range(n)]
                  for _ in range(B)]
        _check(groups, T=12)


def test_duplicates_are_bitwise_equal_and_the_first_wins():
    a, b = [10, 11, 12, 13, 14], [10, 11, 15]
    group = [b, a, [20, 21], a, b, a]
    best, expected = _check([group], T=6)
    e = expected[0]
    assert e[1].item() == e[3].item() == e[5].item() and e[0].item() == e[4].item()
    assert int(best[0]) == 1


def test_valid_mask_and_group_without_candidates():
    rng = random.Random(3)
    groups = [[[rng.choice([10, 11, 12]) for _ in range(rng.randint(1, 7))] for _ in range(5)]
              for _ in range(3)]
    valid = [[True, False, True, True, False], [False] * 5, [False, False, False, True, False]]
    best, expected = _check(groups, T=8, valid=valid)
    assert torch.isinf(expected[1]).all() and int(best[1]) == 0
    assert int(best[2]) == 3 and float(expected[2, 3]) == 1.0
    # an invalid slot is no reference either: its content does not matter
    other = [list(g) for g in groups]
    other[0][1], other[0][4] = [10] * 7, []
    b2, e2 = _check(other, T=8, valid=valid)
    assert torch.equal(b2, best) and torch.equal(e2, expected)


def test_empty_candidates_and_tokens_after_end():
    groups = [[[], [10, 11], [], [10, 11, 12]], [[], [], [], []]]
    best, expected = _check(groups, T=5)
    assert expected[0, 0] == 0 and expected[0, 2] == 0
    assert (expected[1] == 0).all() and int(best[1]) == 0
    # whatever follows the first [END] is ignored, real-looking tokens included
    b2, e2 = _check(groups, T=5, tail=lambda k: [10, END, 11, 12, 10][:k])
    assert torch.equal(b2, best) and torch.equal(e2, expected)
    # no room at all: every candidate is empty
    b3, e3 = mbr_select(torch.full((2, 3, 1), START, dtype=torch.int64), END, PAD_ID)
    assert b3.tolist() == [0, 0] and (e3 == 0).all()
    with pytest.raises(ValueError):
        mbr_select(torch.zeros(1, 2, 514, dtype=torch.int64), END, PAD_ID)


def test_select_text():
    groups = [CANDS, ["only one"], ["B a", "b A", "c"], ["x y", "x y", "z"]]
    got = select_text(groups, device="cpu")
    assert [g[0] for g in got] == [2, 0, 0, 0]
    assert abs(got[0][1] - 0.617337) < 1e-6 and got[1][1] == 1.0
    assert select_text(groups, device="cpu", pairs_per_launch=1) == got  # one group per launch
    lc = select_text(groups, lowercase=True, device="cpu")
    assert lc[2][1] > got[2][1]
    with pytest.raises(ValueError, match="candidate 2 of group 1"):
        select_text([["a", "w " * 513]], device="cpu")


# ---------------------------------------------------------------- corpus BLEU
def test_corpus_bleu_worked_example():
    b = corpus_bleu(HYPS, REFS, device="cpu")
    assert b.matches == (7, 4, 2, 1) and b.totals == (9, 7, 5, 3)
    assert (b.hyp_len, b.ref_len) == (9, 10)
    assert abs(b.score - 44.150346) < 1e-6
    assert format_bleu(b) == BLEU_LINE
    want = R.corpus_bleu_ref(HYPS, REFS)
    assert abs(b.score - want["score"]) < 1e-9 and abs(b.bp - want["bp"]) < 1e-12


def test_corpus_bleu_edges():
    assert corpus_bleu(["a b c", "d e f"], ["a b c x", "d e f y"], device="cpu").score == 0.0  # no 4-gram
    b = corpus_bleu(["a b c d e f"], ["a b c d"], device="cpu")
    assert b.bp == 1.0 and b.matches == (4, 3, 2, 1) and b.totals == (6, 5, 4, 3)
    assert corpus_bleu(["The Cat sat down"], ["the cat SAT down"], device="cpu").score == 0.0
    assert abs(corpus_bleu(["The Cat sat down"], ["the cat SAT down"], lowercase=True,
                           device="cpu").score - 100.0) < 1e-9
    assert corpus_bleu([], [], device="cpu").score == 0.0
    with pytest.raises(ValueError, match="reference line 2"):
        corpus_bleu(["a", "b"], ["a", "w " * 513], device="cpu")
    with pytest.raises(ValueError):
        corpus_bleu(["a"], ["a", "b"], device="cpu")
    rng = random.Random(2)
    words = "a b c d e f g".split()
    hyps = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 30))) for _ in range(20)]
    refs = [" ".join(rng.choice(words) for _ in range(rng.randint(1, 30))) for _ in range(20)]
    b, want = corpus_bleu(hyps, refs, device="cpu"), R.corpus_bleu_ref(hyps, refs)
    assert list(b.matches) == want["matches"] and list(b.totals) == want["totals"]
    assert abs(b.score - want["score"]) < 1e-9


# ---------------------------------------------------------------- Tester and the command line
SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]
LINES = ["olá", "este é um teste", "muitas pessoas"]


def _cli(cmd, *args):
    argv = [cmd]
    if cmd == "test":
        argv += ["--config", os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu"]
        for kv in SETS:
            argv += ["--set", kv]
    return main(argv + list(args))


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """A tiny model whose output bias favours lower-case letters and [END]:
    what it generates is text that survives detokenising and tokenising
    again, and it ends."""
    from tensorflow_distributed_on_gke_amd.train.loop import build_model

    m = build_model(load_settings(overrides=SETS), "cpu")
    keep = [OFFSET + b for b in b"abcdefghijklmnopqrstuvwxyz"]
    m.final.b.master[keep] += 20.0
    m.final.b.master[END] += 22.5
    prefix = str(tmp_path_factory.mktemp("mbr") / "w" / "model_weights")
    bundle.save_weights(m.store, prefix)
    return prefix


@pytest.fixture(scope="module")
def source_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("in") / "in.txt"
    p.write_text("\n".join(LINES) + "\n", encoding="utf-8")
    return str(p)


def _rows(path):
    with open(path, encoding="utf-8") as f:
        return [line.rstrip("\n").split("\t") for line in f]


def _pick(group):
    """Of the (source, hypothesis, score) rows of one source, the one mbr_ref
    keeps, by the hypotheses' byte tokens, and its expected utility."""
    best, expected = R.mbr_ref([list(r[1].encode("utf-8")) for r in group])
    return group[best], expected[best]


def test_cli_sample_mbr(weights, source_file, tmp_path, capsys):
    every, kept = str(tmp_path / "all.tsv"), str(tmp_path / "mbr.tsv")
    base = ["--weights", weights, "--sample", "4", "--seed", "3", "--max-length", "12", "--input", source_file,
            "--output"]
    assert _cli("test", *base, every) == 0
    assert _cli("test", *base, kept, "--mbr") == 0
    ra, rk = _rows(every), _rows(kept)
    assert len(ra) == 4 * len(LINES) and len(rk) == len(LINES)
    for g, row in enumerate(rk):
        want, utility = _pick(ra[4 * g:4 * g + 4])
        assert len(row) == 4 and row[:3] == want, (row, ra[4 * g:4 * g + 4])
        assert abs(float(row[3]) - utility) <= 1e-6
    capsys.readouterr()


def test_cli_beam_mbr_and_text_mbr(weights, source_file, tmp_path, capsys):
    every, kept, text = (str(tmp_path / n) for n in ("all.tsv", "mbr.tsv", "text.tsv"))
    base = ["--weights", weights, "--beam", "4", "--max-length", "12", "--input", source_file, "--output"]
    assert _cli("test", *base, every, "--n-best") == 0
    assert _cli("test", *base, kept, "--mbr") == 0
    ra, rk = _rows(every), _rows(kept)
    assert len(rk) == len(LINES)
    for row in rk:
        group = [r for r in ra if r[0] == row[0]]
        want, utility = _pick(group)
        assert len(row) == 4 and row[:3] == want and abs(float(row[3]) - utility) <= 1e-6
    # the model-free command on that n-best file, spaces between the letters
    # so that its words are the model's tokens
    spaced = str(tmp_path / "spaced.tsv")
    with open(spaced, "w", encoding="utf-8") as f:
        for r in ra:
            f.write(f"{r[0]}\t{' '.join(r[1])}\t{r[2]}\n")
    capsys.readouterr()
    assert main(["mbr", "--input", spaced, "--output", text, "--device", "cpu"]) == 0
    assert f"{len(LINES)} groups, {len(ra)} candidates" in capsys.readouterr().out
    for row, k in zip(_rows(text), rk):
        if all(ord(c) < 128 and c != " " for r in ra if r[0] == k[0] for c in r[1]):
            assert row[1].replace(" ", "") == k[1] and abs(float(row[2]) - float(k[3])) <= 2e-6


def test_cli_mbr_on_a_hand_written_file(tmp_path, capsys):
    src, out = str(tmp_path / "c.tsv"), str(tmp_path / "o.tsv")
    with open(src, "w", encoding="utf-8") as f:
        for c in CANDS:
            f.write(f"s1\t{c}\t-1.5\n")
        f.write("s2\tonly one\n")
        f.write("s1\tx y\ns1\tx y\ns1\tz\n")  # a new run of s1: a group of its own
    assert main(["mbr", "--input", src, "--output", out, "--device", "cpu"]) == 0
    assert "3 groups, 8 candidates" in capsys.readouterr().out
    rows = _rows(out)
    assert [r[:2] for r in rows] == [["s1", CANDS[2]], ["s2", "only one"], ["s1", "x y"]]
    assert rows[0][2] == "0.617337" and rows[1][2] == "1.000000"
    assert main(["mbr", "--input", src, "--output", out, "--lc", "--device", "cpu"]) == 0
    capsys.readouterr()


def test_cli_bleu(tmp_path, capsys):
    hyp, ref, tsv = (str(tmp_path / n) for n in ("hyp.txt", "ref.txt", "out.tsv"))
    with open(hyp, "w", encoding="utf-8") as f:
        f.write("\n".join(HYPS) + "\n")
    with open(ref, "w", encoding="utf-8") as f:
        f.write("\n".join(REFS) + "\n")
    with open(tsv, "w", encoding="utf-8") as f:
        for k, h in enumerate(HYPS):
            f.write(f"source {k}\t{h.upper()}\t-0.5\n")
    assert main(["bleu", "--hyp", hyp, "--ref", ref, "--device", "cpu"]) == 0
    assert capsys.readouterr().out.strip() == BLEU_LINE
    assert main(["bleu", "--hyp", tsv, "--hyp-field", "2", "--ref", ref, "--lc", "--device", "cpu"]) == 0
    assert capsys.readouterr().out.strip() == BLEU_LINE
    assert main(["bleu", "--hyp", tsv, "--hyp-field", "2", "--ref", ref, "--device", "cpu"]) == 0
    assert capsys.readouterr().out.startswith("BLEU = 0.00 ")


def test_cli_argument_errors(weights, source_file, tmp_path, capsys):
    out = str(tmp_path / "o.tsv")
    short = str(tmp_path / "short.txt")
    with open(short, "w", encoding="utf-8") as f:
        f.write("one line\n")
    for argv in (["test", "--weights", weights, "--mbr", "--input", source_file, "--output", out],
                 ["test", "--weights", weights, "--mbr", "--sample", "1", "--input", source_file, "--output", out],
                 ["test", "--weights", weights, "--mbr", "--beam", "3", "--n-best", "--input", source_file,
                  "--output", out],
                 ["bleu", "--hyp", source_file, "--ref", short],
                 ["bleu", "--hyp", source_file, "--ref", source_file, "--hyp-field", "2"],
                 ["mbr", "--input", source_file, "--output", out]):
        with pytest.raises(SystemExit) as e:
            _cli(*argv)
        assert e.value.code != 0, argv
    assert not os.path.exists(out)
    capsys.readouterr()


def test_tester_mbr_returns_the_single_form():
    cfg = model_config("tiny", src_vocab=300, tgt_vocab=300, max_src_len=40, max_tgt_len=40)
    t = Tester(ByteTokenizer(300), Transformer(cfg).build("cpu", seed=4))
    text, tokens, attn = t("olá", max_length=6, sample=4, mbr=True, seed=1)
    many, _, _ = t("olá", max_length=6, sample=4, seed=1)
    assert isinstance(text, str) and text in many and isinstance(tokens, list) and attn
    texts, _, _ = t(["olá", "sim"], max_length=6, beam=3, mbr=True)
    assert len(texts) == 2 and all(isinstance(x, str) for x in texts)
    src = t.src_tok.tokenize(["olá", "sim"])
    tok, sc = t.decode(src, max_length=6, sample=4, seed=1, mbr=True)
    allt, alls = t.decode(src, max_length=6, sample=4, seed=1)
    assert tok.shape[:2] == (2, 1) and sc.shape == (2, 1)
    for b in range(2):
        want, _ = R.mbr_ref([R.content(r, END, PAD_ID) for r in allt[b].tolist()])
        assert torch.equal(tok[b, 0], allt[b, want]) and sc[b, 0] == alls[b, want]
    for kw in (dict(mbr=True), dict(mbr=True, sample=1), dict(mbr=True, beam=3, n_best=True)):
        with pytest.raises(ValueError):
            t.decode(src, max_length=6, **kw)
    with pytest.raises(ValueError):
        t.translate_lines(["olá"], max_length=6, beam=3, n_best=True, mbr=True)
    lines = t.translate_lines(["olá", "sim"], max_length=6, sample=4, seed=1, mbr=True)
    assert [len(x) for x in lines] == [1, 1] and all(len(x[0]) == 3 for x in lines)
