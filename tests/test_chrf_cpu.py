"""chrF on the CPU: the torch arm of the character n-gram counts, the metric,
chrF-utility MBR and their command line, against ref_chrf.py and two examples
worked by hand."""
import pytest
import torch

import ref_chrf as R
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.infer.chrf import corpus_chrf, format_chrf, sentence_chrf
from tensorflow_distributed_on_gke_amd.infer.mbr import select_text
from tensorflow_distributed_on_gke_amd.ops.kernels.chrf import char_ngram_matches

CANDS = ["the cat sat on the mat", "the cat sat on a mat", "a cat sat on the mat", "a dog", "ça, c'est un chat"]


@pytest.mark.parametrize("case", R.cases(257), ids=lambda c: c[0])
def test_cpu_arm_matches_reference(case):
    _, rows, pairs, exp = case
    chr_, length = R.pack(rows, fill=rows[1][0] if rows[1] else 0)  # padding that looks like content
    pa = torch.tensor([p[0] for p in pairs] + [-1, len(rows)], dtype=torch.int32)
    pb = torch.tensor([p[1] for p in pairs] + [0, 0], dtype=torch.int32)
    want = [list(e) for e in exp] + [[-1] * 6] * 2
    assert char_ngram_matches(chr_, length, pa, pb).tolist() == want
    assert char_ngram_matches(chr_, length, pb, pa).tolist() == want


# (hyp, ref, beta, order) -> chrF; the first two by hand: abc / abd has P = R = (2/3 + 1/2 + 0) / 3,
# and ab / abab has P = 1, R = (1/2 + 1/3) / 2, chrF2 = 100 * 5 R / (4 + R)
R2 = (1 / 2 + 1 / 3) / 2
WORKED = [("abc", "abd", 2.0, 6, 100 * 7 / 18), ("ab", "abab", 2.0, 6, 100 * 5 * R2 / (4 + R2)),
          ("ab", "abab", 0.5, 6, 100 * 1.25 * R2 / (0.25 + R2)),
          ("abc", "abd", 2.0, 2, 100 * (2 / 3 + 1 / 2) / 2), ("", "abc", 2.0, 6, 0.0), ("xyz", "abc", 2.0, 6, 0.0)]


@pytest.mark.parametrize("hyp,ref,beta,order,want", WORKED)
def test_worked_examples(hyp, ref, beta, order, want):
    c = corpus_chrf([hyp], [ref], beta=beta, order=order, device="cpu")
    assert abs(c.score - want) <= 1e-12 and len(c.matches) == order
    assert abs(c.score - R.corpus_ref([hyp], [ref], beta=beta, orders=order)) <= 1e-12
    m = torch.tensor(R.matches_ref(R.units(hyp), R.units(ref)))[:order]
    u = sentence_chrf(m, torch.tensor(len(hyp)), torch.tensor(len(ref)), beta)
    assert u.dtype == torch.float64 and abs(100.0 * float(u) - want) <= 1e-12


def test_corpus_chrf_lines():
    assert format_chrf(corpus_chrf(["abc"], ["abd"], device="cpu")) == \
        "chrF2 = 38.89 (P = 38.9 R = 38.9 orders = 6 hyp_chars = 3 ref_chars = 3)"
    hyps, refs = CANDS + ["", "A  b\tC"], CANDS[1:] + ["x", "", "abc"]
    for lc in (False, True):
        got = corpus_chrf(hyps, refs, lowercase=lc, device="cpu")
        assert abs(got.score - R.corpus_ref(hyps, refs, lc)) <= 1e-12
    assert corpus_chrf([], [], device="cpu").score == 0.0
    with pytest.raises(ValueError, match="reference line 2 has 2049"):
        corpus_chrf(["a", "b"], ["a", "w " * 2049], device="cpu")
    assert corpus_chrf(["w " * 2048], ["w"], device="cpu").hyp_chars == 2048


def test_select_text_utilities():
    groups = [CANDS, ["only one"], ["B a", "b A", "c"], ["x y", "xy", "z"], ["", "a"]]
    assert select_text(groups, device="cpu", utility="bleu") == select_text(groups, device="cpu")
    for lc in (False, True):
        got = select_text(groups, lowercase=lc, device="cpu", utility="chrf")
        for (best, util), cands in zip(got, groups):
            want, expected = R.mbr_ref(cands, lc)
            assert best == want and abs(util - expected[want]) <= 1e-14
    assert got[1] == (0, 1.0) and got[3][0] == 0  # whitespace does not count: "x y" ties with "xy"
    with pytest.raises(ValueError, match="candidate 2 of group 1 has 2049 characters"):
        select_text([["a", "w" * 2049]], device="cpu", utility="chrf")
    with pytest.raises(ValueError):
        select_text(groups, device="cpu", utility="ter")


def test_tester_mbr_with_the_chrf_utility():
    from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
    from tensorflow_distributed_on_gke_amd.infer.tokenizer import ByteTokenizer
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config

    cfg = model_config("tiny", src_vocab=300, tgt_vocab=300, max_src_len=40, max_tgt_len=40)
    t = Tester(ByteTokenizer(300), Transformer(cfg).build("cpu", seed=4))
    src = t.src_tok.tokenize(["olá", "sim"])
    tok, sc, util = t.decode_mbr(src, max_length=8, sample=5, seed=1, utility="chrf")
    allt, alls = t.decode(src, max_length=8, sample=5, seed=1)
    for b in range(2):
        want, expected = R.mbr_ref([t._text(r)[0] for r in allt[b].tolist()])
        assert torch.equal(tok[b, 0], allt[b, want]) and sc[b, 0] == alls[b, want]
        assert abs(float(util[b]) - expected[want]) <= 1e-14
    text, _, _ = t("olá", max_length=8, sample=5, seed=1, mbr=True, mbr_utility="chrf")
    assert text == t._text(tok[0, 0].tolist())[0]
    lines = t.translate_lines(["olá", "sim"], max_length=8, sample=5, seed=1, mbr=True, mbr_utility="chrf")
    assert [abs(x[0][2] - float(u)) <= 1e-14 for x, u in zip(lines, util)] == [True, True]
    for kw in (dict(mbr_utility="chrf"), dict(sample=5, mbr=True, mbr_utility="ter")):
        with pytest.raises(ValueError):
            t.decode(src, max_length=8, **kw)


def test_cli(tmp_path, capsys):
    hyp, ref, cand, out = (str(tmp_path / n) for n in ("h.tsv", "r.txt", "c.tsv", "o.tsv"))
    with open(hyp, "w", encoding="utf-8") as f:
        f.write("s1\tABC\t-0.5\ns2\tab\t-0.1\n")
    with open(ref, "w", encoding="utf-8") as f:
        f.write("abd\nabab\n")
    base = ["chrf", "--hyp", hyp, "--hyp-field", "2", "--ref", ref, "--device", "cpu"]
    assert main(base + ["--lc"]) == 0
    want = R.corpus_ref(["abc", "ab"], ["abd", "abab"])
    assert capsys.readouterr().out.startswith(f"chrF2 = {want:.2f} (P = ")
    assert main(base + ["--beta", "1", "--order", "2"]) == 0
    line = capsys.readouterr().out
    assert line.startswith(f"chrF1 = {R.corpus_ref(['ABC', 'ab'], ['abd', 'abab'], beta=1.0, orders=2):.2f} ")
    assert "orders = 2 hyp_chars = 5 ref_chars = 7" in line
    with pytest.raises(SystemExit):
        main(base + ["--order", "7"])
    with open(cand, "w", encoding="utf-8") as f:
        f.write("".join(f"s1\t{c}\n" for c in CANDS) + "s2\tonly one\n")
    assert main(["mbr", "--input", cand, "--output", out, "--utility", "chrf", "--device", "cpu"]) == 0
    assert "2 groups, 6 candidates" in capsys.readouterr().out
    best, expected = R.mbr_ref(CANDS)
    with open(out, encoding="utf-8") as f:
        assert f.read() == f"s1\t{CANDS[best]}\t{expected[best]:.6f}\ns2\tonly one\t1.000000\n"
    capsys.readouterr()
