"""MBR selection and corpus BLEU on the GPU: `mbr_select` on the device tokens
of sampling and of beam search against the Python reference on their CPU
copy, the device against the CPU arm, and `corpus_bleu` on the kernel."""
import random

import pytest
import torch

import ref_overlap as R
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.bleu import corpus_bleu
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.mbr import mbr_select
from tensorflow_distributed_on_gke_amd.infer.sample import sample_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

pytestmark = pytest.mark.gpu
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
MAXLEN = 12
V300 = 300
TOL = 1e-12  # the utility lies in [0, 1]: about ten f64 operations on exact integers
GAP = 1e-9   # a group whose two best reference utilities are closer has no defined best


@pytest.fixture(scope="module")
def model():
    return Transformer(model_config("tiny", src_vocab=V300, tgt_vocab=V300)).build("cuda:0", seed=4)


@pytest.fixture(scope="module")
def candidates(model):
    """(device tokens, valid mask or None) of 8 samples per sentence (top-4
    sampling: the samples of a random model share tokens) and of a beam of 4."""
    src = ByteTokenizer(V300).tokenize(SENTS)
    sampled, _ = sample_search(model, src, START, END, n=8, max_length=MAXLEN, top_k=4, seed=1)
    _, _, hyps, scores = beam_search(model, src, START, END, beam=4, max_length=MAXLEN)
    assert sampled.is_cuda and sampled.shape[:2] == (3, 8) and hyps.shape[:2] == (3, 4)
    valid = scores > float("-inf")
    fewer = valid.clone()
    fewer[:, 1] = False  # as if the second slot had never held a hypothesis
    return {"sample": (sampled, None), "beam": (hyps, valid), "beam-masked": (hyps, fewer)}


def _against_reference(tokens, valid, best, expected):
    excluded = 0
    rows, ok = tokens.cpu().tolist(), None if valid is None else valid.cpu().tolist()
    for b, group in enumerate(rows):
        want_best, want = R.mbr_ref([R.content(r, END, PAD_ID) for r in group], None if ok is None else ok[b])
        for i, w in enumerate(want):
            got = float(expected[b, i])
            print(f"group {b} candidate {i}: expected utility {got:.15f} reference {w:.15f}")
            assert got == w if w == float("-inf") else abs(got - w) <= TOL
        top = sorted((w for w in want if w > float("-inf")), reverse=True)
        if len(top) >= 2 and top[0] - top[1] <= GAP:
            excluded += 1
            continue
        assert int(best[b]) == want_best
    return excluded


@pytest.mark.parametrize("kind", ["sample", "beam", "beam-masked"])
def test_mbr_select_on_device_tokens(candidates, kind):
    tokens, valid = candidates[kind]
    best, expected = mbr_select(tokens, END, PAD_ID, valid)
    assert best.is_cuda and expected.is_cuda and expected.dtype == torch.float64
    assert _against_reference(tokens, valid, best, expected) == 0, "a group without a clear best"
    if valid is not None:
        assert torch.equal(torch.isinf(expected), ~valid)
    # the CPU arm on a copy of the same tokens
    cb, ce = mbr_select(tokens.cpu(), END, PAD_ID, None if valid is None else valid.cpu())
    assert torch.equal(best.cpu(), cb)
    finite = ~torch.isinf(ce)
    assert torch.equal(torch.isinf(expected.cpu()), ~finite)
    assert ((expected.cpu() - ce)[finite].abs() <= TOL).all()


def test_tester_decode_mbr(model):
    t = Tester(ByteTokenizer(V300), model)
    src = t.src_tok.tokenize(SENTS)
    mode = dict(max_length=MAXLEN, sample=8, top_k=4, seed=1)
    tok, score, utility = t.decode_mbr(src, **mode)
    every, scores = t.decode(src, **mode)
    best, expected = mbr_select(every, END, PAD_ID)
    for b in range(len(SENTS)):
        k = int(best[b])
        n = min(tok.shape[2], every.shape[2])
        assert torch.equal(tok[b, 0, :n], every[b, k, :n]) and score[b, 0] == scores[b, k]
        assert abs(float(utility[b]) - float(expected[b, k])) <= TOL
    one, s1 = t.decode(src, mbr=True, **mode)
    assert torch.equal(one, tok) and torch.equal(s1, score)


def test_corpus_bleu_on_the_kernel():
    rng = random.Random(7)
    words = [f"w{k}" for k in range(12)]
    hyps = [" ".join(rng.choice(words) for _ in range(rng.choice([0, 1, 3, 9, 40, 70]))) for _ in range(20)]
    refs = []
    for h in hyps:  # the hypothesis with a few words changed, dropped or added
        r = [w if rng.random() < 0.8 else rng.choice(words) for w in h.split()]
        refs.append(" ".join(r[rng.randrange(3):] + [rng.choice(words) for _ in range(rng.randrange(4))]))
    got, want = corpus_bleu(hyps, refs, device="cuda"), R.corpus_bleu_ref(hyps, refs)
    assert list(got.matches) == want["matches"] and list(got.totals) == want["totals"]
    assert (got.hyp_len, got.ref_len) == (want["hyp_len"], want["ref_len"])
    assert want["score"] > 0 and abs(got.score - want["score"]) <= 1e-9
    assert got == corpus_bleu(hyps, refs, device="cpu")
