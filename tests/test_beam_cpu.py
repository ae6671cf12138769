"""Beam search (infer/beam.py) on the CPU f32 path: against greedy decoding,
a naive hypothesis-list reference that re-forwards every prefix, the
teacher-forced score, the copy-reordering debug mode and the length penalty."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
V = 300
MAXLEN = 12
# the model seed: chosen so that the naive reference's candidates at every cut
# are more than GAP apart for beam 3 and 4 (asserted in test_beam_equals_naive)
SEED = 23
GAP = 1e-3


@pytest.fixture(scope="module")
def setup():
    m = Transformer(model_config("tiny", src_vocab=V, tgt_vocab=V)).build("cpu", seed=SEED)
    tester = Tester(ByteTokenizer(V), m)
    return m, tester, tester.src_tok.tokenize(SENTS)


def naive_beam(m, src_row, beam, max_length):
    """One sentence. Hypotheses as a Python list of [tokens, score, finished];
    every step re-forwards all live prefixes, takes the f64 log-softmax of the
    last position and keeps the best `beam` candidates by a stable sort on
    (-score, flat index). Returns (hypotheses, smallest gap at the cut)."""
    hyps = [[[START], 0.0, False]] + [[[START], float("-inf"), True] for _ in range(beam - 1)]
    min_gap = float("inf")
    for _ in range(max_length):
        live = [i for i, h in enumerate(hyps) if not h[2] and h[1] > float("-inf")]
        logp = {}
        if live:
            pre = torch.tensor([hyps[i][0] for i in live], dtype=torch.int64)
            lg = m.logits(src_row.view(1, -1).expand(len(live), -1), pre)[:, -1].double()
            lp = torch.log_softmax(lg, dim=-1)
            logp = {i: lp[n].tolist() for n, i in enumerate(live)}
        cands = []  # (-score, flat index)
        for i, (toks, sc, fin) in enumerate(hyps):
            if sc == float("-inf"):
                continue
            if fin:
                cands.append((-sc, i * V + PAD_ID))
            else:
                cands += [(-(sc + lpv), i * V + v) for v, lpv in enumerate(logp[i])]
        cands.sort()
        if len(cands) > beam:
            min_gap = min(min_gap, cands[beam][0] - cands[beam - 1][0])
        new = []
        for neg, idx in cands[:beam]:
            i, v = divmod(idx, V)
            new.append([hyps[i][0] + [v], -neg, hyps[i][2] or v == END])
        while len(new) < beam:
            new.append([hyps[0][0] + [PAD_ID], float("-inf"), True])
        hyps = new
        if all(h[2] for h in hyps):
            break
    return hyps, min_gap


@pytest.fixture(scope="module")
def naive(setup):
    m, _, src = setup
    return {beam: [naive_beam(m, src[b], beam, MAXLEN) for b in range(len(SENTS))] for beam in (3, 4)}


def _score_bound(s):
    return 1e-4 * max(1.0, abs(s))  # f32 logsumexp and <= 12 additions against f64


def test_beam1_equals_greedy(setup):
    m, tester, src = setup
    greedy = tester.greedy_cached(src, max_length=MAXLEN)
    tokens, _, all_tokens, _ = beam_search(m, src, START, END, beam=1, max_length=MAXLEN, alpha=0.0)
    assert tokens.dtype == torch.int64 and torch.equal(tokens, greedy)
    assert torch.equal(all_tokens[:, 0], tokens)


@pytest.mark.parametrize("beam", [3, 4])
def test_beam_equals_naive(setup, naive, beam):
    m, _, src = setup
    for hyps, gap in naive[beam]:
        assert gap > GAP, f"reference gap {gap:.3e} at a cut: pick another model seed"
    _, _, all_tokens, all_scores = beam_search(m, src, START, END, beam=beam, max_length=MAXLEN)
    n1 = all_tokens.shape[2]
    assert all_tokens.shape == (len(SENTS), beam, n1) and all_scores.shape == (len(SENTS), beam)
    assert all_scores.dtype == torch.float32
    # sentences stop together: a sentence that ended early is padded
    assert n1 == max(len(h[0]) for hyps, _ in naive[beam] for h in hyps)
    for b, (hyps, _) in enumerate(naive[beam]):
        for k, (toks, sc, _) in enumerate(hyps):
            assert all_tokens[b, k].tolist() == toks + [PAD_ID] * (n1 - len(toks)), (b, k)
            assert abs(float(all_scores[b, k]) - sc) <= _score_bound(sc), (b, k)


@pytest.mark.parametrize("beam", [1, 4])
def test_score_is_teacher_forced_sum(setup, beam):
    m, _, src = setup
    tokens, scores, _, _ = beam_search(m, src, START, END, beam=beam, max_length=MAXLEN)
    lp = torch.log_softmax(m.logits(src, tokens[:, :-1]), dim=-1)
    tok_lp = lp.gather(2, tokens[:, 1:].unsqueeze(-1)).squeeze(-1)
    for b in range(len(SENTS)):
        row = tokens[b, 1:].tolist()
        n = row.index(END) + 1 if END in row else len(row)
        want = float(tok_lp[b, :n].sum())
        assert abs(float(scores[b]) - want) <= _score_bound(want), b


def test_copy_reorder_equals_index(setup):
    m, _, src = setup
    a = beam_search(m, src, START, END, beam=4, max_length=MAXLEN, reorder="index")
    c = beam_search(m, src, START, END, beam=4, max_length=MAXLEN, reorder="copy")
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_length_penalty(setup):
    m, _, src = setup
    for alpha in (0.0, 0.6):
        tokens, scores, all_tokens, all_scores = beam_search(m, src, START, END, beam=4,
                                                             max_length=MAXLEN, alpha=alpha)
        for b in range(len(SENTS)):
            ranked = []
            for k in range(4):
                row = all_tokens[b, k, 1:].tolist()
                n = row.index(END) + 1 if END in row else len(row)
                ranked.append(float(all_scores[b, k]) / ((5.0 + n) / 6.0) ** alpha)
            best = max(range(4), key=lambda k: ranked[k])
            if alpha == 0.0:
                assert best == int(all_scores[b].argmax())
            assert torch.equal(tokens[b], all_tokens[b, best]) and scores[b] == all_scores[b, best]


def test_tester_call_beam(setup):
    _, tester, _ = setup
    text, tokens, attn = tester(SENTS[0], max_length=8, beam=3)
    assert isinstance(text, str) and tokens[0] == "[START]" and len(tokens) <= 9
    assert set(attn) == {f"decoder_layer{i}_block{j}" for i in (1, 2) for j in (1, 2)}
    a1, a2 = attn["decoder_layer1_block1"], attn["decoder_layer2_block2"]
    S = tester.src_tok.tokenize(SENTS[0]).shape[1]
    assert a1.shape[0] == 1 and a1.shape[1] == 8 and a1.shape[2] == a1.shape[3] and a2.shape[3] == S
    texts, toks, _ = tester(SENTS, max_length=8, beam=3)
    assert len(texts) == 3 and len(toks) == 3
    # beam 1 is the call without the argument
    t0, k0, a0 = tester(SENTS[0], max_length=8)
    t1, k1, a1b = tester(SENTS[0], max_length=8, beam=1)
    assert t0 == t1 and k0 == k1 and all(torch.equal(a0[k], a1b[k]) for k in a0)
