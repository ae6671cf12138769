"""The scoring kernel (csrc/kernels/decode.hip score_tokens) against the
float64 reference of ref_score.py, its determinism, its agreement with the
sibling ensemble_logprobs, its binding's validation, and teacher-forced
scoring (infer/score.py) end to end on the GPU."""
import pytest
import torch

import ref_ensemble as re_
import ref_score as rs
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble
from tensorflow_distributed_on_gke_amd.infer.score import score_pairs
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops.kernels.decode import score_tokens
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
MARGIN = 16  # sentinel words beyond R in the allocations the outputs are views of


def _bits(t):
    return t.view(torch.int32)


def _members(logits):
    return [x.to(torch.bfloat16).to(DEV) for x in logits]


def _weights(M, weights):
    w = [1.0] * M if weights is None else [float(x) for x in weights]
    return [x / sum(w) for x in w]


def _run(members, V, labels, weights, want_top=True, pad_id=rs.PAD):
    """The kernel into the first R words of longer, sentinel-filled
    allocations; returns those views after checking the margins."""
    R = members[0].shape[0]
    bufs = [torch.full((R + MARGIN,), SENT, dtype=torch.float32, device=DEV) for _ in range(2)]
    tok, top = bufs[0][:R], bufs[1][:R]
    C().score_tokens(list(members), V, _weights(len(members), weights), labels.to(DEV), pad_id, tok,
                     top if want_top else None)
    torch.cuda.synchronize()
    assert (bufs[0][R:] == SENT).all() and (bufs[1][R:] == SENT).all(), "the kernel wrote beyond row R"
    if not want_top:
        assert (bufs[1] == SENT).all(), "top_lp written though not wanted"
    return tok, (top if want_top else None)


def _check_case(V, ld, M, R, kind):
    logits, weights, sets = rs.case(V, ld, M, R, kind)
    mem = _members(logits)
    for n, (labels, tok_ref, top_ref) in enumerate(sets):
        tok, top = _run(mem, V, labels, weights)
        e1 = rs.check(tok, tok_ref, (kind, M, R, n, "tok"))
        e2 = rs.check(top, top_ref, (kind, M, R, n, "top"))
        print(f"{kind} set {n}: max err tok {e1:.3e} top {e2:.3e}")
        assert (tok <= top).all()
        only, _ = _run(mem, V, labels, weights, want_top=False)
        assert torch.equal(_bits(only), _bits(tok)), "tok_lp depends on want_top"
        t32, p32 = _run(mem, V, labels.to(torch.int32), weights)
        assert torch.equal(_bits(t32), _bits(tok)) and torch.equal(_bits(p32), _bits(top)), "int32 labels"
        # the public wrapper is the same launch
        wt, wp = score_tokens(mem, V, labels.to(DEV), weights, pad_id=rs.PAD, want_top=True)
        assert torch.equal(_bits(wt), _bits(tok)) and torch.equal(_bits(wp), _bits(top))


# ---------------------------------------------------------------- kernel against reference
@pytest.mark.parametrize("R", re_.ROWS)
@pytest.mark.parametrize("M", re_.MEMBERS)
@pytest.mark.parametrize("V,ld", re_.SHAPES)
def test_score_tokens(V, ld, M, R):
    for kind in re_.KINDS:
        _check_case(V, ld, M, R, kind)


@pytest.mark.parametrize("M", re_.MEMBERS)
def test_score_tokens_largest_row(M):
    V, ld = re_.BIG_SHAPE
    for kind in re_.KINDS:
        _check_case(V, ld, M, 2, kind)


@pytest.mark.parametrize("M", re_.MEMBERS)
def test_pad_row_is_never_read(M):
    """Every logit of the pad_id rows is NaN: their outputs are exactly 0 and
    the other rows are what they are without them."""
    V, ld, R = 300, 304, 5
    logits, weights, sets = rs.case(V, ld, M, R, "random")
    labels = sets[0][0].clone()
    labels[1] = labels[3] = rs.PAD
    tok_ref, top_ref = rs.score_ref(re_.ensemble_ref(logits, V, weights), labels)
    mem = _members(logits)
    for x in mem:
        x[1] = float("nan")
        x[3] = float("nan")
    tok, top = _run(mem, V, labels, weights)
    assert tok[1] == 0 and tok[3] == 0 and top[1] == 0 and top[3] == 0
    rs.check(tok, tok_ref, "tok")
    rs.check(top, top_ref, "top")


def test_exact_hit_on_the_peaked_column():
    """tok_lp == top_lp bitwise where the label is the row's most probable
    token (the peaked column, far ahead of the rest), below it elsewhere."""
    V, ld, R = 300, 304, 5
    best = torch.tensor([(37 * r + 5) % V for r in range(R)])
    for M in re_.MEMBERS:
        logits, weights, mix = re_.case(V, ld, M, R, "peaked")
        assert torch.equal(best, mix.argmax(dim=1))
        tok, top = _run(_members(logits), V, best, weights, pad_id=-1)
        assert torch.equal(_bits(tok), _bits(top)), M
        tok, top = _run(_members(logits), V, (best + 1) % V, weights, pad_id=-1)
        assert (tok < top).all(), M


@pytest.mark.parametrize("R", re_.ROWS)
def test_mixed_strides(R):
    """Members with row strides 304 and 312 and one that is a column slice of a
    wider tensor (row stride 640, starting 16 columns in)."""
    V, ld = 300, 304
    logits, weights, sets = rs.case(V, ld, 3, R, "weights")
    labels = sets[-1][0]
    a = logits[0].to(torch.bfloat16).to(DEV)
    b = torch.full((R, 312), 1e4, dtype=torch.bfloat16, device=DEV)
    b[:, :ld] = logits[1].to(torch.bfloat16)
    wide = torch.full((R, 640), 1e4, dtype=torch.bfloat16, device=DEV)
    c = wide[:, 16:16 + ld]
    c.copy_(logits[2].to(torch.bfloat16))
    assert (a.stride(0), b.stride(0), c.stride(0)) == (304, 312, 640)
    tok, top = _run([a, b[:, :ld], c], V, labels, weights)
    rs.check(tok, sets[-1][1], "mixed strides tok")
    rs.check(top, sets[-1][2], "mixed strides top")
    tok2, top2 = _run(_members(logits), V, labels, weights)
    assert torch.equal(_bits(tok), _bits(tok2)) and torch.equal(_bits(top), _bits(top2)), \
        "the result depends on the members' strides"


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("V,ld", re_.SHAPES)
def test_two_launches_and_swapped_members(V, ld):
    for kind in ("random", "peaked", "masked"):
        for M in (2, 8):
            logits, weights, sets = rs.case(V, ld, M, 5, kind)
            mem = _members(logits)
            for labels, _, _ in sets:
                a, b = _run(mem, V, labels, weights), _run(mem, V, labels, weights)
                for x, y in zip(a, b):
                    assert torch.equal(_bits(x), _bits(y)), (kind, M, "two launches differ")
                if M == 2:  # equal weights: f32 max and a two-term sum commute
                    for x, y in zip(a, _run(mem[::-1], V, labels, weights)):
                        assert torch.equal(_bits(x), _bits(y)), (kind, "swapped members differ")


# ---------------------------------------------------------------- the sibling kernel
@pytest.mark.parametrize("M", re_.MEMBERS)
@pytest.mark.parametrize("V,ld", re_.SHAPES)
def test_agrees_with_ensemble_logprobs(V, ld, M):
    """tok_lp is the unrounded value of the column ensemble_logprobs rounds to
    bf16."""
    for kind in re_.KINDS:
        logits, weights, sets = rs.case(V, ld, M, 5, kind)
        mem = _members(logits)
        full = K.ensemble_logprobs(mem, V, weights).float().cpu().double()
        for labels, tok_ref, _ in sets:
            tok = _run(mem, V, labels, weights, want_top=False)[0].cpu().double()
            rows = (labels != rs.PAD) & (labels < V)
            want = full[torch.arange(5)[rows], labels[rows]]
            got = tok[rows]
            assert torch.equal(got == rs.NINF, want == rs.NINF), kind
            live = want > rs.NINF
            assert ((got - want)[live].abs() <= re_.bf16_bound(tok_ref[rows][live])).all(), kind


# ---------------------------------------------------------------- binding
def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert (t.float() == SENT).all().item(), "a rejected call wrote to its output"


def test_binding_rejects():
    R, V = 3, 16
    x = torch.zeros(R, V, dtype=torch.bfloat16, device=DEV)
    lab = torch.tensor([1, 2, 3], device=DEV)
    tok = torch.full((R,), SENT, dtype=torch.float32, device=DEV)
    top = torch.full((R,), SENT, dtype=torch.float32, device=DEV)

    def call(mem=(x, x), v=V, w=(0.5, 0.5), labels=lab, pad=0, o=tok, p=top):
        C().score_tokens(list(mem), v, list(w), labels, pad, o, p)

    flat = torch.zeros(R * V + 8, dtype=torch.bfloat16, device=DEV)
    off = flat[1:1 + R * V].view(R, V)  # 2 bytes off a 16-byte boundary
    odd = torch.zeros(R, 20, dtype=torch.bfloat16, device=DEV)  # row stride 20: not a multiple of 8
    big = torch.zeros(1, 65544, dtype=torch.bfloat16, device=DEV)
    long_out = torch.full((R + 1,), SENT, dtype=torch.float32, device=DEV)
    bad = [dict(mem=[x] * 9, w=[1 / 9] * 9), dict(mem=[], w=[]), dict(mem=(x, x.float())), dict(mem=(x, off)),
           dict(mem=(x, odd)), dict(mem=(big, big), v=65537, labels=lab[:1], o=tok[:1], p=top[:1]),
           dict(v=0), dict(mem=(x, x.cpu())), dict(w=(1.0, 0.0)),
           dict(w=(1.0, float("nan"))), dict(w=(1.0, float("inf"))), dict(w=(1.0, -1.0)), dict(w=(1.0,)),
           dict(mem=(x, x[:2])),
           # labels and outputs
           dict(labels=lab.float()), dict(labels=lab[:2]), dict(labels=lab.cpu()),
           dict(labels=torch.zeros(R, 1, dtype=torch.int64, device=DEV)),
           dict(o=long_out), dict(p=long_out), dict(o=tok[:2]), dict(p=top[:2]),
           dict(o=torch.full((R,), SENT, dtype=torch.float64, device=DEV)),
           dict(p=torch.full((R,), SENT, dtype=torch.float64, device=DEV)),
           dict(o=torch.full((R,), SENT, dtype=torch.float32)),
           dict(o=torch.full((2 * R,), SENT, dtype=torch.float32, device=DEV)[::2])]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
        _untouched(tok, top, long_out, kw.get("o", tok), kw.get("p", top))
    call()  # the same call well-formed
    torch.cuda.synchronize()
    # equal logits in both members: log(1 / 16) everywhere
    assert torch.allclose(tok.cpu(), torch.full((R,), -2.7725887), atol=1e-5)
    assert torch.equal(_bits(tok), _bits(top))
    call(mem=(x,), w=(1.0,), labels=lab.to(torch.int32), p=None)  # top_lp is optional


def test_wrapper_rejects():
    x = torch.zeros(2, 8, dtype=torch.bfloat16, device=DEV)
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    for kw in (dict(logits_list=[x] * 9), dict(logits_list=[]), dict(weights=[1.0, 0.0]),
               dict(weights=[1.0, float("nan")]), dict(V=65537), dict(labels=lab.float())):
        with pytest.raises(RuntimeError):
            score_tokens(**dict(dict(logits_list=[x, x], V=7, labels=lab, weights=None), **kw))


# ---------------------------------------------------------------- end to end
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
MAXLEN = 12
V300 = 300


@pytest.fixture(scope="module")
def gpu_models():
    cfg = model_config("tiny", src_vocab=V300, tgt_vocab=V300)
    m4 = Transformer(cfg).build("cuda:0", seed=4)
    m5 = Transformer(cfg).build("cuda:0", seed=5)
    src = ByteTokenizer(V300).tokenize(SENTS)
    hyps = beam_search(Ensemble([m4, m5]), src, START, END, beam=4, max_length=MAXLEN)[2]  # [3, 4, 1 + n]
    pairs_src = src.repeat_interleave(4, dim=0)
    tgt = hyps.reshape(12, -1).cpu()
    # two more pairs: hypotheses with an [END] put in early and their tail left in place, which
    # the scorer has to ignore
    cut = tgt[[0, 5]].clone()
    cut[:, 3] = END
    return m4, m5, torch.cat([pairs_src, pairs_src[[0, 5]]]), torch.cat([tgt, cut])


def test_score_pairs_against_the_logits(gpu_models):
    m4, m5, src, tgt = gpu_models
    B, T = tgt.shape[0], tgt.shape[1] - 1
    for model in (m4, Ensemble([m4, m5], [3.0, 1.0])):
        sc = score_pairs(model, src, tgt, want_top=True, return_logits=True)
        weights = model.weights if isinstance(model, Ensemble) else None
        assert all(x.dtype == torch.bfloat16 and x.shape == (B * T, m4.vocab_pad) for x in sc.logits)
        assert sc.tok_lp.shape == sc.top_lp.shape == (B, T) and sc.tok_lp.dtype == torch.float32
        assert sc.sent_lp.dtype == torch.float64 and sc.n_tok.dtype == torch.int64
        labels = tgt[:, 1:]
        is_end = (labels == END).long()
        after = is_end.cumsum(dim=1) - is_end > 0
        assert after[12:, 3:].all() and (labels[12:, 3:] != PAD_ID).any()
        labels = labels.masked_fill(after, PAD_ID).reshape(B * T)
        mix = re_.ensemble_ref([x.float().cpu() for x in sc.logits], V300, weights)
        tok_ref, top_ref = rs.score_ref(mix, labels, PAD_ID)
        e1 = rs.check(sc.tok_lp.reshape(-1), tok_ref, "tok")
        e2 = rs.check(sc.top_lp.reshape(-1), top_ref, "top")
        sent_ref = tok_ref.view(B, T).sum(dim=1)
        bound = (re_.f32_bound(tok_ref) * (labels != PAD_ID)).view(B, T).sum(dim=1)
        e3 = (sc.sent_lp.cpu() - sent_ref).abs()
        print(f"max err tok {e1:.3e} top {e2:.3e} sentence {float(e3.max()):.3e}")
        assert (e3 <= bound).all()
        assert torch.equal(sc.n_tok.cpu(), (labels != PAD_ID).view(B, T).sum(dim=1))
        assert (sc.tok_lp.cpu()[after] == 0).all() and (sc.top_lp.cpu()[after] == 0).all()
        assert torch.equal(sc.sent_lp, sc.tok_lp.double().sum(dim=1))


def test_one_member_is_the_model_bitwise(gpu_models):
    m4, _, src, tgt = gpu_models
    a = score_pairs(m4, src, tgt, want_top=True)
    b = score_pairs(Ensemble([m4]), src, tgt, want_top=True)
    assert torch.equal(_bits(a.tok_lp), _bits(b.tok_lp)) and torch.equal(_bits(a.top_lp), _bits(b.top_lp))
    assert torch.equal(a.sent_lp, b.sent_lp) and torch.equal(a.n_tok, b.n_tok)
