"""Greedy translation harness (reference: distributed_training_transformer/
tester.py:4-59 and test.py:1-44).

Same contract as the reference Tester: tokenize the source, start the target
with [START], append the argmax token until [END] or `max_length`, return
(text, tokens, attention_weights), where the attention weights are recomputed
on output[:, :-1] and keyed `decoder_layer{i}_block{1,2}` [B, H, Lq, Lk].

MI355X design: batched (many sentences decode together; finished rows are
padded), the encoder output and the stacked cross-attention K/V projection
are computed once per call instead of once per generated token, and each
step runs the decoder stack through the same HIP kernels as training, with
only the last position projected to the vocabulary.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble, members
from tensorflow_distributed_on_gke_amd.infer.step import DecoderStep
from tensorflow_distributed_on_gke_amd.models.layers import CrossKVFn, EmbedFn, KVGrad, RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, seq_lengths


class Tester:
    __test__ = False  # not a pytest class

    def __init__(self, tokenizers, transformer: Union[Transformer, Ensemble]):
        """`tokenizers` has `.pt` (source) and `.en` (target) tokenizers, as
        the reference's; a single tokenizer object is used for both.
        `transformer` is one model or an `Ensemble` (infer/ensemble.py) of
        several, decoded together."""
        self.src_tok = getattr(tokenizers, "pt", tokenizers)
        self.tgt_tok = getattr(tokenizers, "en", tokenizers)
        self.model = transformer

    def _single(self, what: str) -> Transformer:
        """The one model `what` runs on: an ensemble has no such path."""
        if isinstance(self.model, Ensemble):
            raise ValueError(f"{what} decodes one model; an ensemble decodes with the K/V cache "
                             "(beam search or sampling)")
        return self.model

    @torch.no_grad()
    def greedy(self, src: torch.Tensor, max_length: int = 20) -> torch.Tensor:
        """src int64 [B, S] -> int64 [B, 1 + n] ([START] + generated ids)."""
        m = self._single("greedy")
        dev = m.device
        src = src.to(dev)
        start, end = self.tgt_tok.start_end()
        B = src.shape[0]
        rt = RunCtx(training=False, store=None)
        src_len = seq_lengths(src)
        enc = m.encode(src, src_len, rt)
        kv_all = CrossKVFn.apply(enc, m.cross_kv.w, m.cross_kv.b, KVGrad(), rt)
        out = torch.full((B, 1), start, dtype=torch.int64, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        for _ in range(max_length):
            tgt_len = seq_lengths(out)
            x = EmbedFn.apply(m.store.anchor, out, m.dec_emb, m.pe_tgt, m.dec_site, rt)
            kvh = KVGrad()
            for layer in m.dec_layers:
                x = layer(x, kv_all, kvh, src_len, tgt_len, rt)
            last = x[:, -1:, :]
            lg = m.project(last.contiguous())[:, : m.cfg.tgt_vocab].float()
            nxt = lg.argmax(dim=-1)
            nxt = torch.where(done, torch.full_like(nxt, PAD_ID), nxt)
            out = torch.cat([out, nxt.view(B, 1)], dim=1)
            done |= nxt == end
            if bool(done.all()):
                break
        return out

    @torch.no_grad()
    def greedy_cached(self, src: torch.Tensor, max_length: int = 20) -> torch.Tensor:
        """Greedy decoding with a per-layer self-attention K/V cache: each step
        runs the decoder on the ONE new token (O(T) work per step instead of
        the reference's full re-forward, tester.py:30-42). Same output as
        `greedy` up to floating-point summation order."""
        m = self._single("greedy_cached")
        dev = m.device
        src = src.to(dev)
        start, end = self.tgt_tok.start_end()
        B = src.shape[0]
        src_len = seq_lengths(src)
        step = DecoderStep(m, src, src_len, B, max_length, single_query=False)
        out = torch.full((B, 1), start, dtype=torch.int64, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        for t in range(max_length):
            klen = torch.full((B,), t + 1, dtype=torch.int32, device=dev)
            lg = step.logits(out[:, -1], t, klen, src_len)[:, : m.cfg.tgt_vocab].float()
            nxt = lg.argmax(dim=-1)
            nxt = torch.where(done, torch.full_like(nxt, PAD_ID), nxt)
            out = torch.cat([out, nxt.view(B, 1)], dim=1)
            done |= nxt == end
            if bool(done.all()):
                break
        return out

    @torch.no_grad()
    def attention_weights(self, src: torch.Tensor, tgt_in: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The decoder's attention maps; of an ensemble, its first member's."""
        m = members(self.model)[0][0]
        rt = RunCtx(training=False, store=None, attn_maps={})
        m.features(src.to(m.device), tgt_in.to(m.device), rt)
        out = {}
        for i, layer in enumerate(m.dec_layers):
            out[f"decoder_layer{i + 1}_block1"] = rt.attn_maps[layer.site1]
            out[f"decoder_layer{i + 1}_block2"] = rt.attn_maps[layer.site2]
        return out

    def decode(self, src: torch.Tensor, max_length: int = 20, kv_cache: bool = True, beam: int = 1,
               alpha: float = 0.6, sample: int = 0, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, seed: int = 0, row_id0: int = 0, n_best: bool = False,
               mbr: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """src int64 [B, S] -> (tokens int64 [B, n, 1 + len] on the CPU, scores
        f32 [B, n] or None): greedy (n = 1, no scores), beam search (beam > 1:
        n = 1, the best hypothesis; with `n_best` n = beam, all of them by
        descending ranking score, of which the first is that best one; a slot
        that never held a hypothesis has score -inf) or `sample` draws per
        sentence. An ensemble decodes on the K/V cache only (`kv_cache=False`
        is an error), and its greedy mode is beam search of width 1 with
        alpha 0, whose score is returned. `mbr`: of the `sample` draws, or of
        the beam's hypotheses, the one of highest expected utility
        (`decode_mbr`), in the n = 1 form, with its model score."""
        if sample < 0:
            raise ValueError(f"sample must be >= 0, got {sample}")
        if sample > 0 and beam > 1:
            raise ValueError("beam > 1 and sample > 0 exclude each other")
        if n_best and beam <= 1:
            raise ValueError("n_best lists the hypotheses of a beam search: it needs beam > 1")
        start, end = self.tgt_tok.start_end()
        ensemble = isinstance(self.model, Ensemble)
        if ensemble and not kv_cache:
            raise ValueError("an ensemble decodes with the K/V cache: kv_cache=False is not supported")
        if mbr:
            if n_best:
                raise ValueError("mbr keeps one hypothesis per sentence: it does not go with n_best")
            return self.decode_mbr(src, max_length, beam=beam, alpha=alpha, sample=sample,
                                   temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                   row_id0=row_id0)[:2]
        if sample > 0:
            from tensorflow_distributed_on_gke_amd.infer.sample import sample_search

            tokens, scores = sample_search(self.model, src, start, end, n=sample, max_length=max_length,
                                           temperature=temperature, top_k=top_k, top_p=top_p,
                                           seed=seed, row_id0=row_id0)
            return tokens.cpu(), scores.cpu()
        if beam > 1 or ensemble:
            from tensorflow_distributed_on_gke_amd.infer.beam import beam_search, length_penalty

            tokens, scores, all_tokens, all_scores = beam_search(
                self.model, src, start, end, beam=beam, max_length=max_length,
                alpha=alpha if beam > 1 else 0.0)
            if n_best:
                # beam_search's own ranking: score / ((5 + len) / 6) ** alpha, len up to
                # and including [END], the first of equal values first
                is_end = (all_tokens[:, :, 1:] == end).long()
                length = (is_end.cumsum(dim=2) - is_end == 0).sum(dim=2)
                ranked = all_scores / length_penalty(length, alpha)
                order = torch.sort(-ranked, dim=1, stable=True).indices
                all_tokens = all_tokens.gather(1, order.unsqueeze(-1).expand_as(all_tokens))
                return all_tokens.cpu(), all_scores.gather(1, order).cpu()
            return tokens.cpu().unsqueeze(1), scores.cpu().unsqueeze(1)
        out = (self.greedy_cached if kv_cache else self.greedy)(src, max_length).cpu()
        return out.unsqueeze(1), None

    def decode_mbr(self, src: torch.Tensor, max_length: int = 20, beam: int = 1, alpha: float = 0.6,
                   sample: int = 0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                   seed: int = 0, row_id0: int = 0
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Minimum-Bayes-risk decoding (infer/mbr.py): the candidates of a
        sentence are its `sample` >= 2 draws, or the hypotheses of its beam
        search of width `beam` >= 2 (slots of score -inf, which never held
        one, left out), and the one closest to all of them is kept. Selection
        runs on the device tokens, before anything is copied to the host.
        src int64 [B, S] -> (tokens int64 [B, 1, 1 + len], the kept
        candidate's model score f32 [B, 1], its expected utility f64 [B]), on
        the CPU."""
        from tensorflow_distributed_on_gke_amd.infer.mbr import mbr_select

        if sample > 0 and beam > 1:
            raise ValueError("beam > 1 and sample > 0 exclude each other")
        if max(sample, beam) < 2:
            raise ValueError("mbr selects among candidates: it needs sample >= 2 or beam >= 2")
        start, end = self.tgt_tok.start_end()
        valid = None
        if sample > 0:
            from tensorflow_distributed_on_gke_amd.infer.sample import sample_search

            tokens, scores = sample_search(self.model, src, start, end, n=sample, max_length=max_length,
                                           temperature=temperature, top_k=top_k, top_p=top_p,
                                           seed=seed, row_id0=row_id0)
        else:
            from tensorflow_distributed_on_gke_amd.infer.beam import beam_search

            _, _, tokens, scores = beam_search(self.model, src, start, end, beam=beam,
                                               max_length=max_length, alpha=alpha)
            valid = scores > float("-inf")
        best, expected = mbr_select(tokens, end, PAD_ID, valid)
        pick = best.view(-1, 1)
        kept = tokens.gather(1, pick.unsqueeze(-1).expand(-1, 1, tokens.shape[2]))
        return kept.cpu(), scores.gather(1, pick).cpu(), expected.gather(1, pick).view(-1).cpu()

    @torch.no_grad()
    def score(self, src: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
        """Teacher-forced f32 log-probability [B] of tokens int64 [B, 1 + len]
        ([START] first): the sum over the generated tokens up to and including
        the first [END]. Of an ensemble: the log of the weighted mean of the
        members' probabilities, token by token."""
        _, end = self.tgt_tok.start_end()
        tokens = tokens.to(self.model.device)
        if isinstance(self.model, Ensemble):
            lp = self.model.log_probs(src.to(self.model.device), tokens[:, :-1])
        else:
            lp = torch.log_softmax(self.model.logits(src.to(self.model.device), tokens[:, :-1]), dim=-1)
        tok_lp = lp.gather(2, tokens[:, 1:].unsqueeze(-1)).squeeze(-1)
        after_end = (tokens[:, 1:] == end).long().cumsum(dim=1) - (tokens[:, 1:] == end).long() > 0
        return tok_lp.masked_fill(after_end, 0.0).sum(dim=1).cpu()

    def translate_lines(self, lines: Sequence[str], batch: int = 32, max_length: int = 20, **mode
                        ) -> List[List[Tuple[str, float]]]:
        """Per line, in input order, its (hypothesis, score) list: one entry
        (greedy, beam), `beam` entries (beam search with `n_best`, best first;
        slots that never held a hypothesis are left out) or `sample` entries.
        With `mbr=True` (and sample >= 2 or beam >= 2) one entry, the
        candidate `decode_mbr` keeps, as (hypothesis, score, expected
        utility). Lines are decoded `batch` at a
        time in order of source length, so that a batch pads little; `mode`
        are the decoding arguments of `decode`. In sample mode line i's rows
        have the identities i * sample .. in the random stream, whichever
        batch the line falls into."""
        n = max(1, mode.get("sample", 0))
        mbr = mode.get("mbr", False)
        if mbr and mode.get("n_best"):
            raise ValueError("mbr keeps one hypothesis per sentence: it does not go with n_best")
        lens = [int((self.src_tok.tokenize(s) != PAD_ID).sum()) for s in lines]
        order = sorted(range(len(lines)), key=lambda i: (lens[i], i))
        out: List[List[Tuple[str, float]]] = [[] for _ in lines]
        for b0 in range(0, len(order), batch):
            idx = order[b0:b0 + batch]
            src = self.src_tok.tokenize([lines[i] for i in idx])
            kw = dict(mode, row_id0=[i * n for i in idx]) if mode.get("sample", 0) > 0 else mode
            if mbr:
                kw = {k: v for k, v in kw.items() if k not in ("mbr", "kv_cache")}
                tokens, scores, utility = self.decode_mbr(src, max_length, **kw)
                for j, i in enumerate(idx):
                    out[i] = [(self._text(tokens[j, 0].tolist())[0], float(scores[j, 0]),
                               float(utility[j]))]
                continue
            tokens, scores = self.decode(src, max_length, **kw)
            if scores is None:
                scores = self.score(src, tokens[:, 0]).view(-1, 1)
            for j, i in enumerate(idx):
                out[i] = [(self._text(row)[0], float(scores[j, k]))
                          for k, row in enumerate(tokens[j].tolist())
                          if not mode.get("n_best") or scores[j, k] > float("-inf")]
        return out

    def score_pairs(self, sources: Sequence[str], targets: Sequence[str], batch: int = 32,
                    want_top: bool = False) -> List[Tuple[float, int, List[float], Optional[List[float]]]]:
        """Per (source, target) pair of text, in input order, its teacher-forced
        (log-probability, scored tokens, per-token log-probabilities,
        per-token largest log-probabilities or None): infer/score.py on
        targets tokenised as training tokenises them ([START] ... [END]). Pairs
        are scored `batch` at a time in order of (source length, target
        length), so that a batch pads little. A pair with a side longer than
        the model's positional table is not scored: (nan, 0, [], None)."""
        from tensorflow_distributed_on_gke_amd.infer.score import score_pairs

        if len(sources) != len(targets):
            raise ValueError(f"{len(sources)} sources for {len(targets)} targets")
        src_rows = [self.src_tok.tokenize(s)[0] for s in sources]
        tgt_rows = [self.tgt_tok.tokenize(t)[0] for t in targets]
        slen = [int((r != PAD_ID).sum()) for r in src_rows]
        tlen = [int((r != PAD_ID).sum()) for r in tgt_rows]
        cfg = self.model.cfg
        out: list = [(float("nan"), 0, [], None)] * len(sources)
        order = sorted((i for i in range(len(sources))
                        if slen[i] <= cfg.max_src_len and tlen[i] - 1 <= cfg.max_tgt_len),
                       key=lambda i: (slen[i], tlen[i], i))
        _, end = self.tgt_tok.start_end()
        for b0 in range(0, len(order), batch):
            idx = order[b0:b0 + batch]
            src = torch.zeros(len(idx), max(slen[i] for i in idx), dtype=torch.int64)
            tgt = torch.zeros(len(idx), max(tlen[i] for i in idx), dtype=torch.int64)
            for j, i in enumerate(idx):
                src[j, :slen[i]] = src_rows[i][:slen[i]]
                tgt[j, :tlen[i]] = tgt_rows[i][:tlen[i]]
            sc = score_pairs(self.model, src, tgt, want_top=want_top, end=end)
            tok_lp, top_lp = sc.tok_lp.cpu(), sc.top_lp.cpu() if want_top else None
            sent, n_tok = sc.sent_lp.cpu(), sc.n_tok.cpu()
            for j, i in enumerate(idx):
                n = int(n_tok[j])
                out[i] = (float(sent[j]), n, tok_lp[j, :n].tolist(),
                          top_lp[j, :n].tolist() if want_top else None)
        return out

    def _text(self, row: List[int]):
        """One decoded row -> (text, token names), cut after [END], PAD dropped."""
        _, end = self.tgt_tok.start_end()
        if end in row:
            row = row[: row.index(end) + 1]
        row = [t for t in row if t != PAD_ID]
        return self.tgt_tok.detokenize(row), self.tgt_tok.lookup(row)

    def __call__(self, sentence: Union[str, Sequence[str]], max_length: int = 20, kv_cache: bool = True,
                 beam: int = 1, alpha: float = 0.6, sample: int = 0, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0, seed: int = 0, mbr: bool = False
                 ) -> Tuple[Union[str, List[str]], list, Dict[str, torch.Tensor]]:
        """beam > 1: beam search (infer/beam.py) with length penalty `alpha`
        instead of the greedy argmax; the return value has the same form.
        sample > 0: `sample` translations per sentence drawn with temperature,
        top-k and top-p (infer/sample.py); texts and tokens are then a list per
        sentence, the attention maps those of every sentence's first sample.
        mbr: of those samples, or of the beam's hypotheses, the one `decode_mbr`
        keeps, in the form of the greedy result."""
        single = isinstance(sentence, str)
        src = self.src_tok.tokenize(sentence)
        out, _ = self.decode(src, max_length, kv_cache=kv_cache, beam=beam, alpha=alpha, sample=sample,
                             temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, mbr=mbr)
        many = sample > 0 and not mbr
        texts, tokens = [], []
        for rows in out.tolist():
            pairs = [self._text(row) for row in rows]
            texts.append([p[0] for p in pairs] if many else pairs[0][0])
            tokens.append([p[1] for p in pairs] if many else pairs[0][1])
        attn = self.attention_weights(src, out[:, 0, :-1])
        if single:
            return texts[0], tokens[0], attn
        return texts, tokens, attn
