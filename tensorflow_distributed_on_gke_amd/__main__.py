"""Command line entry point.

    python -m tensorflow_distributed_on_gke_amd train [--config FILE] [--set key=value ...] [--nproc N]
    python -m tensorflow_distributed_on_gke_amd test  --weights PREFIX [PREFIX ...] [--ensemble-weights W ...]
            [--ema] [--sentence TEXT ...] [--beam N]
            [--sample N --temperature T --top-k K --top-p P --seed S] [--mbr]
            [--input FILE --output FILE [--batch N] [--n-best]]
    python -m tensorflow_distributed_on_gke_amd score --weights PREFIX [PREFIX ...] [--ensemble-weights W ...]
            [--ema] --input FILE --output FILE [--batch N] [--tokens] [--accuracy]
            [--rerank [--length-penalty A] [--mix L]]
    python -m tensorflow_distributed_on_gke_amd mbr   --input FILE --output FILE [--lc]
    python -m tensorflow_distributed_on_gke_amd bleu  --hyp FILE --ref FILE [--hyp-field K] [--ref-field K] [--lc]
    python -m tensorflow_distributed_on_gke_amd average --inputs PREFIX PREFIX ... --output PREFIX
    python -m tensorflow_distributed_on_gke_amd heartbeat --port 3479

`train` is the reference's `python -m distributed_training_transformer`
(reference: distributed_training_transformer/__main__.py:1-186): in a
Kubernetes pod (THIS_POD_NAME set) it discovers the StatefulSet peers, runs
the heartbeat barrier and launches one training process per local GPU
(`--nproc`, default: all visible GPUs); locally it launches `--nproc`
processes on 127.0.0.1, or runs in-process when started by
torch.distributed.run (RANK set) or with one process. With `--set
distill_teacher=PREFIX[,PREFIX...]` the model is a student trained on the
next-token distributions of those frozen models (train/distill.py).
`test` is the reference's test.py + Tester (greedy translation, or beam
search with --beam N --length-penalty ALPHA, or --sample N translations drawn
per sentence); with --input / --output it translates a file, one sentence per
line, to source<TAB>hypothesis<TAB>score lines; --ema decodes from the
averaged weights a run with `ema_decay` wrote next to the snapshot
(`<weights>_ema`). Several --weights prefixes decode as an ensemble
(infer/ensemble.py): one model per prefix, all built from the same settings,
their next-token probabilities averaged with --ensemble-weights (default:
equal) at every step; --ema then applies to every prefix. With --beam N
--n-best the file holds all N hypotheses per source, best first. With --mbr
(and --sample N or --beam N, N >= 2, not with --n-best) one hypothesis per
source is kept by minimum-Bayes-risk selection (infer/mbr.py): of the N
candidates the one with the highest mean smoothed sentence BLEU against all of
them; the file then holds source<TAB>hypothesis<TAB>model score<TAB>expected
utility lines.
`score` is teacher-forced scoring (infer/score.py): how probable the model, or
the ensemble, finds each target of source<TAB>target[<TAB>...] lines (the
output of `test --input` is such a file). It writes
source<TAB>target<TAB>logprob<TAB>n_tok lines in input order (--tokens: a fifth
field, the tokens' log-probs) and prints pairs, skipped pairs (a side longer
than the model's max_len: logprob nan, n_tok 0), tokens, total log-prob and
perplexity exp(-total / tokens); --accuracy adds the share of tokens that are
the model's first choice. With --rerank it writes one line per run of lines
with equal source: the one that maximises logprob / ((5 + n_tok) / 6) ** A +
L * the third input field (A default 0.6, as `test`; L default 0), ties to the
first, with that key as its third field.
`mbr` is the same selection on text, without a model: of every run of
source<TAB>candidate[<TAB>...] lines with equal source it writes
source<TAB>best candidate<TAB>expected utility, ties to the first; the units are
the candidates' whitespace-separated words (--lc: lowercased first).
`bleu` is corpus BLEU (infer/bleu.py) of --hyp against --ref, one reference
per line, over whitespace-separated words AS GIVEN: no tokenisation or
detokenisation is applied (a "tokenize none" BLEU; tokenise both files
beforehand to compare with other tools). --hyp-field / --ref-field K take the
K-th tab-separated column (1-based; default: the whole line), so `--hyp out.tsv
--hyp-field 2` reads the output of `test --input`. It prints one line: BLEU, the
four n-gram precisions, brevity penalty, length ratio and both lengths.
`average` is checkpoint averaging: the mean of several weight bundles (float64
on the host) as one f32 bundle `test --weights` and `warm_start` load.
"""
from __future__ import annotations

import argparse
import os
import sys


def _visible_gpus() -> int:
    import torch

    return torch.cuda.device_count()  # does not initialise HIP


def cmd_train(args) -> int:
    from tensorflow_distributed_on_gke_amd.config import load_settings

    settings = load_settings(args.config if os.path.exists(args.config) else None, args.set)
    in_child = "RANK" in os.environ
    if not in_child:
        from tensorflow_distributed_on_gke_amd.cluster import launch, rendezvous

        nproc = args.nproc if args.nproc > 0 else max(1, _visible_gpus())
        pod = os.environ.get("THIS_POD_NAME")
        if pod or nproc > 1:
            spec = rendezvous.bootstrap(settings.worker_count if pod else 1, namespace=args.namespace,
                                        heartbeat_port=args.heartbeat_port, master_port=args.master_port,
                                        verbose=True)
            argv = ["-m", "tensorflow_distributed_on_gke_amd", "train", "--config", args.config]
            for kv in args.set or []:
                argv += ["--set", kv]
            rc = launch.launch(argv, nproc, spec)
            if rc == 0 and settings.idle_after_train:
                from tensorflow_distributed_on_gke_amd.train.loop import idle_forever

                idle_forever()
            return rc
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer, idle_forever

    info = tdist.init_distributed(args.device)
    if info.chief:
        print(f"Number of devices: {info.world}", flush=True)
    trainer = Trainer(settings, info, log=lambda m: print(m, flush=True))
    trainer.fit()
    if trainer.ddp is not None:
        trainer.ddp.close()
    tdist.shutdown()
    if settings.idle_after_train and not in_child:
        idle_forever()
    return 0


def _load_tester(args):
    """The Tester of `test` and `score`: the settings' tokenizers and one model
    per --weights prefix (several: an ensemble)."""
    import torch

    from tensorflow_distributed_on_gke_amd.checkpoint import bundle
    from tensorflow_distributed_on_gke_amd.config import load_settings
    from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
    from tensorflow_distributed_on_gke_amd.infer.tokenizer import ByteTokenizer
    from tensorflow_distributed_on_gke_amd.train.loop import build_model

    settings = load_settings(args.config if os.path.exists(args.config) else None, args.set)
    dev = args.device if args.device != "auto" else ("cuda:0" if torch.cuda.is_available() else "cpu")
    if settings.src_tokenizer and settings.tgt_tokenizer:
        # the WordPiece pair a text-data training run saved (data/text.py); like
        # the reference, the vocabulary sizes come from the tokenizers
        from types import SimpleNamespace

        from tensorflow_distributed_on_gke_amd.data.text import WordPieceTokenizer
        pt = WordPieceTokenizer.load(settings.src_tokenizer)
        en = WordPieceTokenizer.load(settings.tgt_tokenizer)
        settings.src_vocab, settings.tgt_vocab = pt.vocab_size, en.vocab_size
        tok = SimpleNamespace(pt=pt, en=en)
    else:
        tok = ByteTokenizer(min(settings.src_vocab, settings.tgt_vocab))
    models = []
    for w in args.weights or [None]:
        model = build_model(settings, dev)
        if w:
            prefix = bundle.resolve_prefix(w)
            if args.ema:
                prefix += bundle.EMA_SUFFIX
                if not os.path.exists(prefix + ".index"):
                    raise FileNotFoundError(f"{args.cmd} --ema: no averaged weights at {prefix} (written next to "
                                            "a snapshot by a run with ema_decay > 0)")
            bundle.load_weights(model.store, prefix)
        models.append(model)
    if len(models) > 1:
        from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble

        return Tester(tok, Ensemble(models, args.ensemble_weights))
    return Tester(tok, models[0])


def _flat(text: str) -> str:
    """A field of a tab-separated output line."""
    return text.replace("\t", " ").replace("\n", " ").replace("\r", " ")


def cmd_test(args) -> int:
    tester = _load_tester(args)
    mode = dict(beam=args.beam, alpha=args.length_penalty, sample=args.sample,
                temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    if args.n_best:
        mode["n_best"] = True
    if args.mbr:
        mode["mbr"] = True
    if args.input:
        # file mode: source<TAB>hypothesis<TAB>score, input order, `sample` (or, with
        # --n-best, `beam`) lines per source; --mbr: one, with its expected utility
        with open(args.input, encoding="utf-8") as f:
            lines = [line.rstrip("\n") for line in f]
        hyps = tester.translate_lines(lines, batch=args.batch, max_length=args.max_length, **mode)
        with open(args.output, "w", encoding="utf-8") as f:
            for s, hs in zip(lines, hyps):
                for h, sc, *utility in hs:
                    f.write(f"{_flat(s)}\t{_flat(h)}\t{sc:.6f}" + "".join(f"\t{u:.6f}" for u in utility)
                            + "\n")
        print(f"{len(lines)} lines -> {args.output}")
        return 0
    text, tokens, attn = tester(list(args.sentence), max_length=args.max_length, **mode)
    for s, t in zip(args.sentence, text):
        for h in (t if args.sample > 0 and not args.mbr else [t]):
            print(f"{s!r} -> {h!r}")
    print("attention maps:", {k: tuple(v.shape) for k, v in attn.items()})
    return 0


def _read_pairs(path: str, with_prior: bool):
    """The fields of `score`'s input lines, source<TAB>target[<TAB>...], and,
    `with_prior`, the number in every line's third field (else None)."""
    with open(path, encoding="utf-8") as f:
        rows = [line.rstrip("\n").split("\t") for line in f]
    for n, r in enumerate(rows):
        if len(r) < 2:
            raise ValueError(f"{path} line {n + 1}: expected source<TAB>target")
    prior = None
    if with_prior:
        try:
            prior = [float(r[2]) for r in rows]
        except (IndexError, ValueError):
            raise ValueError(f"--mix needs a number in the third field of every line of {path}")
    return rows, prior


def cmd_score(args) -> int:
    import math

    rows, prior = args.pairs
    tester = _load_tester(args)
    scored = tester.score_pairs([r[0] for r in rows], [r[1] for r in rows], batch=args.batch,
                                want_top=args.accuracy)
    pairs = skipped = tokens = hits = 0
    total = 0.0
    out_lines = []
    for r, (lp, n, tok_lp, top_lp) in zip(rows, scored):
        pairs += 1
        if n == 0 and lp != lp:
            skipped += 1
        else:
            tokens += n
            total += lp
            if top_lp is not None:
                hits += sum(1 for a, b in zip(tok_lp, top_lp) if a >= b)
        line = f"{_flat(r[0])}\t{_flat(r[1])}\t{lp:.6f}\t{n}"
        if args.tokens:
            line += "\t" + " ".join(f"{x:.6f}" for x in tok_lp)
        out_lines.append(line)
    if args.rerank:
        # a group: a maximal run of lines with one source; its best line, the first of equal keys
        best = []
        for i, (r, (lp, n, _, _)) in enumerate(zip(rows, scored)):
            if lp != lp:
                key = None  # not scored: never wins
            else:
                key = lp / ((5.0 + n) / 6.0) ** args.length_penalty
                if prior is not None:
                    key += args.mix * prior[i]
            if i == 0 or r[0] != rows[i - 1][0]:
                best.append((i, key))
            elif key is not None and (best[-1][1] is None or key > best[-1][1]):
                best[-1] = (i, key)
        out_lines = [f"{_flat(rows[i][0])}\t{_flat(rows[i][1])}\t"
                     + (f"{key:.6f}" if key is not None else "nan") for i, key in best]
    with open(args.output, "w", encoding="utf-8") as f:
        for line in out_lines:
            f.write(line + "\n")
    ppl = math.exp(-total / tokens) if tokens else float("nan")
    msg = (f"{pairs} pairs ({skipped} skipped), {tokens} tokens, log-prob {total:.6f}, "
           f"perplexity {ppl:.6f}")
    if args.accuracy:
        msg += f", accuracy {hits / tokens if tokens else float('nan'):.6f}"
    print(msg + f" -> {args.output}")
    return 0


def _device(name: str) -> str:
    import torch

    return name if name != "auto" else ("cuda:0" if torch.cuda.is_available() else "cpu")


def _read_candidates(path: str):
    """`mbr`'s input, source<TAB>candidate[<TAB>...] lines -> (sources,
    candidate lists), one entry per maximal run of lines with equal source."""
    sources, groups = [], []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f):
            r = line.rstrip("\n").split("\t")
            if len(r) < 2:
                raise ValueError(f"{path} line {n + 1}: expected source<TAB>candidate")
            if not sources or r[0] != sources[-1]:
                sources.append(r[0])
                groups.append([])
            groups[-1].append(r[1])
    return sources, groups


def cmd_mbr(args) -> int:
    from tensorflow_distributed_on_gke_amd.infer.mbr import select_text

    sources, groups = args.groups
    try:
        picked = select_text(groups, lowercase=args.lc, device=_device(args.device))
    except ValueError as e:
        print(f"mbr: {args.input}: {e}", file=sys.stderr)
        return 2
    with open(args.output, "w", encoding="utf-8") as f:
        for s, cands, (best, utility) in zip(sources, groups, picked):
            f.write(f"{_flat(s)}\t{_flat(cands[best])}\t{utility:.6f}\n")
    print(f"{len(groups)} groups, {sum(len(g) for g in groups)} candidates -> {args.output}")
    return 0


def _read_field(path: str, field: int):
    """The lines of a file, or (field >= 1) their field-th tab-separated column."""
    with open(path, encoding="utf-8") as f:
        lines = [line.rstrip("\n") for line in f]
    if field <= 0:
        return lines
    out = []
    for n, line in enumerate(lines):
        cols = line.split("\t")
        if len(cols) < field:
            raise ValueError(f"{path} line {n + 1}: no field {field}")
        out.append(cols[field - 1])
    return out


def cmd_bleu(args) -> int:
    from tensorflow_distributed_on_gke_amd.infer.bleu import corpus_bleu, format_bleu

    try:
        b = corpus_bleu(args.hyp_lines, args.ref_lines, lowercase=args.lc, device=_device(args.device))
    except ValueError as e:
        print(f"bleu: {e}", file=sys.stderr)
        return 2
    print(format_bleu(b))
    return 0


def cmd_average(args) -> int:
    from tensorflow_distributed_on_gke_amd.checkpoint import bundle

    n = bundle.average_bundles(args.inputs, args.output)
    print(f"average of {len(args.inputs)} bundles ({n} tensors) -> {args.output}")
    return 0


def cmd_heartbeat(args) -> int:
    import time

    from tensorflow_distributed_on_gke_amd.cluster.heartbeat import start_heartbeat_server

    start_heartbeat_server(args.port)
    print(f"heartbeat server on :{args.port}", flush=True)
    while True:
        time.sleep(3600)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="tensorflow_distributed_on_gke_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--config", default="configuration/settings.yaml")
    common.add_argument("--set", action="append", default=[], metavar="KEY=VALUE")
    common.add_argument("--device", default="auto")
    t = sub.add_parser("train", parents=[common])
    t.add_argument("--nproc", type=int, default=0, help="processes (GPUs) per node; 0 = all visible")
    t.add_argument("--namespace", default=os.environ.get("POD_NAMESPACE", "default"))
    t.add_argument("--heartbeat-port", type=int, default=3479)
    t.add_argument("--master-port", type=int, default=int(os.environ.get("MASTER_PORT", 3480)))
    models = argparse.ArgumentParser(add_help=False)
    models.add_argument("--weights", nargs="+", default=None, metavar="PREFIX",
                        help="weights prefix or directory; several (at most 8) are an ensemble")
    models.add_argument("--ensemble-weights", nargs="+", type=float, default=None, metavar="W",
                        help="one positive mixture weight per --weights prefix (default: equal)")
    models.add_argument("--ema", action="store_true",
                        help="load the averaged weights saved next to --weights (<prefix>_ema)")
    e = sub.add_parser("test", parents=[common, models])
    e.add_argument("--sentence", action="append", default=None)
    e.add_argument("--max-length", type=int, default=20)
    e.add_argument("--beam", type=int, default=1, help="beam width (1 = greedy, at most 8)")
    e.add_argument("--length-penalty", type=float, default=0.6,
                   help="alpha of the beam ranking score / ((5 + len) / 6) ** alpha")
    e.add_argument("--sample", type=int, default=0, metavar="N",
                   help="draw N translations per sentence instead (not with --beam)")
    e.add_argument("--temperature", type=float, default=1.0)
    e.add_argument("--top-k", type=int, default=0, help="keep the K most likely tokens (0 = all)")
    e.add_argument("--top-p", type=float, default=1.0, help="keep the top nucleus of this mass (1 = all)")
    e.add_argument("--seed", type=int, default=0, help="seed of the sampling stream")
    e.add_argument("--input", default=None, metavar="FILE", help="one source sentence per line")
    e.add_argument("--output", default=None, metavar="FILE",
                   help="source<TAB>hypothesis<TAB>score lines, in input order")
    e.add_argument("--batch", type=int, default=32, help="sentences per batch of --input")
    e.add_argument("--n-best", action="store_true",
                   help="with --beam N and --input: all N hypotheses per source, best first")
    e.add_argument("--mbr", action="store_true",
                   help="with --sample N or --beam N (N >= 2): keep the candidate of highest expected "
                        "utility; file mode adds that utility as a fourth field")
    sc = sub.add_parser("score", parents=[common, models])
    sc.add_argument("--input", default=None, metavar="FILE",
                    help="source<TAB>target[<TAB>...] lines (the output of test --input is one)")
    sc.add_argument("--output", default=None, metavar="FILE",
                    help="source<TAB>target<TAB>logprob<TAB>n_tok lines, in input order")
    sc.add_argument("--batch", type=int, default=32, help="pairs per batch")
    sc.add_argument("--tokens", action="store_true", help="a fifth field: the tokens' log-probs")
    sc.add_argument("--accuracy", action="store_true",
                    help="also report the share of tokens that are the model's first choice")
    sc.add_argument("--rerank", action="store_true",
                    help="one line per run of equal sources: the best by logprob / "
                         "((5 + n_tok) / 6) ** A + L * third input field, that key third")
    sc.add_argument("--length-penalty", type=float, default=0.6, metavar="A")
    sc.add_argument("--mix", type=float, default=0.0, metavar="L")
    mb = sub.add_parser("mbr")
    mb.add_argument("--input", required=True, metavar="FILE",
                    help="source<TAB>candidate[<TAB>...] lines, a source's candidates on consecutive lines")
    mb.add_argument("--output", required=True, metavar="FILE",
                    help="source<TAB>best candidate<TAB>expected utility, one line per source")
    mb.add_argument("--lc", action="store_true", help="lowercase the candidates first")
    mb.add_argument("--device", default="auto")
    bl = sub.add_parser("bleu")
    bl.add_argument("--hyp", required=True, metavar="FILE")
    bl.add_argument("--ref", required=True, metavar="FILE", help="one reference per hypothesis line")
    bl.add_argument("--hyp-field", type=int, default=0, metavar="K",
                    help="the K-th tab-separated column of --hyp (1-based; default: the whole line)")
    bl.add_argument("--ref-field", type=int, default=0, metavar="K")
    bl.add_argument("--lc", action="store_true", help="lowercase both sides first")
    bl.add_argument("--device", default="auto")
    a = sub.add_parser("average")
    a.add_argument("--inputs", nargs="+", required=True, metavar="PREFIX",
                   help="weight bundles (prefixes or snapshot directories) of one model")
    a.add_argument("--output", required=True, metavar="PREFIX")
    h = sub.add_parser("heartbeat")
    h.add_argument("--port", type=int, default=3479)
    args = ap.parse_args(argv)
    if args.cmd in ("test", "score"):
        if args.ema and not args.weights:
            ap.error(f"{args.cmd}: --ema needs --weights")
        if args.weights and len(args.weights) > 8:
            ap.error(f"{args.cmd}: an ensemble has at most 8 members")
        if args.ensemble_weights is not None:
            if len(args.ensemble_weights) != len(args.weights or []):
                ap.error(f"{args.cmd}: --ensemble-weights needs one value per --weights prefix")
            if not all(0.0 < w < float("inf") for w in args.ensemble_weights):
                ap.error(f"{args.cmd}: --ensemble-weights must be finite and > 0")
    if args.cmd == "score":
        if args.input is None or args.output is None:
            ap.error("score: --input and --output are both needed")
        if args.batch < 1:
            ap.error("score: --batch must be at least 1")
        if not args.rerank and (args.mix != 0.0 or args.length_penalty != 0.6):
            ap.error("score: --mix and --length-penalty belong to --rerank")
        try:  # before any model is built
            args.pairs = _read_pairs(args.input, args.mix != 0.0)
        except (OSError, ValueError) as e:
            ap.error(f"score: {e}")
    if args.cmd == "test":
        if (args.input is None) != (args.output is None) or (args.input and args.sentence):
            ap.error("test: --input and --output go together, without --sentence")
        if args.beam > 1 and args.sample > 0:
            ap.error("test: --beam and --sample exclude each other")
        if args.batch < 1 or args.sample < 0:
            ap.error("test: --batch must be at least 1 and --sample at least 0")
        if args.n_best and (args.beam <= 1 or not args.input):
            ap.error("test: --n-best lists the hypotheses of --beam N > 1 in file mode (--input)")
        if args.mbr and max(args.beam, args.sample) < 2:
            ap.error("test: --mbr selects among candidates: it needs --sample N or --beam N, N >= 2")
        if args.mbr and args.n_best:
            ap.error("test: --mbr keeps one hypothesis per source: not with --n-best")
    if args.cmd == "mbr":
        try:  # before anything else runs
            args.groups = _read_candidates(args.input)
        except (OSError, ValueError) as e:
            ap.error(f"mbr: {e}")
    if args.cmd == "bleu":
        if args.hyp_field < 0 or args.ref_field < 0:
            ap.error("bleu: --hyp-field and --ref-field count columns from 1")
        try:
            args.hyp_lines = _read_field(args.hyp, args.hyp_field)
            args.ref_lines = _read_field(args.ref, args.ref_field)
        except (OSError, ValueError) as e:
            ap.error(f"bleu: {e}")
        if len(args.hyp_lines) != len(args.ref_lines):
            ap.error(f"bleu: {args.hyp} has {len(args.hyp_lines)} lines, {args.ref} "
                     f"{len(args.ref_lines)}")
    if args.cmd == "test" and not args.sentence and not args.input:
        args.sentence = ["muitas pessoas vieram à estação."]  # reference test.py:9
    return {"train": cmd_train, "test": cmd_test, "score": cmd_score, "mbr": cmd_mbr, "bleu": cmd_bleu,
            "average": cmd_average, "heartbeat": cmd_heartbeat}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
