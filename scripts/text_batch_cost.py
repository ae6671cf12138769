#!/usr/bin/env python3
"""What token-budget text batches cost and buy, Transformer-base on one GPU.

On a generated TSV corpus (random words, sentence lengths long-tailed like TED
talk transcripts, as scripts/text_vs_synthetic.py) it prints

1. per-batch assembly time of one epoch of token-budget batches, two ways:
   on the host -- pad_rows, a pinned copy, two host-to-device copies, the
   fixed-batch path's code -- and on the device, one gather launch over a
   resident corpus (data/corpus.py). Wall time of the assembly loop with one
   final synchronisation, the epoch's id layout built beforehand; host and
   device alternate over three epochs after a warm-up one, best epoch each;
2. processed and real (non-PAD) tokens/s of a timed epoch (the second: the
   first captures the step of every batch shape) in fixed-batch mode and in
   token-budget mode with device and with host assembly, on the same model.

    python scripts/text_batch_cost.py [--pairs 6400] [--batch 64]
                                      [--batch-tokens 4096] [--bucket 8]
Prints one JSON line per part.
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensorflow_distributed_on_gke_amd.config import Settings  # noqa: E402
from tensorflow_distributed_on_gke_amd.data.text import TextPairs, build_tokenizers  # noqa: E402
from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.loop import Trainer  # noqa: E402

DEV = torch.device("cuda")


def corpus(path, n, seed=0):
    rng = random.Random(seed)
    src_words = [f"p{i}x" for i in range(6000)]
    tgt_words = [f"e{i}y" for i in range(6000)]
    with open(path, "w") as f:
        for _ in range(n):
            k = min(150, max(2, int(rng.lognormvariate(2.9, 0.55))))
            s = " ".join(rng.choice(src_words) for _ in range(k))
            t = " ".join(rng.choice(tgt_words) for _ in range(max(2, k + rng.randint(-4, 4))))
            f.write(f"{s}\t{t}\n")


def assembly(data, e):
    """Mean wall time per batch (us) of putting epoch e's batches on the
    device, and the bytes a batch holds on average."""
    n = data.steps_per_epoch
    nbytes = 0
    data.batch(e * n)  # the epoch's layout (and its upload) is not assembly
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        s, t = data.batch(e * n + i)
        s, t = s.to(DEV, non_blocking=True), t.to(DEV, non_blocking=True)
        nbytes += (s.numel() + t.numel()) * 8
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6, nbytes / n


def epoch_run(settings):
    info = DistInfo(rank=0, world=1, local_rank=0, device=DEV)
    tr = Trainer(settings, info, log=lambda m: None)
    hist = tr.fit()
    d = tr.train_data
    if d.plan is not None:
        fill = tr.token_history[-1]["fill"]
    else:  # fixed batches: the timed epoch's rows and padded shapes
        n, last = d.steps_per_epoch, len(hist) - 1
        real = processed = 0
        for i in range(n):
            s, t = d.batch(last * n + i)
            real += int((s != 0).sum()) + int((t[:, 1:] != 0).sum())
            processed += s.numel() + t[:, 1:].numel()
        fill = real / processed
    out = {"steps_per_epoch": d.steps_per_epoch, "tokens_per_s": round(hist[-1].tokens_per_s),
           "fill": round(fill, 3), "real_tokens_per_s": round(hist[-1].tokens_per_s * fill),
           "cached_shapes": tr.step_fn.cached_shapes, "graph_stats": tr.step_fn.graph_stats}
    del tr
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6400)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batch-tokens", type=int, default=4096)
    ap.add_argument("--bucket", type=int, default=8)
    ap.add_argument("--graph-cache", type=int, default=256)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "corpus.tsv")
    corpus(path, args.pairs)
    st, tt = build_tokenizers(path, 7765, 7010, cache_dir=tmp)
    toks = dict(src_tokenizer=os.path.join(tmp, "tokenizer_src.json"),
                tgt_tokenizer=os.path.join(tmp, "tokenizer_tgt.json"))

    kw = dict(seed=0, bucket=args.bucket, batch_tokens=args.batch_tokens)
    host = TextPairs(path, st, tt, args.batch, pin=True, **kw)
    dev = TextPairs(path, st, tt, args.batch, corpus=DEV, **kw)
    # alternating, epoch 0 as warm-up; the best epoch of each
    times = [(assembly(host, e), assembly(dev, e)) for e in range(4)][1:]
    h_us, d_us = min(h[0] for h, _ in times), min(d[0] for _, d in times)
    nbytes = times[0][0][1]
    print(json.dumps({"part": "assembly", "pairs": len(host), "batch_tokens": args.batch_tokens,
                      "bucket": args.bucket, "batches_per_epoch": host.steps_per_epoch,
                      "mean_batch_bytes": round(nbytes), "host_us_per_batch": round(h_us, 1),
                      "device_us_per_batch": round(d_us, 1),
                      "host_over_device": round(h_us / d_us, 2)}), flush=True)
    del host, dev

    common = dict(preset="base", data="text", train_file=path, epochs=2, snapshot_every_epochs=0,
                  resume=False, hip_graph=True, log_every=10 ** 9, temporary_directory=tmp,
                  validation_file=None, graph_cache=args.graph_cache, **toks)
    runs = {"fixed": Settings(local_batch_size=args.batch, **common),
            "token_device": Settings(batch_tokens=args.batch_tokens, length_bucket=args.bucket, **common),
            "token_host": Settings(batch_tokens=args.batch_tokens, length_bucket=args.bucket,
                                   corpus_on_device=False, **common)}
    res = {name: epoch_run(s) for name, s in runs.items()}
    res["part"] = "epoch"
    res["real_tokens_per_s_token_device_over_fixed"] = round(
        res["token_device"]["real_tokens_per_s"] / res["fixed"]["real_tokens_per_s"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
