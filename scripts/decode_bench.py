"""Decoding throughput: greedy_cached vs beam_search(beam=1) vs beam_search(beam=4).

    python scripts/decode_bench.py [--repeats 7] [--kernels]

`base` preset, random weights, B 64 sentences of S 64 source tokens,
max_length 64; [END] is masked out of the logits (its output bias is -1e4) so
every run decodes all 64 tokens. After a warm-up of each, the three variants
run interleaved in one process; reported per variant: the median over the
repeats of generated tokens / s (B * 64 tokens per run, whatever the beam) and
the spread (min .. max), with every repeat's time. --kernels adds the per-launch times of the attention
and selection kernels of one step at mid length (beam_topk, and sample_token on the same rows: plain
and with top-k and top-p, which add a 16-pass bisection each). Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensorflow_distributed_on_gke_amd.infer.beam import beam_search  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops import kernels as K  # noqa: E402

B, S, MAXLEN = 64, 64, 64


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _launch_us(fn, iters=100):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 2)


def kernel_times(cfg, dev):
    """us per launch (back-to-back, so launch-bound kernels show the launch
    rate) of one layer's attention work at step t = 32, and of the selection."""
    H, hd, T, t = cfg.heads, cfg.d_model // cfg.heads, MAXLEN + 1, 32
    bf = dict(dtype=torch.bfloat16, device=dev)
    out = {}
    for beam in (1, 4):
        R = B * beam
        qkv = torch.randn(R, 3, H, hd, **bf)
        kc, vc = torch.randn(R, T, H, hd, **bf), torch.randn(R, T, H, hd, **bf)
        kv = torch.randn(B, S, 2, H, hd, **bf)
        klen = torch.full((R,), t + 1, dtype=torch.int32, device=dev)
        slen = torch.full((R,), S, dtype=torch.int32, device=dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)
        anc = rows.view(R, 1).repeat(1, T).contiguous()
        rmap = (rows // beam).to(torch.int32)
        lg = torch.randn(R, 7040, **bf)
        score = torch.zeros(R, device=dev)
        fin = torch.zeros(R, dtype=torch.int32, device=dev)
        o = out[f"beam{beam}"] = {}
        o["decode_attn_self_fused_us"] = _launch_us(lambda: K.decode_attn(
            qkv[:, 0], kc, vc, klen, 0.125, anc=anc, k_new=qkv[:, 1], v_new=qkv[:, 2]))
        o["decode_attn_cross_us"] = _launch_us(lambda: K.decode_attn(
            qkv[:, 0], kv[:, :, 0], kv[:, :, 1], slen, 0.125, row_map=rmap))
        o["beam_topk_us"] = _launch_us(lambda: K.beam_topk(lg, 7010, score, fin, beam, END, 0, anc=anc,
                                                           t=t, anc_out=torch.empty_like(anc)))
        for name, kw in (("sample_token_us", dict()),
                         ("sample_token_topk_topp_us", dict(temperature=0.8, top_k=40, top_p=0.9))):
            o[name] = _launch_us(lambda: K.sample_token(lg, 7010, score, fin, END, 0, seed=1, step=t,
                                                        row_id=rows, **kw))
        if beam == 1:
            q4 = qkv.view(R, 1, 3, H, hd)

            def greedy_self():
                kc[:, t] = q4[:, 0, 1]
                vc[:, t] = q4[:, 0, 2]
                K.attn_fwd(q4[:, :, 0], kc[:, : t + 1], vc[:, : t + 1], klen, 0.125, False)

            o["greedy_self_2copies_attn_fwd_us"] = _launch_us(greedy_self)
            o["greedy_cross_attn_fwd_us"] = _launch_us(lambda: K.attn_fwd(
                q4[:, :, 0], kv[:, :, 0], kv[:, :, 1], slen, 0.125, False))
            o["greedy_argmax_us"] = _launch_us(lambda: lg[:, :7010].float().argmax(dim=-1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    dev = "cuda:0"
    cfg = model_config("base")
    m = Transformer(cfg).build(dev, seed=0)
    m.final.b.master[END] = -1e4  # never [END]: all MAXLEN tokens are decoded
    tester = Tester(ByteTokenizer(min(cfg.src_vocab, cfg.tgt_vocab)), m)
    g = torch.Generator().manual_seed(0)
    src = torch.randint(4, cfg.src_vocab, (B, S), generator=g)
    src[:, 0], src[:, -1] = START, END
    variants = {
        "greedy_cached": lambda: tester.greedy_cached(src, MAXLEN),
        "beam1": lambda: beam_search(m, src, START, END, beam=1, max_length=MAXLEN)[0],
        "beam4": lambda: beam_search(m, src, START, END, beam=4, max_length=MAXLEN)[0],
    }
    for name, fn in variants.items():  # warm-up
        for _ in range(2):
            _, out = _timed(fn)
        assert out.shape == (B, MAXLEN + 1), (name, tuple(out.shape))
    times = {name: [] for name in variants}
    for _ in range(args.repeats):  # interleaved
        for name, fn in variants.items():
            times[name].append(_timed(fn)[0])
    res = {"B": B, "S": S, "max_length": MAXLEN, "repeats": args.repeats}
    for name, ts in times.items():
        tps = sorted(B * MAXLEN / x for x in ts)
        res[name] = {"tokens_per_s_median": round(statistics.median(tps), 1),
                     "tokens_per_s_min": round(tps[0], 1), "tokens_per_s_max": round(tps[-1], 1),
                     "ms_per_run_median": round(statistics.median(ts) * 1e3, 2),
                     "ms_per_run": [round(x * 1e3, 2) for x in ts]}
    if args.kernels:
        res["kernels"] = kernel_times(cfg, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
