"""Times the searches that take a backoff n-gram model (NgramFusion) at the batch, frame and vocabulary sizes of config 2 (B 32,
T 1000, V 72; a 5-gram) and config 5 (B 16, T 1500, V 2048; a trigram, with and without token_min_logp = -5).

    python tools/ngram_fusion_bench.py [--configs c2,c5] [--paths new|unchanged] [--width 16] [--rounds 5] [--tree DIR] [--tag TEXT]
                                       [--out FILE]

Per config one model (tools/ctc_beam_bench.py's: one encoder forward, shared and NOT timed) and search calls only, each timed
from the call to the end of its host sync, W = --width, max_symbols 1:
  --paths new        the backoff policy beside the dense policy ON THE SAME AUTOMATON (lm.to_dense()) and beside the unfused
                     search: sync / sync_dense / sync_ngram (ops.beam_search_sync) and ctc / ctc_dense / ctc_ngram
                     (ops.ctc_beam_search); config 5 twice, "_p5" with token_min_logp = -5.  ratio_to_dense = ngram / dense.
  --paths unchanged  the unfused and the dense-fused calls alone, with a bigram TokenFusion that any tree can build: the lines to
                     compare between two checkouts.  --tree DIR imports the package from another checkout (the parent commit's),
                     --tag names the tree in every line.
The models are synthetic (seeded random n-grams; the automaton's cost does not depend on the numbers): every unigram, then per
order random extensions of the listed n-grams one shorter, so every context is listed and lists a handful of successors.
Timing: one warm-up call each, then --rounds rounds that alternate the calls, median and min..max.  One JSON line each."""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# per config: the model's order and how many n-grams of each order above 1 it lists
LMS = {"c2": dict(order=5, per_order=20000), "c5": dict(order=3, per_order=8000)}


def synthetic_lm(V, order, per_order, seed=0, weight=0.3):
    from rnntransducer_amd import NgramFusion
    r = random.Random(seed)
    p, b = (lambda: r.uniform(-6.0, -0.5)), (lambda: r.uniform(-1.5, 0.0))
    ng = {(k,): (p(), b()) for k in range(1, V)}
    ng[(NgramFusion.BOS,)] = (-99.0, b())
    ng[(NgramFusion.EOS,)] = (p(), None)
    level = [g for g in ng if g != (NgramFusion.EOS,)]
    for n in range(2, order + 1):
        nxt = {}
        want = min(per_order, len(level) * (V - 1) // 2)   # (V = 72 has fewer bigrams than that)
        while len(nxt) < want:
            nxt.setdefault(r.choice(level) + (r.randrange(1, V),), (p(), b() if n < order else None))
        ng.update(nxt)
        level = list(nxt)
    return NgramFusion.from_ngrams(ng, V, weight, 0, oov_logp=-10.0)


def bench(name, cfg, a, out):
    from rnntransducer_amd import TokenFusion, ops
    from tools.ctc_beam_bench import build
    net, audio = build(cfg)
    B, T, V, W = cfg["B"], cfg["T"], cfg["V"], a.width
    t_dev = torch.full((B,), T, dtype=torch.int32, device="cuda")
    d = net.decoder
    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_dev)
        z = net.ctc_head(enc)
        z = (z - z.mean(-1, keepdim=True)) * (4.0 / z.std(-1, keepdim=True))
    pred = (net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias)
    sync = lambda thr, f: (lambda: ops.beam_search_sync(enc, *pred, 0, W, 1, t_dev, token_min_logp=thr, fusion=f))
    ctc = lambda thr, f: (lambda: ops.ctc_beam_search(z, t_dev, 0, W, time_major=True, token_min_logp=thr, fusion=f))
    calls, info = {}, {}
    prunes = [("", -math.inf)] + ([("_p5", -5.0)] if name == "c5" else [])
    if a.paths == "unchanged":
        logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(0)), dim=1)
        dense = TokenFusion.from_bigram(logp, 0.3, 0).to("cuda")
        for sfx, thr in prunes:
            calls.update({"sync" + sfx: sync(thr, None), "sync_dense" + sfx: sync(thr, dense),
                          "ctc" + sfx: ctc(thr, None), "ctc_dense" + sfx: ctc(thr, dense)})
    else:
        lm = synthetic_lm(V, **LMS[name])
        dense, sparse = lm.to_dense().to("cuda"), lm.to("cuda")
        info = {"order": lm.order, "n_states": lm.n_states, "n_arcs": lm.n_arcs}
        for sfx, thr in prunes:
            calls.update({"sync" + sfx: sync(thr, None), "sync_dense" + sfx: sync(thr, dense), "sync_ngram" + sfx: sync(thr, sparse),
                          "ctc" + sfx: ctc(thr, None), "ctc_dense" + sfx: ctc(thr, dense), "ctc_ngram" + sfx: ctc(thr, sparse)})
    times = {k: [] for k in calls}
    same = {}
    for k, f in calls.items():   # warm-up; the backoff policy must return what the dense policy returns
        same[k] = f()
        torch.cuda.synchronize()
    for k in calls:
        if "_ngram" in k and same[k] != same[k.replace("_ngram", "_dense")]:
            raise SystemExit(f"{name} {k}: the backoff and the dense policy disagree")
    for _ in range(a.rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in times:
        med = statistics.median(times[k])
        rec = {"config": name, "call": k, "B": B, "T": T, "V": V, "width": W, "rounds": len(times[k]), "ms_median": round(med, 3),
               "ms_min": round(min(times[k]), 3), "ms_max": round(max(times[k]), 3), "us_per_frame": round(med * 1e3 / T, 2)}
        if a.tag:
            rec = {"tree": a.tag, **rec}
        if "_ngram" in k:
            rec["ratio_to_dense"] = round(med / statistics.median(times[k.replace("_ngram", "_dense")]), 3)
            rec["ratio_to_unfused"] = round(med / statistics.median(times[k.replace("_ngram", "")]), 3)
            rec.update(info)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--paths", choices=("new", "unchanged"), default="new")
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from tools.ctc_beam_bench import CONFIGS
    out = open(a.out, "a") if a.out else None
    for name in a.configs.split(","):
        bench(name, CONFIGS[name], a, out)


if __name__ == "__main__":
    main()
