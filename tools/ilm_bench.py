"""Times the frame-synchronous search with internal-LM subtraction (ilm_weight) at the batch, frame and vocabulary
sizes of config 2 (B 32, T 1000, V 72; a 5-gram) and config 5 (B 16, T 1500, V 2048; a trigram, with and without
token_min_logp = -5).

    python tools/ilm_bench.py [--configs c2,c5] [--paths new|unchanged] [--width 16] [--rounds 5] [--tree DIR] [--tag TEXT]
                              [--out FILE]

Models, inputs and timing are tools/ngram_fusion_bench.py's: per config one model, one encoder forward shared and NOT timed,
search calls only, each timed from the call to the end of its host sync, W = --width, max_symbols 1; one warm-up call each, then
--rounds rounds that alternate the calls, median and min..max.  One JSON line each, with a digest of the returned n-best lists
(token lists and score bits), so that two trees' lines also say whether they computed the same.
  --paths new        sync (unfused) / sync_ngram (the backoff model) / sync_ngram_ilm (the same model with ilm_weight 0.3), and
                     sync_ilm (subtraction alone: the all-zero automaton); config 5 twice, "_p5" with token_min_logp = -5.
                     ratio_to_ngram = ngram_ilm / ngram.  The term is a bonus per emitted token, so with it the search emits
                     more and runs more prediction-net steps: that ratio is the feature's cost to a user, search included.
                     sync_ngram_ilm_tiny runs the ILM instance with a weight of 1e-30, too small to change a decision (its
                     digest is sync_ngram's where no fused score moves by a bit): its ratio is the kernel's own cost.
  --paths unchanged  the unfused and the dense-fused calls alone, with a bigram TokenFusion that any tree can build: the lines to
                     compare between two checkouts.  --tree DIR imports the package from another checkout (the parent commit's),
                     --tag names the tree in every line."""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ILM_WEIGHT = 0.3
TINY_WEIGHT = 1e-30


def digest(result):
    return hashlib.sha1(repr(result).encode()).hexdigest()[:12]


def bench(name, cfg, a, out):
    from rnntransducer_amd import TokenFusion, ops
    from tools.ctc_beam_bench import build
    from tools.ngram_fusion_bench import LMS, synthetic_lm
    net, audio = build(cfg)
    B, T, V, W = cfg["B"], cfg["T"], cfg["V"], a.width
    t_dev = torch.full((B,), T, dtype=torch.int32, device="cuda")
    d = net.decoder
    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_dev)
    pred = (net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias)
    sync = lambda thr, f, **kw: (lambda: ops.beam_search_sync(enc, *pred, 0, W, 1, t_dev, token_min_logp=thr, fusion=f, **kw))
    calls, info = {}, {}
    prunes = [("", -math.inf)] + ([("_p5", -5.0)] if name == "c5" else [])
    if a.paths == "unchanged":
        logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(0)), dim=1)
        dense = TokenFusion.from_bigram(logp, 0.3, 0).to("cuda")
        for sfx, thr in prunes:
            calls.update({"sync" + sfx: sync(thr, None), "sync_dense" + sfx: sync(thr, dense)})
    else:
        lm = synthetic_lm(V, **LMS[name])
        sparse = lm.to("cuda")
        info = {"order": lm.order, "n_states": lm.n_states, "n_arcs": lm.n_arcs, "ilm_weight": ILM_WEIGHT}
        for sfx, thr in prunes:
            calls.update({"sync" + sfx: sync(thr, None), "sync_ngram" + sfx: sync(thr, sparse),
                          "sync_ngram_ilm" + sfx: sync(thr, sparse, ilm_weight=ILM_WEIGHT),
                          "sync_ngram_ilm_tiny" + sfx: sync(thr, sparse, ilm_weight=TINY_WEIGHT),
                          "sync_ilm" + sfx: sync(thr, None, ilm_weight=ILM_WEIGHT)})
    times = {k: [] for k in calls}
    first = {}
    for k, f in calls.items():   # warm-up
        first[k] = f()
        torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in times:
        med = statistics.median(times[k])
        rec = {"config": name, "call": k, "B": B, "T": T, "V": V, "width": W, "rounds": len(times[k]), "ms_median": round(med, 3),
               "ms_min": round(min(times[k]), 3), "ms_max": round(max(times[k]), 3), "us_per_frame": round(med * 1e3 / T, 2),
               "digest": digest(first[k])}
        if a.tag:
            rec = {"tree": a.tag, **rec}
        if "_ngram_ilm" in k:
            rec["ratio_to_ngram"] = round(med / statistics.median(times[k.replace("_ilm_tiny", "").replace("_ilm", "")]), 3)
            rec.update(info)
            if "_tiny" in k:
                rec["ilm_weight"] = TINY_WEIGHT
        elif "sync_ilm" in k:
            rec["ratio_to_unfused"] = round(med / statistics.median(times[k.replace("sync_ilm", "sync")]), 3)
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
