"""Times the frame-synchronous transducer beam search against the other decodes, at the batch, frame and vocabulary sizes of
config 2 (B 32, T 1000, V 72) and config 5 (B 16, T 1500, V 2048).

    python tools/beam_sync_bench.py [--configs c2,c5] [--width 16] [--rounds 5] [--out profiles/beam_sync_bench.txt]

Per config one model (aux_ctc=True, one encoder forward, shared and NOT timed: it is common to all decodes) and the search calls
on its outputs, each timed from the call to the end of its host sync:
    sync_s1 / sync_s3   ops.beam_search_sync, W = --width, max_symbols 1 / 3            (what recognize_beams_sync launches;
                        config 5: max_symbols 1 only)
    rnnt_beam           ops.beam_search, beam = --width, improved                        (what recognize_beams launches; a search
                        that outgrows one of its caps on this synthetic model is recorded as it behaves: skipped, with the message)
    ctc_beam            ops.ctc_beam_search, W = --width, on the CTC head's logits       (rescaled as tools/ctc_beam_bench.py does)
    greedy              ops.greedy_decode, max_iters 3
Timing: one warm-up call each, then --rounds rounds that alternate the calls (so drift of the clocks hits all alike), median and
min..max per call, and for the new search the ratio to rnnt_beam.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tools.ctc_beam_bench import CONFIGS, build   # noqa: E402  (the same models and inputs)


def bench(name, cfg, width, rounds, out):
    from rnntransducer_amd import ops
    from rnntransducer_amd._lib import RnntHipError
    net, audio = build(cfg)
    B, T, V = cfg["B"], cfg["T"], cfg["V"]
    t_dev = torch.full((B,), T, dtype=torch.int32, device="cuda")
    d = net.decoder
    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_dev)
        z = net.ctc_head(enc)
        z = (z - z.mean(-1, keepdim=True)) * (4.0 / z.std(-1, keepdim=True))
    pred = (net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias)
    calls = {"sync_s1": lambda: ops.beam_search_sync(enc, *pred, 0, width, 1, t_dev)}
    if name == "c2":
        calls["sync_s3"] = lambda: ops.beam_search_sync(enc, *pred, 0, width, 3, t_dev)
    calls["rnnt_beam"] = lambda: ops.beam_search(enc, *pred, 0, width, True, t_lens=t_dev)
    calls["ctc_beam"] = lambda: ops.ctc_beam_search(z, t_dev, 0, width, time_major=True)
    calls["greedy"] = lambda: ops.greedy_decode(enc, *pred, 0, 3, t_dev)[1].tolist()
    times = {k: [] for k in calls}
    info, slow = {}, set()
    for k, f in list(calls.items()):   # warm-up; a search that outgrows a cap is reported, not timed
        try:
            t0 = time.perf_counter()
            res = f()
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > 20.0:   # a call of tens of seconds is timed in the first round only
                slow.add(k)
        except RnntHipError as e:
            info[k] = {"skipped": str(e)[:160]}
            del calls[k]
            continue
        if k.startswith("sync"):
            info[k] = {"hyps_per_utt": round(sum(len(h) for h in res) / B, 1), "tokens_in_best": round(sum(len(h[0][0]) - 1 for h in res) / B, 1)}
        elif k == "rnnt_beam":
            info[k] = {"tokens_in_best": round(sum(len(h[0][0]) - 1 for h in res) / B, 1)}
        elif k == "greedy":
            info[k] = {"tokens": round(sum(res) / B, 1)}
    for i in range(rounds):
        for k, f in calls.items():
            if i > 0 and k in slow:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ref = statistics.median(times["rnnt_beam"]) if times.get("rnnt_beam") else None
    for k in times:
        rec = {"config": name, "call": k, "B": B, "T": T, "V": V, "width": width, "rounds": len(times[k])}
        if times[k]:
            med = statistics.median(times[k])
            rec.update(ms_median=round(med, 3), ms_min=round(min(times[k]), 3), ms_max=round(max(times[k]), 3),
                       us_per_frame=round(med * 1e3 / T, 2))
            if k.startswith("sync") and ref:
                rec["ratio_to_rnnt_beam"] = round(med / ref, 3)
        rec.update(info.get(k, {}))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None
    for name in a.configs.split(","):
        bench(name, CONFIGS[name], a.width, a.rounds, out)


if __name__ == "__main__":
    main()
