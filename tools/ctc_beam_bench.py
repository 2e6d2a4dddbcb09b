"""Times the encoder-only decodes through the CTC head against each other and against the transducer's beam search, at the batch,
frame and vocabulary sizes of config 2 (B 32, T 1000, V 72) and config 5 (B 16, T 1500, V 2048).

    python tools/ctc_beam_bench.py [--configs c2,c5] [--width 16] [--rounds 5] [--out profiles/ctc_beam_bench.txt]

Per config one model (aux_ctc=True, one encoder forward, shared and NOT timed: it is common to all four decodes) and four search
calls on its outputs, each timed from the call to the end of its host sync:
    ctc_beam          ops.ctc_beam_search, W = --width, token_min_logp = -inf      (what recognize_ctc_beams launches)
    ctc_beam_pruned   the same with token_min_logp = -5
    ctc_greedy        ops.ctc_greedy                                               (what recognize_ctc_greedy launches)
    rnnt_beam         ops.beam_search, beam = --width, improved                    (what recognize_beams launches; a search
                      that outgrows one of its caps on this synthetic model is reported as skipped, with the message)
The head's logits of an untrained model are nearly uniform, which no decode ever sees; they are rescaled to a standard deviation
of 4 per frame (a confident but not one-hot acoustic model).  Timing: one warm-up call each, then --rounds rounds that alternate
the four calls (so drift of the clocks hits all alike), median and min..max per call.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CONFIGS = {"c2": dict(B=32, T=1000, V=72, H=512), "c5": dict(B=16, T=1500, V=2048, H=512)}


def build(cfg):
    from rnntransducer_amd.networks import JointNet
    V, H = cfg["V"], cfg["H"]
    tn = dict(input_size=80, hidden_size=256, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=H, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(0)
    net = JointNet(dict(tn), dict(pn), V, aux_ctc=True)
    with torch.no_grad():   # tools/beam_bench.py's contrast for the joint
        for n, p in net.named_parameters():
            p.mul_(4.0 if n.startswith("fc.") else 2.0)
        net.decoder.embedding.weight[0].zero_()
    return net.cuda().eval(), torch.randn(cfg["B"], cfg["T"], 80).cuda()


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
    calls = {
        "ctc_beam": lambda: ops.ctc_beam_search(z, t_dev, 0, width, time_major=True),
        "ctc_beam_pruned": lambda: ops.ctc_beam_search(z, t_dev, 0, width, token_min_logp=-5.0, time_major=True),
        "ctc_greedy": lambda: ops.ctc_greedy(z, t_dev, 0, time_major=True),
        "rnnt_beam": lambda: ops.beam_search(enc, net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL,
                                             d.out_proj.weight, d.out_proj.bias, 0, width, True, t_lens=t_dev),
    }
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
        if k.startswith("ctc_beam"):
            info[k] = {"hyps_per_utt": round(sum(len(h) for h in res) / B, 1), "tokens_in_best": round(sum(len(h[0][0]) for h in res) / B, 1)}
        elif k == "ctc_greedy":
            info[k] = {"tokens": round(sum(len(y) for y in res) / B, 1)}
    for i in range(rounds):
        for k, f in calls.items():
            if i > 0 and k in slow:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in times:
        rec = {"config": name, "call": k, "B": B, "T": T, "V": V, "width": width, "rounds": len(times[k])}
        if times[k]:
            med = statistics.median(times[k])
            rec.update(ms_median=round(med, 3), ms_min=round(min(times[k]), 3), ms_max=round(max(times[k]), 3),
                       us_per_frame=round(med * 1e3 / T, 2))
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
