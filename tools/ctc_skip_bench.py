"""What CTC-guided blank-frame skipping (csrc/ctc_skip.hip: rnnt_hip_ctc_frame_skip) costs and saves, at the batch,
frame and vocabulary sizes of config 2 (B 32, T 1000, V 72) and config 5 (B 16, T 1500, V 2048).

    python tools/ctc_skip_bench.py [--configs c2,c5] [--rounds 3] [--calls 50] [--steps 3] [--width 16] [--plain-only]
                                   [--root DIR] [--label NAME] [--out FILE]

The models are tools/ctc_beam_bench.py's (the search benchmarks' models: O = 320, one encoder forward, shared and NOT timed), ragged
batches (t_len in [T/2, T], one full row).  The CTC head is synthetic: its blank bias is set from the quantiles of
logsumexp(non-blank logits) - blank logit over the valid frames so that a threshold of p = 0.9 skips about 50 % / about 75 % of them.

  pass      rnnt_hip_ctc_frame_skip alone, HIP events around windows of --calls calls, next to the bytes it must move (the valid
            frames' logits read, the kept rows read and written, the map and lengths written) and that as a share of 6.29 TB/s, the
            float4-copy rate of the HBM
  search    ops.greedy_decode (max_iters 3), ops.beam_search_sync (W = --width, max_symbols 1) and ops.beam_search (beam = --width,
            improved) on the encoder output, against ctc_head + ctc_frame_skip + the same search at the two skip shares: what
            JointNet.recognize_*(ctc_skip=) runs behind the encoder.  Host clock from the call to the end of its host sync, calls
            alternating, median and min..max of --rounds rounds
  mwer      a training step of RNNTransducer with args.mwer_weight (N = 4) with and without args.mwer_ctc_skip, and the plain
            training step of the same model; windows of --steps steps between device synchronises, alternating.  The joint is
            sharpened as tools/mwer_bench.py does and its blank bias is --blank-bias plus the one of 0, 2, .. 12 whose 1-best
            hypotheses come closest to U tokens (reported as `mwer_calibration`)
  --plain-only   the plain calls alone (no ctc_skip anywhere), which also run on a checkout of the parent commit given as --root:
            the package is then imported from DIR
One JSON line per measurement (appended to --out)."""
import argparse
import json
import math
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

HBM_COPY_RATE = 6.29e12   # bytes/s, float4 copy
P = 0.9


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def ragged(B, T, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()


def set_skip_share(head, enc, valid, share):
    """bias[blank] so that p = P skips `share` of the valid frames: a frame is skipped when gap < bias - logit(P), gap =
    logsumexp(non-blank logits) - blank logit at bias 0."""
    with torch.no_grad():
        head.bias[0] = 0.0
        z = head(enc).double().transpose(0, 1)
        gap = (torch.logsumexp(z[..., 1:], -1) - z[..., 0])[valid]
        head.bias[0] = float(torch.quantile(gap, share)) + math.log(P / (1 - P))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def bench_searches(name, cfg, a):
    from rnntransducer_amd import ops
    from tools.ctc_beam_bench import build
    net, audio = build(cfg)
    B, T, V = cfg["B"], cfg["T"], cfg["V"]
    t_list = ragged(B, T)
    t_dev = torch.tensor(t_list, dtype=torch.int32, device="cuda")
    valid = torch.arange(T, device="cuda")[None, :] < t_dev[:, None]
    d = net.decoder
    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_dev)
    O = enc.shape[2]
    pred = (net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias)
    searches = {"greedy": lambda e, t: ops.greedy_decode(e, *pred, 0, 3, t)[1].tolist(),
                "beams_sync": lambda e, t: ops.beam_search_sync(e, *pred, 0, a.width, 1, t),
                "beams": lambda e, t: ops.beam_search(e, *pred, 0, a.width, True, t_lens=t)}
    base = {"config": name, "label": a.label, "B": B, "T": T, "V": V, "O": O, "valid_frames": int(valid.sum()), "width": a.width}
    shares = () if a.plain_only else (0.5, 0.75)

    def skipped(share):
        with torch.no_grad():
            return ops.ctc_frame_skip(net.ctc_head(enc), t_dev, 0, P, enc)

    # the pass alone
    for share in shares:
        set_skip_share(net.ctc_head, enc, valid, share)
        with torch.no_grad():
            z = net.ctc_head(enc)
        sk = ops.ctc_frame_skip(z, t_dev, 0, P, enc)
        kept = int(sk.t_lens.sum())
        nbytes = 4 * (int(valid.sum()) * V + 2 * kept * O + B * T + B)
        for _ in range(5):
            ops.ctc_frame_skip(z, t_dev, 0, P, enc)
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.ctc_frame_skip(z, t_dev, 0, P, enc)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        med = statistics.median(us)
        emit({**base, "section": "pass", "skip_share": round(1 - kept / int(valid.sum()), 4), "kept_frames": kept, "bytes": nbytes,
              "us_per_call_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
              "floor_us_at_hbm_copy_rate": round(nbytes / HBM_COPY_RATE * 1e6, 2), "share_of_hbm_copy_rate": round(nbytes / HBM_COPY_RATE / (med * 1e-6), 4),
              "timing": f"HIP events around windows of {a.calls} calls (two launches and four torch.empty each), {a.rounds} windows"}, a.out)
    # the searches
    calls = {}
    for k, f in searches.items():
        calls[k, None] = (lambda f=f: f(enc, t_dev))
        for share in shares:
            def with_skip(f=f, share=share):
                sk = skipped(share)
                return f(sk.enc, sk.t_lens)
            calls[k, share] = with_skip
    from rnntransducer_amd._lib import RnntHipError
    times, realised, dead = {c: [] for c in calls}, {}, {}
    for r in range(a.rounds + 1):   # round 0 warms up
        for (k, share), f in calls.items():
            if share is not None:
                set_skip_share(net.ctc_head, enc, valid, share)
                realised[share] = round(1 - int(skipped(share).t_lens.sum()) / int(valid.sum()), 4)
            if k in dead:
                continue
            try:
                ms = timed(f)
            except RnntHipError as e:   # a search that outgrows one of its caps on this synthetic model: reported, not timed
                dead[k] = str(e)[:160]
                continue
            if r:
                times[k, share].append(ms)
    for k, why in dead.items():
        emit({**base, "section": "search", "call": k, "skipped": why}, a.out)
    for (k, share), ms in times.items():
        if k in dead:
            continue
        rec = {**base, "section": "search", "call": k, "ctc_skip": None if share is None else P,
               "skip_share": None if share is None else realised[share], **stats(ms)}
        if share is not None:
            rec["ratio_to_plain"] = round(statistics.median(ms) / statistics.median(times[k, None]), 4)
        emit(rec, a.out)


def bench_mwer(name, cfg, a):
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd.data import synthetic_batch
    B, T, V, U = cfg["B"], cfg["T"], cfg["V"], {"c2": 40, "c5": 80}[name]
    batch = synthetic_batch(B, T, U, V, seed=1234, device="cuda", t_lengths=ragged(B, T))
    tn = dict(input_size=80, hidden_size=256, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=cfg["H"], output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0)

    def build(extra_bias=0.0, **kw):
        args = Namespace(learning_rate=0.0, weight_decay=0.0, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10000,
                         move_metrics_to_cpu=False, **kw)
        torch.manual_seed(0)
        model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V, aux_ctc=True), args)
        with torch.no_grad():   # tools/mwer_bench.py's sharpening, and a blank bias that keeps the hypotheses near U tokens
            for n, p in model.jointnet.named_parameters():
                if not n.startswith("ctc_head."):
                    p.mul_(6.0 if n.startswith("fc.") else 3.0)
            model.jointnet.decoder.embedding.weight[0].zero_()
            model.jointnet.fc.bias[0] += a.blank_bias + extra_bias
        model = model.cuda().train()
        return model, model.configure_optimizers()["optimizer"]

    sides = {"plain_step": build(), "mwer": build(mwer_weight=0.5, mwer_nbest=4)}
    # the blank bias of the joint, calibrated as tools/mwer_bench.py does: the 1-best hypotheses closest to U tokens on average
    from rnntransducer_amd.ops import beam_search_sync_device
    jn = sides["mwer"][0].jointnet
    d, fit = jn.decoder, {}
    with torch.no_grad():
        enc = jn.encoder.forward_time_major(batch[0], batch[2])
        base_bias = float(jn.fc.bias[0])
        for bias in range(0, 13, 2):
            jn.fc.bias[0] = base_bias + bias
            host = beam_search_sync_device(enc, jn.fc.weight, jn.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL,
                                           d.out_proj.weight, d.out_proj.bias, 0, 4, 1, batch[2])[4]
            fit[bias] = float(host[B:].reshape(B, 4)[:, 0].float().mean()) - 1
        jn.fc.bias[0] = base_bias
    best = min(fit, key=lambda b: abs(fit[b] - U))
    emit({"config": name, "label": a.label, "section": "mwer_calibration", "tokens_in_best_by_bias": fit, "bias": best}, a.out)
    sides = {"plain_step": build(best), "mwer": build(best, mwer_weight=0.5, mwer_nbest=4)}
    if not a.plain_only:
        for share in (0.5, 0.75):
            sides[f"mwer_skip_{share}"] = build(best, mwer_weight=0.5, mwer_nbest=4, mwer_ctc_skip=P)
            m = sides[f"mwer_skip_{share}"][0]
            t_dev = batch[2]
            valid = torch.arange(T, device="cuda")[None, :] < t_dev[:, None]
            with torch.no_grad():
                enc = m.jointnet.encoder.forward_time_major(batch[0], t_dev)
            set_skip_share(m.jointnet.ctc_head, enc, valid, share)

    def window(side, n):
        model, opt = sides[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            opt.zero_grad()
            loss = model.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(loss.detach())

    ms, last = {s: [] for s in sides}, {}
    for r in range(a.rounds + 1):   # round 0 warms up
        for s in sides:
            t, last[s] = window(s, a.steps if r else 2)
            if r:
                ms[s].append(t)
    for s in sides:
        rec = {"config": name, "label": a.label, "section": "mwer", "side": s, "B": B, "T": T, "U": U, "V": V, "nbest": 4,
               "steps_per_window": a.steps, **stats(ms[s]), "last_loss": round(last[s], 4)}
        if s.startswith("mwer_skip"):
            rec["ratio_to_mwer"] = round(statistics.median(ms[s]) / statistics.median(ms["mwer"]), 4)
        emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--blank-bias", type=float, default=6.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--skip-mwer", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = os.path.abspath(a.out) if a.out else None
    sys.path.insert(0, os.path.abspath(a.root))
    os.chdir(a.root)
    if not torch.cuda.is_available():
        raise SystemExit("ctc_skip_bench needs the GPU: there is nothing to time without it")
    from tools.ctc_beam_bench import CONFIGS
    for name in a.configs.split(","):
        bench_searches(name, CONFIGS[name], a)
        if not a.skip_mwer:
            bench_mwer(name, CONFIGS[name], a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
