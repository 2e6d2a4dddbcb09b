"""Times an MWER training step (RNNTransducer with args.mwer_weight > 0: JointNet.mwer_loss) against the plain
training step of the same build, at BASELINE config-2 sizes with N = 4 hypotheses, and the parts MWER adds.

    python tools/mwer_bench.py [--config c2] [--nbest 4] [--max-symbols 1] [--steps 5] [--rounds 3] [--calls 10] [--out FILE]

A freshly initialised model is all but uniform over the vocabulary: its hypotheses emit a token in every frame (T tokens, beyond
the 511 the loss takes) or, with a bias on the blank, none.  So the model is sharpened as the search tests sharpen theirs (every
parameter x 3, fc x 6) and the blank's bias is CALIBRATED here: of the biases 0, 1, .. 12 the one whose n-best hypotheses are
closest to U tokens long on average is used — hypotheses about as long as the transcripts, as a converged model gives them.
Both models (plain and MWER) carry the same weights.

Hypotheses longer than --max-hyp-len (default 2 U) are left out, as a training run would cap them.
Steps: zero_grad, training_step (MWER side: its JointNet.mwer_loss call, with that cap), backward, FlatAdamW step at learning rate 0
(the update kernel runs, the calibrated model stays as it is); `rounds` alternating windows of `steps` steps
each between HIP events, median and spread (max - min) per step.  Parts, `calls` calls each, on the step's own tensors: the time
between HIP events around the part (everything it launches, torch's index kernels included) and the library profiler's sum over its
kernel kinds (rnnt_hip_prof_*: the launches the library brackets itself).  Prints one JSON line (appended to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c1": (2, 100, 20, 72, (128, 1), (128, 1), 128), "c2": (32, 1000, 40, 72, (512, 4), (512, 1), 512)}   # bench.py's


def build(cfg, scale, blank_bias, **kw):
    from rnntransducer_amd import RNNTransducer
    B, T, U, V, (He, Le), (Hp, Lp), O = cfg
    tn = dict(input_size=80, hidden_size=He, output_size=O, num_layers=Le, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=Hp, output_size=O, num_layers=Lp, rnn_type="lstm", dropout=0.0)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10000,
                     move_metrics_to_cpu=False, **kw)
    torch.manual_seed(0)
    model = RNNTransducer(pn, tn, dict(num_classes=V), args)
    with torch.no_grad():
        for n, p in model.jointnet.named_parameters():
            p.mul_(2.0 * scale if n.startswith("fc.") else scale)
        model.jointnet.decoder.embedding.weight[0].zero_()
        model.jointnet.fc.bias[0] += blank_bias
    return model.cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=list(CONFIGS))
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--max-symbols", type=int, default=1)
    ap.add_argument("--mwer-weight", type=float, default=0.5)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--max-hyp-len", type=int, default=0, help="hypotheses longer than this are left out (0: 2 U)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mwer_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd import _lib, ops
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.data import synthetic_batch
    lib = _lib.lib()
    nk = len(_lib.KERNEL_KINDS)
    cfg = CONFIGS[a.config]
    B, T, U, V = cfg[:4]
    N, S = a.nbest, a.max_symbols
    max_hyp_len = a.max_hyp_len or 2 * U
    batch = synthetic_batch(B, T, U, V, ragged=True, seed=1234, device="cuda")
    audio, t_lens, targets, u_lens = batch[0], batch[2], batch[5], batch[6]

    def search_of(net, enc):
        dec = net.decoder
        return ops.beam_search_sync_device(enc, net.fc.weight, net.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                                           dec.out_proj.weight, dec.out_proj.bias, 0, N, S, t_lens)

    def mean_len(host):
        counts, lens = host[:B].tolist(), host[B:].reshape(B, N).tolist()
        got = [lens[b][n] - 1 for b in range(B) for n in range(counts[b])]
        return sum(got) / len(got), max(got)

    # calibrate the blank's bias on the sharpened model (the encoder output does not depend on it)
    probe = build(cfg, a.scale, 0.0)
    with torch.no_grad():
        enc = probe.jointnet.encoder.forward_time_major(audio, t_lens)
        trials = {}
        for bias in range(13):
            probe.jointnet.fc.bias[0] += (1.0 if bias else 0.0)
            trials[bias] = mean_len(search_of(probe.jointnet, enc)[4])
    bias = min(trials, key=lambda k: abs(trials[k][0] - U))
    del probe
    plain = build(cfg, a.scale, float(bias))
    mwer = build(cfg, a.scale, float(bias), mwer_weight=a.mwer_weight, mwer_nbest=N, mwer_max_symbols=S)
    sides = {}
    for name, model in (("plain", plain), ("mwer", mwer)):
        opt = model.configure_optimizers()["optimizer"]
        for group in opt.param_groups:   # the update runs, at learning rate 0: every timed step sees the calibrated model
            group["lr"] = 0.0

        def step(model=model, opt=opt, name=name):
            opt.zero_grad()
            if name == "plain":
                loss = model.training_step(batch, 0)["loss"]
            else:   # training_step's call, with the length cap (training_step itself leaves it at 511)
                loss = model.jointnet.mwer_loss(audio, t_lens, batch[3], targets, u_lens, 0, nbest=N, max_symbols=S,
                                                mwer_weight=a.mwer_weight, reduction="mean", audio_lengths=batch[1],
                                                max_hyp_len=max_hyp_len)
            loss.backward()
            opt.step()
            return loss.detach()
        sides[name] = step

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, out

    losses = {}
    for name, step in sides.items():
        for _ in range(2):
            losses[name] = float(step())
    times = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, step in sides.items():
            times[name].append(timed(step, a.steps)[0])

    # the parts, on the MWER model's own tensors
    net = mwer.jointnet
    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_lens)
    tokens, lens, counts, _, host = search_of(net, enc)
    Umax = ops.nbest_umax(host, B, N, max_hyp_len)
    texts, labels, hu, ht, valid = ops.nbest_pack(tokens, lens, counts, t_lens, Umax, 0, max_hyp_len)
    gvec = torch.full((B * N,), 1.0 / (B * N), device="cuda")

    def grouped():
        e = enc.detach().requires_grad_()
        hdec = net.decoder.forward_time_major(texts, hu + 1)
        nll = ops.JointLossGroupedFn.apply(e, hdec, net.fc.weight, net.fc.bias, labels, ht, hu, 0, N, True)
        nll.backward(gvec)
        return nll.detach()
    nll = grouped()
    dist = ops.edit_distance(labels, hu, targets, u_lens, N)
    A = torch.empty(enc.shape[0], B, V, device="cuda")
    rows = torch.arange(B * N, device="cuda") // N
    dAx = torch.empty(enc.shape[0], B * N, V, device="cuda")

    def group_sum():
        g = dAx.view(-1, B, N, V)
        out = g[:, :, 0].contiguous()
        for n in range(1, N):
            out.add_(g[:, :, n])
        return out
    parts = {"search": lambda: search_of(net, enc), "nbest_pack": lambda: ops.nbest_pack(tokens, lens, counts, t_lens, Umax, 0, max_hyp_len),
             "prednet_and_grouped_loss_fwd_bwd": grouped, "edit_distance": lambda: ops.edit_distance(labels, hu, targets, u_lens, N),
             "mwer_risk": lambda: ops.MwerRiskFn.apply(nll, dist, valid, N, "mean"),
             "gather_A": lambda: A.index_select(1, rows), "group_sum_dA": group_sum}
    part_ms = {}
    for name, fn in parts.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        lib.rnnt_hip_prof_enable(1)
        for _ in range(a.calls):
            fn()
        lib.rnnt_hip_prof_enable(0)
        ms, work, cnt = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
        torch.cuda.synchronize()
        ops.check(lib.rnnt_hip_prof_collect(ms, work, cnt, nk), "rnnt_hip_prof_collect")
        part_ms[name] = {"events_ms": round(timed(fn, a.calls)[0], 4), "library_profiler_ms": round(sum(ms) / a.calls, 4),
                         "library_launches": int(sum(cnt)) // a.calls}
    med = {k: statistics.median(v) for k, v in times.items()}
    nvalid = int(valid.sum())
    rec = {"config": a.config, "B": B, "T": T, "U": U, "V": V, "nbest": N, "max_symbols": S, "scale": a.scale, "blank_bias": bias,
           "hyp_len_mean_max_by_bias": {str(k): [round(v[0], 1), v[1]] for k, v in trials.items()},
           "max_hyp_len": max_hyp_len, "hyp_rows": B * N, "hyp_rows_valid": nvalid, "Umax": Umax,
           "hyp_len_mean_valid": round(float(hu.sum()) / max(nvalid, 1), 1),
           "mean_1best_edit_distance": round(float(dist.view(B, N)[:, 0].float().mean()), 2),
           "plain_step_ms": round(med["plain"], 3), "plain_step_spread_ms": round(max(times["plain"]) - min(times["plain"]), 3),
           "mwer_step_ms": round(med["mwer"], 3), "mwer_step_spread_ms": round(max(times["mwer"]) - min(times["mwer"]), 3),
           "mwer_over_plain": round(med["mwer"] / med["plain"], 4), "loss_plain": losses["plain"], "loss_mwer": losses["mwer"],
           "parts": part_ms, "steps": a.steps, "rounds": a.rounds, "calls": a.calls,
           "timing": "steps: HIP events around windows of `steps` steps, alternating sides, median per step; parts: HIP events around "
                     "`calls` calls, and the library profiler's sum over kernel kinds for the same calls",
           "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
