"""What the CTC forced alignment costs (csrc/ctc.hip: rnnt_hip_ctc_align), at the sizes of BASELINE configs 2
(B 32, T 1000, U 40, V 72) and 5 (B 16, T 1500, U 80, V 2048).

    python tools/ctc_align_bench.py [--configs c2,c5] [--calls 20] [--rounds 5] [--steps 5] [--skip-steps] [--out FILE]

1. The call: rnnt_hip_ctc_align (terms, max-plus sweep, back-trace; every output) against rnnt_hip_ctc_loss_fwd (terms, alpha and
   beta sweeps) on the same operands.  Times are the library's profiler slots (HIP events inside the library): lse = the terms kernel,
   alphabeta = the sweep(s), misc = the back-trace, which is a launch of its own.  Alternating windows of `calls` calls; per slot
   the median window per call and the spread (max - min over the windows) of the whole call.
2. A training step (forward, loss, backward, AdamW) with args.ar_source = "ctc" against the same step fed an external frame table
   (the 8-element batch; the table is the model's own CTC alignment of the batch, made once), against the plain step of the same
   model (CTC head, ctc_weight 0.3, no windows).  Host clock between device synchronises around windows of `steps` steps, modes
   alternating in one process.
Prints one JSON line per config and section (and appends them to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (B, T, U, V, enc (H, L), pred (H, L), O): BASELINE configs 2 and 5, as bench.py has them
CONFIGS = {"c2": (32, 1000, 40, 72, (512, 4), (512, 1), 512), "c5": (16, 1500, 80, 2048, (640, 6), (640, 1), 640)}
SLOTS = ("lse_kernel", "alphabeta_kernel", "misc")
LEFT, RIGHT, CTC_WEIGHT = 16, 16, 0.3


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def bench_call(name, cfg, a):
    from rnntransducer_amd import _lib, ops
    from rnntransducer_amd.ops import _addr, _stream, check
    lib = _lib.lib()
    nk = len(_lib.KERNEL_KINDS)
    slots = [_lib.KERNEL_KINDS.index(s) for s in SLOTS]
    B, T, U, V = cfg[:4]
    g = torch.Generator().manual_seed(1234)
    z = torch.randn(B, T, V, generator=g).cuda()
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
    t_list = [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()
    t_lens = torch.tensor(t_list, dtype=torch.int32).cuda()
    u_lens = torch.tensor([max(1, round(U * t / T)) for t in t_list], dtype=torch.int32).cuda()
    nll = torch.empty(B, device="cuda")
    first, last = (torch.empty(B, U, dtype=torch.int32, device="cuda") for _ in range(2))
    path = torch.empty(B, T, dtype=torch.int32, device="cuda")
    tlp, score = torch.empty(B, U, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
    nws_l, nws_a = lib.rnnt_hip_ctc_loss_workspace_bytes(B, T, U, V), ops.ctc_align_workspace_bytes(B, T, U, V)
    ws_l, ws_a = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (nws_l, nws_a))
    head = (_addr(z), T * V, V, _addr(labels), _addr(t_lens), _addr(u_lens), B, T, U, V, 0)

    def call(v):
        if v == "ctc_loss_fwd":
            check(lib.rnnt_hip_ctc_loss_fwd(*head, _addr(nll), _addr(ws_l), nws_l, _stream()), v)
        else:
            check(lib.rnnt_hip_ctc_align(*head, _addr(first), _addr(last), _addr(path), _addr(tlp), _addr(score), _addr(ws_a), nws_a,
                                         _stream()), v)

    def collect():
        ms, work, cnt = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
        torch.cuda.synchronize()
        check(lib.rnnt_hip_prof_collect(ms, work, cnt, nk), "rnnt_hip_prof_collect")
        return [ms[s] for s in slots]

    def window(v):
        lib.rnnt_hip_prof_enable(1)
        for _ in range(a.calls):
            call(v)
        lib.rnnt_hip_prof_enable(0)
        return [m / a.calls for m in collect()]

    variants = ("ctc_loss_fwd", "ctc_align")
    lib.rnnt_hip_prof_enable(0)
    for v in variants:
        for _ in range(5):
            call(v)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(score).all()) and bool((score <= -nll.double() * (1 - 1e-5)).all())
    collect()   # drain whatever was recorded before
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(window(v))
    rec = {"section": "call", "config": name, "B": B, "T": T, "U": U, "V": V, "calls_per_window": a.calls, "rounds": a.rounds}
    tot = {}
    for v in variants:
        per_slot = [statistics.median(w[i] for w in times[v]) for i in range(len(SLOTS))]
        totals = [sum(w) for w in times[v]]
        tot[v] = statistics.median(totals)
        rec[v] = {"ms": {s: round(m, 4) for s, m in zip(SLOTS, per_slot)}, "total_ms": round(tot[v], 4),
                  "spread_ms": round(max(totals) - min(totals), 4)}
    rec["align_over_loss_fwd"] = round(tot["ctc_align"] / tot["ctc_loss_fwd"], 4)
    rec["backtrace_share_of_align"] = round(rec["ctc_align"]["ms"]["misc"] / tot["ctc_align"], 4)
    rec["timing"] = "library profiler slots (HIP events inside the library), alternating windows, median per call"
    emit(rec, a.out)


def bench_step(name, cfg, a):
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd.data import synthetic_batch
    B, T, U, V, (He, Le), (Hp, Lp), O = cfg
    batch = synthetic_batch(B, T, U, V, ragged=False, seed=1234, device="cuda")
    total = 5 + a.steps * a.rounds + 10

    def build(**knobs):
        tn = dict(input_size=80, hidden_size=He, output_size=O, num_layers=Le, rnn_type="lstm", dropout=0.2, bidirectional=True)
        pn = dict(embedding_size=V, hidden_size=Hp, output_size=O, num_layers=Lp, rnn_type="lstm", dropout=0.2)
        args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=total,
                         move_metrics_to_cpu=False, ctc_weight=CTC_WEIGHT, **knobs)
        torch.manual_seed(0)
        model = RNNTransducer(pn, tn, dict(num_classes=V, aux_ctc=True), args).cuda().train()
        conf = model.configure_optimizers()
        return model, conf["optimizer"], conf["lr_scheduler"]["scheduler"]

    sides = {"plain": build(), "ar_frames": build(ar_left=LEFT, ar_right=RIGHT),
             "ar_ctc": build(ar_left=LEFT, ar_right=RIGHT, ar_source="ctc")}
    al = sides["ar_ctc"][0].ctc_align(batch)   # the external table of the "frames" side: one CTC alignment of the batch, made once
    table = torch.where(al.first >= 0, (al.first + al.last) // 2, al.first)
    batches = {"plain": batch, "ar_ctc": batch, "ar_frames": tuple(batch) + (table,)}

    def window(mode, n):
        model, opt, sched = sides[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            opt.zero_grad()
            loss = model.training_step(batches[mode], 0)["loss"]
            loss.backward()
            opt.step()
            sched.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(loss.detach())

    for mode in sides:
        window(mode, 5)
    ms, last = {m: [] for m in sides}, {}
    for _ in range(a.rounds):
        for mode in sides:
            t, last[mode] = window(mode, a.steps)
            ms[mode].append(t)
    med = {m: statistics.median(v) for m, v in ms.items()}
    rec = {"section": "step", "config": name, "B": B, "T": T, "U": U, "V": V, "steps_per_window": a.steps, "rounds": a.rounds,
           "ctc_weight": CTC_WEIGHT, "ar_left": LEFT, "ar_right": RIGHT,
           "ms_per_step": {m: round(v, 3) for m, v in med.items()},
           "spread_ms": {m: round(max(v) - min(v), 3) for m, v in ms.items()},
           "ar_ctc_over_ar_frames": round(med["ar_ctc"] / med["ar_frames"], 4), "ar_ctc_over_plain": round(med["ar_ctc"] / med["plain"], 4),
           "last_loss": {k: round(v, 4) for k, v in last.items()},
           "timing": "host clock between device synchronises around windows of full training steps, modes alternating in one process"}
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench needs the GPU: there is nothing to time without it")
    for name in a.configs.split(","):
        bench_call(name, CONFIGS[name], a)
        if not a.skip_steps:
            bench_step(name, CONFIGS[name], a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
