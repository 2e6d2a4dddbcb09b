"""Times what internal-LM training (ILMT) costs per training step, at BASELINE config-2 and config-5 sizes:

  plain  the plain training step (RNNTransducer.training_step, args.ilmt_weight = 0) — the side to compare with the parent commit,
         which can run this file with --sides plain (nothing else here exists there);
  ilmt   the same step with args.ilmt_weight = 0.2: one more launch in the loss's forward, one more in its backward;
  text   the text-only step: RNNTransducer.ilm_loss on the batch's transcripts, no audio and no encoder call, the encoder frozen
         before the optimizer is built (as text-only adaptation should be set up).

    python tools/ilmt_bench.py [--config c2|c5] [--sides plain,ilmt,text] [--steps 20] [--rounds 5] [--out FILE]

A step is zero_grad, the loss, backward, FlatAdamW step.  Every side has its own freshly initialised model (same seed) and optimizer;
after two warm-up steps per side come `rounds` alternating windows of `steps` steps each between HIP events.  Reported per side: the
windows (ms per step, in run order), their median, minimum and maximum.  Prints one JSON line (appended to --out)."""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bench.py's: (B, T, U, V, enc(H, L), pred(H, L), O)
CONFIGS = {"c2": (32, 1000, 40, 72, (512, 4), (512, 1), 512), "c5": (16, 1500, 80, 2048, (640, 6), (640, 1), 640)}
ILMT_WEIGHT = 0.2


def build(cfg, dropout, **kw):
    from rnntransducer_amd import RNNTransducer
    B, T, U, V, (He, Le), (Hp, Lp), O = cfg
    tn = dict(input_size=80, hidden_size=He, output_size=O, num_layers=Le, rnn_type="lstm", dropout=dropout, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=Hp, output_size=O, num_layers=Lp, rnn_type="lstm", dropout=dropout)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10000,
                     move_metrics_to_cpu=False, **kw)
    torch.manual_seed(0)
    return RNNTransducer(pn, tn, dict(num_classes=V), args).cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=list(CONFIGS))
    ap.add_argument("--sides", default="plain,ilmt,text")
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="free text copied into the record (which tree this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = [s for s in a.sides.split(",") if s]
    if not names or any(s not in ("plain", "ilmt", "text") for s in names):
        raise SystemExit(f"--sides takes a comma-separated subset of plain,ilmt,text, got {a.sides!r}")
    if not torch.cuda.is_available():
        raise SystemExit("ilmt_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.data import synthetic_batch
    cfg = CONFIGS[a.config]
    B, T, U, V = cfg[:4]
    batch = synthetic_batch(B, T, U, V, seed=1234, device="cuda")
    sides = {}
    for name in names:
        model = build(cfg, a.dropout, **({"ilmt_weight": ILMT_WEIGHT} if name == "ilmt" else {}))
        if name == "text":   # frozen before the optimizer is built: weight decay moves a zero-gradient parameter too
            model.jointnet.encoder.requires_grad_(False)
        opt = model.configure_optimizers()["optimizer"]

        def step(model=model, opt=opt, name=name):
            opt.zero_grad()
            loss = model.ilm_loss(batch[3], batch[5], batch[6]) if name == "text" else model.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()
            return loss.detach()
        sides[name] = step

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    losses = {}
    for name, step in sides.items():
        for _ in range(2):
            losses[name] = float(step())
    times = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, step in sides.items():
            times[name].append(timed(step, a.steps))
    rec = {"config": a.config, "label": a.label, "B": B, "T": T, "U": U, "V": V, "dropout": a.dropout, "ilmt_weight": ILMT_WEIGHT,
           "steps": a.steps, "rounds": a.rounds}
    for name, ts in times.items():
        rec[name] = {"windows_ms": [round(t, 3) for t in ts], "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                     "max_ms": round(max(ts), 3), "loss_after_warmup": losses[name]}
    rec.update({"timing": "HIP events around windows of `steps` steps (zero_grad, loss, backward, optimizer step), sides alternating, "
                          "ms per step", "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"})
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
