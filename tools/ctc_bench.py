"""What the auxiliary CTC branch costs per training step: the full step (forward, loss, backward, AdamW) of bench.py at BASELINE
configs 2 and 5, once with the CTC head absent (the path of a model without the feature, bit for bit) and once with the head and
ctc_weight = 0.3 (one more (B*T) x O x V product forward and two backward, csrc/ctc.hip's four launches).

    python tools/ctc_bench.py [--configs c2,c5] [--steps 10] [--rounds 5] [--warmup 5] [--out FILE]

Both models live in ONE process with the same seed, batch and dropout (0.2, bench.py's default) and take turns: `rounds` alternating
windows of `steps` steps each, every window between two device synchronises on the host clock.  Reported per mode: the median
window per step and the spread (max - min over the windows).  Prints one JSON line per config (and appends them to --out)."""
import argparse
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
CTC_WEIGHT = 0.3


def build(cfg, aux, total_steps):
    from rnntransducer_amd import RNNTransducer
    B, T, U, V, (He, Le), (Hp, Lp), O = cfg
    tn = dict(input_size=80, hidden_size=He, output_size=O, num_layers=Le, rnn_type="lstm", dropout=0.2, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=Hp, output_size=O, num_layers=Lp, rnn_type="lstm", dropout=0.2)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=total_steps,
                     move_metrics_to_cpu=False, ctc_weight=CTC_WEIGHT if aux else 0.0)
    torch.manual_seed(0)
    return RNNTransducer(pn, tn, dict(num_classes=V, aux_ctc=True) if aux else dict(num_classes=V), args).cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.data import synthetic_batch
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        B, T, U, V = cfg[:4]
        batch = synthetic_batch(B, T, U, V, ragged=False, seed=1234, device="cuda")
        total = a.warmup + a.steps * a.rounds + 10
        sides = {}
        for mode, aux in (("head_absent", False), ("ctc_0.3", True)):
            model = build(cfg, aux, total)
            conf = model.configure_optimizers()
            sides[mode] = (model, conf["optimizer"], conf["lr_scheduler"]["scheduler"])

        def step(mode):
            model, opt, sched = sides[mode]
            opt.zero_grad()
            loss = model.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()
            sched.step()
            return loss

        def window(mode, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                loss = step(mode)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n, float(loss.detach())

        for mode in sides:
            window(mode, a.warmup)
        ms = {mode: [] for mode in sides}
        last = {}
        for _ in range(a.rounds):
            for mode in sides:
                t, last[mode] = window(mode, a.steps)
                ms[mode].append(t)
        med = {mode: statistics.median(v) for mode, v in ms.items()}
        rec = {"config": name, "B": B, "T": T, "U": U, "V": V, "steps_per_window": a.steps, "rounds": a.rounds, "ctc_weight": CTC_WEIGHT,
               "head_absent_ms_per_step": round(med["head_absent"], 3),
               "head_absent_spread_ms": round(max(ms["head_absent"]) - min(ms["head_absent"]), 3),
               "ctc_ms_per_step": round(med["ctc_0.3"], 3), "ctc_spread_ms": round(max(ms["ctc_0.3"]) - min(ms["ctc_0.3"]), 3),
               "ctc_over_head_absent": round(med["ctc_0.3"] / med["head_absent"], 4),
               "last_loss": {k: round(v, 4) for k, v in last.items()},
               "timing": "host clock between device synchronises around windows of full training steps, modes alternating in one process, median window per step",
               "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del sides, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
