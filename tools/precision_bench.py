"""fp32 vs fp16 compute mode of the recurrent layers (include/rnnt_hip.h RNNT_PRECISION_F16) on the full training step, both modes in
ONE process on one device.

    python tools/precision_bench.py [--config c2] [--steps 20] [--warmup 5]

Per mode: a parity gate against the float64 oracle first (INITIAL weights, dropout off, the whole batch on the HIP side with upstream
weight 0 on rows >= --parity-sample: bench.py's protocol, with the fp16 mode's bounds from tests/test_gpu_f16_compute.py), then
--warmup untimed and --steps timed training steps (fwd + fused joint/loss + bwd + AdamW) with the library's per-kernel profiler on.
Prints one JSON line: ms per step, utt/s, the per-kernel table and the loss / probe-gradient deviation from the oracle of each mode,
and the fp16 / fp32 throughput ratio.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (its model / oracle helpers; bench.py itself is not changed by this tool)

F16_LOSS_RTOL, F16_GRAD_TOL = 2e-3, 2e-2   # fp16 mode: loss relative; probe gradients max |dev| / max |ref|


def kernel_table(L, _lib):
    nk = len(_lib.KERNEL_KINDS)
    ms, work, cnt = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    _lib.check(L.rnnt_hip_prof_collect(ms, work, cnt, nk), "prof_collect")
    return {name: {"launches": int(cnt[i]), "ms_total": round(ms[i], 3), "avg_us": round(1e3 * ms[i] / cnt[i], 2)}
            for i, name in enumerate(_lib.KERNEL_KINDS) if cnt[i]}


def run_mode(precision, cfg, a, batch, threads):
    from rnntransducer_amd import _lib
    B, T, U, V = cfg[:4]
    model, tn, pn = bench.build_model(cfg, a.dropout, max(100, a.warmup + a.steps + 1))
    model = model.cuda().train()
    model.jointnet.set_compute_precision(precision)
    effective = model.jointnet.encoder.rnn.effective_precision(T, B)
    conf = model.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    lrd, gdev, _, finite = bench.parity_vs_float64_oracle(model, opt, tn, pn, V, batch, min(a.parity_sample, B), threads,
                                                          with_fp32_oracle=False)
    loss_tol, grad_tol = (1e-4, 2e-4) if precision == "fp32" else (F16_LOSS_RTOL, F16_GRAD_TOL)
    ok = bool(finite and lrd <= loss_tol and all(v["max_abs_dev"] <= grad_tol * max(v["ref_max_abs"], 1e-3) for v in gdev.values()))
    parity = {"loss_rel_delta": lrd, "grad_max_abs_dev": gdev, "all_rows_finite": finite, "loss_rel_tol": loss_tol,
              "grad_tol_of_max": grad_tol, "ok": ok}
    if not ok:
        return {"precision": precision, "effective_encoder_precision": effective, "parity": parity, "status": "parity failed"}

    def step():
        opt.zero_grad()
        loss = model.training_step(batch, 0)["loss"]
        loss.backward()
        opt.all_reduce_grads()
        opt.step()
        sched.step()
        return loss

    L = _lib.lib()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    L.rnnt_hip_prof_enable(0)
    kernel_table(L, _lib)   # drain whatever the parity gate and the warm-up recorded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        L.rnnt_hip_prof_enable(1 if i % a.profile_every == 0 else 0)
        loss = step()
    L.rnnt_hip_prof_enable(0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nprof = len(range(0, a.steps, a.profile_every))
    kernels = kernel_table(L, _lib)
    for v in kernels.values():
        v["ms_per_step"] = round(v["ms_total"] / nprof, 3)
    return {"precision": precision, "effective_encoder_precision": effective, "ms_per_step": round(1e3 * dt / a.steps, 3),
            "utt_per_s": round(B * a.steps / dt, 2), "last_loss": float(loss.detach()), "parity": parity, "kernels": kernels,
            "profiled_steps": nprof, "status": "ok"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--parity-sample", type=int, default=2)
    ap.add_argument("--profile-every", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=0)
    a = ap.parse_args()
    from rnntransducer_amd.data import synthetic_batch
    cfg = bench.CONFIGS[a.config]
    B, T, U, V = cfg[:4]
    batch = synthetic_batch(B, T, U, V, ragged=False, seed=1234, device="cuda")
    threads = a.cpu_threads or bench.host_cpu_info()[0]
    res = {name: run_mode(name, cfg, a, batch, threads) for name in ("fp32", "fp16")}
    out = {"metric": "precision_modes", "config": a.config, "B": B, "T": T, "U": U, "V": V, "steps": a.steps, "warmup": a.warmup,
           "modes": res}
    if all(r["status"] == "ok" for r in res.values()):
        out["fp16_speedup"] = round(res["fp16"]["utt_per_s"] / res["fp32"]["utt_per_s"], 4)
    print(json.dumps(out))
    return 0 if all(r["status"] == "ok" for r in res.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
