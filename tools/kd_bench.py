"""Times lattice knowledge distillation in the fused RNN-T loss against the plain loss, on the SAME operands, at the lattice shapes of
BASELINE configs 2 and 5:

  plain      forward + backward of the loss without a teacher (rnnt_hip_joint_loss_fwd_bwd_fastemit, then _bwd_fastemit)
  kd         forward + backward with a teacher's planes       (rnnt_hip_joint_loss_fwd_bwd_kd, then _bwd_kd: the KD kernel instances,
             one more plane out of the log-sum-exp pass, kd_value_kernel)
  teacher    the teacher's side alone                          (rnnt_hip_joint_cell_logprobs: one launch)

    python tools/kd_bench.py [--calls 20] [--rounds 5] [--step] [--out FILE]

Times are HIP events around windows of `calls` back-to-back calls on the current stream, `rounds` alternating windows per side after a
warm-up; reported per call: the median window and the spread (max - min over the windows), and kd / plain.  Operands are seeded
unit-variance A, C, bias with ragged lengths; the teacher's planes come from independently drawn operands.
--step: also the full training step (forward, backward, FlatAdamW step) of the config's model with and without args.kd_weight, the
teacher being a second model of the same architecture (its forward, without a graph, is part of the KD step).
Prints one JSON line per shape (and appends them to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("config2", "c2", 32, 1000, 40, 72), ("config5", "c5", 16, 1500, 80, 2048)]


def _windows(sides, calls, rounds, warmup=3):
    """sides: {name: callable}.  -> {name: [ms per call of each window]}, the windows of the sides alternating."""
    for f in sides.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, f in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return times


def _summary(times, prefix=""):
    out = {}
    for k, v in times.items():
        out[f"{prefix}{k}_ms"] = round(statistics.median(v), 4)
        out[f"{prefix}{k}_spread_ms"] = round(max(v) - min(v), 4)
    return out


def loss_level(B, T, U, V, calls, rounds):
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr, _stream, check
    lib = _lib.lib()
    g = torch.Generator().manual_seed(1234)
    U1 = U + 1
    A, At = torch.randn(T, B, V, generator=g).cuda(), torch.randn(T, B, V, generator=g).cuda()
    Cm, Ct = torch.randn(U1, B, V, generator=g).cuda(), torch.randn(U1, B, V, generator=g).cuda()
    bias = torch.randn(V, generator=g).cuda()
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
    t_list = [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()
    t_lens = torch.tensor(t_list, dtype=torch.int32).cuda()
    u_lens = torch.tensor([max(1, round(U * t / T)) for t in t_list], dtype=torch.int32).cuda()
    tail = (_addr(bias), _addr(labels), _addr(t_lens), _addr(u_lens), B, T, U1, V, 0)
    sep = (_addr(A), V, B * V, _addr(Cm), V, B * V) + tail
    sep_t = (_addr(At), V, B * V, _addr(Ct), V, B * V) + tail
    nws, nws_kd = lib.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V), lib.rnnt_hip_joint_loss_kd_workspace_bytes(B, T, U1, V)
    ws, ws_kd = torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(nws_kd, dtype=torch.uint8, device="cuda")
    nll, kd, gvec = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.ones(1, device="cuda")
    dA, dC = torch.empty_like(A), torch.empty_like(Cm)
    planes = tuple(torch.empty(B, U1, T, device="cuda") for _ in range(3))
    tp = tuple(_addr(x) for x in planes)

    def teacher():
        check(lib.rnnt_hip_joint_cell_logprobs(*sep_t, *tp, _stream()), "rnnt_hip_joint_cell_logprobs")

    def plain():
        check(lib.rnnt_hip_joint_loss_fwd_bwd_fastemit(*sep, 1.0, 0.0, _addr(nll), None, None, _addr(ws), nws, _stream()), "fwd")
        check(lib.rnnt_hip_joint_loss_bwd_fastemit(*sep, 1.0 / B, 0.0, _addr(gvec), 0, _addr(dA), _addr(dC), _addr(ws), nws, _stream()), "bwd")

    def with_kd():
        check(lib.rnnt_hip_joint_loss_fwd_bwd_kd(*sep, 1.0, 0.0, *tp, 1.0, _addr(nll), _addr(kd), None, None, _addr(ws_kd), nws_kd, _stream()),
              "fwd_kd")
        check(lib.rnnt_hip_joint_loss_bwd_kd(*sep, 1.0 / B, 0.0, _addr(gvec), 0, *tp, 0.5 / B, _addr(gvec), 0, _addr(dA), _addr(dC),
                                             _addr(ws_kd), nws_kd, _stream()), "bwd_kd")

    teacher()
    times = _windows({"plain": plain, "kd": with_kd, "teacher": teacher}, calls, rounds)
    assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dC).all()) and bool(torch.isfinite(kd).all())
    rec = _summary(times, "loss_")
    rec["loss_kd_over_plain"] = round(rec["loss_kd_ms"] / rec["loss_plain_ms"], 4)
    return rec


def step_level(cfg_name, calls, rounds):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from rnntransducer_amd.data import synthetic_batch
    cfg = bench.CONFIGS[cfg_name]
    B, T, U, V = cfg[:4]
    batch = synthetic_batch(B, T, U, V, ragged=True, seed=3)
    dev = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)
    teacher = bench.build_model(cfg, 0.0, 1000)[0].cuda()
    sides = {}
    for name, kw in (("plain", 0.0), ("kd", 0.5)):
        model = bench.build_model(cfg, 0.0, 1000)[0]
        model.args.kd_weight = kw
        model.kd_weight = kw
        model = model.cuda().train()
        if kw:
            model.set_teacher(teacher)
        opt = model.configure_optimizers()["optimizer"]

        def step(model=model, opt=opt):
            opt.zero_grad()
            model.training_step(dev, 0)["loss"].backward()
            opt.step()
        sides[name] = step
    times = _windows(sides, calls, rounds, warmup=2)
    rec = _summary(times, "step_")
    rec["step_kd_over_plain"] = round(rec["step_kd_ms"] / rec["step_plain_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time the full training step with and without args.kd_weight")
    ap.add_argument("--step-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kd_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd.csrc.build import source_digest
    for name, cfg_name, B, T, U, V in SHAPES:
        rec = {"shape": name, "B": B, "T": T, "U": U, "V": V, "calls": a.calls, "rounds": a.rounds}
        rec.update(loss_level(B, T, U, V, a.calls, a.rounds))
        if a.step:
            rec.update(step_level(cfg_name, a.step_calls, a.rounds))
            torch.cuda.empty_cache()
        rec.update({"timing": "HIP events around windows of back-to-back calls, alternating windows, median per call",
                    "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"})
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
