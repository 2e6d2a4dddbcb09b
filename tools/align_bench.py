"""Times ops.joint_align (forced alignment: log-softmax terms, max-plus sweep, back-trace) against the forward-only fused loss
(rnnt_hip_joint_loss_fwd_bwd with dA = dC = NULL: the same log-softmax kernel, alpha and beta sweeps) on the SAME operands, at the
lattice shapes of BASELINE configs 2, 3 and 5.

    python tools/align_bench.py [--window-ms 500] [--rounds 7] [--out FILE]

Per shape: warm-up of both calls, then `rounds` alternating windows of `reps` back-to-back calls each, every window between device
events and ended by a synchronise; `reps` is chosen per shape from a calibration window so that a window of the faster side lasts
about --window-ms (a window of a few tens of milliseconds would measure the scheduler as much as the kernels).  joint_align goes
through its Python wrapper (argument checks, a workspace-size query), the loss side is the bare library call: the comparison is
tilted slightly against the alignment.  Reported per call: the median window and the spread (max - min over the windows) of each.
Operands are seeded unit-variance A, C, bias with ragged lengths; nothing is copied to the host inside a window.
Prints one JSON line per shape (and appends them to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("config2", 32, 1000, 40, 72), ("config3", 8, 2000, 120, 72), ("config5", 16, 1500, 80, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd import _lib, ops
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.ops import _addr, _stream, check
    lib = _lib.lib()
    for name, B, T, U, V in SHAPES:
        g = torch.Generator().manual_seed(1234)
        U1 = U + 1
        A = torch.randn(T, B, V, generator=g).cuda()
        Cm = torch.randn(U1, B, V, generator=g).cuda()
        bias = torch.randn(V, generator=g).cuda()
        labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
        t_list = [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()
        t_lens = torch.tensor(t_list, dtype=torch.int32).cuda()
        u_lens = torch.tensor([max(1, round(U * t / T)) for t in t_list], dtype=torch.int32).cuda()
        ws_a = torch.empty(ops.align_workspace_bytes(B, T, U1, V), dtype=torch.uint8, device="cuda")
        frames = torch.empty(B, U, dtype=torch.int32, device="cuda")
        score = torch.empty(B, dtype=torch.float64, device="cuda")
        nws = lib.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
        ws_l = torch.empty(nws, dtype=torch.uint8, device="cuda")
        nll = torch.empty(B, device="cuda")

        def align():
            ops.joint_align(A, Cm, bias, labels, t_lens, u_lens, 0, workspace=ws_a, frames=frames, score=score)

        def loss_fwd():
            check(lib.rnnt_hip_joint_loss_fwd_bwd(_addr(A), V, B * V, _addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(t_lens),
                                                  _addr(u_lens), B, T, U1, V, 0, 1.0, _addr(nll), None, None, _addr(ws_l), nws, _stream()),
                  "rnnt_hip_joint_loss_fwd_bwd")

        def window(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        for _ in range(20):
            align()
            loss_fwd()
        torch.cuda.synchronize()
        # both numbers come from the same fp32 cell terms; slack: nll's fp32 rounding and the fp32 correction term of each alpha step
        slack = 2.0 ** -23 * nll.double().abs() + 2e-7 * (t_lens + u_lens).double()
        assert bool((score <= -nll.double() + slack).all()), "best-path score above -nll"
        reps = max(200, int(a.window_ms / min(window(align, 100), window(loss_fwd, 100))))
        ta, tl = [], []
        for _ in range(a.rounds):
            ta.append(window(align, reps))
            tl.append(window(loss_fwd, reps))
        rec = {"shape": name, "B": B, "T": T, "U": U, "V": V, "reps": reps, "rounds": a.rounds,
               "joint_align_ms": round(statistics.median(ta), 4), "joint_align_spread_ms": round(max(ta) - min(ta), 4),
               "loss_fwd_ms": round(statistics.median(tl), 4), "loss_fwd_spread_ms": round(max(tl) - min(tl), 4),
               "align_over_loss": round(statistics.median(ta) / statistics.median(tl), 3),
               "timing": "device events around windows of back-to-back calls, alternating, median window per call",
               "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
