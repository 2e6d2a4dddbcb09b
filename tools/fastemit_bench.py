"""Times the lattice gradient of the fused RNN-T loss (rnnt_hip_joint_loss_bwd_fastemit: grad_sep / grad_sepv + reduce_dc) with
FastEmit off (lambda = 0: the FE = false kernel instances, the default path) and on (lambda = 1: the FE = true instances), on the SAME
operands and the same forward workspace, at the lattice shapes of BASELINE configs 2 and 5.

    python tools/fastemit_bench.py [--calls 40] [--rounds 5] [--out FILE]

The time is the library's own: the profiler slot of the lattice gradient (RNNT_K_LATGRAD, HIP events around the gradient launches
inside the library; rnnt_hip_prof_collect), not a host clock.  Per shape: one forward call fills the workspace, both sides are warmed
up, then `rounds` alternating windows of `calls` profiled backward calls each; reported per call: the median window and the spread
(max - min over the windows) of each side, and their ratio.  Operands are seeded unit-variance A, C, bias with ragged lengths.
Prints one JSON line per shape (and appends them to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("config2", 32, 1000, 40, 72), ("config5", 16, 1500, 80, 2048)]
LAMBDAS = (0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fastemit_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.ops import _addr, _stream, check
    lib = _lib.lib()
    nk = len(_lib.KERNEL_KINDS)
    slot = _lib.KERNEL_KINDS.index("lattice_grad_kernel")

    def collect():
        ms, work, cnt = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
        torch.cuda.synchronize()
        check(lib.rnnt_hip_prof_collect(ms, work, cnt, nk), "rnnt_hip_prof_collect")
        return ms[slot], int(cnt[slot])

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
        nws = lib.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        nll = torch.empty(B, device="cuda")
        gvec = torch.ones(1, device="cuda")
        dA, dC = torch.empty_like(A), torch.empty_like(Cm)
        sep = (_addr(A), V, B * V, _addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(t_lens), _addr(u_lens), B, T, U1, V, 0)
        check(lib.rnnt_hip_joint_loss_fwd_bwd(*sep, 1.0, _addr(nll), None, None, _addr(ws), nws, _stream()), "rnnt_hip_joint_loss_fwd_bwd")

        def bwd(lam):
            check(lib.rnnt_hip_joint_loss_bwd_fastemit(*sep, 1.0 / B, lam, _addr(gvec), 0, _addr(dA), _addr(dC), _addr(ws), nws,
                                                       _stream()), "rnnt_hip_joint_loss_bwd_fastemit")

        def window(lam):
            lib.rnnt_hip_prof_enable(1)
            for _ in range(a.calls):
                bwd(lam)
            lib.rnnt_hip_prof_enable(0)
            ms, cnt = collect()
            assert cnt == a.calls, (cnt, a.calls)
            return ms / cnt

        lib.rnnt_hip_prof_enable(0)
        for lam in LAMBDAS:
            for _ in range(10):
                bwd(lam)
        collect()   # drain whatever was recorded before
        assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dC).all())
        times = {lam: [] for lam in LAMBDAS}
        for _ in range(a.rounds):
            for lam in LAMBDAS:
                times[lam].append(window(lam))
        med = {lam: statistics.median(times[lam]) for lam in LAMBDAS}
        rec = {"shape": name, "B": B, "T": T, "U": U, "V": V, "calls": a.calls, "rounds": a.rounds,
               "latgrad_lambda0_ms": round(med[0.0], 4), "latgrad_lambda0_spread_ms": round(max(times[0.0]) - min(times[0.0]), 4),
               "latgrad_lambda1_ms": round(med[1.0], 4), "latgrad_lambda1_spread_ms": round(max(times[1.0]) - min(times[1.0]), 4),
               "lambda1_over_lambda0": round(med[1.0] / med[0.0], 4),
               "timing": "library profiler slot lattice_grad_kernel (HIP events inside the library), alternating windows, median per call",
               "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
