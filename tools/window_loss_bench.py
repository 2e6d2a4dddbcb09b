"""Times the fused RNN-T loss, forward plus backward in one call, without and with emission windows (the alignment-restricted loss,
DESIGN.md §24), on the SAME operands, at the lattice shapes of BASELINE configs 2, 3 and 5:

    plain      rnnt_hip_joint_loss_fwd_bwd                      (the W = false kernel instances: the default path)
    win_full   rnnt_hip_joint_loss_fwd_bwd_window, lo = 0, hi = T: nothing is skipped (the W = true instances, same results)
    win_16     ... windows (left, right) = (16, 16) around the diagonal alignment frames[u] = round(u (Tb-1) / Ub)
    win_64     ... (64, 64)

    python tools/window_loss_bench.py [--calls 20] [--rounds 5] [--shapes config2,config3,config5] [--variants plain,win_full,...]
                                      [--plain-only] [--out FILE]

The times are the library's own: its profiler slots (HIP events around the launches inside the library; rnnt_hip_prof_collect) of the
log-sum-exp kernel, of the alpha/beta sweep and of the lattice gradient (the gradient kernel and reduce_dc together: the slots are part
of the ABI and there is none for reduce_dc alone; a kernel trace of this tool, `rocprofv3 --kernel-trace --stats -- python
tools/window_loss_bench.py --variants X --rounds 1`, separates the two).  Per shape: every variant is warmed up, then `rounds`
alternating windows of `calls` profiled calls each; reported per call and slot: the median window and the spread (max - min over the
windows), and each windowed variant's ratio to plain.  --plain-only times the plain call alone and touches no windowed entry, so the
same file also runs on a checkout that has none (the comparison with the parent commit).  Operands are seeded unit-variance A, C, bias
with ragged lengths.  Prints one JSON line per shape (and appends them to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"config2": (32, 1000, 40, 72), "config3": (8, 2000, 120, 72), "config5": (16, 1500, 80, 2048)}
VARIANTS = {"plain": None, "win_full": "full", "win_16": 16, "win_64": 64}
SLOTS = ("lse_kernel", "alphabeta_kernel", "lattice_grad_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    variants = ["plain"] if a.plain_only else a.variants.split(",")
    shapes = a.shapes.split(",")
    for v in variants:
        if v not in VARIANTS:
            raise SystemExit(f"unknown variant {v!r}: one of {list(VARIANTS)}")
    for s in shapes:
        if s not in SHAPES:
            raise SystemExit(f"unknown shape {s!r}: one of {list(SHAPES)}")
    if not torch.cuda.is_available():
        raise SystemExit("window_loss_bench needs the GPU: there is nothing to time without it")
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc.build import source_digest
    from rnntransducer_amd.ops import _addr, _stream, check
    lib = _lib.lib()
    nk = len(_lib.KERNEL_KINDS)
    slots = [_lib.KERNEL_KINDS.index(s) for s in SLOTS]

    def collect():
        ms, work, cnt = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
        torch.cuda.synchronize()
        check(lib.rnnt_hip_prof_collect(ms, work, cnt, nk), "rnnt_hip_prof_collect")
        return [ms[s] for s in slots], [int(cnt[s]) for s in slots]

    for name in shapes:
        B, T, U, V = SHAPES[name]
        g = torch.Generator().manual_seed(1234)
        U1 = U + 1
        A = torch.randn(T, B, V, generator=g).cuda()
        Cm = torch.randn(U1, B, V, generator=g).cuda()
        bias = torch.randn(V, generator=g).cuda()
        labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
        t_list = [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()
        u_list = [max(1, round(U * t / T)) for t in t_list]
        t_lens = torch.tensor(t_list, dtype=torch.int32).cuda()
        u_lens = torch.tensor(u_list, dtype=torch.int32).cuda()
        diag = torch.tensor([[round(u * (tb - 1) / max(ub, 1)) for u in range(U)] for tb, ub in zip(t_list, u_list)], dtype=torch.int32)
        nll = torch.empty(B, device="cuda")
        dA, dC = torch.empty_like(A), torch.empty_like(Cm)
        sep = (_addr(A), V, B * V, _addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(t_lens), _addr(u_lens), B, T, U1, V, 0)
        nws = lib.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
        if not a.plain_only:
            nws = max(nws, lib.rnnt_hip_joint_loss_window_workspace_bytes(B, T, U1, V))
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        tables = {}
        for v in variants:
            w = VARIANTS[v]
            if w == "full":
                tables[v] = (torch.zeros(B, U, dtype=torch.int32).cuda(), torch.full((B, U), T, dtype=torch.int32).cuda())
            elif w is not None:
                tables[v] = ((diag - w).cuda(), (diag + w).cuda())

        def call(v):
            if v == "plain":
                check(lib.rnnt_hip_joint_loss_fwd_bwd(*sep, 1.0 / B, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, _stream()),
                      "rnnt_hip_joint_loss_fwd_bwd")
            else:
                lo, hi = tables[v]
                check(lib.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 1.0 / B, 0.0, _addr(lo), _addr(hi), U, _addr(nll), _addr(dA),
                                                             _addr(dC), _addr(ws), nws, _stream()), "rnnt_hip_joint_loss_fwd_bwd_window")

        def window(v):
            lib.rnnt_hip_prof_enable(1)
            for _ in range(a.calls):
                call(v)
            lib.rnnt_hip_prof_enable(0)
            ms, cnt = collect()
            assert all(c == a.calls for c in cnt), (cnt, a.calls)
            return [m / a.calls for m in ms]

        lib.rnnt_hip_prof_enable(0)
        nlls = {}
        for v in variants:
            for _ in range(5):
                call(v)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dC).all()), v
            nlls[v] = round(float(nll.double().mean()), 3)
        collect()   # drain whatever was recorded before
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v in variants:
                times[v].append(window(v))
        rec = {"shape": name, "B": B, "T": T, "U": U, "V": V, "calls": a.calls, "rounds": a.rounds, "mean_nll": nlls}
        total = {}
        for v in variants:
            per = {}
            for k, s in enumerate(SLOTS):
                xs = [w[k] for w in times[v]]
                per[s + "_ms"] = round(statistics.median(xs), 4)
                per[s + "_spread_ms"] = round(max(xs) - min(xs), 4)
            sums = [sum(w) for w in times[v]]
            total[v] = statistics.median(sums)
            per["loss_ms"] = round(total[v], 4)
            per["loss_spread_ms"] = round(max(sums) - min(sums), 4)
            rec[v] = per
        for v in variants:
            if v != "plain" and "plain" in total:
                rec[v]["loss_over_plain"] = round(total[v] / total["plain"], 4)
        rec.update({"timing": "library profiler slots (HIP events inside the library), alternating windows, median per fwd_bwd call; "
                              "loss_ms = the three slots summed; lattice_grad_kernel holds the gradient kernel and reduce_dc",
                    "kernel_sources": source_digest(), "dtype": "f32", "data": "synthetic"})
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
