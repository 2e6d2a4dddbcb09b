"""Bitwise comparison of the loss / alignment entries of csrc/loss.hip and the CTC entries of csrc/ctc.hip under two builds of the library (the in-tree one against
OTHER, e.g. the parent commit built in a git worktree): one fresh process per library, every output as a .npy file, compared byte
for byte.  The method of tools/gemm_hp_epilogue_parity.py.
   python tools/loss_host_parity.py OTHER.so OUTDIR [--bench]
   cases:    seeded inputs, ragged lengths, B = 3, T = 33 (40 for the alignment), lambda in {0, 0.5}, windows off and on (row 1
             infeasible), at the (U1, V) that reach every host decision: (5,7) grad_sep K=1, (70,72) K=2, (130,8) K=3, (160,8)
             grad_sepv unchunked, (200,8) K=4, (320,8) K=8 and the chunked grad_sepv, (5,260) large_vocab, (1,3) no labels.
             Every entry: fused fwd+bwd; forward then _bwd with gvec_stride 0 and 1; the windowed pairs; the dense entries in
             fp32 / fp16 / bf16 at (5,7) and (70,72); both alignment entries.  Outputs: nll, dA, dC, grad, frames, score and the
             workspace's logZ slice.
   CTC (csrc/ctc.hip), in the same child: B = 3, blank in {0, V-1}, (U, V, T) in CTC_SHAPES -- no labels, then the K = 1, 2, 3, 4 and
             8 instances of the sweep with T = U + 41; row 0 full without equal neighbours, row 1 ragged with equal neighbours,
             row 2 with fewer frames than labels (no path); logits batch- and time-major.  ctc_loss_fwd then ctc_loss_bwd with
             gvec_stride 0 and 1 (nll, dlogits, the workspace's logZ slice); ctc_align (first, last, path, token_logp, score, the
             workspace's emission rows); ctc_greedy (tokens, counts, frames).
   --bench:  also `bench.py --config c2 --steps 3 --warmup 1 --dump-outputs`
Exit status 1 when a file differs or is missing on one side, or a child fails (nothing more is started then)."""
import os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (70, 72), (130, 8), (160, 8), (200, 8), (320, 8), (5, 260), (1, 3)]
DENSE_SHAPES = [(5, 7), (70, 72)]
B, T, T_ALIGN = 3, 33, 40
CTC_SHAPES = [(0, 3, 9), (4, 7, 33), (69, 8, 110), (129, 8, 170), (199, 8, 240), (319, 8, 360), (511, 8, 552)]   # (U, V, T)


def dump(out):
    """Child: run every case under the library RNNT_HIP_LIB selects and write the outputs to `out`."""
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    from rnntransducer_amd import _lib
    from rnntransducer_amd._lib import check
    from rnntransducer_amd.ops import _addr, _stream
    L, dev = _lib.lib(), "cuda"
    os.makedirs(out, exist_ok=True)

    def save(name, t):
        a = t.detach().cpu()
        np.save(os.path.join(out, name + ".npy"), (a.view(torch.int16) if a.dtype == torch.bfloat16 else a).numpy())

    def i32(a):
        return torch.tensor(a, dtype=torch.int32, device=dev)

    for U1, V in SHAPES:
        rng = np.random.default_rng(1000 * U1 + V)
        U = U1 - 1
        for Tc, align in ((T, False), (T_ALIGN, True)):
            A = torch.tensor(rng.normal(size=(B, Tc, V)), dtype=torch.float32, device=dev)
            Cm = torch.tensor(rng.normal(size=(B, U1, V)), dtype=torch.float32, device=dev)
            bias = torch.tensor(rng.normal(size=V), dtype=torch.float32, device=dev)
            labels = i32(rng.integers(1, V, size=(B, max(U, 1))))[:, :U].contiguous()
            t_lens, u_lens = i32([Tc, Tc - 5, Tc // 2]), i32([U, U // 2, max(U - 1, 0)])
            # U = 0: the backward-only entries refuse null labels, so u_lens stands in (never read as labels)
            sep = (_addr(A), Tc * V, V, _addr(Cm), U1 * V, V, _addr(bias), _addr(labels if U else u_lens), _addr(t_lens), _addr(u_lens), B, Tc, U1, V, 0)
            logits = (A[:, :, None, :] + Cm[:, None, :, :] + bias).contiguous()
            tag = f"u{U1}_v{V}"
            if align:
                nws = L.rnnt_hip_joint_align_workspace_bytes(B, Tc, U1, V)
                ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
                frames, score = torch.full((B, max(U, 1)), -7, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
                check(L.rnnt_hip_joint_align(*sep, _addr(frames), _addr(score), _addr(ws), nws, _stream()), "joint_align")
                save(f"{tag}_align_frames", frames), save(f"{tag}_align_score", score)
                if (U1, V) in DENSE_SHAPES:
                    for code, dt in enumerate((torch.float32, torch.float16, torch.bfloat16)):
                        z = logits.to(dt)
                        check(L.rnnt_hip_align_from_logits_ex(_addr(z), code, _addr(labels if U else u_lens), _addr(t_lens), _addr(u_lens), B, Tc,
                                                              U1, V, 0, _addr(frames), _addr(score), _addr(ws), nws, _stream()), "align_from_logits")
                        save(f"{tag}_align_dense{code}_frames", frames), save(f"{tag}_align_dense{code}_score", score)
                continue
            # windows: a band of +-3 frames round a diagonal alignment; row 1 infeasible (an empty window)
            ref = (torch.arange(max(U, 1), device=dev)[None, :] * (t_lens[:, None] - 1) // max(U, 1)).to(torch.int32)
            lo, hi = (ref - 3).contiguous(), (ref + 3).contiguous()
            lo[1, 0], hi[1, 0] = 9, 2
            gvec = torch.tensor(rng.normal(size=B), dtype=torch.float32, device=dev)
            for lam in (0.0, 0.5):
                for windowed in (False, True):
                    nws = (L.rnnt_hip_joint_loss_window_workspace_bytes if windowed else L.rnnt_hip_joint_loss_workspace_bytes)(B, Tc, U1, V)
                    win = (_addr(lo), _addr(hi), max(U, 1)) if windowed else ()
                    cname = f"{tag}_lam{lam}_win{int(windowed)}"

                    def fresh():
                        return (torch.zeros(nws, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.float32, device=dev),
                                torch.zeros_like(A), torch.zeros_like(Cm))

                    def ll(ws):   # logZ: after alpha | beta, each 256-byte aligned
                        off = 2 * ((B * Tc * U1 * 8 + 255) // 256 * 256)
                        return ws[off:off + B * 2 * 8].view(torch.float64)
                    ws, nll, dA, dC = fresh()
                    if windowed:
                        fwd = lambda nll, dA, dC, ws: L.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 0.25, lam, *win, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, _stream())
                        bwd = L.rnnt_hip_joint_loss_bwd_window
                    elif lam == 0.0:
                        fwd = lambda nll, dA, dC, ws: L.rnnt_hip_joint_loss_fwd_bwd(*sep, 0.25, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, _stream())
                        bwd = lambda *a: L.rnnt_hip_joint_loss_bwd(*a[:16], *a[17:])
                    else:
                        fwd = lambda nll, dA, dC, ws: L.rnnt_hip_joint_loss_fwd_bwd_fastemit(*sep, 0.25, lam, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, _stream())
                        bwd = L.rnnt_hip_joint_loss_bwd_fastemit
                    check(fwd(nll, dA, dC, ws), "fused")
                    for n, t in (("nll", nll), ("dA", dA), ("dC", dC), ("ll", ll(ws))):
                        save(f"{cname}_fused_{n}", t)
                    for stride in (0, 1):
                        ws, nll, dA, dC = fresh()
                        check(fwd(nll, None, None, ws), "forward")
                        check(bwd(*sep, 0.25, lam, _addr(gvec), stride, _addr(dA), _addr(dC), _addr(ws), nws, _stream()), "bwd")
                        for n, t in (("nll", nll), ("dA", dA), ("dC", dC), ("ll", ll(ws))):
                            save(f"{cname}_split{stride}_{n}", t)
                    if (U1, V) not in DENSE_SHAPES:
                        continue
                    for code, dt in enumerate((torch.float32, torch.float16, torch.bfloat16)):
                        z, (ws, nll, _, _) = logits.to(dt), fresh()
                        grad = torch.zeros_like(z)
                        dense = (_addr(z), code, _addr(labels), _addr(t_lens), _addr(u_lens), B, Tc, U1, V, 0, 0.25)
                        tail = (_addr(nll), _addr(grad), _addr(ws), nws, _stream())
                        if windowed:
                            check(L.rnnt_hip_loss_from_logits_fwd_bwd_window(*dense, lam, *win, *tail), "dense window")
                        elif lam != 0.0:
                            check(L.rnnt_hip_loss_from_logits_fwd_bwd_fastemit(*dense, lam, *tail), "dense fastemit")
                        elif code:
                            check(L.rnnt_hip_loss_from_logits_fwd_bwd_ex(*dense, *tail), "dense ex")
                        else:
                            check(L.rnnt_hip_loss_from_logits_fwd_bwd(dense[0], *dense[2:], *tail), "dense")
                        for n, t in (("nll", nll), ("grad", grad), ("ll", ll(ws))):
                            save(f"{cname}_dense{code}_{n}", t)
    dump_ctc(L, save)
    torch.cuda.synchronize()
    print(f"dumped {len(os.listdir(out))} files under {_lib.LIB_PATH}")


def dump_ctc(L, save):
    """The CTC entries of csrc/ctc.hip (same child, files ctc_*): every output buffer is pre-filled, so what a call leaves alone
    compares equal too."""
    import numpy as np, torch
    from rnntransducer_amd._lib import check
    from rnntransducer_amd.ops import _addr, _stream
    dev = "cuda"

    def i32(a):
        return torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)

    def up(n):
        return (n + 255) // 256 * 256

    for U, V, T in CTC_SHAPES:
        for blank in (0, V - 1):
            rng = np.random.default_rng(100000 * U + 10 * V + (blank != 0))
            tag = f"ctc_u{U}_v{V}_t{T}_bl{blank}"
            z = torch.tensor(rng.normal(size=(B, T, V)), dtype=torch.float32, device=dev)
            nonblank = np.array([v for v in range(V) if v != blank])
            lab = rng.integers(0, V - 1, size=(B, max(U, 1)))
            for u in range(1, lab.shape[1]):   # row 0, full length: no equal neighbours, so T = U + 41 leaves it a path
                lab[0, u] = (lab[0, u - 1] + 1 + rng.integers(0, V - 2)) % (V - 1)
            lab[1, 1::2] = lab[1, 0:lab.shape[1] - 1:2]   # row 1: equal neighbours
            labels = i32(nonblank[lab])[:, :U].contiguous()
            # row 2: fewer frames than labels, no path (U = 0: one frame)
            t_lens, u_lens = i32([T, T - 5, max(1, min(T, U - 1))]), i32([U, U // 2, U])
            lab_p = _addr(labels) if U else None
            cells = B * T * (U + 1)
            gvec = torch.tensor(rng.normal(size=B), dtype=torch.float32, device=dev)
            for layout, zz, z_sb, z_st in (("bm", z, T * V, V), ("tm", z.transpose(0, 1).contiguous(), V, B * V)):
                head = (_addr(zz), z_sb, z_st, lab_p, _addr(t_lens), _addr(u_lens), B, T, U, V, blank)
                nws = L.rnnt_hip_ctc_loss_workspace_bytes(B, T, U, V)
                for stride in (0, 1):
                    ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
                    nll, dz = torch.full((B,), -7.0, dtype=torch.float32, device=dev), torch.full_like(zz, -7.0)
                    check(L.rnnt_hip_ctc_loss_fwd(*head, _addr(nll), _addr(ws), nws, _stream()), "ctc_loss_fwd")
                    check(L.rnnt_hip_ctc_loss_bwd(*head, 0.25, _addr(gvec), stride, _addr(dz), _addr(ws), nws, _stream()), "ctc_loss_bwd")
                    off = 4 * up(cells * 8)   # logZ: after the four alpha / beta planes, each 256-byte aligned
                    for n, t in (("nll", nll), ("dlogits", dz), ("ll", ws[off:off + B * 8].view(torch.float64))):
                        save(f"{tag}_{layout}_g{stride}_{n}", t)
                nws = L.rnnt_hip_ctc_align_workspace_bytes(B, T, U, V)
                ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
                first, last = (torch.full((B, max(U, 1)), -7, dtype=torch.int32, device=dev) for _ in range(2))
                path = torch.full((B, T), -7, dtype=torch.int32, device=dev)
                tlp = torch.full((B, max(U, 1)), -7.0, dtype=torch.float64, device=dev)
                score = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
                check(L.rnnt_hip_ctc_align(*head, _addr(first), _addr(last), _addr(path), _addr(tlp), _addr(score), _addr(ws), nws, _stream()),
                      "ctc_align")
                for n, t in (("first", first), ("last", last), ("path", path), ("token_logp", tlp), ("score", score),
                             ("em", ws[:cells * 4].view(torch.float32))):   # the emission rows: offset 0 of the workspace
                    save(f"{tag}_{layout}_align_{n}", t)
                tokens, frames = (torch.full((B, T), -7, dtype=torch.int32, device=dev) for _ in range(2))
                counts = torch.full((B,), -7, dtype=torch.int32, device=dev)
                check(L.rnnt_hip_ctc_greedy(_addr(zz), z_sb, z_st, _addr(t_lens), B, T, V, blank, _addr(tokens), _addr(counts), _addr(frames),
                                            _stream()), "ctc_greedy")
                for n, t in (("tokens", tokens), ("counts", counts), ("frames", frames)):
                    save(f"{tag}_{layout}_greedy_{n}", t)


def run(cmd, env_extra, limit):
    env = dict(os.environ, **env_extra)
    if not env.get("RNNT_HIP_LIB"):
        env.pop("RNNT_HIP_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:])
        sys.exit(f"FAILED ({r.returncode}): {' '.join(cmd)}")
    print(r.stdout.strip().splitlines()[-1])


def compare(a, b, what):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{what}: {n} MISSING on one side"); bad += 1
        elif open(pa, "rb").read() != open(pb, "rb").read():
            print(f"{what}: {n} DIFFERS"); bad += 1
    print(f"{what}: {len(names)} files, {len(names) - bad} bytewise equal, {bad} differ")
    return bad


def main():
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    other, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    libs = (("other", other), ("main", ""))
    for tag, lib in libs:
        run([sys.executable, os.path.abspath(__file__), "--dump", os.path.join(out, "loss_" + tag)], {"RNNT_HIP_LIB": lib}, 300)
    bad = compare(os.path.join(out, "loss_other"), os.path.join(out, "loss_main"), "loss / alignment entries")
    if "--bench" in sys.argv:
        for tag, lib in libs:
            run([sys.executable, "bench.py", "--config", "c2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs",
                 os.path.join(out, "bench_" + tag)], {"RNNT_HIP_LIB": lib}, 300)
        bad += compare(os.path.join(out, "bench_other"), os.path.join(out, "bench_main"), "bench c2 outputs")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
