"""Alignment-restricted RNN-T loss (per-label emission windows: the W instances of the lse / grad kernels of csrc/loss.hip, band_kernel)
on the device, against the float64 restatement tests/window_restatement.py (itself checked on the CPU by tests/test_window_oracle.py).

The fused kernels are driven through the C ABI with A, C and bias handed in directly, at the six shapes of
tests/test_gpu_fastemit.py::CASES (each names a kernel form), under both kernel families, both layouts and both upstream forms;
outputs and workspace start as NaN.  Bounds are that file's NLL_RTOL / GRAD_TOL / DENSE_ATOL: the arithmetic per live cell is the
same."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import window_restatement as wr
from tests.test_gpu_fastemit import CASES, DENSE_ATOL, FAMILIES, GRAD_TOL, IDS, NLL_RTOL, SCALE, _check, _effective, _problem

pytestmark = pytest.mark.gpu
LEFT, RIGHT = 2, 3


@pytest.fixture(params=FAMILIES, ids=("smallv", "largev"))
def family(request, monkeypatch):
    """large_vocab() reads the environment at every launch: no reload needed."""
    for k in FAMILIES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(request.param, "1")
    return request.param


def _diag(t_lens, u_lens, U, left=LEFT, right=RIGHT):
    fr = wr.diagonal_frames(t_lens, u_lens, U)
    return (fr - left).astype(np.int32), (fr + right).astype(np.int32)


def _nonmonotone(t_lens, u_lens, U):
    """Windows around the diagonal whose edges go back and forth: odd labels reach 7 frames further left, even labels 9 further right,
    so a later label's lo lies below an earlier one's and an earlier label's hi above a later one's.  Every label keeps its
    diagonal frame: feasible."""
    fr = wr.diagonal_frames(t_lens, u_lens, U)
    odd = (np.arange(U) % 2 == 1)[None, :]
    lo = fr - LEFT - 7 * odd
    hi = fr + RIGHT + 9 * ~odd
    return lo.astype(np.int32), hi.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(i, kind, lam):
    """Problem, windows and float64 reference (unit upstream weights) of CASES[i]: computed once, shared by both families and every
    test (treated as read-only).  kind: "diag" | "nonmono"."""
    B, T, U1, V, blank, t_lens, u_lens, _, _, _ = CASES[i]
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=T * 1000 + U1 * 10 + V)
    lo, hi = (_diag if kind == "diag" else _nonmonotone)(t_lens, u_lens, U1 - 1)
    ref = wr.window_fused(A, C, bias, y, t_lens, u_lens, blank, lo, hi, lam, [1.0] * B)
    return (A, C, bias, y), (lo, hi), ref


def _scaled(ref, gw):
    g = np.asarray(gw, dtype=np.float64).reshape(-1, 1, 1)
    return ref[0], ref[1] * g, ref[2] * g


def _other(layout, upstream, B):
    """The other layout and the other upstream form of a case."""
    return ("bm" if layout == "tm" else "tm"), (0.37 if isinstance(upstream, list) else [1.3, -0.7][:B])


def _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, lam, windows, split=True, pad=0):
    """-> nll (B,), dA (B,T,V), dC (B,U1,V) from the library.  windows = None: the entries without windows (lam None: the plain
    ones, a number: the _fastemit ones); windows = (lo, hi): the _window entries, the tables handed over as a (B,U) view of a table
    `pad` columns wider (whose other entries are out-of-range values).  upstream: a list (per-utterance gvec, stride 1) or a float
    (gscale, with a one-element gvec [2.0] of stride 0).  split: the forward call, then the backward call; else one fwd_bwd call
    (gscale 1)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    B, T, V = A.shape
    U1 = C.shape[1]
    if layout == "tm":   # what JointLossFn passes: (T,B,V) and (U1,B,V)
        a = torch.from_numpy(A).transpose(0, 1).contiguous().cuda()
        c = torch.from_numpy(C).transpose(0, 1).contiguous().cuda()
        (a_sb, a_st), (c_sb, c_su) = (V, B * V), (V, B * V)
    else:
        a, c = torch.from_numpy(A).cuda(), torch.from_numpy(C).cuda()
        (a_sb, a_st), (c_sb, c_su) = (T * V, V), (U1 * V, V)
    tb = torch.from_numpy(bias).cuda()
    yl = torch.from_numpy(y).cuda()
    tl = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    ul = torch.tensor(u_lens, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), float("nan"), device="cuda")
    dA, dC = torch.full_like(a, float("nan")), torch.full_like(c, float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    args = (_addr(a), a_sb, a_st, _addr(c), c_sb, c_su, _addr(tb), _addr(yl), _addr(tl), _addr(ul), B, T, U1, V, blank)
    if windows is None:
        nws = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
        extra = () if lam is None else (float(lam),)
        fwd_extra = extra
        fwd_bwd = L.rnnt_hip_joint_loss_fwd_bwd if lam is None else L.rnnt_hip_joint_loss_fwd_bwd_fastemit
        bwd = L.rnnt_hip_joint_loss_bwd if lam is None else L.rnnt_hip_joint_loss_bwd_fastemit
    else:
        nws = L.rnnt_hip_joint_loss_window_workspace_bytes(B, T, U1, V)
        stride = max(U1 - 1, 1) + pad
        wlo = torch.full((B, stride), 2 ** 30, dtype=torch.int32, device="cuda")    # the padding: an empty window, never read
        whi = torch.full((B, stride), -2 ** 30, dtype=torch.int32, device="cuda")
        wlo[:, :U1 - 1] = torch.from_numpy(windows[0]).cuda()
        whi[:, :U1 - 1] = torch.from_numpy(windows[1]).cuda()
        extra = (float(lam),)
        fwd_extra = (float(lam), _addr(wlo), _addr(whi), stride)
        fwd_bwd, bwd = L.rnnt_hip_joint_loss_fwd_bwd_window, L.rnnt_hip_joint_loss_bwd_window
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")   # all-ones bytes: NaN as fp32 and as fp64, -1 as int32
    if not split:
        _lib.check(fwd_bwd(*args, 1.0, *fwd_extra, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, stream), "fwd_bwd")
    else:
        _lib.check(fwd_bwd(*args, 1.0, *fwd_extra, _addr(nll), None, None, _addr(ws), nws, stream), "fwd")
        if isinstance(upstream, float):
            gscale, gvec, gstride = upstream, torch.tensor([2.0], device="cuda"), 0
        else:
            gscale, gvec, gstride = 1.0, torch.tensor(upstream, dtype=torch.float32, device="cuda"), 1
        _lib.check(bwd(*args, gscale, *extra, _addr(gvec), gstride, _addr(dA), _addr(dC), _addr(ws), nws, stream), "bwd")
    torch.cuda.synchronize()
    to_bm = (lambda x: x.cpu().numpy().transpose(1, 0, 2)) if layout == "tm" else (lambda x: x.cpu().numpy())
    return nll.cpu().numpy(), to_bm(dA), to_bm(dC)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_diagonal_windows_match_restatement(family, case):
    """a. Windows (2, 3) around the diagonal alignment: NLL, dA, dC of every kernel form against the restatement, in the case's own
    layout and upstream form and in the other ones; exact zeros on padded frames and on label rows beyond u_len."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    (A, C, bias, y), windows, ref = _case(case, "diag", 0.0)
    for k, (lay, up) in enumerate(((layout, upstream), _other(layout, upstream, B))):
        got = _run(A, C, bias, y, t_lens, u_lens, blank, lay, up, 0.0, windows, pad=3 * k)
        assert not any(np.isnan(x).any() for x in got)
        _check(got, _scaled(ref, _effective(up, B)), t_lens, u_lens, 0.0, f"{family} {lay}")


def test_windows_remove_paths():
    """a. The windows of the cases above do restrict the lattice: the restricted NLL exceeds the unrestricted one."""
    (A, C, bias, y), windows, ref = _case(0, "diag", 0.0)
    B, T, U1, V, blank, t_lens, u_lens = CASES[0][:7]
    full = wr.window_fused(A, C, bias, y, t_lens, u_lens, blank, np.zeros_like(windows[0]), np.full_like(windows[1], T), 0.0, [1.0] * B)
    assert ref[0][0] > full[0][0] + 0.1


@pytest.mark.parametrize("split", [False, True], ids=("fwd_bwd", "fwd_then_bwd"))
@pytest.mark.parametrize("case", [0, 2, 4], ids=[IDS[i] for i in (0, 2, 4)])
def test_full_windows_are_bitwise_the_plain_entries(family, case, split):
    """b. lo = 0, hi >= t_len - 1 through the new entries: NLL, dA and dC are bit for bit those of the plain entries."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    (A, C, bias, y), _, _ = _case(case, "diag", 0.0)
    lo = np.zeros((B, U1 - 1), np.int32)
    hi = np.array([[tb - 1 + (u % 2) for u in range(U1 - 1)] for tb in t_lens], np.int32)   # t_len - 1 and beyond
    old = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, None, None, split=split)
    new = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, 0.0, (lo, hi), split=split)
    for a, b in zip(old, new):
        assert not np.isnan(a).any() and np.array_equal(a, b)


@pytest.mark.parametrize("case", [0, 1, 3], ids=[IDS[i] for i in (0, 1, 3)])
def test_nonmonotone_windows_match_restatement(family, case):
    """c. A later label's lo below an earlier one's (and an earlier label's hi above a later one's)."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    (A, C, bias, y), (lo, hi), ref = _case(case, "nonmono", 0.0)
    assert (np.diff(lo[0, :u_lens[0]]) < 0).any() and (np.diff(hi[0, :u_lens[0]]) < 0).any()
    got = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, 0.0, (lo, hi))
    _check(got, _scaled(ref, _effective(upstream, B)), t_lens, u_lens, 0.0, family)


@pytest.mark.parametrize("case", [0, 2, 3], ids=[IDS[i] for i in (0, 2, 3)])
def test_windows_of_one_frame_leave_the_aligned_path(family, case):
    """d. lo = hi = the forced alignment's frames of the same operands: exactly one path survives, the best one; the NLL is minus
    rnnt_hip_joint_align's score and every frame's dA row sums to 0."""
    from rnntransducer_amd.ops import joint_align
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    (A, C, bias, y), _, _ = _case(case, "diag", 0.0)
    al = joint_align(torch.from_numpy(A).cuda(), torch.from_numpy(C).cuda(), torch.from_numpy(bias).cuda(), torch.from_numpy(y).cuda(),
                     torch.tensor(t_lens, dtype=torch.int32, device="cuda"), torch.tensor(u_lens, dtype=torch.int32, device="cuda"),
                     blank, batch_first=True)
    frames, score = al.frames.cpu().numpy().astype(np.int32), al.score.cpu().numpy()
    nll, dA, dC = _run(A, C, bias, y, t_lens, u_lens, blank, layout, [1.0] * B, 0.0, (frames, frames))
    np.testing.assert_allclose(nll, -score, rtol=NLL_RTOL)
    rows = np.abs(dA.astype(np.float64).sum(-1)).max()
    print(f"{family} dA row sums {rows:.3e}")
    assert rows < GRAD_TOL
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):
        assert np.all(dA[b, tb:] == 0) and np.all(dC[b, ub + 1:] == 0)


@pytest.mark.parametrize("T,U1,V,blank", [(33, 9, 65, 64), (65, 200, 72, 0)])
def test_infeasible_rows(family, T, U1, V, blank):
    """e. A row with an empty window and a row whose windows force labels out of order, next to a feasible row: +inf and all-zero
    dA / dC for the two, the feasible row keeps the bits it has alone (and matches the restatement), no NaN anywhere."""
    B, U = 3, U1 - 1
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=U1 + 1)
    t_lens, u_lens, gw = [T, T - 3, T - 7], [U, U // 2, U - 1], [1.0, 0.5, -0.8]
    lo, hi = _diag(t_lens, u_lens, U)
    lo[0, 2], hi[0, 2] = 9, 8                          # row 0: label 2 has an empty window
    lo[1, 0], hi[1, 0] = 10, 12                        # row 1: label 0 not before frame 10, label 1 not after frame 4
    lo[1, 1], hi[1, 1] = 2, 4
    ref = wr.window_fused(A[2:], C[2:], bias, y[2:], t_lens[2:], u_lens[2:], blank, lo[2:], hi[2:], 0.0, gw[2:])
    for layout in ("tm", "bm"):
        nll, dA, dC = _run(A, C, bias, y, t_lens, u_lens, blank, layout, gw, 0.0, (lo, hi))
        assert not any(np.isnan(x).any() for x in (nll, dA, dC))
        assert np.isposinf(nll[:2]).all() and np.isfinite(nll[2])
        assert np.all(dA[:2] == 0) and np.all(dC[:2] == 0)
        solo = _run(A[2:], C[2:], bias, y[2:], t_lens[2:], u_lens[2:], blank, layout, gw[2:], 0.0, (lo[2:], hi[2:]))
        for full, part in zip((nll, dA, dC), solo):
            assert np.array_equal(full[2:], part)
        _check(solo, ref, t_lens[2:], u_lens[2:], 0.0, f"{family} {layout}")


@pytest.mark.parametrize("T,U1,V,blank", [(33, 9, 65, 64), (65, 200, 72, 0)])
def test_one_frame_row_and_row_without_labels(family, T, U1, V, blank):
    """f. t_len = 1 (every label at frame 0) and u_len = 0 (no window is read) with windows present."""
    B, U = 3, U1 - 1
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=U1 + 2)
    t_lens, u_lens, gw = [1, T, T - 5], [min(U, 3), 0, U], [1.0, 0.5, -0.8]
    lo, hi = _diag(t_lens, u_lens, U)
    lo[1], hi[1] = 7, 3                                # u_len = 0: never read, whatever it holds
    ref = wr.window_fused(A, C, bias, y, t_lens, u_lens, blank, lo, hi, 0.0, gw)
    assert np.isfinite(ref[0]).all()
    for layout in ("tm", "bm"):
        got = _run(A, C, bias, y, t_lens, u_lens, blank, layout, gw, 0.0, (lo, hi))
        _check(got, ref, t_lens, u_lens, 0.0, f"{family} {layout}")


@pytest.mark.parametrize("case", [0, 3, 4], ids=[IDS[i] for i in (0, 3, 4)])
def test_fastemit_with_windows(family, case):
    """g. FastEmit lambda = 0.5 on the windowed lattice: lambda acts on the live cells' scalars; the NLL does not depend on it."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    lam = 0.5
    (A, C, bias, y), windows, ref = _case(case, "diag", lam)
    got = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, lam, windows)
    _check(got, _scaled(ref, _effective(upstream, B)), t_lens, u_lens, lam, family)
    got0 = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, 0.0, windows)
    assert np.array_equal(got[0], got0[0]) and not np.array_equal(got[1][0], got0[1][0])


@functools.lru_cache(maxsize=None)
def _dense_problem():
    rng = np.random.default_rng(34)
    B, T, U1, V = 3, 9, 5, 33
    z = (rng.normal(size=(B, T, U1, V)) * SCALE).astype(np.float32)
    y = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    t_lens, u_lens = [9, 6, 8], [4, 2, 3]
    lo, hi = _diag(t_lens, u_lens, U1 - 1, 1, 2)
    lo[2, 1], hi[2, 1] = 5, 4                          # row 2: infeasible
    return z, y, t_lens, u_lens, lo, hi


def _dense_run(z, y, t_lens, u_lens, lo, hi, lam, dtype):
    from rnntransducer_amd.loss import RNNTLoss
    zg = torch.from_numpy(z).to(dtype).cuda().requires_grad_(True)
    nll = RNNTLoss(0, "none", fastemit_lambda=lam)(zg, torch.from_numpy(y).cuda(), torch.tensor(t_lens, dtype=torch.int32, device="cuda"),
                                                   torch.tensor(u_lens, dtype=torch.int32, device="cuda"),
                                                   emit_windows=(torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()))
    nll[:2].sum().backward()   # (the infeasible row's +inf stays out of the sum; its gradient rows are zeros whatever comes back)
    assert zg.grad.dtype == dtype
    return nll.detach().cpu().numpy(), zg.grad.float().cpu().numpy()


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_dense_logits_fp32(lam):
    """h. lse_dense / grad_dense<float> with windows: against the restatement within 2e-5 (1 + lambda) absolute; per-cell row sums
    below 1e-5 (1 + lambda); exact zeros outside the lattice and in the infeasible row, whose NLL is +inf."""
    z, y, t_lens, u_lens, lo, hi = _dense_problem()
    ref_nll, ref_dz = wr.window_loss(z, y, t_lens, u_lens, 0, lo, hi, lam)
    nll, g = _dense_run(z, y, t_lens, u_lens, lo, hi, lam, torch.float32)
    assert np.isposinf(nll[2]) and np.isposinf(ref_nll[2]) and not np.isnan(g).any()
    np.testing.assert_allclose(nll[:2], ref_nll[:2], rtol=NLL_RTOL)
    err, rows = np.abs(g - ref_dz).max(), np.abs(g.astype(np.float64).sum(-1)).max()
    print(f"lambda {lam}: err {err:.3e} row sums {rows:.3e}")
    assert err < DENSE_ATOL * (1.0 + lam)
    assert rows < 1e-5 * (1.0 + lam)
    assert np.all(g[2] == 0)
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):
        assert np.all(g[b, tb:] == 0) and np.all(g[b, :, ub + 1:] == 0)
    assert np.all(g[0][ref_dz[0].any(-1) == 0] == 0)   # cells no allowed path visits: exact zeros


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("dtype,grad_tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)], ids=("f16", "bf16"))
def test_dense_logits_half(dtype, grad_tol, lam):
    """h. <__half | __hip_bfloat16>: the reference runs on the rounded logits; the half-logit bounds of the FastEmit dense tests."""
    z, y, t_lens, u_lens, lo, hi = _dense_problem()
    zr = torch.from_numpy(z).to(dtype).float().numpy()
    ref_nll, ref_dz = wr.window_loss(zr, y, t_lens, u_lens, 0, lo, hi, lam)
    nll, g = _dense_run(zr, y, t_lens, u_lens, lo, hi, lam, dtype)
    assert np.isposinf(nll[2]) and not np.isnan(g).any() and np.all(g[2] == 0)
    np.testing.assert_allclose(nll[:2], ref_nll[:2], rtol=NLL_RTOL)
    err = np.abs(g - ref_dz).max()
    print(f"{dtype} lambda {lam}: err {err:.3e}")
    assert err < grad_tol * (1.0 + lam)


@functools.lru_cache(maxsize=None)
def _joint_reference():
    """fp64 operands of the JointLossFn test, the windows, the materialised logits' gradient dz (restatement, lambda 0.5) and the NLL."""
    B, T, U, V, Oe, Od = 2, 40, 199, 72, 8, 8
    g = torch.Generator().manual_seed(200)
    enc = torch.randn(B, T, Oe, generator=g, dtype=torch.float64)
    dec = torch.randn(B, U + 1, Od, generator=g, dtype=torch.float64)
    W = torch.randn(V, Oe + Od, generator=g, dtype=torch.float64) * 0.3
    bias = torch.randn(V, generator=g, dtype=torch.float64) * 0.1
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    t_lens, u_lens = [T, 27], [U, 160]
    lo, hi = _diag(t_lens, u_lens, U)
    cat = torch.cat((enc[:, :, None, :].expand(-1, -1, U + 1, -1), dec[:, None, :, :].expand(-1, T, -1, -1)), -1)
    logits = torch.nn.functional.gelu(cat, approximate="tanh") @ W.T + bias
    nll, dz = wr.window_loss(logits.numpy(), y.numpy(), t_lens, u_lens, 0, lo, hi, 0.5)
    return (enc, dec, W, bias, y, t_lens, u_lens, lo, hi), nll, torch.from_numpy(dz)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_joint_loss_fn_with_windows(family, reduction):
    """i. JointLossFn with windows (and lambda = 0.5) at U+1 = 200, V = 72: d_enc, d_dec, d_fc.weight, d_fc.bias against torch-CPU
    float64 autograd through the materialising joint fed with the restatement's dz."""
    from rnntransducer_amd.ops import JointLossFn
    lam = 0.5
    (enc, dec, W, bias, y, t_lens, u_lens, lo, hi), ref_nll, dz = _joint_reference()
    B, T, U = enc.shape[0], enc.shape[1], dec.shape[1] - 1
    e, d, w, bb = (x.clone().requires_grad_(True) for x in (enc, dec, W, bias))
    cat = torch.cat((e[:, :, None, :].expand(-1, -1, U + 1, -1), d[:, None, :, :].expand(-1, T, -1, -1)), -1)
    logits = torch.nn.functional.gelu(cat, approximate="tanh") @ w.T + bb
    gw = {"none": torch.tensor([0.6, -1.2], dtype=torch.float64), "sum": torch.ones(B, dtype=torch.float64),
          "mean": torch.full((B,), 1.0 / B, dtype=torch.float64)}[reduction]
    logits.backward(dz * gw.view(-1, 1, 1, 1))
    dev = "cuda"
    te = enc.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    td = dec.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    tw = W.float().to(dev).requires_grad_(True)
    tb = bias.float().to(dev).requires_grad_(True)
    out = JointLossFn.apply(te, td, tw, tb, y.to(dev), torch.tensor(t_lens, dtype=torch.int32, device=dev),
                            torch.tensor(u_lens, dtype=torch.int32, device=dev), 0, True, reduction, lam,
                            (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)))
    if reduction == "none":
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref_nll, rtol=NLL_RTOL)
        (out * gw.float().to(dev)).sum().backward()
    else:
        want = ref_nll.sum() * (1.0 / B if reduction == "mean" else 1.0)
        assert abs(out.item() - want) < NLL_RTOL * abs(want)
        out.backward()
    for name, got, ref in (("d_enc", te.grad.transpose(0, 1), e.grad), ("d_dec", td.grad.transpose(0, 1), d.grad),
                           ("d_fc.weight", tw.grad, w.grad), ("d_fc.bias", tb.grad, bb.grad)):
        err, bound = (got.double().cpu() - ref).abs().max().item(), GRAD_TOL * (1.0 + lam) * max(1.0, ref.abs().max().item())
        print(f"{reduction} {name}: err {err:.3e} bound {bound:.3e}")
        assert err < bound, f"{name}: {err}"


def test_python_surface_rejects_bad_windows_on_the_device():
    """Type, shape, dtype and device errors raise ValueError before anything runs."""
    from rnntransducer_amd.loss import RNNTLoss
    z = torch.zeros(2, 4, 3, 5, device="cuda")
    y = torch.ones(2, 2, dtype=torch.int32, device="cuda")
    tl = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    ul = torch.full((2,), 2, dtype=torch.int32, device="cuda")
    good = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    for bad in ((good, good.cpu()), (good.long(), good), (good[:, :1], good), good, (good, None)):
        with pytest.raises(ValueError, match="emit_windows"):
            RNNTLoss(0, "none")(z, y, tl, ul, emit_windows=bad)
    assert torch.isfinite(RNNTLoss(0, "none")(z, y, tl, ul, emit_windows=(good, good + 3))).all()


def test_model_level_windows():
    """j. A ragged batch given with the python length list, rows NOT in length order: JointNet.loss(reduction="none", emit_windows)
    equals each row run alone, so the windows followed their rows through the sort; training_step with args.ar_left / ar_right and an
    8-tuple equals jointnet.loss with ops.emit_windows(...), loss and parameter gradients bit for bit; the knobs with a 7-tuple
    raise ValueError."""
    from oracle.rnnt_oracle import make_batch
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd.ops import emit_windows
    V = 10
    tn = dict(input_size=12, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)
    batch = make_batch(4, 24, 5, V, n_mels=12, ragged=True, seed=3)
    batch = tuple(x.flip(0) if isinstance(x, torch.Tensor) else x[::-1] for x in batch)   # the longest row last: the sort moves rows
    t_list, u_list = batch[1], batch[6].tolist()
    assert sorted(t_list, reverse=True) != t_list and len(set(t_list)) > 1
    frames = torch.from_numpy(wr.diagonal_frames(t_list, u_list, 5))
    dev = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)
    lo, hi = emit_windows(frames.cuda(), dev[2], dev[6], LEFT, RIGHT)

    def model(**knobs):
        torch.manual_seed(0)
        return RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), Namespace(move_metrics_to_cpu=False, **knobs)).cuda().train()

    m = model()
    with torch.no_grad():
        rows = m.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="none", audio_lengths=dev[1], emit_windows=(lo, hi))
        plain = m.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="none", audio_lengths=dev[1])
        for b in range(4):
            s = slice(b, b + 1)
            alone = m.jointnet.loss(dev[0][s], dev[2][s], dev[3][s], dev[5][s], dev[6][s], 0, reduction="none",
                                    audio_lengths=[t_list[b]], emit_windows=(lo[s], hi[s]))
            assert abs(rows[b].item() - alone.item()) < 1e-5 * abs(alone.item()), (b, rows[b].item(), alone.item())
    assert torch.isfinite(rows).all() and bool((rows > plain + 1e-3).all())   # the windows restrict every row

    def grads(via_step):
        mm = model(ar_left=LEFT, ar_right=RIGHT) if via_step else model()
        if via_step:
            loss = mm.training_step(dev + (frames.cuda(),), 0)["loss"]
        else:
            loss = mm.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="mean", audio_lengths=dev[1],
                                    emit_windows=(lo, hi))
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in mm.named_parameters() if p.grad is not None}

    l_step, g_step = grads(True)
    l_loss, g_loss = grads(False)
    assert torch.equal(l_step, l_loss) and torch.isfinite(l_step)
    assert abs(l_step.item() - rows.mean().item()) < 1e-5 * abs(l_step.item())
    assert set(g_step) == set(g_loss)
    for k in g_step:
        assert torch.equal(g_step[k], g_loss[k]), k
    with pytest.raises(ValueError, match="8-element batch"):
        model(ar_left=LEFT, ar_right=RIGHT).training_step(dev, 0)
