"""Alignment-restricted RNN-T loss (emission windows), CPU side: the float64 restatement the GPU tests compare against
(tests/window_restatement.py) is checked against brute-force enumeration of every path on tiny lattices, against the C oracle with
full windows and against finite differences; the host-side pieces of the feature (ops.emit_windows, argument validation in python
and in the C ABI, the workspace query) are checked here too."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle.rnnt_oracle import rnnt_loss_c
from tests import window_restatement as wr


def _draw(B, T, U1, V, blank, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(B, T, U1, V)) * 1.5
    others = np.array([v for v in range(V) if v != blank])
    y = others[rng.integers(0, others.size, size=(B, U1 - 1))].astype(np.int32)
    return z, y


def _random_windows(rng, Tb, Ub, kind):
    """kind 0: wide random; 1: narrow random (often empty or out of order: infeasible); 2: non-monotone but feasible."""
    if kind == 0:
        lo = rng.integers(-2, max(Tb // 2, 1), size=Ub)
        hi = lo + rng.integers(0, Tb + 2, size=Ub)
    elif kind == 1:
        lo = rng.integers(-1, Tb + 1, size=Ub)
        hi = lo + rng.integers(-1, 2, size=Ub)
    else:
        lo = np.sort(rng.integers(0, max(Tb - 1, 1), size=Ub))[::-1].copy()   # later labels have LOWER lo
        hi = np.full(Ub, Tb + 3)
    return lo.astype(np.int32), hi.astype(np.int32)


@pytest.mark.parametrize("seed", range(40))
def test_restatement_equals_enumeration_of_every_path(seed):
    """T <= 5, U <= 3: logZ of the restricted lattice is the log-sum over the enumerated allowed paths (-inf when there is none),
    with random windows: negative lo, hi past the end, empty, non-monotone."""
    rng = np.random.default_rng(seed)
    Tb, Ub, V, blank = int(rng.integers(1, 6)), int(rng.integers(0, 4)), 4, int(rng.integers(0, 4))
    z, y = _draw(1, Tb, Ub + 1, V, blank, seed + 100)
    lo, hi = _random_windows(rng, Tb, Ub, seed % 3)
    lp = wr._log_softmax(z[0])
    blk = lp[:, :, blank]
    emit = np.zeros((Tb, Ub + 1))
    for u in range(Ub):
        emit[:, u] = lp[:, u, y[0, u]]
    want = wr.brute_force_logz(blk, emit, Tb, Ub, lo, hi)
    nll, dz = wr.window_loss(z, y, [Tb], [Ub], blank, lo[None], hi[None])
    assert not np.isnan(dz).any()
    if want == -np.inf:
        assert np.isposinf(nll[0]) and np.all(dz == 0)
    else:
        assert abs(-nll[0] - want) < 1e-12


def test_enumeration_cases_cover_both_outcomes():
    """The draw above holds feasible and infeasible rows, and windows that really remove paths."""
    feas = infeas = cut = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        Tb, Ub, V, blank = int(rng.integers(1, 6)), int(rng.integers(0, 4)), 4, int(rng.integers(0, 4))
        z, y = _draw(1, Tb, Ub + 1, V, blank, seed + 100)
        lo, hi = _random_windows(rng, Tb, Ub, seed % 3)
        nll, _ = wr.window_loss(z, y, [Tb], [Ub], blank, lo[None], hi[None])
        full, _ = wr.window_loss(z, y, [Tb], [Ub], blank, np.zeros((1, Ub), np.int32), np.full((1, Ub), Tb, np.int32))
        feas += np.isfinite(nll[0])
        infeas += np.isposinf(nll[0])
        cut += np.isfinite(nll[0]) and nll[0] > full[0] + 1e-9
    assert feas >= 10 and infeas >= 5 and cut >= 5, (feas, infeas, cut)


SHAPES = [
    (3, 5, 4, 6, 0, [5, 3, 1], [3, 1, 0]),
    (2, 7, 3, 5, 4, [7, 6], [2, 0]),
    (2, 4, 6, 9, 3, [4, 2], [5, 4]),
]
IDS = [f"T{s[1]}-U1_{s[2]}-V{s[3]}" for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_full_windows_equal_the_oracle(shape):
    B, T, U1, V, blank, t_lens, u_lens = shape
    z, y = _draw(B, T, U1, V, blank, seed=T * 100 + V)
    lo = np.zeros((B, U1 - 1), np.int32)
    hi = np.array([[tb - 1] * (U1 - 1) for tb in t_lens], np.int32)
    nll, dz = wr.window_loss(z, y, t_lens, u_lens, blank, lo, hi)
    ref_nll, ref_dz = rnnt_loss_c(z, y, t_lens, u_lens, blank)
    np.testing.assert_allclose(nll, ref_nll, rtol=1e-12)
    assert np.abs(dz - ref_dz).max() < 1e-12


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_gradient_equals_finite_differences(lam):
    """dz is d nll / dz of the restricted lattice (lam = 0), checked entry by entry with central differences; with lam > 0 it is the
    gradient of nll + lam * sum stopgrad(ce) * (-emit'), checked the same way with ce frozen at the base point."""
    B, T, U1, V, blank = 2, 5, 4, 4, 1
    t_lens, u_lens = [5, 4], [3, 2]
    z, y = _draw(B, T, U1, V, blank, seed=77)
    lo = np.array([[0, 1, 2], [1, 0, 9]], np.int32)     # row 1: non-monotone; its third entry is past u_len and never read
    hi = np.array([[2, 3, 9], [2, 3, -5]], np.int32)
    nll, dz = wr.window_loss(z, y, t_lens, u_lens, blank, lo, hi, lam)
    assert np.isfinite(nll).all()

    def surrogate(zz, b, ce0):
        n, _ = wr.window_loss(zz[None], y[b:b + 1], t_lens[b:b + 1], u_lens[b:b + 1], blank, lo[b:b + 1], hi[b:b + 1])
        if lam == 0.0:
            return n[0]
        lp = wr._log_softmax(zz)
        extra = sum(ce0[t, u] * -lp[t, u, y[b, u]] for t in range(t_lens[b]) for u in range(u_lens[b]) if ce0[t, u] > 0)
        return n[0] + lam * extra

    eps = 1e-6
    for b in range(B):
        Tb, Ub = t_lens[b], u_lens[b]
        lp = wr._log_softmax(z[b])
        emit = np.zeros((Tb, Ub + 1))
        for u in range(Ub):
            emit[:, u] = lp[:Tb, u, y[b, u]]
        _, _, ce0, _ = wr.posteriors(lp[:Tb, :Ub + 1, blank], wr.masked_emit(emit, Tb, Ub, lo[b], hi[b]), Tb, Ub)
        num = np.zeros_like(z[b])
        for idx in np.ndindex(*z[b].shape):
            zp, zm = z[b].copy(), z[b].copy()
            zp[idx] += eps
            zm[idx] -= eps
            num[idx] = (surrogate(zp, b, ce0) - surrogate(zm, b, ce0)) / (2 * eps)
        assert np.abs(num - dz[b]).max() < 1e-7
    assert np.abs(dz.sum(-1)).max() < 1e-12   # row sums over v vanish in every cell


def test_fused_form_sums_the_dense_gradient():
    B, T, U1, V, blank, t_lens, u_lens = SHAPES[0]
    rng = np.random.default_rng(5)
    A, C, bias = rng.normal(size=(B, T, V)), rng.normal(size=(B, U1, V)), rng.normal(size=V)
    _, y = _draw(B, T, U1, V, blank, seed=6)
    fr = wr.diagonal_frames(t_lens, u_lens, U1 - 1)
    lo, hi = fr - 1, fr + 1
    gw = [0.5, -1.5, 2.0]
    nll, dA, dC = wr.window_fused(A, C, bias, y, t_lens, u_lens, blank, lo, hi, 0.7, gw)
    z = A[:, :, None, :] + C[:, None, :, :] + bias
    nll2, dz = wr.window_loss(z, y, t_lens, u_lens, blank, lo, hi, 0.7)
    g = np.asarray(gw).reshape(-1, 1, 1, 1)
    np.testing.assert_allclose(nll, nll2, rtol=1e-14)
    assert np.abs(dA - (dz * g).sum(2)).max() < 1e-13 and np.abs(dC - (dz * g).sum(1)).max() < 1e-13


def test_emit_windows_builder():
    from rnntransducer_amd.ops import emit_windows
    frames = torch.tensor([[3, 5, 9], [2, -1, -1]], dtype=torch.int64)
    lo, hi = emit_windows(frames, [12, 4], torch.tensor([3, 1]), 2, 3)
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32
    assert lo.tolist() == [[1, 3, 7], [0, -3, -3]] and hi.tolist() == [[6, 8, 12], [5, 2, 2]]
    lo0, hi0 = emit_windows(frames.to(torch.int32), [12, 4], [3, 1], 0, 0)
    assert torch.equal(lo0, hi0) and torch.equal(lo0, frames.to(torch.int32))
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="left"):
            emit_windows(frames, [12, 4], [3, 1], bad, 0)
        with pytest.raises(ValueError, match="right"):
            emit_windows(frames, [12, 4], [3, 1], 0, bad)
    with pytest.raises(ValueError, match="frames"):
        emit_windows(frames.float(), [12, 4], [3, 1], 1, 1)
    with pytest.raises(ValueError, match="frames"):
        emit_windows(frames[0], [12], [3], 1, 1)
    with pytest.raises(ValueError, match="t_lens"):
        emit_windows(frames, [12], [3, 1], 1, 1)


def test_check_emit_windows_rejects_bad_arguments():
    from rnntransducer_amd.ops import check_emit_windows
    B, U = 2, 3
    lo = torch.zeros(B, U, dtype=torch.int32)
    assert check_emit_windows(None, B, U, "cpu") is None
    got = check_emit_windows((lo, lo + 4), B, U, "cpu")
    assert got[2] == U and torch.equal(got[0], lo)
    wide = torch.zeros(B, 8, dtype=torch.int32)
    assert check_emit_windows((wide[:, :U], wide[:, :U]), B, U, "cpu")[0].is_contiguous()
    assert check_emit_windows((lo[:, :0], lo[:, :0]), B, 0, "cpu")[0].shape == (B, 1)   # U = 0: a column of padding, no null pointer
    for bad in (lo, (lo,), (lo, lo, lo), "ab", (lo, None), (lo, lo.long()), (lo, lo.float()), (lo, lo[:, :2]), (lo[:1], lo[:1]),
                (lo, lo.tolist())):
        with pytest.raises(ValueError, match="emit_windows"):
            check_emit_windows(bad, B, U, "cpu")
    with pytest.raises(ValueError, match="must be on"):
        check_emit_windows((lo, lo), B, U, "cuda:0")


def _tiny_model_args():
    prednet = dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1)
    transnet = dict(input_size=12, hidden_size=8, output_size=12, num_layers=1)
    return prednet, transnet, dict(num_classes=10)


def test_model_knobs():
    from rnntransducer_amd import RNNTransducer
    prednet, transnet, joint = _tiny_model_args()
    m = RNNTransducer(prednet, transnet, joint, Namespace())
    assert m.ar_left is None and m.ar_right is None
    m = RNNTransducer(prednet, transnet, joint, Namespace(ar_left=2, ar_right=0))
    assert (m.ar_left, m.ar_right) == (2, 0)
    for bad in (dict(ar_left=1), dict(ar_right=1), dict(ar_left=-1, ar_right=1), dict(ar_left=1, ar_right=1.5),
                dict(ar_left=True, ar_right=1)):
        with pytest.raises(ValueError, match="ar_left|ar_right"):
            RNNTransducer(prednet, transnet, joint, Namespace(**bad))
    with pytest.raises(ValueError, match="8-element batch"):   # the knobs set and the 7-tuple batch: refused before anything runs
        m.training_step((None,) * 7, 0)


def test_abi_checks_the_windows_before_any_device_work():
    """Every other argument is acceptable and the pointers are stand-ins that are never dereferenced: the refusals are the windows'."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P = 0x10000
    B, T, U1, V = 2, 4, 3, 5
    nws = L.rnnt_hip_joint_loss_window_workspace_bytes(B, T, U1, V)
    plain = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
    assert nws > plain and nws - plain <= 3 * 256 + 2 * 4 * B * U1 + 4 * B   # the band tables and the flags, each 256-aligned
    assert L.rnnt_hip_joint_loss_window_workspace_bytes(0, T, U1, V) == 0
    sep = (P, T * V, V, P, U1 * V, V, P, P, P, P, B, T, U1, V, 0)
    for lo, hi in ((None, P), (P, None), (None, None)):
        rc = L.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 1.0, 0.0, lo, hi, U1 - 1, P, P, P, P, nws, None)
        assert rc == -1 and b"emit_lo" in L.rnnt_hip_last_error()
        rc = L.rnnt_hip_loss_from_logits_fwd_bwd_window(P, 0, P, P, P, B, T, U1, V, 0, 1.0, 0.0, lo, hi, U1 - 1, P, P, P, nws, None)
        assert rc == -1 and b"emit_lo" in L.rnnt_hip_last_error()
    for stride in (0, -3, U1 - 2):
        rc = L.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 1.0, 0.0, P, P, stride, P, P, P, P, nws, None)
        assert rc == -1 and b"stride" in L.rnnt_hip_last_error()
        rc = L.rnnt_hip_loss_from_logits_fwd_bwd_window(P, 0, P, P, P, B, T, U1, V, 0, 1.0, 0.0, P, P, stride, P, P, P, nws, None)
        assert rc == -1 and b"stride" in L.rnnt_hip_last_error()
    # good windows (a wider table's stride too) pass that check: the next refusal is another argument's
    for stride in (U1 - 1, 17):
        rc = L.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 1.0, 0.0, P, P, stride, P, P, P, P, plain, None)
        assert rc == -1 and b"workspace" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_loss_fwd_bwd_window(*sep, 1.0, -1.0, P, P, U1 - 1, P, P, P, P, nws, None)
    assert rc == -1 and b"fastemit_lambda" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_loss_bwd_window(*sep, 1.0, 0.0, P, 1, P, P, P, plain, None)
    assert rc == -1 and b"workspace" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_loss_bwd_window(*sep, 1.0, 0.0, P, 2, P, P, P, nws, None)
    assert rc == -1 and b"gvec_stride" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_loss_from_logits_fwd_bwd_window(P, 7, P, P, P, B, T, U1, V, 0, 1.0, 0.0, P, P, U1 - 1, P, P, P, nws, None)
    assert rc == -1 and b"dtype" in L.rnnt_hip_last_error()
    # U = 0 (U1 = 1): the tables are still required and the stride still positive
    sep0 = (P, T * V, V, P, V, V, P, None, P, P, B, T, 1, V, 0)
    n0 = L.rnnt_hip_joint_loss_window_workspace_bytes(B, T, 1, V)
    assert L.rnnt_hip_joint_loss_fwd_bwd_window(*sep0, 1.0, 0.0, P, P, 0, P, P, P, P, n0, None) == -1
    assert b"stride" in L.rnnt_hip_last_error()


def test_plain_workspace_query_is_unchanged():
    """The plain entries' workspace is the sum of its 256-aligned parts, as before this feature."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    up = lambda n: (n + 255) // 256 * 256   # noqa: E731
    for B, T, U1, V in ((2, 4, 3, 5), (3, 65, 33, 129), (1, 31, 512, 129)):
        cells = B * T * U1
        want = 2 * up(cells * 8) + up(B * 16) + 2 * up(cells * 4) + up(B * ((T + 31) // 32) * U1 * V * 4)
        assert L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V) == want
