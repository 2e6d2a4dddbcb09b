"""Lattice knowledge distillation on the CPU: the float64 restatement tests/kd_restatement.py against torch autograd through the
materialised collapsed KL, the properties of the term, and every refusal that needs no device (the C ABI's with stand-in addresses
that are never dereferenced, the python surface's on CPU tensors)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import kd_restatement as kr

# (B, T, U1, V, blank, t_lens, u_lens)
TINY = [
    (2, 5, 4, 7, 0, [5, 3], [3, 1]),
    (3, 4, 3, 3, 1, [4, 1, 2], [2, 0, 1]),      # V = 3: the rest class is one entry with a label, two without; t_len 1; u_len 0
    (1, 1, 1, 4, 3, [1], [0]),                  # a single cell, no label row at all
    (2, 6, 5, 9, 8, [6, 6], [4, 0]),
]


def _problem(B, T, U1, V, blank, seed, scale=1.5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(B, T, V)) * scale
    C = rng.normal(size=(B, U1, V)) * scale
    bias = rng.normal(size=V) * 0.1
    others = np.array([v for v in range(V) if v != blank])
    y = others[rng.integers(0, others.size, size=(B, max(U1 - 1, 0)))].astype(np.int32)
    return A, C, bias, y


@pytest.mark.parametrize("case", TINY, ids=[f"T{c[1]}-U1_{c[2]}-V{c[3]}" for c in TINY])
def test_restatement_matches_autograd_of_the_materialised_kl(case):
    B, T, U1, V, blank, t_lens, u_lens = case
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=V)
    At, Ct, bt, _ = _problem(B, T, U1, V, blank, seed=V + 100)
    teacher = kr.cell_planes(At, Ct, bt, y, u_lens, blank)
    ref_kd, ref_dA, ref_dC = kr.kd_materialised_autograd(A, C, bias, y, t_lens, u_lens, blank, teacher)
    got = kr.kd_fused(A, C, bias, y, t_lens, u_lens, blank, teacher, [0.0] * B, [1.0] * B)
    np.testing.assert_allclose(got["kd"], ref_kd, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got["dA"], ref_dA, rtol=0, atol=1e-13)
    np.testing.assert_allclose(got["dC"], ref_dC, rtol=0, atol=1e-13)
    assert np.all(got["kd"] >= 0) and np.all(got["kd"] > 0)
    for b in range(B):                                   # exact zeros outside the lattice
        assert np.all(got["dA"][b, t_lens[b]:] == 0) and np.all(got["dC"][b, u_lens[b] + 1:] == 0)
    assert np.all(got["S_A"] >= np.abs(got["dA"]) - 1e-15) and np.all(got["S_C"] >= np.abs(got["dC"]) - 1e-15)
    # the three collapsed probabilities of a cell sum to 1
    s = got["planes"]
    for b in range(B):
        ub = u_lens[b]
        tot = np.exp(s[0][b, :ub + 1]) + np.exp(s[2][b, :ub + 1])
        tot[:ub] += np.exp(s[1][b, :ub])
        np.testing.assert_allclose(tot, 1.0, atol=1e-14)


def test_three_scalar_form_is_the_gradient():
    """dz[v] = w p[v] - [v = blank] cb - [v = y] ce with w = 1 - rho, cb = a - rho p_b, ce = c - rho p_y (the form the kernels'
    scalars take) is what the restatement evaluates as p - q."""
    B, T, U1, V, blank = 1, 3, 3, 6, 2
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=1)
    At, Ct, bt, _ = _problem(B, T, U1, V, blank, seed=2)
    teacher = kr.cell_planes(At, Ct, bt, y, [2], blank)
    student = kr.cell_planes(A, C, bias, y, [2], blank)
    lp = kr.fr.log_softmax(A[0][:, None, :] + C[0][None, :, :] + bias)
    dz = kr.kd_cell_gradient(lp, y[0].astype(np.int64), 3, 2, blank, teacher[0][0], teacher[1][0], teacher[2][0])
    p = np.exp(lp)
    for u in range(3):
        for t in range(3):
            rho = np.exp(teacher[2][0, u, t] - student[2][0, u, t])
            g = p[t, u] * (1.0 - rho)
            g[blank] -= np.exp(teacher[0][0, u, t]) - rho * np.exp(student[0][0, u, t])
            if u < 2:
                g[y[0, u]] -= np.exp(teacher[1][0, u, t]) - rho * np.exp(student[1][0, u, t])
            np.testing.assert_allclose(g, dz[t, u], atol=1e-14)
            assert abs(dz[t, u].sum()) < 1e-14       # sum over v: 0, as for the transducer term


def test_teacher_equal_to_student_gives_zero():
    B, T, U1, V, blank, t_lens, u_lens = TINY[0]
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=5)
    own = kr.cell_planes(A, C, bias, y, u_lens, blank)
    got = kr.kd_fused(A, C, bias, y, t_lens, u_lens, blank, own, [0.0] * B, [1.0] * B)
    assert np.all(np.abs(got["kd"]) < 1e-13) and np.abs(got["dA"]).max() < 1e-14 and np.abs(got["dC"]).max() < 1e-14


def test_a_teacher_class_of_probability_zero_contributes_nothing():
    B, T, U1, V, blank, t_lens, u_lens = TINY[0]
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=6)
    own = kr.cell_planes(A, C, bias, y, u_lens, blank)
    teacher = tuple(x.copy() for x in own)
    teacher[1][:] = -np.inf                               # the teacher never emits the label
    kd, mag = kr.kd_value(own, teacher, t_lens, u_lens)
    assert np.all(np.isfinite(kd)) and np.all(np.abs(kd) < 1e-13)


def test_library_refuses_bad_kd_calls_before_any_device_work():
    """The three KD entries with stand-in addresses: every call below is a refused one, so nothing reaches a launch."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P = 0x10000
    B, T, U1, V = 2, 4, 3, 5
    plain, need = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V), L.rnnt_hip_joint_loss_kd_workspace_bytes(B, T, U1, V)
    assert need == plain + 256 * -(-(B * T * U1 * 4) // 256)          # the plain layout, then the student's rest plane
    assert L.rnnt_hip_joint_loss_kd_workspace_bytes(0, T, U1, V) == 0 and L.rnnt_hip_joint_loss_kd_workspace_bytes(B, T, U1, -1) == 0
    sep = dict(A=P, a_sb=T * V, a_st=V, C=P, c_sb=U1 * V, c_su=V, bias=P, labels=P, t_lens=P, u_lens=P, B=B, T=T, U1=U1, V=V, blank=0)
    fwd = dict(sep, gscale=1.0, lam=0.0, t_blk=P, t_emit=P, t_rest=P, kd_gscale=1.0, nll=P, kd=P, dA=P, dC=P, workspace=P,
               workspace_bytes=need, stream=None)
    bwd = dict(sep, gscale=1.0, lam=0.0, gvec=P, gvec_stride=1, t_blk=P, t_emit=P, t_rest=P, kd_gscale=1.0, kd_gvec=P, kd_gvec_stride=1,
               dA=P, dC=P, workspace=P, workspace_bytes=need, stream=None)
    planes = dict(sep, blk=P, emit=P, rest=P, stream=None)
    common = [{"V": 2}, {"V": 1, "blank": 0}, {"A": None}, {"bias": None}, {"u_lens": None}, {"labels": None}, {"B": 0}, {"T": -1},
              {"blank": 5}, {"blank": -1}, {"U1": 513}]
    loss_only = [{"t_blk": None}, {"t_emit": None}, {"t_rest": None}, {"workspace_bytes": need - 1}, {"workspace_bytes": plain},
                 {"workspace": None}, {"lam": -1.0}, {"lam": float("nan")}, {"kd_gscale": float("inf")}, {"kd_gscale": float("nan")}]
    table = [
        (L.rnnt_hip_joint_loss_fwd_bwd_kd, fwd, common + loss_only + [{"kd": None}, {"nll": None}, {"dA": None}, {"dC": None}]),
        (L.rnnt_hip_joint_loss_bwd_kd, bwd, common + loss_only + [{"kd_gvec_stride": 2}, {"kd_gvec_stride": -1}, {"gvec_stride": 2},
                                                                  {"dA": None}, {"dC": None}]),
        (L.rnnt_hip_joint_cell_logprobs, planes, common + [{"blk": None}, {"emit": None}, {"rest": None}]),
    ]
    calls = 0
    for entry, good, bad in table:
        for over in bad:
            args = {**good, **over}
            assert entry(*args.values()) == -1, (entry.__name__, over)
            assert L.rnnt_hip_last_error(), (entry.__name__, over)
            calls += 1
    assert calls == 25 + 26 + 14
    assert b"V >= 3" in (L.rnnt_hip_joint_cell_logprobs(*{**planes, "V": 2}.values()), L.rnnt_hip_last_error())[1]
    assert b"teacher" in (L.rnnt_hip_joint_loss_fwd_bwd_kd(*{**fwd, "t_rest": None}.values()), L.rnnt_hip_last_error())[1]


def test_python_surface_refuses_bad_kd_arguments():
    from rnntransducer_amd import ops
    for bad in (-0.1, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError):
            ops.check_kd_weight(bad)
    assert ops.check_kd_weight(0) == 0.0 and ops.check_kd_weight(0.5) == 0.5
    B, U1, T, V = 2, 3, 4, 5
    good = ops.CellLogProbs(*(torch.zeros(B, U1, T) for _ in range(3)))
    assert ops.check_kd_teacher(None, B, U1, T, V, "cpu") is None
    assert isinstance(ops.check_kd_teacher(good, B, U1, T, V, "cpu"), ops.CellLogProbs)
    with pytest.raises(ValueError, match="emit_windows"):
        ops.check_kd_teacher(good, B, U1, T, V, "cpu", emit_windows=(torch.zeros(B, U1 - 1), torch.zeros(B, U1 - 1)))
    with pytest.raises(ValueError, match="at least 3"):
        ops.check_kd_teacher(good, B, U1, T, 2, "cpu")
    for bad in (good[:2], ops.CellLogProbs(good.blk, good.emit, torch.zeros(B, T, U1)),
                ops.CellLogProbs(good.blk, good.emit.double(), good.rest), ops.CellLogProbs(good.blk, good.emit, None),
                ops.CellLogProbs(good.blk, good.emit, torch.zeros(B, U1, T, device="meta")), "planes"):
        with pytest.raises(ValueError):
            ops.check_kd_teacher(bad, B, U1, T, V, "cpu")


def _model(V=9, bidirectional=False, **args):
    from rnntransducer_amd import RNNTransducer
    tn = dict(input_size=12, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=bidirectional)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)
    return RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), Namespace(move_metrics_to_cpu=False, **args))


def test_model_level_refusals_and_the_teacher_stays_outside_the_module_tree():
    for bad in (dict(kd_weight=-1.0), dict(kd_weight=float("nan")), dict(kd_weight=0.5, ar_left=1, ar_right=1),
                dict(kd_weight=0.5, mwer_weight=0.5)):
        with pytest.raises(ValueError):
            _model(**bad)
    student, teacher = _model(kd_weight=0.5), _model(bidirectional=True)
    keys, nparam = list(student.state_dict().keys()), len(list(student.parameters()))
    assert student.set_teacher(teacher) is student
    assert list(student.state_dict().keys()) == keys and len(list(student.parameters())) == nparam
    assert all(m is not teacher and m is not teacher.jointnet for m in student.modules())
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    student.train()
    assert not teacher.training                          # the student's mode changes do not reach it
    with pytest.raises(ValueError, match="vocabulary"):
        student.set_teacher(_model(V=10))
    with pytest.raises(ValueError):
        student.set_teacher(student)
    with pytest.raises(ValueError):
        student.set_teacher(teacher.jointnet)
    student.set_teacher(None)
    batch = (torch.zeros(2, 6, 12), [6, 6], torch.tensor([6, 6], dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int64), [4, 4],
             torch.ones(2, 3, dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match="set_teacher"):
        student.training_step(batch, 0)                  # kd_weight > 0 without a teacher: refused at the first step
