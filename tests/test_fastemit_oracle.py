"""FastEmit regularisation, CPU side: the float64 restatement the GPU tests compare against (tests/fastemit_restatement.py) is itself
checked against the C oracle at lambda = 0 and against torch-fp64 autograd of the surrogate loss at lambda > 0; the host-side
pieces of the feature (metrics.emission_delay, argument validation in python and in the C ABI) are checked here too."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle.rnnt_oracle import rnnt_loss_c
from tests import fastemit_restatement as fr

# (B, T, U+1, V, blank, t_lens, u_lens): ragged, one row without labels
SHAPES = [
    (3, 5, 4, 6, 0, [5, 3, 1], [3, 1, 0]),
    (2, 7, 3, 5, 4, [7, 6], [2, 0]),
    (2, 4, 6, 9, 3, [4, 2], [5, 4]),
]
IDS = [f"T{s[1]}-U1_{s[2]}-V{s[3]}" for s in SHAPES]


def _draw(B, T, U1, V, blank, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(B, T, U1, V)) * 1.5
    others = np.array([v for v in range(V) if v != blank])
    y = others[rng.integers(0, others.size, size=(B, U1 - 1))].astype(np.int32)
    return z, y


def _torch_nll(lp, y, Tb, Ub, blank):
    """Plain DP in torch: -log P(y|x) from the log-softmax lp (T,U+1,V), differentiable; also returns the emit terms it used."""
    emit = [[lp[t, u, int(y[u])] for u in range(Ub)] for t in range(Tb)]
    neg = torch.tensor(-math.inf, dtype=torch.float64)
    alpha = [[neg] * (Ub + 1) for _ in range(Tb)]
    alpha[0][0] = torch.zeros((), dtype=torch.float64)
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t][u - 1] + emit[t][u - 1])
            alpha[t][u] = torch.logsumexp(torch.stack(terms), 0)
    return -(alpha[Tb - 1][Ub] + lp[Tb - 1, Ub, blank]), emit


def _surrogate_grad(z, y, t_lens, u_lens, blank, lam):
    """d/dz of  NLL_b + lam * sum_{t,u} stopgrad(ce[t,u]) * (-emit(t,u)),  ce = -d NLL / d emit taken by autograd and detached."""
    out = np.zeros_like(z)
    for b in range(z.shape[0]):
        Tb, Ub = t_lens[b], u_lens[b]
        zb = torch.tensor(z[b], dtype=torch.float64, requires_grad=True)
        lp = torch.log_softmax(zb, -1)
        nll, emit = _torch_nll(lp, y[b], Tb, Ub, blank)
        loss = nll
        flat = [e for row in emit for e in row]
        if flat:
            ce = torch.autograd.grad(nll, flat, retain_graph=True)      # = -ce
            loss = nll + lam * sum((-c).detach() * (-e) for c, e in zip(ce, flat))
        loss.backward()
        out[b] = zb.grad.numpy()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_equals_the_oracle_without_fastemit(shape):
    B, T, U1, V, blank, t_lens, u_lens = shape
    z, y = _draw(B, T, U1, V, blank, seed=T * 100 + V)
    nll, dz = fr.fastemit_loss(z, y, t_lens, u_lens, blank, 0.0)
    ref_nll, ref_dz = rnnt_loss_c(z, y, t_lens, u_lens, blank)
    np.testing.assert_allclose(nll, ref_nll, rtol=1e-12)
    assert np.abs(dz - ref_dz).max() < 1e-12


@pytest.mark.parametrize("lam", [0.01, 0.7, 2.0])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_equals_autograd_of_the_surrogate(shape, lam):
    B, T, U1, V, blank, t_lens, u_lens = shape
    z, y = _draw(B, T, U1, V, blank, seed=T * 100 + V + 1)
    nll, dz = fr.fastemit_loss(z, y, t_lens, u_lens, blank, lam)
    nll0, dz0 = fr.fastemit_loss(z, y, t_lens, u_lens, blank, 0.0)
    assert np.array_equal(nll, nll0)                                  # the value is the unregularised NLL
    want = _surrogate_grad(z, y, t_lens, u_lens, blank, lam)
    assert np.abs(dz - want).max() < 1e-12
    assert np.abs(dz.sum(-1)).max() < 1e-12                           # row sums over v vanish in every cell
    assert np.abs(dz - dz0).max() > 1e-3                              # and lambda does something
    for b, ub in enumerate(u_lens):
        if ub == 0:
            assert np.array_equal(dz[b], dz0[b])                      # no label transition: exactly the plain gradient


def test_fused_form_sums_the_dense_gradient():
    B, T, U1, V, blank, t_lens, u_lens = SHAPES[0]
    rng = np.random.default_rng(5)
    A, C, bias = rng.normal(size=(B, T, V)), rng.normal(size=(B, U1, V)), rng.normal(size=V)
    _, y = _draw(B, T, U1, V, blank, seed=6)
    gw = [0.5, -1.5, 2.0]
    nll, dA, dC = fr.fastemit_fused(A, C, bias, y, t_lens, u_lens, blank, 0.7, gw)
    z = A[:, :, None, :] + C[:, None, :, :] + bias
    nll2, dz = fr.fastemit_loss(z, y, t_lens, u_lens, blank, 0.7)
    g = np.asarray(gw).reshape(-1, 1, 1, 1)
    np.testing.assert_allclose(nll, nll2, rtol=1e-14)
    assert np.abs(dA - (dz * g).sum(2)).max() < 1e-13 and np.abs(dC - (dz * g).sum(1)).max() < 1e-13


def test_restatement_zero_length_row():
    B, T, U1, V, blank, _, _ = SHAPES[0]
    z, y = _draw(B, T, U1, V, blank, seed=9)
    nll, dz = fr.fastemit_loss(z, y, [5, 0, 2], [3, 2, 1], blank, 0.5)
    assert np.isposinf(nll[1]) and np.all(dz[1] == 0) and np.isfinite(nll[[0, 2]]).all()


def test_emission_delay():
    from rnntransducer_amd.metrics import emission_delay
    frames = torch.tensor([[3, 5, 9, -1], [2, 2, -1, -1]], dtype=torch.int32)
    ref = torch.tensor([[1, 5, 4, 8], [4, -1, -1, -1]], dtype=torch.int32)
    # valid in both: (3,1) (5,5) (9,4) (2,4) -> differences 2, 0, 5, -2
    d = emission_delay(frames, ref)
    assert d["count"] == 4
    assert d["mean"] == pytest.approx(1.25) and d["median"] == pytest.approx(1.0)
    assert d["p90"] == pytest.approx(float(np.percentile([2, 0, 5, -2], 90)))
    # unequal widths: the narrower table counts as padded; lists and arrays are taken too
    d2 = emission_delay(frames[:, :2].tolist(), ref.numpy())
    assert d2["count"] == 3 and d2["mean"] == pytest.approx((2 + 0 - 2) / 3)
    same = emission_delay(ref, ref)
    assert same["count"] == 5 and same["mean"] == 0.0 and same["median"] == 0.0 and same["p90"] == 0.0
    none = emission_delay(torch.full((2, 3), -1), ref[:, :3])
    assert none["count"] == 0 and math.isnan(none["mean"]) and math.isnan(none["median"]) and math.isnan(none["p90"])
    with pytest.raises(ValueError):
        emission_delay(frames, ref[:1])
    with pytest.raises(ValueError):
        emission_delay(frames[0], ref[0])


def _tiny_model_args():
    prednet = dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1)
    transnet = dict(input_size=12, hidden_size=8, output_size=12, num_layers=1)
    return prednet, transnet, dict(num_classes=10)


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), -float("inf")])
def test_python_surface_rejects_a_bad_lambda(bad):
    from rnntransducer_amd import RNNTLoss, RNNTransducer
    from rnntransducer_amd.ops import check_fastemit_lambda
    with pytest.raises(ValueError, match="fastemit_lambda"):
        RNNTLoss(blank=0, reduction="mean", fastemit_lambda=bad)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        check_fastemit_lambda(bad)
    prednet, transnet, joint = _tiny_model_args()
    with pytest.raises(ValueError, match="fastemit_lambda"):
        RNNTransducer(prednet, transnet, joint, Namespace(fastemit_lambda=bad))


def test_python_surface_defaults_and_accepts_a_good_lambda():
    from rnntransducer_amd import RNNTLoss, RNNTransducer
    assert RNNTLoss().fastemit_lambda == 0.0 and RNNTLoss(0, "sum", 0.25).fastemit_lambda == 0.25
    prednet, transnet, joint = _tiny_model_args()
    assert RNNTransducer(prednet, transnet, joint, Namespace()).fastemit_lambda == 0.0
    m = RNNTransducer(prednet, transnet, joint, Namespace(fastemit_lambda=0.01))
    assert m.fastemit_lambda == 0.01 and m.rnnt_loss.fastemit_lambda == 0.01


def test_abi_rejects_a_bad_lambda_before_any_device_work():
    """Every other argument is acceptable and the pointers are stand-ins that are never dereferenced: the refusal is lambda's."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P = 0x10000
    B, T, U1, V = 2, 4, 3, 5
    nws = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
    sep = (P, T * V, V, P, U1 * V, V, P, P, P, P, B, T, U1, V, 0)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        rc = L.rnnt_hip_joint_loss_fwd_bwd_fastemit(*sep, 1.0, bad, P, P, P, P, nws, None)
        assert rc == -1 and b"fastemit_lambda" in L.rnnt_hip_last_error()
        rc = L.rnnt_hip_joint_loss_fwd_bwd_fastemit(*sep, 1.0, bad, P, None, None, P, nws, None)      # the forward-only call too
        assert rc == -1 and b"fastemit_lambda" in L.rnnt_hip_last_error()
        rc = L.rnnt_hip_joint_loss_bwd_fastemit(*sep, 1.0, bad, P, 1, P, P, P, nws, None)
        assert rc == -1 and b"fastemit_lambda" in L.rnnt_hip_last_error()
        for dtype in (0, 1, 2):
            rc = L.rnnt_hip_loss_from_logits_fwd_bwd_fastemit(P, dtype, P, P, P, B, T, U1, V, 0, 1.0, bad, P, P, P, nws, None)
            assert rc == -1 and b"fastemit_lambda" in L.rnnt_hip_last_error()
    # a good lambda passes that check: the next refusal is another argument's
    rc = L.rnnt_hip_joint_loss_fwd_bwd_fastemit(*sep, 1.0, 0.5, P, P, P, P, nws - 1, None)
    assert rc == -1 and b"workspace" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_loss_bwd_fastemit(*sep, 1.0, 0.5, P, 2, P, P, P, nws, None)
    assert rc == -1 and b"gvec_stride" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_loss_from_logits_fwd_bwd_fastemit(P, 7, P, P, P, B, T, U1, V, 0, 1.0, 0.5, P, P, P, nws, None)
    assert rc == -1 and b"dtype" in L.rnnt_hip_last_error()
