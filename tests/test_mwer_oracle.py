"""CPU side of MWER training: the float64 restatement of the risk against torch autograd and brute force, its
properties, the restated prefix-minimum edit distance against metrics.edit_distance, the three C entries' argument checks and the
python argument errors.  No device work."""
import itertools
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from rnntransducer_amd.metrics import edit_distance
from tests.mwer_restatement import edit_distance_prefix_min, risk_and_weights, risk_batch, risk_brute_force, risk_torch

EDGE_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511]


def _case(seed, N, spread=3.0, wmax=9):
    g = np.random.default_rng(seed)
    return g.uniform(1.0, 1.0 + spread, N), g.integers(0, wmax + 1, N)


@pytest.mark.parametrize("N,nvalid", [(2, 2), (4, 4), (4, 3), (5, 2), (8, 5), (64, 64), (64, 17)])
def test_restatement_equals_autograd_of_the_formula(N, nvalid):
    nll, W = _case(N * 100 + nvalid, N)
    valid = [True] * N
    for i in np.random.default_rng(N + nvalid).permutation(N)[:N - nvalid]:
        valid[i] = False
    risk, weights = risk_and_weights(nll, W, valid)
    x = torch.tensor(nll, dtype=torch.float64, requires_grad=True)
    out = risk_torch(x, torch.tensor(W), valid)
    out.backward()
    assert abs(out.item() - risk) < 1e-12
    assert np.abs(x.grad.numpy() - np.array(weights)).max() < 1e-12
    assert all(w == 0.0 for w, v in zip(weights, valid) if not v)
    assert abs(sum(weights)) < 1e-12                   # a softmax's gradient sums to zero


def test_restatement_equals_brute_force_on_hand_made_cases():
    # two hypotheses, equally likely: P = 1/2 each, Wbar = 2 -> risk 0; weights -1/2 (W - 2) = (+1, -1)
    risk, w = risk_and_weights([3.0, 3.0], [0, 4], [True, True])
    assert abs(risk) < 1e-15 and np.allclose(w, [1.0, -1.0], atol=1e-15)
    # P = (e^-1, e^-2) / (e^-1 + e^-2); risk = P0 (0 - 1) + P1 (2 - 1) = P1 - P0
    p0 = 1.0 / (1.0 + math.exp(-1.0))
    risk, w = risk_and_weights([1.0, 2.0], [0, 2], [True, True])
    assert abs(risk - ((1 - p0) - p0)) < 1e-15
    ew = 2 * (1 - p0)
    assert np.allclose(w, [-p0 * (0 - ew), -(1 - p0) * (2 - ew)], atol=1e-15)
    for seed in range(5):
        nll, W = _case(seed, 6)
        assert abs(risk_and_weights(nll, W, [True] * 6)[0] - risk_brute_force(list(nll), list(W))) < 1e-12
    # the finite-difference slope of the brute-force value is the weight
    nll, W = _case(11, 4)
    _, w = risk_and_weights(nll, W, [True] * 4)
    for j in range(4):
        hi, lo = nll.copy(), nll.copy()
        hi[j] += 1e-6
        lo[j] -= 1e-6
        assert abs((risk_brute_force(list(hi), list(W)) - risk_brute_force(list(lo), list(W))) / 2e-6 - w[j]) < 1e-8


def test_risk_properties():
    nll, W = _case(3, 5)
    valid = [True, True, False, True, True]
    risk, w = risk_and_weights(nll, W, valid)
    assert abs(risk) > 1e-3 and max(abs(x) for x in w) > 1e-3
    # a constant added to every nll of the utterance changes nothing
    risk2, w2 = risk_and_weights(nll + 123.25, W, valid)
    assert abs(risk2 - risk) < 1e-12 and np.abs(np.array(w2) - np.array(w)).max() < 1e-12
    # equal W: risk 0, zero weights
    risk3, w3 = risk_and_weights(nll, [4] * 5, valid)
    assert abs(risk3) < 1e-12 and max(abs(x) for x in w3) < 1e-12
    # one valid hypothesis (or none): 0 and 0
    for v in ([False, True, False, False, False], [False] * 5):
        assert risk_and_weights(nll, W, v) == (0.0, [0.0] * 5)
    # invalid rows carry nll = +inf: no NaN, weight exactly 0, the valid rows as without them
    inf_nll = np.where(valid, nll, np.inf)
    risk4, w4 = risk_and_weights(inf_nll, W, valid)
    assert risk4 == risk and w4 == w and w4[2] == 0.0 and not any(math.isnan(x) for x in w4)
    # an nll gap of 800: exp underflows to 0, everything stays finite
    risk5, w5 = risk_and_weights([2.0, 802.0, 5.0], [1, 7, 3], [True] * 3)
    assert math.isfinite(risk5) and all(math.isfinite(x) for x in w5) and w5[1] == 0.0
    p0 = 1.0 / (1.0 + math.exp(-3.0))
    assert abs(risk5 - (p0 * 1 + (1 - p0) * 3 - 11 / 3)) < 1e-12
    # the batched front is the per-utterance function row by row
    r, wb = risk_batch(np.stack([nll, nll + 1]), np.stack([W, W]), np.stack([valid, valid]))
    assert r.shape == (2,) and wb.shape == (2, 5) and abs(r[0] - risk) < 1e-12 and abs(r[1] - risk) < 1e-12


def test_prefix_minimum_row_update_is_the_edit_distance_exhaustive():
    seqs = [list(s) for n in range(7) for s in itertools.product((1, 2), repeat=n)]
    assert len(seqs) == 127
    for a in seqs:
        for b in seqs:
            assert edit_distance_prefix_min(a, b) == edit_distance(a, b), (a, b)


@pytest.mark.parametrize("alphabet", [2, 50])
def test_prefix_minimum_row_update_at_the_lane_edges(alphabet):
    g = np.random.default_rng(alphabet)
    for lh in EDGE_LENGTHS:
        for lr in EDGE_LENGTHS:
            a, b = g.integers(1, alphabet + 1, lh).tolist(), g.integers(1, alphabet + 1, lr).tolist()
            assert edit_distance_prefix_min(a, b) == edit_distance(a, b), (lh, lr)
    a = g.integers(1, alphabet + 1, 511).tolist()
    assert edit_distance_prefix_min(a, a) == 0
    assert edit_distance_prefix_min(a, [x + alphabet for x in a[:65]]) == 511


def test_symbols_are_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from rnntransducer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnnt_hip.h")).read()
    declared = set(re.findall(r"\b(rnnt_hip_\w+)\s*\(", header))
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnnt_hip_edit_distance", "rnnt_hip_nbest_pack", "rnnt_hip_mwer_risk"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name)
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    assert "mwer.hip" in __import__("rnntransducer_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    assert L.rnnt_hip_version() == _lib.ABI_VERSION


def test_entries_refuse_bad_arguments_on_the_host():
    """-1 with an error text, from addresses that are never dereferenced: nothing is launched."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P, Q = 0x10000, 0x20000

    def refused(rc, *words):
        msg = L.rnnt_hip_last_error()
        return rc == -1 and all(w in msg for w in words)
    ed = L.rnnt_hip_edit_distance
    assert refused(ed(None, 8, P, Q, 8, P, 1, 4, Q, None), b"edit_distance", b"null")
    assert refused(ed(P, 8, P, Q, 8, P, 1, 4, None, None), b"null")
    assert refused(ed(P, 8, P, Q, 8, P, 1, 0, Q, None), b"P = 0")
    assert refused(ed(P, 8, P, Q, 8, P, 0, 4, Q, None), b"ref_div = 0")
    assert refused(ed(P, 512, P, Q, 8, P, 1, 4, Q, None), b"511", b"hyp_ld = 512")
    assert refused(ed(P, 8, P, Q, 512, P, 1, 4, Q, None), b"511", b"ref_ld = 512")
    assert refused(ed(P, -1, P, Q, 8, P, 1, 4, Q, None), b"511")
    pk = L.rnnt_hip_nbest_pack
    assert refused(pk(None, 9, P, P, P, 2, 4, 8, 511, 0, Q, Q, Q, Q, Q, None), b"nbest_pack", b"null")
    assert refused(pk(P, 9, P, P, P, 2, 4, 8, 511, 0, Q, Q, Q, Q, None, None), b"null")
    assert refused(pk(P, 9, P, P, P, 2, 65, 8, 511, 0, Q, Q, Q, Q, Q, None), b"N = 65")
    assert refused(pk(P, 9, P, P, P, 0, 4, 8, 511, 0, Q, Q, Q, Q, Q, None), b"B = 0")
    assert refused(pk(P, 9, P, P, P, 2, 4, 512, 511, 0, Q, Q, Q, Q, Q, None), b"Umax = 512")
    assert refused(pk(P, 9, P, P, P, 2, 4, 8, 512, 0, Q, Q, Q, Q, Q, None), b"max_hyp_len = 512")
    assert refused(pk(P, 9, P, P, P, 2, 4, 8, 0, 0, Q, Q, Q, Q, Q, None), b"max_hyp_len = 0")
    assert refused(pk(P, 0, P, P, P, 2, 4, 8, 511, 0, Q, Q, Q, Q, Q, None), b"max_len")
    rk = L.rnnt_hip_mwer_risk
    assert refused(rk(None, P, P, 2, 4, 1.0, Q, Q, None), b"mwer_risk", b"null")
    assert refused(rk(P, P, P, 2, 4, 1.0, Q, None, None), b"null")
    assert refused(rk(P, P, P, 2, 65, 1.0, Q, Q, None), b"N = 65")
    assert refused(rk(P, P, P, 2, 0, 1.0, Q, Q, None), b"N = 0")
    assert refused(rk(P, P, P, 0, 4, 1.0, Q, Q, None), b"B = 0")
    assert refused(rk(P, P, P, 2, 4, math.inf, Q, Q, None), b"gscale")
    assert refused(rk(P, P, P, 2, 4, math.nan, Q, Q, None), b"gscale")


def test_python_wrappers_refuse_bad_arguments_before_the_device():
    from rnntransducer_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)   # noqa: E731
    with pytest.raises(ValueError, match="ref_div"):
        ops.edit_distance(i32(4, 3), i32(4), i32(4, 3), i32(4), ref_div=0)
    with pytest.raises(ValueError, match="do not match"):
        ops.edit_distance(i32(4, 3), i32(4), i32(3, 3), i32(3), ref_div=1)
    with pytest.raises(ValueError, match="511"):
        ops.edit_distance(i32(4, 512), i32(4), i32(4, 3), i32(4))
    with pytest.raises(ValueError, match="int32"):
        ops.edit_distance(torch.zeros(4, 3, dtype=torch.int64), i32(4), i32(4, 3), i32(4))
    with pytest.raises(ValueError, match="N must be"):
        ops.nbest_pack(i32(2, 65, 5), i32(2, 65), i32(2), i32(2), 4, 0)
    with pytest.raises(ValueError, match="max_hyp_len"):
        ops.nbest_pack(i32(2, 4, 5), i32(2, 4), i32(2), i32(2), 4, 0, max_hyp_len=512)
    with pytest.raises(ValueError, match="N must be"):
        ops.MwerRiskFn.apply(torch.zeros(8), i32(8), i32(8), 65)
    with pytest.raises(ValueError, match="reduction"):
        ops.MwerRiskFn.apply(torch.zeros(8), i32(8), i32(8), 4, "avg")
    with pytest.raises(ValueError, match="group"):
        ops.JointLossGroupedFn.apply(torch.zeros(3, 2, 4), torch.zeros(2, 4, 4), torch.zeros(5, 8), torch.zeros(5), i32(4, 1), i32(4),
                                     i32(4), 0, 0)
    host = torch.tensor([2, 1, 3, 9, 0, 2, 7, 7], dtype=torch.int32)       # counts (2) | lens (2, 3)
    assert ops.nbest_umax(host, 2, 3) == 8 and ops.nbest_umax(host, 2, 3, max_hyp_len=5) == 2
    assert ops.nbest_umax(torch.tensor([1, 1], dtype=torch.int32), 1, 1) == 1


def _cpu_model(**args):
    from rnntransducer_amd import RNNTransducer
    ns = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10, **args)
    return RNNTransducer(dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1),
                         dict(input_size=12, hidden_size=8, output_size=8, num_layers=1), dict(num_classes=10), ns)


@pytest.mark.parametrize("kw", [dict(nbest=0), dict(nbest=65), dict(nbest=2.0), dict(max_symbols=0), dict(max_symbols=5),
                                dict(max_hyp_len=0), dict(max_hyp_len=512), dict(mwer_weight=-0.5), dict(mwer_weight=math.inf),
                                dict(mwer_weight=math.nan), dict(token_min_logp=math.inf), dict(reduction="avg"),
                                dict(fastemit_lambda=-1.0)])
def test_mwer_loss_argument_errors_come_before_any_device_check(kw):
    net = _cpu_model().jointnet
    audio, texts = torch.zeros(2, 5, 12), torch.zeros(2, 3, dtype=torch.long)
    lens, targets = torch.tensor([5, 4], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        net.mwer_loss(audio, lens, texts, targets, torch.tensor([2, 1], dtype=torch.int32), 0, **kw)


def test_mwer_loss_on_a_cpu_model_fails_loudly_with_good_arguments():
    from rnntransducer_amd._lib import RnntHipError
    net = _cpu_model().jointnet
    with pytest.raises(RnntHipError):
        net.mwer_loss(torch.zeros(2, 5, 12), torch.tensor([5, 4], dtype=torch.int32), torch.zeros(2, 3, dtype=torch.long),
                      torch.zeros(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32), 0)


def test_transducer_args_fields():
    m = _cpu_model()
    assert (m.mwer_weight, m.mwer_nbest, m.mwer_max_symbols) == (0.0, 4, 1)
    m = _cpu_model(mwer_weight=0.25, mwer_nbest=8, mwer_max_symbols=2)
    assert (m.mwer_weight, m.mwer_nbest, m.mwer_max_symbols) == (0.25, 8, 2)
    for bad in (dict(mwer_weight=-1.0), dict(mwer_weight=math.nan), dict(mwer_nbest=0), dict(mwer_nbest=65),
                dict(mwer_max_symbols=5), dict(mwer_max_symbols=0)):
        with pytest.raises(ValueError):
            _cpu_model(**bad)
