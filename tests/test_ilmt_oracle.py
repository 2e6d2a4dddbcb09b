"""CPU side of internal-LM training (ILMT): the float64 restatement (tests/ilmt_restatement.py) against torch autograd
and a brute-force loop, the two C entries' declarations, bindings and host-side refusals, and the python surface's defaults and
argument errors.  Nothing here needs a GPU."""
import inspect
import math
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.ilmt_restatement import ilm_restatement


def _case(seed, U1, B, V, blank):
    g = np.random.default_rng(seed)
    C = torch.tensor(g.normal(size=(U1, B, V)) * 2.0)
    bias = torch.tensor(g.normal(size=(V,)))
    others = [v for v in range(V) if v != blank]
    labels = torch.tensor(g.choice(others, size=(B, U1 - 1)).reshape(B, U1 - 1), dtype=torch.long)
    u_lens = [int(g.integers(0, U1)) for _ in range(B)]
    u_lens[0] = U1 - 1
    gw = torch.tensor(g.normal(size=(B,)))
    return C, bias, labels, u_lens, gw


@pytest.mark.parametrize("U1,B,V,blank", [(1, 2, 5, 0), (4, 3, 7, 3), (6, 2, 3, 2), (3, 2, 2, 1), (5, 4, 70, 0)])
def test_restatement_equals_autograd_of_cross_entropy_on_the_non_blank_columns(U1, B, V, blank):
    C, bias, labels, u_lens, gw = _case(U1 * 100 + V, U1, B, V, blank)
    nll, dC, lse = ilm_restatement(C, bias, labels, u_lens, blank, gw)
    Ct = C.clone().requires_grad_(True)
    keep = torch.tensor([v for v in range(V) if v != blank])
    z = (Ct + bias)[..., keep]                                  # the blank column is gone: an ordinary (V-1)-way softmax
    remap = torch.full((V,), -1, dtype=torch.long)
    remap[keep] = torch.arange(V - 1)
    want = []
    for b in range(B):
        ub = u_lens[b]
        want.append(F.cross_entropy(z[:ub, b], remap[labels[b, :ub]], reduction="sum") if ub else z.sum() * 0.0)
    want = torch.stack(want)
    (want * gw).sum().backward()
    assert torch.allclose(nll, want.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dC, Ct.grad, rtol=1e-12, atol=1e-12)
    assert torch.all(dC[..., blank] == 0) and torch.all(dC[U1 - 1] == 0)
    for b in range(B):
        assert torch.all(dC[u_lens[b]:, b] == 0)
    assert torch.allclose(lse, torch.logsumexp(z.detach(), -1), rtol=1e-12, atol=1e-12)
    if V == 2:                                                  # one non-blank token: nothing to learn
        assert torch.all(nll == 0) and torch.all(dC == 0)


def test_the_differentiable_form_for_the_oracle_networks_equals_the_restatement():
    from tests.ilmt_restatement import ilm_nll_autograd
    U1, B, V, blank = 5, 3, 9, 4
    C, bias, labels, u_lens, gw = _case(2, U1, B, V, blank)
    nll, dC, _ = ilm_restatement(C, bias, labels, u_lens, blank, gw)
    Ct, bt = C.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    got = ilm_nll_autograd(Ct, bt, labels, u_lens, blank)
    (got * gw).sum().backward()
    assert torch.allclose(got.detach(), nll, rtol=1e-12, atol=1e-12) and torch.allclose(Ct.grad, dC, rtol=1e-12, atol=1e-12)
    assert torch.allclose(bt.grad, dC.sum((0, 1)), rtol=1e-12, atol=1e-12)   # z = C + bias: the bias gradient is dC's column sums


def test_restatement_equals_a_brute_force_loop():
    U1, B, V, blank = 4, 3, 6, 2
    C, bias, labels, u_lens, gw = _case(11, U1, B, V, blank)
    nll, dC, _ = ilm_restatement(C, bias, labels, u_lens, blank, gw)
    for b in range(B):
        tot = 0.0
        for u in range(U1):
            zs = {v: float(C[u, b, v]) + float(bias[v]) for v in range(V) if v != blank}
            den = sum(math.exp(x) for x in zs.values())
            for v in range(V):
                want = 0.0
                if u < u_lens[b] and v != blank:
                    want = float(gw[b]) * (math.exp(zs[v]) / den - (1.0 if v == int(labels[b, u]) else 0.0))
                assert abs(float(dC[u, b, v]) - want) < 1e-12
            if u < u_lens[b]:
                tot += math.log(den) - zs[int(labels[b, u])]
        assert abs(float(nll[b]) - tot) < 1e-12


@pytest.mark.parametrize("bad", ["blank", "V", -1])
def test_restatement_infeasible_rows(bad):
    U1, B, V, blank = 4, 3, 6, 2
    C, bias, labels, u_lens, gw = _case(5, U1, B, V, blank)
    u_lens = [3, 2, 2]
    ref_nll, ref_dC, _ = ilm_restatement(C, bias, labels, u_lens, blank, gw)
    labels = labels.clone()
    value = {"blank": blank, "V": V, -1: -1}[bad]
    labels[1, 1] = value                                        # counted: row 1 is infeasible
    labels[2, 2] = value                                        # padding (u_lens[2] = 2): never looked at
    nll, dC, _ = ilm_restatement(C, bias, labels, u_lens, blank, gw)
    assert torch.isposinf(nll[1]) and torch.all(dC[:, 1] == 0) and torch.isfinite(ref_nll[1])
    for b in (0, 2):
        assert nll[b] == ref_nll[b] and torch.equal(dC[:, b], ref_dC[:, b])


def test_symbols_are_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc import build
    build.build()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnnt_hip.h")).read()
    declared = set(re.findall(r"\b(rnnt_hip_\w+)\s*\(", header))
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnnt_hip_ilm_loss_fwd", "rnnt_hip_ilm_loss_bwd"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name)
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1] and getattr(L, name).restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["rnnt_hip_ilm_loss_fwd"][1]) == 13 and len(_lib.SYMBOLS["rnnt_hip_ilm_loss_bwd"][1]) == 17
    assert "ilm_loss.hip" in build.SOURCES
    assert L.rnnt_hip_version() == _lib.ABI_VERSION == 4


def test_entries_refuse_bad_arguments_on_the_host():
    """-1 with an error text, from addresses that are never dereferenced: nothing is launched."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P, Q = 0x10000, 0x20000

    def refused(rc, *words):
        msg = L.rnnt_hip_last_error()
        return rc == -1 and all(w in msg for w in words)

    def fwd(C=P, c_sb=8, c_su=24, bias=P, labels=Q, u_lens=Q, B=3, U1=4, V=8, blank=0, nll=Q, lse=None):
        return L.rnnt_hip_ilm_loss_fwd(C, c_sb, c_su, bias, labels, u_lens, B, U1, V, blank, nll, lse, None)

    def bwd(C=P, c_sb=8, c_su=24, bias=P, labels=Q, u_lens=Q, lse=None, B=3, U1=4, V=8, blank=0, gvec=None, dC=Q):
        return L.rnnt_hip_ilm_loss_bwd(C, c_sb, c_su, bias, labels, u_lens, lse, B, U1, V, blank, 1.0, gvec, 0, 0, dC, None)

    for fn, what, out in ((fwd, b"ilm_loss_fwd", "nll"), (bwd, b"ilm_loss_bwd", "dC")):
        for ptr in ("C", "bias", "labels", "u_lens", out):
            assert refused(fn(**{ptr: None}), what, b"null"), (what, ptr)
        assert refused(fn(B=0), what, b"B = 0")
        assert refused(fn(U1=0), what, b"U1 = 0")
        assert refused(fn(V=1), what, b"V = 1")
        assert refused(fn(V=0), what, b"V = 0")
        assert refused(fn(blank=-1), what, b"blank -1")
        assert refused(fn(blank=8), what, b"blank 8")
        assert refused(fn(c_sb=32, c_su=7), what, b"c_su = 7")


def test_weight_defaults():
    from rnntransducer_amd import JointNet, RNNTransducer
    from rnntransducer_amd.ops import IlmLossFn, JointLossFn
    assert inspect.signature(JointNet.loss).parameters["ilmt_weight"].default == 0.0
    assert inspect.signature(JointLossFn.forward).parameters["ilmt_weight"].default == 0.0
    assert list(inspect.signature(JointLossFn.forward).parameters)[-1] == "ilmt_weight"
    assert list(inspect.signature(IlmLossFn.forward).parameters)[1:] == ["dec", "W", "bias", "labels", "u_lens", "blank", "want_grad",
                                                                         "reduction"]
    assert inspect.signature(JointNet.ilm_loss).parameters["reduction"].default == "none"
    assert inspect.signature(RNNTransducer.ilm_loss).parameters["reduction"].default == "mean"
    m = _cpu_model()
    assert m.ilmt_weight == 0.0 and isinstance(m.ilmt_weight, float)
    assert _cpu_model(ilmt_weight=0.2).ilmt_weight == 0.2 and _cpu_model(ilmt_weight=None).ilmt_weight == 0.0
    import rnntransducer_amd
    assert not any("ilm" in n.lower() for n in rnntransducer_amd.__all__)


def _cpu_model(**args):
    from rnntransducer_amd import RNNTransducer
    ns = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10, **args)
    return RNNTransducer(dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1),
                         dict(input_size=12, hidden_size=8, output_size=8, num_layers=1), dict(num_classes=10), ns)


@pytest.mark.parametrize("bad", [-0.1, math.nan, math.inf, -math.inf, "0.2", True])
def test_bad_weights_raise_before_any_device_check(bad):
    from rnntransducer_amd.ops import check_ilmt_weight
    with pytest.raises(ValueError, match="ilmt_weight"):
        check_ilmt_weight(bad)
    with pytest.raises(ValueError, match="ilmt_weight"):
        _cpu_model(ilmt_weight=bad)
    net = _cpu_model().jointnet
    with pytest.raises(ValueError, match="ilmt_weight"):     # CPU tensors: the weight is refused before the missing GPU is noticed
        net.loss(torch.zeros(2, 5, 12), torch.tensor([5, 4], dtype=torch.int32), torch.zeros(2, 3, dtype=torch.long),
                 torch.zeros(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32), 0, ilmt_weight=bad)


def test_good_weights_pass_and_the_cpu_model_fails_loudly():
    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.ops import check_ilmt_weight
    assert check_ilmt_weight(0) == 0.0 and check_ilmt_weight(0.25) == 0.25 and check_ilmt_weight(3) == 3.0
    net = _cpu_model().jointnet
    with pytest.raises(RnntHipError):                         # no CPU / eager fallback for the text-only loss either
        net.ilm_loss(torch.zeros(2, 3, dtype=torch.long), torch.ones(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="reduction"):
        net.ilm_loss(torch.zeros(2, 3, dtype=torch.long), torch.ones(2, 2, dtype=torch.int32), [2, 1], 0, reduction="avg")
    with pytest.raises(ValueError, match="blank"):
        net.ilm_loss(torch.zeros(2, 3, dtype=torch.long), torch.ones(2, 2, dtype=torch.int32), [2, 1], 10)
    with pytest.raises(ValueError, match="input_texts"):
        net.ilm_loss(torch.zeros(2, 2, dtype=torch.long), torch.ones(2, 2, dtype=torch.int32), [2, 1], 0)


def test_mwer_and_ilmt_weights_do_not_combine():
    with pytest.raises(ValueError, match="ilmt_weight"):
        _cpu_model(mwer_weight=0.5, ilmt_weight=0.2)
    assert _cpu_model(mwer_weight=0.5, ilmt_weight=0.0).mwer_weight == 0.5
    assert _cpu_model(mwer_weight=0.0, ilmt_weight=0.2).ilmt_weight == 0.2
