"""CPU-side checks of the forced alignment: the float64 restatement (tests/align_restatement.py) against brute force on every tiny
lattice, the tie rule on constructed exact ties, and the C ABI / python surface of the feature (symbols, argument validation before
any device work, loud failure on CPU tensors).  No GPU here."""
import ctypes
import os
import re
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_restatement as ar  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rnnt_hip_joint_align_workspace_bytes", "rnnt_hip_joint_align", "rnnt_hip_align_from_logits_ex")


def _random_lattice(rng, T, U, kind):
    if kind == "real":      # log-softmax of random logits: no ties
        V = 5
        labels = rng.integers(1, V, size=U)
        return ar.lattice(rng.normal(size=(T, U + 1, V)) * 2.0, labels, 0)
    # small negative integers: every path score is an exact float64 sum, ties are frequent and exact
    blk = -rng.integers(0, 3 if kind == "ties" else 9, size=(T, U + 1)).astype(np.float64)
    emit = -rng.integers(0, 3 if kind == "ties" else 9, size=(T, U + 1)).astype(np.float64)
    emit[:, U] = 0.0
    return blk, emit


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("U", [0, 1, 2, 3, 4])
def test_restatement_equals_brute_force(T, U):
    rng = np.random.default_rng(100 * T + U)
    tied = 0
    for kind in ("real", "int", "ties"):
        for _ in range(12):
            blk, emit = _random_lattice(rng, T, U, kind)
            frames, best, M = ar.viterbi(blk, emit, T, U)
            want, wbest, second = ar.brute_force(blk, emit, T, U)
            mg = ar.margin(frames, best, M)
            assert len(frames) == U and all(0 <= f < T for f in frames) and frames == sorted(frames)
            if kind == "real":
                assert abs(best - wbest) <= 1e-12 * max(1.0, abs(wbest))
                assert abs(ar.path_score(blk, emit, frames, T) - best) <= 1e-12 * max(1.0, abs(best))
                if wbest - second > 1e-9:
                    assert frames == want
                if np.isfinite(second):
                    assert abs(mg - (wbest - second)) <= 1e-9
                else:
                    assert mg == np.inf
            else:           # exact arithmetic: everything is equal to the bit, the tie-broken path included
                assert best == wbest and frames == want
                assert ar.path_score(blk, emit, frames, T) == best
                assert mg == wbest - second
                tied += int(mg == 0.0)
    if T >= 2 and U >= 1:
        assert tied > 0, "the integer lattices were meant to contain exact ties"


def test_tie_rule_blank_predecessor_wins():
    # all-zero lattice: every path scores 0.  Walking back from (T-1, U) the blank predecessor is taken while there is one, so
    # every label lands on frame 0 (only there is the label predecessor strictly greater: the blank one does not exist).
    T, U = 4, 3
    blk, emit = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    frames, best, M = ar.viterbi(blk, emit, T, U)
    assert frames == [0, 0, 0] and best == 0.0 and ar.margin(frames, best, M) == 0.0
    assert ar.brute_force(blk, emit, T, U)[0] == [0, 0, 0]
    # one label, two frames, the two paths tie exactly: emit at frame 0 then blank, blank (-1 -1 -1), or blank, emit at frame 1, blank
    blk = np.array([[-1.0, -1.0], [-5.0, -1.0]])
    emit = np.array([[-1.0, 0.0], [-1.0, 0.0]])
    assert ar.path_score(blk, emit, [0], 2) == ar.path_score(blk, emit, [1], 2) == -3.0
    frames, best, _ = ar.viterbi(blk, emit, 2, 1)
    assert frames == [0] and best == -3.0       # at (1,1): blank predecessor (0,1) ties the label predecessor (1,0) and wins
    # the label predecessor strictly greater, by the smallest step these sums can show: it is taken
    emit2 = emit.copy()
    emit2[1, 0] = -1.0 + 2.0 ** -51
    assert ar.viterbi(blk, emit2, 2, 1)[0] == [1]


def test_edge_cases_of_the_restatement():
    rng = np.random.default_rng(7)
    blk, emit = _random_lattice(rng, 6, 3, "real")
    frames, best, M = ar.viterbi(blk, emit, 1, 3)           # one frame: every label on frame 0
    assert frames == [0, 0, 0] and best == emit[0, :3].sum() + blk[0, 3] and ar.margin(frames, best, M) == np.inf
    frames, best, M = ar.viterbi(blk, emit, 6, 0)           # no label: the all-blank path
    assert frames == [] and abs(best - blk[:, 0].sum()) < 1e-12 and M.shape == (6, 0)
    A, C, bias = rng.normal(size=(6, 7)), rng.normal(size=(4, 7)), rng.normal(size=7)
    labels = [3, 1, 6]
    b1, e1 = ar.lattice(A[:, None, :] + C[None, :, :] + bias, labels, 2)
    b2, e2 = ar.lattice_sep(A, C, bias, labels, 2, chunk=4)
    assert np.abs(b1 - b2).max() < 1e-12 and np.abs(e1 - e2).max() < 1e-12


def test_new_symbols_are_declared_exported_and_bound():
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc import build
    build.build()
    header = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    declared = set(re.findall(r"\b(rnnt_hip_\w+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/rnnt_hip.h"
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.SYMBOLS"
    assert _lib.lib().rnnt_hip_version() == _lib.ABI_VERSION == 4
    for word in ("max(", "blank predecessor", "frames[b][u]", "-inf", "u_lens[b] = 0", "T = 1"):
        assert word in header, f"the header comment does not state {word!r}"


def test_align_arguments_are_validated_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    assert L.rnnt_hip_joint_align_workspace_bytes(0, 1, 1, 1) == 0
    nws = L.rnnt_hip_joint_align_workspace_bytes(2, 10, 3, 5)
    assert nws >= 2 * 10 * 3 * 8 + 2 * 3 * 4                   # blk + emit (fp32) and one 32-frame word per label row
    one = 8                                                   # any non-null address: validation never dereferences it
    rc = L.rnnt_hip_joint_align(None, 5, 50, None, 5, 15, None, None, None, None, 2, 10, 3, 5, 0, None, None, None, 0, None)
    assert rc == -1 and b"null" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_align(one, 5, 50, one, 5, 15, one, one, one, one, 1, 4, 513, 5, 0, one, one, one, 1 << 30, None)
    assert rc == -1 and b"512" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_align(one, 5, 50, one, 5, 15, one, one, one, one, 2, 10, 3, 5, 5, one, one, one, 1 << 30, None)
    assert rc == -1 and b"blank" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_joint_align(one, 5, 50, one, 5, 15, one, one, one, one, 2, 10, 3, 5, 0, one, one, one, nws - 1, None)
    assert rc == -1 and b"workspace too small" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_align_from_logits_ex(None, 0, None, None, None, 1, 1, 600, 3, 0, None, None, None, 0, None)
    assert rc == -1 and b"512" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_align_from_logits_ex(None, 0, one, one, one, 2, 10, 3, 5, 0, one, one, one, 1 << 30, None)
    assert rc == -1 and b"null logits" in L.rnnt_hip_last_error()
    rc = L.rnnt_hip_align_from_logits_ex(one, 7, one, one, one, 2, 10, 3, 5, 0, one, one, one, 1 << 30, None)
    assert rc == -1 and b"dtype" in L.rnnt_hip_last_error()


def test_python_surface_exists_and_fails_loudly_on_cpu():
    from rnntransducer_amd import RNNTransducer, ops
    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.loss import rnnt_align
    from rnntransducer_amd.networks import JointNet
    assert callable(JointNet.align) and callable(RNNTransducer.align) and callable(ops.joint_align) and callable(ops.align_from_logits)
    B, T, U, V = 2, 5, 2, 6
    i32 = dict(dtype=torch.int32)
    targets, t_lens, u_lens = torch.ones(B, U, **i32), torch.tensor([5, 4], **i32), torch.tensor([2, 1], **i32)
    with pytest.raises(RnntHipError):
        rnnt_align(torch.zeros(B, T, U + 1, V), targets, t_lens, u_lens, 0)
    with pytest.raises(RnntHipError):
        ops.joint_align(torch.zeros(T, B, V), torch.zeros(U + 1, B, V), torch.zeros(V), targets, t_lens, u_lens, 0)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    m = RNNTransducer(dict(embedding_size=V, hidden_size=8, output_size=8, num_layers=1),
                      dict(input_size=4, hidden_size=8, output_size=8, num_layers=1), dict(num_classes=V), args)
    texts = torch.zeros(B, U + 1, dtype=torch.long)
    batch = (torch.zeros(B, T, 4), [5, 4], t_lens, texts, [3, 2], targets, u_lens)
    with pytest.raises(RuntimeError, match="eval"):             # training mode is refused, as recognize_greedy refuses it
        m.jointnet.align(batch[0], t_lens, texts, targets, u_lens, 0)
    m.eval()
    with pytest.raises(RnntHipError):
        m.jointnet.align(batch[0], t_lens, texts, targets, u_lens, 0)
    with pytest.raises(RnntHipError):
        m.align(batch)
    res = ops.Alignment(torch.tensor([[3, 4], [2, -1]], **i32), torch.zeros(B, dtype=torch.float64), u_lens)
    assert res.token_frames(0) == [3, 4] and res.token_frames(1) == [2]
