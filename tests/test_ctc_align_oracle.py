"""CPU checks of the float64 restatement of the CTC forced alignment (tests/ctc_align_restatement.py) and of the inputs the GPU
tests use: the restatement against brute force on every tiny lattice, against torch's float64 CTC likelihood, the tie rule's known
answers, and the cap on low-margin utterances of the GPU file's seeded sets (a property of the float64 side alone)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_restatement as cr  # noqa: E402


def _tiny_lattices(V=3):
    for blank in (0, V - 1):
        vals = [v for v in range(V) if v != blank]
        for T in range(1, 6):
            for U in range(0, 3):
                for labels in itertools.product(vals, repeat=U):
                    yield T, list(labels), blank


def test_restatement_against_brute_force():
    rng = np.random.default_rng(0)
    n = 0
    for T, labels, blank in _tiny_lattices():
        lp = cr.log_softmax64(rng.normal(size=(T, 3)))
        best, all_paths = cr.viterbi(lp, labels, blank), cr.brute_force(lp, labels, blank)
        if not all_paths:
            assert not best.ok and best.score == -np.inf and T < len(labels) + cr.repeats(labels)
            assert (best.first == -1).all() and (best.last == -1).all() and (best.token_logp == 0).all()
            continue
        assert best.ok and T >= len(labels) + cr.repeats(labels)
        score, _, seq = all_paths[0]
        assert best.score == pytest.approx(score, abs=1e-12)
        m = cr.margin(lp, labels, blank, best)
        if len(all_paths) == 1:
            assert m == np.inf
        else:
            assert m == pytest.approx(score - all_paths[1][0], abs=1e-12)
        assert list(best.states) == list(seq)   # (random reals: no ties)
        first, last = cr.spans(seq, len(labels))
        assert list(best.first) == list(first) and list(best.last) == list(last)
        assert all(f <= l for f, l in zip(first, last)) and all(last[u] < first[u + 1] for u in range(len(labels) - 1))
        for u, y in enumerate(labels):
            assert best.token_logp[u] == pytest.approx(lp[first[u]:last[u] + 1, y].sum(), abs=1e-12)
        n += 1
    assert n >= 50


def test_tie_rule_against_brute_force_on_integer_terms():
    """Small integer terms make equal scores exact: the restatement's path is the first of the best in the tie rule's order."""
    rng = np.random.default_rng(1)
    ties = 0
    for T, labels, blank in _tiny_lattices():
        for _ in range(3):
            lp = -rng.integers(0, 2, size=(T, 3)).astype(np.float64)
            best, all_paths = cr.viterbi(lp, labels, blank), cr.brute_force(lp, labels, blank)
            if not all_paths:
                assert not best.ok
                continue
            assert best.score == all_paths[0][0] and list(best.states) == list(all_paths[0][2])
            ties += len(all_paths) > 1 and all_paths[1][0] == all_paths[0][0]
    assert ties >= 50


def test_tie_rule_known_answers():
    """Constant terms: every path scores the same.  Walking back from the trailing blank the path stays wherever the state was
    reachable a frame earlier, so every label sits on the earliest frame it can: one frame each from frame 0, a free frame between
    equal neighbours, blanks after."""
    lp = np.full((6, 4), -1.0)
    p = cr.viterbi(lp, [1, 2, 3], 0)
    assert list(p.first) == [0, 1, 2] and list(p.last) == [0, 1, 2] and list(p.states) == [1, 3, 5, 6, 6, 6] and p.score == -6.0
    p = cr.viterbi(lp[:3], [1, 2, 3], 0)      # T = U: the last label state ends the path
    assert list(p.first) == [0, 1, 2] and list(p.states) == [1, 3, 5]
    p = cr.viterbi(lp[:4], [1, 1], 0)         # aa: a, blank, a, blank
    assert list(p.states) == [1, 2, 3, 4] and list(p.first) == [0, 2] and list(p.last) == [0, 2]
    p = cr.viterbi(lp[:3], [1, 1], 0)         # aa in three frames: the single path a, blank, a
    assert list(p.states) == [1, 2, 3] and cr.margin(lp[:3], [1, 1], 0, p) == np.inf
    assert not cr.viterbi(lp[:2], [1, 1], 0).ok and not cr.viterbi(lp[:0], [], 0).ok
    p = cr.viterbi(lp, [], 0)                 # no labels: the all-blank path
    assert p.ok and list(p.states) == [0] * 6 and p.score == -6.0
    assert list(p.tokens([], 0)) == [0] * 6
    # the end rule: S-2 only when strictly greater
    lp2 = np.zeros((2, 2))
    assert list(cr.viterbi(lp2, [1], 0).states) == [1, 2]
    lp2[1, 0] = -1.0
    assert list(cr.viterbi(lp2, [1], 0).states) == [1, 1]


def test_score_against_the_float64_ctc_likelihood():
    rng = np.random.default_rng(2)
    for T, labels, blank in _tiny_lattices():
        if not labels:
            continue
        z = rng.normal(size=(T, 3))
        lp = cr.log_softmax64(z)
        nll = torch.nn.functional.ctc_loss(torch.from_numpy(lp).unsqueeze(1), torch.tensor([labels]), torch.tensor([T]),
                                           torch.tensor([len(labels)]), blank=blank, reduction="none", zero_infinity=False).item()
        best = cr.viterbi(lp, labels, blank)
        if not best.ok:
            assert nll == np.inf
            continue
        assert best.score <= -nll + 1e-12
        if T == len(labels) + cr.repeats(labels):   # a single path: the sum over all paths is that path
            assert best.score == pytest.approx(-nll, abs=1e-12) and cr.margin(lp, labels, blank, best) == np.inf


def _cap(case):
    low = sum(1 for best, m, tol in case.oracle() if best.ok and m < 2 * tol)
    return low, case.B


@pytest.mark.parametrize("case", cr.margin_cases(), ids=lambda c: c.name)
def test_cap_on_low_margin_utterances_of_the_gpu_sets(case):
    """At most one utterance in ten of every seeded set of tests/test_gpu_ctc_align.py lies below 2 TOL; and every row of these sets
    has a path, so the margin rule covers them."""
    low, n = _cap(case)
    assert all(best.ok for best, _, _ in case.oracle())
    assert low * 10 <= n, f"{case.name}: {low} of {n} utterances below the margin"


def test_edge_and_known_answer_sets():
    c = cr.edge_case()
    o = c.oracle()
    assert [best.ok for best, _, _ in o] == [True, False, True, False, False, True]
    assert o[0][1] == np.inf and o[2][1] == np.inf          # single paths
    assert o[5][1] >= 2 * o[5][2]
    assert cr.repeats(list(c.labels[0, :6])) >= 1
    k = cr.known_answer_case()
    want = [[(0, 0), (1, 3), (9, 9)], [(2, 5), (7, 7)], [], [(39, 39)], [(0, 39)]]
    for (best, m, tol), row in zip(k.oracle(), want):
        assert best.ok and m > 2 * tol
        assert [(int(f), int(l)) for f, l in zip(best.first, best.last)] == row
