"""CPU checks of the internal-LM subtraction's float64 restatement (tests/ilm_restatement.py) and of the seeded cases the GPU
tests use (tests/ilm_cases.py): no GPU, no library call."""
import math

import pytest

from tests import beam_sync_cases as K
from tests import ilm_cases as IK
from tests import ilm_restatement as IR


@pytest.mark.parametrize("c", K.SHAPE_CASES, ids=K.case_id)
def test_weight_zero_is_the_plain_restatement(c):
    """mu = 0: the same hypotheses, scores, frames and margins as beam_sync_restatement.search_one, on every shape case."""
    T, V, Hp, L, cell, W, S, O, min_logp, _ = c
    _, ora, _, _, x, want = K.shape_case(c)
    got = IR.search(ora, x, [T], 0, W, S, min_logp, None, 0.0)[0]
    assert got.hyps == want.hyps
    assert (got.boundary_margin, got.order_margin, got.merges) == (want.boundary_margin, want.order_margin, want.merges)


def test_weight_zero_with_fusion_is_the_fused_restatement():
    from tests import beam_sync_restatement as R
    T, V, W, S = (K.FUSION[k] for k in ("T", "V", "W", "S"))
    _, ora, _, _, x, fusion, want = K.fusion_case("bigram")
    got = IR.search(ora, x, [T], 0, W, S, fusion=fusion, mu=0.0)[0]
    assert got.hyps == want.hyps == R.search(ora, x, [T], 0, W, S, fusion=fusion)[0].hyps
    assert (got.boundary_margin, got.order_margin) == (want.boundary_margin, want.order_margin)


@pytest.mark.parametrize("T,S", K.EXHAUSTIVE)
def test_exhaustive_fused_minus_score_is_the_teacher_forced_ilm(T, S):
    """Every sequence is in the beam: score is the brute-force path sum as without the term, and fused - score is
    -mu * ilm_score(y) from an independent teacher-forced loop, to 1e-12."""
    _, net64, mass, res = IK.exhaustive_case(T, S)
    assert {tuple(y) for y, *_ in res.hyps} == set(mass) and len(res.hyps) == len(mass)
    for y, score, fused, _ in res.hyps:
        assert abs(score - mass[tuple(y)]) <= 1e-12
        assert abs((fused - score) + IK.MU * IR.ilm_score_fp64(net64, y, 0)) <= 1e-12
    assert any(fused - score > 0.1 for _, score, fused, _ in res.hyps)   # the term is a bonus, and not a small one


def test_ilm_of_one_token_vocabulary_is_zero():
    T, V, Hp, L, cell, W, S = IK.V2
    ora, _, _ = K.model(V, Hp, L, cell, 8, 2, scale=1.0)
    x = K.audio(T, 2)
    on = IR.search(ora, x, [T], 0, W, S, mu=IK.MU)[0]
    off = IR.search(ora, x, [T], 0, W, S, mu=0.0)[0]
    assert [(y, s, f) for y, s, _, f in on.hyps] == off.hyps and all(fs == s for _, s, fs, _ in on.hyps)


@pytest.mark.parametrize("c", IK.SHAPE_CASES, ids=K.case_id)
def test_every_shape_case_finds_its_seed(c):
    case = IK.shape_case(c)
    assert case is not None, "no seed in range(20) keeps a boundary margin >= 1e-4: change the case's scale or mu"
    res = case[-1]
    print(K.case_id(c), "seed", case[0], "boundary margin %.3g" % res.boundary_margin, "merges", res.merges)
    assert res.boundary_margin >= IK.MARGIN and all(math.isfinite(e[1]) and math.isfinite(e[2]) for e in res.hyps)
    assert any(e[2] != e[1] for e in res.hyps)


@pytest.mark.parametrize("c", K.BLANKS, ids=["first", "middle", "last"])
def test_every_blank_case_finds_its_seed(c):
    case = IK.blank_case(*c)
    assert case is not None and case[-1].boundary_margin >= IK.MARGIN


def test_the_other_cases_find_their_seeds():
    for case in (IK.no_fusion_case(), IK.ngram_case()):
        assert case is not None and case[-1].boundary_margin >= IK.MARGIN
    case = IK.ragged_case()
    assert case is not None and min(r.boundary_margin for r in case[-1]) >= IK.MARGIN
    assert case[-1][1].hyps == [([0], 0.0, float(case[-2].final[0]), [-1])]   # no frames: [[blank]], score 0, final[0]


def test_the_stream_case_finds_its_seed():
    case = IK.stream_case()
    assert case is not None, "no seed keeps the margin with a keep set that fits max_nodes and a tree that does not"
    res = case[-1]
    print("stream case: seed", case[0], "margin %.3g" % res.boundary_margin, "keep max", max(res.keep), "tree", res.tree[-1])


def test_subtraction_changes_the_search():
    """The term steers: on the first shape the n-best with mu differs from the n-best without it."""
    T, V, Hp, L, cell, W, S, O, min_logp, _ = IK.NO_FUSION
    _, ora, _, _, x, res = IK.no_fusion_case()
    plain = IR.search(ora, x, [T], 0, W, S, min_logp, None, 0.0)[0]
    assert [e[0] for e in res.hyps] != [e[0] for e in plain.hyps]
