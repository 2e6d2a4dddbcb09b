"""CPU side of the end-to-end MWER cases (tests/mwer_cases.py): at the chosen seeds the float64 restatement of the search on the
oracle networks keeps its decision margin and gives a problem in which the risk does something.  tests/test_gpu_mwer_model.py
asserts the same non-vacuity on what the device produced."""
import pytest

from tests import mwer_cases as M


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_case_seed_gives_a_margin_and_a_non_trivial_risk(name):
    c = M.cpu_case(name)
    assert c["margin"] >= M.MARGIN, c["margin"]
    assert all(1 <= len(h) <= M.N for h in c["hyps"])
    assert all(len(set(map(tuple, h))) == len(h) for h in c["hyps"])          # the search merges equal sequences
    assert M.non_vacuous(c["W"], c["weights"]), (c["W"], c["weights"])
    assert max(len(y) for h in c["hyps"] for y in h) <= 511
