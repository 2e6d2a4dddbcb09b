"""GPU tests of the CTC forced alignment (rnnt_hip_ctc_align, ops.ctc_align) against the float64 restatement in
tests/ctc_align_restatement.py, by the rules of tests/test_gpu_align.py.

Per utterance, TOL = NLL_RTOL * |best float64 score| with that file's NLL_RTOL = 1e-5 (the same fp32 per-frame terms are compared
with a float64 log-softmax):
  * the returned path is valid: collapsing `path` gives the labels, `first` / `last` agree with `path`, first[u] <= last[u] <
    first[u+1] inside [0, t_lens[b]), -1 past u_lens[b] and past t_lens[b];
  * the returned score equals the float64 score of THAT path within TOL;
  * that float64 score is at least the restatement's best minus TOL;
  * where the float64 margin exceeds 2 TOL, first, last and path equal the restatement's exactly (tests/test_ctc_align_oracle.py
    asserts, without a GPU, that at most one utterance in ten of every set lies below);
  * token_logp equals the ascending float64 sum of the device's own fp32 lp (the emission rows the call leaves at the start of
    its workspace) over the returned span within T * 2^-52 relative;
  * score <= -nll of rnnt_hip_ctc_loss_fwd within TOL, with equality on a single-path row.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


class Got:
    def __init__(self, res, em, nll):
        self.first, self.last, self.path = (x.cpu().numpy() for x in (res.first, res.last, res.path))
        self.score, self.token_logp = res.score.cpu().numpy(), res.token_logp.cpu().numpy()
        self.em, self.nll = em, nll


def run(case, rows=None, time_major=False, pad=0, with_nll=True):
    """ops.ctc_align with every output on the rows `rows` of the case (all by default); time_major: a (T,B,V) buffer whose rows are
    `pad` floats longer than V (z_st > V is reached through the C entry)."""
    from rnntransducer_amd import _lib, ops
    from rnntransducer_amd.ops import _addr, _stream, check
    sl = slice(None) if rows is None else rows
    z, y = case.logits[sl], case.labels[sl]
    tl, ul = _dev(np.array(case.t_lens)[sl], torch.int32), _dev(np.array(case.u_lens)[sl], torch.int32)
    B, T, V = z.shape
    U = y.shape[1]
    ws = torch.empty(ops.ctc_align_workspace_bytes(B, T, U, V), device="cuda", dtype=torch.uint8)
    yd = _dev(y)
    if not time_major:
        zd = _dev(z)
        res = ops.ctc_align(zd, yd, tl, ul, case.blank, return_path=True, return_token_logp=True, workspace=ws)
    else:
        buf = torch.full((T, B, V + pad), 1e30, device="cuda")   # the padding would wreck any row that read it
        buf[:, :, :V] = _dev(z).transpose(0, 1)
        first, last = (torch.empty(B, U, device="cuda", dtype=torch.int32) for _ in range(2))
        path = torch.empty(B, T, device="cuda", dtype=torch.int32)
        tlp, score = torch.empty(B, U, device="cuda", dtype=torch.float64), torch.empty(B, device="cuda", dtype=torch.float64)
        check(_lib.lib().rnnt_hip_ctc_align(_addr(buf), V + pad, B * (V + pad), _addr(yd) if U else None, _addr(tl), _addr(ul), B, T, U,
                                            V, case.blank, _addr(first) if U else None, _addr(last) if U else None, _addr(path),
                                            _addr(tlp) if U else None, _addr(score), _addr(ws), ws.numel(), _stream()), "ctc_align")
        res = ops.CtcAlignment(first, last, score, path, tlp)
        zd = _dev(z)
    torch.cuda.synchronize()
    em = ws[:4 * B * (U + 1) * T].view(torch.float32).view(B, U + 1, T).cpu().numpy()
    nll = None
    if with_nll:
        nll = ops.CtcLossFn.apply(zd, yd, tl, ul, case.blank, False, "none").cpu().numpy().astype(np.float64)
    return Got(res, em, nll)


def check_case(case, got, rows=None, score_abs=None):
    """The rules above on every row; -> the number of rows below the margin.  score_abs: an absolute tolerance that replaces TOL
    in the score rules (the known-answer set, whose scores are too close to 0 for any relative one)."""
    rows = list(range(case.B)) if rows is None else rows
    low = 0
    for i, b in enumerate(rows):
        tag = f"{case.name}[{b}]"
        Tb, Ub = case.t_lens[b], case.u_lens[b]
        lp, y = case.row(b)
        best, margin, tol = case.oracle()[b]
        stol = tol if score_abs is None else score_abs
        first, last, path = got.first[i], got.last[i], got.path[i]
        print(f"{tag}: Tb {Tb} Ub {Ub} score {got.score[i]!r} best {best.score!r} margin {margin:.3e} tol {tol:.3e}")
        assert (first[Ub:] == -1).all() and (last[Ub:] == -1).all() and (got.token_logp[i, Ub:] == 0).all(), tag
        assert (path[Tb:] == -1).all(), tag
        if not best.ok:
            assert got.score[i] == -np.inf and (first == -1).all() and (last == -1).all() and (path == -1).all(), tag
            assert (got.token_logp[i] == 0).all(), tag
            if got.nll is not None:
                assert got.nll[i] == np.inf, tag
            continue
        # validity
        f, l = [int(x) for x in first[:Ub]], [int(x) for x in last[:Ub]]
        assert all(0 <= a <= z < Tb for a, z in zip(f, l)) and all(l[u] < f[u + 1] for u in range(Ub - 1)), f"{tag}: spans {f} {l}"
        want_path = np.full(Tb, case.blank, dtype=np.int64)
        for u in range(Ub):
            want_path[f[u]:l[u] + 1] = y[u]
            if u and y[u] == y[u - 1]:
                assert f[u] > l[u - 1] + 1, f"{tag}: equal labels {u - 1}, {u} without a blank between"
        assert (path[:Tb] == want_path).all(), f"{tag}: path disagrees with first / last"
        collapsed = [int(v) for t, v in enumerate(path[:Tb]) if v != case.blank and (t == 0 or path[t - 1] != v)]
        assert collapsed == y, f"{tag}: the path collapses to {collapsed}, labels {y}"
        # score of that path, optimality, exact path above the margin
        mine = float(sum(lp[t, path[t]] for t in range(Tb)))
        assert abs(got.score[i] - mine) <= stol, f"{tag}: score {got.score[i]} vs the path's float64 score {mine}"
        assert mine >= best.score - tol, f"{tag}: path score {mine} below the best {best.score}"
        if margin > 2 * tol:
            assert f == list(best.first) and l == list(best.last), f"{tag}: spans differ from the oracle's"
            assert (path[:Tb] == best.tokens(y, case.blank)).all(), tag
        else:
            low += 1
        # token_logp: the ascending fp64 sum of the device's own fp32 terms
        for u in range(Ub):
            acc = 0.0
            for t in range(f[u], l[u] + 1):
                acc += float(got.em[i, u + 1, t])
            assert abs(got.token_logp[i, u] - acc) <= Tb * 2.0 ** -52 * abs(acc), f"{tag}: token_logp[{u}]"
        if got.nll is not None:
            assert got.score[i] <= -got.nll[i] + stol, f"{tag}: score {got.score[i]} above -nll {-got.nll[i]}"
            if margin == np.inf:   # a single path
                assert abs(got.score[i] + got.nll[i]) <= stol, f"{tag}: single path, score {got.score[i]} vs -nll {-got.nll[i]}"
    return low


@pytest.mark.parametrize("case", cr.margin_cases(), ids=lambda c: c.name)
def test_against_the_restatement(case):
    low = check_case(case, run(case))
    assert low * 10 <= case.B


def test_single_path_no_path_and_empty_rows():
    case = cr.edge_case()
    got = run(case)
    check_case(case, got)
    ok = [best.ok for best, _, _ in case.oracle()]
    assert ok == [True, False, True, False, False, True]
    assert np.isfinite(got.score[[0, 2, 5]]).all()
    # every row is untouched by the rows without a path: the good rows alone give the same bits
    alone = run(case, rows=[0, 2, 5])
    for name in ("first", "last", "path", "score", "token_logp"):
        assert np.array_equal(getattr(alone, name), getattr(got, name)[[0, 2, 5]]), name


def test_known_answer_spans():
    """Label u leads by 20 on the frames of its span and the blank leads by 20 everywhere else, so the spans are exactly those.
    Every frame's lp is about -2e-9 and the score about -1e-7: below what fp32 terms of magnitude 20 resolve (z - lse is 0 exactly),
    so the score rules take an absolute tolerance here, one fp32 ulp of 20 per frame; every other rule is as everywhere."""
    case = cr.known_answer_case()
    got = run(case)
    assert check_case(case, got, score_abs=case.T * 20 * 2.0 ** -23) == 0
    want = [[(0, 0), (1, 3), (9, 9)], [(2, 5), (7, 7)], [], [(39, 39)], [(0, 39)]]
    for b, row in enumerate(want):
        assert [(int(f), int(l)) for f, l in zip(got.first[b, :len(row)], got.last[b, :len(row)])] == row
    assert (got.path[2] == case.blank).all() and np.isfinite(got.score[2])   # no labels: the all-blank path


def test_tie_rule_on_constant_logits():
    """Every path scores the same: the labels sit on the earliest frames they can (tests/test_ctc_align_oracle.py derives it)."""
    z = np.zeros((3, 6, 4), np.float32)
    labels = np.array([[1, 2, 3], [1, 1, 2], [2, 2, 2]], np.int32)
    case = cr.Case("ties", z, labels, [6, 4, 5], [3, 2, 3], 0)
    got = run(case)
    assert got.first[0].tolist() == [0, 1, 2] and got.last[0].tolist() == [0, 1, 2] and got.path[0].tolist() == [1, 2, 3, 0, 0, 0]
    assert got.first[1].tolist() == [0, 2, -1] and got.path[1].tolist() == [1, 0, 1, 0, -1, -1]
    assert got.first[2].tolist() == [0, 2, 4] and got.path[2].tolist() == [2, 0, 2, 0, 2, -1]   # the label state ends the path
    for b in range(3):
        best = cr.viterbi(*case.row(b), 0)
        assert got.first[b, :case.u_lens[b]].tolist() == list(best.first) and got.last[b, :case.u_lens[b]].tolist() == list(best.last)


def test_time_major_with_padded_rows():
    case = cr.margin_cases()[4]
    a, b = run(case, with_nll=False), run(case, time_major=True, pad=5, with_nll=False)
    for name in ("first", "last", "path", "score", "token_logp"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    check_case(case, b)


@pytest.mark.parametrize("idx", [3, 8, 11])
def test_row_alone_and_two_calls_bit_for_bit(idx):
    case = cr.margin_cases()[idx]
    full, again = run(case, with_nll=False), run(case, with_nll=False)
    for name in ("first", "last", "path", "score", "token_logp"):
        assert np.array_equal(getattr(full, name), getattr(again, name)), name
    for b in range(case.B):
        alone = run(case, rows=[b], with_nll=False)
        for name in ("first", "last", "path", "score", "token_logp"):
            assert np.array_equal(getattr(alone, name)[0], getattr(full, name)[b]), (name, b)


def test_optional_outputs_and_no_labels():
    from rnntransducer_amd import ops
    case = cr.margin_cases()[0]   # U = 0
    res = ops.ctc_align(_dev(case.logits), _dev(case.labels), _dev(np.array(case.t_lens), torch.int32),
                        _dev(np.array(case.u_lens), torch.int32), case.blank)
    assert res.path is None and res.token_logp is None and res.first.shape == (case.B, 0) and torch.isfinite(res.score).all()
    case = cr.margin_cases()[5]
    full = run(case, with_nll=False)
    res = ops.ctc_align(_dev(case.logits), _dev(case.labels), _dev(np.array(case.t_lens), torch.int32),
                        _dev(np.array(case.u_lens), torch.int32), case.blank)
    assert res.path is None and res.token_logp is None
    assert np.array_equal(res.first.cpu().numpy(), full.first) and np.array_equal(res.score.cpu().numpy(), full.score)
