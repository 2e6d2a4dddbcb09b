"""CPU side of the search kernels' shape-edge tests: every case of tests/search_shape_cases.py finds its seed in range(20) with a
decision margin >= 1e-4 and the properties the GPU tests (tests/test_gpu_search_shapes.py) rely on, and every float64 reference
finishes in a few seconds.  The host-side LDS limit of the batched prediction-net step is checked here too, through the C ABI."""
import ctypes as C
import time

import pytest
import torch

from tests import search_shape_cases as sc

REF_SECONDS = 5.0   # per restated search


def test_step_cases_cover_the_edges():
    hps = {Hp for Hp, L, cell in sc.STEP_CASES if L == 1 and cell == "lstm"}
    assert hps >= {4, 8, 60, 252, 256, 260, 508, 516, 1024, 1028}
    for Hp in (60, 260):
        assert {cell for h, L, cell in sc.STEP_CASES if h == Hp} == set(sc.CELLS)
        assert {L for h, L, cell in sc.STEP_CASES if h == Hp} >= {1, 3, 8}
    assert (1024, 8, "gru") in sc.STEP_CASES and sc.step_lds_bytes(8, 1024) == 102400 > 64 * 1024
    L, Hp = sc.STEP_LDS_FITS[:2]
    assert sc.step_lds_bytes(L, Hp) <= sc.DEC_MAX_LDS < sc.step_lds_bytes(L, Hp + 4) and sc.STEP_LDS_OVER[1] == Hp + 4


@pytest.mark.parametrize("case", [(4, 1, "lstm"), (260, 8, "lstm"), (260, 1, "gru"), (60, 1, "rnn_relu")], ids=str)
def test_step_reference_steps_as_a_two_step_sequence(case):
    """The reference's two successive steps are torch's own two-step sequence; tokens hold 0 and the embedding's last row."""
    Hp, L, cell = case
    emb, rnn, tokens, (h_in, c_in), want = sc.step_case(Hp, L, cell)
    assert tokens.tolist()[:2] == [0, sc.STEP_V - 1] and len(set(tokens.tolist())) == sc.STEP_B
    x = emb.double()[tokens][:, None]
    with torch.no_grad():
        _, s = rnn.double()(torch.cat((x, x), dim=1), None)
    h2 = s[0] if cell == "lstm" else s
    torch.testing.assert_close(want[1][0], h2, rtol=0, atol=1e-12)
    assert want[0][0].shape == (L, sc.STEP_B, Hp) and (want[0][1] is None) == (cell != "lstm")
    assert float((want[2][0] - want[0][0]).abs().max()) > 1e-3   # the carried state enters the step


def test_step_over_the_lds_limit_is_refused_on_the_host():
    """8 layers at Hp = 1640 need 164000 B of LDS: RNNT_ERR_INVALID with the "> 160 KiB" message before anything is launched
    (placeholder pointers: nothing is dereferenced)."""
    from rnntransducer_amd import _lib
    lib = _lib.lib()
    keep = C.create_string_buffer(64)
    p = C.addressof(keep)
    L, Hp, cell, B = sc.STEP_LDS_OVER
    assert sc.step_lds_bytes(L, Hp) == 164000
    d = _lib.PrednetStepDesc()
    d.B, d.Hp, d.L, d.cell = B, Hp, L, sc.CELLS[cell]
    d.tokens = d.emb = d.h_out = d.c_out = p
    for l in range(L):
        d.w_ih[l] = d.w_hh[l] = d.b_ih[l] = d.b_hh[l] = p
    assert lib.rnnt_hip_prednet_step(C.byref(d), None) == -1   # RNNT_ERR_INVALID
    msg = lib.rnnt_hip_last_error().decode()
    assert "164000 B of LDS" in msg and "> 160 KiB" in msg, msg
    with pytest.raises(ValueError, match="160 KiB"):
        _lib.check(-1, "rnnt_hip_prednet_step")


@pytest.mark.parametrize("name", list(sc.GREEDY_CASES))
def test_greedy_case_has_a_seed(name):
    case = sc.greedy_case(name)
    assert case is not None, "no seed in range(20) qualifies"
    seed, net, enc, lens, ref, secs = case
    Hp, O, Oe, V, L, cell, blank, T, _ = sc.GREEDY_CASES[name]
    assert T <= 12 and Oe % 4 == 0 and enc.shape == (T, sc.GREEDY_B, Oe)
    assert ref.margin >= sc.MARGIN and secs < REF_SECONDS
    assert all(2 * len(ref.tokens[b]) >= n for b, n in enumerate(lens))
    assert all(blank not in t for t in ref.tokens)
    if V > sc.THREADS:
        assert any(k >= sc.THREADS for t in ref.tokens for k in t)


def test_greedy_cases_hold_what_the_issue_names():
    shapes = {c[:7] for c in sc.GREEDY_CASES.values()}
    assert shapes == {(4, 4, 4, 2, 1, "lstm", 0), (260, 12, 20, 65, 1, "gru", 64), (516, 260, 8, 72, 2, "lstm", 0),
                      (1028, 36, 12, 1030, 1, "rnn_relu", 1029), (1024, 320, 320, 72, 8, "lstm", 0), (60, 8, 8, 7, 8, "gru", 3)}
    assert any(c[8] is not None and 0 in c[8] and 1 in c[8] for c in sc.GREEDY_CASES.values())
    assert sc.greedy_lds_bytes(8, 1024, 320, 72) > 64 * 1024


@pytest.mark.parametrize("name", list(sc.TIE_CASES))
def test_tie_case_has_a_seed(name):
    t0 = time.perf_counter()
    case = sc.tie_case(name)
    assert case is not None and time.perf_counter() - t0 < REF_SECONDS
    seed, net, A, want, margin, wins = case
    group, blank = sc.TIE_CASES[name]
    lo = group[0]
    assert margin >= sc.MARGIN and wins >= sc.TIE_B * len(sc.TIE_FRAMES)
    w = net.fc.weight
    assert all(torch.equal(w[v], w[lo]) and torch.equal(A[:, :, v], A[:, :, lo]) for v in group[1:])
    for toks, frames in want:
        assert not set(toks) & set(group[1:])                      # torch.argmax: the lowest index among equal maxima
        on_lifted = [k for k, t in zip(toks, frames) if t in sc.TIE_FRAMES]
        if blank == lo:
            assert on_lifted == []                                  # the blank wins the tie: nothing on that frame
        else:
            assert on_lifted and set(on_lifted) == {lo}


def test_tie_groups_span_lanes_waves_and_passes():
    diffs = {name: {b - a for a in g for b in g if b > a} for name, (g, _) in sc.TIE_CASES.items()}
    assert diffs["neighbouring_lanes"] == {1} and diffs["two_waves"] == {64} and diffs["two_passes_of_a_thread"] == {1024}
    assert diffs["three_way"] >= {1, 64, 1024}
    assert sc.TIE_CASES["blank_lowest"][1] == min(sc.TIE_CASES["blank_lowest"][0])
    assert sc.TIE_CASES["blank_highest"][1] == max(sc.TIE_CASES["blank_highest"][0])


@pytest.mark.parametrize("name", list(sc.BEAM_CASES))
def test_beam_case_has_a_seed(name):
    case = sc.beam_case(name)
    assert case is not None, "no seed in range(20) qualifies"
    seed, net, enc, want, margin, pops, secs = case
    lens = sc.BEAM_CASES[name][6]
    assert margin >= sc.MARGIN and pops > 2 * sum(lens) and secs < REF_SECONDS
    assert any(k >= sc.THREADS for nb in want for y, _ in nb for k in y)
    assert any(0 < k < sc.THREADS for nb in want for y, _ in nb for k in y)   # and one from the first pass
    caps = sc.beam_caps(sc.BEAM_CASES[name][2])
    assert caps["max_candidates"] >= 4 * sc.BEAM_CASES[name][2]


@pytest.mark.parametrize("name", list(sc.BEAM_CASES))
def test_beam_stream_case_keeps_the_margin_and_ends_at_the_offline_result(name):
    sc.beam_case(name)   # (the seed search is not what is timed)
    t0 = time.perf_counter()
    after, margin = sc.beam_stream_case(name)
    assert time.perf_counter() - t0 < 2 * REF_SECONDS   # two streams
    assert margin >= sc.MARGIN
    lens = sc.BEAM_CASES[name][6]
    sched = sc.stream_schedule(lens)
    assert [sum(ns[b] for _, ns in sched) for b in range(len(lens))] == lens and {Tc for Tc, _ in sched} == {1, 2}
    assert after[-1] == [[(list(y), s) for y, s in nb] for nb in sc.beam_case(name)[3]]


def test_fused_case_has_a_seed():
    case = sc.fused_case()
    assert case is not None
    seed, net, enc, fusion, want, margin, pops, secs = case
    lens = sc.BEAM_CASES[sc.FUSED_CASE][6]
    assert margin >= sc.MARGIN and pops > 2 * sum(lens) and secs < REF_SECONDS
    assert any(k >= sc.THREADS for nb in want for y, _, _ in nb for k in y)
    assert any(abs(f - a) > 1e-3 for nb in want for _, a, f in nb)   # the bigram moves the scores
