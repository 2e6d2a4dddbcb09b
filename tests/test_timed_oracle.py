"""Recognition with token timestamps and confidences, CPU side: the restatements of tests/timed_restatement.py pinned to the
REFERENCE's fixtures (tests/golden/d*_greedy.npz, b*_beams.npz, s*_beams.npz), the properties every timed result has, what
the GPU tests (tests/test_gpu_timed.py) rely on in their cases, and the new C entry points' existence and argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import timed_restatement as tr
from tests.test_beam_stream_oracle import UNI_FIXTURES, fixture_oracle
from tests.test_oracle_beam import FIXTURES, fixture_nbest, load_fixture
from tests.test_oracle_decode import DECODE_CONFIGS, fixture_tokens
from tests.test_stream_oracle import chunk_batches, random_schedules, uniform_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMED_SYMBOLS = ["rnnt_hip_greedy_decode_timed", "rnnt_hip_stream_greedy_timed", "rnnt_hip_beam_search_timed",
                 "rnnt_hip_beam_stream_chunk_timed"]


def check_greedy_properties(ref, lens, max_iters):
    for b, n in enumerate(lens):
        toks, frames, logp = ref.tokens[b], ref.frames[b], ref.logp[b]
        assert len(toks) == len(frames) == len(logp)
        assert all(x <= y for x, y in zip(frames, frames[1:]))                 # non-decreasing
        assert all(0 <= f < n for f in frames)                                  # below the utterance length
        assert all(frames.count(f) <= max_iters for f in set(frames))           # at most max_iters appended tokens share a frame
        assert all(lp <= 0.0 for lp in logp)
        assert all(x != y for x, y in zip(toks, toks[1:]))                      # the dedupe rule


def check_beam_properties(nbest, blank, n_frames):
    for y, f, _ in nbest:
        assert len(y) == len(f) and y[0] == blank and f[0] == -1               # the leading blank has frame -1
        assert all(x <= z for x, z in zip(f[1:], f[2:])) and all(0 <= x < n_frames for x in f[1:])


@pytest.mark.parametrize("tag", list(DECODE_CONFIGS))
def test_restated_greedy_matches_reference_fixture(golden_dir, tag):
    from oracle.rnnt_oracle import OracleJointNet
    g = dict(np.load(os.path.join(golden_dir, tag + ".npz")))
    tn, pn, V = DECODE_CONFIGS[tag]
    net = OracleJointNet(tn, pn, V)
    net.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    net.eval()
    audios, t_list, max_iters = torch.from_numpy(g["audios"]), g["t_lens"].tolist(), int(g["max_iters"])
    ref = tr.greedy_timed(net, audios, t_list, pn["pad_token_id"], max_iters)
    assert ref.tokens == fixture_tokens(g)
    assert sum(map(len, ref.tokens)) > 0
    check_greedy_properties(ref, t_list, max_iters)


@pytest.mark.parametrize("tag", FIXTURES)
def test_restated_beams_match_reference_fixture(golden_dir, tag):
    from oracle.rnnt_oracle import OracleJointNet
    g, cfg, sd = load_fixture(golden_dir, tag)
    net = OracleJointNet(cfg["transnet"], cfg["prednet"], cfg["V"])
    net.load_state_dict(sd)
    net.eval()
    blank, t_list = cfg["prednet"]["pad_token_id"], g["t_lens"].tolist()
    ref = tr.beam_timed(net, torch.from_numpy(g["audios"]), t_list, blank, cfg["beam"], cfg["improved"], cfg["state_beam"],
                        cfg["expand_beam"], padded_batch=True)
    got = [ref.nbest(b) for b in range(len(t_list))]
    assert [[y for y, _, _ in h] for h in got] == fixture_nbest(g)
    assert ref.margin >= 1e-4
    scores = np.array([[s for _, _, s in h] + [0.0] * (g["scores"].shape[1] - len(h)) for h in got])
    assert np.allclose(scores, g["scores"], rtol=1e-5, atol=1e-5)
    for b, n in enumerate(t_list):
        check_beam_properties(got[b], blank, n)


@pytest.mark.parametrize("tag", UNI_FIXTURES)
def test_restated_streaming_beams_match_reference_fixture(tag):
    g, cfg, net = fixture_oracle(tag)
    blank = cfg["prednet"]["pad_token_id"]
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    finals = []
    for sched in (uniform_schedule(t_list, max(t_list)), uniform_schedule(t_list, 7), random_schedules(t_list, 3)):
        ref = tr.BeamTimedRef(net, len(t_list), blank, cfg["beam"], cfg["improved"], cfg["state_beam"], cfg["expand_beam"])
        for x, ns in chunk_batches(audios, t_list, sched):
            ref.feed(x, ns)
        got = [ref.nbest(b) for b in range(len(t_list))]
        assert [[y for y, _, _ in h] for h in got] == fixture_nbest(g)
        assert ref.margin >= 1e-4
        scores = np.array([[s for _, _, s in h] + [0.0] * (g["scores"].shape[1] - len(h)) for h in got])
        assert np.allclose(scores, g["scores"], rtol=1e-5, atol=1e-5)
        for b, n in enumerate(t_list):
            check_beam_properties(got[b], blank, n)
            sp, spf = ref.stable_prefix(b)
            assert all(y[:len(sp)] == sp and f[:len(sp)] == spf for y, f, _ in got[b])
        finals.append([[(y, f) for y, f, _ in h] for h in got])
    assert all(f == finals[0] for f in finals[1:])   # frames are absolute: the chunking does not show in them


@pytest.mark.parametrize("name", list(tr.GREEDY_CASES))
def test_greedy_cases_of_the_gpu_tests(name):
    """What tests/test_gpu_timed.py relies on: real tokens, decisions far from fp32 rounding, a zero-length utterance, and at
    least half of the utterances fit for the dense-joint check (no dropped duplicate, no frame that used all max_iters)."""
    ora, _, _, audios, lens, max_iters, ref = tr.greedy_case(name)
    check_greedy_properties(ref, lens, max_iters)
    assert ref.margin >= 1e-3 and 0 in lens
    assert 2 * sum(tr.qualifies(ref, b) for b in range(len(lens))) >= len(lens)
    # streaming restatement, frame by frame: the same tokens and frames, logp to float64 rounding
    st = tr.GreedyTimedRef(ora, len(lens), 0, max_iters)
    for x, ns in chunk_batches(audios, lens, uniform_schedule(lens, 1)):
        st.feed(x, ns)
    assert st.tokens == ref.tokens and st.frames == ref.frames
    assert all(abs(x - y) < 1e-9 for a, b in zip(st.logp, ref.logp) for x, y in zip(a, b))


def test_greedy_cases_cover_a_dropped_duplicate_and_an_exhausted_frame():
    refs = [tr.greedy_case(n)[-1] for n in tr.GREEDY_CASES]
    assert any(any(r.dropped) for r in refs) and any(any(r.exhausted) for r in refs)


@pytest.mark.parametrize("name", list(tr.BEAM_CASES))
def test_beam_cases_of_the_gpu_tests(name):
    ora, _, _, audios, lens, beam, improved, ref = tr.beam_case(name)
    off = [ref.nbest(b) for b in range(len(lens))]
    assert ref.margin >= 1e-4
    assert any(len(y) > 2 for h in off for y, _, _ in h)
    for b, n in enumerate(lens):
        check_beam_properties(off[b], 0, n)
    st = tr.BeamTimedRef(ora, len(lens), 0, beam, improved)   # frame by frame, the n-best asked for after every frame
    for x, ns in chunk_batches(audios, lens, uniform_schedule(lens, 1)):
        st.feed(x, ns)
        for b in range(len(lens)):
            st.nbest(b)
    assert st.margin >= 1e-4
    assert [[(y, f) for y, f, _ in st.nbest(b)] for b in range(len(lens))] == [[(y, f) for y, f, _ in h] for h in off]


def test_timed_symbols_are_declared_and_exported():
    from rnntransducer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in TIMED_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SYMBOLS
    assert _lib.lib().rnnt_hip_version() == 4   # new entries beside the old ones: the descriptors keep their layout


def test_timed_entries_reject_null_outputs_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    one = C.c_int(0)
    p = C.addressof(one)   # a non-null address: the argument check never dereferences it
    calls = [(L.rnnt_hip_greedy_decode_timed, _lib.DecodeDesc, _lib.GreedyTiming, [(None, p, None), (p, None, None)]),
             (L.rnnt_hip_stream_greedy_timed, _lib.StreamGreedyDesc, _lib.GreedyTiming, [(None, p, None), (p, None, None)]),
             (L.rnnt_hip_beam_search_timed, _lib.BeamDesc, _lib.BeamTiming, [(None, None)]),
             (L.rnnt_hip_beam_stream_chunk_timed, _lib.BeamStreamDesc, _lib.BeamTiming, [(None, p), (p, None)])]
    for fn, desc, timing, bad in calls:
        d = desc()
        assert fn(C.byref(d), None, None) == -1 and b"null timing" in L.rnnt_hip_last_error()
        for fields in bad:
            assert fn(C.byref(d), C.byref(timing(*fields)), None) == -1 and b"null timing" in L.rnnt_hip_last_error()
        assert fn(None, C.byref(timing(*([p] * len(bad[0])))), None) == -1   # complete outputs, null descriptor


def test_python_surface_has_the_keywords():
    import inspect
    from rnntransducer_amd import JointNet, LogMelFrontend, RNNTransducer
    from rnntransducer_amd.ops import TimedTokens
    from rnntransducer_amd.streaming import BeamStreamState
    assert TimedTokens._fields == ("tokens", "frames", "logp")
    for fn, kw in ((JointNet.recognize_greedy, "return_timing"), (JointNet.recognize_greedy_stream, "return_timing"),
                   (JointNet.recognize_beams, "return_frames"), (JointNet.recognize_beams_stream, "return_frames"),
                   (BeamStreamState.stable_prefix, "return_frames"), (RNNTransducer.recognize_greedy_stream, "return_timing"),
                   (RNNTransducer.recognize_beams_stream, "return_frames")):
        assert inspect.signature(fn).parameters[kw].default is False, (fn.__qualname__, kw)
    fe = LogMelFrontend()
    assert fe.frame_seconds(100) == 100 * fe.hop / fe.sample_rate == 1.0
    assert fe.frame_seconds([0, 50]) == [0.0, 0.5]
    assert torch.equal(fe.frame_seconds(torch.tensor([0, 150], dtype=torch.int32)), torch.tensor([0.0, 1.5], dtype=torch.float64))
