"""The streaming beam-search restatement (tests/beam_stream_restatement.py, CPU) pinned against
  * the offline restatement (tests/beam_restatement.py): any chunking gives the same n-best and the same scores;
  * fixtures produced by the REFERENCE's JointNet.recognize_beams on unidirectional encoders (tests/golden/s*_beams.npz, made
    by tests/golden/make_golden_beams_uni.py);
and its stable prefix checked for the properties a partial result needs."""
import os

import numpy as np
import pytest
import torch

from tests import beam_restatement
from tests.beam_stream_restatement import BeamStreamRef, common_prefix
from tests.test_oracle_beam import fixture_nbest, load_fixture
from tests.test_stream_oracle import chunk_batches, make_oracle, random_schedules, uniform_schedule

UNI_FIXTURES = ["s1_beams", "s2_beams", "s3_beams"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_oracle(tag):
    from oracle.rnnt_oracle import OracleJointNet
    g, cfg, sd = load_fixture(GOLDEN, tag)
    net = OracleJointNet(cfg["transnet"], cfg["prednet"], cfg["V"])
    net.load_state_dict(sd)
    return g, cfg, net.eval()


def fixture_schedules(t_list):
    return [uniform_schedule(t_list, max(t_list)), uniform_schedule(t_list, 1), uniform_schedule(t_list, 7), random_schedules(t_list, 3)]


def same_nbest(got, want):
    """Token lists equal; scores equal to 1e-9 relative.  The restatement's logic is chunk-invariant, torch's CPU recurrences
    are not to the last bit (a whole padded batch and a 1-frame call take different kernels), so float64 scores differ by a
    few ulp (seen: 4e-15); 1e-9 is a million times that and a hundred thousand times below the decision margins asked for."""
    assert [y for y, _ in got] == [y for y, _ in want]
    assert all(abs(s - w) <= 1e-9 * max(1.0, abs(w)) for (_, s), (_, w) in zip(got, want))
    return True


def stream_ref(net, cfg, n):
    return BeamStreamRef(net, n, cfg["prednet"]["pad_token_id"], cfg["beam"], cfg["improved"], cfg["state_beam"], cfg["expand_beam"])


@pytest.mark.parametrize("tag", UNI_FIXTURES)
def test_streaming_restatement_matches_reference_fixture(tag):
    g, cfg, net = fixture_oracle(tag)
    assert not cfg["transnet"]["bidirectional"] and float(g["margin"]) >= 1e-4
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    want = fixture_nbest(g)
    for sched in fixture_schedules(t_list):
        ref = stream_ref(net, cfg, len(t_list))
        for x, ns in chunk_batches(audios, t_list, sched):
            ref.feed(x, ns)
        got = [ref.nbest(b) for b in range(len(t_list))]
        assert [[y for y, _ in h] for h in got] == want
        assert ref.margin >= 1e-4
        scores = np.array([[s for _, s in h] + [0.0] * (g["scores"].shape[1] - len(h)) for h in got])
        assert np.allclose(scores, g["scores"], rtol=1e-5, atol=1e-5)
        for b, hyps in enumerate(want):   # the stable prefix is a prefix of every entry the reference returned
            sp = ref.stable_prefix(b)
            assert all(y[:len(sp)] == sp for y in hyps)


@pytest.mark.parametrize("cells,beam,improved", [(("lstm", "lstm"), 4, True), (("gru", "lstm"), 3, False), (("rnn", "gru"), 4, True)])
def test_any_chunking_equals_the_offline_restatement(cells, beam, improved):
    ora, _, _ = make_oracle(enc_cell=cells[0], dec_cell=cells[1])
    lens = [14, 9, 1, 0] if improved else [5, 3, 1, 0]
    audios = torch.randn(4, max(lens), 16, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    for b, n in enumerate(lens):
        audios[b, n:] = 0
    with torch.no_grad():
        want, _, _ = beam_restatement.beam_search(ora, audios[:3], lens[:3], 0, beam, improved)
    want.append([([0], 0.0)])   # no frames: the initial hypothesis (the offline encoder does not take an empty utterance)
    assert any(len(y) > 2 for y, _ in want[0])
    for sched in (uniform_schedule(lens, max(lens)), uniform_schedule(lens, 1), uniform_schedule(lens, 4), random_schedules(lens, 4)):
        ref = BeamStreamRef(ora, 4, 0, beam, improved)
        for x, ns in chunk_batches(audios, lens, sched):
            ref.feed(x, ns)
        assert all(same_nbest(ref.nbest(b), want[b]) for b in range(4))


def test_n_best_after_every_chunk_is_the_offline_result_for_the_frames_so_far():
    ora, _, _ = make_oracle()
    T = 9
    audios = torch.randn(1, T, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    ref = BeamStreamRef(ora, 1, 0, 3, True)
    assert ref.nbest(0) == [([0], 0.0)]
    for t in range(T):
        ref.feed(audios[:, t:t + 1], [1])
        with torch.no_grad():
            want, _, _ = beam_restatement.beam_search(ora, audios[:, :t + 1], [t + 1], 0, 3, True)
        assert same_nbest(ref.nbest(0), want[0])


def test_stable_prefix_properties():
    ora, _, _ = make_oracle(seed=3, fc_scale=15.0, dtype=torch.float32)   # a confident model: the beam agrees on a long prefix
    lens = [40, 31]
    audios = torch.randn(2, 40, 16, generator=torch.Generator().manual_seed(103))
    for b, n in enumerate(lens):
        audios[b, n:] = 0
    ref = BeamStreamRef(ora, 2, 0, 4, True)
    history = [[[0]], [[0]]]
    for x, ns in chunk_batches(audios, lens, random_schedules(lens, 6, max_chunk=5)):
        ref.feed(x, ns)
        for b in range(2):
            sp = ref.stable_prefix(b)
            assert sp == common_prefix([h["y"] for h in ref.hyps[b]])         # what it is
            assert sp[:len(history[b][-1])] == history[b][-1]                  # it never shrinks and never changes
            for earlier in history[b]:
                assert all(y[:len(earlier)] == earlier for y, _ in ref.nbest(b))   # a prefix of every later n-best entry
            history[b].append(sp)
    assert min(len(h[-1]) for h in history) >= 5   # leading blank + at least 4 tokens: the property is not vacuous


def test_reset_starts_a_fresh_utterance():
    ora, _, _ = make_oracle()
    g = torch.Generator().manual_seed(2)
    first, second = torch.randn(2, 6, 16, dtype=torch.float64, generator=g), torch.randn(2, 8, 16, dtype=torch.float64, generator=g)
    ref, fresh, cont = (BeamStreamRef(ora, 2, 0, 3, True) for _ in range(3))
    ref.feed(first, [6, 6])
    ref.reset([1])
    assert ref.nbest(1) == [([0], 0.0)] and ref.stable_prefix(1) == [0]
    ref.feed(second, [8, 8])
    fresh.feed(second, [8, 8])
    cont.feed(first, [6, 6])
    cont.feed(second, [8, 8])
    assert ref.nbest(1) == fresh.nbest(1) and ref.nbest(0) == cont.nbest(0)
