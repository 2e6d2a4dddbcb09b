"""Beam search with token-level fusion on the GPU (the FUSED instance of csrc/beam_shared.hpp, offline and streaming) vs the CPU
restatement (tests/fusion_restatement.py), the unfused search (all-zero automaton: same bits), itself under re-chunking
(bitwise), and its guards.  Every case compared with the restatement has a decision margin >= 1e-4 there, asserted on the CPU
by tests/test_fusion_oracle.py; scores are held to 1e-4 * max(1, |s|), the tolerance of tests/test_gpu_beam.py."""
import os

import pytest
import torch

from tests import fusion_cases, fusion_restatement
from tests.test_beam_stream_oracle import UNI_FIXTURES, fixture_oracle
from tests.test_oracle_beam import FIXTURES, fixture_nbest, load_fixture
from tests.test_stream_oracle import chunk_batches, random_schedules, uniform_schedule

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _jointnet(tn, pn, V, sd):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in sd.items()})
    return net.cuda().eval()


def _fixture_net(tag):
    g, cfg, sd = load_fixture(GOLDEN, tag)
    net = _jointnet(cfg["transnet"], cfg["prednet"], cfg["V"], sd)
    opts = dict(beam_widths=cfg["beam"], improved=cfg["improved"], state_beam=cfg["state_beam"], expand_beam=cfg["expand_beam"])
    return g, cfg, net, torch.from_numpy(g["audios"]), g["t_lens"].tolist(), cfg["prednet"]["pad_token_id"], opts


def _ref_opts(cfg):
    return cfg["prednet"]["pad_token_id"], cfg["beam"], cfg["improved"], cfg["state_beam"], cfg["expand_beam"]


def _close(s, w):
    return abs(s - w) <= 1e-4 * max(1.0, abs(w))


def _same(got, want):
    """One utterance: lists equal, asr_score and fused_score within the tolerance."""
    assert [y for y, _, _ in got] == [y for y, _, _ in want], (got, want)
    for (_, a, f), (_, wa, wf) in zip(got, want):
        assert _close(a, wa) and _close(f, wf), (a, wa, f, wf)


# 1. the reference's fixtures with hotword automata, against the restatement -----------------------------------------------------
@pytest.mark.parametrize("tag,weight,phrases,rows", fusion_cases.FIXTURE_CASES)
def test_fused_beams_match_the_restatement_on_fixtures(tag, weight, phrases, rows):
    from rnntransducer_amd import TokenFusion
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    _, _, ora = fixture_oracle(tag)
    fusion = TokenFusion.from_hotwords(phrases, weight, cfg["V"], blank)
    want, _, margins, _ = fusion_restatement.fused_beam_search(ora, audios, t_list, fusion, *_ref_opts(cfg))
    assert all(margins[b] >= 1e-4 for b in rows)
    got = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=fusion.to("cuda"), **opts)
    unfused = net.recognize_beams(audios.cuda(), t_list, blank, **opts)
    assert unfused == fixture_nbest(g)                       # the unfused call is still the reference's
    for b in rows:
        _same(got[b], want[b])
        for y, a, f in got[b]:                                # fused_score = asr_score + total + final of that y_star
            total, final, _ = fusion.score(y)
            assert abs(f - (a + total + final)) <= 1e-12 * max(1.0, abs(f))
    assert any([y for y, _, _ in got[b]] != unfused[b] for b in rows)
    if tag == "b2_beams":
        assert any(got[b][0][0] != unfused[b][0] for b in rows)   # a top hypothesis changes
    if len(phrases) == 2:
        assert any(f != a for b in rows for _, a, f in got[b])    # nonzero totals in the output
    # each row alone (the reference's call shape) gives the batch's lists
    for b in rows:
        alone = net.recognize_beams(audios[b:b + 1, :t_list[b]].contiguous().cuda(), [t_list[b]], blank, return_scores=True,
                                    fusion=fusion.to("cuda"), **opts)
        _same(alone, got[b])


# 2. the all-zero automaton is the unfused search, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("tag", FIXTURES)
def test_zero_automaton_gives_the_unfused_lists_and_score_bits(tag):
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    zero = fusion_cases.zero_fusion(cfg["V"]).to("cuda")
    unfused = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, **opts)
    assert [[y for y, _ in h] for h in unfused] == fixture_nbest(g)
    fused = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=zero, **opts)
    assert [[(y, a) for y, a, _ in h] for h in fused] == unfused          # python floats: == is bitwise
    assert all(f == a for h in fused for _, a, f in h)
    fr_unfused = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, return_frames=True, **opts)
    fr_fused = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, return_frames=True, fusion=zero, **opts)
    assert [[e[:3] for e in h] for h in fr_fused] == fr_unfused and all(e[3] == e[2] for h in fr_fused for e in h)


@pytest.mark.parametrize("tag", UNI_FIXTURES[1:])
def test_zero_automaton_stream_gives_the_unfused_stream_bits(tag):
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    zero = fusion_cases.zero_fusion(cfg["V"]).to("cuda")
    plain, fused = net.init_beam_stream(len(t_list), blank, **opts), net.init_beam_stream(len(t_list), blank, fusion=zero, **opts)
    assert fused.workspace_bytes > plain.workspace_bytes
    for x, ns in chunk_batches(audios, t_list, random_schedules(t_list, 5)):
        a = net.recognize_beams_stream(x.cuda(), ns, plain, return_scores=True)
        b = net.recognize_beams_stream(x.cuda(), ns, fused, return_scores=True)
        assert [[(y, s) for y, s, _ in h] for h in b] == a and all(f == s for h in b for _, s, f in h)
        assert [plain.stable_prefix(i) for i in range(len(t_list))] == [fused.stable_prefix(i) for i in range(len(t_list))]
    assert [[y for y, _ in h] for h in a] == fixture_nbest(g)


# 3. the prediction net at config-2 size, bigram and hotword automata -------------------------------------------------------------
@pytest.mark.parametrize("cell,layers,beam,improved,kind", fusion_cases.CONFIG2_CASES)
def test_fused_beams_vs_restatement_config2_sizes(cell, layers, beam, improved, kind):
    """The seed loop and margin gate of test_gpu_beam.test_beams_vs_restatement_config2_sizes, started at the first seed of the
    range that the CPU test found to have a margin (the loop still skips a seed whose margin is < 1e-4 here)."""
    first = fusion_cases.CONFIG2_FIRST_SEED[(cell, layers, kind)]
    kept = 0
    for seed in range(first, fusion_cases.CONFIG2_SEEDS.stop):
        ora, tn, pn, audios, lens = fusion_cases.config2_model(cell, layers, seed)
        fusion = fusion_cases.config2_fusion(kind, ora, audios, lens, beam, improved, seed)
        want, margin, _, stats = fusion_restatement.fused_beam_search(ora, audios, lens, fusion, 0, beam, improved, max_pops=1024)
        if margin < 1e-4:
            continue
        net = _jointnet(tn, pn, 72, ora.state_dict())
        got = net.recognize_beams(audios.cuda(), lens, 0, beam, improved, return_scores=True, fusion=fusion.to("cuda"))
        for gh, wh in zip(got, want):
            _same(gh, wh)
        assert sum(st["pops"] for st in stats) > 2 * sum(lens)          # the search really branches
        assert any(len(y) > 1 for h in want for y, _, _ in h)            # emits symbols
        assert any(f != a for h in want for _, a, f in h)                # and the automaton scores them
        kept += 1
        break
    assert kept >= 1, "no seed with a decision margin >= 1e-4"


def test_fused_beams_with_a_vocabulary_larger_than_the_workgroup():
    """V = 300: the children loop takes several passes of the workgroup, each with its fusion loads (bigram automaton, S = 300)."""
    kept = 0
    for seed in range(fusion_cases.BIGV_FIRST_SEED, fusion_cases.BIGV_SEEDS.stop):
        ora, tn, pn, audios, lens = fusion_cases.bigv_model(seed)
        fusion = fusion_cases.bigram_fusion(fusion_cases.BIGV["V"], 0, seed)
        beam, improved = fusion_cases.BIGV["beam"], fusion_cases.BIGV["improved"]
        want, margin, _, _ = fusion_restatement.fused_beam_search(ora, audios, lens, fusion, 0, beam, improved, max_pops=1024)
        if margin < 1e-4:
            continue
        net = _jointnet(tn, pn, fusion_cases.BIGV["V"], ora.state_dict())
        got = net.recognize_beams(audios.cuda(), lens, 0, beam, improved, return_scores=True, fusion=fusion.to("cuda"))
        for gh, wh in zip(got, want):
            _same(gh, wh)
        assert any(len(y) > 1 for h in want for y, _, _ in h) and any(f != a for h in want for _, a, f in h)
        kept += 1
        break
    assert kept >= 1, "no seed with a decision margin >= 1e-4"


# 4. determinism, frames ---------------------------------------------------------------------------------------------------------
def test_fused_calls_are_bit_identical_and_return_frames():
    from rnntransducer_amd import TokenFusion
    tag, weight, phrases, rows = fusion_cases.FIXTURE_CASES[1]
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    fusion = TokenFusion.from_hotwords(phrases, weight, cfg["V"], blank).to("cuda")
    a = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=fusion, **opts)
    b = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=fusion, **opts)
    assert a == b
    assert net.recognize_beams(audios.cuda(), t_list, blank, fusion=fusion, **opts) == [[y for y, _, _ in h] for h in a]
    timed = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, return_frames=True, fusion=fusion, **opts)
    assert [[(y, s, f) for y, _, s, f in h] for h in timed] == a            # the timed fused entry: the same bits
    for u, hyps in enumerate(timed):
        for y, frames, _, _ in hyps:
            assert len(frames) == len(y) and frames[0] == -1
            assert all(0 <= p <= q < t_list[u] for p, q in zip(frames[1:], frames[2:])) and all(0 <= f < t_list[u] for f in frames[1:])
    pairs = net.recognize_beams(audios.cuda(), t_list, blank, return_frames=True, fusion=fusion, **opts)
    assert pairs == [[(y, fr) for y, fr, _, _ in h] for h in timed]


# 5. streaming ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", UNI_FIXTURES)
def test_fused_stream_is_chunk_invariant_and_equals_offline_and_restatement(tag):
    """Hotwords [[4, 6, 4]] at weight 0.5.  Three chunkings give bitwise equal lists and both scores wherever they meet at the
    same number of frames.  After every one-frame chunk the streams whose restatement margin is >= 1e-4 (STREAM_ROWS; the
    n-best sorts after every frame included) equal the restatement and the offline fused recognize_beams on the frames so far
    (other encoder kernels than the streaming ones, so scores to the tolerance and lists only where the margin holds).  The
    stable prefix never shrinks and is a prefix of every later answer."""
    from rnntransducer_amd import TokenFusion
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    _, _, ora = fixture_oracle(tag)
    cpu_fusion = TokenFusion.from_hotwords(fusion_cases.STREAM_PHRASES, fusion_cases.STREAM_WEIGHT, cfg["V"], blank)
    fusion = cpu_fusion.to("cuda")
    rows, B = fusion_cases.STREAM_ROWS[tag], len(t_list)
    ref = fusion_restatement.FusedBeamStreamRef(ora, B, cpu_fusion, *_ref_opts(cfg), only=rows)
    seen, shared = {}, 0
    scheds = [uniform_schedule(t_list, max(t_list)), uniform_schedule(t_list, 1), random_schedules(t_list, 3)]
    for si, sched in enumerate(scheds):
        state = net.init_beam_stream(B, blank, fusion=fusion, **opts)
        assert state.results(True) == [[([blank], 0.0, 0.0)]] * B
        fed, prefix = [0] * B, [[blank] for _ in range(B)]
        for x, ns in chunk_batches(audios, t_list, sched):
            out = net.recognize_beams_stream(x.cuda(), ns, state, return_scores=True)
            fed = [f + n for f, n in zip(fed, ns)]
            for b in range(B):
                if (b, fed[b]) in seen:
                    assert out[b] == seen[(b, fed[b])], (b, fed[b])    # python floats: == is bitwise
                    shared += 1
                else:
                    seen[(b, fed[b])] = out[b]
                sp = state.stable_prefix(b)
                assert sp[:len(prefix[b])] == prefix[b] and all(y[:len(sp)] == sp for y, _, _ in out[b])
                prefix[b] = sp
            if si == 1:
                ref.feed(x, ns)
                off = net.recognize_beams(audios[:, :max(fed)].contiguous().cuda(), fed, blank, return_scores=True, fusion=fusion, **opts)
                off = [off] if B == 1 else off
                for b in rows:
                    _same(out[b], ref.nbest(b))
                    _same(out[b], off[b])
                    assert state.stable_prefix(b) == ref.stable_prefix(b)
        assert state.frames_seen.tolist() == t_list
    assert shared >= 2 * B and all(ref.margin(b) >= 1e-4 for b in rows)
    if tag == "s1_beams":   # the automaton decides something: row 2's list is not the unfused fixture's
        assert [y for y, _, _ in seen[(2, t_list[2])]] != fixture_nbest(g)[2]


def test_fused_stream_reset_restarts_the_automaton_and_frames_work():
    """A two-phrase automaton on s1 ([8, 6] is completed by every returned hypothesis: total 0.6): after reset(rows) a stream's carried B entry is back in state 0 with total 0, so the
    same utterance gives the same bits again; the other streams are untouched.  return_frames runs the timed fused entry."""
    from rnntransducer_amd import TokenFusion
    g, cfg, net, audios, t_list, blank, opts = _fixture_net("s1_beams")
    fusion = TokenFusion.from_hotwords([[8, 6], [8, 9]], 0.3, cfg["V"], blank).to("cuda")
    B = len(t_list)
    state = net.init_beam_stream(B, blank, fusion=fusion, **opts)
    first = None
    for x, ns in chunk_batches(audios, t_list, uniform_schedule(t_list, 5)):
        first = net.recognize_beams_stream(x.cuda(), ns, state, return_scores=True, return_frames=True)
    assert any(f != a for h in first for _, _, a, f in h)       # nonzero totals or finals are carried
    plain = net.init_beam_stream(B, blank, fusion=fusion, **opts)
    for x, ns in chunk_batches(audios, t_list, uniform_schedule(t_list, 5)):
        untimed = net.recognize_beams_stream(x.cuda(), ns, plain, return_scores=True)
    assert [[(y, a, f) for y, _, a, f in h] for h in first] == untimed          # timed and untimed fused chunks: the same bits
    for hyps in first:
        for y, frames, _, _ in hyps:
            assert len(frames) == len(y) and frames[0] == -1 and all(p <= q for p, q in zip(frames[1:], frames[2:]))
    state.reset([2, 0])
    assert state.results(True)[2] == [([blank], 0.0, 0.0)] and state.results(True)[1] == [(y, a, f) for y, _, a, f in first[1]]
    keep = [0, 2]
    lens2 = [t_list[b] if b in keep else 0 for b in range(B)]
    again = None
    for x, ns in chunk_batches(audios, lens2, uniform_schedule(lens2, 7)):   # stream 1 gets no frames: its list stays
        again = net.recognize_beams_stream(x.cuda(), ns, state, return_scores=True, return_frames=True)
    assert [again[b] for b in keep] == [first[b] for b in keep] and again[1] == first[1]


# 6. caps and guards -------------------------------------------------------------------------------------------------------------
def test_fused_max_pops_raises_and_the_next_call_succeeds():
    """A runaway frame (a bonus that outgrows the log-probabilities) ends the same way: RnntHipError naming max_pops."""
    from rnntransducer_amd import TokenFusion
    from rnntransducer_amd._lib import RnntHipError
    tag, weight, phrases, rows = fusion_cases.FIXTURE_CASES[1]
    g, cfg, net, audios, t_list, blank, opts = _fixture_net(tag)
    fusion = TokenFusion.from_hotwords(phrases, weight, cfg["V"], blank).to("cuda")
    good = net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=fusion, **opts)
    with pytest.raises(RnntHipError, match="max_pops"):
        net.recognize_beams(audios.cuda(), t_list, blank, fusion=fusion, max_pops=2, **opts)
    runaway = TokenFusion.from_hotwords(phrases, 1.5, cfg["V"], blank).to("cuda")     # tests/test_fusion_oracle.py: never ends
    with pytest.raises(RnntHipError, match="max_pops"):
        net.recognize_beams(audios.cuda(), t_list, blank, fusion=runaway, max_pops=64, **opts)
    assert net.recognize_beams(audios.cuda(), t_list, blank, return_scores=True, fusion=fusion, **opts) == good
    g, cfg, net, audios, t_list, blank, opts = _fixture_net("s2_beams")
    state = net.init_beam_stream(len(t_list), blank, fusion=fusion_cases.zero_fusion(cfg["V"]).to("cuda"), max_pops=1, **opts)
    with pytest.raises(RnntHipError, match="max_pops"):
        net.recognize_beams_stream(audios.cuda(), t_list, state)
    state.reset(range(len(t_list)))
    assert state.results(False) == [[[blank]]] * len(t_list)


def test_fusion_guards_refuse_before_any_launch():
    from rnntransducer_amd import TokenFusion
    g, cfg, net, audios, t_list, blank, opts = _fixture_net("s2_beams")
    V = cfg["V"]
    good = TokenFusion.from_hotwords([[4, 6, 4]], 0.5, V, blank)
    wrong_v = TokenFusion.from_hotwords([[4, 6, 4]], 0.5, V + 1, blank).to("cuda")
    for bad in (good, wrong_v, object()):                      # on the CPU; over another vocabulary; not a TokenFusion
        with pytest.raises(ValueError):
            net.recognize_beams(audios.cuda(), t_list, blank, fusion=bad, **opts)
        with pytest.raises(ValueError):
            net.init_beam_stream(len(t_list), blank, fusion=bad, **opts)
    with pytest.raises(NotImplementedError, match="fusion="):
        net.recognize_beams(audios.cuda(), t_list, blank, lm=object(), **opts)
    with pytest.raises(NotImplementedError, match="fusion="):
        net.recognize_beams(audios.cuda(), t_list, blank, hotwords=["x"], fusion=good.to("cuda"), **opts)
    assert net.recognize_beams(audios.cuda(), t_list, blank, fusion=good.to("cuda"), **opts)   # and a good one runs
