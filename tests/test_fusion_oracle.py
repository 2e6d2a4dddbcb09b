"""Token-level fusion on the CPU: the automaton builders (rnntransducer_amd/fusion.py) against separately written scorers, and
the fused restatement (tests/fusion_restatement.py) tied to the REFERENCE's fixtures through the all-zero automaton.  The
decision margins of every case the GPU tests use are asserted here first."""
import os
import random

import pytest
import torch

from tests import beam_restatement, fusion_cases, fusion_restatement
from tests.test_beam_stream_oracle import UNI_FIXTURES, fixture_oracle
from tests.test_oracle_beam import FIXTURES, fixture_nbest
from tests.test_stream_oracle import chunk_batches, random_schedules, uniform_schedule


def _opts(cfg):
    return cfg["prednet"]["pad_token_id"], cfg["beam"], cfg["improved"], cfg["state_beam"], cfg["expand_beam"]


# 1. the all-zero automaton: the fused restatement is the reference's search ---------------------------------------------------
@pytest.mark.parametrize("tag", FIXTURES + UNI_FIXTURES)
def test_zero_automaton_restatement_returns_the_reference_fixture(tag):
    from rnntransducer_amd import TokenFusion
    assert TokenFusion is not None
    g, cfg, net = fixture_oracle(tag)
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    got, margin, _, _ = fusion_restatement.fused_beam_search(net, audios, t_list, fusion_cases.zero_fusion(cfg["V"]), *_opts(cfg))
    assert [[y for y, _, _ in h] for h in got] == fixture_nbest(g)
    assert all(a == f for h in got for _, a, f in h)   # total 0, final 0: the fused score is the ASR score, bit for bit
    want, want_margin, _ = beam_restatement.beam_search(net, audios, t_list, *_opts(cfg))
    assert [[(y, a) for y, a, _ in h] for h in got] == want and margin == want_margin   # and the unfused restatement's bits


# 2. the builders -----------------------------------------------------------------------------------------------------------------
def _brute_hotword_total(y, phrases, weight):
    """Written apart from the builder: walk y_star; after each token the match in progress is the LONGEST suffix of the tokens
    since the last completion that is a prefix of a phrase; when that suffix is a whole phrase it is completed (its length is
    banked, matching restarts).  -> (weight * (banked + depth), depth)."""
    banked, seg = 0, []
    for k in y[1:]:
        seg.append(k)
        depth = 0
        for n in range(len(seg), 0, -1):
            if any(p[:n] == seg[-n:] for p in phrases):
                depth = n
                break
        if depth and seg[-depth:] in phrases:
            banked += depth
            seg = []
    depth = 0
    for n in range(len(seg), 0, -1):
        if any(p[:n] == seg[-n:] for p in phrases):
            depth = n
            break
    return weight * (banked + depth), depth


PHRASE_SETS = [[[4, 6, 4]], [[4, 5], [4, 6, 4]], [[1, 2, 3, 4], [2, 3], [3, 1]], [[1, 2, 1, 3], [2, 1, 2], [5]],
               [[1, 2, 3, 1, 2, 4], [3, 1, 2, 3], [2, 4, 1]]]


@pytest.mark.parametrize("phrases", PHRASE_SETS)
def test_from_hotwords_agrees_with_a_brute_force_scorer(phrases):
    from rnntransducer_amd import TokenFusion
    V, blank, weight = 7, 0, 0.75
    f = TokenFusion.from_hotwords(phrases, weight, V, blank)
    assert f.n_states == 1 + len({tuple(p[:n]) for p in phrases for n in range(1, len(p))}) and f.vocab_size == V
    depth_of = [0] * f.n_states   # depth of a state = -final / weight
    for s in range(f.n_states):
        depth_of[s] = round(-float(f.final[s]) / weight)
    rng = random.Random(len(phrases) * 31 + len(phrases[0]))
    met_completion = met_revoke = 0
    for _ in range(1000):
        y = [blank]
        for _ in range(rng.randint(0, 14)):
            y.append(rng.choice([k for k in range(1, V) if k != y[-1]]))   # y_star never repeats a token back to back
        total, final, state = f.score(y)
        want, depth = _brute_hotword_total(y, phrases, weight)
        assert total == want, (y, total, want)                 # multiples of 0.75: exact in fp32 and fp64
        assert depth_of[state] == depth and final == -weight * depth
        met_completion += want > weight * depth
        met_revoke += any(float(f.arc[s, k]) < 0 for s, k in _path(f, y))
    assert met_completion > 10 and met_revoke > 10   # strings that bank a phrase, strings that lose a partial match
    # the identity of the docstring, on the tables: arc = weight * (depth(target) - depth(s)), unreduced on completion
    trie = {tuple(p[:n]) for p in phrases for n in range(len(p) + 1)}
    for s in range(f.n_states):
        for k in range(V):
            gain = float(f.arc[s, k]) / weight + depth_of[s]      # depth of the goto target
            nxt = int(f.next[s, k])
            assert gain == depth_of[nxt] or (nxt == 0 and gain >= 1 and gain in {len(p) for p in phrases})
    assert len(trie) - len(phrases) == f.n_states


def _path(f, y):
    s = 0
    for k in y[1:]:
        yield s, k
        s = int(f.next[s, k])


def test_from_bigram_totals_are_the_summed_table_entries():
    from rnntransducer_amd import TokenFusion
    V, blank, weight = 9, 3, 0.3
    logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(4)), dim=1)
    f = TokenFusion.from_bigram(logp, weight, blank)
    assert f.n_states == V and float(f.final.abs().max()) == 0.0
    table = (weight * logp.double()).float()
    rng = random.Random(2)
    for _ in range(200):
        y = [blank]
        for _ in range(rng.randint(0, 12)):
            y.append(rng.choice([k for k in range(V) if k != blank and k != y[-1]]))
        want = 0.0
        for prev, k in zip(y, y[1:]):
            want += float(table[prev, k])          # fp64 sum of the fp32 entries, in append order
        total, final, _ = f.score(y)
        assert total == want and final == 0.0
    assert f.score([blank]) == (0.0, 0.0, 0)


def test_builders_and_constructor_refuse_bad_input():
    from rnntransducer_amd import TokenFusion
    hot = lambda phrases, weight=0.5, V=8, blank=0: TokenFusion.from_hotwords(phrases, weight, V, blank)
    for bad in ([], [[]], [[1, 2], []], [[8]], [[-1, 2]], [[1, 0, 2]], [[1, 2, 2, 3]], [[1, 2], [1, 2, 3]], [[1, 2, 3], [1, 2]],
                [[1, 2], [1, 2]]):
        with pytest.raises(ValueError):
            hot(bad)
    for w in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            hot([[1, 2]], weight=w)
    assert hot([[1, 2], [2, 1, 3]]).n_states == 4
    nxt, arc, fin = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5), torch.zeros(2)
    TokenFusion(nxt, arc, fin)
    bad_next, bad_arc, bad_fin = nxt.clone(), arc.clone(), fin.clone()
    bad_next[1, 2], bad_arc[0, 0], bad_fin[1] = 2, float("nan"), float("inf")
    for args in ((nxt.long(), arc, fin), (nxt, arc.double(), fin), (nxt, arc, fin.double()), (nxt, arc[:1], fin), (nxt, arc, fin[:1]),
                 (nxt[0], arc[0], fin), (bad_next, arc, fin), (-1 - nxt, arc, fin), (nxt, bad_arc, fin), (nxt, arc, bad_fin)):
        with pytest.raises(ValueError):
            TokenFusion(*args)
    meta = lambda *shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device="meta")
    with pytest.raises(ValueError, match="2\\^27"):
        TokenFusion(meta(1 << 14, (1 << 13) + 1, dt=torch.int32), meta(1 << 14, (1 << 13) + 1), meta(1 << 14))
    with pytest.raises(ValueError):
        TokenFusion.from_bigram(torch.zeros(4, 5), 0.3, 0)
    with pytest.raises(ValueError):
        TokenFusion.from_bigram(torch.zeros(4, 4), 0.3, 4)
    assert TokenFusion(nxt, arc, fin).to("cpu").device.type == "cpu"


# 3. the cases of the GPU tests: their margins, here first ----------------------------------------------------------------------
@pytest.mark.parametrize("tag,weight,phrases,rows", fusion_cases.FIXTURE_CASES)
def test_fixture_cases_have_their_margin_and_change_the_lists(tag, weight, phrases, rows):
    from rnntransducer_amd import TokenFusion
    g, cfg, net = fixture_oracle(tag)
    fusion = TokenFusion.from_hotwords(phrases, weight, cfg["V"], cfg["prednet"]["pad_token_id"])
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    got, _, margins, _ = fusion_restatement.fused_beam_search(net, audios, t_list, fusion, *_opts(cfg), max_pops=1024)
    want = fixture_nbest(g)
    assert all(margins[b] >= 1e-4 for b in rows), margins
    assert any([y for y, _, _ in got[b]] != want[b] for b in rows)   # the automaton decides something
    for b in rows:
        for y, a, f in got[b]:
            total, final, _ = fusion.score(y)
            assert f == a + total + final


def test_fixture_cases_change_a_top_hypothesis_and_score_nonzero_totals():
    from rnntransducer_amd import TokenFusion
    tops, nonzero = 0, 0
    for tag, weight, phrases, rows in fusion_cases.FIXTURE_CASES[:2]:
        g, cfg, net = fixture_oracle(tag)
        fusion = TokenFusion.from_hotwords(phrases, weight, cfg["V"], 0)
        got, _, _, _ = fusion_restatement.fused_beam_search(net, torch.from_numpy(g["audios"]), g["t_lens"].tolist(), fusion, *_opts(cfg))
        tops += sum(got[b][0][0] != fixture_nbest(g)[b][0] for b in rows)
        nonzero += sum(f != a for b in rows for _, a, f in got[b])
    assert tops >= 1 and nonzero >= 1


def _stream_fusion(cfg):
    from rnntransducer_amd import TokenFusion
    return TokenFusion.from_hotwords(fusion_cases.STREAM_PHRASES, fusion_cases.STREAM_WEIGHT, cfg["V"], cfg["prednet"]["pad_token_id"])


@pytest.mark.parametrize("tag", UNI_FIXTURES)
def test_streaming_restatement_is_chunk_invariant_and_equals_the_offline_one(tag):
    """On the streams the GPU test compares with the restatement (STREAM_ROWS: the others fall below 1e-4, s1 rows 0 and 1 at
    1.1e-5 and 8.9e-5): any chunking gives the offline fused result, and the one-frame-at-a-time margin, the n-best sort after
    every frame included, is >= 1e-4."""
    g, cfg, net = fixture_oracle(tag)
    fusion = _stream_fusion(cfg)
    rows = fusion_cases.STREAM_ROWS[tag]
    audios, t_list = torch.from_numpy(g["audios"])[rows], [g["t_lens"].tolist()[b] for b in rows]
    want, _, margins, _ = fusion_restatement.fused_beam_search(net, audios, t_list, fusion, *_opts(cfg))
    assert min(margins) >= 1e-4
    for sched in (uniform_schedule(t_list, 1), random_schedules(t_list, 3)):
        ref = fusion_restatement.FusedBeamStreamRef(net, len(t_list), fusion, *_opts(cfg))
        for x, ns in chunk_batches(audios, t_list, sched):
            ref.feed(x, ns)
            for b, n in enumerate(ns):
                got = ref.nbest(b)
                sp = ref.stable_prefix(b)
                assert all(y[:len(sp)] == sp for y, _, _ in got)
        for b in range(len(t_list)):
            got = ref.nbest(b)
            assert [y for y, _, _ in got] == [y for y, _, _ in want[b]]
            # fp32 models: torch's CPU recurrences differ between a padded batch and short chunks in the last bits (the
            # tolerance of tests/test_beam_stream_oracle.py for these fixtures)
            assert all(abs(a - wa) <= 1e-5 * max(1.0, abs(wa)) and abs(f - wf) <= 1e-5 * max(1.0, abs(wf))
                       for (_, a, f), (_, wa, wf) in zip(got, want[b]))
        assert ref.margin() >= 1e-4
    if tag == "s1_beams":   # row 2: the automaton changes the list
        assert [y for y, _, _ in want[0]] != fixture_nbest(g)[2]


@pytest.mark.parametrize("cell,layers,beam,improved,kind", fusion_cases.CONFIG2_CASES)
def test_config2_seed_range_holds_a_seed_with_margin(cell, layers, beam, improved, kind):
    """What the GPU test's seed loop needs: the seed it starts at takes no decision within 1e-4 in the fused restatement."""
    first = fusion_cases.CONFIG2_FIRST_SEED[(cell, layers, kind)]
    assert first in fusion_cases.CONFIG2_SEEDS
    seed, want, fusion = fusion_cases.config2_first_seed(cell, layers, beam, improved, kind, seeds=[first])
    assert seed == first, "the decision margin of that seed is < 1e-4"
    assert any(f != a for h in want for _, a, f in h)   # the automaton scores something


def test_big_vocabulary_seed_range_holds_a_seed_with_margin():
    assert fusion_cases.BIGV_FIRST_SEED in fusion_cases.BIGV_SEEDS
    seed, want, fusion = fusion_cases.bigv_first_seed([fusion_cases.BIGV_FIRST_SEED])
    assert seed == fusion_cases.BIGV_FIRST_SEED
    assert any(f != a for h in want for _, a, f in h) and any(len(y) > 1 for h in want for y, _, _ in h)


def test_a_large_bonus_makes_a_frame_run_away():
    """README / fusion.py "Runaway frames": at weight 1.5 a hypothesis of b2 keeps completing [4, 5] and gains more than its
    log-probability falls; the restatement's frame loop passes any bound (the kernel's max_pops ends it)."""
    from rnntransducer_amd import TokenFusion
    g, cfg, net = fixture_oracle("b2_beams")
    fusion = TokenFusion.from_hotwords([[4, 5], [4, 6, 4]], 1.5, cfg["V"], 0)
    with pytest.raises(RuntimeError, match="runaway"):
        fusion_restatement.fused_beam_search(net, torch.from_numpy(g["audios"]), g["t_lens"].tolist(), fusion, *_opts(cfg), max_pops=300)
