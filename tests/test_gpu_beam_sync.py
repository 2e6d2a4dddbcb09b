"""The frame-synchronous transducer beam search on the GPU (csrc/beam_sync.hip) against its float64 restatement
(tests/beam_sync_restatement.py), a brute force over all paths, greedy search, and itself (bitwise).  Every case compared with the
restatement keeps a boundary margin >= 1e-4 there, asserted on the CPU by tests/test_beam_sync_oracle.py; token lists and
frames are exact, scores agree to 1e-5 relative (fp32 log-probabilities, about 1e-6 off each, summed in fp64 over at most a few
dozen choices), and output order is compared only across pairs at least 1e-4 apart.  The shapes are the smallest at which each
mechanism can go wrong; every reference is computed once (tests/beam_sync_cases.py)."""
import math

import pytest
import torch

from tests import beam_sync_cases as K
from tests import beam_sync_restatement as R

pytestmark = pytest.mark.gpu


def _jointnet(tn, pn, V, ora):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    return net.cuda().eval()


def _entries(hyps):
    """(y, frames, score[, fused]) of the model-level call -> the restatement's (y, score[, fused], frames)"""
    return [(e[0], *e[2:], e[1]) for e in hyps]


def _decode(net, x, lens, blank, W, S, **kw):
    out = net.recognize_beams_sync(x.cuda(), lens, blank, W, S, return_scores=True, return_frames=True, **kw)
    return _entries(out) if len(lens) == 1 else [_entries(h) for h in out]


def _ops_search(net, enc_tm, t_lens, blank, W, S, **kw):
    """ops.beam_search_sync on given encoder outputs (T,B,Oe): entries (y, score[, fused], frames)"""
    from rnntransducer_amd import ops
    dec = net.decoder
    return ops.beam_search_sync(enc_tm, net.fc.weight, net.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                                dec.out_proj.weight, dec.out_proj.bias, blank, W, S, t_lens, frames=True, **kw)


def _encode(net, x, lens):
    from rnntransducer_amd.networks.encoder import lengths_to_device
    with torch.no_grad():
        return net.encoder.forward_time_major(x.cuda(), lengths_to_device(lens, "cuda")).contiguous()


# shape cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.SHAPE_CASES, ids=K.case_id)
def test_shape_cases_match_the_restatement(c):
    T, V, Hp, L, cell, W, S, O, min_logp, _ = c
    _, ora, tn, pn, x, want = K.shape_case(c)
    net = _jointnet(tn, pn, V, ora)
    got = _decode(net, x, [T], 0, W, S, token_min_logp=min_logp)
    K.same_hyps(got, want.hyps)
    assert all(len(y) <= 1 + S * T for y, _, _ in got)


# 1. W = 1 against greedy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", K.GREEDY)
def test_width_one_is_greedy_search(g):
    """recognize_greedy drops a token that repeats the last appended one (it still advances the prediction net) and its
    TimedTokens.logp lists the appended tokens only, so: the tokens are compared under that rule, and the score against the sum
    of TimedTokens.logp plus the float64 log-probabilities of the choices it does not list (the blanks and the dropped
    repeats), to 1e-6 relative."""
    S, T, V, Hp = g
    _, ora, tn, pn, x, (tokens, picks), want = K.greedy_case(*g)
    net = _jointnet(tn, pn, V, ora)
    (y, score, frames), = _decode(net, x, [T], 0, 1, S)
    timed = net.recognize_greedy(x.cuda(), [T], 0, max_iters=S, return_timing=True)
    assert y == tokens                                                         # the float64 greedy search, nothing dropped
    assert R.drop_repeats(y[1:], 0) == timed.tokens.tolist()                   # recognize_greedy, exactly
    listed, last, rest = [], 0, 0.0
    for t, k, lp in picks:   # what TimedTokens lists: a token that differs from the last appended one
        if k != 0 and k != last:
            listed.append(t)
            last = k
        else:
            rest += lp
    assert listed == timed.frames.tolist()
    total = float(timed.logp.double().sum()) + rest
    print("W=1 S=%d: score %.9f, greedy sum %.9f, diff %.3g" % (S, score, total, score - total))
    assert abs(score - total) <= 1e-6 * max(1.0, abs(total))
    assert frames[1:] == [t for t, k, _ in picks if k != 0]


# 2. exhaustive ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S", K.EXHAUSTIVE)
def test_scores_are_the_brute_force_mass(T, S):
    ora, tn, pn, x, mass, _ = K.exhaustive_case(T, S)
    net = _jointnet(tn, pn, 3, ora)
    got = _decode(net, x, [T], 0, 64, S)
    assert {tuple(y) for y, _, _ in got} == set(mass) and len(got) == len(mass)
    assert all(abs(s - mass[tuple(y)]) <= 1e-5 for y, s, _ in got)
    assert abs(math.fsum(math.exp(s) for _, s, _ in got) - 1.0) <= 1e-5


# 3. bit invariance ------------------------------------------------------------------------------------------------------------------
def _ragged():
    """The ragged batch (T_b = T, 0, < T) at the level of the search: the encoder runs once, on lengths of at least 1 (a row
    without frames is never read).  -> net, enc (T,B,Oe), lens, device lens, the restatement's results"""
    c = K.RAGGED
    _, ora, tn, pn, x, want = K.ragged_case()
    net = _jointnet(tn, pn, c["V"], ora)
    enc = _encode(net, x, [max(n, 1) for n in c["lens"]])
    return net, enc, c["lens"], torch.tensor(c["lens"], dtype=torch.int32, device="cuda"), want


def test_same_bits_twice_alone_in_a_batch_and_across_batch_orders():
    c = K.RAGGED
    net, enc, lens, t_lens, want = _ragged()
    a = _ops_search(net, enc, t_lens, 0, c["W"], c["S"])
    assert _ops_search(net, enc, t_lens, 0, c["W"], c["S"]) == a              # python floats: == is bitwise
    for b, n in enumerate(lens):
        K.same_hyps(a[b], want[b].hyps)
        if n > 0:   # alone, and alone on exactly its own frames
            assert _ops_search(net, enc[:, b:b + 1].contiguous(), t_lens[b:b + 1], 0, c["W"], c["S"]) == [a[b]]
            assert _ops_search(net, enc[:n, b:b + 1].contiguous(), None, 0, c["W"], c["S"]) == [a[b]]
    perm = [2, 0, 3, 1]
    p = _ops_search(net, enc[:, perm].contiguous(), t_lens[perm].contiguous(), 0, c["W"], c["S"])
    assert [p[perm.index(b)] for b in range(len(lens))] == a
    assert a[1] == [([0], 0.0, [-1])]                                          # T_b = 0: [[blank]] with score 0


@pytest.mark.parametrize("idx", [5, 6], ids=["W64-S2", "config2-prednet"])
def test_same_bits_for_any_step_group(idx):
    """W = 64 advances up to 64 hypotheses a round, the config-2 prediction net 16: in groups of 8, of 3 (a ragged last group) and
    one by one, every list, frame and score bit is the same."""
    T, V, Hp, L, cell, W, S, O, min_logp, _ = c = K.SHAPE_CASES[idx]
    _, ora, tn, pn, x, want = K.shape_case(c)
    net = _jointnet(tn, pn, V, ora)
    enc = _encode(net, x, [T])
    full = _ops_search(net, enc, None, 0, W, S)
    K.same_hyps(full[0], want.hyps)
    for g in (3, 1):
        assert _ops_search(net, enc, None, 0, W, S, step_group=g) == full


# 4. edge rows -----------------------------------------------------------------------------------------------------------------------
def test_nan_beyond_the_lengths_is_never_read():
    c = K.RAGGED
    net, enc, lens, t_lens, want = _ragged()
    clean = _ops_search(net, enc, t_lens, 0, c["W"], c["S"])
    dirty = enc.clone()
    for b, n in enumerate(lens):
        dirty[n:, b] = float("nan")
    got = _ops_search(net, dirty, t_lens, 0, c["W"], c["S"])
    assert got == clean
    for b in range(len(lens)):
        K.same_hyps(got[b], want[b].hyps)
        assert all(math.isfinite(s) for _, s, _ in got[b])


def test_nan_filled_outputs_and_workspace_and_nothing_written_past_the_counts():
    """The C entry on buffers filled with 0xFF bytes (NaN as floats, -1 as ints): the same lists and score bits as the Python
    call, and every output entry past count[b] / lens[b, o] still holds the fill."""
    import ctypes as C

    from rnntransducer_amd import _lib, ops
    c = K.RAGGED
    net, enc, lens, t_lens, _ = _ragged()
    want = _ops_search(net, enc, t_lens, 0, c["W"], c["S"])
    T, B, Oe = enc.shape
    V, W, S = c["V"], c["W"], c["S"]
    dec = net.decoder
    d = _lib.BeamSyncDesc()
    keep = ops._fill_prednet(d, net.fc.weight, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight,
                             dec.out_proj.bias, 0, "test")
    A = torch.empty(T, B, V, device="cuda")
    ops.gemm(T * B, V, Oe, enc, keep[-1], A, b_sn=net.fc.weight.shape[1], b_sk=1, bias=net.fc.bias, flags=ops.GEMM_GELU_A)
    for b, n in enumerate(lens):
        A[n:, b] = float("nan")
    ML = 1 + S * T
    fill = lambda *shape, dt: torch.full((math.prod(shape) * dt.itemsize,), 255, dtype=torch.uint8, device="cuda").view(dt).reshape(*shape)
    tokens, frames = fill(B, W, ML, dt=torch.int32), fill(B, W, ML, dt=torch.int32)
    olens, count, scores = fill(B, W, dt=torch.int32), fill(B, dt=torch.int32), fill(B, W, dt=torch.float64)
    d.T, d.B, d.beam, d.max_symbols, d.step_group, d.token_min_logp = T, B, W, S, 0, -math.inf
    d.A, d.a_st, d.a_sb, d.t_lens = A.data_ptr(), B * V, V, t_lens.data_ptr()
    nws = _lib.lib().rnnt_hip_beam_sync_workspace_bytes(C.byref(d))
    ws = torch.full((nws + 256,), 255, dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = (ws.data_ptr() + 255) // 256 * 256, nws
    d.tokens, d.lens, d.scores, d.count = tokens.data_ptr(), olens.data_ptr(), scores.data_ptr(), count.data_ptr()
    tm = _lib.BeamTiming(frames.data_ptr(), None)
    _lib.check(_lib.lib().rnnt_hip_beam_sync_search(C.byref(d), None, C.byref(tm), ops._stream()), "rnnt_hip_beam_sync_search")
    torch.cuda.synchronize()
    tokens, frames, olens, count, scores = (t.cpu() for t in (tokens, frames, olens, count, scores))
    for b in range(B):
        n = int(count[b])
        got = [(tokens[b, o, :olens[b, o]].tolist(), float(scores[b, o]), frames[b, o, :olens[b, o]].tolist()) for o in range(n)]
        assert got == want[b]
        assert bool((olens[b, n:] == -1).all()) and bool((tokens[b, n:] == -1).all()) and bool((frames[b, n:] == -1).all())
        assert bool(torch.isnan(scores[b, n:]).all())
        for o in range(n):
            assert bool((tokens[b, o, olens[b, o]:] == -1).all()) and bool((frames[b, o, olens[b, o]:] == -1).all())


@pytest.mark.parametrize("c", K.BLANKS, ids=["first", "middle", "last"])
def test_blank_first_in_the_middle_and_last(c):
    blank, V, T, W, S = c
    _, ora, tn, pn, x, want = K.blank_case(*c)
    net = _jointnet(tn, pn, V, ora)
    got = _decode(net, x, [T], blank, W, S)
    K.same_hyps(got, want.hyps)
    assert all(y[0] == blank and blank not in y[1:] for y, _, _ in got)


# 5. candidates ----------------------------------------------------------------------------------------------------------------------
def test_fewer_candidates_than_the_beam_is_wide():
    """V = 2, W = 8: the first frames have 2 and 4 candidates; with token_min_logp above every log-probability only the blank."""
    ora, tn, pn = K.model(2, 4, 1, "lstm", 8, 2, scale=1.0)
    x = K.audio(3, 2)
    net = _jointnet(tn, pn, 2, ora)
    want = R.search(ora, x, [3], 0, 8, 1)[0]
    got = _decode(net, x, [3], 0, 8, 1)
    assert len(got) == 4 == len(want.hyps)                                   # [0], [0,1], [0,1,1], [0,1,1,1]
    by_y = {tuple(y): s for y, s, _ in want.hyps}
    assert all(K.close(s, by_y[tuple(y)]) for y, s, _ in got)
    only_blank = _decode(net, x, [3], 0, 8, 1, token_min_logp=1.0)
    assert [y for y, _, _ in only_blank] == [[0]]


def test_uniform_logits_tie_in_id_order():
    """All keys of a round are equal: the select chooses by its id passes alone.  V = 5: one populated bin in all but the last
    8-bit digit of the id; V = 300: the middle digit decides too (the first: test_gpu_ctc_beam.py, the same function)."""
    for V in (5, 300):
        ora, tn, pn = K.model(V, 4, 1, "lstm", 8, 3)
        with torch.no_grad():
            ora.fc.weight.zero_()
            ora.fc.bias.zero_()
        x = K.audio(2, 3)
        net = _jointnet(tn, pn, V, ora)
        got = _decode(net, x, [2], 0, 3, 1)
        want = R.search(ora, x, [2], 0, 3, 1)[0].hyps
        assert [(y, f) for y, _, f in got] == [(y, f) for y, _, f in want] == [([0], [-1]), ([0, 1], [-1, 0]), ([0, 2], [-1, 0])]
        assert all(K.close(s, w) for (_, s, _), (_, w, _) in zip(got, want))
        assert all(K.close(s, -2.0 * math.log(V)) for _, s, _ in got)


# 6. fusion --------------------------------------------------------------------------------------------------------------------------
def test_zero_automaton_gives_the_unfused_lists_and_score_bits():
    c = K.RAGGED
    net, enc, lens, t_lens, _ = _ragged()
    plain = _ops_search(net, enc, t_lens, 0, c["W"], c["S"])
    fused = _ops_search(net, enc, t_lens, 0, c["W"], c["S"], fusion=K.zero_fusion(c["V"]).to("cuda"))
    assert [[(y, s, f) for y, s, _, f in h] for h in fused] == plain
    assert all(fs == s for h in fused for _, s, fs, _ in h)


@pytest.mark.parametrize("kind", ["bigram", "hotwords"])
def test_fused_search_matches_the_fused_restatement(kind):
    """hotwords: a weight of 10, far above a typical -log p, the setting that makes recognize_beams' pop loop run away: here the
    search returns, and no hypothesis is longer than 1 + S T."""
    T, V, W, S = (K.FUSION[k] for k in ("T", "V", "W", "S"))
    _, ora, tn, pn, x, fusion, want = K.fusion_case(kind)
    net = _jointnet(tn, pn, V, ora)
    got = _decode(net, x, [T], 0, W, S, fusion=fusion.to("cuda"))
    K.same_hyps(got, want.hyps)
    for y, s, f, _ in got:
        total, final, _ = fusion.score(y)
        assert abs(f - (s + total + final)) <= 1e-12 * max(1.0, abs(f))
        assert len(y) <= 1 + S * T
    if kind == "hotwords":
        assert max(f - s for _, s, f, _ in got) > 10.0   # the bonus was earned: the automaton did steer the search


# 7. model level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidirectional", [False, True], ids=["uni", "bi"])
def test_model_level_calls_and_frames(bidirectional):
    from argparse import Namespace

    from rnntransducer_amd.model import RNNTransducer
    V, W, S, lens = (K.MODEL[k] for k in ("V", "W", "S", "lens"))
    _, ora, tn, pn, x, want = K.model_case(bidirectional)
    model = RNNTransducer(pn, tn, dict(num_classes=V), Namespace(blank_token_id=0)).cuda().eval()
    model.jointnet.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    net = model.jointnet
    full = model.recognize_beams_sync(x.cuda(), lens, beam_widths=W, max_symbols=S, return_scores=True, return_frames=True)
    assert full == net.recognize_beams_sync(x.cuda(), lens, 0, W, S, return_scores=True, return_frames=True)
    assert [[y for y, _, _ in h] for h in full] == net.recognize_beams_sync(x.cuda(), lens, 0, W, S)
    assert [[(y, s) for y, _, s in h] for h in full] == net.recognize_beams_sync(x.cuda(), lens, 0, W, S, return_scores=True)
    assert [[(y, f) for y, f, _ in h] for h in full] == net.recognize_beams_sync(x.cuda(), lens, 0, W, S, return_frames=True)
    single = net.recognize_beams_sync(x[1:, :4].contiguous().cuda(), [4], 0, W, S)
    assert single == [y for y, _, _ in full[1]] and isinstance(single[0][0], int)    # the list itself for one utterance
    for b, n in enumerate(lens):
        K.same_hyps(_entries(full[b]), want[b].hyps)
        for y, frames, score in full[b]:
            assert y[0] == 0 and frames[0] == -1 and len(frames) == len(y) <= 1 + S * n
            assert all(0 <= f < n for f in frames[1:]) and frames[1:] == sorted(frames[1:])   # non-decreasing along a hypothesis
            assert all(frames[1:].count(f) <= S for f in set(frames[1:]))                      # at most S equal
