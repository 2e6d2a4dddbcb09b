"""The restatement of the frame-synchronous beam search (tests/beam_sync_restatement.py) pinned to quantities that come from no
search, the cases of tests/beam_sync_cases.py (every one finds its seed), and the refusals of the new entries: the ValueErrors
of ops.beam_search_sync / recognize_beams_sync and the C entry's host-side checks, on a machine that may have no GPU."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import beam_sync_cases as K
from tests import beam_sync_restatement as R


# 0. every listed case finds its seed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.SHAPE_CASES, ids=K.case_id)
def test_every_shape_case_finds_a_seed_with_a_margin(c):
    found = K.shape_case(c)
    assert found is not None, "no seed in %r keeps a boundary margin of %g: change this shape's logit scale" % (K.SEEDS, K.MARGIN)
    res = found[5]
    T, V, W, S = c[0], c[1], c[5], c[6]
    assert res.boundary_margin >= K.MARGIN and 1 <= len(res.hyps) <= W
    assert all(len(y) <= 1 + S * T and y[0] == 0 for y, _, _ in res.hyps)
    assert len({tuple(y) for y, _, _ in res.hyps}) == len(res.hyps)


def test_the_other_cases_find_their_seeds():
    assert all(K.greedy_case(*g) is not None for g in K.GREEDY)
    assert all(K.fusion_case(kind) is not None for kind in ("bigram", "hotwords"))
    assert all(K.blank_case(*c) is not None for c in K.BLANKS) and K.ragged_case() is not None
    assert K.model_case(False) is not None and K.model_case(True) is not None
    assert [r.hyps for r in K.ragged_case()[5]][1] == [([0], 0.0, [-1])]   # no frames: [[blank]] with score 0


# 1. exhaustive mass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S", K.EXHAUSTIVE)
def test_scores_are_the_brute_force_mass_when_the_beam_holds_everything(T, S):
    _, _, _, _, mass, res = K.exhaustive_case(T, S)
    assert {tuple(y) for y, _, _ in res.hyps} == set(mass) and len(res.hyps) == len(mass) <= 64
    for y, s, _ in res.hyps:
        assert abs(s - mass[tuple(y)]) <= 1e-12, (y, s, mass[tuple(y)])
    assert abs(math.fsum(math.exp(s) for _, s, _ in res.hyps) - 1.0) <= 1e-12
    assert res.merges > 0   # a score is a mass: several paths met in one node


# 2. W = 1 against greedy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", K.GREEDY)
def test_width_one_is_greedy_search(g):
    S = g[0]
    _, ora, _, _, x, (tokens, picks), res = K.greedy_case(*g)
    (y, score, _), = res.hyps
    assert y == tokens
    assert abs(score - math.fsum(lp for _, _, lp in picks)) <= 1e-12 * max(1.0, abs(score))
    # the oracle's own greedy search (fp32) drops a token that repeats the last appended one: the same tokens under that rule
    want = ora.recognize_greedy(x, [x.size(1)], 0, max_iters=S)[0]
    assert R.drop_repeats(y[1:], 0) == want


# 3. merging -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_a_sequence_that_reaches_d_twice_in_a_frame_carries_both_paths_once():
    ora, _, _ = K.model(3, 4, 1, "lstm", 8, 7, scale=1.0)
    net = R.double_net(ora)
    enc = net.encoder(K.audio(2, 7).double(), [2])[0]
    res = R.search_one(net, enc, 0, 64, 1)
    steps = R._Steps(net)
    lp = lambda t, y: torch.log_softmax(net.fc(F.gelu(torch.cat((enc[t], steps(y)[0])), approximate="tanh")), dim=0).tolist()
    # [0, 1] after frame 1: by blank from [0, 1], and as the extension of [0] by 1
    by_blank = lp(0, (0,))[1] + lp(1, (0, 1))[0]
    by_parent = lp(0, (0,))[0] + lp(1, (0,))[1]
    hits = [s for y, s, _ in res.hyps if y == [0, 1]]
    assert len(hits) == 1 and abs(hits[0] - R.logaddexp(by_blank, by_parent)) <= 1e-12
    assert res.merges >= 1


# 4. ties ----------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_uniform_joint_logits_tie_in_id_order():
    ora, _, _ = K.model(5, 4, 1, "lstm", 8, 3)
    with torch.no_grad():
        ora.fc.weight.zero_()
        ora.fc.bias.zero_()
    net = R.double_net(ora)
    enc = net.encoder(K.audio(2, 3).double(), [2])[0]
    res = R.search_one(net, enc, 0, 3, 1)
    # frame 0: ids 0 (blank), 1, 2 of the root; frame 1: the three members' blanks and tokens all tie: ids 0, 1, 2 of member 0
    assert [y for y, _, _ in res.hyps] == [[0], [0, 1], [0, 2]]
    assert all(abs(s - 2 * math.log(1 / 5)) <= 1e-12 or y == [0, 1] for y, s, _ in res.hyps)
    assert res.boundary_margin == 0.0


# 5. pruning -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_token_min_logp_never_prunes_the_blank():
    ora, _, _ = K.model(6, 4, 1, "lstm", 8, 5)
    net = R.double_net(ora)
    enc = net.encoder(K.audio(4, 5).double(), [4])[0]
    res = R.search_one(net, enc, 0, 4, 2, token_min_logp=1.0)   # no log-probability reaches 1: only blanks are candidates
    (y, s, frames), = res.hyps
    steps = R._Steps(net)
    want = sum(float(torch.log_softmax(net.fc(F.gelu(torch.cat((enc[t], steps((0,))[0])), approximate="tanh")), dim=0)[0]) for t in range(4))
    assert y == [0] and frames == [-1] and abs(s - want) <= 1e-12
    loose = R.search_one(net, enc, 0, 4, 2, token_min_logp=-math.inf)
    assert len(loose.hyps) == 4


# 6. fusion --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bigram", "hotwords"])
def test_fused_score_is_score_plus_total_plus_final(kind):
    _, ora, _, _, x, fusion, res = K.fusion_case(kind)
    plain = R.search(ora, x, [x.size(1)], 0, K.FUSION["W"], K.FUSION["S"])[0]
    for y, s, f, frames in res.hyps:
        total, final, _ = fusion.score(y)
        assert abs(f - (s + total + final)) <= 1e-9 * max(1.0, abs(f))
        assert len(y) <= 1 + K.FUSION["S"] * K.FUSION["T"] and len(frames) == len(y)
    assert [h[0] for h in res.hyps] != [h[0] for h in plain.hyps]
    zero = R.search(ora, x, [x.size(1)], 0, K.FUSION["W"], K.FUSION["S"], fusion=K.zero_fusion(K.FUSION["V"]))[0]
    assert [(y, s) for y, s, _, _ in zero.hyps] == [(y, s) for y, s, _ in plain.hyps] and all(f == s for _, s, f, _ in zero.hyps)


# 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _op_args(V=6, Hp=8, O=8, Oe=8, T=3, B=2):
    enc = torch.zeros(T, B, Oe)
    fc_w, fc_b, emb = torch.zeros(V, Oe + O), torch.zeros(V), torch.zeros(V, Hp)
    rnn = [torch.zeros(4 * Hp, Hp), torch.zeros(4 * Hp, Hp), torch.zeros(4 * Hp), torch.zeros(4 * Hp)]
    return [enc, fc_w, fc_b, emb, rnn, 0, torch.zeros(O, Hp), torch.zeros(O)]


def test_beam_search_sync_refuses_bad_arguments_before_anything_runs():
    from rnntransducer_amd import ops
    call = lambda *a, args=None, **kw: ops.beam_search_sync(*(args or _op_args()), *a, **kw)
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="beam width"):
            call(0, bad)
    for bad in (0, 5, True, 1.5):
        with pytest.raises(ValueError, match="max_symbols"):
            call(0, 4, bad)
    for bad in (math.nan, math.inf, "x"):
        with pytest.raises(ValueError, match="token_min_logp"):
            call(0, 4, 1, token_min_logp=bad)
    for bad in (-1, 6):
        with pytest.raises(ValueError, match="blank"):
            call(bad, 4)
    with pytest.raises(ValueError, match="step_group"):
        call(0, 4, step_group=-1)
    with pytest.raises(ValueError, match="V = 1"):
        call(0, 4, args=_op_args(V=1))
    with pytest.raises(ValueError, match="2\\^24"):
        call(0, 64, args=[torch.zeros(1, 1, 8), torch.zeros((1 << 18) + 1, 16), torch.zeros((1 << 18) + 1),
                          torch.zeros((1 << 18) + 1, 8)] + _op_args()[4:])
    with pytest.raises(ValueError, match="do not fit"):
        call(0, 4, args=_op_args(Oe=12)[:1] + _op_args()[1:])
    with pytest.raises(ValueError, match="t_lens"):
        call(0, 4, 1, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="fusion"):
        call(0, 4, fusion=object())
    with pytest.raises(ValueError, match="over 7 tokens"):
        call(0, 4, fusion=K.zero_fusion(7))


def test_recognize_beams_sync_refuses_bad_arguments_before_anything_runs():
    from rnntransducer_amd.networks import JointNet
    tn, pn = K.params(6, 8, 1, "lstm", 8)
    net = JointNet(dict(tn), dict(pn), 6)
    x = torch.zeros(1, 3, 6)
    with pytest.raises(ValueError, match="eval"):
        net.train().recognize_beams_sync(x, [3], 0)
    net.eval()
    for kw, what in ((dict(beam_widths=65), "beam width"), (dict(max_symbols=5), "max_symbols"),
                     (dict(token_min_logp=math.nan), "token_min_logp"), (dict(fusion=K.zero_fusion(5)), "over 5 tokens")):
        with pytest.raises(ValueError, match=what):
            net.recognize_beams_sync(x, [3], 0, **kw)
    with pytest.raises(ValueError, match="blank"):
        net.recognize_beams_sync(x, [3], 6)
    from rnntransducer_amd.model import RNNTransducer
    assert callable(getattr(RNNTransducer, "recognize_beams_sync"))


P, Q = 0x10000, 0x20000   # 256-byte aligned stand-ins for device pointers, never dereferenced


def _desc(**kw):
    from rnntransducer_amd import _lib
    d = _lib.BeamSyncDesc()
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank = 3, 2, 10, 8, 8, 1, 0, 0
    d.beam, d.max_symbols, d.step_group, d.token_min_logp = 4, 2, 0, -math.inf
    d.A, d.a_st, d.a_sb, d.t_lens = P, 20, 10, Q
    d.emb, d.w_o, d.b_o, d.w_d, d.ld_d = P, P, P, P, 16
    d.w_ih[0], d.w_hh[0], d.b_ih[0], d.b_hh[0] = P, P, P, P
    d.tokens, d.lens, d.scores, d.count = Q, Q, Q, Q
    for k, v in kw.items():
        setattr(d, k, v)
    d.workspace, d.workspace_bytes = 0x100000, _lib.lib().rnnt_hip_beam_sync_workspace_bytes(C.byref(d))
    return d


def test_the_c_entry_validates_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    err = lambda: L.rnnt_hip_last_error()
    run = lambda d, f=None, tm=None: L.rnnt_hip_beam_sync_search(C.byref(d), f, tm, None)
    a256 = lambda n: (n + 255) // 256 * 256
    d = _desc()
    # the workspace: the layer-0 table, W V keys, 5 (1 + W S T) node ints and (S+2) W slots of h | c | Cv per utterance
    slot = (1 * 8 * 2 + 10 + 3) // 4 * 4
    assert d.workspace_bytes == a256(10 * 4 * 8 * 4) + a256(2 * 4 * 10 * 8) + a256(2 * 5 * (1 + 4 * 2 * 3) * 4) + a256(2 * 16 * slot * 4)
    assert L.rnnt_hip_beam_sync_step_group(C.byref(d)) == 8
    assert L.rnnt_hip_beam_sync_step_group(C.byref(_desc(step_group=3))) == 3
    assert L.rnnt_hip_beam_sync_workspace_bytes(None) == 0 and L.rnnt_hip_beam_sync_search(None, None, None, None) == -1
    for kw, what in ((dict(beam=0), b"beam width"), (dict(beam=65), b"beam width"), (dict(max_symbols=0), b"max_symbols"),
                     (dict(max_symbols=5), b"max_symbols"), (dict(V=1), b"V = 1"), (dict(blank=10), b"blank"), (dict(blank=-1), b"blank"),
                     (dict(V=1 << 23, beam=3), b"2^24"), (dict(token_min_logp=math.nan), b"token_min_logp"),
                     (dict(token_min_logp=math.inf), b"token_min_logp"), (dict(step_group=-1), b"step_group"),
                     (dict(Hp=6), b"multiples of 4"), (dict(L=9), b"layers"), (dict(cell=7), b"cell"), (dict(T=0), b"positive"),
                     (dict(T=1 << 24, beam=64, max_symbols=4), b"node index"), (dict(Hp=4096, L=8), b"LDS")):
        bad = _desc(**kw)
        assert bad.workspace_bytes == 0 and what in err(), (kw, err())
        bad.workspace_bytes = 1 << 30
        assert run(bad) == -1 and what in err(), (kw, err())
    for kw, what in ((dict(A=None), b"null"), (dict(tokens=None), b"null"), (dict(lens=None), b"null"), (dict(scores=None), b"null"),
                     (dict(count=None), b"null"), (dict(emb=None), b"null"), (dict(w_o=None), b"null"), (dict(a_st=0), b"strides"),
                     (dict(ld_d=18), b"16-byte aligned"), (dict(w_d=P + 4), b"16-byte aligned")):
        assert run(_desc(**kw)) == -1 and what in err(), (kw, err())
    bad = _desc()
    bad.w_hh[0] = None
    assert run(bad) == -1 and b"null weight" in err()
    # workspace: short, misaligned, missing
    bad = _desc()
    bad.workspace_bytes -= 1
    assert run(bad) == -1 and b"workspace too small" in err()
    bad = _desc()
    bad.workspace = 0x100000 + 64
    assert run(bad) == -1 and b"256-byte aligned" in err()
    bad = _desc()
    bad.workspace = None
    assert run(bad) == -1 and b"workspace" in err()
    # the fusion tables: check_fusion's rules; a timing struct must hold its output
    fus = lambda **kw: C.byref(_lib.BeamFusion(**{**dict(next=P, arc=P, final=P, n_states=4, fused_scores=Q), **kw}))
    d = _desc()
    for kw, what in ((dict(next=None), b"null fusion table"), (dict(arc=None), b"null fusion table"), (dict(final=None), b"null fusion table"),
                     (dict(n_states=0), b"n_states"), (dict(n_states=(1 << 27) // 10 + 1), b"2^27"), (dict(fused_scores=None), b"fused_scores")):
        assert run(d, fus(**kw)) == -1 and what in err(), (kw, err())
    assert run(d, None, C.byref(_lib.BeamTiming(None, None))) == -1 and b"frames" in err()
