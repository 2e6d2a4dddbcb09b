"""Internal-LM subtraction on the GPU (the ILM instances of beam_sync_kernel, csrc/beam_sync_shared.hpp) against
its float64 restatement (tests/ilm_restatement.py), the fused instances it extends (bitwise where the term is zero), itself
(bitwise: alone / in a batch, any step group, offline / streamed in any chunking, sparse / dense automaton) and the host scorer
JointNet.ilm_score.  Every case compared with the restatement keeps a boundary margin >= 1e-4 there, asserted on the CPU by
tests/test_ilm_oracle.py; the tolerances are tests/beam_sync_cases.py's same_hyps: token lists and frames exact, scores to 1e-5
relative, output order only across pairs at least 1e-4 apart."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import beam_sync_cases as K
from tests import ilm_cases as IK
from tests import ilm_restatement as IR

pytestmark = pytest.mark.gpu
MU = IK.MU


def _jointnet(tn, pn, V, ora):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    return net.cuda().eval()


def _entries(hyps):
    """(y, frames, score, fused) of the model-level call -> the restatement's (y, score, fused, frames)"""
    return [(e[0], *e[2:], e[1]) for e in hyps]


def _decode(net, x, lens, blank, W, S, **kw):
    out = net.recognize_beams_sync(x.cuda(), lens, blank, W, S, return_scores=True, return_frames=True, **kw)
    return _entries(out) if len(lens) == 1 else [_entries(h) for h in out]


def _ops_search(net, enc_tm, t_lens, blank, W, S, **kw):
    """ops.beam_search_sync on given encoder outputs (T,B,Oe): entries (y, score, fused, frames)"""
    from rnntransducer_amd import ops
    dec = net.decoder
    return ops.beam_search_sync(enc_tm, net.fc.weight, net.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                                dec.out_proj.weight, dec.out_proj.bias, blank, W, S, t_lens, frames=True, **kw)


def _encode(net, x, lens):
    from rnntransducer_amd.networks.encoder import lengths_to_device
    with torch.no_grad():
        return net.encoder.forward_time_major(x.cuda(), lengths_to_device(lens, "cuda")).contiguous()


# 1. against the restatement, a bigram automaton plus ILM; 8. the host scorer on the first shape ---------------------------------------
@pytest.mark.parametrize("c", IK.SHAPE_CASES, ids=K.case_id)
def test_shape_cases_match_the_restatement(c):
    T, V, Hp, L, cell, W, S, O, min_logp, _ = c
    _, ora, tn, pn, x, fusion, want = IK.shape_case(c)
    net = _jointnet(tn, pn, V, ora)
    got = _decode(net, x, [T], 0, W, S, token_min_logp=min_logp, fusion=fusion.to("cuda"), ilm_weight=MU)
    K.same_hyps(got, want.hyps)
    assert all(len(y) <= 1 + S * T for y, *_ in got)
    assert any(f != s for _, s, f, _ in got)


def test_ilm_score_explains_the_fused_scores():
    """fused_score - score - (the automaton's total + final) = -mu * ilm_score(y), and ilm_score is the float64 teacher-forced
    sum, both to 1e-5 relative (fp32 log-softmax terms, about 1e-6 off each, a handful per sequence)."""
    c = IK.SHAPE_CASES[0]
    T, V, Hp, L, cell, W, S, O, min_logp, _ = c
    _, ora, tn, pn, x, fusion, _ = IK.shape_case(c)
    net = _jointnet(tn, pn, V, ora)
    net64 = IR.double_net(ora)
    got = _decode(net, x, [T], 0, W, S, fusion=fusion.to("cuda"), ilm_weight=MU)
    U = max(len(y) for y, *_ in got) - 1
    targets = torch.tensor([y[1:] + [0] * (U - len(y) + 1) for y, *_ in got], dtype=torch.int64, device="cuda").reshape(len(got), U)
    lens = [len(y) - 1 for y, *_ in got]
    ilm = net.ilm_score(targets, lens, 0)
    assert ilm.dtype == torch.float64 and tuple(ilm.shape) == (len(got),)
    assert max(lens) >= 1
    for (y, s, f, _), got_ilm in zip(got, ilm.tolist()):
        total, final, _ = fusion.score(y)
        want_ilm = IR.ilm_score_fp64(net64, y, 0)
        print(y, "ilm_score %.9f fp64 %.9f; fused - score - automaton %.9f" % (got_ilm, want_ilm, f - s - (total + final)))
        assert K.close(got_ilm, want_ilm)
        assert K.close(f - s - (total + final), -MU * got_ilm)
        assert got_ilm <= 0.0
    with pytest.raises(ValueError):
        net.ilm_score(torch.zeros(1, 2, dtype=torch.int64, device="cuda"), [2], 0)        # the blank among the counted tokens


# 2. the blank first, in the middle and last ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.BLANKS, ids=["first", "middle", "last"])
def test_the_excluded_index_moves_with_the_blank(c):
    blank, V, T, W, S = c
    _, ora, tn, pn, x, fusion, want = IK.blank_case(*c)
    net = _jointnet(tn, pn, V, ora)
    got = _decode(net, x, [T], blank, W, S, fusion=fusion.to("cuda"), ilm_weight=MU)
    K.same_hyps(got, want.hyps)
    assert all(y[0] == blank and blank not in y[1:] for y, *_ in got)


# 3. V = 2: one non-blank token, ilm = 0 exactly ------------------------------------------------------------------------------------------
def test_one_token_vocabulary_gives_the_fused_instances_bits():
    T, V, Hp, L, cell, W, S = IK.V2
    ora, tn, pn = K.model(V, Hp, L, cell, 8, 2, scale=1.0)
    x = K.audio(T, 2)
    net = _jointnet(tn, pn, V, ora)
    fusion = K.bigram_fusion(V, 0, 2).to("cuda")
    off = _decode(net, x, [T], 0, W, S, fusion=fusion)
    on = _decode(net, x, [T], 0, W, S, fusion=fusion, ilm_weight=MU)
    assert on == off and len(on) >= 2                                          # python floats: == is bitwise
    assert any(f != s for _, s, f, _ in on)                                    # (the automaton's part is there in both)


# 4. subtraction alone ----------------------------------------------------------------------------------------------------------------
def test_no_fusion_is_the_zero_automaton_bit_for_bit_and_matches_the_restatement():
    T, V, Hp, L, cell, W, S, O, min_logp, _ = IK.NO_FUSION
    _, ora, tn, pn, x, want = IK.no_fusion_case()
    net = _jointnet(tn, pn, V, ora)
    alone = _decode(net, x, [T], 0, W, S, ilm_weight=MU)
    assert alone == _decode(net, x, [T], 0, W, S, fusion=K.zero_fusion(V).to("cuda"), ilm_weight=MU)
    K.same_hyps(alone, want.hyps)
    assert all(f >= s for _, s, f, _ in alone) and any(f > s for _, s, f, _ in alone)   # the term is a bonus


# 5. bit invariance -------------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_alone_in_a_batch_and_for_any_step_group():
    c = K.RAGGED
    _, ora, tn, pn, x, fusion, want = IK.ragged_case()
    net = _jointnet(tn, pn, c["V"], ora)
    lens = c["lens"]
    enc = _encode(net, x, [max(n, 1) for n in lens])
    t_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(fusion=fusion.to("cuda"), ilm_weight=MU)
    a = _ops_search(net, enc, t_lens, 0, c["W"], c["S"], **kw)
    assert _ops_search(net, enc, t_lens, 0, c["W"], c["S"], **kw) == a
    assert _ops_search(net, enc, t_lens, 0, c["W"], c["S"], step_group=1, **kw) == a
    for b, n in enumerate(lens):
        K.same_hyps(a[b], want[b].hyps)
        if n > 0:
            assert _ops_search(net, enc[:, b:b + 1].contiguous(), t_lens[b:b + 1], 0, c["W"], c["S"], **kw) == [a[b]]
    assert a[1] == [([0], 0.0, float(fusion.final[0]), [-1])]                  # T_b = 0: [[blank]], score 0, final[0]


# 6. streaming ------------------------------------------------------------------------------------------------------------------------
def _offline_ilm(net, A, t_lens, W, S, fusion, mu, ngram=False):
    """rnnt_hip_beam_sync_search_ilm on A (T,B,V) -> per stream [(y, score, fused, frames)]"""
    from rnntransducer_amd import _lib, ops
    T, B, _ = A.shape
    dec = net.decoder
    d = _lib.BeamSyncDesc()
    keep = ops._fill_prednet(d, net.fc.weight, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight,
                             dec.out_proj.bias, 0, "test")
    ML = 1 + S * T
    tokens = torch.zeros(B, W, ML, dtype=torch.int32, device="cuda")
    frames = torch.zeros_like(tokens)
    olens, count = torch.zeros(B, W, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    scores, fused = torch.zeros(B, W, dtype=torch.float64, device="cuda"), torch.zeros(B, W, dtype=torch.float64, device="cuda")
    lens_dev = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    d.T, d.B, d.beam, d.max_symbols, d.step_group, d.token_min_logp = T, B, W, S, 0, -math.inf
    d.A, d.a_st, d.a_sb, d.t_lens = A.data_ptr(), A.stride(0), A.stride(1), lens_dev.data_ptr()
    nws = _lib.lib().rnnt_hip_beam_sync_ilm_workspace_bytes(C.byref(d))
    assert nws > _lib.lib().rnnt_hip_beam_sync_workspace_bytes(C.byref(d)) > 0
    ws = torch.zeros(nws + 256, dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = (ws.data_ptr() + 255) // 256 * 256, nws
    d.tokens, d.lens, d.scores, d.count = tokens.data_ptr(), olens.data_ptr(), scores.data_ptr(), count.data_ptr()
    tm = _lib.BeamTiming(frames.data_ptr(), None)
    fs = ops.fusion_struct(fusion, fused)
    ilm = _lib.BeamIlm(net.fc.bias.data_ptr(), mu)
    sparse = isinstance(fs, _lib.BeamNgram)
    _lib.check(_lib.lib().rnnt_hip_beam_sync_search_ilm(C.byref(d), None if sparse else C.byref(fs), C.byref(fs) if sparse else None,
                                                        C.byref(ilm), C.byref(tm), ops._stream()), "rnnt_hip_beam_sync_search_ilm")
    torch.cuda.synchronize()
    tokens, frames, olens, count, scores, fused = (t.cpu() for t in (tokens, frames, olens, count, scores, fused))
    return [[(tokens[b, o, :olens[b, o]].tolist(), float(scores[b, o]), float(fused[b, o]), frames[b, o, :olens[b, o]].tolist())
             for o in range(int(count[b]))] for b in range(B)]


def _results(state):
    """the state's n-best lists as the offline helper writes them: (y, score, fused, frames)"""
    return [[(e[0], *e[2:], e[1]) for e in hyps] for hyps in state.results(True, True)]


def _feed(state, A, lens, n0, k):
    part = [max(0, min(n, n0 + k) - n0) for n in lens]
    if k > 0 and max(part) > 0:
        state.run_chunk(A[n0:n0 + k], torch.tensor(part, dtype=torch.int32, device="cuda"), part)


def test_every_chunking_gives_the_offline_ilm_calls_bits():
    """Chunks of 1, 3 and T frames: after every chunk lists, fp64 scores, fused scores and absolute frames are bitwise the
    offline ILM call's for the frames fed so far.  The second stream hears the frames in reverse and stops after 9.  Between
    the schedules the rows are reset: a reset stream starts clean (the carried pairs are rewritten before they are read)."""
    from rnntransducer_amd import ops
    from rnntransducer_amd.streaming import BeamSyncStreamState
    c = IK.STREAM
    T, W, S, V = c["T"], c["W"], c["S"], c["V"]
    _, ora, tn, pn, x, fusion, want = IK.stream_case()
    net = _jointnet(tn, pn, V, ora)
    fusion = fusion.to("cuda")
    enc = _encode(net, x, [T])
    A1 = torch.empty(T, 1, V, device="cuda")
    ops.gemm(T, V, enc.shape[2], enc, net.fc.weight, A1, b_sn=net.fc.weight.shape[1], b_sk=1, bias=net.fc.bias, flags=ops.GEMM_GELU_A)
    A = torch.cat([A1, A1.flip(0)], dim=1).contiguous()
    lens = [T, 9]
    offline = functools.lru_cache(maxsize=None)(lambda n: _offline_ilm(net, A, [min(m, n) for m in lens], W, S, fusion, MU))
    K.same_hyps(offline(T)[0], want.hyps)                                      # the offline entry against the restatement
    roomy = max(1 + W * S * T, 1 + 4 * W * S)
    state = BeamSyncStreamState(net, 2, 0, W, S, fusion=fusion, ilm_weight=MU, max_nodes=roomy)
    plain = BeamSyncStreamState(net, 2, 0, W, S, fusion=fusion, max_nodes=roomy)
    assert state.ilm_weight == MU and state.workspace_bytes > plain.workspace_bytes
    assert state.workspace_row(1).numel() == state.bytes_per_stream
    for step in (1, 3, T):
        state.reset(range(2))
        assert _results(state) == offline(0) == [[([0], 0.0, float(fusion.final[0]), [-1])]] * 2
        for n0 in range(0, T, step):
            _feed(state, A, lens, n0, step)
            assert _results(state) == offline(min(n0 + step, T)), (step, n0)   # python floats: == is bitwise
        assert [state.header(b)["frames"] for b in range(2)] == lens
    # one row reset: it starts clean and reproduces its bits, the other row does not move
    keep1 = state.workspace_row(1).clone()
    state.reset([0])
    _feed(state, A, [T, 0], 0, T)
    assert _results(state) == offline(T) and torch.equal(state.workspace_row(1), keep1)
    # the least max_nodes: the collection runs inside the one chunk and moves nodes, never state slots or their pairs
    small = BeamSyncStreamState(net, 1, 0, W, S, fusion=fusion, ilm_weight=MU, max_nodes=IK.STREAM_MAX_NODES)
    _feed(small, A1, [T], 0, T)
    assert _results(small) == [offline(T)[0]]
    h = small.header(0)
    assert h["collections_in_chunk"] >= 1 and h["peak_nodes"] <= IK.STREAM_MAX_NODES and h["nodes"] == want.keep[-1]
    small.reset([0])
    for n0 in range(0, T, 5):
        _feed(small, A1, [T], n0, 5)
    assert _results(small) == [offline(T)[0]]


def test_model_level_stream_matches_the_restatement():
    """Through the streaming encoder (whose rows are chunk-invariant, not the offline encoder's bits): against the restatement."""
    c = IK.STREAM
    T, W, S, V = c["T"], c["W"], c["S"], c["V"]
    _, ora, tn, pn, x, fusion, want = IK.stream_case()
    net = _jointnet(tn, pn, V, ora)
    state = net.init_beam_sync_stream(1, 0, W, S, fusion=fusion.to("cuda"), ilm_weight=MU)
    xc = x.cuda()
    for n0 in range(0, T, 7):
        got = net.recognize_beams_sync_stream(xc[:, n0:n0 + 7], [min(7, T - n0)], state, return_scores=True, return_frames=True)
    K.same_hyps(_entries(got[0]), want.hyps)                                   # (y, frames, score, fused_score) per entry
    alone = net.init_beam_sync_stream(1, 0, W, S, ilm_weight=MU)               # subtraction alone: entries carry fused_score
    out = net.recognize_beams_sync_stream(xc, [T], alone, return_scores=True)
    assert all(len(e) == 3 and e[2] >= e[1] for e in out[0])


# 7. a backoff n-gram model plus ILM ------------------------------------------------------------------------------------------------------
def test_sparse_automaton_is_its_dense_expansion_bit_for_bit():
    from tests import ngram_cases as NK
    W, S, thr = IK.NGRAM
    _, ora, tn, pn, x, lm, want = IK.ngram_case()
    net = _jointnet(tn, pn, NK.V, ora)
    sparse = _decode(net, x, [NK.T], 0, W, S, token_min_logp=thr, fusion=lm.to("cuda"), ilm_weight=MU)
    dense = _decode(net, x, [NK.T], 0, W, S, token_min_logp=thr, fusion=lm.to_dense().to("cuda"), ilm_weight=MU)
    assert sparse == dense
    K.same_hyps(sparse, want.hyps)
    assert sparse != _decode(net, x, [NK.T], 0, W, S, token_min_logp=thr, fusion=lm.to("cuda"))


# 9. guards, before any launch ------------------------------------------------------------------------------------------------------------
def test_python_guards():
    T, V, Hp, L, cell, W, S, O, min_logp, _ = IK.NO_FUSION
    ora, tn, pn = K.model(V, Hp, L, cell, O, 0)
    net = _jointnet(tn, pn, V, ora)
    x = K.audio(T, 0).cuda()
    for bad in (-0.1, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="ilm_weight"):
            net.recognize_beams_sync(x, [T], 0, W, S, ilm_weight=bad)
        with pytest.raises(ValueError, match="ilm_weight"):
            net.init_beam_sync_stream(1, 0, W, S, ilm_weight=bad)
        with pytest.raises(ValueError, match="ilm_weight"):
            _ops_search(net, _encode(net, x, [T]), None, 0, W, S, ilm_weight=bad)
    for call in (lambda: net.recognize_beams(x, [T], 0, 4, ilm_weight=MU),
                 lambda: net.init_beam_stream(1, 0, 4, ilm_weight=MU),
                 lambda: net.recognize_ctc_beams(x, [T], 0, 4, ilm_weight=MU)):
        with pytest.raises(ValueError, match="recognize_beams_sync.*init_beam_sync_stream"):
            call()
    assert net.recognize_beams_sync(x, [T], 0, W, S, ilm_weight=0.0) == net.recognize_beams_sync(x, [T], 0, W, S)
    with pytest.raises(ValueError):
        net.train().ilm_score(torch.ones(1, 2, dtype=torch.int64, device="cuda"), [2], 0)
    net.eval()


def test_c_entries_refuse_bad_arguments_and_launch_nothing():
    from rnntransducer_amd import _lib, ops
    from rnntransducer_amd.streaming import BeamSyncStreamState
    T, V, Hp, L, cell, W, S, O, min_logp, _ = IK.NO_FUSION
    ora, tn, pn = K.model(V, Hp, L, cell, O, 0)
    net = _jointnet(tn, pn, V, ora)
    Lb = _lib.lib()
    dec = net.decoder
    A = torch.randn(T, 1, V, generator=torch.Generator().manual_seed(0)).cuda()
    # offline
    d = _lib.BeamSyncDesc()
    keep = ops._fill_prednet(d, net.fc.weight, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight,
                             dec.out_proj.bias, 0, "test")
    ML = 1 + S * T
    fill = lambda *shape, dt: torch.full((math.prod(shape) * dt.itemsize,), 255, dtype=torch.uint8, device="cuda").view(dt).reshape(*shape)
    tokens, olens, count = fill(1, W, ML, dt=torch.int32), fill(1, W, dt=torch.int32), fill(1, dt=torch.int32)
    scores, fused = fill(1, W, dt=torch.float64), fill(1, W, dt=torch.float64)
    d.T, d.B, d.beam, d.max_symbols, d.step_group, d.token_min_logp = T, 1, W, S, 0, -math.inf
    d.A, d.a_st, d.a_sb, d.t_lens = A.data_ptr(), V, V, None
    nws = Lb.rnnt_hip_beam_sync_ilm_workspace_bytes(C.byref(d))
    small = Lb.rnnt_hip_beam_sync_workspace_bytes(C.byref(d))
    assert nws >= small + 8 * (S + 2) * W
    ws = fill(nws + 256, dt=torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    d.workspace, d.workspace_bytes = base, nws
    d.tokens, d.lens, d.scores, d.count = tokens.data_ptr(), olens.data_ptr(), scores.data_ptr(), count.data_ptr()
    zero = K.zero_fusion(V).to("cuda")
    lm_t = __import__("tests.ngram_cases", fromlist=["x"]).random_lm(V, 0).to("cuda")
    fs, ng = ops.fusion_struct(zero, fused), ops.fusion_struct(lm_t, fused)
    good = _lib.BeamIlm(net.fc.bias.data_ptr(), MU)
    call = lambda f, g, i: Lb.rnnt_hip_beam_sync_search_ilm(C.byref(d), f, g, i, None, ops._stream())
    cases = [(C.byref(fs), None, None, b"null ilm"),
             (C.byref(fs), None, C.byref(_lib.BeamIlm(None, MU)), b"bias"),
             (C.byref(fs), None, C.byref(_lib.BeamIlm(net.fc.bias.data_ptr(), 0.0)), b"weight"),
             (C.byref(fs), None, C.byref(_lib.BeamIlm(net.fc.bias.data_ptr(), float("nan"))), b"weight"),
             (C.byref(fs), None, C.byref(_lib.BeamIlm(net.fc.bias.data_ptr(), float("inf"))), b"weight"),
             (C.byref(fs), C.byref(ng), C.byref(good), b"both"),
             (None, None, C.byref(good), b"neither")]
    for f, g, i, msg in cases:
        assert call(f, g, i) == -1 and msg in Lb.rnnt_hip_last_error(), (msg, Lb.rnnt_hip_last_error())
    d.workspace_bytes = small                                                  # the fused entry's size: too small here
    assert call(C.byref(fs), None, C.byref(good)) == -1 and b"workspace" in Lb.rnnt_hip_last_error()
    d.workspace, d.workspace_bytes = base + 64, nws
    assert call(C.byref(fs), None, C.byref(good)) == -1 and b"aligned" in Lb.rnnt_hip_last_error()
    d.workspace = base
    torch.cuda.synchronize()
    for t in (tokens, olens, count, ws):                                       # nothing was launched: every byte is the fill
        assert bool((t.view(torch.uint8) == 255).all())
    assert call(C.byref(fs), None, C.byref(good)) == 0                         # the same descriptor, good arguments: it runs
    torch.cuda.synchronize()
    assert int(count[0]) >= 1
    # streaming
    state = BeamSyncStreamState(net, 1, 0, W, S, fusion=zero, ilm_weight=MU)
    plain = BeamSyncStreamState(net, 1, 0, W, S, fusion=zero)
    sd, keep2 = state._descriptor()
    commit = torch.empty(1, state.caps["max_nodes"] + S * T, dtype=torch.int32, device="cuda")
    lens_dev = torch.tensor([T], dtype=torch.int32, device="cuda")
    sd.T, sd.A, sd.a_st, sd.a_sb, sd.lens, sd.commit = T, A.data_ptr(), V, V, lens_dev.data_ptr(), commit.data_ptr()
    sfs = ops.fusion_struct(zero, state._fused)
    before = state.workspace.clone()
    scall = lambda f, g, i: Lb.rnnt_hip_beam_sync_stream_chunk_ilm(C.byref(sd), f, g, i, None, ops._stream())
    for f, g, i, msg in [(C.byref(sfs), None, None, b"null ilm"), (C.byref(sfs), None, C.byref(_lib.BeamIlm(None, MU)), b"bias"),
                         (C.byref(sfs), None, C.byref(_lib.BeamIlm(net.fc.bias.data_ptr(), 0.0)), b"weight"),
                         (C.byref(sfs), C.byref(ng), C.byref(good), b"both"), (None, None, C.byref(good), b"neither")]:
        assert scall(f, g, i) == -1 and msg in Lb.rnnt_hip_last_error(), msg
    assert Lb.rnnt_hip_beam_sync_stream_ilm_workspace_bytes(C.byref(sd)) == state.workspace_bytes > plain.workspace_bytes
    sd.workspace_bytes = plain.workspace_bytes                                 # a stream opened without ILM: too small
    assert scall(C.byref(sfs), None, C.byref(good)) == -1 and b"workspace" in Lb.rnnt_hip_last_error()
    rows = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert Lb.rnnt_hip_beam_sync_stream_reset_ilm(C.byref(sd), rows.data_ptr(), 1, 0, ops._stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(state.workspace, before)
