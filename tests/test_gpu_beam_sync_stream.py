"""The streaming frame-synchronous beam search on the GPU (csrc/beam_sync_stream.hip).  Its definition is the
offline entry: after every chunk a stream's n-best must be BITWISE what rnnt_hip_beam_sync_search returns on the rows of A fed
so far (lists, fp64 score bits, frames), for any chunking.  Beside that: the float64 restatement through the model-level call
(lists and frames exact, scores 1e-5 relative, the tolerances of tests/test_gpu_beam_sync.py; margins asserted on the CPU by
tests/test_beam_sync_stream_oracle.py), the tree collection on a model that prunes prefixes and reaches them again, fusion, row
isolation, the two caps and memory discipline.  Shapes are the smallest at which each mechanism can go wrong."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import beam_sync_cases as K
from tests import beam_sync_stream_cases as SK

pytestmark = pytest.mark.gpu

V, HP = SK.V, SK.HP
LENS = [24, 9, 1]


def _jointnet(tn, pn, ora):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), pn["embedding_size"])
    net.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    return net.cuda().eval()


@functools.lru_cache(maxsize=None)
def _net(cell="lstm", L=1, seed=0):
    ora, tn, pn = K.model(V, HP, L, cell, 8, seed)
    return _jointnet(tn, pn, ora)


def _joint_rows(T, B, seed=0, scale=3.0):
    """One (T, B, V) A tensor: what the encoder half of the joint would hand the search."""
    return (scale * torch.randn(T, B, V, generator=torch.Generator().manual_seed(seed))).cuda()


def _offline(net, A, t_lens, W, S, fusion=None, step_group=0):
    """rnnt_hip_beam_sync_search on A (T,B,V) with its descriptor built as tests/test_gpu_beam_sync.py builds it.
    -> per stream [(y, score[, fused], frames)]"""
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
    d.T, d.B, d.beam, d.max_symbols, d.step_group, d.token_min_logp = T, B, W, S, step_group, -math.inf
    d.A, d.a_st, d.a_sb, d.t_lens = A.data_ptr(), A.stride(0), A.stride(1), lens_dev.data_ptr()
    nws = _lib.lib().rnnt_hip_beam_sync_workspace_bytes(C.byref(d))
    ws = torch.zeros(nws + 256, dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = (ws.data_ptr() + 255) // 256 * 256, nws
    d.tokens, d.lens, d.scores, d.count = tokens.data_ptr(), olens.data_ptr(), scores.data_ptr(), count.data_ptr()
    tm = _lib.BeamTiming(frames.data_ptr(), None)
    fs = ops.fusion_struct(fusion, fused) if fusion is not None else None
    _lib.check(_lib.lib().rnnt_hip_beam_sync_search(C.byref(d), C.byref(fs) if fs is not None else None, C.byref(tm), ops._stream()),
               "rnnt_hip_beam_sync_search")
    torch.cuda.synchronize()
    tokens, frames, olens, count, scores, fused = (t.cpu() for t in (tokens, frames, olens, count, scores, fused))
    out = []
    for b in range(B):
        out.append([(tokens[b, o, :olens[b, o]].tolist(), float(scores[b, o])) + ((float(fused[b, o]),) if fusion is not None else ())
                    + (frames[b, o, :olens[b, o]].tolist(),) for o in range(int(count[b]))])
    return out


def _state(net, B, W, S, **kw):
    from rnntransducer_amd.streaming import BeamSyncStreamState
    return BeamSyncStreamState(net, B, 0, W, S, **kw)


def _results(state):
    """the state's n-best lists as the offline helper writes them: (y, score[, fused], frames)"""
    return [[(e[0], *e[2:], e[1]) for e in hyps] for hyps in state.results(True, True)]


def _feed(state, A, lens, n0, k):
    """rows [n0, n0 + k) of A to the streams that still have frames there"""
    part = [max(0, min(n, n0 + k) - n0) for n in lens]
    if k > 0 and max(part) > 0:
        state.run_chunk(A[n0:n0 + k], torch.tensor(part, dtype=torch.int32, device="cuda"), part)
    return part


def _roomy(W, S, T):
    """A max_nodes no stream of T frames can outgrow: the offline tree's bound.  (A random joint keeps W diverging hypotheses
    and their descendants alive; the tests of the cap itself choose their model on the CPU.)"""
    return max(1 + W * S * T, 1 + 4 * W * S)


def _schedules(T):
    return [[1] * T, [7] * (T // 7) + ([T % 7] if T % 7 else []), [T]] + SK.random_schedules(T, 2)


# 1. bitwise against the offline entry on the same A ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,L,W,S", [("lstm", 1, 4, 1), ("lstm", 1, 4, 2), ("lstm", 1, 8, 3), ("lstm", 1, 1, 1), ("gru", 1, 4, 2),
                                         ("lstm", 2, 4, 1)], ids=["W4-S1", "W4-S2", "W8-S3", "W1", "gru", "2-layer"])
def test_every_chunking_gives_the_offline_entrys_bits(cell, L, W, S):
    net, T, B = _net(cell, L), max(LENS), len(LENS)
    A = _joint_rows(T, B)
    offline = functools.lru_cache(maxsize=None)(lambda n: _offline(net, A, [min(m, n) for m in LENS], W, S))
    assert offline(0) == [[([0], 0.0, [-1])]] * B
    state = _state(net, B, W, S, max_nodes=_roomy(W, S, T))
    for sched in _schedules(T):
        state.reset(range(B))                                   # after the first schedule: a reset row is a fresh row
        assert _results(state) == offline(0)                    # no frames: [[blank]], score 0
        n = 0
        for k in sched:
            _feed(state, A, LENS, n, k)
            n += k
            assert _results(state) == offline(n), (sched, n)    # python floats: == is bitwise; every shared count, transitively
        for b in range(B):
            h = state.header(b)
            assert h["frames"] == LENS[b] == int(state.frames_seen[b]) and h["status"] == 0 and h["n_beam"] == len(offline(T)[b])
            sp, spf = state.stable_prefix(b, return_frames=True)
            assert h["committed"] == len(sp) and all(e[0][:len(sp)] == sp and e[-1][:len(sp)] == spf for e in offline(T)[b])
            assert len(sp) == len(SK.SR.common_prefix([e[0] for e in offline(T)[b]]))


# 2. the re-reach case ----------------------------------------------------------------------------------------------------------------
def test_pruned_prefixes_reached_again_keep_their_first_frame():
    """The blank-biased model at the least max_nodes (33 against an offline tree of 126 nodes and 1 + W S T = 385 slots).  Fed
    frame by frame the tree is collected after every frame; fed as one chunk it has to be collected INSIDE the chunk, whenever a
    frame would not find W S free slots.  Either way the frames are the offline entry's: those of each prefix's FIRST creation."""
    from rnntransducer_amd import ops
    c = SK.BIASED
    T, W, S = c["T"], c["W"], c["S"]
    ora, tn, pn, x, _, _ = SK.biased_case()
    tr = SK.biased_trace()
    net = _jointnet(tn, pn, ora)
    with torch.no_grad():
        enc = net.encoder.forward_time_major(x.cuda(), torch.tensor([T], dtype=torch.int32, device="cuda")).contiguous()
    A = torch.empty(T, 1, V, device="cuda")
    ops.gemm(T, V, enc.shape[2], enc, net.fc.weight, A, b_sn=net.fc.weight.shape[1], b_sk=1, bias=net.fc.bias, flags=ops.GEMM_GELU_A)
    want = _offline(net, A, [T], W, S)
    K.same_hyps(want[0], tr.hyps)                               # the offline entry against the float64 trace: frames exact
    for y in tr.final_rereached:                                # the frames that a paths-only collection would get wrong
        e = next(e for e in want[0] if tuple(e[0][:len(y)]) == y)
        assert e[-1][len(y) - 1] == tr.rereached[y][0] < tr.rereached[y][1]
    for sched in ([1] * T, [T], [5] * 9 + [3]):
        state = _state(net, 1, W, S, max_nodes=SK.BIASED_MAX_NODES)
        n = 0
        for k in sched:
            _feed(state, A, [T], n, k)
            n += k
        assert _results(state) == want, sched
        h = state.header(0)
        print(sched[:2], h)
        assert h["peak_nodes"] <= SK.BIASED_MAX_NODES and h["nodes"] == tr.keep[-1]
        assert h["collections"] >= len(sched)
        if len(sched) == T:
            assert h["collections_in_chunk"] == 0               # a collected tree that a frame does not fit in would be the cap
        elif len(sched) == 1:
            assert h["collections_in_chunk"] >= 1 and h["collections"] == h["collections_in_chunk"] + 1


# 3. against the float64 restatement, through the model -------------------------------------------------------------------------------
def test_model_level_call_matches_the_restatement_after_every_frame():
    c = SK.CONFIDENT
    T, W, S = c["T"], c["W"], c["S"]
    ora, tn, pn, x, per_n = SK.confident_case()
    assert min(m for *_, m in per_n) >= K.MARGIN                # asserted on the CPU too; never skipped
    net = _jointnet(tn, pn, ora)
    state = net.init_beam_sync_stream(1, 0, W, S)
    xc = x.cuda()
    assert net.recognize_beams_sync_stream(xc[:, :0], [0], state) == [[[0]]]
    for n in range(1, T + 1):
        got = net.recognize_beams_sync_stream(xc[:, n - 1:n], [1], state, return_scores=True, return_frames=True)
        hyps, sp, spf, _ = per_n[n]
        K.same_hyps([(y, s, f) for y, f, s in got[0]], hyps)
        assert state.stable_prefix(0, return_frames=True) == (sp, spf), n
        assert state.stable_prefix(0) == sp
    assert len(state.stable_prefix(0)) >= 5 and state.header(0)["committed"] == len(sp)
    assert net.recognize_beams_sync_stream(xc[:, :1], [0], state) == [[y for y, _, _ in got[0]]]   # 0 frames: the previous list


def test_model_wrappers_and_guards():
    from argparse import Namespace

    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.model import RNNTransducer
    ora, tn, pn = K.model(V, HP, 1, "lstm", 8, 0)
    model = RNNTransducer(pn, tn, dict(num_classes=V), Namespace(blank_token_id=0)).cuda().eval()
    model.jointnet.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    net, x = model.jointnet, K.audio(6, 0, B=2).cuda()
    state, twin = model.init_beam_sync_stream(2, beam_widths=4, max_symbols=2), net.init_beam_sync_stream(2, 0, 4, 2)
    a = model.recognize_beams_sync_stream(x[:, :4], [4, 2], state, return_scores=True, return_frames=True)
    assert a == net.recognize_beams_sync_stream(x[:, :4], [4, 2], twin, return_scores=True, return_frames=True)
    assert [[y for y, _, _ in h] for h in a] == state.results(False) and [[(y, f) for y, f, _ in h] for h in a] == state.results(False, True)
    assert state.workspace_bytes > state.bytes_per_stream * 2 > 0 and state.workspace_row(1).numel() == state.bytes_per_stream
    before = state.workspace.clone()
    other = _jointnet(tn, pn, ora)
    for call in (lambda: other.recognize_beams_sync_stream(x, [1, 1], state),                       # another model's state
                 lambda: net.recognize_beams_sync_stream(x[:1], [1], state),                        # another B
                 lambda: net.recognize_beams_sync_stream(x, [1, 7], state),                         # a length past the chunk
                 lambda: net.recognize_beams_sync_stream(x.double(), [1, 1], state),
                 lambda: net.recognize_beams_sync_stream(x, [1, 1], net.init_beam_stream(2, 0, 4)),  # the other search's state
                 lambda: net.train().recognize_beams_sync_stream(x, [1, 1], state)):
        with pytest.raises(ValueError):
            call()
        net.eval()
    ws = state.workspace
    state.workspace = ws.clone()[1:]                                                                # a replaced workspace
    with pytest.raises(ValueError, match="workspace"):
        net.recognize_beams_sync_stream(x, [1, 1], state)
    state.workspace = ws
    assert torch.equal(state.workspace, before) and int(state.frames_seen.sum()) == 6
    state.failed[1] = True                                                                          # a failed stream fed again
    with pytest.raises(RnntHipError, match="reset"):
        net.recognize_beams_sync_stream(x, [0, 1], state)
    assert torch.equal(state.workspace, before)
    net.recognize_beams_sync_stream(x, [1, 0], state)                                               # ... but not if it gets no frames


# 4. fusion ---------------------------------------------------------------------------------------------------------------------------
def test_zero_automaton_gives_the_unfused_bits_and_hotwords_the_offline_fused_bits():
    from rnntransducer_amd import TokenFusion
    net, T, B, W, S = _net(), max(LENS), len(LENS), 4, 2
    A = _joint_rows(T, B)
    plain = _state(net, B, W, S, max_nodes=_roomy(W, S, T))
    zero = _state(net, B, W, S, max_nodes=_roomy(W, S, T), fusion=K.zero_fusion(V).to("cuda"))
    first = _offline(net, A, LENS, W, S)[0][0][0]
    hot = TokenFusion.from_hotwords([first[1:3], [first[2], first[1]]], K.HOTWORD_WEIGHT, V, 0).to("cuda")
    fused = _state(net, B, W, S, max_nodes=_roomy(W, S, T), fusion=hot)
    assert _results(fused)[0] == [([0], 0.0, float(hot.final[0]), [-1])]
    n = 0
    for k in [3, 0, 1, 7, 5, 8]:
        for st in (plain, zero, fused):
            _feed(st, A, LENS, n, k)
        n += k
        lim = [min(m, n) for m in LENS]
        assert [[(y, s, f) for y, s, _, f in h] for h in _results(zero)] == _results(plain) == _offline(net, A, lim, W, S)
        assert all(fs == s for h in _results(zero) for _, s, fs, _ in h)
        assert _results(fused) == _offline(net, A, lim, W, S, fusion=hot)
    assert n == T and max(e[2] - e[1] for e in _results(fused)[0]) > 0.0      # a bonus was earned


# 5. row isolation and reset ----------------------------------------------------------------------------------------------------------
def test_rows_are_isolated_and_runs_repeat_bit_for_bit():
    net, T, W, S = _net(), 12, 4, 2
    B = 300                                                     # more streams than the device has compute units
    A = _joint_rows(T, B, seed=1)
    lens = [(7 * b) % (T + 1) for b in range(B)]
    lens[5] = T
    runs = []
    for _ in range(2):
        state = _state(net, B, W, S, max_nodes=_roomy(W, S, T))
        start = state.workspace.clone()
        _feed(state, A, lens, 0, 5)
        mid = state.workspace.clone()
        off = state._ws_off + state._table_bytes
        for b in range(B):                                      # a row without frames in the chunk is bitwise as it was
            lo = off + b * state.bytes_per_stream
            assert (lens[b] > 0) != torch.equal(mid[lo:lo + state.bytes_per_stream], start[lo:lo + state.bytes_per_stream])
        _feed(state, A, lens, 5, 7)
        runs.append((state.workspace.clone(), _results(state)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    want = _offline(net, A[:, :8].contiguous(), lens[:8], W, S)
    assert runs[0][1][:8] == want
    alone = _state(net, 1, W, S, max_nodes=_roomy(W, S, T))                  # the same bits alone as among 300
    one = A[:, 5:6].contiguous()
    _feed(alone, one, [T], 0, 5)
    _feed(alone, one, [T], 5, 7)
    assert _results(alone)[0] == runs[0][1][5]
    assert torch.equal(alone.workspace_row(0), state.workspace_row(5))
    # reset: row 5 starts over and reproduces a fresh state's bytes and results; row 6, not reset, does not move
    keep6 = state.workspace_row(6).clone()
    state.reset([5])
    fresh = _state(net, 1, W, S, max_nodes=_roomy(W, S, T))
    assert torch.equal(state.workspace_row(6), keep6) and int(state.frames_seen[5]) == 0 and state.stable_prefix(5) == [0]
    only5 = [T if b == 5 else 0 for b in range(B)]
    _feed(state, A, only5, 0, T)
    _feed(fresh, one, [T], 0, T)
    assert _results(state)[5] == _results(fresh)[0] == runs[0][1][5]
    assert torch.equal(state.workspace_row(6), keep6)
    assert torch.equal(state.workspace_row(5)[:32], fresh.workspace_row(0)[:32])   # the header words


# 6. caps -----------------------------------------------------------------------------------------------------------------------------
def test_max_nodes_fails_the_same_stream_at_the_same_frame_under_any_chunking():
    from rnntransducer_amd._lib import RnntHipError
    c = SK.CAPS
    T, W, S, cap = c["T"], c["W"], c["S"], c["max_nodes"]
    ora, tn, pn, x, tr = SK.caps_case()
    t_fail = SK.caps_fail_frame()
    net = _jointnet(tn, pn, ora)
    xs = torch.cat([x, x], 0).cuda()
    lens = [T, c["short"]]                                      # stream 1 hears the start of the same audio and stays small
    roomy = net.init_beam_sync_stream(2, 0, W, S)
    want = net.recognize_beams_sync_stream(xs, lens, roomy, return_scores=True, return_frames=True)
    assert roomy.header(0)["peak_nodes"] == tr.tree[-1] > cap   # uncollected within the one chunk: the offline tree
    K.same_hyps([(y, s, f) for y, f, s in want[0]], tr.hyps)
    for step in (1, 7):
        state = net.init_beam_sync_stream(2, 0, W, S, max_nodes=cap)
        with pytest.raises(RnntHipError, match="max_nodes") as err:
            for n0 in range(0, T, step):
                got = net.recognize_beams_sync_stream(xs[:, n0:n0 + step], [max(0, min(m, n0 + step) - n0) for m in lens], state,
                                                      return_scores=True, return_frames=True)
        assert "stream 0 " in str(err.value) and n0 <= t_fail < n0 + step
        h = state.header(0)
        assert (h["status"], h["frames"]) == (4, t_fail) and state.failed == [True, False]
        assert state.results(True, True)[1] == want[1]          # the other stream was updated, with the bits it has anyway
        with pytest.raises(RnntHipError, match="reset"):
            net.recognize_beams_sync_stream(xs[:, :1], [1, 0], state)
        state.reset([0])                                        # recovers
        fresh = net.init_beam_sync_stream(2, 0, W, S, max_nodes=cap)
        a = net.recognize_beams_sync_stream(xs[:, :5], [5, 0], state, return_scores=True, return_frames=True)
        assert a[0] == net.recognize_beams_sync_stream(xs[:, :5], [5, 0], fresh, return_scores=True, return_frames=True)[0]
        assert a[1] == want[1]


def test_max_len_fails_where_the_long_tail_would_be_returned():
    """max_len bounds the uncommitted tail of a RETURNED sequence: fed frame by frame, the caps model's stream fails at the
    first fed count at which the restatement's longest tail passes max_len."""
    from rnntransducer_amd._lib import RnntHipError
    c = SK.CAPS
    ora, tn, pn, x, _ = SK.caps_case()
    tails, _ = SK.caps_tails()
    max_len = 10
    n_fail = next(n for n, t in enumerate(tails) if t > max_len)
    net, xc = _jointnet(tn, pn, ora), x.cuda()
    state = net.init_beam_sync_stream(1, 0, c["W"], c["S"], max_len=max_len)
    with pytest.raises(RnntHipError, match="max_len") as err:
        for n in range(c["T"]):
            net.recognize_beams_sync_stream(xc[:, n:n + 1], [1], state)
            assert max(len(y) for y in state.results(False)[0]) - len(state.stable_prefix(0)) == tails[n + 1] <= max_len
    assert n + 1 == n_fail and "stream 0 " in str(err.value)
    h = state.header(0)
    assert (h["status"], h["frames"]) == (5, n_fail) and state.failed == [True]
    state.reset([0])
    fresh = net.init_beam_sync_stream(1, 0, c["W"], c["S"])
    assert net.recognize_beams_sync_stream(xc[:, :3], [3], state, return_scores=True) == \
        net.recognize_beams_sync_stream(xc[:, :3], [3], fresh, return_scores=True)


# 7. memory discipline ----------------------------------------------------------------------------------------------------------------
def test_nan_fills_change_nothing_and_nothing_is_written_past_the_counts():
    net, T, B, W, S = _net(), max(LENS), len(LENS), 4, 2
    A = _joint_rows(T, B)
    clean = _state(net, B, W, S, max_nodes=_roomy(W, S, T))
    dirty = _state(net, B, W, S, max_nodes=_roomy(W, S, T))
    dirty.workspace.fill_(255)                                  # NaN as floats, -1 as ints: only what a reset writes is defined
    dirty._reset(list(range(B)), build_table=True)
    Ad = A.clone()
    for b, m in enumerate(LENS):
        Ad[m:, b] = float("nan")
    n = 0
    for k in (7, 7, 10):
        for buf in (dirty._tokens, dirty._frames, dirty._lens, dirty._scores, dirty._small):
            buf.view(torch.uint8).fill_(255)
        dirty._commit = dirty._commit_frames = None
        part = [max(0, min(m, n + k) - n) for m in LENS]
        ncom = dirty.caps["max_nodes"] + S * k
        dirty._commit = torch.full((B, ncom), -1, dtype=torch.int32, device="cuda")
        dirty._commit_frames = torch.full((B, ncom), -1, dtype=torch.int32, device="cuda")
        _feed(clean, A, LENS, n, k)
        _feed(dirty, Ad, LENS, n, k)
        n += k
        assert _results(dirty) == _results(clean) == _offline(net, A, [min(m, n) for m in LENS], W, S)
        count, status, ncommit = dirty._small.cpu().tolist()
        tokens, frames, olens, scores = (t.cpu() for t in (dirty._tokens, dirty._frames, dirty._lens, dirty._scores))
        commit, cframes = dirty._commit.cpu(), dirty._commit_frames.cpu()
        for b in range(B):
            if part[b] == 0:                                    # not fed: count -1, nothing else written
                assert count[b] == -1 and status[b] == 0 and ncommit[b] == 0
                assert bool((olens[b] == -1).all()) and bool((tokens[b] == -1).all()) and bool((commit[b] == -1).all())
                continue
            m = count[b]
            assert 1 <= m <= W and status[b] == 0
            assert bool((olens[b, m:] == -1).all()) and bool((tokens[b, m:] == -1).all()) and bool((frames[b, m:] == -1).all())
            assert bool(torch.isnan(scores[b, m:]).all())
            for o in range(m):
                assert bool((tokens[b, o, olens[b, o]:] == -1).all()) and bool((frames[b, o, olens[b, o]:] == -1).all())
            assert bool((commit[b, ncommit[b]:] == -1).all()) and bool((cframes[b, ncommit[b]:] == -1).all())
            assert bool((commit[b, :ncommit[b]] >= 0).all())


# 8. step group -----------------------------------------------------------------------------------------------------------------------
def test_same_bits_for_any_step_group():
    net, T, W, S = _net(), 12, 8, 3
    A = _joint_rows(T, 2, seed=3)
    want = _offline(net, A, [T, 5], W, S)
    rows = []
    for g in (8, 3, 1):
        state = _state(net, 2, W, S, max_nodes=_roomy(W, S, T), step_group=g)
        for n in range(0, T, 4):
            _feed(state, A, [T, 5], n, 4)
        assert _results(state) == want
        rows.append(state.workspace.clone())
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
