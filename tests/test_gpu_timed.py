"""Recognition with token timestamps and confidences on the GPU (the *_timed entries of include/rnnt_hip.h: the four search
kernels with their extra output pointers set) vs the float64 restatements of tests/timed_restatement.py, the dense joint, the
untimed calls (bitwise) and re-chunking (bitwise).

logp tolerance: two fp32 quantities enter a logp, the chosen logit and the lse, each built from A / C as accurate as the
encoder outputs that tests/test_gpu_stream.py::test_encoder_stream_vs_float64 holds to 2e-5 of float64; twice that is allowed.
Each case prints its largest |logp - float64| before asserting; DESIGN.md §15 keeps what was recorded."""
import pytest
import torch

from tests import timed_restatement as tr
from tests.test_oracle_beam import fixture_nbest
from tests.test_stream_oracle import chunk_batches, random_schedules, uniform_schedule

pytestmark = pytest.mark.gpu
LOGP_ATOL = 2 * 2e-5   # twice tests/test_gpu_stream.py's FWD_ATOL


def _jointnet(tn, pn, V, state_dict):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in state_dict.items()})
    return net.cuda().eval()


def _greedy(name):
    ora, tn, pn, audios, lens, max_iters, ref = tr.greedy_case(name)
    return _jointnet(tn, pn, pn["embedding_size"], ora.state_dict()), audios, lens, max_iters, ref


def _check_timed(got, ref, b, n=None):
    """One utterance's TimedTokens against the restatement's first n entries; -> largest |logp - float64|."""
    n = len(ref.tokens[b]) if n is None else n
    assert got.tokens.dtype == torch.int64 and got.frames.dtype == torch.int32 and got.logp.dtype == torch.float32
    assert got.tokens.dim() == got.frames.dim() == got.logp.dim() == 1
    assert got.tokens.tolist() == ref.tokens[b][:n] and got.frames.tolist() == ref.frames[b][:n]
    err = max([abs(x - y) for x, y in zip(got.logp.tolist(), ref.logp[b][:n])] or [0.0])
    assert err <= LOGP_ATOL, (b, err)
    return err


# 1. greedy vs the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tr.GREEDY_CASES))
def test_greedy_timed_vs_restatement(name):
    net, audios, lens, max_iters, ref = _greedy(name)
    x = audios.float().cuda()
    got = net.recognize_greedy(x, lens, 0, max_iters, return_timing=True)
    assert len(got) == len(lens) and sum(len(t) for t in ref.tokens) > 0
    worst = max(_check_timed(got[b], ref, b) for b in range(len(lens)))
    print(f"{name}: largest |logp - float64| = {worst:.3e} over {sum(map(len, ref.tokens))} tokens")
    assert got[lens.index(0)].tokens.numel() == 0                         # the utterance without frames
    # the untimed call: the same tokens, bitwise
    plain = net.recognize_greedy(x, lens, 0, max_iters)
    assert all(torch.equal(p, g.tokens) for p, g in zip(plain, got))
    # truncation: entries past max_out are dropped exactly as tokens are
    b = max(range(len(lens)), key=lambda i: len(ref.tokens[i]))
    cut = len(ref.tokens[b]) - 1
    assert cut >= 1
    short = net.recognize_greedy(x, lens, 0, max_iters, return_timing=True, max_out=cut)
    for i in range(len(lens)):
        _check_timed(short[i], ref, i, min(cut, len(ref.tokens[i])))
        assert torch.equal(short[i].logp, got[i].logp[:cut])
    # a single utterance: one tuple, not a list
    one = net.recognize_greedy(x[b:b + 1, :lens[b]].contiguous(), [lens[b]], 0, max_iters, return_timing=True)
    assert one.tokens.tolist() == ref.tokens[b] and one.frames.tolist() == ref.frames[b]


# 2. the dense joint: an independent check ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tr.GREEDY_CASES))
def test_greedy_timed_vs_dense_joint(name):
    net, audios, lens, max_iters, ref = _greedy(name)
    ok = [b for b in range(len(lens)) if tr.qualifies(ref, b)]
    assert 2 * len(ok) >= len(lens)
    x = audios.float().cuda()
    got = net.recognize_greedy(x, lens, 0, max_iters, return_timing=True)
    U = max(len(ref.tokens[b]) for b in ok)
    texts = torch.zeros(len(ok), U, dtype=torch.int64)
    for i, b in enumerate(ok):
        toks = got[b].tokens.tolist()
        texts[i, :len(toks)] = torch.tensor([0] + toks[:-1])             # [blank] + tokens[:-1]
    with torch.no_grad():
        logits = net(x[ok].contiguous(), [lens[b] for b in ok], texts.cuda(), [len(ref.tokens[b]) for b in ok])   # (B,T,U,V)
    lsm = torch.log_softmax(logits.double(), dim=-1).cpu()
    for i, b in enumerate(ok):
        for j, (k, t, lp) in enumerate(zip(got[b].tokens.tolist(), got[b].frames.tolist(), got[b].logp.tolist())):
            assert int(lsm[i, t, j].argmax()) == k
            assert abs(float(lsm[i, t, j, k]) - lp) <= LOGP_ATOL, (b, j, float(lsm[i, t, j, k]), lp)


# 3. streaming greedy --------------------------------------------------------------------------------------------------
def _stream_timed(net, audios, lens, schedule, max_iters, state=None):
    state = state or net.init_stream(len(lens), 0)
    out = [[] for _ in lens]
    for x, ns in chunk_batches(audios.float(), lens, schedule):
        for b, t in enumerate(net.recognize_greedy_stream(x.cuda(), ns, state, max_iters, return_timing=True)):
            out[b].append(t)
    cat = lambda parts, i, dt: torch.cat([p[i] for p in parts]) if parts else torch.empty(0, dtype=dt, device="cuda")
    from rnntransducer_amd.ops import TimedTokens
    return [TimedTokens(cat(o, 0, torch.int64), cat(o, 1, torch.int32), cat(o, 2, torch.float32)) for o in out], state


def _ragged_schedule(lens):
    return [(2, [0] * len(lens))] + random_schedules(lens, 4, max_chunk=6)   # zero-length chunks included


@pytest.mark.parametrize("name", list(tr.GREEDY_CASES))
def test_stream_greedy_timed_any_chunking_same_bits(name):
    net, audios, lens, max_iters, ref = _greedy(name)
    base, st0 = _stream_timed(net, audios, lens, uniform_schedule(lens, max(lens)), max_iters)
    for b in range(len(lens)):
        _check_timed(base[b], ref, b)                                      # absolute frames = the offline frames
    for sched in (uniform_schedule(lens, 1), _ragged_schedule(lens)):
        got, st = _stream_timed(net, audios, lens, sched, max_iters)
        for g, w in zip(got, base):
            assert torch.equal(g.tokens, w.tokens) and torch.equal(g.frames, w.frames) and torch.equal(g.logp, w.logp)
        assert torch.equal(st.frames_seen, st0.frames_seen)
    # the offline search of this library: equal tokens and frames (margins >= 1e-3, tests/test_timed_oracle.py)
    off = net.recognize_greedy(audios.float().cuda(), lens, 0, max_iters, return_timing=True)
    for g, w in zip(off, base):
        assert torch.equal(g.tokens, w.tokens) and torch.equal(g.frames, w.frames)
    # the untimed streaming call: the same tokens
    plain_state = net.init_stream(len(lens), 0)
    plain = net.recognize_greedy_stream(audios.float().cuda(), lens, plain_state, max_iters)
    assert all(torch.equal(p, w.tokens) for p, w in zip(plain, base))


def test_stream_greedy_timed_reset_and_zero_frame_streams():
    net, audios, lens, max_iters, ref = _greedy("lstm_h32_l1")
    x = audios.float().cuda()
    state = net.init_stream(len(lens), 0)
    half = [n // 2 for n in lens]
    net.recognize_greedy_stream(x, half, state, max_iters, return_timing=True)
    state.reset([0])
    assert state.frames_seen.tolist() == [0] + half[1:]
    # row 0 starts again at frame 0; row 1 goes on where it was; a stream without frames is untouched and returns nothing
    rest = [lens[0], lens[1] - half[1], 0, 0]
    chunk = torch.zeros_like(x)
    chunk[0], chunk[1, :rest[1]] = x[0], x[1, half[1]:lens[1]]
    before = [t.clone() for t in (state.pred_h, state.pred_joint, state.last_token, state.frames_seen)]
    got = net.recognize_greedy_stream(chunk, rest, state, max_iters, return_timing=True)
    _check_timed(got[0], ref, 0)
    k = sum(f < half[1] for f in ref.frames[1])
    assert got[1].tokens.tolist() == ref.tokens[1][k:] and got[1].frames.tolist() == ref.frames[1][k:]
    assert got[2].tokens.numel() == got[2].frames.numel() == got[2].logp.numel() == 0
    for a, c in zip(before, (state.pred_h, state.pred_joint, state.last_token, state.frames_seen)):
        sel = (lambda t: t[:, 3]) if a.dim() == 3 else (lambda t: t[3])
        assert torch.equal(sel(a), sel(c))
    empty = net.recognize_greedy_stream(x, [0] * len(lens), state, max_iters, return_timing=True)
    assert all(e.tokens.numel() == 0 and e.frames.dtype == torch.int32 and e.logp.dtype == torch.float32 for e in empty)


# 4. beam, offline -----------------------------------------------------------------------------------------------------
def _beam(name):
    ora, tn, pn, audios, lens, beam, improved, ref = tr.beam_case(name)
    return _jointnet(tn, pn, tr.BEAM_V, ora.state_dict()), ora, audios, lens, beam, improved, ref


@pytest.mark.parametrize("name", list(tr.BEAM_CASES))
def test_beam_frames_vs_restatement(name):
    net, _, audios, lens, beam, improved, ref = _beam(name)
    x = audios.float().cuda()
    want = [ref.nbest(b) for b in range(len(lens))]
    got = net.recognize_beams(x, lens, 0, beam, improved, return_frames=True, return_scores=True)
    assert [[(y, f) for y, f, _ in h] for h in got] == [[(y, f) for y, f, _ in h] for h in want]
    for gh, wh in zip(got, want):
        for (_, _, s), (_, _, w) in zip(gh, wh):
            assert abs(s - w) <= 1e-4 * max(1.0, abs(w)), (s, w)          # fp32 log-probs against float64, as tests/test_gpu_beam.py
    # the untimed call: the same lists and the same score bits
    plain = net.recognize_beams(x, lens, 0, beam, improved, return_scores=True)
    assert plain == [[(y, s) for y, _, s in h] for h in got]
    assert net.recognize_beams(x, lens, 0, beam, improved, return_frames=True) == [[(y, f) for y, f, _ in h] for h in got]
    assert net.recognize_beams(x[:1], [0], 0, beam, improved, return_frames=True) == [([0], [-1])]   # no frames: [blank] at -1


# 5. beam, streaming ---------------------------------------------------------------------------------------------------
COMMITS_TWICE = "gru_h64_l2_b2_improved"   # its second stream commits at frames 0 and 3 (the restatement, frame by frame)


@pytest.mark.parametrize("name", list(tr.BEAM_CASES))
def test_stream_beam_frames_after_every_chunk(name):
    net, ora, audios, lens, beam, improved, _ = _beam(name)
    B = len(lens)
    for sched in (uniform_schedule(lens, 1), [(3, [0] * B)] + random_schedules(lens, 6, max_chunk=4)):
        state = net.init_beam_stream(B, 0, beam_widths=beam, improved=improved)
        ref = tr.BeamTimedRef(ora, B, 0, beam, improved)
        fed, commits = [0] * B, [0] * B   # commits: the chunks whose collection committed frames, per stream
        for x, ns in chunk_batches(audios, lens, sched):
            before = [len(c) for c in state.committed_frames]
            got = net.recognize_beams_stream(x.float().cuda(), ns, state, return_frames=True, return_scores=True)
            ref.feed(x, ns)
            fed = [f + n for f, n in zip(fed, ns)]
            commits = [c + (len(f) > n) for c, f, n in zip(commits, state.committed_frames, before)]
            for b in range(B):
                want = ref.nbest(b)
                assert [(y, f) for y, f, _ in got[b]] == [(y, f) for y, f, _ in want], (b, fed)
                assert state.stable_prefix(b, return_frames=True) == ref.stable_prefix(b)
                assert state.stable_prefix(b) == ref.stable_prefix(b)[0]
                if fed[b] and ns[b]:   # the offline search of this library on the frames fed so far
                    off = net.recognize_beams(audios[b:b + 1, :fed[b]].float().cuda().contiguous(), [fed[b]], 0, beam, improved,
                                              return_frames=True)
                    assert off == [(y, f) for y, f, _ in got[b]], (b, fed)
            assert ref.margin >= 1e-4
        assert state.frames_seen.tolist() == lens
        if name == COMMITS_TWICE and sched[0][0] == 1:   # committed frames accumulated over several collections of one stream
            assert max(commits) >= 2
    # reset restarts the frames of those rows; a chunk without return_frames leaves a stream's frames unknown until its reset
    state.reset([0])
    one = net.recognize_beams_stream(audios.float().cuda(), [lens[0]] + [0] * (B - 1), state, return_frames=True)
    assert one[0] == net.recognize_beams(audios[:1, :lens[0]].float().cuda().contiguous(), [lens[0]], 0, beam, improved, return_frames=True)
    net.recognize_beams_stream(audios.float().cuda()[:, :1].contiguous(), [1] + [0] * (B - 1), state)
    with pytest.raises(ValueError, match="return_frames"):
        state.stable_prefix(0, return_frames=True)
    assert state.stable_prefix(1, return_frames=True) == ref.stable_prefix(1)
    # the refused call launches nothing: encoder state, workspace and counters stay bitwise as they were, and the stream goes on
    # untimed to the offline result for everything it was fed
    kept = [t.clone() for t in (state.enc_h, state.enc_c, state.workspace, state.frames_seen) if t is not None]
    nxt = audios.float().cuda()[:, 1:2].contiguous()
    with pytest.raises(ValueError, match="return_frames"):
        net.recognize_beams_stream(nxt, [1] + [0] * (B - 1), state, return_frames=True)
    assert all(torch.equal(a, c) for a, c in zip(kept, [t for t in (state.enc_h, state.enc_c, state.workspace, state.frames_seen)
                                                        if t is not None]))
    after = net.recognize_beams_stream(nxt, [1] + [0] * (B - 1), state)
    utt = torch.cat((audios[0, :lens[0]], audios[0, :1], audios[0, 1:2]))[None].float().cuda()   # what stream 0 was fed since its reset
    assert after[0] == net.recognize_beams(utt, [utt.shape[1]], 0, beam, improved)
    assert state.frames_seen.tolist() == [lens[0] + 2] + lens[1:]


def test_stream_beam_collection_moves_frames_with_their_nodes():
    """A max_nodes the whole-utterance tree exceeds: the live tree is collected and compacted after every 1-frame chunk, and the
    frames are those of one whole chunk (no collection before the end) and of the restatement; committed frames plus the tail
    are the full list after every chunk.  This fixture commits one token only; commits in several chunks of one stream are
    covered by test_stream_beam_frames_after_every_chunk (COMMITS_TWICE)."""
    from rnntransducer_amd import ops
    from tests.test_beam_stream_oracle import fixture_oracle
    g, cfg, ora = fixture_oracle("s1_beams")
    net = _jointnet(cfg["transnet"], cfg["prednet"], cfg["V"], ora.state_dict())
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    B = len(t_list)
    opts = dict(beam_widths=cfg["beam"], improved=cfg["improved"])
    t_dev = torch.tensor(t_list, dtype=torch.int32, device="cuda")
    d = net.decoder
    _, st = ops.beam_search(net.encoder.forward_time_major(audios.cuda(), t_dev), net.fc.weight, net.fc.bias, d.embedding.weight,
                            d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias, 0, cfg["beam"], cfg["improved"],
                            t_lens=t_dev, stats=True)
    N = int(st[:, 5].max())
    cap = N - N // 8   # the whole-utterance tree of the longest utterance does not fit; its live tree does
    from rnntransducer_amd._lib import RnntHipError
    with pytest.raises(RnntHipError, match="max_nodes"):
        net.recognize_beams(audios.cuda(), t_list, 0, max_nodes=cap, return_frames=True, **opts)
    ref = tr.BeamTimedRef(ora, B, 0, cfg["beam"], cfg["improved"])
    ref.feed(audios, t_list)
    want = [[(y, f) for y, f, _ in ref.nbest(b)] for b in range(B)]
    assert [[y for y, _ in h] for h in want] == fixture_nbest(g)
    whole_state = net.init_beam_stream(B, 0, **opts)
    whole = net.recognize_beams_stream(audios.cuda(), t_list, whole_state, return_frames=True)
    assert whole == want
    state = net.init_beam_stream(B, 0, max_nodes=cap, **opts)
    grew, live = 0, 0
    for x, ns in chunk_batches(audios, t_list, uniform_schedule(t_list, 1)):
        before = [len(c) for c in state.committed_frames]
        small = net.recognize_beams_stream(x.cuda(), ns, state, return_frames=True)
        grew += sum(len(c) > n for c, n in zip(state.committed_frames, before))
        live = max(live, int(state.last_stats[:, 5].max()))
        for b in range(B):   # committed so far + tail = the full list, for every hypothesis
            sp, spf = state.stable_prefix(b, return_frames=True)
            assert all(y[:len(sp)] == sp and f[:len(sp)] == spf for y, f in small[b])
    assert small == want and live <= cap
    assert grew >= 1 and max(len(state.stable_prefix(b)) for b in range(B)) >= 2   # a frame really was committed by a chunk
    assert [state.stable_prefix(b, return_frames=True) for b in range(B)] == [ref.stable_prefix(b) for b in range(B)]


# 7. the offline and the streaming greedy entries on the same A: one loop, the same bits ----------------------------------
def _ops_greedy_net(cell, L, V, Hp, O, Oe, seed):
    """Random prediction net / joint weights at the ops level, scaled so that the argmax is rarely the blank."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: (scale * torch.randn(*shape, generator=g)).cuda()  # noqa: E731
    G = {0: 4, 1: 3, 2: 1}[cell]
    rnn = []
    for _ in range(L):
        rnn += [r(G * Hp, Hp, scale=0.3), r(G * Hp, Hp, scale=0.3), r(G * Hp, scale=0.3), r(G * Hp, scale=0.3)]
    return dict(fc_w=r(V, Oe + O, scale=0.5), fc_b=r(V, scale=0.1), emb_w=r(V, Hp), rnn=rnn, out_w=r(O, Hp, scale=0.3),
                out_b=r(O, scale=0.1))


@pytest.mark.parametrize("cell,L", [(0, 2), (1, 1), (2, 1)], ids=["lstm-2", "gru-1", "rnn_tanh-1"])
def test_offline_and_stream_greedy_entries_same_bits_on_the_same_A(cell, L):
    """ops.greedy_decode(timing=True), ops.stream_greedy on the whole A in one chunk and on A[:5] / A[5:] run the same frame
    loop (csrc/decode_shared.hpp) on the same A: tokens, counts, frames and logp are bitwise equal; a row without frames keeps
    the state its reset left, bitwise.  V = 1100: more than one pass of the 1024 threads and no multiple of 64."""
    from rnntransducer_amd import ops
    B, T, V, Hp, O, Oe, max_iters, blank = 4, 12, 1100, 32, 24, 16, 3, 0
    t_list = [12, 7, 0, 1]
    w = _ops_greedy_net(cell, L, V, Hp, O, Oe, 40 + cell)
    enc = (2.0 * torch.randn(T, B, Oe, generator=torch.Generator().manual_seed(7))).cuda()
    dev = enc.device
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    tok0, n0, fr0, lp0 = ops.greedy_decode(enc, w["fc_w"], w["fc_b"], w["emb_w"], w["rnn"], cell, w["out_w"], w["out_b"], blank,
                                           max_iters, t_lens=i32(t_list), timing=True)
    n0 = n0.tolist()
    assert sum(n0) > 10 and n0[2] == 0
    # the A greedy_decode computed: the same deterministic GEMM call on the same operands
    A = torch.empty(T, B, V, device=dev, dtype=torch.float32)
    ops.gemm(T * B, V, Oe, enc, w["fc_w"], A, b_sn=Oe + O, b_sk=1, bias=w["fc_b"], flags=ops.GEMM_GELU_A)
    h = torch.zeros(L, B, Hp, device=dev)
    c = torch.zeros(L, B, Hp, device=dev) if cell == 0 else None
    Cs, last = torch.zeros(B, V, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    net = (w["fc_w"], w["emb_w"], w["rnn"], cell, w["out_w"], w["out_b"], blank)

    def run(chunks):
        """reset every row, feed the chunks [(A_chunk, lens, frame_base)] -> per row (tokens, frames, logp) concatenated"""
        ops.stream_greedy_reset(i32(list(range(B))), *net, h, c, Cs, last)
        carried = [t for t in (h, c) if t is not None]
        primed = [t[:, 2].clone() for t in carried] + [Cs[2].clone(), last[2].clone()]
        out = [[[], [], []] for _ in range(B)]
        for a, lens, base in chunks:
            tok, n, fr, lp = ops.stream_greedy(a.contiguous(), i32(lens), *net, max_iters, h, c, Cs, last,
                                               frame_base=torch.tensor(base, dtype=torch.int64, device=dev))
            for b, k in enumerate(n.tolist()):
                for dst, src in zip(out[b], (tok, fr, lp)):
                    dst.append(src[b, :k])
        assert all(torch.equal(a, w) for a, w in zip([t[:, 2] for t in carried] + [Cs[2], last[2]], primed))
        return [[torch.cat(part) for part in row] for row in out]

    one = run([(A, t_list, [0] * B)])
    two = run([(A[:5], [min(t, 5) for t in t_list], [0] * B),
               (A[5:], [max(t - 5, 0) for t in t_list], [min(t, 5) for t in t_list])])
    for b in range(B):
        want = (tok0[b, :n0[b]], fr0[b, :n0[b]], lp0[b, :n0[b]])
        for got in (one[b], two[b]):
            assert len(got[0]) == n0[b]
            assert all(torch.equal(x, y) for x, y in zip(got, want)), b
