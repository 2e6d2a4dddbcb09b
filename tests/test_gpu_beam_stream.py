"""Streaming beam search on the GPU (csrc/beam_stream.hip: the offline kernel's frame loop from a carried hypothesis set) vs
the reference's fixtures on unidirectional encoders, itself under re-chunking (bitwise), the streaming restatement
(tests/beam_stream_restatement.py), and its guards."""
import ctypes
import os

import pytest
import torch

from tests.beam_stream_restatement import BeamStreamRef
from tests.test_beam_stream_oracle import UNI_FIXTURES, fixture_schedules
from tests.test_oracle_beam import fixture_nbest, load_fixture
from tests.test_stream_oracle import chunk_batches, make_oracle, random_schedules, uniform_schedule

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _jointnet(tn, pn, V, state_dict):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in state_dict.items()})
    return net.cuda().eval()


def _utterances(B, T, Fdim, lens, seed, dtype=torch.float64):
    x = torch.randn(B, T, Fdim, dtype=dtype, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def _run(net, audios, lens, schedule, blank=0, state=None, each=None, **opts):
    """Feed the schedule; -> (final n-best with scores per stream, state).  each(frames fed per stream, n-best, state) after
    every chunk."""
    state = state or net.init_beam_stream(len(lens), blank, **opts)
    fed, out = [0] * len(lens), None
    for x, ns in chunk_batches(audios.float(), lens, schedule):
        out = net.recognize_beams_stream(x.cuda(), ns, state, return_scores=True)
        fed = [f + n for f, n in zip(fed, ns)]
        if each:
            each(fed, out, state)
    return out, state


def _lists(nbest):
    return [[y for y, _ in h] for h in nbest]


def _state_tensors(st):
    return [t for t in (st.enc_h, st.enc_c, st.frames_seen) if t is not None]


def _row(t, r):
    return t.select(1 if t.dim() == 3 else 0, r)


# 1. the reference's fixtures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", UNI_FIXTURES)
def test_stream_beams_match_reference_fixture(tag):
    g, cfg, sd = load_fixture(GOLDEN, tag)
    net = _jointnet(cfg["transnet"], cfg["prednet"], cfg["V"], sd)
    blank = cfg["prednet"]["pad_token_id"]
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    opts = dict(beam_widths=cfg["beam"], improved=cfg["improved"], state_beam=cfg["state_beam"], expand_beam=cfg["expand_beam"])
    want = fixture_nbest(g)
    assert net.recognize_beams(audios.cuda(), t_list, blank, **opts) == want   # the offline search on the same model
    for sched in fixture_schedules(t_list):
        got, state = _run(net, audios, t_list, sched, blank, **opts)
        assert _lists(got) == want
        for b, hyps in enumerate(got):
            for r, (_, s) in enumerate(hyps):
                assert abs(s - g["scores"][b, r]) <= 1e-4 * max(1.0, abs(g["scores"][b, r]))
            sp = state.stable_prefix(b)
            assert sp[0] == blank and all(y[:len(sp)] == sp for y in want[b])
        assert state.frames_seen.tolist() == t_list


# 2. chunk invariance, bitwise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc_cell,dec_cell", [("lstm", "lstm"), ("gru", "rnn")])
def test_any_chunking_gives_the_same_lists_and_score_bits(enc_cell, dec_cell):
    ora, tn, pn = make_oracle(enc_cell=enc_cell, dec_cell=dec_cell, enc_layers=3, H=128, Hp=64, V=40, F_in=80, O=64, seed=11)
    net = _jointnet(tn, pn, 40, ora.state_dict())
    lens = [70, 33, 1, 64, 50]
    audios = _utterances(5, 70, 80, lens, 21)
    scheds = [uniform_schedule(lens, 70), uniform_schedule(lens, 1), uniform_schedule(lens, 7), uniform_schedule(lens, 64),
              random_schedules(lens, 5)]
    seen = {}   # (stream, frames fed) -> the n-best (lists and fp64 scores) of the first schedule that got there
    shared = 0

    def each(fed, out, state):
        nonlocal shared
        for b, n in enumerate(fed):
            if (b, n) in seen:
                assert out[b] == seen[(b, n)], (b, n)   # python floats: == is bitwise for non-NaN scores
                shared += 1
            else:
                seen[(b, n)] = out[b]

    finals = []
    for sched in scheds:
        out, state = _run(net, audios, lens, sched, beam_widths=5, improved=True, max_pops=1024, each=each)   # a random model pops a lot
        finals.append((out, [state.stable_prefix(b) for b in range(5)]))
    assert all(f == finals[0] for f in finals[1:])
    assert shared > 100 and sum(len(y) for y in _lists(finals[0][0])[0]) > 10
    # and the lists are the offline search's (other encoder kernels: tokens only where nothing hangs on fp32 rounding, so
    # only the count and the leading blank are asserted here; the fixtures above pin the values)
    off = net.recognize_beams(audios.float().cuda(), lens, 0, 5, True)
    assert [len(h) for h in off] == [len(h) for h in finals[0][0]]


# 3. against the restatement at config-2 sizes -------------------------------------------------------------------------
CONFIG2_CASES = [("lstm", 1, 5, True, 43), ("lstm", 1, 20, False, 43), ("gru", 1, 5, False, 42), ("lstm", 2, 20, True, 47)]


@pytest.mark.parametrize("cell,layers,beam,improved,seed", CONFIG2_CASES)
def test_stream_beams_vs_restatement_config2_sizes(cell, layers, beam, improved, seed):
    """The seeds were chosen on the CPU: the first of 40.. whose restatement margin, n-best sorts after every frame included,
    is >= 1e-4 (asserted, not skipped)."""
    from oracle.rnnt_oracle import OracleJointNet
    tn = dict(input_size=80, hidden_size=256, output_size=320, num_layers=2, rnn_type="lstm", dropout=0.0, bidirectional=False)
    pn = dict(embedding_size=72, pad_token_id=0, hidden_size=512, output_size=320, num_layers=layers, rnn_type=cell, dropout=0.0)
    lens = [3, 2]
    torch.manual_seed(seed)
    ora = OracleJointNet(tn, pn, 72).eval()
    with torch.no_grad():
        for n, p in ora.named_parameters():
            p.mul_(6.0 if n.startswith("fc.") else 3.0)
        ora.decoder.embedding.weight[0].zero_()
    audios = _utterances(2, 3, 80, lens, seed, torch.float32)
    net = _jointnet(tn, pn, 72, ora.state_dict())
    ref = BeamStreamRef(ora, 2, 0, beam, improved)
    state = net.init_beam_stream(2, 0, beam, improved)
    for x, ns in chunk_batches(audios, lens, uniform_schedule(lens, 1)):
        ref.feed(x, ns)
        got = net.recognize_beams_stream(x.cuda(), ns, state, return_scores=True)
        for b in range(2):
            want = ref.nbest(b)
            assert [y for y, _ in got[b]] == [y for y, _ in want]
            for (_, s), (_, w) in zip(got[b], want):
                assert abs(s - w) <= 1e-4 * max(1.0, abs(w)), (s, w)
            assert state.stable_prefix(b) == ref.stable_prefix(b)
    assert ref.margin >= 1e-4
    assert ref.pops > 2 * sum(lens) and any(len(y) > 1 for b in range(2) for y, _ in ref.nbest(b))


# 4. stable prefix and collection ---------------------------------------------------------------------------------------
def test_stable_prefix_matches_the_restatement_after_every_chunk():
    """Model and input chosen on the CPU: a confident model (fc scale 15) whose restatement margin over 1-frame chunks is
    1.9e-4 and whose committed list reaches 5 tokens (blank + 4) in both streams."""
    ora, tn, pn = make_oracle(seed=3, fc_scale=15.0, dtype=torch.float32)
    net = _jointnet(tn, pn, 12, ora.state_dict())
    lens = [40, 31]
    audios = _utterances(2, 40, 16, lens, 103, torch.float32)
    ref = BeamStreamRef(ora, 2, 0, 4, True)
    state = net.init_beam_stream(2, 0, 4, True)
    for x, ns in chunk_batches(audios, lens, uniform_schedule(lens, 1)):
        ref.feed(x, ns)
        got = net.recognize_beams_stream(x.cuda(), ns, state)
        for b in range(2):
            assert got[b] == [y for y, _ in ref.nbest(b)]
            assert state.stable_prefix(b) == ref.stable_prefix(b)
    assert ref.margin >= 1e-4
    assert all(len(state.stable_prefix(b)) >= 5 for b in range(2))
    whole, st_w = _run(net, audios, lens, uniform_schedule(lens, 40), beam_widths=4, improved=True)
    assert _lists(whole) == got and [st_w.stable_prefix(b) for b in range(2)] == [state.stable_prefix(b) for b in range(2)]


# 5. zero-frame chunks, reset, batch independence, determinism ---------------------------------------------------------
def test_zero_frame_streams_stay_bitwise_unchanged():
    ora, tn, pn = make_oracle(H=64, Hp=32, V=20, F_in=80, O=32)
    net = _jointnet(tn, pn, 20, ora.state_dict())
    state = net.init_beam_stream(3, 0, 4, True)
    assert net.recognize_beams_stream(torch.randn(3, 2, 80, device="cuda"), [0, 0, 0], state) == [[[0]]] * 3
    x = torch.randn(3, 10, 80, device="cuda")
    first = net.recognize_beams_stream(x, [10, 4, 10], state, return_scores=True)
    before = [t.clone() for t in _state_tensors(state)]
    ws = [state.workspace_row(b).clone() for b in range(3)]
    out = net.recognize_beams_stream(torch.randn(3, 6, 80, device="cuda"), [0, 6, 0], state, return_scores=True)
    assert out[0] == first[0] and out[2] == first[2] and out[1] != first[1]
    for a, b in zip(before, _state_tensors(state)):
        assert torch.equal(_row(a, 0), _row(b, 0)) and torch.equal(_row(a, 2), _row(b, 2))
    assert torch.equal(ws[0], state.workspace_row(0)) and torch.equal(ws[2], state.workspace_row(2))
    assert not torch.equal(ws[1], state.workspace_row(1))
    assert state.frames_seen.tolist() == [10, 10, 10]


def test_reset_starts_a_new_utterance_and_leaves_other_rows_alone():
    ora, tn, pn = make_oracle(enc_layers=2, H=128, Hp=64, V=30, F_in=80, O=64, seed=5)
    net = _jointnet(tn, pn, 30, ora.state_dict())
    first, second = _utterances(4, 24, 80, [24] * 4, 1), _utterances(4, 40, 80, [40] * 4, 2)
    sched1, sched2 = uniform_schedule([24] * 4, 8), uniform_schedule([40] * 4, 8)
    opts = dict(beam_widths=4, improved=True)
    _, st = _run(net, first, [24] * 4, sched1, **opts)
    keep = [t.clone() for t in _state_tensors(st)]
    ws = [st.workspace_row(b).clone() for b in range(4)]
    prefixes = [st.stable_prefix(b) for b in range(4)]
    st.reset([1, 3])
    for a, b in zip(keep, _state_tensors(st)):
        assert torch.equal(_row(a, 0), _row(b, 0)) and torch.equal(_row(a, 2), _row(b, 2))
    assert torch.equal(ws[0], st.workspace_row(0)) and torch.equal(ws[2], st.workspace_row(2))
    assert st.frames_seen.tolist() == [24, 0, 24, 0]
    assert st.stable_prefix(1) == [0] and st.stable_prefix(0) == prefixes[0]
    assert net.recognize_beams_stream(torch.zeros(4, 1, 80, device="cuda"), [0] * 4, st)[1] == [[0]]
    out_b, st = _run(net, second, [40] * 4, sched2, state=st)
    fresh, _ = _run(net, second, [40] * 4, sched2, **opts)
    cont, _ = _run(net, torch.cat([first, second], 1), [64] * 4, sched1 + sched2, **opts)
    assert any(len(y) > 1 for y, _ in fresh[1])   # the search emits symbols: the comparison is not between two [blank] lists
    assert out_b[1] == fresh[1] and out_b[3] == fresh[3]
    assert out_b[0] == cont[0] and out_b[2] == cont[2]


def test_more_streams_than_cus_and_determinism():
    ora, tn, pn = make_oracle(enc_layers=2, H=256, Hp=128, V=50, F_in=80, O=128, seed=7)
    net = _jointnet(tn, pn, 50, ora.state_dict())
    B = 300
    g = torch.Generator().manual_seed(6)
    lens = [int(n) for n in torch.randint(1, 25, (B,), generator=g)]
    audios = _utterances(B, 24, 80, lens, 4)
    sched = uniform_schedule(lens, 8)
    opts = dict(beam_widths=3, improved=True, max_pops=256, max_nodes=2048, max_len=64)   # small caps: a modest workspace
    out1, st1 = _run(net, audios, lens, sched, **opts)
    assert st1.workspace_bytes < 512 * (1 << 20)
    out2, st2 = _run(net, audios, lens, sched, **opts)
    assert out1 == out2
    assert all(torch.equal(a, b) for a, b in zip(_state_tensors(st1), _state_tensors(st2)))
    assert torch.equal(st1.workspace, st2.workspace) or all(torch.equal(st1.workspace_row(b), st2.workspace_row(b)) for b in (0, 150, 299))
    sub = [0, 77, 150, 299]
    sub_lens = [lens[b] for b in sub]
    out_s, st_s = _run(net, audios[sub], sub_lens, uniform_schedule(sub_lens, 8), **opts)
    assert out_s == [out1[b] for b in sub]   # a stream's result does not depend on the batch it is in
    assert [st_s.stable_prefix(i) for i in range(4)] == [st1.stable_prefix(b) for b in sub]
    assert any(len(y) > 1 for h in out_s for y, _ in h)


# 6. caps and guards ---------------------------------------------------------------------------------------------------
def test_caps_raise_name_themselves_and_reset_recovers():
    from rnntransducer_amd._lib import RnntHipError
    g, cfg, sd = load_fixture(GOLDEN, "s1_beams")
    net = _jointnet(cfg["transnet"], cfg["prednet"], cfg["V"], sd)
    audios, t_list = torch.from_numpy(g["audios"]).cuda(), g["t_lens"].tolist()
    opts = dict(beam_widths=cfg["beam"], improved=cfg["improved"])
    want = fixture_nbest(g)
    for kw in ("max_pops", "max_candidates", "max_states", "max_nodes", "max_len"):
        state = net.init_beam_stream(3, 0, **opts, **{kw: 1})
        with pytest.raises(RnntHipError, match=kw) as e:
            for t0 in range(0, max(t_list), 4):
                net.recognize_beams_stream(audios[:, t0:t0 + 4], [max(0, min(4, n - t0)) for n in t_list], state)
        assert "reset" in str(e.value)
        assert any(state.failed)
        with pytest.raises(RnntHipError, match="reset"):   # refused on the host until it is reset
            net.recognize_beams_stream(audios[:, :1], [1, 1, 1], state)
        state.reset([b for b in range(3) if state.failed[b]])
        assert not any(state.failed)
        net.recognize_beams_stream(audios[:, :1], [0, 0, 0], state)
    # one stream fails (a cap the long one outgrows, the short ones do not); the others keep their results and go on
    state = net.init_beam_stream(3, 0, **opts)
    whole = net.recognize_beams_stream(audios, t_list, state)
    assert whole == want
    nodes = [int(n) for n in state.last_stats[:, 5]]
    from rnntransducer_amd import ops
    t_dev = torch.tensor(t_list, dtype=torch.int32, device="cuda")
    d = net.decoder
    _, st = ops.beam_search(net.encoder.forward_time_major(audios, t_dev), net.fc.weight, net.fc.bias, d.embedding.weight,
                            d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias, 0, cfg["beam"], cfg["improved"],
                            t_lens=t_dev, stats=True)
    offline_nodes = st[:, 5].tolist()
    assert all(a <= b for a, b in zip(nodes, offline_nodes))
    cap = offline_nodes[2] + 1   # enough for the 9-frame utterance in one chunk, not for the 24-frame one
    assert cap < offline_nodes[0]
    state = net.init_beam_stream(3, 0, **opts, max_nodes=cap)
    with pytest.raises(RnntHipError, match="stream 0 .*max_nodes"):
        net.recognize_beams_stream(audios, t_list, state)
    assert state.failed == [True, state.failed[1], False]
    assert state.nbest[2] == [(y, s) for y, s in zip(want[2], g["scores"][2])] or [y for y, _ in state.nbest[2]] == want[2]
    state.reset([b for b in range(3) if state.failed[b]])
    out = net.recognize_beams_stream(audios[:, :9], [9, 9, 0], state)
    assert out[2] == want[2] and out[0] != [[0]]


def test_small_max_nodes_is_enough_when_the_tree_is_collected():
    """max_nodes bounds the LIVE tree: a cap the whole-utterance tree exceeds (offline raises) is enough for the stream fed in
    small chunks, and collection after every 1-frame chunk changes no result against one whole chunk."""
    from rnntransducer_amd import ops
    from rnntransducer_amd._lib import RnntHipError
    g, cfg, sd = load_fixture(GOLDEN, "s1_beams")
    net = _jointnet(cfg["transnet"], cfg["prednet"], cfg["V"], sd)
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    opts = dict(beam_widths=cfg["beam"], improved=cfg["improved"])
    t_dev = torch.tensor(t_list, dtype=torch.int32, device="cuda")
    d = net.decoder
    _, st = ops.beam_search(net.encoder.forward_time_major(audios.cuda(), t_dev), net.fc.weight, net.fc.bias, d.embedding.weight,
                            d.rnn.flat_weights(), d.rnn.CELL, d.out_proj.weight, d.out_proj.bias, 0, cfg["beam"], cfg["improved"],
                            t_lens=t_dev, stats=True)
    N = int(st[:, 5].max())
    cap = N - N // 8   # the whole-utterance tree of the longest utterance does not fit; its live tree does
    with pytest.raises(RnntHipError, match="max_nodes"):
        net.recognize_beams(audios.cuda(), t_list, 0, max_nodes=cap, **opts)
    whole, st_w = _run(net, audios, t_list, uniform_schedule(t_list, max(t_list)), **opts)
    live = []
    small, st_s = _run(net, audios, t_list, uniform_schedule(t_list, 1), max_nodes=cap, **opts,
                       each=lambda fed, out, state: live.append(int(state.last_stats[:, 5].max())))
    assert small == whole and _lists(small) == fixture_nbest(g)
    assert [st_s.stable_prefix(b) for b in range(3)] == [st_w.stable_prefix(b) for b in range(3)]
    print("offline nodes", st[:, 5].tolist(), "cap", cap, "max live nodes after a chunk", max(live))
    assert max(live) <= cap


def test_guards():
    from argparse import Namespace
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.networks import JointNet
    ora, tn, pn = make_oracle(H=64, Hp=32, V=20, F_in=80, O=32)
    net = _jointnet(tn, pn, 20, ora.state_dict())
    state = net.init_beam_stream(2, 0, 3, True)
    x = torch.randn(2, 5, 80, device="cuda")
    keep = [t.clone() for t in _state_tensors(state)] + [state.workspace.clone()]

    def untouched():
        return all(torch.equal(a, b) for a, b in zip(keep, _state_tensors(state) + [state.workspace]))

    with pytest.raises(RnntHipError):
        net.recognize_beams_stream(x.cpu(), [5, 5], state)
    with pytest.raises(ValueError):
        net.recognize_beams_stream(torch.randn(3, 5, 80, device="cuda"), [5, 5, 5], state)
    for bad in ([6, 5], [-1, 2], [5]):
        with pytest.raises(ValueError):
            net.recognize_beams_stream(x, bad, state)
    with pytest.raises(ValueError, match="features"):
        net.recognize_beams_stream(torch.randn(2, 5, 81, device="cuda"), [5, 5], state)
    with pytest.raises(ValueError):
        state.reset([2])
    net.train()
    with pytest.raises(RuntimeError):
        net.recognize_beams_stream(x, [5, 5], state)
    net.eval()
    same = _jointnet(tn, pn, 20, ora.state_dict())
    with pytest.raises(ValueError, match="another model"):
        net.recognize_beams_stream(x, [5, 5], same.init_beam_stream(2, 0, 3, True))
    with pytest.raises(ValueError, match="init_beam_stream"):
        net.recognize_beams_stream(x, [5, 5], net.init_stream(2, 0))     # a greedy state to the beam call
    with pytest.raises(ValueError, match="init_stream"):
        net.recognize_greedy_stream(x, [5, 5], state)                    # and the reverse
    assert untouched()
    bi = JointNet(dict(tn, bidirectional=True), dict(pn), 20).cuda().eval()
    with pytest.raises(ValueError):
        bi.init_beam_stream(2, 0)
    with pytest.raises(ValueError):
        net.init_beam_stream(2, 0, device="cpu")
    with pytest.raises(ValueError):
        net.init_beam_stream(2, 0, max_pops=0)
    with pytest.raises(TypeError):
        net.init_beam_stream(2, 0, max_everything=3)
    # fp16 compute mode is not an error: streaming computes fp32
    a = net.set_compute_precision("fp16").recognize_beams_stream(x, [5, 5], net.init_beam_stream(2, 0, 3, True), return_scores=True)
    b = net.set_compute_precision("fp32").recognize_beams_stream(x, [5, 5], net.init_beam_stream(2, 0, 3, True), return_scores=True)
    assert a == b
    # the model surface passes through with its blank
    args = Namespace(learning_rate=1e-3, weight_decay=0.0, warmup_ratio=0.1, final_div_factor=10.0, total_steps=10)
    m = RNNTransducer(dict(pn), dict(tn), dict(num_classes=20), args).cuda().eval()
    st = m.init_beam_stream(2, beam_widths=3, improved=True)
    out = m.recognize_beams_stream(x, [5, 3], st)
    assert st.blank == m.blank_token_id and len(out) == 2 and all(h[0][0] == m.blank_token_id for h in out)
    assert st.workspace_bytes >= 2 * st.bytes_per_stream > 0


# 7. the C ABI ---------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_workspace_query():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    for name in ("rnnt_hip_beam_stream_workspace_bytes", "rnnt_hip_beam_stream_reset", "rnnt_hip_beam_stream_chunk"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.rnnt_hip_beam_stream_workspace_bytes(None) == 0
    d = _lib.BeamStreamDesc()
    assert L.rnnt_hip_beam_stream_workspace_bytes(ctypes.byref(d)) == 0     # all zero: bad dims
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank, d.beam = 0, 3, 72, 512, 320, 1, 0, 0, 5
    d.max_candidates, d.max_pops, d.max_states, d.max_nodes, d.max_len = 128 * 72, 128, 384, 8192, 256
    n = L.rnnt_hip_beam_stream_workspace_bytes(ctypes.byref(d))
    assert 3 * (2 << 20) < n < 3 * (5 << 19)    # about 2.15 MB per stream at these (default) caps
    d.max_nodes = 0
    assert L.rnnt_hip_beam_stream_workspace_bytes(ctypes.byref(d)) == 0     # a cap below 1
    assert L.rnnt_hip_beam_stream_chunk(None, None) == -1 and L.rnnt_hip_beam_stream_reset(None, None, 0, 0, None) == -1
    assert _lib.ABI_VERSION == 4
