"""(The encoder kernels at their own shape edges, driven without a model: tests/test_gpu_stream_shapes.py.)
Streaming greedy recognition on the GPU (csrc/stream.hip): the chunked encoder against float64, bitwise chunk invariance,
tokens against the offline search (the oracle's and this library's), slot reset, many streams, determinism and the guards."""
import pytest
import torch

from tests.test_stream_oracle import StreamRef, chunk_batches, make_oracle, random_schedules, uniform_schedule

pytestmark = pytest.mark.gpu

FWD_ATOL = 2e-5   # tests/test_gpu_lstm.py


def _jointnet(tn, pn, V, state_dict):
    from rnntransducer_amd.networks import JointNet
    net = JointNet(dict(tn), dict(pn), V)
    net.load_state_dict({k: v.float() for k, v in state_dict.items()})
    return net.cuda().eval()


def _utterances(B, T, Fdim, lens, seed):
    x = torch.randn(B, T, Fdim, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def _stream_encoder(net, audios, lens, schedule):
    """forward_stream over the schedule -> per-stream concatenated outputs and the final state."""
    outs, state = [[] for _ in lens], None
    for x, ns in chunk_batches(audios.float(), lens, schedule):
        y, state = net.encoder.forward_stream(x.cuda(), ns, state)
        for b, n in enumerate(ns):
            outs[b].append(y[b, :n])
        assert all(bool((y[b, n:] == 0).all()) for b, n in enumerate(ns))
    return [torch.cat(o) for o in outs], state


def _stream_tokens(net, audios, lens, schedule, max_iters=3, blank=0, state=None):
    state = state or net.init_stream(len(lens), blank)
    toks = [[] for _ in lens]
    for x, ns in chunk_batches(audios.float(), lens, schedule):
        for b, t in enumerate(net.recognize_greedy_stream(x.cuda(), ns, state, max_iters)):
            assert t.dtype == torch.int64 and t.dim() == 1
            toks[b] += t.tolist()
    return toks, state


def _row(t, r):
    """Row r of a state tensor: dim 1 of (L,B,H), dim 0 of (B,V) / (B,)."""
    return t.select(1 if t.dim() == 3 else 0, r)


def _state_tensors(st):
    return [t for t in (st.enc_h, st.enc_c, st.pred_h, st.pred_c, st.pred_joint, st.last_token, st.frames_seen) if t is not None]


# 1. encoder vs float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "gru", "rnn-tanh", "rnn-relu"])
@pytest.mark.parametrize("L,H", [(1, 64), (2, 512), (4, 512), (8, 64), (1, 1024), (8, 1024), (4, 64), (2, 1024)])
def test_encoder_stream_vs_float64(cell, L, H):
    from oracle.rnnt_oracle import OracleJointNet
    rnn_type = cell.split("-")[0]
    tn = dict(input_size=80, hidden_size=H, output_size=96, num_layers=L, rnn_type=rnn_type, dropout=0.0, bidirectional=False)
    pn = dict(embedding_size=8, pad_token_id=0, hidden_size=16, output_size=16, num_layers=1, dropout=0.0)
    torch.manual_seed(L * 1000 + H)
    ora = OracleJointNet(tn, pn, 8).eval()
    if cell == "rnn-relu":
        ora.encoder.rnn.nonlinearity, ora.encoder.rnn.mode = "relu", "RNN_RELU"
    ora = ora.double()
    net = _jointnet(tn, pn, 8, ora.state_dict())
    if cell == "rnn-relu":
        net.encoder.rnn.CELL = 3
    lens = [23, 9, 0, 16]
    audios = _utterances(4, 23, 80, lens, L + H)
    got, state = _stream_encoder(net, audios, lens, uniform_schedule(lens, 7))
    h, c = state if rnn_type == "lstm" else (state, None)
    with torch.no_grad():
        for b, n in enumerate(lens):
            if n == 0:
                assert bool((h[:, b] == 0).all())
                continue
            y, st = ora.encoder.rnn(audios[b:b + 1, :n])
            want = ora.encoder.out_proj(y[0])
            assert (got[b].double().cpu() - want).abs().max().item() < FWD_ATOL
            hn, cn = st if rnn_type == "lstm" else (st, None)
            assert (h[:, b].double().cpu() - hn[:, 0]).abs().max().item() < FWD_ATOL
            if cn is not None:
                assert (c[:, b].double().cpu() - cn[:, 0]).abs().max().item() < FWD_ATOL


# 2. bitwise chunk invariance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc_cell,dec_cell", [("lstm", "lstm"), ("gru", "rnn")])
def test_any_chunking_gives_the_same_bits(enc_cell, dec_cell):
    ora, tn, pn = make_oracle(enc_cell=enc_cell, dec_cell=dec_cell, enc_layers=3, H=128, Hp=64, V=40, F_in=80, O=64, seed=11)
    net = _jointnet(tn, pn, 40, ora.state_dict())
    lens = [70, 33, 1, 64, 50]
    audios = _utterances(5, 70, 80, lens, 21)
    scheds = [uniform_schedule(lens, 70), uniform_schedule(lens, 1), uniform_schedule(lens, 7), uniform_schedule(lens, 64),
              random_schedules(lens, 5)]
    base_enc, base_state = _stream_encoder(net, audios, lens, scheds[0])
    base_tok, base_st = _stream_tokens(net, audios, lens, scheds[0])
    assert sum(map(len, base_tok)) > 20
    for sched in scheds[1:]:
        enc, state = _stream_encoder(net, audios, lens, sched)
        assert all(torch.equal(a, b) for a, b in zip(enc, base_enc))
        st_a = state if isinstance(state, tuple) else (state,)
        st_b = base_state if isinstance(base_state, tuple) else (base_state,)
        assert all(torch.equal(a, b) for a, b in zip(st_a, st_b))
        tok, st = _stream_tokens(net, audios, lens, sched)
        assert tok == base_tok
        assert all(torch.equal(a, b) for a, b in zip(_state_tensors(st), _state_tensors(base_st)))
        assert torch.equal(st.enc_h, st_a[0])   # the greedy path runs the same encoder


def test_zero_frame_streams_stay_bitwise_unchanged():
    ora, tn, pn = make_oracle(H=64, Hp=32, V=20, F_in=80, O=32)
    net = _jointnet(tn, pn, 20, ora.state_dict())
    state = net.init_stream(3, 0)
    x = torch.randn(3, 10, 80, device="cuda")
    net.recognize_greedy_stream(x, [10, 4, 10], state)
    before = [t.clone() for t in _state_tensors(state)]
    out = net.recognize_greedy_stream(torch.randn(3, 6, 80, device="cuda"), [0, 6, 0], state)
    assert out[0].numel() == 0 and out[2].numel() == 0
    after = _state_tensors(state)
    for a, b in zip(before, after):
        assert torch.equal(_row(a, 0), _row(b, 0)) and torch.equal(_row(a, 2), _row(b, 2))
    assert state.frames_seen.tolist() == [10, 10, 10]
    assert all(t.numel() == 0 for t in net.recognize_greedy_stream(x, [0, 0, 0], state))


# 3. tokens vs offline -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["base", "gru_encoder", "pred2", "max_iters1", "V2048"])
def test_stream_tokens_vs_offline(variant):
    enc_cell = "gru" if variant == "gru_encoder" else "lstm"
    V = 2048 if variant == "V2048" else 72
    max_iters = 1 if variant == "max_iters1" else 3
    ora, tn, pn = make_oracle(enc_cell=enc_cell, enc_layers=4, H=512, dec_layers=2 if variant == "pred2" else 1, Hp=512, V=V,
                              F_in=80, O=320, seed=17)
    net = _jointnet(tn, pn, V, ora.state_dict())
    lens = [60, 48, 31, 5]
    audios = _utterances(4, 60, 80, lens, 3)
    with torch.no_grad():
        want, margin = ora.recognize_greedy(audios, lens, 0, max_iters, return_margin=True)
    assert sum(len(w) for w in want) > 20   # the case really decodes something
    offline = [t.tolist() for t in net.recognize_greedy(audios.float().cuda(), lens, 0, max_iters)]
    for sched in (uniform_schedule(lens, 16), random_schedules(lens, 8)):
        got, _ = _stream_tokens(net, audios, lens, sched, max_iters)
        for ref in (want, offline):
            if margin >= 1e-4:
                assert got == ref
            else:   # a near-tie somewhere: fp32 summation order may flip it; everything before must agree
                for a, b in zip(got, ref):
                    if a != b:
                        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                        assert k >= 3, (margin, a[:12], b[:12])


# 4. reset -------------------------------------------------------------------------------------------------------------
def test_reset_starts_a_new_utterance_and_leaves_other_rows_alone():
    ora, tn, pn = make_oracle(enc_layers=2, H=128, Hp=64, V=30, F_in=80, O=64, seed=5)
    net = _jointnet(tn, pn, 30, ora.state_dict())
    first, second = _utterances(4, 24, 80, [24] * 4, 1), _utterances(4, 40, 80, [40] * 4, 2)
    sched1, sched2 = uniform_schedule([24] * 4, 8), uniform_schedule([40] * 4, 8)
    tok_a, st = _stream_tokens(net, first, [24] * 4, sched1)
    keep = [t.clone() for t in _state_tensors(st)]
    st.reset([1, 3])
    for a, b in zip(keep, _state_tensors(st)):   # rows 0 and 2 untouched by the reset itself
        assert torch.equal(_row(a, 0), _row(b, 0)) and torch.equal(_row(a, 2), _row(b, 2))
    assert st.frames_seen.tolist() == [24, 0, 24, 0] and st.last_token[1].item() == 0
    tok_b, st = _stream_tokens(net, second, [40] * 4, sched2, state=st)
    fresh, _ = _stream_tokens(net, second, [40] * 4, sched2)
    cont, st_c = _stream_tokens(net, torch.cat([first, second], 1), [64] * 4, sched1 + sched2)
    assert sum(map(len, fresh)) > 10
    assert tok_b[1] == fresh[1] and tok_b[3] == fresh[3]
    assert tok_a[0] + tok_b[0] == cont[0] and tok_a[2] + tok_b[2] == cont[2]
    for a, b in zip(_state_tensors(st), _state_tensors(st_c)):
        assert torch.equal(_row(a, 0), _row(b, 0)) and torch.equal(_row(a, 2), _row(b, 2))


# 5. scale and determinism ---------------------------------------------------------------------------------------------
def test_more_streams_than_cus_and_determinism():
    ora, tn, pn = make_oracle(enc_layers=2, H=256, Hp=128, V=50, F_in=80, O=128, seed=7)
    net = _jointnet(tn, pn, 50, ora.state_dict())
    B = 300
    g = torch.Generator().manual_seed(6)
    lens = [int(n) for n in torch.randint(1, 41, (B,), generator=g)]
    audios = _utterances(B, 40, 80, lens, 4)
    sched = uniform_schedule(lens, 16)
    tok1, st1 = _stream_tokens(net, audios, lens, sched)
    tok2, st2 = _stream_tokens(net, audios, lens, sched)
    assert tok1 == tok2
    assert all(torch.equal(a, b) for a, b in zip(_state_tensors(st1), _state_tensors(st2)))
    # a stream's bits do not depend on the batch it is in
    sub = [0, 77, 150, 299]
    tok_s, st_s = _stream_tokens(net, audios[sub], [lens[b] for b in sub], uniform_schedule([lens[b] for b in sub], 16))
    assert tok_s == [tok1[b] for b in sub]
    assert torch.equal(st_s.pred_h, st1.pred_h[:, sub]) and torch.equal(st_s.enc_h, st1.enc_h[:, sub])
    # and the tokens are the float64 restatement's
    with torch.no_grad():
        ref = StreamRef(ora, len(sub), 0)
        for x, ns in chunk_batches(audios[sub], [lens[b] for b in sub], uniform_schedule([lens[b] for b in sub], 16)):
            ref.feed(x, ns)
    assert sum(map(len, ref.tokens)) > 5
    assert tok_s == ref.tokens


# 6. guards ------------------------------------------------------------------------------------------------------------
def test_guards():
    from rnntransducer_amd.networks import JointNet
    from rnntransducer_amd._lib import RnntHipError
    ora, tn, pn = make_oracle(H=64, Hp=32, V=20, F_in=80, O=32)
    net = _jointnet(tn, pn, 20, ora.state_dict())
    state = net.init_stream(2, 0)
    x = torch.randn(2, 5, 80, device="cuda")
    with pytest.raises(RnntHipError):
        net.recognize_greedy_stream(x.cpu(), [5, 5], state)
    with pytest.raises(RnntHipError):
        net.encoder.forward_stream(x.cpu(), [5, 5])
    with pytest.raises(ValueError):
        net.recognize_greedy_stream(torch.randn(3, 5, 80, device="cuda"), [5, 5, 5], state)
    for bad in ([6, 5], [-1, 2], [5]):
        with pytest.raises(ValueError):
            net.recognize_greedy_stream(x, bad, state)
        with pytest.raises(ValueError):
            net.encoder.forward_stream(x, bad)
    with pytest.raises(ValueError):
        state.reset([2])
    net.train()
    with pytest.raises(RuntimeError):
        net.recognize_greedy_stream(x, [5, 5], state)
    with pytest.raises(RuntimeError):
        net.encoder.forward_stream(x, [5, 5])
    net.eval()
    # fp16 compute mode is not an error: streaming computes fp32
    net.set_compute_precision("fp16")
    assert [t.tolist() for t in net.recognize_greedy_stream(x, [5, 5], net.init_stream(2, 0))] == \
        [t.tolist() for t in net.set_compute_precision("fp32").recognize_greedy_stream(x, [5, 5], net.init_stream(2, 0))]
    bi = JointNet(dict(tn, bidirectional=True), dict(pn), 20).cuda().eval()
    with pytest.raises(ValueError):
        bi.init_stream(2, 0)
    with pytest.raises(ValueError):
        bi.encoder.forward_stream(x, [5, 5])
    # kernel limits name themselves
    deep = JointNet(dict(tn, num_layers=9), dict(pn), 20).cuda().eval()
    with pytest.raises(RnntHipError, match="RNNT_STREAM_MAX_LAYERS"):
        deep.encoder.forward_stream(x, [5, 5])
    wide = JointNet(dict(tn, input_size=4096, hidden_size=1024), dict(pn), 20).cuda().eval()
    with pytest.raises(RnntHipError, match="LDS"):
        wide.encoder.forward_stream(torch.randn(2, 3, 4096, device="cuda"), [3, 3])
    # the model surface passes through with its blank
    from argparse import Namespace
    from rnntransducer_amd import RNNTransducer
    args = Namespace(learning_rate=1e-3, weight_decay=0.0, warmup_ratio=0.1, final_div_factor=10.0, total_steps=10)
    m = RNNTransducer(dict(pn), dict(tn), dict(num_classes=20), args).cuda().eval()
    st = m.init_stream(2)
    assert st.blank == m.blank_token_id and len(m.recognize_greedy_stream(x, [5, 3], st)) == 2


def test_shape_guards_before_any_launch():
    """The kernels index raw pointers: a chunk of another feature width, a state opened by another model and mismatched
    tensors at the ops level are refused on the host; a caller's state of another dtype / device is refused and a strided one
    is read as a dense copy."""
    from rnntransducer_amd import ops
    from rnntransducer_amd.networks import JointNet
    ora, tn, pn = make_oracle(H=64, Hp=32, V=20, F_in=80, O=32)
    net = _jointnet(tn, pn, 20, ora.state_dict())
    state = net.init_stream(2, 0)
    x = torch.randn(2, 5, 80, device="cuda")
    keep = [t.clone() for t in _state_tensors(state)]
    for width in (79, 81, 160):
        with pytest.raises(ValueError, match="features"):
            net.recognize_greedy_stream(torch.randn(2, 5, width, device="cuda"), [5, 5], state)
        with pytest.raises(ValueError, match="features"):
            net.encoder.forward_stream(torch.randn(2, 5, width, device="cuda"), [5, 5])
    # a state opened by another model, of the same sizes or of others
    same = _jointnet(tn, pn, 20, ora.state_dict())
    other = JointNet(dict(tn, hidden_size=128), dict(pn, hidden_size=48, embedding_size=24), 24).cuda().eval()
    for foreign in (same.init_stream(2, 0), other.init_stream(2, 0)):
        with pytest.raises(ValueError, match="another model"):
            net.recognize_greedy_stream(x, [5, 5], foreign)
    state.pred_joint = state.pred_joint[:, :10]
    with pytest.raises(ValueError, match="pred_joint"):
        net.recognize_greedy_stream(x, [5, 5], state)
    state.pred_joint = keep[4].clone()
    assert all(torch.equal(a, b) for a, b in zip(keep, _state_tensors(state)))   # nothing ran
    # the ops entries check every shape on their own
    st_other = other.init_stream(2, 0)
    enc, dec = net.encoder, net.decoder
    out = torch.zeros(2, 5, 32, device="cuda")
    lens = torch.tensor([5, 5], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):   # encoder state of another hidden size
        ops.stream_rnn_chunk(x, lens, enc.rnn.flat_weights(), enc.rnn.CELL, st_other.enc_h, st_other.enc_c, enc.out_proj.weight,
                             enc.out_proj.bias, out, (5 * 32, 32))
    with pytest.raises(ValueError):   # chunk of another width
        ops.stream_rnn_chunk(torch.randn(2, 5, 81, device="cuda"), lens, enc.rnn.flat_weights(), enc.rnn.CELL, state.enc_h,
                             state.enc_c, enc.out_proj.weight, enc.out_proj.bias, out, (5 * 32, 32))
    with pytest.raises(ValueError):   # output buffer too small
        ops.stream_rnn_chunk(x, lens, enc.rnn.flat_weights(), enc.rnn.CELL, state.enc_h, state.enc_c, enc.out_proj.weight,
                             enc.out_proj.bias, out[:1], (5 * 32, 32))
    A = torch.zeros(5, 2, 20, device="cuda")
    with pytest.raises(ValueError):   # prediction-net state of another model
        ops.stream_greedy(A, lens, net.fc.weight, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight,
                          dec.out_proj.bias, 0, 3, st_other.pred_h, st_other.pred_c, st_other.pred_joint, st_other.last_token)
    # init_stream only on the model's device
    with pytest.raises(ValueError):
        net.init_stream(2, 0, device="cpu")
    assert net.init_stream(2, 0, device="cuda").device == net.fc.weight.device
    # forward_stream's state: float32 on the chunk's device; a strided view is read as what it holds
    y, (h, c) = net.encoder.forward_stream(x, [5, 5])
    with pytest.raises(ValueError):
        net.encoder.forward_stream(x, [5, 5], (h.double(), c.double()))
    with pytest.raises(ValueError):
        net.encoder.forward_stream(x, [5, 5], (h.cpu(), c.cpu()))
    ht, ct = h.transpose(0, 1).contiguous().transpose(0, 1), c.transpose(0, 1).contiguous().transpose(0, 1)
    assert not ht.is_contiguous() and torch.equal(ht, h)
    y1, (h1, c1) = net.encoder.forward_stream(x, [5, 5], (h, c))
    y2, (h2, c2) = net.encoder.forward_stream(x, [5, 5], (ht, ct))
    assert torch.equal(y1, y2) and torch.equal(h1, h2) and torch.equal(c1, c2)
