"""Backoff n-gram fusion on the GPU (csrc/search_shared.hpp: ngram_lookup, the FUSE_NGRAM instances of the frame-synchronous
transducer search, its streaming form and the CTC prefix beam search).  The oracle is the model's own dense expansion: with
fusion=lm and fusion=lm.to_dense() a search must return the same lists, the same fp64 score and fused-score bits and the same
frames.  The seeded cases (tests/ngram_cases.py, their margins asserted on the CPU by tests/test_ngram_fusion.py) are also
compared with the float64 restatements, and a model too large for the dense form with the host scorer, bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests import beam_sync_cases as K
from tests import ctc_beam_cases as CK
from tests import ngram_cases as NK
from tests.test_gpu_ctc_beam import compare as ctc_compare

pytestmark = pytest.mark.gpu


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


# ---- sparse equals dense, and both the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("c", NK.SYNC_CASES, ids=NK.sync_id)
def test_sync_search_sparse_is_dense_bit_for_bit_and_matches_the_restatement(c):
    W, S, thr = c
    _, ora, tn, pn, x, lm, want = NK.sync_case(c)
    net = _jointnet(tn, pn, NK.V, ora)
    sparse = _decode(net, x, [NK.T], 0, W, S, token_min_logp=thr, fusion=lm.to("cuda"))
    dense = _decode(net, x, [NK.T], 0, W, S, token_min_logp=thr, fusion=lm.to_dense().to("cuda"))
    assert sparse == dense                                                     # python floats: == is bitwise
    K.same_hyps(sparse, want.hyps)
    for y, s, f, _ in sparse:
        total, final, _ = lm.score(y)
        assert f == (s + total) + final
    assert any(f != s for _, s, f, _ in sparse)


def test_ragged_batch_sparse_is_dense():
    from rnntransducer_amd import ops
    from rnntransducer_amd.networks.encoder import lengths_to_device
    c = K.RAGGED
    _, ora, tn, pn, x, lm, want = NK.ragged_case()
    net = _jointnet(tn, pn, c["V"], ora)
    with torch.no_grad():
        enc = net.encoder.forward_time_major(x.cuda(), lengths_to_device([max(n, 1) for n in c["lens"]], "cuda")).contiguous()
    t_lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    dec = net.decoder
    run = lambda f: ops.beam_search_sync(enc, net.fc.weight, net.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                                         dec.out_proj.weight, dec.out_proj.bias, 0, c["W"], c["S"], t_lens, frames=True, fusion=f)
    sparse, dense = run(lm.to("cuda")), run(lm.to_dense().to("cuda"))
    assert sparse == dense
    for b in range(len(c["lens"])):
        K.same_hyps(sparse[b], want[b].hyps)
    assert sparse[1] == [([0], 0.0, lm.score([0])[1], [-1])]                    # no frames: [[blank]], the start state's final


def test_blank_in_the_last_position_sparse_is_dense():
    blank, V, T, W, S = NK.BLANK_LAST
    _, ora, tn, pn, x, lm, want = NK.blank_last_case()
    net = _jointnet(tn, pn, V, ora)
    sparse = _decode(net, x, [T], blank, W, S, fusion=lm.to("cuda"))
    assert sparse == _decode(net, x, [T], blank, W, S, fusion=lm.to_dense().to("cuda"))
    K.same_hyps(sparse, want.hyps)
    assert all(y[0] == blank and blank not in y[1:] for y, *_ in sparse)


@pytest.mark.parametrize("c", NK.CTC_CASES, ids=lambda c: "W%d-%s" % (c[2], "all" if c[3] == -math.inf else "pruned"))
def test_ctc_search_sparse_is_dense_bit_for_bit_and_matches_the_restatement(c):
    from rnntransducer_amd.ops import ctc_beam_search
    T, V, W, thr, _ = c
    _, z, want, lm = NK.ctc_case(c)
    zb, tl = CK.batch_of([z, z[:T // 2]], T + 3, V)
    run = lambda f: ctc_beam_search(zb.cuda(), tl.cuda(), 0, W, token_min_logp=thr, fusion=f, return_frames=True)
    sparse, dense = run(lm.to("cuda")), run(lm.to_dense().to("cuda"))
    assert sparse == dense
    ctc_compare(sparse[0], want, fused=True, frames=True)
    for y, s, f, _ in sparse[0] + sparse[1]:
        total, final, _ = lm.score([0] + y)
        assert f == (s + total) + final


@pytest.mark.parametrize("W", [1, 6])
def test_recognize_ctc_beams_sparse_is_dense(W):
    from rnntransducer_amd import JointNet
    torch.manual_seed(3)
    tn = dict(input_size=12, hidden_size=16, output_size=12, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=False)
    pn = dict(embedding_size=NK.V, hidden_size=8, output_size=8, num_layers=1, pad_token_id=0)
    net = JointNet(tn, pn, NK.V, aux_ctc=True)
    with torch.no_grad():
        net.ctc_head.weight.mul_(8.0)      # logits with some contrast: an untrained head is close to uniform
    net = net.cuda().eval()
    x = torch.randn(2, 9, 12, generator=torch.Generator().manual_seed(5)).cuda()
    lm = NK.random_lm(NK.V, 0)
    kw = dict(return_scores=True, return_frames=True)
    sparse = net.recognize_ctc_beams(x, [9, 6], 0, W, fusion=lm.to("cuda"), **kw)
    assert sparse == net.recognize_ctc_beams(x, [9, 6], 0, W, fusion=lm.to_dense().to("cuda"), **kw)
    assert all(len(h) == min(W, len(h)) >= 1 for h in sparse)


@pytest.mark.parametrize("chunk", [1, 3, NK.T])
def test_sync_stream_sparse_is_dense_after_every_chunk(chunk):
    c = (6, 3, -math.inf)
    W, S, _ = c
    _, ora, tn, pn, x, lm, _ = NK.sync_case(c)
    net = _jointnet(tn, pn, NK.V, ora)
    sparse, dense = (net.init_beam_sync_stream(1, 0, W, S, fusion=f) for f in (lm.to("cuda"), lm.to_dense().to("cuda")))
    xc = x.cuda()
    kw = dict(return_scores=True, return_frames=True)
    got = None
    for n in range(0, NK.T, chunk):
        k = min(chunk, NK.T - n)
        got = net.recognize_beams_sync_stream(xc[:, n:n + k], [k], sparse, **kw)
        assert got == net.recognize_beams_sync_stream(xc[:, n:n + k], [k], dense, **kw), n
        assert sparse.stable_prefix(0, return_frames=True) == dense.stable_prefix(0, return_frames=True)
        assert sparse.header(0) == dense.header(0)
    for y, _, s, f in got[0]:
        total, final, _ = lm.score(y)
        assert f == (s + total) + final


# ---- a model the dense form refuses ----------------------------------------------------------------------------------------------
def _check_big(hyps, lm, lead):
    """hyps: (y, score, fused) best first; lead: what y lacks of the automaton's y_star (the blank, for CTC)"""
    ends = set()
    for y, s, f in hyps:
        total, final, state = lm.score(lead + y)
        assert f == (s + total) + final, (y, f, s, total, final)                # bitwise against the host scorer
        ends.add(state)
    assert [f for *_, f in hyps] == sorted((f for *_, f in hyps), reverse=True)
    assert ends - {0, lm.root}, "every hypothesis ends at the root or the start state: no context was ever reached"


def test_a_model_too_large_for_the_dense_form_decodes_with_the_host_scorers_bits():
    T, V, Hp, L, cell, W, S, O, thr, scale = NK.BIG
    ora, tn, pn = K.model(V, Hp, L, cell, O, 0, scale)
    x = K.audio(T, 0)
    net = _jointnet(tn, pn, V, ora)
    plain = net.recognize_beams_sync(x.cuda(), [T], 0, W, S, token_min_logp=thr)
    lm = NK.big_lm(V, [y[1:] for y in plain])
    assert lm.n_states > 65536
    with pytest.raises(ValueError, match="2\\^27"):
        lm.to_dense()
    got = net.recognize_beams_sync(x.cuda(), [T], 0, W, S, token_min_logp=thr, fusion=lm.to("cuda"), return_scores=True)
    assert len(got) == W
    _check_big(got, lm, [])


def test_the_large_model_through_the_ctc_search():
    from rnntransducer_amd.ops import ctc_beam_search
    T, V, W, thr = 12, NK.BIG[1], 16, -5.0
    z = (3.0 * np.random.default_rng(1000).standard_normal((T, V))).astype(np.float32)
    zb, tl = CK.batch_of([z], T, V)
    plain = ctc_beam_search(zb.cuda(), tl.cuda(), 0, W, token_min_logp=thr)[0]
    lm = NK.big_lm(V, [y for y, _ in plain])
    with pytest.raises(ValueError, match="2\\^27"):
        lm.to_dense()
    got = ctc_beam_search(zb.cuda(), tl.cuda(), 0, W, token_min_logp=thr, fusion=lm.to("cuda"))[0]
    assert len(got) == W
    _check_big(got, lm, [0])


# ---- guards ---------------------------------------------------------------------------------------------------------------------
def test_guards_before_any_launch():
    ora, tn, pn = K.model(NK.V, NK.HP, 1, "lstm", 8, 0)
    net = _jointnet(tn, pn, NK.V, ora)
    x = K.audio(4, 0).cuda()
    lm = NK.random_lm(NK.V, 0)
    for call in (lambda: net.recognize_beams(x, [4], 0, 4, fusion=lm.to("cuda")),
                 lambda: net.init_beam_stream(1, 0, 4, fusion=lm.to("cuda"))):
        with pytest.raises(ValueError, match="recognize_beams_sync.*recognize_ctc_beams"):
            call()
    with pytest.raises(ValueError, match="over 13 tokens"):
        net.recognize_beams_sync(x, [4], 0, 4, fusion=NK.random_lm(NK.V + 1, 0).to("cuda"))
    with pytest.raises(ValueError, match="tables are on cpu"):
        net.recognize_beams_sync(x, [4], 0, 4, fusion=lm)
    with pytest.raises(ValueError, match="tables are on cpu"):
        net.init_beam_sync_stream(1, 0, 4, fusion=lm)
