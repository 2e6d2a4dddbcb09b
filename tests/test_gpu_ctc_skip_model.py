"""ctc_skip= of the transducer searches and of mwer_loss at model level (JointNet with aux_ctc=True), on the SMALL and LSTM1
configs of tests/test_gpu_ctc_model.py (redefined here).

The head's blank bias is set so that about half of the valid frames are skipped at p = 0.9: bias[blank] = the median over valid
frames of logsumexp(non-blank logits) - blank logit, plus log(p / (1 - p)); the median frame's blank posterior is then p.

A search with ctc_skip=p must equal, bit for bit, the same ops search on an encoder output compacted by torch indexing with the
device's own keep mask, its frames mapped through the kept indices: tokens, fp64 scores and frames."""
import math
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
P = 0.9
LSTM1 = (dict(input_size=80, hidden_size=128, output_size=128, num_layers=1, dropout=0.0, bidirectional=True),
         dict(embedding_size=72, pad_token_id=0, hidden_size=128, output_size=128, num_layers=1, dropout=0.0), 72)
SMALL = (dict(input_size=12, hidden_size=16, output_size=8, num_layers=2, rnn_type="gru", dropout=0.0, bidirectional=True),
         dict(embedding_size=10, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, dropout=0.0), 10)
CONFIGS = {"small": SMALL, "lstm1": LSTM1}
B, T, U = 3, 40, 6
_CASES = {}


def _fusion(V, on):
    from rnntransducer_amd import TokenFusion
    return TokenFusion.from_hotwords([[3, 5], [7]], 0.3, V, 0).to("cuda") if on else None


def _case(name):
    """Per config, built once and left unchanged: the eval() model with the calibrated head, the batch on the device, the encoder
    output, the device's keep decision at P, and the compacted operands made from it by torch indexing."""
    if name in _CASES:
        return _CASES[name]
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd.data import synthetic_batch
    from rnntransducer_amd.ops import ctc_frame_skip
    tn, pn, V = CONFIGS[name]
    torch.manual_seed(7)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100, ctc_weight=0.3)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V, aux_ctc=True), args).cuda().eval()
    jn = model.jointnet
    batch = synthetic_batch(B, T, U, V, n_mels=tn["input_size"], ragged=True, seed=11, device="cuda")
    audios, t_lens = batch[0], batch[2]
    valid = torch.arange(T, device="cuda")[None, :] < t_lens[:, None]                     # (B, T)
    with torch.no_grad():
        jn.ctc_head.bias[0] = 0.0
        enc = jn.encoder.forward_time_major(audios, t_lens)                               # (T, B, O)
        z = jn.ctc_head(enc).double().transpose(0, 1)                                     # (B, T, V)
        gap = (torch.logsumexp(z[..., 1:], -1) - z[..., 0])[valid]
        jn.ctc_head.bias[0] = float(gap.median()) + math.log(P / (1 - P))
        sk = ctc_frame_skip(jn.ctc_head(enc), t_lens, 0, P, enc, return_blank_logp=True)
    keep = valid & ~(sk.blank_logp > torch.tensor(math.log(P), dtype=torch.float32))      # the device's own decision
    share = 1.0 - keep.sum().item() / valid.sum().item()
    print(f"{name}: {valid.sum().item()} valid frames, skipped share at p = {P}: {share:.3f}")
    assert 0.25 <= share <= 0.75
    kept = [torch.nonzero(keep[b]).flatten() for b in range(B)]
    enc_c = torch.zeros_like(enc)
    for b in range(B):
        enc_c[:len(kept[b]), b] = enc[kept[b], b]
    lens_c = torch.tensor([len(k) for k in kept], dtype=torch.int32, device="cuda")
    assert torch.equal(lens_c, sk.t_lens)
    _CASES[name] = dict(model=model, jn=jn, batch=batch, V=V, enc=enc, enc_c=enc_c, lens_c=lens_c, kept=[k.tolist() for k in kept])
    return _CASES[name]


def _weights(jn):
    dec = jn.decoder
    return (jn.fc.weight, jn.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight, dec.out_proj.bias)


def _orig(frames, kept_b):
    return [f if f < 0 else kept_b[f] for f in frames]


def _kept_only(frames, kept_b):
    return all(f == -1 or f in kept_b for f in frames)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_greedy_with_skipping_is_the_search_on_the_compacted_frames(name):
    from rnntransducer_amd.ops import greedy_decode
    c = _case(name)
    jn, (audios, t_lens) = c["jn"], (c["batch"][0], c["batch"][2])
    tokens, ntok, frames, logp = greedy_decode(c["enc_c"], *_weights(jn), 0, 3, c["lens_c"], timing=True)
    n = ntok.tolist()
    got = jn.recognize_greedy(audios, t_lens, 0, 3, return_timing=True, ctc_skip=P)
    plain_tokens = jn.recognize_greedy(audios, t_lens, 0, 3, ctc_skip=P)
    assert sum(n) > 0
    for b in range(B):
        assert torch.equal(got[b].tokens, tokens[b, :n[b]]) and torch.equal(plain_tokens[b], tokens[b, :n[b]])
        assert got[b].frames.tolist() == _orig(frames[b, :n[b]].tolist(), c["kept"][b])
        assert torch.equal(got[b].logp.view(torch.int32), logp[b, :n[b]].view(torch.int32))
        assert _kept_only(got[b].frames.tolist(), c["kept"][b]) and got[b].frames.dtype == torch.int32
    # p = 1 skips nothing, None is the plain call
    plain = jn.recognize_greedy(audios, t_lens, 0, 3, return_timing=True)
    for other in (jn.recognize_greedy(audios, t_lens, 0, 3, return_timing=True, ctc_skip=1.0),
                  jn.recognize_greedy(audios, t_lens, 0, 3, return_timing=True, ctc_skip=None)):
        for b in range(B):
            assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                       for x, y in zip(other[b], plain[b]))


def _same_lists(got, want):
    """Search results as nested lists of (y, frames, score[, fused]) tuples: equal, the fp64 scores bit for bit."""
    assert len(got) == len(want)
    for hg, hw in zip(got, want):
        assert len(hg) == len(hw)
        for eg, ew in zip(hg, hw):
            assert eg[0] == ew[0] and eg[1] == ew[1]
            assert [float(s).hex() for s in eg[2:]] == [float(s).hex() for s in ew[2:]]


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fusion"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_beams_with_skipping_is_the_search_on_the_compacted_frames(name, fused):
    from rnntransducer_amd.ops import beam_search
    c = _case(name)
    jn, (audios, t_lens) = c["jn"], (c["batch"][0], c["batch"][2])
    fusion = _fusion(c["V"], fused)
    res = beam_search(c["enc_c"], *_weights(jn), 0, 4, False, 4.6, 2.3, c["lens_c"], frames=True, fusion=fusion)
    want = [[(e[0], _orig(e[-1], c["kept"][b]), *e[1:-1]) for e in hyps] for b, hyps in enumerate(res)]
    kw = dict(beam_widths=4, return_scores=True, return_frames=True, fusion=fusion)
    got = jn.recognize_beams(audios, t_lens, 0, ctc_skip=P, **kw)
    _same_lists(got, want)
    assert all(len(h) > 0 for h in got) and any(len(e[0]) > 1 for h in got for e in h)
    for b, hyps in enumerate(got):
        assert all(_kept_only(e[1], c["kept"][b]) for e in hyps)
    plain = jn.recognize_beams(audios, t_lens, 0, **kw)
    _same_lists(jn.recognize_beams(audios, t_lens, 0, ctc_skip=1.0, **kw), plain)
    _same_lists(jn.recognize_beams(audios, t_lens, 0, ctc_skip=None, **kw), plain)
    # without return_frames nothing is mapped and the token lists are the same
    assert jn.recognize_beams(audios, t_lens, 0, beam_widths=4, fusion=fusion, ctc_skip=P) == [[e[0] for e in h] for h in want]


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fusion"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_beams_sync_with_skipping_is_the_search_on_the_compacted_frames(name, fused):
    from rnntransducer_amd.ops import beam_search_sync
    c = _case(name)
    jn, (audios, t_lens) = c["jn"], (c["batch"][0], c["batch"][2])
    fusion = _fusion(c["V"], fused)
    res = beam_search_sync(c["enc_c"], *_weights(jn), 0, 4, 2, c["lens_c"], frames=True, fusion=fusion)
    want = [[(e[0], _orig(e[-1], c["kept"][b]), *e[1:-1]) for e in hyps] for b, hyps in enumerate(res)]
    kw = dict(beam_widths=4, max_symbols=2, return_scores=True, return_frames=True, fusion=fusion)
    got = jn.recognize_beams_sync(audios, t_lens, 0, ctc_skip=P, **kw)
    _same_lists(got, want)
    assert all(len(h) > 0 for h in got) and any(len(e[0]) > 1 for h in got for e in h)
    for b, hyps in enumerate(got):
        assert all(_kept_only(e[1], c["kept"][b]) for e in hyps)
    plain = jn.recognize_beams_sync(audios, t_lens, 0, **kw)
    _same_lists(jn.recognize_beams_sync(audios, t_lens, 0, ctc_skip=1.0, **kw), plain)
    _same_lists(jn.recognize_beams_sync(audios, t_lens, 0, ctc_skip=None, **kw), plain)
    _same_lists(c["model"].recognize_beams_sync(audios, t_lens, ctc_skip=P, **kw), want)   # the RNNTransducer wrapper


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mwer_with_skipping_keeps_the_reference_term_and_finite_gradients(name):
    c = _case(name)
    model, jn, batch = c["model"], c["jn"], c["batch"]
    jn.train()
    try:
        kw = dict(nbest=4, max_symbols=2, mwer_weight=0.5, reduction="mean", audio_lengths=batch[1], ctc_weight=0.3, return_parts=True)
        plain = jn.mwer_loss(batch[0], batch[2], batch[3], batch[5], batch[6], 0, **kw)
        model.zero_grad()
        parts = jn.mwer_loss(batch[0], batch[2], batch[3], batch[5], batch[6], 0, ctc_skip=P, **kw)
        assert len(parts) == 5 and all(torch.isfinite(x).all() for x in parts)
        assert torch.equal(parts[1].view(torch.int32), plain[1].view(torch.int32))       # rnnt: all frames, untouched
        assert torch.equal(parts[2].view(torch.int32), plain[2].view(torch.int32))       # and so is the CTC term
        parts[0].backward()
        for pname, p in jn.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), pname
        same = jn.mwer_loss(batch[0], batch[2], batch[3], batch[5], batch[6], 0, ctc_skip=1.0, **kw)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(same, plain))
    finally:
        jn.eval()
        model.zero_grad()


def test_validation_step_uses_val_ctc_skip():
    c = _case("small")
    model, batch = c["model"], c["batch"]
    want = c["jn"].recognize_greedy(batch[0], batch[2], 0, 3, ctc_skip=P)
    assert model.val_ctc_skip is None
    model.val_ctc_skip = P
    try:
        out = model.validation_step(batch, 0)
    finally:
        model.val_ctc_skip = None
    assert all(torch.equal(a, b) for a, b in zip(out["pred_tokens"], want))
