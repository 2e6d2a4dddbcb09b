"""CPU-side checks of the searches' host path: one table of (call, exception type, regex) over every guard of the search surface
that is reachable without a device.  Models and tensors live on the CPU, so a call that got past its guards would end in the
"CPU tensor" RnntHipError (or try to allocate on a device); each row therefore also shows that its guard fires before anything
needs one.  The last rows are that RnntHipError itself, behind valid arguments: the guards of ops.beam_search_sync all run first."""
import math

import pytest
import torch

V = 7


def _net(aux_ctc=False, bidirectional=False):
    from rnntransducer_amd.networks import JointNet
    tn = dict(input_size=6, hidden_size=8, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=bidirectional)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=12, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)
    return JointNet(tn, pn, V, aux_ctc=aux_ctc).eval()


def _fusion(n):
    from rnntransducer_amd.fusion import TokenFusion
    return TokenFusion(torch.zeros(1, n, dtype=torch.int32), torch.zeros(1, n), torch.zeros(1))


def _sync(**over):
    """ops.beam_search_sync on CPU operands of a fitting model (T=4, B=2, Oe=Od=8, Hp=12, one LSTM layer), `over` replacing some."""
    from rnntransducer_amd import ops
    a = dict(enc_tm=torch.zeros(4, 2, 8), fc_w=torch.zeros(V, 16), fc_b=torch.zeros(V), emb_w=torch.zeros(V, 12),
             rnn_weights=[torch.zeros(48, 12), torch.zeros(48, 12), torch.zeros(48), torch.zeros(48)], cell=0,
             out_w=torch.zeros(8, 12), out_b=torch.zeros(8), blank=0, beam_width=4, max_symbols=1,
             t_lens=torch.tensor([4, 3], dtype=torch.int32))
    kw = {k: over.pop(k) for k in list(over) if k not in a}
    return ops.beam_search_sync(*{**a, **over}.values(), **kw)


X, LENS = torch.zeros(2, 4, 6), [4, 3]   # CPU audio: nothing below may touch it
PLAIN, CTC = _net(), _net(aux_ctc=True)

ROWS = [
    # ops.beam_search_sync: widths, max_symbols, token_min_logp, step_group, blank, t_lens, shapes; then the device
    ("sync beam 0", lambda: _sync(beam_width=0), ValueError, "beam width"),
    ("sync beam 65", lambda: _sync(beam_width=65), ValueError, "beam width"),
    ("sync beam bool", lambda: _sync(beam_width=True), ValueError, "beam width"),
    ("sync max_symbols 0", lambda: _sync(max_symbols=0), ValueError, "max_symbols"),
    ("sync max_symbols 5", lambda: _sync(max_symbols=5), ValueError, "max_symbols"),
    ("sync logp nan", lambda: _sync(token_min_logp=math.nan), ValueError, "token_min_logp"),
    ("sync logp inf", lambda: _sync(token_min_logp=math.inf), ValueError, "token_min_logp"),
    ("sync logp str", lambda: _sync(token_min_logp="x"), ValueError, "token_min_logp"),
    ("sync ilm_weight", lambda: _sync(ilm_weight=-0.5), ValueError, "ilm_weight"),
    ("sync step_group -1", lambda: _sync(step_group=-1), ValueError, "step_group.*-1"),
    ("sync step_group bool", lambda: _sync(step_group=True), ValueError, "step_group.*True"),
    ("sync step_group float", lambda: _sync(step_group=1.5), ValueError, "step_group.*1.5"),
    ("sync enc 2-D", lambda: _sync(enc_tm=torch.zeros(4, 8)), ValueError, r"\(T,B,Oe\)"),
    ("sync V 1", lambda: _sync(fc_w=torch.zeros(1, 16), fc_b=torch.zeros(1)), ValueError, "V = 1 < 2"),
    ("sync T 0", lambda: _sync(enc_tm=torch.zeros(0, 2, 8)), ValueError, "T=0"),
    ("sync blank -1", lambda: _sync(blank=-1), ValueError, "blank -1 outside"),
    ("sync blank V", lambda: _sync(blank=V), ValueError, f"blank {V} outside"),
    ("sync enc width", lambda: _sync(enc_tm=torch.zeros(4, 2, 9)), ValueError, "do not fit encoder width 9"),
    ("sync fc bias", lambda: _sync(fc_b=torch.zeros(V + 1)), ValueError, "do not fit encoder width"),
    ("sync out_proj", lambda: _sync(out_w=torch.zeros(8, 11)), ValueError, "do not fit together"),
    ("sync rnn weight", lambda: _sync(rnn_weights=[torch.zeros(48, 12)] * 4), ValueError, "weight #2"),
    ("sync fusion type", lambda: _sync(fusion=object()), ValueError, "fusion must be"),
    ("sync fusion vocab", lambda: _sync(fusion=_fusion(5)), ValueError, "over 5 tokens"),
    ("sync t_lens dtype", lambda: _sync(t_lens=torch.tensor([4, 3])), ValueError, "t_lens must be.*int64"),
    ("sync t_lens shape", lambda: _sync(t_lens=torch.tensor([4], dtype=torch.int32)), ValueError, "t_lens must be"),
    ("sync valid: the device", lambda: _sync(), RuntimeError, "CPU tensor"),
    ("sync valid, fused: the device", lambda: _sync(fusion=_fusion(V), ilm_weight=0.3, frames=True), RuntimeError, "CPU tensor"),
    # init_stream
    ("greedy stream batch", lambda: PLAIN.init_stream(0, 0), ValueError, "batch_size must be.*>= 1, got 0"),
    ("greedy stream blank", lambda: PLAIN.init_stream(2, V), ValueError, f"blank_token_id {V} outside"),
    ("greedy stream device", lambda: PLAIN.init_stream(2, 0, device="cuda:0"), ValueError, "init_stream.*cuda:0 is not the model's"),
    ("greedy stream bidirectional", lambda: _net(bidirectional=True).init_stream(2, 0), ValueError, "init_stream.*bidirectional"),
    ("greedy stream training", lambda: _net().train().init_stream(2, 0), RuntimeError, "init_stream expects eval"),
    # init_beam_stream
    ("beam stream batch", lambda: PLAIN.init_beam_stream(0, 0), ValueError, "batch_size must be.*>= 1, got 0"),
    ("beam stream blank", lambda: PLAIN.init_beam_stream(2, -1), ValueError, "blank_token_id -1 outside"),
    ("beam stream device", lambda: PLAIN.init_beam_stream(2, 0, device="cuda:0"), ValueError,
     "init_beam_stream.*cuda:0 is not the model's"),
    ("beam stream unknown cap", lambda: PLAIN.init_beam_stream(2, 0, max_pop=5), TypeError, r"init_beam_stream.*max_pop.*max_pops"),
    ("beam stream cap 0", lambda: PLAIN.init_beam_stream(2, 0, 4, max_pops=0), ValueError, "max_pops must be an integer >= 1, got 0"),
    ("beam stream cap float", lambda: PLAIN.init_beam_stream(2, 0, 4, max_len=8.0), ValueError, "max_len must be an integer"),
    ("beam stream fusion vocab", lambda: PLAIN.init_beam_stream(2, 0, 4, fusion=_fusion(5)), ValueError,
     "init_beam_stream.*over 5 tokens"),
    ("beam stream fusion type", lambda: PLAIN.init_beam_stream(2, 0, 4, fusion=object()), ValueError, "fusion must be"),
    ("beam stream ilm", lambda: PLAIN.init_beam_stream(2, 0, 4, ilm_weight=0.3), ValueError, "init_beam_stream: ilm_weight"),
    ("beam stream training", lambda: _net().train().init_beam_stream(2, 0), RuntimeError, "init_beam_stream expects eval"),
    # init_beam_sync_stream
    ("sync stream batch 0", lambda: PLAIN.init_beam_sync_stream(0, 0), ValueError, "init_beam_sync_stream: batch_size.*got 0"),
    ("sync stream batch float", lambda: PLAIN.init_beam_sync_stream(1.5, 0), ValueError, "batch_size.*got 1.5"),
    ("sync stream batch bool", lambda: PLAIN.init_beam_sync_stream(True, 0), ValueError, "batch_size.*got True"),
    ("sync stream blank", lambda: PLAIN.init_beam_sync_stream(2, V), ValueError, f"init_beam_sync_stream: blank_token_id {V} outside"),
    ("sync stream device", lambda: PLAIN.init_beam_sync_stream(2, 0, device="cuda:0"), ValueError,
     "init_beam_sync_stream.*cuda:0 is not the model's"),
    ("sync stream beam", lambda: PLAIN.init_beam_sync_stream(2, 0, 65), ValueError, "init_beam_sync_stream: beam width"),
    ("sync stream max_symbols", lambda: PLAIN.init_beam_sync_stream(2, 0, 4, 5), ValueError, "max_symbols"),
    ("sync stream max_nodes", lambda: PLAIN.init_beam_sync_stream(2, 0, 4, 2, max_nodes=32), ValueError, "max_nodes = 32 outside"),
    ("sync stream max_len", lambda: PLAIN.init_beam_sync_stream(2, 0, max_len=0), ValueError, "max_len must be an integer >= 1, got 0"),
    ("sync stream unknown cap", lambda: PLAIN.init_beam_sync_stream(2, 0, max_pops=5), TypeError, "max_pops"),
    ("sync stream fusion vocab", lambda: PLAIN.init_beam_sync_stream(2, 0, fusion=_fusion(5)), ValueError,
     "init_beam_sync_stream.*over 5 tokens"),
    ("sync stream ilm", lambda: PLAIN.init_beam_sync_stream(2, 0, ilm_weight=-1.0), ValueError, "init_beam_sync_stream: ilm_weight"),
    ("sync stream training", lambda: _net().train().init_beam_sync_stream(2, 0), ValueError, "init_beam_sync_stream expects eval"),
    # the chunk calls, up to the state's type
    ("greedy chunk training", lambda: _net().train().recognize_greedy_stream(X, LENS, None), RuntimeError, "recognize_greedy_stream expects eval"),
    ("beam chunk training", lambda: _net().train().recognize_beams_stream(X, LENS, None), RuntimeError, "recognize_beams_stream expects eval"),
    ("sync chunk training", lambda: _net().train().recognize_beams_sync_stream(X, LENS, None), ValueError,
     "recognize_beams_sync_stream expects eval"),
    ("sync chunk state", lambda: PLAIN.recognize_beams_sync_stream(X, LENS, object()), ValueError,
     "takes the state of init_beam_sync_stream, got object"),
    # training-mode refusals of the offline searches
    ("greedy training", lambda: _net().train().recognize_greedy(X, LENS, 0), RuntimeError, "recognize_greedy expects eval"),
    ("beams training", lambda: _net().train().recognize_beams(X, LENS, 0, 4), RuntimeError, "recognize_beams expects eval"),
    ("beams_sync training", lambda: _net().train().recognize_beams_sync(X, LENS, 0, 4), ValueError, "recognize_beams_sync expects eval"),
    ("align training", lambda: _net().train().align(X, LENS, None, None, [1, 1], 0), RuntimeError, "align expects eval"),
    # the offline searches' own argument checks
    ("beams lm", lambda: PLAIN.recognize_beams(X, LENS, 0, 4, lm=object()), NotImplementedError, "fusion="),
    ("beams ilm", lambda: PLAIN.recognize_beams(X, LENS, 0, 4, ilm_weight=0.3), ValueError, "recognize_beams: ilm_weight"),
    ("beams fusion vocab", lambda: PLAIN.recognize_beams(X, LENS, 0, 4, fusion=_fusion(5)), ValueError, "recognize_beams: .*over 5 tokens"),
    ("beams_sync beam", lambda: PLAIN.recognize_beams_sync(X, LENS, 0, 65), ValueError, "recognize_beams_sync: beam width"),
    ("beams_sync ilm", lambda: PLAIN.recognize_beams_sync(X, LENS, 0, 4, ilm_weight=math.nan), ValueError, "recognize_beams_sync: ilm_weight"),
    ("beams_sync fusion vocab", lambda: PLAIN.recognize_beams_sync(X, LENS, 0, 4, fusion=_fusion(5)), ValueError, "over 5 tokens"),
    ("beams_sync blank", lambda: PLAIN.recognize_beams_sync(X, LENS, V, 4), ValueError, f"recognize_beams_sync: blank {V} outside"),
    ("mwer nbest", lambda: PLAIN.mwer_loss(X, LENS, None, None, [1, 1], 0, nbest=65), ValueError, "mwer_loss: beam width"),
    ("mwer blank", lambda: PLAIN.mwer_loss(X, LENS, None, None, [1, 1], V), ValueError, f"mwer_loss: blank {V} outside"),
]
# ctc_skip: the head, the threshold, the blank, visit_padded_frames; in every search that takes it
for _name, _call in (("greedy", lambda net, **kw: net.recognize_greedy(X, LENS, kw.pop("blank", 0), **kw)),
                     ("beams", lambda net, **kw: net.recognize_beams(X, LENS, kw.pop("blank", 0), 4, **kw)),
                     ("beams_sync", lambda net, **kw: net.recognize_beams_sync(X, LENS, kw.pop("blank", 0), 4, **kw)),
                     ("mwer", lambda net, **kw: net.mwer_loss(X, LENS, None, None, [1, 1], kw.pop("blank", 0), **kw))):
    ROWS += [(f"{_name} ctc_skip no head", lambda c=_call: c(PLAIN, ctc_skip=0.9), ValueError, "needs the CTC head"),
             (f"{_name} ctc_skip 0", lambda c=_call: c(CTC, ctc_skip=0.0), ValueError, "threshold"),
             (f"{_name} ctc_skip 1.5", lambda c=_call: c(CTC, ctc_skip=1.5), ValueError, "threshold"),
             (f"{_name} ctc_skip bool", lambda c=_call: c(CTC, ctc_skip=True), ValueError, "threshold"),
             (f"{_name} ctc_skip blank", lambda c=_call: c(CTC, ctc_skip=0.9, blank=V), ValueError, f"blank {V}.* outside")]
    if _name in ("greedy", "beams"):
        ROWS.append((f"{_name} ctc_skip padded", lambda c=_call: c(CTC, ctc_skip=0.9, visit_padded_frames=True), ValueError,
                     "visit_padded_frames=True cannot be combined with ctc_skip"))


@pytest.mark.parametrize("call,exc,regex", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_guard_fires_before_anything_needs_a_device(call, exc, regex):
    with pytest.raises(exc, match=regex) as err:
        call()
    from rnntransducer_amd._lib import RnntHipError
    if "CPU tensor" not in regex:   # the guard itself, not the refusal of a CPU tensor behind it
        assert not isinstance(err.value, RnntHipError) and "CPU tensor" not in str(err.value), err.value
