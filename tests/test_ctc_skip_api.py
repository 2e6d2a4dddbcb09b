"""CTC frame skipping: every argument error is a ValueError (a negative return with a message at the C entry) before any device
work.  No device here: a call that got as far as a launch would fail differently."""
import ctypes as C
from argparse import Namespace

import pytest
import torch

SMALL = (dict(input_size=12, hidden_size=16, output_size=8, num_layers=2, rnn_type="gru", dropout=0.0, bidirectional=True),
         dict(embedding_size=10, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, dropout=0.0), 10)
BAD_THRESHOLDS = (0.0, -0.1, 1.5, float("nan"), float("inf"), True, "0.9", None)


def _model(aux=True, **args):
    from rnntransducer_amd import RNNTransducer
    tn, pn, V = SMALL
    ns = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100, **args)
    return RNNTransducer(dict(pn), dict(tn), dict(num_classes=V, aux_ctc=True) if aux else dict(num_classes=V), ns)


def _operands():
    return torch.zeros(7, 2, 5), torch.tensor([7, 4], dtype=torch.int32), torch.zeros(7, 2, 8)


@pytest.mark.parametrize("p", BAD_THRESHOLDS, ids=repr)
def test_ops_refuses_a_bad_threshold(p):
    from rnntransducer_amd.ops import ctc_frame_skip
    z, t_lens, enc = _operands()
    with pytest.raises(ValueError, match="threshold"):
        ctc_frame_skip(z, t_lens, 0, p, enc)


def test_ops_refuses_cpu_tensors_dtypes_and_shapes():
    from rnntransducer_amd.ops import ctc_frame_skip
    z, t_lens, enc = _operands()
    with pytest.raises(ValueError, match="CPU tensor"):
        ctc_frame_skip(z, t_lens, 0, 0.9, enc)
    for bad in ((z.double(), t_lens, enc), (z, t_lens.long(), enc), (z, t_lens, enc.half()), (z, t_lens, enc[:6]),
                (z, t_lens[:1], enc), (z, t_lens, enc[:, :, 0]), (z[0], t_lens, enc), (z[:, :, :1], t_lens, enc)):
        with pytest.raises(ValueError):
            ctc_frame_skip(bad[0], bad[1], 0, 0.9, bad[2])
    for blank in (-1, 5, True):
        with pytest.raises(ValueError, match="blank"):
            ctc_frame_skip(z, t_lens, blank, 0.9, enc)
    with pytest.raises(ValueError):   # batch-major logits against time-major enc
        ctc_frame_skip(z, t_lens, 0, 0.9, enc, time_major=False)


def test_log_threshold_is_the_float32_log():
    import math
    import numpy as np
    from rnntransducer_amd.ops import check_ctc_skip
    assert check_ctc_skip(1.0, "x") == 0.0 and check_ctc_skip(1, "x") == 0.0
    assert check_ctc_skip(0.9, "x") == float(np.float32(math.log(0.9)))


def test_searches_refuse_before_the_encoder_runs():
    audios, lens = torch.zeros(2, 9, 12), torch.tensor([9, 5], dtype=torch.int32)   # CPU tensors: nothing below may touch them
    plain, model = _model(aux=False).jointnet.eval(), _model().jointnet.eval()
    for search in ("recognize_greedy", "recognize_beams", "recognize_beams_sync"):
        with pytest.raises(ValueError, match="CTC head"):
            getattr(plain, search)(audios, lens, 0, ctc_skip=0.9)
        for p in BAD_THRESHOLDS[:-1]:   # None is "no skipping"
            with pytest.raises(ValueError, match="threshold"):
                getattr(model, search)(audios, lens, 0, ctc_skip=p)
        with pytest.raises(ValueError, match="blank"):
            getattr(model, search)(audios, lens, 10, ctc_skip=0.9)
    for search in ("recognize_greedy", "recognize_beams"):
        with pytest.raises(ValueError, match="visit_padded_frames"):
            getattr(model, search)(audios, lens, 0, visit_padded_frames=True, ctc_skip=0.9)


def test_mwer_and_the_module_arguments_refuse():
    texts, targets, u = torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    audios, lens = torch.zeros(2, 9, 12), torch.tensor([9, 5], dtype=torch.int32)
    with pytest.raises(ValueError, match="CTC head"):
        _model(aux=False).jointnet.mwer_loss(audios, lens, texts, targets, u, 0, ctc_skip=0.9)
    with pytest.raises(ValueError, match="threshold"):
        _model().jointnet.mwer_loss(audios, lens, texts, targets, u, 0, ctc_skip=1.5)
    for key in ("mwer_ctc_skip", "val_ctc_skip"):
        with pytest.raises(ValueError, match="CTC head"):
            _model(aux=False, **{key: 0.9})
        with pytest.raises(ValueError, match="threshold"):
            _model(**{key: 0.0})
        assert getattr(_model(**{key: 0.9}), key) == 0.9
    m = _model()
    assert m.mwer_ctc_skip is None and m.val_ctc_skip is None


def test_entry_refuses_bad_arguments_on_the_host():
    """rnnt_hip_ctc_frame_skip against the argument sets it must refuse: each returns -1 and leaves a message.  The addresses are
    stand-ins that are never dereferenced; every call in here is a refused one, so nothing reaches a launch."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    B, T, V, O = 2, 40, 5, 8
    P, Q, R = 0x100000, 0x200000, 0x300000
    need = L.rnnt_hip_ctc_frame_skip_workspace_bytes(B, T)
    assert need >= 4 * B * 2 and L.rnnt_hip_ctc_frame_skip_workspace_bytes(0, T) == 0 == L.rnnt_hip_ctc_frame_skip_workspace_bytes(B, 0)
    assert L.rnnt_hip_ctc_frame_skip_workspace_bytes(1, 2081) >= 4 * 66
    good = dict(logits=P, z_sb=T * V, z_st=V, t_lens=P, B=B, T=T, V=V, blank=0, log_threshold=-0.1, enc=P, e_sb=O, e_st=B * O, O=O,
                enc_out=Q, o_sb=O, o_st=B * O, new_lens=R, frame_map=R, blank_logp=None, workspace=R, workspace_bytes=need,
                stream=None)
    refused = [dict(V=1), dict(V=0), dict(blank=-1), dict(blank=V), dict(enc_out=P), dict(enc_out=P + 4 * O),
               dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=None), dict(log_threshold=float("nan")),
               dict(log_threshold=0.5), dict(log_threshold=float("inf")), dict(B=0), dict(T=0), dict(O=0), dict(B=70000),
               dict(z_st=V - 1), dict(e_st=O - 1), dict(o_st=O - 1), dict(z_sb=0), dict(logits=None), dict(t_lens=None),
               dict(enc=None), dict(enc_out=None), dict(new_lens=None), dict(frame_map=None)]
    for over in refused:
        args = {**good, **over}
        rc = L.rnnt_hip_ctc_frame_skip(*(args[k] for k in good))
        assert rc == -1, f"{over}: returned {rc}"
        assert L.rnnt_hip_last_error(), f"{over}: no message"
    assert C.sizeof(C.c_void_p) == 8
