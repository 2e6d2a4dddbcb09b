"""The CTC forced alignment at model level, on tiny models: JointNet.ctc_align / RNNTransducer.ctc_align, the emission windows
from the CTC head (loss(emit_windows=ops.CtcEmitWindows(l, r))) and args.ar_source = "ctc".  The kernel itself is checked against
float64 in tests/test_gpu_ctc_align.py; here every statement is an exact one between two ways of asking for the same thing."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu

V, LEFT, RIGHT = 10, 1, 2
TN = dict(input_size=12, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
PN = dict(embedding_size=V, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)


def _model(aux=True, **knobs):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(0)
    jp = dict(num_classes=V, aux_ctc=True) if aux else dict(num_classes=V)
    return RNNTransducer(dict(PN), dict(TN), jp, Namespace(move_metrics_to_cpu=False, **knobs)).cuda().train()


@pytest.fixture(scope="module")
def dev():
    """A ragged batch with the python length list, rows NOT in length order (the ragged sort moves rows)."""
    from oracle.rnnt_oracle import make_batch
    batch = make_batch(4, 24, 5, V, n_mels=12, ragged=True, seed=3)
    batch = tuple(x.flip(0) if isinstance(x, torch.Tensor) else x[::-1] for x in batch)
    assert sorted(batch[1], reverse=True) != batch[1] and len(set(batch[1])) > 1
    return tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)


def _loss(m, dev, **kw):
    return m.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1], **kw)


def _step_grads(m, loss):
    loss.backward()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_ctc_align_rows_in_the_callers_order(dev):
    m = _model()
    j = m.jointnet
    a = j.ctc_align(dev[0], dev[2], dev[5], dev[6], 0, audio_lengths=dev[1], return_path=True, return_token_logp=True)
    b = j.ctc_align(dev[0], dev[2], dev[5], dev[6], 0, return_path=True, return_token_logp=True)
    c = m.ctc_align(dev, return_path=True, return_token_logp=True)
    for name, x, y, z in zip(a._fields, a, b, c):
        assert torch.equal(x, z), name   # the same call
        if x.dtype == torch.int32:
            assert torch.equal(x, y), name
        else:   # (the ragged plan may change the encoder's last bits)
            assert torch.allclose(x, y, rtol=1e-5, atol=1e-6), name
    t, u = dev[2].tolist(), dev[6].tolist()
    assert torch.isfinite(a.score).all()
    for r in range(4):
        f, l = a.first[r, :u[r]].tolist(), a.last[r, :u[r]].tolist()
        assert all(0 <= x <= y < t[r] for x, y in zip(f, l)) and all(l[k] < f[k + 1] for k in range(u[r] - 1))
        assert (a.first[r, u[r]:] == -1).all() and (a.path[r, t[r]:] == -1).all() and (a.path[r, :t[r]] >= 0).all()
        alone = j.ctc_align(dev[0][r:r + 1], dev[2][r:r + 1], dev[5][r:r + 1], dev[6][r:r + 1], 0, audio_lengths=[t[r]])
        assert alone.first[0, :u[r]].tolist() == f and alone.last[0, :u[r]].tolist() == l   # the row's own answer, wherever it sits
    plain = j.ctc_align(dev[0], dev[2], dev[5], dev[6], 0)
    assert plain.path is None and plain.token_logp is None and torch.equal(plain.first, a.first)


def test_a_model_without_the_head_is_refused(dev):
    from rnntransducer_amd.ops import CtcEmitWindows
    m = _model(aux=False)
    with pytest.raises(ValueError, match="aux_ctc"):
        m.jointnet.ctc_align(dev[0], dev[2], dev[5], dev[6], 0)
    with pytest.raises(ValueError, match="aux_ctc"):
        m.ctc_align(dev)
    with pytest.raises(ValueError, match="aux_ctc"):
        _loss(m, dev, emit_windows=CtcEmitWindows(LEFT, RIGHT))


@pytest.mark.parametrize("ctc_weight", [0.0, 0.3])
def test_windows_from_the_head_equal_windows_from_a_separate_alignment(dev, ctc_weight):
    from rnntransducer_amd.ops import CtcEmitWindows

    def run(own):
        m = _model()
        if own:
            win = CtcEmitWindows(LEFT, RIGHT)
        else:
            al = m.jointnet.ctc_align(dev[0], dev[2], dev[5], dev[6], 0, audio_lengths=dev[1])
            win = (al.first - LEFT, al.last + RIGHT)
        parts = _loss(m, dev, reduction="mean", emit_windows=win, ctc_weight=ctc_weight, return_parts=True)
        return [p.detach().clone() for p in parts], _step_grads(m, parts[0])

    (pa, ga), (pb, gb) = run(True), run(False)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb)) and torch.isfinite(pa[0])   # finite on random untrained weights
    assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    # the CTC part is the one without windows, and the windows restrict the transducer part
    m = _model()
    plain = _loss(m, dev, reduction="mean", ctc_weight=ctc_weight, return_parts=True)
    assert torch.equal(plain[2], pa[2]) and pa[1] >= plain[1]
    with torch.no_grad():
        rows = _loss(_model(), dev, reduction="none", emit_windows=CtcEmitWindows(LEFT, RIGHT))
    assert torch.isfinite(rows).all()


def test_windows_wider_than_the_utterance_are_the_plain_loss(dev):
    from rnntransducer_amd.ops import CtcEmitWindows
    T = dev[0].size(1)

    def run(win):
        m = _model()
        loss = _loss(m, dev, reduction="mean", emit_windows=win)
        return loss.detach().clone(), _step_grads(m, loss)

    (la, ga), (lb, gb) = run(CtcEmitWindows(T, T)), run(None)
    assert torch.equal(la, lb)
    assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)


@pytest.mark.parametrize("ctc_weight", [0.0, 0.3])
def test_training_step_with_ar_source_ctc(dev, ctc_weight):
    from rnntransducer_amd.ops import CtcEmitWindows
    m = _model(ar_source="ctc", ar_left=LEFT, ar_right=RIGHT, ctc_weight=ctc_weight)
    l_step = m.training_step(dev, 0)["loss"]
    g_step = _step_grads(m, l_step)
    m2 = _model()
    l_loss = _loss(m2, dev, reduction="mean", emit_windows=CtcEmitWindows(LEFT, RIGHT), ctc_weight=ctc_weight)
    g_loss = _step_grads(m2, l_loss)
    assert torch.equal(l_step.detach(), l_loss.detach()) and torch.isfinite(l_step)
    assert set(g_step) == set(g_loss) and all(torch.equal(g_step[k], g_loss[k]) for k in g_step)
    with pytest.raises(ValueError, match="7-element"):
        m.training_step(dev + (torch.zeros(4, 5, dtype=torch.int32, device="cuda"),), 0)
