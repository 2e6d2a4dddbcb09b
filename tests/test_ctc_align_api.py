"""CPU-side checks of the CTC forced alignment's surface (csrc/ctc.hip: rnnt_hip_ctc_align): the C ABI's argument validation, which
happens on the host before any launch (the pointers below are stand-ins that are never dereferenced), the workspace query, and the
`args.ar_source` rules of RNNTransducer.  No device work."""
from argparse import Namespace

import pytest
import torch

P, Q, R = 0x10000, 0x20000, 0x30000   # stand-ins for device pointers

ENTRIES = ("rnnt_hip_ctc_align_workspace_bytes", "rnnt_hip_ctc_align")
CFG = (dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=2), dict(input_size=12, hidden_size=8, output_size=12, num_layers=2))


def _model(aux=True, **args):
    from rnntransducer_amd import RNNTransducer
    a = dict(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    a.update(args)
    torch.manual_seed(0)
    return RNNTransducer(*CFG, dict(num_classes=10, aux_ctc=True) if aux else dict(num_classes=10), Namespace(**a))


def test_entries_are_declared_and_exported():
    import os
    from rnntransducer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnnt_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name + "(" in header and hasattr(L, name)
    assert L.rnnt_hip_version() == 4 and _lib.ABI_VERSION == 4


def test_workspace_query():
    from rnntransducer_amd import _lib, ops
    q = _lib.lib().rnnt_hip_ctc_align_workspace_bytes
    assert q(0, 1, 1, 2) == 0 and q(1, 0, 1, 2) == 0 and q(1, 1, 1, 0) == 0 and q(1, 1, -1, 2) == 0
    assert q(2, 10, 3, 5) > 0 and q(2, 10, 0, 5) > 0
    assert q(2, 100, 40, 5) > q(2, 100, 39, 5) and q(2, 200, 40, 5) > q(2, 100, 40, 5)
    # the header's formula: emission rows, lse, chains, three bit planes of 32-frame words, the end states; each rounded up to 256
    r = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for B, T, U in ((2, 10, 3), (32, 1000, 40), (3, 70, 511), (1, 33, 0)):
        want = r(4 * B * (U + 1) * T) + r(4 * B * T) + r(4 * B * (U + 1)) + r(12 * B * (U + 1) * ((T + 31) // 32)) + r(4 * B)
        assert q(B, T, U, 7) == want == ops.ctc_align_workspace_bytes(B, T, U, 7)
        assert 12 * B * (U + 1) * ((T + 31) // 32) <= B * (U + 1) * T + 12 * B * (U + 1)   # at most a byte per (frame, position)
    with pytest.raises(ValueError):
        ops.ctc_align_workspace_bytes(0, 1, 1, 2)


def test_arguments_are_refused_before_any_launch():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    B, T, U, V = 2, 10, 3, 5
    need = L.rnnt_hip_ctc_align_workspace_bytes(B, T, U, V)

    def call(logits=P, labels=Q, t_lens=Q, u_lens=Q, U=U, V=V, blank=0, first=R, last=R, path=R, tlp=R, score=R, ws=R, nws=need,
             z_sb=T * V, z_st=V, T=T):
        return L.rnnt_hip_ctc_align(logits, z_sb, z_st, labels, t_lens, u_lens, B, T, U, V, blank, first, last, path, tlp, score, ws,
                                    nws, None)

    err = L.rnnt_hip_last_error
    assert call(logits=None) == -1 and b"null" in err()
    assert call(labels=None) == -1 and b"null" in err()
    assert call(t_lens=None) == -1 and call(u_lens=None) == -1
    assert call(score=None) == -1 and b"null" in err()
    assert call(first=None) == -1 and b"null" in err()
    assert call(last=None) == -1 and b"null" in err()
    assert call(ws=None) == -1 and b"workspace" in err()
    assert call(blank=-1) == -1 and b"blank" in err()
    assert call(blank=V) == -1 and b"blank" in err()
    assert call(U=512, nws=1 << 40) == -1 and b"511" in err()
    assert call(z_st=V - 1) == -1 and b"stride" in err()
    assert call(nws=need - 1) == -1 and b"workspace too small" in err()
    # path / token_logp NULL are accepted: with them the call gets past every check (it is stopped by the short workspace here)
    assert call(path=None, tlp=None, nws=need - 1) == -1 and b"workspace too small" in err()
    assert call(U=0, labels=None, first=None, last=None, tlp=None, nws=0) == -1 and b"workspace too small" in err()


def test_python_surface():
    from rnntransducer_amd import ops
    from rnntransducer_amd._lib import RnntHipError
    assert ops.CtcAlignment._fields == ("first", "last", "score", "path", "token_logp")
    assert ops.CtcEmitWindows(2, 3).left == 2 and ops.CtcEmitWindows(2, 3).right == 3
    for bad in ((-1, 0), (0, -1), (1.5, 0), (True, 0)):
        with pytest.raises(ValueError):
            ops.check_ctc_emit_windows(ops.CtcEmitWindows(*bad))
    z, y = torch.zeros(2, 5, 10), torch.ones(2, 2, dtype=torch.int32)
    tl, ul = torch.tensor([5, 4], dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    with pytest.raises(RnntHipError):   # no CPU / eager fallback
        ops.ctc_align(z, y, tl, ul, 0)
    plain = _model(aux=False)
    x = torch.zeros(2, 5, 12)
    with pytest.raises(ValueError):
        plain.jointnet.ctc_align(x, tl, y, ul, 0)
    with pytest.raises(ValueError):
        plain.jointnet.loss(x, tl, torch.zeros(2, 3, dtype=torch.long), y, ul, 0, emit_windows=ops.CtcEmitWindows(1, 1))
    with pytest.raises(ValueError):
        _model().jointnet.loss(x, tl, torch.zeros(2, 3, dtype=torch.long), y, ul, 0, emit_windows=ops.CtcEmitWindows(-1, 1))


def test_ar_source_is_validated_at_construction():
    assert _model().ar_source == "frames" and _model(ar_left=1, ar_right=2).ar_source == "frames"
    assert _model(ar_source=None).ar_source == "frames"
    m = _model(ar_source="ctc", ar_left=1, ar_right=2)
    assert m.ar_source == "ctc" and (m.ar_left, m.ar_right) == (1, 2)
    with pytest.raises(ValueError):
        _model(ar_source="viterbi", ar_left=1, ar_right=2)
    with pytest.raises(ValueError):
        _model(ar_source="ctc")                                  # no ar_left / ar_right
    with pytest.raises(ValueError):
        _model(aux=False, ar_source="ctc", ar_left=1, ar_right=2)   # no CTC head
    with pytest.raises(ValueError):
        _model(ar_source="ctc", ar_left=1, ar_right=2, kd_weight=0.5)   # the refusal of windows next to a teacher holds
    m = _model(ar_source="ctc", ar_left=1, ar_right=2, mwer_weight=0.5)
    with pytest.raises(ValueError):   # ... and next to MWER, as with a frame table
        m.training_step((torch.zeros(2, 5, 12), [5, 4], torch.tensor([5, 4], dtype=torch.int32), torch.zeros(2, 3, dtype=torch.long),
                         [3, 2], torch.ones(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)), 0)
    with pytest.raises(ValueError):   # the 7-element batch
        _model(ar_source="ctc", ar_left=1, ar_right=2).training_step((0,) * 8, 0)
