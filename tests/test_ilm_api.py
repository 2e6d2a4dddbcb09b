"""CPU-side checks of the internal-LM subtraction's surface: the ilm_weight guards run before anything needs a device, the new
entries refuse bad arguments on the host, and the searches that cannot take the term name the two that can."""
import ctypes as C
import inspect

import pytest
import torch


def _net(aux_ctc=False):
    from rnntransducer_amd.networks import JointNet
    tn = dict(input_size=6, hidden_size=8, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=False)
    pn = dict(embedding_size=5, pad_token_id=0, hidden_size=12, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)
    return JointNet(tn, pn, 5, aux_ctc=aux_ctc).eval()


def test_ilm_weight_defaults_to_off_everywhere_it_is_taken():
    from rnntransducer_amd import ops
    from rnntransducer_amd.networks import JointNet
    from rnntransducer_amd.streaming import BeamSyncStreamState
    for fn in (ops.beam_search_sync, ops.beam_search_sync_device, JointNet.recognize_beams_sync, JointNet.init_beam_sync_stream,
               BeamSyncStreamState.__init__):
        assert inspect.signature(fn).parameters["ilm_weight"].default == 0.0, fn.__qualname__


def test_bad_weights_raise_before_anything_runs():
    net, x = _net(), torch.zeros(1, 4, 6)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "0.3", None, True, [0.3]):
        with pytest.raises(ValueError, match="ilm_weight"):
            net.recognize_beams_sync(x, [4], 0, 4, 2, ilm_weight=bad)
        with pytest.raises(ValueError, match="ilm_weight"):
            net.init_beam_sync_stream(1, 0, 4, 2, ilm_weight=bad)


def test_the_other_searches_name_the_two_that_take_it():
    net, x = _net(aux_ctc=True), torch.zeros(1, 4, 6)
    for call in (lambda: net.recognize_beams(x, [4], 0, 4, ilm_weight=0.3),
                 lambda: net.init_beam_stream(1, 0, 4, ilm_weight=0.3),
                 lambda: net.recognize_ctc_beams(x, [4], 0, 4, ilm_weight=0.3)):
        with pytest.raises(ValueError, match="recognize_beams_sync.*init_beam_sync_stream"):
            call()


def test_c_entries_check_the_ilm_struct_on_the_host():
    """NULL descriptors never reach a dereference: the ilm struct and the fusion / lm pair are checked first."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P = 0x10000                                                        # a stand-in for a device pointer, never dereferenced
    fs, ng = _lib.BeamFusion(), _lib.BeamNgram()
    good = _lib.BeamIlm(P, 0.3)
    for entry in (L.rnnt_hip_beam_sync_search_ilm, L.rnnt_hip_beam_sync_stream_chunk_ilm):
        assert entry(None, C.byref(fs), None, None, None, None) == -1 and b"null ilm" in L.rnnt_hip_last_error()
        assert entry(None, C.byref(fs), None, C.byref(_lib.BeamIlm(None, 0.3)), None, None) == -1 and b"bias" in L.rnnt_hip_last_error()
        for w in (0.0, -1.0, float("nan"), float("inf")):
            assert entry(None, C.byref(fs), None, C.byref(_lib.BeamIlm(P, w)), None, None) == -1
            assert b"weight" in L.rnnt_hip_last_error()
        assert entry(None, C.byref(fs), C.byref(ng), C.byref(good), None, None) == -1 and b"both" in L.rnnt_hip_last_error()
        assert entry(None, None, None, C.byref(good), None, None) == -1 and b"neither" in L.rnnt_hip_last_error()
        assert entry(None, C.byref(fs), None, C.byref(good), None, None) == -1 and b"null descriptor" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_beam_sync_ilm_workspace_bytes(None) == 0 and L.rnnt_hip_beam_sync_stream_ilm_workspace_bytes(None) == 0
    assert L.rnnt_hip_beam_sync_stream_reset_ilm(None, None, 0, 0, None) == -1


def test_workspace_queries_add_the_pairs():
    """The ILM queries ask for the extended entry's bytes plus 2 floats per state slot, rounded up to 256; the existing queries
    are what they were."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    d = _lib.BeamSyncDesc()
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank, d.beam, d.max_symbols = 7, 3, 5, 12, 8, 1, 0, 0, 4, 2
    d.token_min_logp = -float("inf")
    plain, ilm = L.rnnt_hip_beam_sync_workspace_bytes(C.byref(d)), L.rnnt_hip_beam_sync_ilm_workspace_bytes(C.byref(d))
    assert plain > 0 and ilm - plain == (3 * (2 + 2) * 4 * 2 * 4 + 255) // 256 * 256
    s = _lib.BeamSyncStreamDesc()
    s.T, s.B, s.V, s.Hp, s.O, s.L, s.cell, s.blank, s.beam, s.max_symbols = 0, 3, 5, 12, 8, 1, 0, 0, 4, 2
    s.token_min_logp, s.max_nodes, s.max_len = -float("inf"), 64, 16
    plain = L.rnnt_hip_beam_sync_stream_workspace_bytes(C.byref(s))
    ilm = L.rnnt_hip_beam_sync_stream_ilm_workspace_bytes(C.byref(s))
    assert plain > 0 and ilm - plain == 3 * (((2 + 2) * 4 * 2 * 4 + 255) // 256 * 256)
