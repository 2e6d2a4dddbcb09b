"""The fused beam-search entries (include/rnnt_hip.h, rnnt_beam_fusion) refuse bad arguments on the host, before any device
work: every call here passes stand-in addresses that are never dereferenced, on a machine that may have no GPU."""
import ctypes as C


P, Q = 0x10000, 0x20000   # 256-byte aligned stand-ins for device pointers


def _fill(d, stream):
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank = (0 if stream else 3), 2, 10, 8, 8, 1, 0, 0
    d.beam, d.improved, d.state_beam, d.expand_beam = 3, 1, 4.6, 2.3
    d.max_candidates, d.max_pops, d.max_states, d.max_nodes, d.max_len = 64, 8, 24, 64, 16
    d.emb, d.w_o, d.b_o, d.w_d, d.ld_d = P, P, P, P, 16
    for l in range(d.L):
        d.w_ih[l], d.w_hh[l], d.b_ih[l], d.b_hh[l] = P, P, P, P
    d.tokens, d.scores, d.count, d.status = Q, Q, Q, Q
    return d


def _offline():
    from rnntransducer_amd import _lib
    d = _fill(_lib.BeamDesc(), False)
    d.A, d.lens = P, Q
    return d


def _stream():
    from rnntransducer_amd import _lib
    d = _fill(_lib.BeamStreamDesc(), True)
    d.out_lens, d.commit, d.ncommit = Q, Q, Q
    return d


def _fusion(**kw):
    from rnntransducer_amd import _lib
    f = _lib.BeamFusion(P, P, P, 4, Q)
    for k, v in kw.items():
        setattr(f, k, v)
    return C.byref(f)


def test_fused_workspace_queries_add_the_side_arrays_and_leave_the_unfused_size():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    a256 = lambda n: (n + 255) // 256 * 256
    for d, plain, fused in ((_offline(), L.rnnt_hip_beam_workspace_bytes, L.rnnt_hip_beam_fused_workspace_bytes),
                            (_stream(), L.rnnt_hip_beam_stream_workspace_bytes, L.rnnt_hip_beam_stream_fused_workspace_bytes)):
        n0, n1 = plain(C.byref(d)), fused(C.byref(d))
        assert n0 > 0 and n1 - n0 == d.B * (a256(12 * d.max_candidates) + a256(12 * d.max_pops))
        d.max_pops = 0
        assert plain(C.byref(d)) == 0 and fused(C.byref(d)) == 0
    assert L.rnnt_hip_beam_fused_workspace_bytes(None) == 0 and L.rnnt_hip_beam_stream_fused_workspace_bytes(None) == 0
    # the unfused sizes are what they were before the fused entries existed (layout: include/rnnt_hip.h)
    d = _offline()
    table = a256(10 * 4 * 8 * 4)
    slot = (1 * 8 * 2 + 10 + 3) // 4 * 4
    per = a256(64 * 32) + a256(8 * 32) + a256(24 * slot * 4) + a256(24 * 4) + a256(64 * 16)
    assert L.rnnt_hip_beam_workspace_bytes(C.byref(d)) == table + 2 * per
    assert L.rnnt_hip_beam_stream_workspace_bytes(C.byref(_stream())) == table + 2 * (256 + per + a256(64 * 4))


def test_fused_entries_validate_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    err = lambda: L.rnnt_hip_last_error()
    d = _offline()
    ws = L.rnnt_hip_beam_fused_workspace_bytes(C.byref(d))
    d.workspace, d.workspace_bytes = 0x100000, ws
    calls = [
        lambda f, dd=d: L.rnnt_hip_beam_search_fused(C.byref(dd), f, None, None),
    ]
    s = _stream()
    sws = L.rnnt_hip_beam_stream_fused_workspace_bytes(C.byref(s))
    s.workspace, s.workspace_bytes = 0x100000, sws
    rows = 0x30000
    calls.append(lambda f, dd=s: L.rnnt_hip_beam_stream_reset_fused(C.byref(dd), f, rows, 1, 0, None))
    s2 = _stream()
    s2.workspace, s2.workspace_bytes, s2.T, s2.A, s2.lens = 0x100000, sws, 2, P, Q
    calls.append(lambda f, dd=s2: L.rnnt_hip_beam_stream_chunk_fused(C.byref(dd), f, None, None))
    for call in calls:
        assert call(None) == -1 and b"null fusion struct" in err()
        assert call(_fusion(next=None)) == -1 and b"null fusion table" in err()          # a null table with n_states > 0
        assert call(_fusion(arc=None)) == -1 and b"null fusion table" in err()
        assert call(_fusion(final=None)) == -1 and b"null fusion table" in err()
        assert call(_fusion(n_states=0)) == -1 and b"n_states >= 1" in err()
        assert call(_fusion(n_states=-3, next=None)) == -1 and b"n_states >= 1" in err()
        assert call(_fusion(n_states=(1 << 27) // 10 + 1)) == -1 and b"2^27" in err()
        assert call(_fusion(fused_scores=None)) == -1 and b"fused_scores" in err()
    # workspace: misaligned, short (the unfused size does not do), missing
    for dd, call, short in ((d, calls[0], L.rnnt_hip_beam_workspace_bytes(C.byref(d))),
                            (s, calls[1], L.rnnt_hip_beam_stream_workspace_bytes(C.byref(s))),
                            (s2, calls[2], L.rnnt_hip_beam_stream_workspace_bytes(C.byref(s)))):
        full = dd.workspace_bytes
        dd.workspace = 0x100000 + 64
        assert call(_fusion()) == -1 and b"256-byte aligned" in err() and b"_fused_workspace_bytes" in err()
        dd.workspace, dd.workspace_bytes = 0x100000, short
        assert short < full and call(_fusion()) == -1 and b"workspace" in err()
        dd.workspace, dd.workspace_bytes = None, full
        assert call(_fusion()) == -1
        dd.workspace = 0x100000
    # a timing struct, when given, must hold its outputs; a null descriptor
    tm = _lib.BeamTiming(None, None)
    assert L.rnnt_hip_beam_search_fused(C.byref(d), _fusion(), C.byref(tm), None) == -1 and b"frames" in err()
    tm = _lib.BeamTiming(P, None)
    assert L.rnnt_hip_beam_stream_chunk_fused(C.byref(s2), _fusion(), C.byref(tm), None) == -1 and b"commit_frames" in err()
    assert L.rnnt_hip_beam_search_fused(None, _fusion(), None, None) == -1
    assert L.rnnt_hip_beam_stream_chunk_fused(None, _fusion(), None, None) == -1
    assert L.rnnt_hip_beam_stream_reset_fused(None, _fusion(), None, 0, 0, None) == -1
    s3 = _stream()
    s3.workspace, s3.workspace_bytes = 0x100000, sws   # T = 0: a chunk needs frames, refused after the fusion checks
    assert L.rnnt_hip_beam_stream_chunk_fused(C.byref(s3), _fusion(), None, None) == -1 and b"T >= 1" in err()
