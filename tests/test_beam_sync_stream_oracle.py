"""CPU side of the streaming frame-synchronous beam search (csrc/beam_sync_stream.hip): its float64 restatement
(tests/beam_sync_stream_restatement.py) against the offline one, the seeds the GPU tests rely on, the new C symbols, the
workspace query, and every refusal that needs no device."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import beam_sync_cases as K
from tests import beam_sync_restatement as R
from tests import beam_sync_stream_cases as SK
from tests import beam_sync_stream_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_hip_beam_sync_stream_workspace_bytes", "rnnt_hip_beam_sync_stream_reset", "rnnt_hip_beam_sync_stream_chunk")


# 1. the restatement ------------------------------------------------------------------------------------------------------------------
def test_any_chunking_ends_at_the_offline_restatement():
    c = SK.BIASED
    ora, _, _, x, net64, rows = SK.biased_case()
    want = R.search(ora, x, [c["T"]], 0, c["W"], c["S"])[0]
    for sched in [[1] * c["T"], [7] * 6 + [6], [c["T"]]] + SK.random_schedules(c["T"]):
        st = SR.Stream(net64, x, 0, c["W"], c["S"])
        assert st.result.hyps == [([0], 0.0, [-1])] and st.stable_prefix() == ([0], [-1])     # no frames: [[blank]], score 0
        for k in sched:
            before = st.result
            got = st.feed(k)
            assert k > 0 or got is before                                                      # 0 frames: the previous list
        assert got.hyps == want.hyps and st.n == c["T"]
        tokens, frames = st.stable_prefix()
        assert all(h[0][:len(tokens)] == tokens and h[-1][:len(tokens)] == frames for h in got.hyps)
    tr = SK.biased_trace()
    assert [(y, f) for y, _, f in tr.hyps] == [(y, f) for y, _, f in want.hyps]
    assert all(K.close(a[1], b[1], 1e-12) for a, b in zip(tr.hyps, want.hyps))


def test_the_blank_biased_seed_reaches_pruned_prefixes_again_and_its_keep_set_is_small():
    c = SK.BIASED
    tr = SK.biased_trace()
    print("re-reached %d, of them in the final n-best %d; offline tree %d nodes, keep set at most %d, at the end %d"
          % (len(tr.rereached), len(tr.final_rereached), tr.tree[-1], max(tr.keep), tr.keep[-1]))
    assert len(tr.final_rereached) >= 1
    assert all(created < again for created, again in tr.rereached.values())
    # a collection that kept only the paths to the members would stamp these with the later frame: the final frames show the first
    for y in tr.final_rereached:
        h = next(h for h in tr.hyps if tuple(h[0][:len(y)]) == y)
        assert h[2][len(y) - 1] == tr.rereached[y][0]
    assert max(tr.keep) < tr.tree[-1] and all(k <= n for k, n in zip(tr.keep, tr.tree))
    # what tests/test_gpu_beam_sync_stream.py relies on: the least max_nodes holds the keep set plus a frame's W S nodes, and
    # the uncollected tree outgrows it, so collection has to run inside a chunk of all T frames
    assert max(tr.keep) + c["W"] * c["S"] <= SK.BIASED_MAX_NODES < tr.tree[-1]
    _, _, _, _, net64, rows = SK.biased_case()
    assert R.search_one(net64, rows, 0, c["W"], c["S"]).boundary_margin >= K.MARGIN


def test_the_confident_seed_keeps_its_margin_and_commits():
    c = SK.CONFIDENT
    _, _, _, _, per_n = SK.confident_case()
    assert min(m for *_, m in per_n) >= K.MARGIN
    assert len(per_n[-1][1]) >= 5
    for (_, a, fa, _), (_, b, fb, _) in zip(per_n, per_n[1:]):      # a stable prefix only grows
        assert b[:len(a)] == a and fb[:len(fa)] == fa


def test_the_caps_seed_outgrows_max_nodes_and_max_len_where_the_gpu_tests_expect_it():
    c = SK.CAPS
    tr = SK.caps_case()[4]
    t_fail = SK.caps_fail_frame()
    print("keep set per frame", tr.keep, "-> max_nodes = %d stops the stream after %d frames" % (c["max_nodes"], t_fail))
    assert c["short"] + 7 < t_fail < c["T"] and max(tr.keep[:c["short"]]) + c["W"] * c["S"] <= c["max_nodes"]
    assert c["max_nodes"] >= 1 + 4 * c["W"] * c["S"] and tr.tree[-1] > c["max_nodes"]
    tails, margin = SK.caps_tails()
    assert margin >= K.MARGIN and tails[0] == 0
    n_fail = next(n for n, t in enumerate(tails) if t > 10)
    assert 1 < n_fail < c["T"]


# 2. the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_and_bound():
    from rnntransducer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    declared = set(re.findall(r"\b(rnnt_hip_\w+)\s*\(", header))
    handle = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert "typedef struct rnnt_beam_sync_stream_desc" in header
    fields = re.search(r"typedef struct rnnt_beam_sync_stream_desc \{(.*?)\} rnnt_beam_sync_stream_desc;", header, re.S).group(1)
    names = [n.strip(" *") for line in re.findall(r"^\s*(?:const )?\w+\*? ([^;/]+);", fields, re.M) for n in line.split(",")]
    names = [re.sub(r"\[.*\]", "", n) for n in names]
    assert names == [n for n, _ in _lib.BeamSyncStreamDesc._fields_]
    assert _lib.lib().rnnt_hip_version() == _lib.ABI_VERSION == 4


# 3. the workspace query and the C-side refusals --------------------------------------------------------------------------------------
P, Q = 0x10000, 0x20000   # 256-byte aligned stand-ins for device pointers, never dereferenced


def _desc(**kw):
    from rnntransducer_amd import _lib
    d = _lib.BeamSyncStreamDesc()
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank = 3, 2, 10, 8, 8, 1, 0, 0
    d.beam, d.max_symbols, d.step_group, d.token_min_logp = 4, 2, 0, -math.inf
    d.max_nodes, d.max_len = 64, 16
    d.A, d.a_st, d.a_sb, d.lens = P, 20, 10, Q
    d.emb, d.w_o, d.b_o, d.w_d, d.ld_d = P, P, P, P, 16
    d.w_ih[0], d.w_hh[0], d.b_ih[0], d.b_hh[0] = P, P, P, P
    d.tokens, d.out_lens, d.scores, d.count, d.status, d.commit, d.ncommit = Q, Q, Q, Q, Q, Q, Q
    for k, v in kw.items():
        setattr(d, k, v)
    d.workspace, d.workspace_bytes = 0x100000, _lib.lib().rnnt_hip_beam_sync_stream_workspace_bytes(C.byref(d))
    return d


def test_the_workspace_query_is_positive_and_grows():
    a256 = lambda n: (n + 255) // 256 * 256
    slot = (1 * 8 * 2 + 10 + 3) // 4 * 4
    per = 256 + a256(4 * 32) + a256(16 * slot * 4) + a256(4 * 10 * 8) + a256(5 * 64 * 4) + 2 * a256(64 * 4)
    base = _desc().workspace_bytes
    assert base == a256(10 * 4 * 8 * 4) + 2 * per > 0
    assert _desc(B=3).workspace_bytes == base + per
    assert _desc(beam=5).workspace_bytes > base and _desc(max_nodes=65).workspace_bytes > base
    assert _desc(max_symbols=3, max_nodes=64).workspace_bytes > base
    assert _desc(T=0).workspace_bytes == base == _desc(T=500).workspace_bytes      # the chunk length sizes nothing carried
    assert _desc(max_len=1000).workspace_bytes == base                              # nor does max_len: it sizes the outputs


def test_the_c_entries_validate_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    err = lambda: L.rnnt_hip_last_error()
    chunk = lambda d, f=None, tm=None: L.rnnt_hip_beam_sync_stream_chunk(C.byref(d), f, tm, None)
    reset = lambda d, rows=Q, n=1: L.rnnt_hip_beam_sync_stream_reset(C.byref(d), rows, n, 0, None)
    assert L.rnnt_hip_beam_sync_stream_workspace_bytes(None) == 0 and b"null descriptor" in err()
    assert L.rnnt_hip_beam_sync_stream_chunk(None, None, None, None) == -1 and L.rnnt_hip_beam_sync_stream_reset(None, Q, 1, 0, None) == -1
    for kw, what in ((dict(beam=0), b"beam width"), (dict(beam=65), b"beam width"), (dict(max_symbols=0), b"max_symbols"),
                     (dict(max_symbols=5), b"max_symbols"), (dict(V=1), b"V = 1"), (dict(blank=10), b"blank"), (dict(blank=-1), b"blank"),
                     (dict(V=1 << 23, beam=3), b"2^24"), (dict(token_min_logp=math.nan), b"token_min_logp"),
                     (dict(token_min_logp=math.inf), b"token_min_logp"), (dict(step_group=-1), b"step_group"),
                     (dict(Hp=6), b"multiples of 4"), (dict(L=9), b"layers"), (dict(cell=7), b"cell"), (dict(T=-1), b"negative"),
                     (dict(B=0), b"B positive"), (dict(max_nodes=32), b"max_nodes"), (dict(max_nodes=1 << 30), b"max_nodes"),
                     (dict(max_len=0), b"max_len"), (dict(Hp=4096, L=8, max_nodes=64), b"LDS")):
        bad = _desc(**kw)
        assert bad.workspace_bytes == 0 and what in err(), (kw, err())
        bad.workspace_bytes = 1 << 40
        assert chunk(bad) == -1 and what in err(), (kw, err())
        assert reset(bad) == -1 and what in err(), (kw, err())
    assert _desc(max_nodes=33).workspace_bytes > 0                                  # 1 + 4 W S is accepted
    for kw, what in ((dict(A=None), b"A and lens"), (dict(lens=None), b"A and lens"), (dict(T=0), b"T >= 1"), (dict(tokens=None), b"null"),
                     (dict(out_lens=None), b"null"), (dict(scores=None), b"null"), (dict(count=None), b"null"), (dict(status=None), b"null"),
                     (dict(commit=None), b"null"), (dict(ncommit=None), b"null"), (dict(emb=None), b"null"), (dict(w_o=None), b"null"),
                     (dict(a_st=0), b"strides"), (dict(a_sb=0), b"strides"), (dict(ld_d=18), b"16-byte aligned"),
                     (dict(w_d=P + 4), b"16-byte aligned")):
        assert chunk(_desc(**kw)) == -1 and what in err(), (kw, err())
    bad = _desc()
    bad.w_hh[0] = None
    assert chunk(bad) == -1 and b"null weight" in err() and reset(bad) == -1 and b"null weight" in err()
    for entry in (chunk, reset):                                                    # the workspace: short, misaligned, missing
        bad = _desc()
        bad.workspace_bytes -= 1
        assert entry(bad) == -1 and b"workspace" in err()
        bad = _desc()
        bad.workspace = 0x100000 + 64
        assert entry(bad) == -1 and b"256-byte aligned" in err()
        bad = _desc()
        bad.workspace = None
        assert entry(bad) == -1 and b"workspace" in err()
    assert reset(_desc(), None, 1) == -1 and b"row list" in err() and reset(_desc(), Q, -1) == -1 and b"row list" in err()
    fus = lambda **kw: C.byref(_lib.BeamFusion(**{**dict(next=P, arc=P, final=P, n_states=4, fused_scores=Q), **kw}))
    d = _desc()
    for kw, what in ((dict(next=None), b"null fusion table"), (dict(arc=None), b"null fusion table"), (dict(final=None), b"null fusion table"),
                     (dict(n_states=0), b"n_states"), (dict(n_states=(1 << 27) // 10 + 1), b"2^27"), (dict(fused_scores=None), b"fused_scores")):
        assert chunk(d, fus(**kw)) == -1 and what in err(), (kw, err())
    assert chunk(d, None, C.byref(_lib.BeamTiming(None, None))) == -1 and b"timing" in err()
    assert chunk(d, None, C.byref(_lib.BeamTiming(Q, None))) == -1 and b"commit_frames" in err()


# 4. the Python guards that need no device --------------------------------------------------------------------------------------------
def _net(bidirectional=False, V=6):
    from rnntransducer_amd.networks import JointNet
    tn, pn = K.params(V, 8, 1, "lstm", 8, bidirectional=bidirectional)
    return JointNet(dict(tn), dict(pn), V).eval()


def test_init_refuses_bad_arguments_before_anything_is_allocated():
    net = _net()
    for kw, what in ((dict(beam_widths=0), "beam width"), (dict(beam_widths=65), "beam width"), (dict(beam_widths=True), "beam width"),
                     (dict(max_symbols=0), "max_symbols"), (dict(max_symbols=5), "max_symbols"),
                     (dict(token_min_logp=math.nan), "token_min_logp"), (dict(token_min_logp=math.inf), "token_min_logp"),
                     (dict(token_min_logp="x"), "token_min_logp"), (dict(fusion=object()), "fusion"),
                     (dict(fusion=K.zero_fusion(5)), "over 5 tokens"), (dict(device="cuda:7"), "not the model's"),
                     (dict(max_nodes=64), "max_nodes"), (dict(beam_widths=4, max_symbols=2, max_nodes=32), "max_nodes"),
                     (dict(max_nodes=1 << 30), "max_nodes"), (dict(max_nodes=8192.0), "max_nodes"), (dict(max_len=0), "max_len")):
        with pytest.raises(ValueError, match=what):
            net.init_beam_sync_stream(2, 0, **kw)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="batch_size"):
            net.init_beam_sync_stream(bad, 0)
    for bad in (-1, 6):
        with pytest.raises(ValueError, match="blank"):
            net.init_beam_sync_stream(2, bad)
    with pytest.raises(ValueError, match="bidirectional"):
        _net(bidirectional=True).init_beam_sync_stream(2, 0)
    with pytest.raises(ValueError, match="eval"):
        _net().train().init_beam_sync_stream(2, 0)
    with pytest.raises(TypeError):
        net.init_beam_sync_stream(2, 0, max_pops=5)                                 # no such cap: there is no pop loop


def test_the_chunk_call_refuses_before_it_looks_at_the_chunk():
    from rnntransducer_amd.model import RNNTransducer
    net, x = _net(), torch.zeros(2, 3, 6)
    with pytest.raises(ValueError, match="eval"):
        _net().train().recognize_beams_sync_stream(x, [3, 3], None)
    with pytest.raises(ValueError, match="bidirectional"):
        _net(bidirectional=True).recognize_beams_sync_stream(x, [3, 3], None)
    with pytest.raises(ValueError, match="init_beam_sync_stream"):
        net.recognize_beams_sync_stream(x, [3, 3], object())
    for name in ("init_beam_sync_stream", "recognize_beams_sync_stream"):
        assert callable(getattr(RNNTransducer, name))


def test_ops_guards():
    from rnntransducer_amd import ops
    assert ops.beam_sync_stream_caps(16, 1) == dict(max_nodes=8192, max_len=256)
    assert ops.beam_sync_stream_caps(4, 2, max_nodes=33)["max_nodes"] == 33
    with pytest.raises(ValueError, match="max_nodes"):
        ops.beam_sync_stream_caps(64, 4, max_nodes=1024)                             # 1 + 4 * 64 * 4 = 1025
    args = [torch.zeros(6, 16), torch.zeros(6, 8), [torch.zeros(32, 8), torch.zeros(32, 8), torch.zeros(32), torch.zeros(32)], 0,
            torch.zeros(8, 8), torch.zeros(8)]
    caps = ops.beam_sync_stream_caps(4, 1)
    for a, what in (((0, 65, 1, -math.inf), "beam width"), ((0, 4, 5, -math.inf), "max_symbols"), ((0, 4, 1, math.nan), "token_min_logp")):
        with pytest.raises(ValueError, match=what):
            ops.beam_sync_stream_desc(2, *args, *a, caps)
    with pytest.raises(ValueError, match="step_group"):
        ops.beam_sync_stream_desc(2, *args, 0, 4, 1, -math.inf, caps, step_group=-1)
    with pytest.raises(ValueError, match="streams"):
        ops.beam_sync_stream_desc(0, *args, 0, 4, 1, -math.inf, caps)
