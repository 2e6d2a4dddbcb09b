"""NgramFusion on the host (rnntransducer_amd/fusion.py): the ARPA reader against an independent recursive backoff scorer, the
sparse lookup against its own dense expansion, every refusal, the three *_ngram C entries' host checks (stand-in addresses that
are never dereferenced), and the seeds of tests/ngram_cases.py.  No GPU."""
import ctypes as C
import itertools
import math
import random

import numpy as np
import pytest
import torch

from tests import ngram_cases as NK

LN10 = math.log(10.0)
WEIGHT = 0.3

ARPA = """
\\data\\
ngram 1=7
ngram 2=5
ngram 3=3

\\1-grams:
-99 <s> -0.4
-1.2 </s>
-1.7 <unk>
-0.8 a -0.3
-0.9 b -0.25
-1.1 zed -0.2
-1.0 c

\\2-grams:
-0.5 <s> a -0.2
-0.6 a b -0.15
-0.7 b a
-0.4 b </s>
-0.9 a zed

\\3-grams:
-0.3 <s> a b
-0.2 a b a
-0.35 a b </s>

\\end\\
"""
SYMBOLS = [None, "a", "b", "c", "d"]   # the blank; "zed" is absent; "d" has no unigram: <unk>'s
# the same model written down by hand: words -> (log10 p, log10 backoff); a missing backoff is 0
LISTED = {("<s>",): (-99.0, -0.4), ("</s>",): (-1.2, 0.0), ("a",): (-0.8, -0.3), ("b",): (-0.9, -0.25), ("c",): (-1.0, 0.0),
          ("<s>", "a"): (-0.5, -0.2), ("a", "b"): (-0.6, -0.15), ("b", "a"): (-0.7, 0.0), ("b", "</s>"): (-0.4, 0.0),
          ("<s>", "a", "b"): (-0.3, 0.0), ("a", "b", "a"): (-0.2, 0.0), ("a", "b", "</s>"): (-0.35, 0.0)}
UNK = -1.7


def _f32(x):
    return float(np.float32(x))


def _p(w, h, acc=0.0):
    """p(w | h) = listed ? p : bow(h) p(w | h[1:]), in the logarithm, the backoffs summed oldest first in float64 and every
    table entry the float32 of weight * ln: what the automaton's definition fixes"""
    if h + (w,) in LISTED:
        return acc + _f32(WEIGHT * (LISTED[h + (w,)][0] * LN10))
    if not h:
        return acc + _f32(WEIGHT * (UNK * LN10))
    return _p(w, h[1:], acc + _f32(WEIGHT * (LISTED.get(h, (0.0, 0.0))[1] * LN10)))


def _score(y):
    h, total = ("<s>",), 0.0
    for k in y[1:]:
        total += _f32(_p(SYMBOLS[k], h))
        h = (h + (SYMBOLS[k],))[-2:]
    return total, _f32(_p("</s>", h))


def test_hand_written_arpa_scores_as_the_recursive_backoff_scorer():
    from rnntransducer_amd import NgramFusion
    lm = NgramFusion.from_arpa(ARPA.splitlines(), SYMBOLS, WEIGHT, 0)
    assert (lm.order, lm.vocab_size, lm.root, lm.n_arcs) == (3, 5, 1, lm.tok.numel()) and lm.device.type == "cpu"
    # states: [<s>], the root, a, b, c, <s> a, a b, b a
    assert lm.n_states == 8 and int(lm.backoff[0]) == lm.root == int(lm.backoff[lm.root])
    assert lm.score([0]) == (0.0, _f32(_p("</s>", ("<s>",))), 0)               # the start state: the context [<s>]
    assert lm.lookup(lm.root, 4) == (_f32(WEIGHT * (UNK * LN10)), lm.root)      # no unigram: <unk>'s, and no context
    assert lm.lookup(lm.root, 0)[0] == lm.lookup(lm.root, 4)[0]                 # the blank too
    n = 0
    for length in range(5):
        for y in itertools.product(range(1, 5), repeat=length):
            total, final, _ = lm.score([0, *y])
            assert (total, final) == _score([0, *y]), y                         # python floats: == is bitwise
            n += 1
    assert n == 341
    explicit = NgramFusion.from_arpa(ARPA.splitlines(), SYMBOLS, WEIGHT, 0, oov_logp=-3.0)
    assert explicit.lookup(explicit.root, 4)[0] == _f32(WEIGHT * -3.0)


def test_arpa_from_a_path(tmp_path):
    from rnntransducer_amd import NgramFusion
    path = tmp_path / "lm.arpa"
    path.write_text(ARPA)
    a, b = NgramFusion.from_arpa(str(path), SYMBOLS, WEIGHT, 0), NgramFusion.from_arpa(ARPA.splitlines(), SYMBOLS, WEIGHT, 0)
    assert all(torch.equal(getattr(a, t), getattr(b, t)) for t in NgramFusion._TABLES)


@pytest.mark.parametrize("sentences", [True, False], ids=["bos-eos", "plain"])
def test_the_dense_expansion_is_the_same_automaton(sentences):
    from rnntransducer_amd import TokenFusion
    for seed in range(3):
        lm = NK.random_lm(NK.V, seed, 0, sentences)
        dense = lm.to_dense()
        assert isinstance(dense, TokenFusion) and dense.n_states == lm.n_states and dense.vocab_size == NK.V
        assert lm.order == 3 and (lm.root == 1) == sentences
        r = random.Random(seed)
        for _ in range(200):
            y = [0] + [r.randrange(0, NK.V) for _ in range(r.randrange(0, 10))]
            assert lm.score(y) == dense.score(y), y                             # total, final and state, bitwise
        assert lm.to("cpu") is lm


def _arpa(unigrams, bigrams=(), trigrams=(), counts=None):
    secs = [list(unigrams), list(bigrams), list(trigrams)]
    counts = counts or [len(s) for s in secs]
    out = ["\\data\\"] + ["ngram %d=%d" % (i + 1, c) for i, c in enumerate(counts) if secs[i]] + [""]
    for i, s in enumerate(secs):
        if s:
            out += ["\\%d-grams:" % (i + 1)] + s + [""]
    return out + ["\\end\\"]


def test_every_refusal():
    from rnntransducer_amd import NgramFusion
    sym = [None, "a", "b"]
    uni = ["-1 a -0.1", "-1 b -0.1", "-2 <unk>"]
    ok = NgramFusion.from_arpa(_arpa(uni, ["-0.5 a b -0.1"], ["-0.2 a b a"]), sym, 0.5, 0)
    assert (ok.order, ok.n_states) == (3, 4)
    for lines, what in ((_arpa(uni, ["-0.5 a b"], ["-0.2 b a b"]), "context"),                        # "b a" is not listed
                        (_arpa(uni + ["-1 a"], counts=[4, 0, 0]), "twice"),
                        (_arpa(uni, ["-0.5 a b"], counts=[3, 2, 0]), "counts"),
                        (_arpa(["-1 a -0.1", "-inf b", "-2 <unk>"]), "non-finite"),
                        (_arpa(["-1 a -0.1", "nan b", "-2 <unk>"]), "non-finite"),
                        (_arpa(["-1 a -0.1", "-1 b"]), "no unigram"),                                  # the blank has none, no <unk>
                        (_arpa(["-1 a b -0.1"]), "fields"),
                        (["\\data\\", "ngram 1=1", "", "\\2-grams:", "-1 a b", "\\end\\"], "count line")):
        with pytest.raises(ValueError, match=what):
            NgramFusion.from_arpa(lines, sym, 0.5, 0)
    with pytest.raises(ValueError, match="twice"):
        NgramFusion.from_arpa(_arpa(uni), [None, "a", "a"], 0.5, 0)
    nine = ["\\data\\"] + ["ngram %d=1" % n for n in range(1, 10)]
    for n in range(1, 10):
        nine += ["\\%d-grams:" % n, "-1 " + " ".join(["a"] * n) + (" -0.1" if n < 9 else "")]
    with pytest.raises(ValueError, match="order 9"):
        NgramFusion.from_arpa(nine + ["\\end\\"], sym, 0.5, 0, oov_logp=-5.0)
    chain = {tuple([1] * n): (-1.0, -0.1) for n in range(1, 10)}
    with pytest.raises(ValueError, match="order 9"):
        NgramFusion.from_ngrams(chain, 3, 0.5, 0, oov_logp=-5.0)
    B, E = NgramFusion.BOS, NgramFusion.EOS
    base = {(1,): (-1.0, -0.1), (2,): (-1.0, None)}
    for extra, kw, what in (({(2, 1, 2): (-1.0, None)}, {}, "context"), ({(3,): (-1.0, None)}, {}, r"outside \[0, 3\)"),
                            ({(0,): (-1.0, None)}, {}, "blank"), ({(1, B): (-1.0, None)}, {}, "<s> past"),
                            ({(E, 1): (-1.0, None)}, {}, "</s> before"), ({(1, E): (-1.0, None)}, {}, "unigram of </s>"),
                            ({(1, 2): (math.inf, None)}, {}, "non-finite"), ({}, dict(oov_logp=None), "no unigram"),
                            ({}, dict(oov_logp=math.nan), "oov_logp"), ({}, dict(weight=math.inf), "weight")):
        with pytest.raises(ValueError, match=what):
            NgramFusion.from_ngrams({**base, **extra}, 3, kw.get("weight", 0.5), 0, oov_logp=kw.get("oov_logp", -5.0))
    with pytest.raises(ValueError, match="no n-grams"):
        NgramFusion.from_ngrams({}, 3, 0.5, 0, oov_logp=-5.0)
    # tables given directly: the constructor checks what the device relies on
    lm = NK.random_lm(NK.V, 0)
    t = lambda **kw: NgramFusion(**{**{n: getattr(lm, n).clone() for n in NgramFusion._TABLES},
                                    **dict(root=lm.root, order=lm.order, vocab_size=NK.V), **kw})
    assert t().score([0, 3, 4, 5]) == lm.score([0, 3, 4, 5])
    swapped = lm.tok.clone()
    lo = int(lm.row_ptr[lm.root])
    swapped[lo], swapped[lo + 1] = swapped[lo + 1].item(), swapped[lo].item()
    loop = lm.backoff.clone()
    loop[0] = 0
    for kw, what in ((dict(order=9), "order"), (dict(order=0), "order"), (dict(root=lm.n_states), "root"), (dict(tok=swapped), "ascending"),
                     (dict(next=lm.next + lm.n_states), "next"), (dict(backoff=loop), "backoff chain"), (dict(order=2), "backoff chain"),
                     (dict(arc=lm.arc.double()), "float32"), (dict(bow=lm.bow * math.inf), "finite"), (dict(root=0), "root"),
                     (dict(row_ptr=lm.row_ptr[:-1].clone()), "row_ptr"), (dict(vocab_size=NK.V + 1), "root's row")):
        with pytest.raises(ValueError, match=what):
            t(**kw)
    with pytest.raises(ValueError, match="2\\^27"):
        big = object.__new__(NgramFusion)
        big.bow, big._V = torch.zeros(1 << 20), 1 << 8
        big.to_dense()


def test_searches_without_a_bound_refuse_an_ngram_model_and_name_those_that_take_one():
    from rnntransducer_amd import ops
    from rnntransducer_amd.networks import JointNet
    from tests import beam_sync_cases as K
    lm = NK.random_lm(NK.V, 0)
    tn, pn = K.params(NK.V, 8, 1, "lstm", 8)
    net = JointNet(dict(tn), dict(pn), NK.V).eval()
    x = torch.zeros(1, 4, 6)
    for call in (lambda: net.recognize_beams(x, [4], 0, 4, fusion=lm), lambda: net.init_beam_stream(1, 0, 4, fusion=lm)):
        with pytest.raises(ValueError, match="recognize_beams_sync.*recognize_ctc_beams"):
            call()
    with pytest.raises(ValueError, match="over 12 tokens"):
        ops.check_fusion(lm, NK.V + 1, torch.device("cpu"), "x", ngram=True)
    with pytest.raises(ValueError, match="tables are on cpu"):
        ops.check_fusion(lm, NK.V, torch.device("cuda", 0), "x", ngram=True)
    with pytest.raises(ValueError, match="TokenFusion or NgramFusion"):
        ops.check_fusion(object(), NK.V, torch.device("cpu"), "x", ngram=True)
    ops.check_fusion(lm, NK.V, torch.device("cpu"), "x", ngram=True)


# ---- the C entries -----------------------------------------------------------------------------------------------------------------
P, Q = 0x10000, 0x20000   # 256-byte aligned stand-ins for device pointers, never dereferenced


def _fill(d):
    d.T, d.B, d.V, d.Hp, d.O, d.L, d.cell, d.blank = 3, 2, 10, 8, 8, 1, 0, 0
    d.beam, d.max_symbols, d.step_group, d.token_min_logp = 4, 2, 0, -math.inf
    d.A, d.a_st, d.a_sb = P, 20, 10
    d.emb, d.w_o, d.b_o, d.w_d, d.ld_d = P, P, P, P, 16
    d.w_ih[0], d.w_hh[0], d.b_ih[0], d.b_hh[0] = P, P, P, P
    d.tokens, d.scores, d.count = Q, Q, Q
    return d


def _ngram(**kw):
    from rnntransducer_amd import _lib
    g = _lib.BeamNgram(row_ptr=P, tok=P, arc=P, next=P, bow=P, backoff=P, final=P, root=1, order=3, n_states=4, n_arcs=16, fused_scores=Q)
    for k, v in kw.items():
        setattr(g, k, v)
    return C.byref(g)


def test_the_ngram_entries_validate_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    err = lambda: L.rnnt_hip_last_error()
    d = _fill(_lib.BeamSyncDesc())
    d.t_lens, d.lens = Q, Q
    d.workspace, d.workspace_bytes = 0x100000, L.rnnt_hip_beam_sync_workspace_bytes(C.byref(d))
    s = _fill(_lib.BeamSyncStreamDesc())
    s.max_nodes, s.max_len, s.lens = 64, 16, Q
    s.out_lens, s.status, s.commit, s.ncommit = Q, Q, Q, Q
    s.workspace, s.workspace_bytes = 0x100000, L.rnnt_hip_beam_sync_stream_workspace_bytes(C.byref(s))
    assert d.workspace_bytes > 0 and s.workspace_bytes > 0
    nws = L.rnnt_hip_ctc_beam_workspace_bytes(2, 3, 10, 4)
    calls = (lambda g: L.rnnt_hip_beam_sync_search_ngram(C.byref(d), g, None, None),
             lambda g: L.rnnt_hip_beam_sync_stream_chunk_ngram(C.byref(s), g, None, None),
             lambda g: L.rnnt_hip_ctc_beam_search_ngram(P, 30, 10, Q, 2, 3, 10, 0, 4, -math.inf, g, Q, Q, Q, None, Q, 0x100000, nws, None))
    tables = ("row_ptr", "tok", "arc", "next", "bow", "backoff", "final")
    for call in calls:
        assert call(None) == -1 and b"null ngram struct" in err()
        for t in tables:
            assert call(_ngram(**{t: None})) == -1 and b"null ngram table" in err(), t
        for kw, what in ((dict(n_states=0), b"n_states >= 1"), (dict(root=4), b"root"), (dict(root=-1), b"root"), (dict(order=9), b"order"),
                         (dict(order=0), b"order"), (dict(n_arcs=9), b"n_arcs"), (dict(fused_scores=None), b"fused_scores")):
            assert call(_ngram(**kw)) == -1 and what in err(), (kw, err())
    # the extended entries' own checks still come first
    d.beam = 65
    assert calls[0](_ngram()) == -1 and b"beam width" in err()
    assert L.rnnt_hip_ctc_beam_search_ngram(P, 30, 10, Q, 2, 3, 10, 10, 4, -math.inf, _ngram(), Q, Q, Q, None, Q, 0x100000, nws, None) == -1
    assert b"blank" in err()


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", NK.SYNC_CASES, ids=NK.sync_id)
def test_every_sync_case_finds_its_seed(c):
    found = NK.sync_case(c)
    assert found is not None and found[-1].boundary_margin >= NK.MARGIN


def test_the_ragged_blank_last_and_ctc_cases_find_their_seeds():
    assert NK.ragged_case() is not None and NK.blank_last_case() is not None
    assert all(NK.ctc_case(c) is not None for c in NK.CTC_CASES)


def test_the_large_model_is_one_the_dense_form_refuses():
    lm = NK.big_lm(NK.BIG[1], [[5, 9, 5, 1000], [7, 2047]])
    assert lm.n_states * lm.vocab_size > 1 << 27 and lm.n_states > 65536 and lm.order == 3
    with pytest.raises(ValueError, match="2\\^27"):
        lm.to_dense()
    total, final, state = lm.score([0, 5, 9, 5, 1000])
    assert state not in (0, lm.root) and math.isfinite(total) and final < 0.0
