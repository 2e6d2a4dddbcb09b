"""Shared inputs of the backoff n-gram fusion tests (CPU and GPU): seeded random language models built with
NgramFusion.from_ngrams, and the cases with the seed at which the float64 restatements (tests/beam_sync_restatement.py,
tests/ctc_beam_restatement.py), run with the model's dense expansion, keep a boundary margin >= MARGIN.
tests/test_ngram_fusion.py asserts that every case finds its seed, so the GPU tests are never the first to see a case.  The
models need not be normalised: the automaton is the specification.  References are computed once per process and shared."""
import functools
import math
import random

import numpy as np

from tests import beam_sync_cases as K
from tests import beam_sync_restatement as R
from tests import ctc_beam_cases as CK
from tests import ctc_beam_restatement as CR

MARGIN = K.MARGIN
WEIGHT = 0.3
OOV_LOGP = -8.0
T, V, HP, W, S = (K.FUSION[k] for k in ("T", "V", "Hp", "W", "S"))


def random_ngrams(V, seed, blank=0, sentences=True):
    """Order 3: every unigram, a random third of the bigrams, a tenth of the trigrams over those bigrams, random backoffs;
    sentences: <s> as a context and </s> as a successor, like an ARPA model.  -> the mapping from_ngrams takes"""
    from rnntransducer_amd import NgramFusion
    BOS, EOS = NgramFusion.BOS, NgramFusion.EOS
    r = random.Random(3000 + seed)
    toks = [k for k in range(V) if k != blank]
    p, b = (lambda: r.uniform(-4.0, -0.5)), (lambda: r.uniform(-1.5, 0.0))
    ng = {(k,): (p(), b()) for k in toks}
    if sentences:
        ng[(BOS,)] = (-99.0, b())
        ng[(EOS,)] = (p(), None)
    bigrams = [(a, k) for a in toks + ([BOS] if sentences else []) for k in toks if r.random() < 1.0 / 3.0]
    for g in bigrams:
        ng[g] = (p(), b())
    for g in bigrams:
        for k in toks:
            if r.random() < 0.1:
                ng[g + (k,)] = (p(), None)
        if sentences and r.random() < 0.2:
            ng[g + (EOS,)] = (p(), None)
    return ng


@functools.lru_cache(maxsize=None)
def random_lm(V, seed, blank=0, sentences=True):
    from rnntransducer_amd import NgramFusion
    return NgramFusion.from_ngrams(random_ngrams(V, seed, blank, sentences), V, WEIGHT, blank, oov_logp=OOV_LOGP)


# ---- frame-synchronous transducer search: FUSION's net; (W, S, token_min_logp)
SYNC_CASES = [(w, s, thr) for w in (1, 6, 16) for s in (1, 3) for thr in (-math.inf, -3.0)]


def sync_id(c):
    return "W%d-S%d-%s" % (c[0], c[1], "all" if c[2] == -math.inf else "pruned")


@functools.lru_cache(maxsize=None)
def sync_case(c):
    """-> (seed, ora, tn, pn, x (1,T,6), lm, Result) at the first seed whose restatement keeps a margin, or None"""
    w, s, thr = c
    for seed in K.SEEDS:
        ora, tn, pn = K.model(V, HP, 1, "lstm", 8, seed)
        x = K.audio(T, seed)
        lm = random_lm(V, seed)
        res = R.search(ora, x, [T], 0, w, s, thr, fusion=lm.to_dense())[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, lm, res
    return None


@functools.lru_cache(maxsize=None)
def ragged_case():
    """K.RAGGED's batch (lens 6, 0, 3, 5) with an LM over its 9 tokens"""
    c = K.RAGGED
    for seed in K.SEEDS:
        ora, tn, pn = K.model(c["V"], c["Hp"], 1, "lstm", 8, seed)
        x = K.audio(max(c["lens"]), seed, B=len(c["lens"]))
        lm = random_lm(c["V"], seed)
        res = R.search(ora, x, c["lens"], 0, c["W"], c["S"], fusion=lm.to_dense())
        if min(r.boundary_margin for r in res) >= MARGIN:
            return seed, ora, tn, pn, x, lm, res
    return None


BLANK_LAST = K.BLANKS[2]   # (blank, V, T, W, S)


@functools.lru_cache(maxsize=None)
def blank_last_case():
    blank, v, t, w, s = BLANK_LAST
    for seed in K.SEEDS:
        ora, tn, pn = K.model(v, 8, 1, "gru", 8, seed, blank=blank)
        x = K.audio(t, seed)
        lm = random_lm(v, seed, blank)
        res = R.search(ora, x, [t], blank, w, s, fusion=lm.to_dense())[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, lm, res
    return None


# ---- CTC prefix beam search: (T, V, W, token_min_logp, scale)
CTC_CASES = [(10, V, 1, -math.inf, 3.0), (10, V, 6, -math.inf, 3.0), (10, V, 6, -3.0, 3.0)]


@functools.lru_cache(maxsize=None)
def ctc_case(c):
    """-> (seed, logits (T,V) fp32, hyps, lm) at the first seed whose restatement keeps a margin, or None"""
    t, v, w, thr, scale = c
    for seed in range(20):
        z = (scale * np.random.default_rng(1000 + seed).standard_normal((t, v))).astype(np.float32)
        lm = random_lm(v, seed)
        hyps, bm, _ = CR.search(z, 0, w, thr, fusion=lm.to_dense())
        if bm >= CK.MARGIN:
            return seed, z, hyps, lm
    return None


# ---- a model the dense form refuses: V = 2048 with more than 2^27 / 2048 = 65 536 contexts
BIG = K.SHAPE_CASES[7]   # (T, V, Hp, L, cell, W, S, O, token_min_logp, scale) = (12, 2048, 64, 1, "lstm", 16, 1, 8, -5.0, 3.0)
BIG_CONTEXTS = 70000


def big_lm(V, nbest, seed=0):
    """A trigram over V tokens (blank 0): every unigram, BIG_CONTEXTS random bigrams, a trigram behind every tenth of them, and
    every bigram and trigram of the token lists `nbest` (without blanks).  More than 65 536 contexts: to_dense() raises."""
    from rnntransducer_amd import NgramFusion
    r = random.Random(4000 + seed)
    p, b = (lambda: r.uniform(-6.0, -0.5)), (lambda: r.uniform(-1.5, 0.0))
    ng = {(k,): (p(), b()) for k in range(1, V)}
    ng[(NgramFusion.BOS,)] = (-99.0, b())
    ng[(NgramFusion.EOS,)] = (p(), None)
    while len(ng) < V + 1 + BIG_CONTEXTS:
        ng.setdefault((r.randrange(1, V), r.randrange(1, V)), (p(), b()))
    for i, g in enumerate([g for g in ng if len(g) == 2]):
        if i % 10 == 0:
            ng[g + (r.randrange(1, V),)] = (p(), None)
    for y in nbest:
        for i in range(len(y) - 1):
            ng.setdefault((y[i], y[i + 1]), (p(), b()))
        for i in range(len(y) - 2):
            ng.setdefault((y[i], y[i + 1], y[i + 2]), (p(), None))
    return NgramFusion.from_ngrams(ng, V, WEIGHT, 0, oov_logp=OOV_LOGP)
