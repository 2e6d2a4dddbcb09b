"""Shared inputs of the internal-LM subtraction tests (CPU and GPU): tests/beam_sync_cases.py's models with a fusion automaton and
the weight MU, and for every case the first seed in K.SEEDS at which tests/ilm_restatement.py keeps a boundary margin >= K.MARGIN
(the searches' fp32-against-fp64 decision margin; the term is one more fp32 log-softmax of the same width, inside a key that
already holds one).  tests/test_ilm_oracle.py asserts that every case finds its seed, so the GPU tests are never the first to see
a case.  References are computed once per process and shared."""
import functools
import math

from tests import beam_sync_cases as K
from tests import ilm_restatement as IR
from tests import ngram_cases as NK

MU = 0.3
MARGIN = K.MARGIN

# (T, V, Hp, L, cell, W, S, O, token_min_logp, scale), the layout of K.SHAPE_CASES: the smallest shapes at which the new code can
# go wrong.  V = 63 / 64: one wavefront, the blank takes a lane out of the reduction; 65: a second lane stride, padded Hp;
# W = 64: more new hypotheses than one step group; V = 2048 with a threshold: pruned candidates never read the term
SHAPE_CASES = [
    (7, 5, 12, 1, "gru", 4, 2, 8, -math.inf, 3.0),
    (20, 63, 64, 2, "lstm", 8, 1, 8, -math.inf, 3.0),
    (20, 64, 64, 1, "rnn", 1, 3, 8, -math.inf, 3.0),
    (20, 65, 260, 1, "lstm", 16, 4, 8, -math.inf, 3.0),
    (12, 300, 64, 1, "lstm", 64, 2, 8, -math.inf, 3.0),
    (12, 2048, 64, 1, "lstm", 16, 1, 8, -5.0, 3.0),
]
assert all(c in K.SHAPE_CASES for c in SHAPE_CASES)


@functools.lru_cache(maxsize=None)
def shape_case(c):
    """A bigram TokenFusion plus ILM -> (seed, ora, tn, pn, x (1,T,6), fusion, Result), or None."""
    T, V, Hp, L, cell, W, S, O, min_logp, scale = c
    for seed in K.SEEDS:
        ora, tn, pn = K.model(V, Hp, L, cell, O, seed, scale)
        x = K.audio(T, seed)
        fusion = K.bigram_fusion(V, 0, seed)
        res = IR.search(ora, x, [T], 0, W, S, min_logp, fusion, MU)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, fusion, res
    return None


@functools.lru_cache(maxsize=None)
def blank_case(blank, V, T, W, S):
    """K.BLANKS' shapes with a bigram TokenFusion plus ILM: the excluded index moves with the blank."""
    for seed in K.SEEDS:
        ora, tn, pn = K.model(V, 8, 1, "gru", 8, seed, blank=blank)
        x = K.audio(T, seed)
        fusion = K.bigram_fusion(V, blank, seed)
        res = IR.search(ora, x, [T], blank, W, S, fusion=fusion, mu=MU)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, fusion, res
    return None


NO_FUSION = SHAPE_CASES[0]


@functools.lru_cache(maxsize=None)
def no_fusion_case():
    """ILM subtraction alone (fusion=None) on the first shape -> (seed, ora, tn, pn, x, Result), or None."""
    T, V, Hp, L, cell, W, S, O, min_logp, scale = NO_FUSION
    for seed in K.SEEDS:
        ora, tn, pn = K.model(V, Hp, L, cell, O, seed, scale)
        x = K.audio(T, seed)
        res = IR.search(ora, x, [T], 0, W, S, min_logp, None, MU)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, res
    return None


@functools.lru_cache(maxsize=None)
def ragged_case():
    """K.RAGGED's batch (lens 6, 0, 3, 5) with a bigram TokenFusion plus ILM."""
    c = K.RAGGED
    for seed in K.SEEDS:
        ora, tn, pn = K.model(c["V"], c["Hp"], 1, "lstm", 8, seed)
        x = K.audio(max(c["lens"]), seed, B=len(c["lens"]))
        fusion = K.bigram_fusion(c["V"], 0, seed)
        res = IR.search(ora, x, c["lens"], 0, c["W"], c["S"], fusion=fusion, mu=MU)
        if min(r.boundary_margin for r in res) >= MARGIN:
            return seed, ora, tn, pn, x, fusion, res
    return None


NGRAM = (6, 3, -math.inf)   # (W, S, token_min_logp): one of NK.SYNC_CASES
assert NGRAM in NK.SYNC_CASES


@functools.lru_cache(maxsize=None)
def ngram_case():
    """NK's net and random backoff model plus ILM; the restatement runs on the model's dense expansion."""
    w, s, thr = NGRAM
    for seed in K.SEEDS:
        ora, tn, pn = K.model(NK.V, NK.HP, 1, "lstm", 8, seed)
        x = K.audio(NK.T, seed)
        lm = NK.random_lm(NK.V, seed)
        res = IR.search(ora, x, [NK.T], 0, w, s, thr, lm.to_dense(), MU)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, lm, res
    return None


@functools.lru_cache(maxsize=None)
def exhaustive_case(T, S):
    """K.exhaustive_case's tiny model (V = 3; a beam of 64 holds every sequence) searched with ILM subtraction alone.
    -> (ora, fp64 net, brute-force masses, Result)"""
    ora, tn, pn, x, mass, _ = K.exhaustive_case(T, S)
    net64 = IR.double_net(ora)
    enc = net64.encoder(x.double(), [T])[0]
    return ora, net64, mass, IR.search_one(net64, enc, 0, 64, S, mu=MU)


# Streaming: tests/beam_sync_stream_cases.py's blank-biased model (fc.bias[blank] += 4, V = 12, Hp = 40) with a bigram TokenFusion
# plus ILM, at the least max_nodes the entry accepts (1 + 4 W S = 33, what the existing stream tests use to force a collection
# inside a chunk).  The seed is the first at which the float64 search keeps its margin, the exact keep set leaves a frame its
# W S free slots at every frame, and the uncollected tree outgrows max_nodes: a one-chunk run must collect inside the chunk.
STREAM = dict(T=24, W=4, S=2, V=12, Hp=40)
STREAM_MAX_NODES = 1 + 4 * STREAM["W"] * STREAM["S"]


@functools.lru_cache(maxsize=None)
def stream_case():
    """-> (seed, ora, tn, pn, x (1,T,6), fusion, Result with .keep / .tree), or None"""
    import torch
    c = STREAM
    for seed in K.SEEDS:
        ora, tn, pn = K.model(c["V"], c["Hp"], 1, "lstm", 8, seed)
        with torch.no_grad():
            ora.fc.bias[0] += 4.0
        x = K.audio(c["T"], seed)
        fusion = K.bigram_fusion(c["V"], 0, seed)
        res = IR.search(ora, x, [c["T"]], 0, c["W"], c["S"], fusion=fusion, mu=MU)[0]
        if res.boundary_margin >= MARGIN and max(res.keep) + c["W"] * c["S"] <= STREAM_MAX_NODES < res.tree[-1] - c["W"] * c["S"]:
            return seed, ora, tn, pn, x, fusion, res
    return None


V2 = (3, 2, 4, 1, "lstm", 2, 2)   # (T, V, Hp, L, cell, W, S): one non-blank token, ilm = 0 exactly
