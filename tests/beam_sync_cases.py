"""Shared inputs of the frame-synchronous beam search tests (CPU and GPU): the models, and the cases with the seed at which
tests/beam_sync_restatement.py keeps a boundary margin >= 1e-4 (the searches' decision margin: fp32 against fp64
log-probabilities differ by about 1e-6).  tests/test_beam_sync_oracle.py asserts that every case finds its seed, so the GPU
tests are never the first to see a case.  References are computed once per process and shared."""
import functools
import math

import torch

from tests import beam_sync_restatement as R

MARGIN = 1e-4
SEEDS = range(20)

# (T, V, Hp, L, cell, W, S, O, token_min_logp, scale): O = joint input width per side; scale multiplies the oracle's initial
# parameters (fc twice as much), which sets the sharpness of the joint's distribution
SHAPE_CASES = [
    (1, 2, 4, 1, "lstm", 1, 1, 8, -math.inf, 3.0),
    (7, 5, 12, 1, "gru", 4, 2, 8, -math.inf, 3.0),
    (20, 63, 64, 2, "lstm", 8, 1, 8, -math.inf, 3.0),
    (20, 64, 64, 1, "rnn", 1, 3, 8, -math.inf, 3.0),
    (20, 65, 260, 1, "lstm", 16, 4, 8, -math.inf, 3.0),
    (12, 300, 64, 1, "lstm", 64, 2, 8, -math.inf, 3.0),     # more candidates than threads; more hypotheses than one step group
    (16, 72, 512, 1, "lstm", 16, 3, 320, -math.inf, 3.0),   # config-2 prediction net
    (12, 2048, 64, 1, "lstm", 16, 1, 8, -5.0, 3.0),
]


def case_id(c):
    return "T%d-V%d-H%d-L%d-%s-W%d-S%d" % c[:7]


def params(V, Hp, L, cell, O, blank=0, bidirectional=False):
    tn = dict(input_size=6, hidden_size=8, output_size=O, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=bidirectional)
    pn = dict(embedding_size=V, pad_token_id=blank, hidden_size=Hp, output_size=O, num_layers=L, rnn_type=cell, dropout=0.0)
    return tn, pn


def model(V, Hp, L, cell, O, seed, scale=3.0, blank=0, bidirectional=False):
    from oracle.rnnt_oracle import OracleJointNet
    tn, pn = params(V, Hp, L, cell, O, blank, bidirectional)
    torch.manual_seed(seed)
    ora = OracleJointNet(tn, pn, V).eval()
    with torch.no_grad():
        for n, p in ora.named_parameters():
            p.mul_(2.0 * scale if n.startswith("fc.") else scale)
        ora.decoder.embedding.weight[blank].zero_()
    return ora, tn, pn


def audio(T, seed, B=1):
    return torch.randn(B, T, 6, generator=torch.Generator().manual_seed(1000 + seed))


@functools.lru_cache(maxsize=None)
def shape_case(c):
    """-> (seed, oracle net, tn, pn, audios (1,T,6), Result) for the first seed with a boundary margin >= MARGIN, or None."""
    T, V, Hp, L, cell, W, S, O, min_logp, scale = c
    for seed in SEEDS:
        ora, tn, pn = model(V, Hp, L, cell, O, seed, scale)
        x = audio(T, seed)
        res = R.search(ora, x, [T], 0, W, S, min_logp)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, res
    return None


# exhaustive: tiny models over V = 3 whose beam of 64 holds every sequence
EXHAUSTIVE = [(3, 1), (2, 2)]   # (T, S)


@functools.lru_cache(maxsize=None)
def exhaustive_case(T, S):
    ora, tn, pn = model(3, 4, 1, "lstm", 8, 7, scale=1.0)
    x = audio(T, 7)
    net64 = R.double_net(ora)
    enc = net64.encoder(x.double(), [T])[0]
    return ora, tn, pn, x, R.brute_force(net64, enc, 0, S), R.search_one(net64, enc, 0, 64, S)


# W = 1 against greedy
GREEDY = [(1, 11, 12, 16), (3, 11, 12, 16)]   # (S, T, V, Hp)


@functools.lru_cache(maxsize=None)
def greedy_case(S, T, V, Hp):
    for seed in SEEDS:
        ora, tn, pn = model(V, Hp, 1, "lstm", 8, seed)
        x = audio(T, seed)
        net64 = R.double_net(ora)
        enc = net64.encoder(x.double(), [T])[0]
        res = R.search_one(net64, enc, 0, 1, S)
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, R.greedy_one(net64, enc, 0, S), res
    return None


# the blank first, in the middle and last: (blank, V, T, W, S)
BLANKS = [(0, 7, 6, 4, 2), (3, 7, 6, 4, 2), (6, 7, 6, 4, 2)]


@functools.lru_cache(maxsize=None)
def blank_case(blank, V, T, W, S):
    for seed in SEEDS:
        ora, tn, pn = model(V, 8, 1, "gru", 8, seed, blank=blank)
        x = audio(T, seed)
        res = R.search(ora, x, [T], blank, W, S)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, res
    return None


# a ragged batch (T_b = T, 0, < T) for the edge rows and the bit-invariance tests: (V, Hp, W, S, lens)
RAGGED = dict(V=9, Hp=12, W=5, S=2, lens=[6, 0, 3, 5])


@functools.lru_cache(maxsize=None)
def ragged_case():
    c = RAGGED
    for seed in SEEDS:
        ora, tn, pn = model(c["V"], c["Hp"], 1, "lstm", 8, seed)
        x = audio(max(c["lens"]), seed, B=len(c["lens"]))
        res = R.search(ora, x, c["lens"], 0, c["W"], c["S"])
        if min(r.boundary_margin for r in res) >= MARGIN:
            return seed, ora, tn, pn, x, res
    return None


MODEL = dict(V=9, Hp=12, W=5, S=2, lens=[6, 4])


@functools.lru_cache(maxsize=None)
def model_case(bidirectional):
    c = MODEL
    for seed in SEEDS:
        ora, tn, pn = model(c["V"], c["Hp"], 1, "lstm", 8, seed, bidirectional=bidirectional)
        x = audio(max(c["lens"]), seed, B=len(c["lens"]))
        res = R.search(ora, x, c["lens"], 0, c["W"], c["S"])
        if min(r.boundary_margin for r in res) >= MARGIN:
            return seed, ora, tn, pn, x, res
    return None


def zero_fusion(V):
    from rnntransducer_amd import TokenFusion
    return TokenFusion(torch.zeros(1, V, dtype=torch.int32), torch.zeros(1, V), torch.zeros(1))


def bigram_fusion(V, blank, seed, weight=0.3):
    from rnntransducer_amd import TokenFusion
    logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(2000 + seed)), dim=1)
    return TokenFusion.from_bigram(logp, weight, blank)


FUSION = dict(T=10, V=12, Hp=16, W=6, S=2)
HOTWORD_WEIGHT = 10.0   # far above a typical -log p: the setting that makes the best-first search's pop loop run away


def hotword_fusion(V, ora, x, T, W, S, weight):
    """Two phrases a search over these frames meets: the first two tokens of the best unfused hypothesis that has two different
    ones, and another token followed by its first."""
    from rnntransducer_amd import TokenFusion
    plain = R.search(ora, x, [T], 0, W, S)[0].hyps
    a, b = next(((y[1], y[2]) for y, _, _ in plain if len(y) >= 3 and y[1] != y[2]), (1, 2))
    other = next(k for k in range(1, V) if k not in (a, b))
    return TokenFusion.from_hotwords([[a, b], [other, a]], weight, V, 0)


@functools.lru_cache(maxsize=None)
def fusion_case(kind):
    """kind: "bigram" | "hotwords" -> (seed, ora, tn, pn, x, fusion, Result) at the first seed with a margin, or None."""
    T, V, Hp, W, S = (FUSION[k] for k in ("T", "V", "Hp", "W", "S"))
    for seed in SEEDS:
        ora, tn, pn = model(V, Hp, 1, "lstm", 8, seed)
        x = audio(T, seed)
        fusion = bigram_fusion(V, 0, seed) if kind == "bigram" else hotword_fusion(V, ora, x, T, W, S, HOTWORD_WEIGHT)
        res = R.search(ora, x, [T], 0, W, S, fusion=fusion)[0]
        if res.boundary_margin >= MARGIN:
            return seed, ora, tn, pn, x, fusion, res
    return None


def close(got, want, rel=1e-5):
    return abs(got - want) <= rel * max(1.0, abs(want))


def same_hyps(got, want, order_gap=MARGIN):
    """One utterance, GPU against restatement: entries (y, score[, fused], frames).  Token lists and frames exact, scores to
    1e-5 relative; output order compared only across pairs at least `order_gap` apart (by the last score of the entry)."""
    assert len(got) == len(want), (got, want)
    by_y = {tuple(e[0]): e for e in got}
    assert len(by_y) == len(got), "a sequence sits in the beam twice"
    for e in want:
        g = by_y.get(tuple(e[0]))
        assert g is not None, (e, got)
        assert g[-1] == e[-1], (g, e)                       # frames
        assert all(close(a, b) for a, b in zip(g[1:-1], e[1:-1])), (g, e)
    pos = {tuple(e[0]): i for i, e in enumerate(got)}
    for i in range(len(want)):
        for j in range(i + 1, len(want)):
            if want[i][-2] - want[j][-2] >= order_gap:
                assert pos[tuple(want[i][0])] < pos[tuple(want[j][0])], (want[i], want[j], got)
