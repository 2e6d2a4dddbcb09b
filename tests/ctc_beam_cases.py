"""Shared inputs of the CTC beam-search tests (CPU and GPU): the shapes, the seed walk and the automata.  The restatement of a case is
computed once per process and shared (and left unchanged) by the tests that need it."""
import functools
import math

import numpy as np
import torch

from tests import ctc_beam_restatement as R

# (T, V, W, token_min_logp): one frame / the smallest V and W; odd sizes; V one below, at and one above a wavefront's 64 lanes; the
# config-2 vocabulary; more candidates than the workgroup has threads at every W up to the largest; the config-5 vocabulary pruned
SHAPES = [(1, 2, 1, -math.inf), (7, 5, 4, -math.inf), (33, 63, 8, -math.inf), (40, 64, 1, -math.inf), (40, 65, 16, -math.inf),
          (64, 72, 16, -math.inf), (24, 129, 64, -math.inf), (12, 300, 128, -math.inf), (40, 2048, 16, -5.0), (40, 72, 16, -3.0)]
# (V, W, T, seed): peaked logits (3 * standard normal from default_rng(7000 + seed)) over which a prefix falls out of the beam while
# one of its extensions stays, is reached again later and is extended into that member: the prefix must keep ONE node, or the
# labelling sits in the beam twice.  Boundary margins 2.6e-2, 1.1e-1, 2.4e-2, 5.0e-3.
REREACH_CASES = [(3, 3, 8, 7), (4, 3, 10, 56), (5, 4, 12, 56), (4, 2, 10, 317)]
MARGIN = 1e-4


def rereach_logits(V, T, seed):
    return (3.0 * np.random.default_rng(7000 + seed).standard_normal((T, V))).astype(np.float32)
HOTWORD_WEIGHT, BIGRAM_WEIGHT = 0.5, 0.3


def blank_of(V, where):
    return {"first": 0, "middle": V // 2, "last": V - 1}[where]


@functools.lru_cache(maxsize=None)
def shape_case(T, V, W, thr, scale, blank=0, kind=None):
    """(seed, logits (T,V) fp32, hyps, boundary margin, order margin) of the first of 20 seeds from 0 whose restatement keeps a
    boundary margin >= 1e-4, or None.  kind: None | "hotwords" | "bigram" | "zero", the automaton of fusion_for(kind, V, blank, 0)."""
    fusion = fusion_for(kind, V, blank, 0) if kind else None
    return R.first_seed(T, V, W, scale, thr, blank, fusion, start=0, tries=20, margin=MARGIN)


@functools.lru_cache(maxsize=None)
def fusion_for(kind, V, blank, seed):
    from rnntransducer_amd import TokenFusion
    if kind == "zero":
        return TokenFusion(torch.zeros(1, V, dtype=torch.int32), torch.zeros(1, V), torch.zeros(1))
    if kind == "bigram":
        logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(1000 + seed)), dim=1)
        return TokenFusion.from_bigram(logp, BIGRAM_WEIGHT, blank)
    toks = [k for k in range(V) if k != blank]
    # a one-token phrase (banked whenever it is appended) and two longer ones that share a start (begun often, finished rarely)
    phrases = [[toks[0]], [toks[1], toks[2]], [toks[1], toks[3], toks[0]]] if len(toks) >= 4 else [[toks[0]]]
    return TokenFusion.from_hotwords(phrases, HOTWORD_WEIGHT, V, blank)


@functools.lru_cache(maxsize=None)
def fused_case(T, V, W, scale, blank, kind):
    """As shape_case with an automaton, the margin being that of score + total: (seed, logits, hyps, boundary margin, order margin,
    fusion) or None.  "hotwords": phrases the search meets, taken from the best unfused hypothesis of the same logits — its first
    distinct token alone (banked whenever it is appended) and its next two distinct tokens as a pair."""
    from rnntransducer_amd import TokenFusion
    for seed in range(20):
        z = (scale * np.random.default_rng(1000 + seed).standard_normal((T, V))).astype(np.float32)
        if kind == "hotwords":
            u = list(dict.fromkeys(R.search(z, blank, W)[0][0]["tokens"]))
            if len(u) < 3:
                continue
            fusion = TokenFusion.from_hotwords([[u[0]], [u[1], u[2]]], HOTWORD_WEIGHT, V, blank)
        else:
            fusion = fusion_for(kind, V, blank, seed)
        hyps, bm, om = R.search(z, blank, W, fusion=fusion)
        if bm >= MARGIN:
            return seed, z, hyps, bm, om, fusion
    return None


def batch_of(rows, T, V, pad=np.nan):
    """logits (B, T, V) fp32 with row b = rows[b] (T_b, V) and `pad` in every frame >= T_b, and the lengths."""
    z = np.full((len(rows), T, V), pad, dtype=np.float32)
    for b, r in enumerate(rows):
        z[b, :r.shape[0]] = r
    return torch.from_numpy(z), torch.tensor([r.shape[0] for r in rows], dtype=torch.int32)
