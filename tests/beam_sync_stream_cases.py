"""Shared inputs of the streaming frame-synchronous beam search tests (CPU and GPU): the models, with the seeds chosen on the
CPU (tests/test_beam_sync_stream_oracle.py asserts what each seed is chosen for, so the GPU tests are never the first to see a
case), and chunk schedules.  References are computed once per process and shared."""
import functools
import random

import torch

from tests import beam_sync_cases as K
from tests import beam_sync_restatement as R
from tests import beam_sync_stream_restatement as SR

V, HP = 12, 40

# The blank-biased model: K.model's default scale (fc x 6) with fc.bias[blank] += 4, T = 48.  Its beam keeps dropping the
# hypotheses that emitted and reaching their prefixes again a few frames later.  At this seed 29 prefixes are pruned and
# reached again, 8 of them are prefixes of a final hypothesis, the offline tree ends with 126 nodes and the exact keep set
# never exceeds 17.
BIASED = dict(seed=4, T=48, W=4, S=2)
# max_nodes for it: the least the entry accepts, 1 + 4 W S = 33.  A frame needs W S = 8 free slots, the keep set stays at or
# below 17 <= 33 - 8, and the uncollected tree would pass 33 within the first dozen frames: collection must run inside a chunk.
BIASED_MAX_NODES = 1 + 4 * BIASED["W"] * BIASED["S"]

# The confident model: fc x 15.  Its hypotheses agree on a long prefix, so commits do happen.
CONFIDENT = dict(seed=6, T=40, W=4, S=1, scale=7.5)


@functools.lru_cache(maxsize=None)
def biased_case():
    """-> (ora, tn, pn, audio (1,T,6), fp64 net, encoder rows (T, Oe) fp64)"""
    c = BIASED
    ora, tn, pn = K.model(V, HP, 1, "lstm", 8, c["seed"])
    with torch.no_grad():
        ora.fc.bias[0] += 4.0
    x = K.audio(c["T"], c["seed"])
    net64 = R.double_net(ora)
    return ora, tn, pn, x, net64, SR.encode(net64, x, c["T"])


@functools.lru_cache(maxsize=None)
def biased_trace():
    c = BIASED
    _, _, _, _, net64, rows = biased_case()
    return SR.traced(net64, rows, 0, c["W"], c["S"])


@functools.lru_cache(maxsize=None)
def confident_case():
    """-> (ora, tn, pn, audio, per fed count n = 0..T: (hyps, stable prefix tokens, stable prefix frames, boundary margin))"""
    c = CONFIDENT
    ora, tn, pn = K.model(V, HP, 1, "lstm", 8, c["seed"], scale=c["scale"])
    x = K.audio(c["T"], c["seed"])
    st = SR.Stream(R.double_net(ora), x, 0, c["W"], c["S"])
    per_n = []
    for n in range(c["T"] + 1):
        res = st.feed(1 if n else 0)
        per_n.append((res.hyps, *st.stable_prefix(), res.boundary_margin))
    return ora, tn, pn, x, per_n


def random_schedules(T, count=3, seed=0, zeros=True):
    """`count` chunkings of T frames: lists of chunk lengths, each chunk 0..5 frames (0 only with `zeros`), summing to T."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        left, sched = T, []
        while left > 0:
            k = min(left, rng.randint(0 if zeros else 1, 5))
            sched.append(k)
            left -= k
        out.append(sched)
    return out


# The caps.  A blank-biased model (seed 1) that emits at nearly every frame with four hypotheses side by side: its exact keep
# set grows past 40 - W S nodes, so max_nodes = 40 cannot hold the live tree, and its uncommitted tails grow past a handful of
# tokens.  `short`: the frames a second stream hears of the same audio; it stays far below the cap.
CAPS = dict(seed=1, T=48, W=4, S=1, max_nodes=40, short=6)


@functools.lru_cache(maxsize=None)
def caps_case():
    """-> (ora, tn, pn, audio (1,T,6), Trace)"""
    c = CAPS
    ora, tn, pn = K.model(V, HP, 1, "lstm", 8, c["seed"])
    with torch.no_grad():
        ora.fc.bias[0] += 4.0
    x = K.audio(c["T"], c["seed"])
    net64 = R.double_net(ora)
    return ora, tn, pn, x, SR.traced(net64, SR.encode(net64, x, c["T"]), 0, c["W"], c["S"])


def caps_fail_frame():
    """The frames the stream consumes before max_nodes stops it: the first frame t that finds fewer than W S slots free even in
    the collected tree, keep[t - 1] + W S > max_nodes."""
    c = CAPS
    keep = caps_case()[4].keep
    return next(t for t in range(1, c["T"]) if keep[t - 1] + c["W"] * c["S"] > c["max_nodes"])


@functools.lru_cache(maxsize=None)
def caps_tails():
    """Per fed count n = 0..T of the caps model: the longest uncommitted tail of a returned sequence (its tokens past the
    common prefix), and the Results' smallest boundary margin."""
    c = CAPS
    ora, _, _, x, _ = caps_case()
    st = SR.Stream(R.double_net(ora), x, 0, c["W"], c["S"])
    tails, margin = [], float("inf")
    for n in range(c["T"] + 1):
        res = st.feed(1 if n else 0)
        tails.append(max(len(h[0]) for h in res.hyps) - len(st.stable_prefix()[0]))
        margin = min(margin, res.boundary_margin)
    return tails, margin
