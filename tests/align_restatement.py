"""float64 restatement of the forced alignment (include/rnnt_hip.h: rnnt_hip_joint_align) — test support only, numpy; the
product never imports it.

Lattice of one utterance: blk[t, u] = log p(blank | t, u), emit[t, u] = log p(y_u | t, u) (0 in the last label row), t < T,
u <= U.  Recurrence and tie rule as the header states them:
    v(t,u) = max( v(t-1,u) + blk(t-1,u), v(t,u-1) + emit(t,u-1) ),  v(0,0) = 0,  best = v(Tb-1,Ub) + blk(Tb-1,Ub);
    on exactly equal candidates the blank predecessor (t-1,u) wins.
Walking back from (Tb-1, Ub) under that rule picks, among all paths of the best score, the one whose LAST label is emitted earliest,
then the one before it, and so on: the smallest (f_{U-1}, ..., f_0) in lexicographic order.
"""
import itertools

import numpy as np

NEG = -np.inf


def lattice(logits, labels, blank):
    """logits (T, U+1, V) -> blk, emit (T, U+1) float64 through a float64 log-softmax; labels: U ints."""
    z = np.asarray(logits, dtype=np.float64)
    T, U1, _ = z.shape
    m = z.max(axis=-1, keepdims=True)
    lp = z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))
    blk = lp[:, :, blank].copy()
    emit = np.zeros((T, U1))
    for u in range(U1 - 1):
        emit[:, u] = lp[:, u, int(labels[u])]
    return blk, emit


def lattice_sep(A, C, bias, labels, blank, chunk=16):
    """lattice() for logits[t,u,:] = A[t,:] + C[u,:] + bias without building them all: A (T,V), C (U+1,V), bias (V)."""
    A, C, bias = (np.asarray(x, dtype=np.float64) for x in (A, C, bias))
    T, U1 = A.shape[0], C.shape[0]
    Cb = C + bias
    lse = np.empty((T, U1))
    for t0 in range(0, T, chunk):
        z = A[t0:t0 + chunk, None, :] + Cb[None, :, :]
        m = z.max(axis=-1)
        lse[t0:t0 + chunk] = m + np.log(np.exp(z - m[..., None]).sum(axis=-1))
    blk = A[:, None, blank] + Cb[None, :, blank] - lse
    emit = np.zeros((T, U1))
    if U1 > 1:
        y = np.asarray(labels[:U1 - 1], dtype=np.int64)
        u = np.arange(U1 - 1)
        emit[:, :U1 - 1] = A[:, y] + Cb[u, y][None, :] - lse[:, :U1 - 1]
    return blk, emit


def _sweep_fwd(blk, emit, Tb, Ub):
    """v and the back-pointer bits (True = came from (t, u-1)), one anti-diagonal per step: each v is one add and one max."""
    v = np.full((Tb, Ub + 1), NEG)
    bp = np.zeros((Tb, Ub + 1), dtype=bool)
    v[0, 0] = 0.0
    for d in range(1, Tb + Ub):
        t = np.arange(max(0, d - Ub), min(Tb - 1, d) + 1)
        u = d - t
        tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        down = np.where(t > 0, v[tm, u] + blk[tm, u], NEG)
        left = np.where(u > 0, v[t, um] + emit[t, um], NEG)
        lab = left > down                       # strict: a tie keeps the blank predecessor
        v[t, u] = np.where(lab, left, down)
        bp[t, u] = lab
    return v, bp


def _sweep_bwd(blk, emit, Tb, Ub):
    """w(t,u) = best score of the rest of a path from cell (t,u), the final blank included."""
    w = np.full((Tb + 1, Ub + 2), NEG)
    w[Tb - 1, Ub] = blk[Tb - 1, Ub]
    for d in range(Tb + Ub - 2, -1, -1):
        t = np.arange(max(0, d - Ub), min(Tb - 1, d) + 1)
        u = d - t
        stay = np.where(t + 1 < Tb, blk[t, u] + w[t + 1, u], NEG)
        go = np.where(u < Ub, emit[t, u] + w[t, u + 1], NEG)
        w[t, u] = np.maximum(stay, go)
    return w[:Tb, :Ub + 1]


def log_likelihood(blk, emit, Tb, Ub):
    """log P(y|x) = -nll in float64: the same sweep with log-sum-exp in place of max (the sum over all paths)."""
    a = np.full((Tb, Ub + 1), NEG)
    a[0, 0] = 0.0
    for d in range(1, Tb + Ub):
        t = np.arange(max(0, d - Ub), min(Tb - 1, d) + 1)
        u = d - t
        tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        down = np.where(t > 0, a[tm, u] + blk[tm, u], NEG)
        left = np.where(u > 0, a[t, um] + emit[t, um], NEG)
        a[t, u] = np.logaddexp(down, left)
    return float(a[Tb - 1, Ub] + blk[Tb - 1, Ub])


def viterbi(blk, emit, Tb, Ub):
    """-> frames (Ub ints), best score, M (Tb, Ub): M[t,u] = fwd(t,u) + emit(t,u) + bwd(t,u+1), the best score of any path that
    emits label u at frame t."""
    v, bp = _sweep_fwd(blk, emit, Tb, Ub)
    best = v[Tb - 1, Ub] + blk[Tb - 1, Ub]
    frames = [0] * Ub
    t, u = Tb - 1, Ub
    while u > 0:
        if bp[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    w = _sweep_bwd(blk, emit, Tb, Ub)
    M = v[:, :Ub] + emit[:Tb, :Ub] + w[:, 1:Ub + 1]
    return frames, float(best), M


def margin(frames, best, M):
    """best score minus the best score of any OTHER path (one that emits some label u at a frame t != frames[u]); +inf when
    there is no other path (Ub = 0 or Tb = 1)."""
    Tb, Ub = M.shape
    if Ub == 0 or Tb == 1:
        return np.inf
    other = M.copy()
    other[np.asarray(frames), np.arange(Ub)] = NEG
    return float(best - other.max())


def path_score(blk, emit, frames, Tb):
    """float64 score of the path that emits label u at frames[u] (non-decreasing, in [0, Tb)): its labels, and one blank per frame
    taken in the label row the path has reached when it leaves that frame."""
    f = np.asarray(frames, dtype=np.int64)
    s = float(emit[f, np.arange(len(f))].sum()) if len(f) else 0.0
    row = np.searchsorted(f, np.arange(Tb), side="right")   # labels emitted at frames <= t
    return s + float(blk[np.arange(Tb), row].sum())


def brute_force(blk, emit, Tb, Ub):
    """Every monotone path of a tiny lattice: -> (frames of the best path under the tie rule, best score, second-best score
    over the other paths or -inf)."""
    paths = list(itertools.combinations_with_replacement(range(Tb), Ub))
    scores = [path_score(blk, emit, p, Tb) for p in paths]
    best = max(scores)
    winners = [p for p, s in zip(paths, scores) if s == best]
    win = min(winners, key=lambda p: p[::-1])
    rest = [s for p, s in zip(paths, scores) if p != win]
    return list(win), best, (max(rest) if rest else NEG)
