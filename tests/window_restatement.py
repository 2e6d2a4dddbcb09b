"""Alignment-restricted RNN-T loss (per-label emission windows) in float64 numpy, written from the definition (include/rnnt_hip.h,
DESIGN.md §24), for the tests.

Label u of an utterance with Tb frames and Ub labels may be emitted at frame t only if max(lo[u], 0) <= t <= min(hi[u], Tb - 1); blank
transitions are unrestricted.  The lattice is the usual one over the table emit'(t,u) = emit(t,u) inside the window, -inf outside:
    alpha(0,0) = 0,   alpha(t,u) = logaddexp(alpha(t-1,u) + blk(t-1,u), alpha(t,u-1) + emit'(t,u-1))
    beta(Tb-1,Ub) = blk(Tb-1,Ub),   beta(t,u) = logaddexp(beta(t+1,u) + blk(t,u), beta(t,u+1) + emit'(t,u))
    logZ = beta(0,0),   nll = -logZ   (+inf, with a zero gradient, when no path is left)
    cb = exp(alpha + blk + beta(t+1,u) - logZ),  ce = exp(alpha + emit' + beta(t,u+1) - logZ),  w = exp(alpha + beta - logZ)
    dz[t,u,v] = softmax_v (w + lam ce) - [v = blank] cb - [v = y_u] (1 + lam) ce        (lam: FastEmit's weight, 0 = off)
No band and no work skipping here: every cell of the lattice is computed.  Nothing is shared with the library, with oracle/ or with
the other restatements."""
import itertools

import numpy as np

NEG = -np.inf


def _log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def _lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log1p(np.exp(min(a, b) - m))


def masked_emit(emit, Tb, Ub, lo, hi):
    """emit (T, U+1) -> (Tb, Ub+1) copy with -inf outside each label's window (column Ub: no label, left as it is)."""
    e = np.array(emit[:Tb, :Ub + 1], dtype=np.float64)
    t = np.arange(Tb)
    for u in range(Ub):
        a, b = max(int(lo[u]), 0), min(int(hi[u]), Tb - 1)
        e[(t < a) | (t > b), u] = NEG
    return e


def lattice(blk, emit, Tb, Ub):
    """blk, emit (>= Tb, >= Ub+1) float64 with -inf allowed -> alpha, beta (Tb, Ub+1), logZ."""
    a = np.full((Tb, Ub + 1), NEG)
    b = np.full((Tb, Ub + 1), NEG)
    a[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            down = a[t - 1, u] + blk[t - 1, u] if t > 0 else NEG
            left = a[t, u - 1] + emit[t, u - 1] if u > 0 else NEG
            a[t, u] = _lae(down, left)
    b[Tb - 1, Ub] = blk[Tb - 1, Ub]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                continue
            nb = b[t + 1, u] + blk[t, u] if t < Tb - 1 else NEG
            ne = b[t, u + 1] + emit[t, u] if u < Ub else NEG
            b[t, u] = _lae(nb, ne)
    return a, b, b[0, 0]


def _exp0(x):
    """exp with NaN (from -inf - -inf, which cannot happen once logZ is finite, or +inf - inf) mapped to 0."""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.exp(x), nan=0.0)


def posteriors(blk, emit, Tb, Ub):
    """-> logZ, cb, ce, w (each (Tb, Ub+1)); logZ = -inf: all zeros."""
    a, b, logZ = lattice(blk, emit, Tb, Ub)
    z = np.zeros((Tb, Ub + 1))
    if logZ == NEG:
        return logZ, z, z.copy(), z.copy()
    bl, em = blk[:Tb, :Ub + 1], emit[:Tb, :Ub + 1]
    bt = np.full((Tb, Ub + 1), NEG)
    bt[:-1] = b[1:]
    bt[Tb - 1, Ub] = 0.0
    bu = np.full((Tb, Ub + 1), NEG)
    bu[:, :-1] = b[:, 1:]
    with np.errstate(invalid="ignore"):
        cb, ce, w = _exp0(a + bl + bt - logZ), _exp0(a + em + bu - logZ), _exp0(a + b - logZ)
    ce[:, Ub] = 0.0
    return logZ, cb, ce, w


def window_loss(z, labels, t_lens, u_lens, blank, lo, hi, lam=0.0):
    """z (B,T,U+1,V) logits, labels (B,U), lo / hi (B,U) -> nll (B,), dz (B,T,U+1,V) float64; zeros outside each utterance's lattice and
    in every infeasible row (nll = +inf there, also for t_lens[b] = 0)."""
    z = np.asarray(z, dtype=np.float64)
    B, T, U1, V = z.shape
    nll, dz = np.zeros(B), np.zeros_like(z)
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        if Tb == 0:
            nll[b] = np.inf
            continue
        lp = _log_softmax(z[b])
        y = np.asarray(labels[b][:U1 - 1], dtype=np.int64) if U1 > 1 else np.zeros(0, dtype=np.int64)
        blk = lp[:Tb, :Ub + 1, blank]
        emit = np.zeros((Tb, Ub + 1))
        for u in range(Ub):
            emit[:, u] = lp[:Tb, u, y[u]]
        emit = masked_emit(emit, Tb, Ub, lo[b], hi[b])
        logZ, cb, ce, w = posteriors(blk, emit, Tb, Ub)
        nll[b] = -logZ if logZ != NEG else np.inf
        g = np.exp(lp[:Tb, :Ub + 1]) * (w + lam * ce)[:, :, None]
        g[:, :, blank] -= cb
        for u in range(Ub):
            g[:, u, y[u]] -= (1.0 + lam) * ce[:, u]
        dz[b, :Tb, :Ub + 1] = g
    return nll, dz


def window_fused(A, C, bias, labels, t_lens, u_lens, blank, lo, hi, lam, gw):
    """The separable form z[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias with per-utterance upstream weights gw:
    -> nll (B,), dA (B,T,V) = gw_b sum_u dz, dC (B,U+1,V) = gw_b sum_t dz.  One utterance at a time."""
    A, C, bias = (np.asarray(x, dtype=np.float64) for x in (A, C, bias))
    B = A.shape[0]
    nll, dA, dC = np.zeros(B), np.zeros_like(A), np.zeros_like(C)
    for b in range(B):
        z = A[b][None, :, None, :] + C[b][None, None, :, :] + bias
        n, dz = window_loss(z, labels[b:b + 1], t_lens[b:b + 1], u_lens[b:b + 1], blank, lo[b:b + 1], hi[b:b + 1], lam)
        nll[b] = n[0]
        dA[b] = float(gw[b]) * dz[0].sum(1)
        dC[b] = float(gw[b]) * dz[0].sum(0)
    return nll, dA, dC


def brute_force_logz(blk, emit, Tb, Ub, lo, hi):
    """log of the sum over EVERY path (one emission frame per label, non-decreasing; Tb blanks) that emits each label inside its
    window, by enumeration: the definition itself, for tiny lattices.  -inf when there is none."""
    terms = []
    for frames in itertools.combinations_with_replacement(range(Tb), Ub):   # non-decreasing emission frames
        if any(not (max(int(lo[u]), 0) <= f <= min(int(hi[u]), Tb - 1)) for u, f in enumerate(frames)):
            continue
        s = sum(emit[f, u] for u, f in enumerate(frames))
        for t in range(Tb):   # the blank of frame t is taken at label position (number of labels emitted at frames <= t)
            s += blk[t, sum(1 for f in frames if f <= t)]
        terms.append(s)
    if not terms:
        return NEG
    m = max(terms)
    return m + np.log(sum(np.exp(x - m) for x in terms))


def diagonal_frames(t_lens, u_lens, U):
    """The tests' reference alignment: frames[b][u] = round(u (Tb - 1) / max(Ub, 1)) for u < Ub, -1 beyond."""
    fr = np.full((len(t_lens), U), -1, dtype=np.int32)
    for b, (Tb, Ub) in enumerate(zip(t_lens, u_lens)):
        for u in range(Ub):
            fr[b, u] = int(round(u * (Tb - 1) / max(Ub, 1)))
    return fr
