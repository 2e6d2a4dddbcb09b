"""FastEmit-regularised RNN-T loss in float64 numpy, written from the definition (include/rnnt_hip.h), for the tests.

Per lattice cell (t,u) of an utterance with Tb frames and Ub labels (cells t < Tb, u <= Ub), with blk / emit the log-softmax values of
the blank and of label y_u, alpha / beta the forward / backward log-sums and logZ = log P(y|x):
    cb(t,u) = exp(alpha + blk + beta(t+1,u) - logZ)      (at t = Tb-1: exp(alpha + blk - logZ) for u = Ub, else 0)
    ce(t,u) = exp(alpha + emit + beta(t,u+1) - logZ)     (0 at u = Ub)
    w(t,u)  = exp(alpha + beta - logZ) = cb + ce
    dz[t,u,v] = softmax_v (w + lam ce) - [v = blank] cb - [v = y_u] (1 + lam) ce
The returned NLL is -logZ whatever lam is.  Nothing here is shared with the library or with oracle/."""
import numpy as np

NEG = -np.inf


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def alpha_beta(blk, emit, Tb, Ub):
    """blk, emit (T, U+1) float64 -> alpha, beta (Tb, Ub+1) and logZ."""
    a = np.full((Tb, Ub + 1), NEG)
    b = np.full((Tb, Ub + 1), NEG)
    a[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            down = a[t - 1, u] + blk[t - 1, u] if t > 0 else NEG
            left = a[t, u - 1] + emit[t, u - 1] if u > 0 else NEG
            a[t, u] = np.logaddexp(down, left)
    b[Tb - 1, Ub] = blk[Tb - 1, Ub]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                continue
            nb = b[t + 1, u] + blk[t, u] if t < Tb - 1 else NEG
            ne = b[t, u + 1] + emit[t, u] if u < Ub else NEG
            b[t, u] = np.logaddexp(nb, ne)
    return a, b, b[0, 0]


def cell_posteriors(blk, emit, Tb, Ub):
    """-> logZ, cb, ce, w (each (Tb, Ub+1))."""
    a, b, logZ = alpha_beta(blk, emit, Tb, Ub)
    bl, em = blk[:Tb, :Ub + 1], emit[:Tb, :Ub + 1]
    b_next_t = np.full((Tb, Ub + 1), NEG)
    b_next_t[:-1] = b[1:]
    b_next_t[Tb - 1, Ub] = 0.0                      # the final blank leaves the lattice
    b_next_u = np.full((Tb, Ub + 1), NEG)
    b_next_u[:, :-1] = b[:, 1:]
    with np.errstate(invalid="ignore"):
        cb = np.exp(a + bl + b_next_t - logZ)
        ce = np.exp(a + em + b_next_u - logZ)
        w = np.exp(a + b - logZ)
    ce[:, Ub] = 0.0
    return logZ, np.nan_to_num(cb), np.nan_to_num(ce), np.nan_to_num(w)


def fastemit_loss(z, labels, t_lens, u_lens, blank, lam):
    """z (B,T,U+1,V) logits, labels (B,U) -> nll (B,), dz (B,T,U+1,V) float64: d/dz of the FastEmit surrogate, zeros outside each
    utterance's lattice.  t_lens[b] = 0: nll = +inf and a zero gradient (the library's rule)."""
    z = np.asarray(z, dtype=np.float64)
    B, T, U1, V = z.shape
    nll = np.zeros(B)
    dz = np.zeros_like(z)
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        if Tb == 0:
            nll[b] = np.inf
            continue
        lp = log_softmax(z[b])
        y = np.asarray(labels[b][:U1 - 1], dtype=np.int64) if U1 > 1 else np.zeros(0, dtype=np.int64)
        blk = lp[:, :, blank]
        emit = np.zeros((T, U1))
        if U1 > 1:
            emit[:, :U1 - 1] = np.take_along_axis(lp[:, :U1 - 1, :], y[None, :, None], axis=2)[:, :, 0]
        logZ, cb, ce, w = cell_posteriors(blk, emit, Tb, Ub)
        nll[b] = -logZ
        g = np.exp(lp[:Tb, :Ub + 1]) * (w + lam * ce)[:, :, None]
        g[:, :, blank] -= cb
        for u in range(Ub):
            g[:, u, y[u]] -= (1.0 + lam) * ce[:, u]
        dz[b, :Tb, :Ub + 1] = g
    return nll, dz


def fastemit_fused(A, C, bias, labels, t_lens, u_lens, blank, lam, gw):
    """The separable form z[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias with per-utterance upstream weights gw:
    -> nll (B,), dA (B,T,V) = gw_b sum_u dz, dC (B,U+1,V) = gw_b sum_t dz.  One utterance at a time (no (B,T,U+1,V) array)."""
    A, C, bias = (np.asarray(x, dtype=np.float64) for x in (A, C, bias))
    B = A.shape[0]
    nll, dA, dC = np.zeros(B), np.zeros_like(A), np.zeros_like(C)
    for b in range(B):
        z = A[b][None, :, None, :] + C[b][None, None, :, :] + bias
        n, dz = fastemit_loss(z, labels[b:b + 1], t_lens[b:b + 1], u_lens[b:b + 1], blank, lam)
        nll[b] = n[0]
        dA[b] = float(gw[b]) * dz[0].sum(1)
        dC[b] = float(gw[b]) * dz[0].sum(0)
    return nll, dA, dC


def viterbi_frames(z, labels, Tb, Ub, blank):
    """Best-path frame of every label of one utterance (z (T,U+1,V)); on exactly equal candidates the blank predecessor wins."""
    lp = log_softmax(z)
    v = np.full((Tb, Ub + 1), NEG)
    bp = np.zeros((Tb, Ub + 1), dtype=bool)
    v[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            down = v[t - 1, u] + lp[t - 1, u, blank] if t > 0 else NEG
            left = v[t, u - 1] + lp[t, u - 1, labels[u - 1]] if u > 0 else NEG
            bp[t, u] = left > down
            v[t, u] = left if bp[t, u] else down
    frames, t, u = [0] * Ub, Tb - 1, Ub
    while u > 0:
        if bp[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    return frames
