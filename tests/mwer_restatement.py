"""Plain CPU restatements for MWER training (include/rnnt_hip.h: rnnt_hip_mwer_risk, rnnt_hip_edit_distance), test side, float64.

Risk.  For one utterance with hypotheses i = 0..N-1, nll_i = -log P(y_i | x), W_i token errors, valid_i; over the valid ones:
    P^_i   = softmax_i(-nll_i)                 (the minimum nll subtracted first)
    Wbar   = mean_i W_i
    risk   = sum_i P^_i (W_i - Wbar)
    d risk / d nll_j = -P^_j (W_j - sum_i P^_i W_i)
Invalid rows contribute nothing and get weight exactly 0 (their nll, +inf by convention, never enters the arithmetic); fewer than
two valid rows give risk 0 and weights 0.  `risk_and_weights` is that, written with python floats; `risk_torch` is the same formula
in differentiable torch (no analytic gradient in it: autograd supplies the weights the first one is checked against).

Edit distance.  `edit_distance_prefix_min` restates the kernel's row update: per hypothesis token
    tmp[j] = min(prev[j] + 1, prev[j-1] + (h != r_j)),  tmp[0] = i
    cur[j] = j + min_{k <= j} (tmp[k] - k)
the prefix minimum taken as the kernel takes it: serially inside a lane's 8 columns, then as a scan over the 64 lanes' totals.
"""
import math

import numpy as np
import torch

LANES, COLS = 64, 8
BIG = 1 << 20


def risk_and_weights(nll, W, valid):
    """One utterance: sequences of N numbers / N truth values -> (risk, [weights]) as python floats."""
    idx = [i for i in range(len(nll)) if valid[i]]
    weights = [0.0] * len(nll)
    if len(idx) < 2:
        return 0.0, weights
    mn = min(float(nll[i]) for i in idx)
    if not mn < math.inf:
        return 0.0, weights
    e = {i: math.exp(-(float(nll[i]) - mn)) for i in idx}
    z = math.fsum(e.values())
    p = {i: e[i] / z for i in idx}
    wbar = math.fsum(float(W[i]) for i in idx) / len(idx)
    ew = math.fsum(p[i] * float(W[i]) for i in idx)
    risk = math.fsum(p[i] * (float(W[i]) - wbar) for i in idx)
    for j in idx:
        weights[j] = -p[j] * (float(W[j]) - ew)
    return risk, weights


def risk_batch(nll, W, valid):
    """(B, N) arrays -> risk (B,) float64, weights (B, N) float64."""
    nll, W, valid = np.asarray(nll, dtype=np.float64), np.asarray(W), np.asarray(valid)
    out = [risk_and_weights(list(n), list(w), list(v)) for n, w, v in zip(nll, W, valid)]
    return np.array([r for r, _ in out], dtype=np.float64), np.array([w for _, w in out], dtype=np.float64).reshape(W.shape)


def risk_torch(nll: torch.Tensor, W: torch.Tensor, valid) -> torch.Tensor:
    """The formula on the valid entries of one utterance, differentiable in nll (float64)."""
    idx = [i for i in range(nll.numel()) if valid[i]]
    if len(idx) < 2:
        return nll.sum() * 0.0
    sel = torch.tensor(idx, dtype=torch.long)
    x, w = nll[sel], W[sel].to(torch.float64)
    p = torch.softmax(-(x - x.min().detach()), dim=0)
    return (p * (w - w.mean())).sum()


def risk_brute_force(nll, W):
    """All rows valid, probabilities formed directly (no shift): only for small, well-scaled hand-made cases."""
    p = [math.exp(-x) for x in nll]
    z = sum(p)
    wbar = sum(W) / len(W)
    return sum(pi / z * (wi - wbar) for pi, wi in zip(p, W))


def edit_distance_prefix_min(hyp, ref) -> int:
    """The kernel's DP, with the in-row dependency as a two-level prefix minimum over 64 lanes x 8 columns."""
    H, R = len(hyp), len(ref)
    assert H < LANES * COLS and R < LANES * COLS
    n = LANES * COLS
    j = np.arange(n, dtype=np.int64)
    rtok = np.full(n, -(1 << 40), dtype=np.int64)      # a column outside the reference never matches
    rtok[1:R + 1] = np.asarray(ref, dtype=np.int64)
    prev = j.copy()
    for i in range(1, H + 1):
        h = int(hyp[i - 1])
        left = np.concatenate(([BIG], prev[:-1]))       # prev[j - 1]
        tmp = np.minimum(prev + 1, left + (rtok != h))
        tmp[0] = i
        v = np.minimum.accumulate((tmp - j).reshape(LANES, COLS), axis=1)           # serial part inside a lane
        inc = np.minimum.accumulate(v[:, -1])                                        # scan over the lanes' totals
        exc = np.concatenate(([BIG], inc[:-1]))                                      # the lanes below
        prev = np.minimum(np.minimum(v, exc[:, None]).reshape(n) + j, BIG)
    return int(prev[R])
