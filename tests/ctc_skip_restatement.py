"""float64 numpy restatement of rnnt_hip_ctc_frame_skip (include/rnnt_hip.h): the blank log-posterior per frame, the keep decision,
the frame map and the new lengths.  Loops, no vectorised tricks beyond the log-sum-exp."""
import math

import numpy as np


def blank_logp(z, blank):
    """z (..., V) -> z[..., blank] - logsumexp(z) in float64, the row maximum subtracted."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1)
    return z[..., blank] - (m + np.log(np.exp(z - m[..., None]).sum(-1)))


def frame_skip(z, t_lens, blank, p):
    """z (B, T, V), t_lens (B,), threshold p in (0, 1] -> lp (B, T) float64, keep (B, T) bool (False for t >= T_b), frame_map
    (B, T) int (-1 behind the kept frames), new_lens (B,).  A frame is skipped exactly when lp > log p."""
    B, T, _ = z.shape
    lp = blank_logp(z, blank)
    log_p = math.log(p)
    keep = np.zeros((B, T), dtype=bool)
    frame_map = np.full((B, T), -1, dtype=np.int64)
    new_lens = np.zeros(B, dtype=np.int64)
    for b in range(B):
        Tb = min(max(int(t_lens[b]), 0), T)
        j = 0
        for t in range(Tb):
            if not lp[b, t] > log_p:
                keep[b, t] = True
                frame_map[b, j] = t
                j += 1
        new_lens[b] = j
    return lp, keep, frame_map, new_lens
