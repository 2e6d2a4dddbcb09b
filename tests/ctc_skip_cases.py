"""Shared inputs of the CTC frame-skipping tests (tests/test_ctc_skip_oracle.py on the CPU, tests/test_gpu_ctc_skip.py on the device).

Logits with a known blank posterior: z = 2 N(0,1) in fp32, then z[..., blank] = logsumexp(non-blank z) + u with u ~ U(-1, 5), so the
blank posterior of a frame is sigmoid(u) and a threshold p skips the share P(u > logit p) of the frames: 0.47 at p = 0.9, 0.83 at
p = 0.5, 0.07 at p = 0.99.

TOL = 1e-5 absolute on the blank log-posterior: what the alignment tests allow the same fp32 per-frame terms against a float64
log-softmax.  A frame is DECIDED at threshold p when |lp64 - log p| > 2 TOL: the device's fp32 value is then on the same side of
the threshold as the float64 one, and the keep bit must agree with the restatement."""
import math

import numpy as np

TOL = 1e-5
# (B, T, V, blank, O)
SHAPES = [(3, 33, 2, 0, 6),        # O % 4 != 0: the 4-byte copy; one row with t_len = 0
          (2, 31, 5, 4, 8),        # one tile, not full; the blank is the last entry
          (1, 1, 3, 1, 4),         # one frame
          (4, 64, 65, 0, 512),     # V one past the wavefront; two full tiles
          (3, 97, 72, 0, 128),     # four tiles, the last with one frame
          (2, 40, 2048, 7, 16),    # 32 values per lane
          (1, 2081, 3, 1, 4)]      # 66 tile words: the gather's sum strides over more than one wavefront of them
PS = (0.5, 0.9, 1.0)


def case_id(shape):
    return "B%d-T%d-V%d-blank%d-O%d" % shape


def t_lens_of(shape):
    """Ragged frame counts: row 0 is full, the others U{T/2 .. T}; the first shape's last row has no frames."""
    B, T = shape[:2]
    rng = np.random.default_rng(1000 + SHAPES.index(shape))
    lens = [T] + [int(x) for x in rng.integers(max(1, T // 2), T + 1, size=B - 1)]
    if shape == SHAPES[0]:
        lens[-1] = 0
    return np.asarray(lens, dtype=np.int32)


def logits_of(shape):
    """(B, T, V) fp32, batch-major."""
    B, T, V, blank, _ = shape
    rng = np.random.default_rng(2000 + SHAPES.index(shape))
    z = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    nb = np.delete(z.astype(np.float64), blank, axis=-1)
    m = nb.max(-1)
    lse = m + np.log(np.exp(nb - m[..., None]).sum(-1))
    z[..., blank] = (lse + rng.uniform(-1.0, 5.0, size=(B, T))).astype(np.float32)
    return z


def enc_of(shape):
    """(T, B, O) fp32, time-major: every row distinct."""
    B, T, _, _, O = shape
    rng = np.random.default_rng(3000 + SHAPES.index(shape))
    return rng.standard_normal((T, B, O)).astype(np.float32)


def valid_mask(shape):
    B, T = shape[:2]
    return np.arange(T)[None, :] < t_lens_of(shape)[:, None]


def decided(lp64, p):
    return np.abs(lp64 - math.log(p)) > 2 * TOL
