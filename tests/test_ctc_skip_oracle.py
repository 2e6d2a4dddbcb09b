"""The float64 restatement of CTC frame skipping (tests/ctc_skip_restatement.py) against torch.log_softmax in float64, and the
properties of the shared cases (tests/ctc_skip_cases.py) that the device tests rely on: nearly every frame is decided at each
threshold, and p = 0.9 skips between 30 % and 70 % of the valid frames.  No device here."""
import math

import numpy as np
import pytest
import torch

from tests import ctc_skip_cases as K
from tests.ctc_skip_restatement import blank_logp, frame_skip


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.case_id)
def test_restatement_is_the_float64_log_softmax(shape):
    z, blank = K.logits_of(shape), shape[3]
    ref = torch.log_softmax(torch.from_numpy(z).double(), -1)[..., blank].numpy()
    assert np.abs(blank_logp(z, blank) - ref).max() < 1e-12


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.case_id)
def test_keep_map_and_lengths_restate_the_rule(shape):
    B, T, _, blank, _ = shape
    z, t_lens, valid = K.logits_of(shape), K.t_lens_of(shape), K.valid_mask(shape)
    ref = torch.log_softmax(torch.from_numpy(z).double(), -1)[..., blank].numpy()
    for p in K.PS + (0.99,):
        lp, keep, frame_map, new_lens = frame_skip(z, t_lens, blank, p)
        assert np.array_equal(keep, valid & ~(ref > math.log(p)))
        for b in range(B):
            kept = np.nonzero(keep[b])[0]
            assert new_lens[b] == len(kept) and np.array_equal(frame_map[b, :len(kept)], kept)
            assert (frame_map[b, len(kept):] == -1).all()
        if p == 1.0:   # lp > 0 never holds
            assert np.array_equal(keep, valid) and np.array_equal(new_lens, t_lens)


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.case_id)
def test_cases_are_decided_and_skip_about_half(shape):
    """At most 1 frame in 100 undecided at every threshold; at p = 0.9 the skipped share of the valid frames lies in [0.3, 0.7].
    The share is asserted for every case with more than one valid frame: with a single frame (the (1, 1, 3, 1, 4) case) it can only
    be 0 or 1."""
    z, t_lens, blank, valid = K.logits_of(shape), K.t_lens_of(shape), shape[3], K.valid_mask(shape)
    n = int(valid.sum())
    for p in (0.5, 0.9, 0.99):
        lp, keep, _, new_lens = frame_skip(z, t_lens, blank, p)
        undecided = int((~K.decided(lp, p))[valid].sum())
        print(f"{K.case_id(shape)} p={p}: {n} valid frames, skipped {1 - new_lens.sum() / n:.3f}, undecided {undecided}")
        assert undecided <= n / 100
        if p == 0.9 and n > 1:
            assert 0.3 <= 1 - new_lens.sum() / n <= 0.7


def test_a_nan_row_is_kept():
    z = K.logits_of(K.SHAPES[1]).copy()
    z[0, 3, 1] = np.nan
    _, keep, _, _ = frame_skip(z, K.t_lens_of(K.SHAPES[1]), 4, 0.5)
    assert keep[0, 3]
