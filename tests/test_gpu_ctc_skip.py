"""rnnt_hip_ctc_frame_skip (csrc/ctc_skip.hip) through the C entry and through ops.ctc_frame_skip, against the float64 restatement
(tests/ctc_skip_restatement.py) on the shared cases (tests/ctc_skip_cases.py).

blank_logp is held to TOL = 1e-5 of float64.  Everything else is exact: the keep decision is a pure function of the returned
blank_logp (lp > float32(log p)), it equals the restatement's on every decided frame, the map lists the kept frames in order, the
compacted rows are bitwise the originals, and a row alone gives the bits it gives in its batch."""
import math

import numpy as np
import pytest
import torch

from tests import ctc_skip_cases as K
from tests.ctc_skip_restatement import frame_skip

pytestmark = pytest.mark.gpu
_REF = {}


def _reference(shape, p):
    """The float64 restatement of a case, computed once and shared."""
    if (shape, p) not in _REF:
        _REF[shape, p] = frame_skip(K.logits_of(shape), K.t_lens_of(shape), shape[3], p)
    return _REF[shape, p]


def _entry(z, z_sb, z_st, t_lens, B, T, V, blank, p, enc_tm, want_lp=True, ws_extra=0):
    """The C entry on device tensors: z any layout through (z_sb, z_st), enc_tm (T, B, O) contiguous -> (enc_out, new_lens,
    frame_map, blank_logp); blank_logp pre-filled with NaN so that unwritten entries show."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr, _stream, check, check_ctc_skip
    L, O, dev = _lib.lib(), enc_tm.shape[2], enc_tm.device
    out = torch.full_like(enc_tm, float("nan"))
    new_lens = torch.full((B,), -7, device=dev, dtype=torch.int32)
    frame_map = torch.full((B, T), -7, device=dev, dtype=torch.int32)
    lp = torch.full((B, T), float("nan"), device=dev, dtype=torch.float32) if want_lp else None
    nws = L.rnnt_hip_ctc_frame_skip_workspace_bytes(B, T)
    ws = torch.empty(nws + ws_extra, device=dev, dtype=torch.uint8)
    check(L.rnnt_hip_ctc_frame_skip(_addr(z), z_sb, z_st, _addr(t_lens), B, T, V, blank, check_ctc_skip(p, "test"), _addr(enc_tm), O,
                                    B * O, O, _addr(out), O, B * O, _addr(new_lens), _addr(frame_map), _addr(lp), _addr(ws), nws,
                                    _stream()), "rnnt_hip_ctc_frame_skip")
    return out, new_lens, frame_map, lp


def _check(shape, p, t_lens, enc, out, new_lens, frame_map, lp_dev):
    """Every property of one result, on host arrays: enc / out (T, B, O), lp_dev (B, T)."""
    B, T = shape[:2]
    lp64, keep64, _, _ = _reference(shape, p)
    valid = np.arange(T)[None, :] < t_lens[:, None]
    err = np.abs(lp_dev.astype(np.float64) - lp64)[valid]
    print(f"{K.case_id(shape)} p={p}: max |blank_logp - float64| = {err.max() if err.size else 0.0:.3e}")
    assert (err < K.TOL).all()
    log_p = np.float32(math.log(p))
    keep = valid & ~(lp_dev > log_p)                       # a pure function of the returned values
    dec = K.decided(lp64, p) & valid
    assert np.array_equal(keep[dec], keep64[dec])
    for b in range(B):
        kept = np.nonzero(keep[b])[0]
        n = len(kept)
        assert new_lens[b] == n
        assert np.array_equal(frame_map[b, :n], kept) and (frame_map[b, n:] == -1).all()
        assert (np.diff(frame_map[b, :n]) > 0).all()
        assert np.array_equal(out[:n, b].view(np.uint32), enc[kept, b].view(np.uint32))
    if p == 1.0:
        assert np.array_equal(new_lens, t_lens)


@pytest.mark.parametrize("p", K.PS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.case_id)
def test_frame_skip_matches_the_restatement(shape, p):
    """ops.ctc_frame_skip on time-major logits and the C entry on batch-major logits: both checked, and bitwise equal."""
    from rnntransducer_amd.ops import ctc_frame_skip
    B, T, V, blank, O = shape
    z, t_lens, enc = K.logits_of(shape), K.t_lens_of(shape), K.enc_of(shape)
    zd, td, ed = torch.from_numpy(z).cuda(), torch.from_numpy(t_lens).cuda(), torch.from_numpy(enc).cuda()
    res = ctc_frame_skip(zd.transpose(0, 1).contiguous(), td, blank, p, ed, return_blank_logp=True)
    got = [x.cpu().numpy() for x in (res.enc, res.t_lens, res.frame_map, res.blank_logp)]
    _check(shape, p, t_lens, enc, *got)
    raw = [x.cpu().numpy() for x in _entry(zd, T * V, V, td, B, T, V, blank, p, ed)]
    _check(shape, p, t_lens, enc, *raw)
    valid = K.valid_mask(shape)
    assert np.array_equal(raw[3][valid].view(np.uint32), got[3][valid].view(np.uint32))
    assert np.array_equal(raw[1], got[1]) and np.array_equal(raw[2], got[2])
    assert np.isnan(raw[3][~valid]).all()                  # blank_logp past a row's frames is not written
    for b in range(B):                                     # nor are the rows behind the kept frames
        assert np.isnan(raw[0][raw[1][b]:, b]).all()
    assert res.blank_logp is not None and ctc_frame_skip(zd.transpose(0, 1).contiguous(), td, blank, p, ed).blank_logp is None


@pytest.mark.parametrize("shape", [K.SHAPES[0], K.SHAPES[3], K.SHAPES[4]], ids=K.case_id)
def test_each_row_alone_gives_its_batch_bits(shape):
    B, T, V, blank, O = shape
    p = 0.9
    zd, td, ed = (torch.from_numpy(x).cuda() for x in (K.logits_of(shape), K.t_lens_of(shape), K.enc_of(shape)))
    out, new_lens, frame_map, lp = (x.cpu().numpy() for x in _entry(zd, T * V, V, td, B, T, V, blank, p, ed))
    for b in range(B):
        one = _entry(zd[b:b + 1].contiguous(), T * V, V, td[b:b + 1].contiguous(), 1, T, V, blank, p, ed[:, b:b + 1].contiguous())
        o1, n1, f1, l1 = (x.cpu().numpy() for x in one)
        assert n1[0] == new_lens[b] and np.array_equal(f1[0], frame_map[b])
        assert np.array_equal(l1[0].view(np.uint32), lp[b].view(np.uint32))
        assert np.array_equal(o1[:, 0].view(np.uint32), out[:, b].view(np.uint32))


def test_padding_is_never_read():
    """Padded logits and padded enc rows set to NaN: the result is the clean one's, bit for bit."""
    shape, p = K.SHAPES[4], 0.9
    B, T, V, blank, O = shape
    z, t_lens, enc = K.logits_of(shape).copy(), K.t_lens_of(shape), K.enc_of(shape).copy()
    valid = K.valid_mask(shape)
    assert (~valid).any()
    td = torch.from_numpy(t_lens).cuda()
    clean = [x.cpu().numpy() for x in _entry(torch.from_numpy(z).cuda(), T * V, V, td, B, T, V, blank, p, torch.from_numpy(enc).cuda())]
    z[~valid] = np.nan
    enc[(~valid).T] = np.nan
    dirty = [x.cpu().numpy() for x in _entry(torch.from_numpy(z).cuda(), T * V, V, td, B, T, V, blank, p, torch.from_numpy(enc).cuda())]
    _check(shape, p, t_lens, K.enc_of(shape), *dirty)
    for a, b in zip(clean, dirty):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.isnan(dirty[0][:1]).any()


def test_time_major_logits_with_a_wide_row_stride():
    """Time-major logits whose rows are wider than V, the padding columns at 1e30: only the V entries count."""
    shape, p = K.SHAPES[1], 0.9
    B, T, V, blank, O = shape
    z, t_lens, enc = K.logits_of(shape), K.t_lens_of(shape), K.enc_of(shape)
    wide = np.full((T, B, V + 3), 1e30, dtype=np.float32)
    wide[:, :, :V] = z.transpose(1, 0, 2)
    got = _entry(torch.from_numpy(wide).cuda(), V + 3, B * (V + 3), torch.from_numpy(t_lens).cuda(), B, T, V, blank, p,
                 torch.from_numpy(enc).cuda())
    _check(shape, p, t_lens, enc, *(x.cpu().numpy() for x in got))


def test_a_nan_row_is_kept_and_no_blank_logp_is_fine():
    shape, p = K.SHAPES[1], 0.5
    B, T, V, blank, O = shape
    z, t_lens, enc = K.logits_of(shape).copy(), K.t_lens_of(shape), K.enc_of(shape)
    lp64, keep64, _, _ = _reference(shape, p)
    t = int(np.nonzero(~keep64[0, :t_lens[0]])[0][0])      # a frame the clean logits skip
    z[0, t, 0] = np.nan
    out, new_lens, frame_map, lp = _entry(torch.from_numpy(z).cuda(), T * V, V, torch.from_numpy(t_lens).cuda(), B, T, V, blank, p,
                                          torch.from_numpy(enc).cuda(), want_lp=False)
    assert lp is None
    fm = frame_map.cpu().numpy()
    assert t in fm[0, :int(new_lens[0])].tolist() and int(new_lens[0]) == keep64[0].sum() + 1
    assert np.array_equal(fm[1], _reference(shape, p)[2][1])
