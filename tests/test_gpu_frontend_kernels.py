"""The two kernels of csrc/frontend.hip through their C entries, each against float64 at the sizes where its code changes path,
and LogMelFrontend at other configurations than the default one of tests/test_frontend.py.

rnnt_hip_frontend_norm_pad: lengths around the reflect pad and around the 1024-thread stride, NaN beyond every length, a
constant utterance, a large DC offset, lengths outside the row.  rnnt_hip_power_mel_log1p: n_bins / n_mels / row counts off the
thread strides, NaN in every dead frame, the LDS guard.  Every output buffer holds NaN before the call and is one row longer
than needed; that row must stay NaN."""
import numpy as np
import pytest
import torch

from oracle.frontend_oracle import log_mel
from tests.test_frontend import OTHER_CONFIGS, OTHER_LENGTHS, other_config_wave

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24   # unit roundoff of fp32
NAN = float("nan")
LMAX = 1100


def _norm_pad(wav, lens, P, Lp, normalize):
    """wav (B, ld) and lens (B,) int32 on the device -> out (B, Lp)"""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _stream
    B, ld = wav.shape
    buf = torch.full((B + 1, Lp), NAN, device="cuda")
    _lib.check(_lib.lib().rnnt_hip_frontend_norm_pad(wav.data_ptr(), ld, lens.data_ptr(), B, P, Lp, normalize, buf.data_ptr(), _stream()),
               "rnnt_hip_frontend_norm_pad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[B]).all()), "the row after the output was written"
    return buf[:B]


def _norm_pad_ref(x, L, P, Lp, normalize):
    """One row in float64 (datamodule.py:87-90, then np.pad reflect, then zeros) and its per-sample tolerance."""
    row, tol = np.zeros(Lp), np.zeros(Lp)
    if L == 0:
        return row, tol
    v = x[:L].astype(np.float64)
    if normalize:
        m, rstd = v.mean(), 1.0 / np.sqrt(v.var() + 1e-7)
        y = (v - m) * rstd
        # the kernel's mean and rstd are double-accurate and rounded once to fp32 ((|m| + 1 ulp of rstd) u), then x - mean and
        # the product round once each ((|x| + |m|) u each): 4 u (|x| + |m|) rstd covers them
        e = 4 * U32 * (np.abs(v) + abs(m)) * rstd
    else:
        y, e = v, np.zeros(L)   # (x - 0.f) * 1.f is x: bitwise
    row[:L + 2 * P] = np.pad(y, P, mode="reflect")
    tol[:L + 2 * P] = np.pad(e, P, mode="reflect")
    return row, tol


def _waves(P):
    """Rows: the lengths of the issue, then a constant utterance and one with mean 1000 and unit variance; NaN beyond each length."""
    lengths = [P + 1, P + 2, 1023, 1024, 1025, LMAX, 0, 1025, LMAX]
    g = torch.Generator().manual_seed(P)
    wav = 0.3 * torch.randn(len(lengths), LMAX, generator=g) + 0.05
    wav[7] = 0.37
    wav[8] = 1000.0 + torch.randn(LMAX, generator=g)
    for b, n in enumerate(lengths):
        wav[b, n:] = NAN
    return wav, lengths


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("P", [0, 8, 200])
def test_norm_pad_vs_float64(P, normalize):
    wav, lengths = _waves(P)
    Lp = LMAX + 2 * P + 13   # longer than any padded utterance: the tail must be exactly 0
    wav_d, lens_d = wav.cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    got = _norm_pad(wav_d, lens_d, P, Lp, normalize)
    assert torch.equal(got, _norm_pad(wav_d, lens_d, P, Lp, normalize)), "a second run gives other bits"
    got = got.cpu().numpy()
    assert not np.isnan(got).any()
    worst = 0.0
    for b, n in enumerate(lengths):
        want, tol = _norm_pad_ref(wav[b].numpy(), n, P, Lp, normalize)
        err = np.abs(got[b].astype(np.float64) - want)
        if normalize:
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()) if n else 0.0)
            assert (err <= tol).all(), (b, n, float((err - tol).max()))
        else:
            assert np.array_equal(got[b], want.astype(np.float32)), (b, n)
        assert (got[b, (n + 2 * P if n else 0):] == 0).all(), (b, n)
    print(f"P={P} normalize={normalize}: worst |error| / tolerance {worst:.3f}")
    assert (got[6] == 0).all()                   # length 0: all zeros
    if normalize:
        assert (got[7] == 0).all()               # zero variance: x - mean is exactly 0


@pytest.mark.parametrize("normalize", [0, 1])
def test_norm_pad_clamps_lengths_to_the_row(normalize):
    """A device length beyond the row width gives the bits of the full row (it must not read past the row: the last row ends
    the allocation), a negative one the bits of length 0."""
    P, B = 8, 3
    Lp = LMAX + 2 * P + 4
    wav = (0.3 * torch.randn(B, LMAX, generator=torch.Generator().manual_seed(5)) + 0.05).cuda()
    lens = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    want = _norm_pad(wav, lens(LMAX, 0, LMAX), P, Lp, normalize)
    got = _norm_pad(wav, lens(LMAX + 5, -3, 2 ** 31 - 1), P, Lp, normalize)
    assert not bool(torch.isnan(got).any()) and torch.equal(got, want)
    assert bool((got[1] == 0).all())


# (B, F, nframes): M = B * F with M % 16 in {0, 1, 15}, one workgroup and more; nframes of 0, 1 and F
ROWS = [(4, 8, [0, 1, 8, 5]), (3, 11, [11, 0, 1]), (3, 5, [5, 1, 0]), (1, 31, [17])]


def _power_mel(spec, n_bins, fb, n_mels, nframes, F):
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _stream
    M = spec.shape[0]
    buf = torch.full((M + 1, n_mels), NAN, device="cuda")
    _lib.check(_lib.lib().rnnt_hip_power_mel_log1p(spec.data_ptr(), M, n_bins, fb.data_ptr(), n_mels, nframes.data_ptr(), F,
                                                   buf.data_ptr(), _stream()), "rnnt_hip_power_mel_log1p")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[M]).all()), "the row after the output was written"
    return buf[:M]


@pytest.mark.parametrize("n_mels", [1, 15, 16, 17, 80, 128])
@pytest.mark.parametrize("n_bins", [1, 9, 201, 257])
def test_power_mel_log1p_vs_float64(n_bins, n_mels):
    g = torch.Generator().manual_seed(1000 * n_bins + n_mels)
    fb = torch.rand(n_bins, n_mels, generator=g)   # non-negative: every term of the sum is, so the bound is relative
    worst = 0.0
    for B, F, nframes in ROWS:
        spec = 3.0 * torch.randn(B, F, 2 * n_bins, generator=g)
        live = torch.zeros(B, F, dtype=torch.bool)
        for b, n in enumerate(nframes):
            live[b, :n] = True
        spec[~live] = NAN
        got = _power_mel(spec.view(B * F, -1).cuda(), n_bins, fb.cuda(), n_mels, torch.tensor(nframes, dtype=torch.int32, device="cuda"), F)
        got = got.view(B, F, n_mels).double().cpu()
        assert bool((got[~live] == 0).all()), "a dead frame is exactly 0 whatever spec holds there"
        s = spec[live].double()
        acc = (s[:, :n_bins] ** 2 + s[:, n_bins:] ** 2) @ fb.double()
        want = torch.log1p(acc)
        # re^2 + im^2 (three roundings) and n_bins products added in order: |d acc| <= (n_bins + 4) u acc, all terms being
        # non-negative; log1p has slope 1 / (1 + acc); log1pf itself is good to a few ulp of its result
        bound = (n_bins + 4) * U32 * acc / (1 + acc) + 4 * U32 * want.abs()
        err = (got[live] - want).abs()
        assert not bool(torch.isnan(err).any())
        worst = max(worst, (err / bound).max().item())
        assert bool((err <= bound).all()), (B, F, (err / bound).max().item())
    print(f"n_bins={n_bins} n_mels={n_mels}: worst |error| / bound {worst:.3f}")


def test_power_mel_log1p_refuses_tables_beyond_lds():
    n_bins, n_mels, M = 321, 128, 16   # (321 * 128 + 16 * 321) * 4 = 184896 B > 160 KiB
    spec, fb = torch.zeros(M, 2 * n_bins, device="cuda"), torch.zeros(n_bins, n_mels, device="cuda")
    nframes = torch.tensor([M], dtype=torch.int32, device="cuda")
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _stream
    out = torch.full((M, n_mels), NAN, device="cuda")
    with pytest.raises(ValueError, match="does not fit LDS"):
        _lib.check(_lib.lib().rnnt_hip_power_mel_log1p(spec.data_ptr(), M, n_bins, fb.data_ptr(), n_mels, nframes.data_ptr(), M,
                                                       out.data_ptr(), _stream()), "rnnt_hip_power_mel_log1p")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())   # nothing was launched


@pytest.mark.parametrize("window,stride,n_mels", OTHER_CONFIGS)
def test_log_mel_other_configurations_match_oracle(window, stride, n_mels):
    from rnntransducer_amd.frontend import LogMelFrontend
    lengths = OTHER_LENGTHS
    B, Lmax = len(lengths), max(lengths)
    wav = torch.full((B, Lmax), NAN)   # anything beyond a length is ignored
    for b, n in enumerate(lengths):
        wav[b, :n] = other_config_wave(n, n)
    fe = LogMelFrontend(window_size_sec=window, window_stride_sec=stride, n_mels=n_mels).cuda()
    feats, nframes = fe(wav.cuda(), lengths)
    assert feats.shape == (B, 1 + Lmax // fe.hop, n_mels) and nframes.tolist() == [1 + n // fe.hop for n in lengths]
    for b, n in enumerate(lengths):
        want = log_mel(wav[b, :n].numpy(), window_size_sec=window, window_stride_sec=stride, n_mels=n_mels)
        got = feats[b, :nframes[b]].double().cpu().numpy()
        err = np.abs(got - want).max()
        print(f"n_mels={n_mels} hop={fe.hop} L={n}: |features - f64| {err:.2e}")
        assert err < 2e-4 * max(1.0, np.abs(want).max()), (b, err)   # the tolerance of tests/test_frontend.py
        assert torch.all(feats[b, nframes[b]:] == 0)
    # device-tensor lengths: the same bits; one beyond L_max is clamped, frame count included
    dev = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    feats2, nframes2 = fe(wav.cuda(), dev)
    assert torch.equal(feats2, feats) and torch.equal(nframes2, nframes)
    over = dev.clone()
    over[3] = Lmax + 5 * fe.hop
    feats3, nframes3 = fe(wav.cuda(), over)
    assert torch.equal(feats3, feats) and torch.equal(nframes3, nframes)


def test_log_mel_configuration_beyond_lds_is_refused():
    from rnntransducer_amd.frontend import LogMelFrontend
    fe = LogMelFrontend(window_size_sec=0.04, window_stride_sec=0.01, n_mels=128).cuda()   # n_fft 640: 321 bins x 128 mels
    with pytest.raises(ValueError, match="does not fit LDS"):
        fe(torch.zeros(1, 4000, device="cuda"), [4000])
