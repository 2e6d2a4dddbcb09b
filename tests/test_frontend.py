"""Input side: LogMelFrontend on the GPU vs the CPU oracle (oracle/frontend_oracle.py: torch.stft in float64 +
the documented HTK filterbank), SpecAugment properties, and on the CPU: the oracle's own sanity (at the default configuration and at
the ones tests/test_gpu_frontend_kernels.py runs) and the checks LogMelFrontend makes on the host before any device work."""
import math

import numpy as np
import pytest
import torch

from oracle.frontend_oracle import log_mel, melscale_fbanks_htk64


def test_oracle_filterbank_and_tone():
    fb = melscale_fbanks_htk64(201, 0.0, 8000.0, 80, 16000)
    assert fb.shape == (201, 80) and fb.min() >= 0.0 and fb.max() <= 1.0 + 1e-12
    peaks = fb.argmax(0)
    assert np.all(np.diff(peaks) >= 0) and peaks[0] >= 1 and peaks[-1] <= 199  # ordered triangles inside (0, Nyquist)
    assert np.all(fb[0] == 0.0)                                                # DC belongs to no filter (f_min = 0)
    # a pure tone lights up the filter whose triangle contains its frequency
    t = np.arange(16000) / 16000.0
    f0 = 1000.0
    feats = log_mel(np.sin(2 * math.pi * f0 * t))
    assert feats.shape == (1 + 16000 // 160, 80)
    mel_of = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    centre = int(round(mel_of(f0) / mel_of(8000.0) * 81)) - 1
    assert abs(int(feats[50].argmax()) - centre) <= 1


def test_package_filterbank_equals_oracle_constants():
    from rnntransducer_amd.frontend import melscale_fbanks_htk
    got = melscale_fbanks_htk(201, 0.0, 8000.0, 80, 16000).double().numpy()
    assert np.abs(got - melscale_fbanks_htk64(201, 0.0, 8000.0, 80, 16000)).max() < 1e-6


# Other configurations than the default (tests/test_gpu_frontend_kernels.py runs them on the GPU): n_fft = 512 with hop 128 and
# 40 mels, and with hop 160 and 128 mels (257 x 128 filterbank + 16 frames of power: 148032 B of LDS, just under the 160 KiB guard).
OTHER_CONFIGS = [(0.032, 0.008, 40), (0.032, 0.01, 128)]
OTHER_LENGTHS = [257, 258, 4000, 5003]   # one and two samples more than the reflect pad n_fft // 2 = 256, ..., L_max


def other_config_wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    return 0.3 * torch.randn(n, generator=g) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t)) + 0.2 * torch.sin(2 * math.pi * 440.0 * t) + 0.05


@pytest.mark.parametrize("window,stride,n_mels", OTHER_CONFIGS)
def test_oracle_runs_at_the_other_configurations(window, stride, n_mels):
    n_fft, hop = int(math.ceil(16000 * window)), int(16000 * stride)
    assert n_fft == 512 and hop in (128, 160)
    for n in OTHER_LENGTHS:
        feats = log_mel(other_config_wave(n, n).numpy(), window_size_sec=window, window_stride_sec=stride, n_mels=n_mels)
        assert feats.shape == (1 + n // hop, n_mels) and np.isfinite(feats).all() and feats.max() > 0.0
    with pytest.raises(RuntimeError):   # one reflection does not land inside the utterance: torch.stft's reflect pad raises
        log_mel(other_config_wave(256, 1).numpy(), window_size_sec=window, window_stride_sec=stride, n_mels=n_mels)


def test_frontend_refuses_windows_and_strides_the_kernels_cannot_take():
    from rnntransducer_amd.frontend import LogMelFrontend
    with pytest.raises(ValueError, match="n_fft"):
        LogMelFrontend(window_size_sec=0.0255)    # n_fft = 408: not a multiple of 16
    with pytest.raises(ValueError, match="hop"):
        LogMelFrontend(window_stride_sec=0.0101)  # hop = 161: not a multiple of 4
    fe = LogMelFrontend(window_size_sec=0.032, window_stride_sec=0.008, n_mels=40)
    assert (fe.n_fft, fe.hop, fe.n_bins, tuple(fe.fb.shape)) == (512, 128, 257, (257, 40))


def test_python_lengths_are_checked_on_the_host_before_any_device_work():
    """Lengths as a Python sequence (the reference's form): a length outside [0, L_max], or one a single reflection cannot pad
    (0 < L <= n_fft // 2, where the reference's reflect pad raises too), is a ValueError naming the utterance.  The waveform is
    on the CPU here: the check comes before the device is asked for (a good batch on the CPU is refused as a CPU tensor)."""
    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.frontend import LogMelFrontend
    fe = LogMelFrontend()
    wav = torch.zeros(3, 1000)
    for bad, who in (([1000, 1001, 500], "utterance 1"), ([1000, 500, -1], "utterance 2"), ([200, 500, 1000], "utterance 0"),
                     ([1000, 1, 1000], "utterance 1")):
        with pytest.raises(ValueError, match=who):
            fe(wav, bad)
    with pytest.raises(ValueError):
        fe(wav, [1000, 1000])          # two lengths for three utterances
    with pytest.raises(ValueError):
        fe(wav, torch.tensor([1000, 1000]))
    with pytest.raises(RnntHipError):  # lengths 0, n_fft // 2 + 1 and L_max are all fine: only the device is missing
        fe(wav, [0, 201, 1000])


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", [[16000], [4000, 1600, 2399, 400, 241], [48000, 31999]])
def test_log_mel_matches_oracle(lengths):
    from rnntransducer_amd.frontend import LogMelFrontend
    g = torch.Generator().manual_seed(sum(lengths))
    B, Lmax = len(lengths), max(lengths)
    wav = torch.zeros(B, Lmax)
    for b, n in enumerate(lengths):  # speech-like dynamics: noise with a slow envelope, a tone and a DC offset
        t = torch.arange(n) / 16000.0
        wav[b, :n] = (0.3 * torch.randn(n, generator=g) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t)) + 0.2 * torch.sin(2 * math.pi * 440.0 * t) + 0.05)
        wav[b, n:] = 123.0  # garbage beyond the length must be ignored
    fe = LogMelFrontend().cuda()
    feats, nframes = fe(wav.cuda(), lengths)
    assert feats.shape == (B, 1 + Lmax // 160, 80) and nframes.tolist() == [1 + n // 160 for n in lengths]
    for b, n in enumerate(lengths):
        want = log_mel(wav[b, :n].numpy())
        got = feats[b, :nframes[b]].double().cpu().numpy()
        # fp32 DFT (split-bf16 GEMM, fp32 accumulate) vs float64: log1p compresses; absolute tolerance on the features
        assert np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max()), (b, np.abs(got - want).max())
        assert torch.all(feats[b, nframes[b]:] == 0)  # the collate's padding value (dataloader.py:40)
    # un-normalised variant
    raw, _ = LogMelFrontend(normalize=False).cuda()(wav.cuda(), lengths)
    want = log_mel(wav[0, :lengths[0]].numpy(), normalize=False)
    assert np.abs(raw[0, :nframes[0]].double().cpu().numpy() - want).max() < 2e-4 * max(1.0, np.abs(want).max())


@pytest.mark.gpu
def test_spec_augment_properties():
    from rnntransducer_amd.frontend import spec_augment
    gen = torch.Generator(device="cuda").manual_seed(3)
    feats = torch.ones(6, 50, 80, device="cuda")
    lens = torch.tensor([50, 40, 30, 20, 10, 5], dtype=torch.int32, device="cuda")
    out = spec_augment(feats, lens, freq_mask_param=15, time_mask_param=12, freq_mask_cnt=2, time_mask_cnt=2, generator=gen)
    assert out.shape == feats.shape and torch.all((out == 0) | (out == 1))
    for b in range(6):
        z = out[b] == 0
        mel_cols = z.all(0).sum().item()       # fully masked mel bins
        frm_rows = z.all(1).sum().item()       # fully masked frames
        assert mel_cols < 2 * 15 and frm_rows < 2 * 12
        assert not z[lens[b]:].all(1).any() or mel_cols == 80  # time masks stay inside the utterance
    assert torch.equal(spec_augment(feats, lens, 15, 12, 0, 0), feats)
