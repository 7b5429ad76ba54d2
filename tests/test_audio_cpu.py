"""CPU: the mel-extraction oracle (oracle/audio.py) against its pins — librosa's published known answers for
the Slaney mel scale / filterbank, the committed torch.stft golden, and an independent float64 numpy rfft framing — and
the host-side filterbank of the product (tts_king_amd/audio.py) against the oracle's."""
import os

import numpy as np
import pytest
import torch

from oracle import audio as OA
from tests import mel_ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "mel_extraction.npz"))
N_FFT, HOP, WIN, N_MEL, SR, FMIN, FMAX = (int(v) for v in GOLD["params"])

# librosa.mel_frequencies(n_mels=40) as printed in its docstring (librosa 0.7.2, core/time_frequency.py)
LIBROSA_MEL_FREQS_40 = [0., 85.317, 170.635, 255.952, 341.269, 426.586, 511.904, 597.221, 682.538, 767.855, 853.173, 938.49,
                        1024.856, 1119.114, 1222.042, 1334.436, 1457.167, 1591.187, 1737.532, 1897.337, 2071.84, 2262.393,
                        2470.47, 2697.686, 2945.799, 3216.731, 3512.582, 3835.643, 4188.417, 4573.636, 4994.285, 5453.621,
                        5955.205, 6502.92, 7101.009, 7754.107, 8467.272, 9246.028, 10096.408, 11025.]


def test_mel_frequencies_known_answer():
    got = OA.mel_frequencies(40, 0.0, 11025.0)
    assert np.allclose(got, LIBROSA_MEL_FREQS_40, atol=6e-4)


def test_filterbank_known_answer_and_shape_properties():
    w = OA.mel_filterbank(22050, 2048, 128, 0.0, None)
    assert w.shape == (128, 1025) and w.dtype == np.float32
    assert round(float(w[0][1]), 3) == 0.016 and w[0][0] == 0.0          # librosa.filters.mel docstring: [0., 0.016, ...
    w = OA.mel_filterbank(SR, N_FFT, N_MEL, FMIN, FMAX).astype(np.float64)
    assert (w >= 0).all() and (w.sum(1) > 0).all()
    # Slaney normalisation: every triangle has unit area in Hz (sampled at the FFT bin spacing)
    area = w.sum(1) * (SR / N_FFT)
    assert np.allclose(area[5:], 1.0, atol=0.12)
    # filters above fmax are empty
    assert w[:, int(FMAX / (SR / N_FFT)) + 2:].sum() == 0.0


def test_oracle_matches_golden():
    y = torch.from_numpy(GOLD["y"])
    mel = OA.mel_spectrogram(y, N_FFT, N_MEL, SR, HOP, WIN, FMIN, FMAX)
    assert mel.shape == (2, N_MEL, y.shape[1] // HOP)
    assert np.allclose(mel.numpy(), GOLD["mel_hifi"], atol=1e-5)
    mel_t, energy = OA.tacotron_mel(y, N_FFT, HOP, WIN, N_MEL, SR, FMIN, FMAX)
    assert mel_t.shape == (2, N_MEL, 1 + y.shape[1] // HOP)
    assert np.allclose(mel_t.numpy(), GOLD["mel_taco"], atol=1e-5) and np.allclose(energy.numpy(), GOLD["energy"], rtol=1e-5)


def test_oracle_against_numpy_rfft():
    """Independent float64 restatement: explicit framing + numpy rfft."""
    y = GOLD["y"].astype(np.float64)
    win = torch.hann_window(WIN, dtype=torch.float64).numpy()
    fb = OA.mel_filterbank(SR, N_FFT, N_MEL, FMIN, FMAX).astype(np.float64)
    for pad, eps, key in (((N_FFT - HOP) // 2, 1e-9, "mel_hifi"), (N_FFT // 2, 0.0, "mel_taco")):
        for b in range(y.shape[0]):
            yp = np.pad(y[b], (pad, pad), mode="reflect")
            T = (len(yp) - N_FFT) // HOP + 1
            fr = np.stack([yp[t * HOP: t * HOP + N_FFT] * win for t in range(T)])
            mag2 = np.abs(np.fft.rfft(fr, axis=1)) ** 2
            ref = np.log(np.maximum(fb @ np.sqrt(mag2 + eps).T, 1e-5))
            assert np.abs(ref - GOLD[key][b]).max() < 2e-4
            if key == "mel_taco":
                assert np.allclose(np.sqrt(mag2.sum(1)), GOLD["energy"][b], rtol=1e-4)


def test_product_filterbank_equals_oracle():
    from tts_king_amd.audio import slaney_mel_filterbank
    for args in ((SR, N_FFT, N_MEL, FMIN, FMAX), (22050, 2048, 128, 0.0, None), (16000, 512, 40, 50.0, 7600.0)):
        assert np.array_equal(slaney_mel_filterbank(*args), OA.mel_filterbank(*args)) or \
            np.allclose(slaney_mel_filterbank(*args), OA.mel_filterbank(*args), atol=1e-8)


def test_mel_ref_reproduces_golden():
    """tests/mel_ref.py (the fp64 restatement the GPU envelope tests compare against) at the golden's configuration, within the
    bars test_oracle_against_numpy_rfft uses."""
    args = (N_FFT, HOP, WIN, N_MEL, SR, FMIN, FMAX)
    mel_h = mel_ref.hifi(GOLD["y"], *args)
    mel_t, energy = mel_ref.tacotron(GOLD["y"], *args)
    assert mel_h.shape == GOLD["mel_hifi"].shape and mel_t.shape == GOLD["mel_taco"].shape and energy.shape == GOLD["energy"].shape
    dh, dt = np.abs(mel_h - GOLD["mel_hifi"]).max(), np.abs(mel_t - GOLD["mel_taco"]).max()
    print("mel_ref vs golden: hifi %.2e, tacotron %.2e, energy rel %.2e" % (dh, dt, np.abs(energy / GOLD["energy"] - 1).max()))
    assert dh < 2e-4 and dt < 2e-4
    assert np.allclose(energy, GOLD["energy"], rtol=1e-4)


@pytest.mark.parametrize("cid", sorted(mel_ref.CONFIGS))
def test_mel_ref_against_fp32_oracle(cid):
    """At every configuration of the envelope table, on the broadband input of the GPU tests: the fp32 oracle (torch.stft / conv1d)
    and the fp64 restatement are independent code for the same definition, so they differ by fp32 rounding only.  A broadband
    frame keeps every mel channel within a few decades of its largest bin, where an fp32 FFT of <= 2048 points is good to
    ~log2(n) * 2^-24 of that bin: the bars are this file's own for oracle against golden (log-mel 1e-5 absolute, energy 1e-5
    relative).  Measured: log-mel 4.1e-7 .. 5.6e-6 (the largest at (d), whose lowest filters are a single bin wide), energy 2.2e-7 .. 6.0e-7."""
    cfg = mel_ref.CONFIGS[cid]
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    y = mel_ref.broadband(2, mel_ref.signal_length(n_fft, hop), seed=n_fft + hop)
    yt = torch.from_numpy(y)
    mel_h = mel_ref.hifi(y, *cfg)
    mel_t, energy = mel_ref.tacotron(y, *cfg)
    o_h = OA.mel_spectrogram(yt, n_fft, n_mels, sr, hop, win, fmin, fmax).numpy()
    o_t, o_e = (v.numpy() for v in OA.tacotron_mel(yt, n_fft, hop, win, n_mels, sr, fmin, fmax))
    assert mel_h.shape == o_h.shape == (2, n_mels, y.shape[1] // hop)
    assert mel_t.shape == o_t.shape == (2, n_mels, 1 + y.shape[1] // hop) and energy.shape == o_e.shape
    dh, dt, de = np.abs(mel_h - o_h).max(), np.abs(mel_t - o_t).max(), np.abs(o_e / energy - 1).max()
    print("config %s: fp32 oracle vs fp64: hifi %.2e, tacotron %.2e, energy rel %.2e" % (cid, dh, dt, de))
    assert dh < 1e-5 and dt < 1e-5 and de < 1e-5


def test_product_filterbank_equals_oracle_at_every_envelope_configuration():
    from tts_king_amd.audio import slaney_mel_filterbank
    for n_fft, hop, win, n_mels, sr, fmin, fmax in mel_ref.CONFIGS.values():
        got, ref = slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax), OA.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        assert got.shape == ref.shape == (n_mels, n_fft // 2 + 1) and got.dtype == np.float32
        assert np.array_equal(got, ref) or np.allclose(got, ref, atol=1e-8)
