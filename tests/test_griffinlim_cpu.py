"""CPU: the Griffin-Lim route without a device.  (1) the fp64 restatement tests/griffinlim_ref.py against the reference's own
`pinv` formulation of STFT.inverse and against itself (istft(stft(x)) == x); (2) the bars of tests/test_griffinlim_gpu.py are not
tighter than float32 itself; (3) the loop's spectral convergence falls monotonically; (4) constructor and argument refusals
name their argument; (5) `vocoder=` and `mi355x.vocoder` reach the right object, with stubs in place of the device calls."""
import copy

import numpy as np
import pytest
import torch

from tests import griffinlim_ref as R


def pinv_inverse(mag, phase, n_fft, hop, win):
    """fs_two/audio/stft.py:20-55, 92-137 in float64: pinv(scale * basis), conv_transpose1d, window-sum division, * n_fft / hop, trim."""
    scale = n_fft / hop
    fb = np.fft.fft(np.eye(n_fft))
    cutoff = n_fft // 2 + 1
    fb = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
    w = R.window(n_fft, win)
    inverse_basis = np.linalg.pinv(scale * fb).T * w[None, :]            # (2 * cutoff, n_fft)
    rec = np.concatenate([mag * np.cos(phase), mag * np.sin(phase)], axis=0)      # (2 * cutoff, T)
    T = mag.shape[1]
    y = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        y[t * hop:t * hop + n_fft] += rec[:, t] @ inverse_basis
    s = R.wss(T, n_fft, hop, win)
    ok = s > R.TINY
    y[ok] /= s[ok]
    y *= scale
    return y[n_fft // 2:len(y) - n_fft // 2]


def test_istft_is_the_reference_pinv_formulation():
    cfg = (64, 16, 64)
    r = np.random.RandomState(0)
    mag, phase = r.rand(33, 9) * 3, r.rand(33, 9) * 2 * np.pi - np.pi
    got = R.istft(mag * np.exp(1j * phase), *cfg)
    want = pinv_inverse(mag, phase, *cfg)
    d = float(np.abs(got - want).max())
    print("istft against pinv at (64, 16, 64): %.2e" % d)
    assert got.shape == want.shape == (16 * 8,) and d <= 1e-12


@pytest.mark.parametrize("cfg", [(64, 16, 64), (1024, 256, 1024), (256, 64, 200)])
def test_istft_inverts_stft(cfg):
    n_fft, hop, win = cfg
    T = 24
    x = R.signal(hop * (T - 1), 7).astype(np.float64)
    Z = R.stft(x, *cfg)
    assert Z.shape == (n_fft // 2 + 1, T)
    d = float(np.abs(R.istft(Z, *cfg) - x).max())
    kept = R.wss(T, *cfg)[n_fft // 2:-(n_fft // 2)]
    print("%s: istft(stft(x)) - x %.2e, wss on the kept range >= %.3f" % (cfg, d, kept.min()))
    assert d <= 1e-12 and kept.min() >= 1.08


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_bars_are_not_tighter_than_float32(cfg):
    """The restatement in float32 (radix-2 FFT, twiddles rounded once) meets the GPU tests' bars (A) and (B) with room."""
    n_fft, hop, win = cfg
    for T in (R.min_frames(n_fft, hop), 24):
        x = R.signal(hop * (T - 1), 3)
        Z = R.stft(x, *cfg)
        a = float((np.linalg.norm(R.stft32(x, *cfg) - Z, axis=0) / np.linalg.norm(Z, axis=0)).max())
        b = float((np.abs(R.istft32(Z, *cfg) - R.istft(Z.astype(np.complex64), *cfg)) / R.inverse_bar(Z, *cfg)).max())
        print("%s T %d: float32 transform %.2e of bar %.2e, inverse at %.3f of its bar" % (cfg, T, a, R.transform_bar(n_fft), b))
        assert a <= R.transform_bar(n_fft) and b <= 1.0


COUNTS = (0, 1, 2, 4, 8, 16, 32)


@pytest.mark.parametrize("cfg,T", [((64, 16, 64), 24), ((1024, 256, 1024), 12), ((256, 64, 200), 20)])
def test_loop_converges_monotonically_and_float32_agrees(cfg, T):
    x = R.signal(cfg[1] * (T - 1), 11)
    m = np.abs(R.stft(x, *cfg))
    phase0 = np.random.RandomState(5).rand(*m.shape) * 2 * np.pi
    c64 = [R.convergence(v, m, *cfg) for v in R.griffin_lim(m, phase0, *cfg, 32, keep=COUNTS).values()]
    c32 = [R.convergence(v, m, *cfg) for v in R.griffin_lim32(m, phase0, *cfg, 32, keep=COUNTS).values()]
    print("%s T %d: C fp64 %s, float32 %s" % (cfg, T, ["%.4f" % c for c in c64], ["%.4f" % c for c in c32]))
    assert all(b <= a for a, b in zip(c64, c64[1:])) and c64[0] > 0.5 and c64[-1] < 0.25
    assert all(abs(a - b) <= 5e-4 * a for a, b in zip(c64, c32))


def test_stft_constructor_refusals_name_the_argument():
    from tts_king_amd.audio import STFT
    for args, name in (((1000, 250, 1000), "filter_length"), ((32, 8, 32), "filter_length"), ((4096, 1024, 4096), "filter_length"),
                       ((1024.0, 256, 1024), "filter_length"), ((1024, 300, 1024), "hop_length"), ((1024, 0, 1024), "hop_length"),
                       ((1024, 2048, 1024), "hop_length"), ((1024, 256, 1025), "win_length"), ((1024, 256, 0), "win_length"),
                       ((1024, 256, 1024, "hamming"), "window"), ((1024, 256, 1024, None), "window")):
        with pytest.raises(ValueError, match=name):
            STFT(*args)
    s = STFT(256, 64, 200)
    assert (s.filter_length, s.hop_length, s.win_length, s.nbins, s.min_frames()) == (256, 64, 200, 129, 4)
    assert np.allclose(s._win, R.window(256, 200), atol=6e-8) and s._tw.shape == (128, 2)
    assert np.abs(s._tw.astype(np.float64) - np.stack([np.cos(2 * np.pi * np.arange(128) / 256), -np.sin(2 * np.pi * np.arange(128) / 256)], 1)).max() <= 2.0 ** -24


def test_argument_refusals_name_the_argument():
    from tts_king_amd.audio import STFT, griffin_lim, vocoder_name
    s = STFT(64, 16, 64)
    m = torch.ones(1, 33, 8)
    with pytest.raises(ValueError, match="momentum"):
        griffin_lim(m, s, 2, momentum=1.0)
    with pytest.raises(ValueError, match="momentum"):
        griffin_lim(m, s, 2, momentum=-0.1)
    with pytest.raises(ValueError, match="reflect padding"):
        griffin_lim(torch.ones(1, 33, 3), s, 2)                 # 16 * 2 = 32 samples, the padding itself
    with pytest.raises(ValueError, match="reflect padding"):
        griffin_lim(torch.ones(2, 33, 8), s, 2, lens=[8, 3])
    with pytest.raises(ValueError, match="lens"):
        griffin_lim(torch.ones(2, 33, 8), s, 2, lens=[8, 9])
    with pytest.raises(ValueError, match="magnitudes"):
        griffin_lim(torch.ones(1, 32, 8), s, 2)
    with pytest.raises(ValueError, match="phase0"):
        griffin_lim(m, s, 2, phase0=torch.zeros(1, 33, 7))
    with pytest.raises(ValueError, match="reflect padding"):
        s.transform(torch.zeros(1, 32))
    with pytest.raises(ValueError, match="reflect padding"):
        s.transform(torch.zeros(2, 100), lens=[100, 32])
    with pytest.raises(ValueError, match="input_data"):
        s.transform(torch.zeros(100))
    with pytest.raises(ValueError, match="magnitude and phase"):
        s.inverse(torch.zeros(1, 33, 8), torch.zeros(1, 33, 7))
    with pytest.raises(ValueError, match="vocoder"):
        vocoder_name("wavenet")
    assert vocoder_name(None) == "hifigan" and vocoder_name(None, "griffin_lim") == "griffin_lim"


def _vocoder_config(cfg, **changes):
    """The shipped config with preprocessing.stft / .mel / .audio keys replaced."""
    c = copy.deepcopy(cfg)
    pp = c["preprocess_config"]["preprocessing"]
    for key, value in changes.items():
        group = "stft" if key in pp["stft"] else "mel" if key in pp["mel"] else "audio"
        pp[group][key] = value
    return c


def test_vocoder_envelope_is_the_kernels_not_the_extractors(cfg):
    """GriffinLimVocoder takes every mel width FastSpeech2 takes (up to 1024) and hops that are no multiple of 8: it packs the filterbank
    without building a MelExtractor, whose own limits (80 mels, hop % 8 == 0) still hold for MelExtractor and TacotronSTFT."""
    from tts_king_amd.audio import GriffinLimVocoder, MelExtractor, PackedMelFilterbank, slaney_mel_filterbank
    for changes in (dict(n_mel_channels=128), dict(n_mel_channels=1024, filter_length=2048, hop_length=512, win_length=2048),
                    dict(n_mel_channels=24, filter_length=64, hop_length=4, win_length=48, sampling_rate=8000, mel_fmax=None)):
        v = GriffinLimVocoder(_vocoder_config(cfg, **changes), device="cpu")
        pp = v.cfg["preprocess_config"]["preprocessing"]
        n_mels, n_fft = pp["mel"]["n_mel_channels"], pp["stft"]["filter_length"]
        assert not hasattr(v, "_ex") and isinstance(v.fb, PackedMelFilterbank)
        assert (v.n_mel_channels, v.fb.num_mels, v.fb.nbins, v.stft_fn.filter_length, v.hop) == (n_mels, n_mels, n_fft // 2 + 1, n_fft, pp["stft"]["hop_length"])
        # the pack unpacks to the dense filterbank
        fb = slaney_mel_filterbank(v.sampling_rate, n_fft, n_mels, pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])
        start, off, vals = v.fb.start.numpy(), v.fb.off.numpy(), v.fb.vals.numpy()
        dense = np.zeros_like(fb)
        for m in range(n_mels):
            dense[m, start[m]:start[m] + off[m + 1] - off[m]] = vals[off[m]:off[m + 1]]
        assert start.shape == (n_mels,) and off.shape == (n_mels + 1,) and np.array_equal(dense, fb)
    for bad in (dict(num_mels=128), dict(hop_size=4)):
        with pytest.raises(ValueError, match="MelExtractor"):
            MelExtractor(**dict(dict(n_fft=64, num_mels=20, sampling_rate=8000, hop_size=8, win_size=64, fmin=0, fmax=None, pad=32, eps=0.0,
                                     device="cpu"), **bad))


def test_vocoder_refusals_name_the_config_key(cfg):
    from tts_king_amd.audio import GriffinLimVocoder
    for changes, key in ((dict(n_mel_channels=1032), "mel.n_mel_channels"), (dict(n_mel_channels=0), "mel.n_mel_channels"),
                         (dict(n_mel_channels=80.0), "mel.n_mel_channels"),
                         (dict(filter_length=1000, hop_length=250, win_length=1000), r"preprocessing\.stft.*filter_length"),
                         (dict(hop_length=300), r"preprocessing\.stft.*hop_length"), (dict(win_length=2048), r"preprocessing\.stft.*win_length")):
        with pytest.raises(ValueError, match=key) as e:
            GriffinLimVocoder(_vocoder_config(cfg, **changes), device="cpu")
        assert "GriffinLimVocoder" in str(e.value) and "preprocess_config.preprocessing" in str(e.value) and "MelExtractor" not in str(e.value)


class _Stub:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def __call__(self, x, **kw):
        self.log.append((self.name, "call", tuple(x.shape), kw))
        return "wav"

    def generate(self, x, **kw):
        self.log.append((self.name, "generate", tuple(x.shape), kw))
        return "i16"

    def call_ragged(self, mels, **kw):
        self.log.append((self.name, "call_ragged", len(mels), kw))
        return ["wav"] * len(mels)

    def generate_ragged(self, mels, **kw):
        self.log.append((self.name, "generate_ragged", len(mels), kw))
        return ["i16"] * len(mels)


def _stubbed(monkeypatch, cfg, vocoder=None):
    """A TTSKing whose three back ends are stubs that log their construction and calls."""
    import tts_king
    log = []

    class Tts:
        speaker_names = ["a", "b"]

        def __init__(self, c, gpu):
            log.append(("tts", "init"))

    class Hifi(_Stub):
        def __init__(self, c, gpu):
            _Stub.__init__(self, "hifigan", log)
            log.append(("hifigan", "init"))

    class Griffin(_Stub):
        def __init__(self, c, gpu):
            _Stub.__init__(self, "griffin_lim", log)
            log.append(("griffin_lim", "init"))

    c = copy.deepcopy(cfg)
    if vocoder is not None:
        c.mi355x["vocoder"] = vocoder
    monkeypatch.setattr(tts_king, "load_config", lambda path: c)
    monkeypatch.setattr(tts_king, "FSTWOapi", Tts)
    monkeypatch.setattr(tts_king, "HIFIapi", Hifi)
    monkeypatch.setattr(tts_king, "GriffinLimVocoder", Griffin)
    return tts_king.TTSKing("unused.yaml"), log


def test_vocoder_argument_routes(monkeypatch, cfg):
    t, log = _stubbed(monkeypatch, cfg)
    assert t.vocoder.name == "hifigan" and ("griffin_lim", "init") not in log
    mel = torch.zeros(1, 24, 80)
    del log[:]
    assert t.mel_to_wav(mel) == "i16" and log == [("hifigan", "generate", (1, 80, 24), dict(sample_rate=None))]
    del log[:]
    assert t.mel_to_wav(mel, vocoder="griffin_lim", griffin_iters=7, sample_rate=16000) == "i16"
    assert log == [("griffin_lim", "init"), ("griffin_lim", "generate", (1, 80, 24), dict(sample_rate=16000, griffin_iters=7))]
    del log[:]
    assert t.mel_to_wav([mel, mel], vocoder="griffin_lim") == ["i16", "i16"]
    assert log == [("griffin_lim", "generate_ragged", 2, dict(frames_first=True, sample_rate=None, griffin_iters=60))]
    del log[:]
    assert t.mel_to_wav([mel], vocoder="hifigan") == ["i16"] and log == [("hifigan", "generate_ragged", 1, dict(frames_first=True, sample_rate=None))]
    t.generate_mel = lambda text, *a, **kw: [mel, mel] if isinstance(text, list) else mel
    del log[:]
    assert t.speak("x", vocoder="griffin_lim", griffin_iters=3) == "wav" and t.speak(["x", "y"], vocoder="griffin_lim") == ["wav", "wav"]
    assert t.speak("x") == "wav"
    assert log == [("griffin_lim", "call", (1, 80, 24), dict(sample_rate=None, griffin_iters=3)),
                   ("griffin_lim", "call_ragged", 2, dict(frames_first=True, sample_rate=None, griffin_iters=60)),
                   ("hifigan", "call", (1, 80, 24), dict(sample_rate=None))]
    with pytest.raises(ValueError, match="vocoder"):
        t.mel_to_wav(mel, vocoder="wavenet")


def test_configured_griffin_lim_builds_no_hifigan(monkeypatch, cfg):
    t, log = _stubbed(monkeypatch, cfg, vocoder="griffin_lim")
    assert t.vocoder.name == "griffin_lim" and ("hifigan", "init") not in log
    del log[:]
    assert t.mel_to_wav(torch.zeros(1, 24, 80)) == "i16"
    assert log == [("griffin_lim", "generate", (1, 80, 24), dict(sample_rate=None, griffin_iters=60))]
    with pytest.raises(ValueError, match="vocoder"):
        _stubbed(monkeypatch, cfg, vocoder="melgan")
