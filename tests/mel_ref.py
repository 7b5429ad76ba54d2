"""fp64 restatement of mel extraction (tts_king_amd/audio.py), in plain numpy: reflect pad, explicit framing, periodic Hann of
`win` centre-padded to `n_fft`, `np.fft.rfft`, sqrt(re^2 + im^2 + eps), the oracle's mel filterbank in float64, log(max(., 1e-5)),
energy = sqrt(sum(re^2 + im^2)).  Two call forms: `hifi` (pad (n_fft - hop)//2, eps 1e-9: hifi/meldataset.py) and `tacotron`
(pad n_fft//2, eps 0, energy too: fs_two/audio/stft.py).  Plus what the two kernels either side of the STFT contraction are held
to on their own: `stft_rows` (ttsk_stft_frames, exact), `mel_from_spec` (ttsk_mel_from_spec from a given spec and packed table) and
`pack` (the packed filterbank as `MelExtractor.__init__` builds it).  Test infrastructure: shared by tests/test_audio_cpu.py and
tests/test_mel_envelope_gpu.py, which also take the configuration table and the two input makers from here."""
import numpy as np

from oracle import audio as OA

CLIP = 1e-5

# (n_fft, hop, win, n_mels, sr, fmin, fmax) and what each reaches in the kernels
CONFIGS = {
    "a": (2048, 512, 2048, 80, 48000, 0, None),        # mel_from_spec<17> at nbins 1025, fmax=None
    "b": (2048, 256, 1200, 80, 44100, 20, 16000),      # <17>, win < n_fft, 8 taps
    "c": (512, 128, 512, 40, 16000, 50, 7600),         # fewer than 64 filters
    "d": (256, 64, 256, 80, 8000, 0, 4000),            # one- and two-bin filters, K = 192
    "e": (1024, 256, 800, 64, 22050, 0, 8000),         # exactly 64 filters, win < n_fft
    "f": (1024, 128, 1024, 65, 24000, 1500, 12000),    # one filter on the four-lane half, fmin in the log region
    "g": (1024, 32, 1024, 80, 22050, 0, 8000),         # 32 taps
    "h": (1152, 128, 1152, 80, 22050, 0, 8000),        # nbins 577, the first size on <17>; 9 taps
    "i": (1144, 88, 1144, 80, 22050, 0, 8000),         # nbins 573, the last sizes on <9>; hop not a power of two; 13 taps
}


def signal_length(n_fft, hop):
    """hop*37 + 11 samples, and at least n_fft + hop (+ 11: never a multiple of the hop)."""
    return max(hop * 37 + 11, n_fft + hop + 11)


def broadband(Bsz, n, seed):
    """(rand*2 - 1) * linspace(1, 0.001): the envelope tests/test_audio_gpu.py::test_vs_oracle_ragged_sizes uses.  (B, n) float32."""
    r = np.random.RandomState(seed)
    return ((r.rand(Bsz, n) * 2 - 1) * np.linspace(1.0, 0.001, n)[None, :]).astype(np.float32)


def tonal(n, sr, seed, floor=1e-2):
    """Row 0: 0.5 sin(2 pi 440 t) + 0.2 sin(2 pi 1320 t + 1); row 1: a 0.9 square wave at 211 Hz; uniform noise of amplitude `floor` on
    both, clamped to [-1, 1].  (2, n) float32."""
    r = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / sr
    y = np.stack([0.5 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1320 * t + 1.0),
                  0.9 * np.where(np.sin(2 * np.pi * 211 * t) >= 0, 1.0, -1.0)])
    y += floor * (r.rand(2, n) * 2 - 1)
    return np.clip(y, -1.0, 1.0).astype(np.float32)


def reflect_index(n, pad):
    """Source index of every sample of a length-n signal reflect-padded by `pad` < n on both sides (edge sample not repeated)."""
    assert 0 <= pad < n
    j = np.abs(np.arange(-pad, n + pad))
    return np.where(j >= n, 2 * (n - 1) - j, j)


def window(n_fft, win):
    """Periodic Hann of `win`, centre-padded to n_fft (oracle/audio.py:fourier_basis, torch.stft)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    lpad = (n_fft - win) // 2
    return np.pad(w, (lpad, n_fft - win - lpad))


def power_spectrum(y, n_fft, hop, win, pad):
    """y (B, L) -> re^2 + im^2, float64 (B, T, n_fft//2 + 1), T = 1 + (L + 2 pad - n_fft) // hop."""
    y = np.asarray(y, dtype=np.float64)
    yp = y[:, reflect_index(y.shape[1], pad)]
    T = 1 + (yp.shape[1] - n_fft) // hop
    assert T >= 1
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(yp[:, idx] * window(n_fft, win), axis=2)
    return spec.real ** 2 + spec.imag ** 2


def _log_mel(p, eps, n_fft, n_mels, sr, fmin, fmax):
    fb = OA.mel_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(np.float64)
    return np.log(np.maximum(np.einsum("mk,btk->bmt", fb, np.sqrt(p + eps)), CLIP))


def hifi(y, n_fft, hop, win, n_mels, sr, fmin, fmax):
    """hifi/meldataset.py:49-74 -> log-mel (B, n_mels, L // hop), float64."""
    return _log_mel(power_spectrum(y, n_fft, hop, win, (n_fft - hop) // 2), 1e-9, n_fft, n_mels, sr, fmin, fmax)


def tacotron(y, n_fft, hop, win, n_mels, sr, fmin, fmax):
    """fs_two/audio/stft.py -> (log-mel (B, n_mels, 1 + L // hop), energy (B, 1 + L // hop)), float64."""
    p = power_spectrum(y, n_fft, hop, win, n_fft // 2)
    return _log_mel(p, 0.0, n_fft, n_mels, sr, fmin, fmax), np.sqrt(p.sum(axis=2))


def stft_rows(x, pad, rows, hop, scale):
    """ttsk_stft_frames, exactly: x (B, len) float32 -> float16 (B, rows, 3*hop) = [hi | hi | lo] per hop block.  Reflect padding,
    zeros from index len + 2 pad on, v = float32(x) * float32(scale), hi = float16(v), lo = float16(v - float32(hi)).  numpy's
    float16 cast rounds to nearest even and keeps subnormals, as __float2half_rn does."""
    x = np.asarray(x, dtype=np.float32)
    Bsz, n = x.shape
    v = np.zeros((Bsz, rows * hop), dtype=np.float32)
    m = min(rows * hop, n + 2 * pad)
    v[:, :m] = (x[:, reflect_index(n, pad)] * np.float32(scale))[:, :m]
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.reshape(Bsz, rows, hop), lo.reshape(Bsz, rows, hop)
    return np.concatenate([hi, hi, lo], axis=2)


def pack(fb):
    """(n_mels, nbins) filterbank -> (vals float32, start int32 (n_mels,), off int32 (n_mels + 1,)): filter m is vals[off[m] : off[m+1]]
    on bins start[m] .., its first to its last nonzero (as MelExtractor.__init__ packs it; `vals` is one zero when all are empty)."""
    start, off, vals = [], [0], []
    for m in range(fb.shape[0]):
        nz = np.nonzero(fb[m])[0]
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        start.append(lo)
        vals.append(fb[m, lo:hi])
        off.append(off[-1] + hi - lo)
    vals = np.concatenate(vals).astype(np.float32) if off[-1] else np.zeros(1, np.float32)
    return vals, np.asarray(start, np.int32), np.asarray(off, np.int32)


def mel_from_spec(spec, T, nbins, vals, start, off, eps, clip=CLIP):
    """ttsk_mel_from_spec in float64: spec (B, rows, ld) with Re in columns [0, nbins) and Im in [nbins, 2 nbins) ->
    (log-mel (B, n_mels, T), energy (B, T), entries per filter (n_mels,)).  Only rows < T are read."""
    s = np.asarray(spec, dtype=np.float64)[:, :T]
    p = s[:, :, :nbins] ** 2 + s[:, :, nbins:2 * nbins] ** 2
    mag = np.sqrt(p + float(eps))
    n_mels = len(start)
    lin = np.zeros((s.shape[0], n_mels, T))
    for m in range(n_mels):
        k = int(off[m + 1] - off[m])
        assert start[m] + k <= nbins
        lin[:, m] = mag[:, :, start[m]:start[m] + k] @ np.asarray(vals[off[m]:off[m + 1]], dtype=np.float64)
    return np.log(np.maximum(lin, clip)), np.sqrt(p.sum(axis=2)), np.diff(np.asarray(off, dtype=np.int64))
