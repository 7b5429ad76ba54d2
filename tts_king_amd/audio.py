"""Mel-spectrogram extraction on the GPU, behind the reference's two call surfaces:

  * `mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)`
    — hifi/meldataset.py:49-74 (what the vocoder is trained on and what `hifiapi` consumers feed it);
  * `TacotronSTFT(...).mel_spectrogram(y) -> (mel, energy)` — fs_two/audio/stft.py:145-193 (FS2 preprocessing features).

Pipeline (all on the current stream, no host math after construction): `ttsk_stft_frames` (reflect pad, hop-block rows,
fp16 hi/lo split) -> one `ttsk_gemm` conv launch with the windowed Fourier basis (hi*hi + hi*lo + lo*hi as one contraction,
fp32 accumulate: the reference's own conv-STFT, stft.py:77-84) -> `ttsk_mel_from_spec` (magnitude, Slaney mel filterbank,
log-clamp, energy).  The filterbank is librosa 0.7.2's `filters.mel(htk=False, norm=1)` (reference requirements.txt:3),
built here from its published definition because librosa is not a dependency of this package.

Accepted envelope (pinned by tests/test_mel_envelope_gpu.py against an fp64 restatement): n_fft % hop == 0, hop % 8 == 0,
1 <= win <= n_fft <= 2048 (a shorter window is centre-padded), 1 <= num_mels <= 80, any sampling rate, fmin and fmax (None = Nyquist);
anything else is a ValueError at construction.  Every accepted configuration runs: n_fft / hop is the conv's tap count and is not
limited (ttsk_gemm plans more than 32 taps onto its register-staged kernels; tested to 128 taps at hop = 8), n_fft <= 1150
launches mel_from_spec_kernel<9> and larger ones <17>.  A signal must be longer than its reflect padding ((n_fft - hop)//2 on the
vocoder surface, n_fft//2 on Tacotron's) and give one frame, else ValueError.  Amplitude: the signal is scaled by 4096 and rounded to fp16,
so |y| must stay below MAX_AMPLITUDE = 65520/4096 (just under 16).  `mel_spectrogram` checks that (one reduction and one host read per
call) and raises ValueError; `TacotronSTFT` keeps the reference's own |y| <= 1 assertion.  Log-mel is within 1e-4 of fp64 on broadband
input at every such configuration, energy within 1e-4 relative.

The way back, mel -> waveform without a vocoder checkpoint, is a second, phase-carrying transform pair in fp32
on the FFT kernels of csrc/griffinlim.hip: `STFT` (fs_two/audio/stft.py:17-142), `griffin_lim` (audio_processing.py:66-82),
`mel_to_spec` / `inv_mel_spec` (tools.py:18-34), and `GriffinLimVocoder`, what `TTSKing` runs for `vocoder="griffin_lim"`.  It shares
the window and the filterbank's packing (`PackedMelFilterbank`) with the extractor above and none of its launches or limits: the
vocoder takes n_mel_channels up to 1024 and any hop that divides a power-of-two filter_length in 64..2048."""
import numpy as np
import torch

from . import ops

_SIG_SCALE = 4096.0      # powers of two: keep the fp16 low parts of signal and basis in the normal range
_BASIS_SCALE = 1024.0
MAX_AMPLITUDE = 65520.0 / _SIG_SCALE     # 15.996...: from here on the scaled sample rounds to fp16 inf


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) * 27.0 / np.log(6.4), lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), m * 200.0 / 3.0)


def slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """(n_mels, 1 + n_fft//2) float32: triangular filters on the Slaney mel scale, each with unit area in Hz."""
    fmax = sr / 2.0 if fmax is None else fmax
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    up = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - freqs[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return w.astype(np.float32)


class PackedMelFilterbank:
    """The Slaney filterbank (num_mels, n_fft//2 + 1) on the device, each filter as its run of non-zero weights: `vals` (nnz,) fp32,
    `start` (num_mels,) int32 the first bin of each run, `off` (num_mels + 1,) int32 the runs' offsets into `vals`.  What
    `ttsk_mel_from_spec` (through `MelExtractor`) and `ttsk_mel_to_spec` read; it has no limits of its own, each user states its."""

    def __init__(self, sampling_rate, n_fft, num_mels, fmin, fmax, device):
        self.num_mels, self.nbins = int(num_mels), n_fft // 2 + 1
        fb = slaney_mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)
        start, off, vals = [], [0], []
        for m in range(num_mels):
            nz = np.nonzero(fb[m])[0]
            lo, hi = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
            start.append(lo)
            vals.append(fb[m, lo:hi])
            off.append(off[-1] + hi - lo)
        self.nnz = off[-1]
        self.vals = torch.from_numpy(np.concatenate(vals) if self.nnz else np.zeros(1, np.float32)).to(device)
        self.start = torch.tensor(start, dtype=torch.int32, device=device)
        self.off = torch.tensor(off, dtype=torch.int32, device=device)


class MelExtractor:
    """Device-resident bases + the launch sequence.  `pad` samples are reflected on each side; `eps` is added under
    the magnitude's square root (1e-9 in hifi/meldataset.py:69, 0 in fs_two/audio/stft.py:86)."""

    def __init__(self, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, pad, eps, device="cuda:0"):
        if hop_size < 8 or n_fft % hop_size or hop_size % 8 or not 1 <= win_size <= n_fft or not 1 <= num_mels <= 80 or n_fft > 2048:
            raise ValueError("MelExtractor needs n_fft %% hop_size == 0, hop_size %% 8 == 0, win_size <= n_fft <= 2048, num_mels <= 80 "
                             "(any number n_fft / hop_size of taps), got n_fft=%r hop_size=%r win_size=%r num_mels=%r"
                             % (n_fft, hop_size, win_size, num_mels))
        self.n_fft, self.hop, self.num_mels, self.pad, self.eps = n_fft, hop_size, num_mels, int(pad), float(eps)
        self.taps = n_fft // hop_size
        self.nbins = n_fft // 2 + 1
        self.device = torch.device(device)
        # windowed Fourier basis, rows [Re bins | Im bins | zero rows up to a multiple of 8]  (stft.py:25-50)
        n = np.arange(n_fft, dtype=np.float64)
        ang = 2.0 * np.pi * np.outer(np.arange(self.nbins, dtype=np.float64), n) / n_fft
        win = torch.hann_window(win_size, periodic=True, dtype=torch.float64).numpy()
        lpad = (n_fft - win_size) // 2
        win = np.pad(win, (lpad, n_fft - win_size - lpad))
        self.cout = (2 * self.nbins + 7) // 8 * 8
        basis = np.zeros((self.cout, n_fft), dtype=np.float64)
        basis[: self.nbins] = np.cos(ang) * win
        basis[self.nbins: 2 * self.nbins] = -np.sin(ang) * win
        b = torch.from_numpy(basis * _BASIS_SCALE).float().view(self.cout, self.taps, hop_size)
        b_hi = b.half()
        b_lo = (b - b_hi.float()).half()
        # per tap [hi | lo | hi] against the signal rows' [hi | hi | lo]: one contraction = hi*hi + hi*lo + lo*hi
        self.basis = torch.cat([b_hi, b_lo, b_hi], dim=2).contiguous().to(self.device)      # (cout, taps, 3*hop)
        self.fb = PackedMelFilterbank(sampling_rate, n_fft, num_mels, fmin, fmax, self.device)
        self.nnz, self.fb_vals, self.fb_start, self.fb_off = self.fb.nnz, self.fb.vals, self.fb.start, self.fb.off

    def frames(self, n_samples):
        return 1 + (n_samples + 2 * self.pad - self.n_fft) // self.hop

    def __call__(self, y):
        """y (B, L) fp32 on the device, |y| < MAX_AMPLITUDE (not checked here) -> (log-mel (B, num_mels, T), energy (B, T))."""
        if y.dim() != 2 or y.dtype != torch.float32:
            raise ValueError("MelExtractor: y must be (B, L) fp32")
        Bsz, n = y.shape
        T = self.frames(n)
        if T < 1:
            raise ValueError("MelExtractor: signal shorter than one frame")
        if n <= self.pad:
            raise ValueError("MelExtractor: reflect padding by %d samples needs a signal longer than that, got %d" % (self.pad, n))
        rows = T + self.taps - 1
        sig = ops.stft_frames(y.contiguous(), self.pad, rows, self.hop, _SIG_SCALE)
        spec = torch.empty(Bsz * rows, self.cout, dtype=torch.float32, device=y.device)
        K = 3 * self.hop
        ops.gemm(sig, self.basis, spec, Bsz * rows, self.cout, K, K, self.taps * K, self.cout,
                 alpha=1.0 / (_SIG_SCALE * _BASIS_SCALE), taps=self.taps, seg_len=rows, tap_shift0=0, tap_dshift=1, b_tap_stride=K)
        return ops.mel_from_spec(spec, Bsz, rows, T, self.nbins, self.fb_vals, self.fb_start, self.fb_off, self.nnz,
                                 self.num_mels, self.eps)


_extractors = {}


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """Drop-in for hifi/meldataset.py:49-74: y (B, L) fp32 CUDA tensor -> log-mel (B, num_mels, L // hop_size)."""
    if center:
        raise ValueError("mel_spectrogram: the reference only ever calls this with center=False")
    key = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, str(y.device))
    if key not in _extractors:
        _extractors[key] = MelExtractor(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax,
                                        pad=(n_fft - hop_size) // 2, eps=1e-9, device=y.device)
    # the reference takes any amplitude; here the scaled signal must fit fp16.  One reduction and one host read per call.
    peak = float(y.abs().max()) if y.numel() else 0.0
    if not peak < MAX_AMPLITUDE:
        raise ValueError("mel_spectrogram: |y| must stay below 16 (%g: the signal is scaled by %g and rounded to fp16), got %g"
                         % (MAX_AMPLITUDE, _SIG_SCALE, peak))
    return _extractors[key](y)[0]


def _frame_counts(what, lens, Bsz, T):
    """`lens` (a sequence or tensor of B frame counts, or None) as a list of ints in 1..T."""
    if lens is None:
        return None
    lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(lens) != Bsz or any(not 1 <= v <= T for v in lens):
        raise ValueError("%s: lens must hold %d frame counts in 1..%d, got %r" % (what, Bsz, T, lens))
    return lens


class STFT:
    """Drop-in for fs_two/audio/stft.py:17-142 (`STFT(filter_length, hop_length, win_length, window)`, `transform`, `inverse`,
    `forward`) on the fp32 FFT kernels of csrc/griffinlim.hip, not the conv-GEMM of `MelExtractor`.
    Accepted: filter_length a power of two in 64..2048, hop_length a divisor of it, 1 <= win_length <= filter_length, window
    "hann" (periodic, centre-padded, as `MelExtractor` builds it); anything else is a ValueError that names the argument.  The
    tensors live on the device of the input; the window and the twiddle table (fp64, rounded once) are uploaded once per device."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not is_int(filter_length) or not 64 <= filter_length <= 2048 or filter_length & (filter_length - 1):
            raise ValueError("STFT: filter_length must be a power of two in 64..2048, got %r" % (filter_length,))
        if not is_int(hop_length) or hop_length < 1 or filter_length % hop_length:
            raise ValueError("STFT: hop_length must be a positive divisor of filter_length = %d, got %r" % (filter_length, hop_length))
        if not is_int(win_length) or not 1 <= win_length <= filter_length:
            raise ValueError("STFT: win_length must be in 1..filter_length = %d, got %r" % (filter_length, win_length))
        if window != "hann":
            raise ValueError("STFT: window must be 'hann' (periodic Hann, centre-padded to filter_length), got %r" % (window,))
        self.filter_length, self.hop_length, self.win_length, self.window = int(filter_length), int(hop_length), int(win_length), window
        self.nbins = self.filter_length // 2 + 1
        self.pad = self.filter_length // 2
        win = torch.hann_window(self.win_length, periodic=True, dtype=torch.float64).numpy()
        lpad = (self.filter_length - self.win_length) // 2
        self._win = np.pad(win, (lpad, self.filter_length - self.win_length - lpad)).astype(np.float32)
        ang = 2.0 * np.pi * np.arange(self.filter_length // 2, dtype=np.float64) / self.filter_length
        self._tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)
        self._on_device = {}

    def tables(self, device):
        """(window (n_fft,), twiddle (n_fft/2, 2)) fp32 on `device`."""
        key = str(device)
        if key not in self._on_device:
            self._on_device[key] = (torch.from_numpy(self._win).to(device), torch.from_numpy(self._tw).to(device))
        return self._on_device[key]

    def min_frames(self):
        """The fewest frames whose hop_length * (T - 1) samples are longer than the reflect padding."""
        return self.pad // self.hop_length + 2

    def check_frames(self, what, T, lens=None):
        for v in [T] + list(lens or []):
            if self.hop_length * (v - 1) <= self.pad:
                raise ValueError("%s: %d frames are hop_length * (T - 1) = %d samples, not longer than the reflect padding filter_length / 2 = %d "
                                 "(at least %d frames)" % (what, v, self.hop_length * (v - 1), self.pad, self.min_frames()))

    def transform(self, input_data, lens=None):
        """y (B, N) fp32 on the device -> (magnitude, phase), each (B, filter_length/2 + 1, 1 + N // hop_length).  `lens`: samples per
        row; a row then reflects about its own end and its frames past 1 + lens[b] // hop_length are zeros."""
        if input_data.dim() != 2 or input_data.dtype != torch.float32:
            raise ValueError("STFT.transform: input_data must be (B, N) fp32")
        Bsz, n = input_data.shape
        if lens is not None:
            lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
            if len(lens) != Bsz or any(not 0 <= v <= n for v in lens):
                raise ValueError("STFT.transform: lens must hold %d sample counts in 0..%d, got %r" % (Bsz, n, lens))
        for v in [n] + list(lens or []):
            if v <= self.pad:
                raise ValueError("STFT.transform: reflect padding by filter_length / 2 = %d samples needs a signal longer than that, got %d"
                                 % (self.pad, v))
        win, tw = self.tables(input_data.device)
        dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=input_data.device)
        return ops.stft_polar(input_data.contiguous(), dl, self.filter_length, self.hop_length, win, tw)

    def inverse(self, magnitude, phase, lens=None):
        """(magnitude, phase) (B, filter_length/2 + 1, T) -> (B, 1, hop_length * (T - 1)): inverse real FFT per frame (imaginary parts of
        DC and Nyquist ignored), window, overlap-add, division by the window's sum of squares where it exceeds float32 tiny, filter_length / 2
        trimmed from both ends.  `lens`: frames per row; zeros past hop_length * (lens[b] - 1)."""
        if magnitude.dim() != 3 or magnitude.shape[1] != self.nbins or magnitude.shape != phase.shape or magnitude.shape[2] < 2:
            raise ValueError("STFT.inverse: magnitude and phase must both be (B, %d, T >= 2), got %s and %s"
                             % (self.nbins, tuple(magnitude.shape), tuple(phase.shape)))
        Bsz, _, T = magnitude.shape
        lens = _frame_counts("STFT.inverse", lens, Bsz, T)
        win, tw = self.tables(magnitude.device)
        dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=magnitude.device)
        wav = ops.istft(magnitude.float().contiguous(), phase.float().contiguous(), dl, self.filter_length, self.hop_length, win, tw)
        return wav.unsqueeze(1)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    __call__ = forward


def griffin_lim(magnitudes, stft_fn, n_iters=30, *, momentum=0.0, phase0=None, seed=None, lens=None):
    """Drop-in for fs_two/audio/audio_processing.py:66-82 on the device: magnitudes (B, filter_length/2 + 1, T) fp32 -> signal
    (B, hop_length * (T - 1)) after `n_iters` iterations x <- inverse(magnitudes, phase(transform(x))), one launch each.
    momentum a in [0, 1): the phase comes from Z - a / (1 + a) Zprev (fast Griffin-Lim, Perraudin et al. 2013); 0 is the reference's
    iteration.  phase0: the initial phases, a device tensor shaped like `magnitudes`; absent, uniform in [0, 2 pi) from `torch.rand`
    with a generator seeded by `seed` (None: torch's default generator).  lens: frames per row; a row's frames past its count do not
    exist for it, and its signal is zero from hop_length * (lens[b] - 1) on."""
    import math
    if magnitudes.dim() != 3 or magnitudes.shape[1] != stft_fn.nbins or magnitudes.dtype != torch.float32:
        raise ValueError("griffin_lim: magnitudes must be (B, %d, T) fp32, got %s %s" % (stft_fn.nbins, tuple(magnitudes.shape), magnitudes.dtype))
    if not 0.0 <= float(momentum) < 1.0:
        raise ValueError("griffin_lim: momentum must be in [0, 1), got %r" % (momentum,))
    if int(n_iters) < 0:
        raise ValueError("griffin_lim: n_iters must be at least 0, got %r" % (n_iters,))
    Bsz, nbins, T = magnitudes.shape
    lens = _frame_counts("griffin_lim", lens, Bsz, T)
    stft_fn.check_frames("griffin_lim", T, lens)
    dev = magnitudes.device
    if phase0 is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        phase0 = torch.rand(magnitudes.shape, generator=gen, device=dev, dtype=torch.float32) * (2.0 * math.pi)
    elif phase0.shape != magnitudes.shape or phase0.dtype != torch.float32 or phase0.device != dev:
        raise ValueError("griffin_lim: phase0 must be an fp32 tensor shaped like magnitudes, on their device")
    n_fft, hop = stft_fn.filter_length, stft_fn.hop_length
    win, tw = stft_fn.tables(dev)
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    # frame-major copies: a workgroup reads one frame's bins, which are then contiguous
    m = magnitudes.transpose(1, 2).contiguous().transpose(1, 2)
    p = phase0.transpose(1, 2).contiguous().transpose(1, 2)
    cur = ops.istft_frames(m, p, dl, n_fft, hop, win, tw)
    nxt = torch.empty_like(cur)
    zprev = torch.zeros(Bsz, T, nbins, 2, dtype=torch.float32, device=dev) if momentum > 0 else None
    for _ in range(int(n_iters)):
        ops.griffinlim_step(cur, m, dl, n_fft, hop, win, tw, nxt, zprev, float(momentum))
        cur, nxt = nxt, cur
    return ops.istft_ola(cur, dl, hop, win)


SPEC_FROM_MEL_SCALING = 1000.0      # fs_two/audio/tools.py:22


MAX_MELS_TO_SPEC = 1024            # ttsk_mel_to_spec's limit (FastSpeech2 here goes up to n_mel_channels = 1024)


def mel_to_spec(mel, _stft):
    """log-mel (B, n_mel_channels, T) fp32 on the device -> linear magnitudes (B, filter_length/2 + 1, T): the reference's
    exp(mel)^T @ mel_basis * 1000 (tools.py:20-25: the transposed filterbank, not a pseudo-inverse), one launch on the packed filterbank
    `_stft.fb` (a `PackedMelFilterbank`: `TacotronSTFT` and `GriffinLimVocoder` both hold one), n_mel_channels <= 1024."""
    fb = _stft.fb
    if mel.dim() != 3 or mel.shape[1] != fb.num_mels or mel.dtype != torch.float32:
        raise ValueError("mel_to_spec: mel must be (B, %d, T) fp32, got %s %s" % (fb.num_mels, tuple(mel.shape), mel.dtype))
    return ops.mel_to_spec(mel.contiguous(), fb.vals, fb.start, fb.off, fb.nbins, SPEC_FROM_MEL_SCALING)


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60):
    """Drop-in for fs_two/audio/tools.py:18-34: log-mel (n_mel_channels, T) -> Griffin-Lim audio written to `out_filename` as a float32
    wav at `_stft.sampling_rate` (and returned, (hop_length * (T - 1),) on the host).  Two slips of the reference are not reproduced:
    it drops the last frame (`spec_from_mel[:, :, :-1]`), here all T frames are used; and it reads `_stft._stft_fn`, an attribute that
    does not exist, here `_stft.stft_fn`."""
    from scipy.io import wavfile
    mel = mel.to(_stft.device).float()
    audio = griffin_lim(mel_to_spec(mel.unsqueeze(0), _stft), _stft.stft_fn, griffin_iters)[0]
    audio = ops.to_host(audio).numpy()
    wavfile.write(out_filename, int(_stft.sampling_rate), audio)
    return audio


class TacotronSTFT:
    """Drop-in for fs_two/audio/stft.py:145-193: constructor arguments, `mel_spectrogram(y) -> (mel, energy)` on the conv-GEMM route
    of `MelExtractor`, and for the way back `stft_fn` (an `STFT`, built on first use: its envelope is narrower than `MelExtractor`'s),
    `mel_basis` (dense fp32 on the device), `spectral_normalize` and `spectral_de_normalize`."""

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax, device="cuda:0"):
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.device = torch.device(device)
        self._stft_args = (filter_length, hop_length, win_length)
        self._mel_args = (sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self._ex = MelExtractor(filter_length, n_mel_channels, sampling_rate, hop_length, win_length, mel_fmin, mel_fmax,
                                pad=filter_length // 2, eps=0.0, device=device)
        self.fb = self._ex.fb

    @property
    def stft_fn(self):
        if not hasattr(self, "_stft_fn"):
            self._stft_fn = STFT(*self._stft_args)
        return self._stft_fn

    @property
    def mel_basis(self):
        if not hasattr(self, "_mel_basis"):
            self._mel_basis = torch.from_numpy(slaney_mel_filterbank(*self._mel_args)).to(self.device)
        return self._mel_basis

    def spectral_normalize(self, magnitudes):
        return torch.log(torch.clamp(magnitudes, min=1e-5))       # audio_processing.py:85-91

    def spectral_de_normalize(self, magnitudes):
        return torch.exp(magnitudes)                              # audio_processing.py:94-100

    def mel_spectrogram(self, y):
        if float(y.min()) < -1.0 or float(y.max()) > 1.0:      # stft.py:185-186
            raise AssertionError("TacotronSTFT.mel_spectrogram: input outside [-1, 1]")
        return self._ex(y)


VOCODERS = ("hifigan", "griffin_lim")


def vocoder_name(name, default="hifigan"):
    """`name` (None: `default`) as one of VOCODERS, or ValueError."""
    name = default if name is None else name
    if name not in VOCODERS:
        raise ValueError("vocoder must be one of %s (or None for the configured one), got %r" % (", ".join(repr(v) for v in VOCODERS), name))
    return name


class GriffinLimVocoder:
    """mel -> waveform without a checkpoint (`mi355x.vocoder: griffin_lim`, or `vocoder="griffin_lim"` on `TTSKing.mel_to_wav` /
    `speak`), with `HIFIapi`'s four call forms.  STFT and mel parameters come from preprocess_config.preprocessing (`stft`, `mel`,
    `audio.sampling_rate`).  Accepted: `STFT`'s envelope (filter_length a power of two in 64..2048, hop_length a divisor of it,
    1 <= win_length <= filter_length), 1 <= n_mel_channels <= 1024 (`ttsk_mel_to_spec`'s limit), any sampling rate, mel_fmin and
    mel_fmax; anything else is a ValueError at construction that names the config key.  It holds an `STFT` and a
    `PackedMelFilterbank` and no `MelExtractor`: that one's narrower envelope (n_mel_channels <= 80, hop_length a multiple of 8)
    and its conv basis belong to the analysis route, which nothing here launches.
    log-mel -> `mel_to_spec` -> `griffin_lim` from phases drawn per utterance from `seed` (so a batch row
    equals its solo run) -> every utterance scaled to a peak of PEAK (Griffin-Lim on the transposed filterbank is not calibrated)
    -> float, or int16 = trunc(y * 32767).  `sample_rate` goes through the polyphase resampler (tts_king_amd/resample.py)."""
    PEAK = 0.95
    INT16_SCALE = 32767.0

    def __init__(self, config, device="cuda:0", seed=None):
        pp = config.preprocess_config["preprocessing"]
        mi = (config.get("mi355x", None) if hasattr(config, "get") else None) or {}
        self.cfg = config
        self.device = torch.device("cuda:0" if device in ("gpu", None) else device)
        self.sampling_rate = int(pp["audio"]["sampling_rate"])
        where = "GriffinLimVocoder (mi355x.vocoder: griffin_lim): preprocess_config.preprocessing."
        n_mels = pp["mel"]["n_mel_channels"]
        if not isinstance(n_mels, (int, np.integer)) or isinstance(n_mels, bool) or not 1 <= n_mels <= MAX_MELS_TO_SPEC:
            raise ValueError("%smel.n_mel_channels must be an integer in 1..%d, got %r" % (where, MAX_MELS_TO_SPEC, n_mels))
        try:
            self.stft_fn = STFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"])
        except ValueError as e:
            raise ValueError("%sstft is outside the accepted values: %s" % (where, e)) from None
        self.n_mel_channels = int(n_mels)
        self.fb = PackedMelFilterbank(self.sampling_rate, self.stft_fn.filter_length, self.n_mel_channels, pp["mel"]["mel_fmin"],
                                      pp["mel"]["mel_fmax"], self.device)
        self.hop = self.stft_fn.hop_length
        self.seed = int(mi.get("seed", 1234) if seed is None else seed)
        self.momentum = float(mi.get("griffin_momentum", 0.0))
        self.output_sample_rate = mi.get("output_sample_rate", None)

    def _rate(self, sample_rate):
        from . import resample
        rate = self.output_sample_rate if sample_rate is None else sample_rate
        return None if rate is None or resample.check_rate(rate) == self.sampling_rate else int(rate)

    def _signals(self, mels, griffin_iters):
        """mels: a list of (n_mels, T_i) fp32 device tensors -> (y (B, hop * (T_max - 1)) with every row at peak PEAK, samples per row)."""
        for m in mels:
            if m.dim() != 2 or m.shape[0] != self.n_mel_channels:
                raise ValueError("GriffinLimVocoder: every mel must have n_mel_channels = %d channels, got %s" % (self.n_mel_channels, tuple(m.shape)))
        frames = [int(m.shape[1]) for m in mels]
        Bsz, T = len(mels), max(frames)
        self.stft_fn.check_frames("GriffinLimVocoder", T, frames)
        mel = torch.zeros(Bsz, self.n_mel_channels, T, dtype=torch.float32, device=self.device)
        phase0 = torch.zeros(Bsz, self.stft_fn.nbins, T, dtype=torch.float32, device=self.device)
        gen = torch.Generator(device=self.device)
        for b, m in enumerate(mels):
            mel[b, :, :frames[b]] = m
            gen.manual_seed(self.seed)
            phase0[b, :, :frames[b]] = torch.rand(self.stft_fn.nbins, frames[b], generator=gen, device=self.device) * (2.0 * np.pi)
        y = griffin_lim(mel_to_spec(mel, self), self.stft_fn, griffin_iters, momentum=self.momentum, phase0=phase0,
                        lens=frames)
        peak = y.abs().amax(dim=1, keepdim=True)
        y = y * torch.where(peak > 0, self.PEAK / peak, torch.zeros_like(peak))
        return y, [self.hop * (t - 1) for t in frames]

    def _finish(self, y, ns, sample_rate, int16):
        """The rows of y cut to their ns samples, resampled and converted as asked: a list of (1, 1, n) device tensors."""
        from . import resample
        rate = self._rate(sample_rate)
        if rate is None:
            out = ops.to_int16(y, self.INT16_SCALE) if int16 else y
            return [out[b, :n].reshape(1, 1, n) for b, n in enumerate(ns)]
        filt = resample.filter_for(self.sampling_rate, rate, y.device)
        segs = resample.segments([b * y.shape[1] for b in range(len(ns))], ns, filt.L, filt.M)
        out = torch.empty(segs.n_dst, dtype=torch.int16 if int16 else torch.float32, device=y.device)
        ops.resample(y.contiguous().view(-1), torch.from_numpy(segs.table).to(y.device), filt, out=out,
                     int16_scale=self.INT16_SCALE if int16 else None)
        return [out[o:o + n].reshape(1, 1, n) for o, n in segs.spans]

    def _list(self, mels, frames_first):
        out = []
        for m in mels:
            m = torch.as_tensor(m).to(self.device).float()
            m = m[0] if m.dim() == 3 else m
            out.append(m.transpose(0, 1) if frames_first else m)
        return out

    def __call__(self, x, sample_rate=None, griffin_iters=60):
        """mel (B, n_mels, T) -> float waveforms (B, 1, hop * (T - 1)) on the device (at `sample_rate`: ceil of that times L / M)."""
        with torch.no_grad():
            rows = self._finish(*self._signals(self._list(list(x), False), griffin_iters), sample_rate, False)
            return torch.cat(rows, dim=0)

    def generate(self, mel_specs, sample_rate=None, griffin_iters=60):
        """mel (B, n_mels, T) -> int16 ndarray (B, 1, hop * (T - 1)) on the host."""
        with torch.no_grad():
            rows = self._finish(*self._signals(self._list(list(mel_specs), False), griffin_iters), sample_rate, True)
            return ops.to_host(torch.cat(rows, dim=0)).numpy()

    def call_ragged(self, mels, frames_first=False, sample_rate=None, griffin_iters=60):
        """A list of mels of any lengths -> a list of float waveforms (1, 1, hop * (T_i - 1)) on the device: one batch with `lens`,
        each waveform bit for bit what its mel gives alone."""
        with torch.no_grad():
            return self._finish(*self._signals(self._list(mels, frames_first), griffin_iters), sample_rate, False)

    def generate_ragged(self, mels, frames_first=False, sample_rate=None, griffin_iters=60):
        """`call_ragged` as int16 ndarrays on the host."""
        with torch.no_grad():
            rows = self._finish(*self._signals(self._list(mels, frames_first), griffin_iters), sample_rate, True)
            return [ops.to_host(r).numpy() for r in rows]

    def output_rate(self, sample_rate=None):
        """The rate (Hz) of what a call with `sample_rate` returns."""
        rate = self._rate(sample_rate)
        return self.sampling_rate if rate is None else rate

    def _joined(self, mels, join, frames_first, sample_rate, griffin_iters, int16):
        """The padded batch of `_signals` (resampled row by row when asked) joined by `join` (`narrate.Join`): (out, info) on the device."""
        from . import narrate, resample
        mels = self._list(mels, frames_first)
        if len(join) != len(mels):
            raise ValueError("GriffinLimVocoder: the join names %d utterances, the call has %d" % (len(join), len(mels)))
        y, ns = self._signals(mels, griffin_iters)
        offs, src = [b * y.shape[1] for b in range(len(ns))], y.contiguous().view(-1)
        rate = self._rate(sample_rate)
        if rate is not None:
            filt = resample.filter_for(self.sampling_rate, rate, y.device)
            segs = resample.segments(offs, ns, filt.L, filt.M)
            src = ops.resample(src, torch.from_numpy(segs.table).to(y.device), filt,
                               out=torch.empty(max(segs.n_dst, 1), dtype=torch.float32, device=y.device))
            offs, ns = [o for o, _ in segs.spans], [n for _, n in segs.spans]
        table = join.table(offs, ns)
        return ops.wav_join(src, torch.from_numpy(table).to(y.device), n_dst=max(narrate.out_bound(table), 1),
                            int16_scale=self.INT16_SCALE if int16 else None)

    def call_joined(self, mels, join, frames_first=False, sample_rate=None, griffin_iters=60):
        """The waveforms of `call_ragged` as ONE float waveform (1, 1, total) on the device, joined there by `join` (a `narrate.Join`:
        per utterance trim, level, fade, pause) -> (waveform, `narrate.Info`)."""
        from . import narrate
        with torch.no_grad():
            out, info = self._joined(mels, join, frames_first, sample_rate, griffin_iters, False)
            info = narrate.Info(ops.to_host(info).numpy(), len(join))
            return out[:info.total].reshape(1, 1, info.total), info

    def generate_joined(self, mels, join, frames_first=False, sample_rate=None, griffin_iters=60):
        """`call_joined` as an int16 ndarray (1, 1, total) on the host, saturating at +-32767 / 32768 of INT16_SCALE."""
        from . import narrate
        with torch.no_grad():
            out, info = self._joined(mels, join, frames_first, sample_rate, griffin_iters, True)
            host = ops.to_host(out).numpy()
            info = narrate.Info(ops.to_host(info).numpy(), len(join))
            return host[:info.total].reshape(1, 1, info.total), info


class PitchExtractor:
    """F0 per frame on the device by YIN (`ops.pitch_yin`): frame t is centred on sample t * hop_length, the
    frame grid of `TacotronSTFT` and of DIO at that frame period.  The method is not DIO: values differ from pyworld's."""

    def __init__(self, sampling_rate, hop_length, window=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.15):
        self.sampling_rate, self.hop_length, self.window = int(sampling_rate), int(hop_length), int(window)
        self.f0_floor, self.f0_ceil, self.threshold = float(f0_floor), float(f0_ceil), float(threshold)
        self.tau_min, self.tau_max = ops.yin_lags(self.sampling_rate, self.f0_floor, self.f0_ceil)

    def frames(self, n_samples):
        return 1 + int(n_samples) // self.hop_length

    def __call__(self, y, lens=None):
        """y (B, L) fp32 on the device, lens (B,) int32 on the device or None -> f0 (B, 1 + L // hop_length), 0 = unvoiced."""
        if y.dim() != 2 or y.dtype != torch.float32:
            raise ValueError("PitchExtractor: y must be (B, L) fp32")
        return ops.pitch_yin(y.contiguous(), lens, sr=self.sampling_rate, hop=self.hop_length, window=self.window,
                             f0_floor=self.f0_floor, f0_ceil=self.f0_ceil, threshold=self.threshold)
