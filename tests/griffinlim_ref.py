"""fp64 restatement of the Griffin-Lim route (tts_king_amd/audio.py: STFT, griffin_lim, mel-to-linear; csrc/griffinlim.hip), in plain
numpy and written from the definitions, not from the kernels:

  stft      reflect pad by n_fft/2, frame t at padded sample t*hop, periodic Hann of `win` centre-padded to n_fft, np.fft.rfft
  istft     np.fft.irfft per frame (the imaginary parts of DC and Nyquist are ignored), times the window, overlap-add, divided by
            wss[n] = sum_t w^2[n - t*hop] where that exceeds float32 tiny, n_fft/2 trimmed from both ends: hop*(T-1) samples
  step      Z = stft(x); A = Z - a/(1+a) Zprev; Y = m A/|A| ((m, 0) where |A| == 0); x' = istft(Y); Zprev' = Z
  loop      x0 = istft(m exp(i phase0)), then `step` n times
  C(x)      || |stft(x)| - m ||_F / ||m||_F, the spectral convergence

Spectra are (n_fft/2 + 1, T) arrays of one row; T = 1 + N // hop.  `stft32` / `istft32` are the same two transforms in float32 with
a radix-2 FFT whose twiddles are fp64 values rounded once: what an fp32 implementation can be held to, used by the tests to check
that their bars are not tighter than float32 itself.  Test infrastructure shared by tests/test_griffinlim_cpu.py and
tests/test_griffinlim_gpu.py."""
import numpy as np

TINY = float(np.finfo(np.float32).tiny)
U = 2.0 ** -24

# (n_fft, hop, win): the configurations the tests run
CONFIGS = [(64, 16, 64), (64, 8, 64), (64, 32, 64), (256, 64, 200), (1024, 256, 1024), (2048, 512, 2048)]
GAPPED = (64, 32, 16)         # wss == 0 between the frames' windows


def min_frames(n_fft, hop):
    """The fewest frames whose signal hop*(T-1) is longer than its reflect padding n_fft/2."""
    return n_fft // (2 * hop) + 2


def window(n_fft, win):
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    lpad = (n_fft - win) // 2
    return np.pad(w, (lpad, n_fft - win - lpad))


def reflect_index(n, pad):
    assert 0 <= pad < n
    j = np.abs(np.arange(-pad, n + pad))
    return np.where(j >= n, 2 * (n - 1) - j, j)


def frame_index(T, n_fft, hop):
    return hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]


def signal(n, seed):
    """Broadband noise plus a chirp, |y| <= 1: float32 (n,)."""
    r = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64)
    y = 0.45 * (r.rand(n) * 2 - 1) + 0.5 * np.sin(2 * np.pi * (0.01 + 0.2 * t / max(n, 1)) * t)
    return np.clip(y, -1.0, 1.0).astype(np.float32)


def stft(x, n_fft, hop, win):
    """x (N,) -> complex128 (n_fft/2 + 1, 1 + N // hop)."""
    x = np.asarray(x, dtype=np.float64)
    xp = x[reflect_index(len(x), n_fft // 2)]
    T = 1 + len(x) // hop
    return np.fft.rfft(xp[frame_index(T, n_fft, hop)] * window(n_fft, win), axis=1).T


def wss(T, n_fft, hop, win):
    """sum_t w^2[n - t*hop] over the n_fft + hop*(T-1) padded samples."""
    out = np.zeros(n_fft + hop * (T - 1))
    w2 = window(n_fft, win) ** 2
    for t in range(T):
        out[t * hop:t * hop + n_fft] += w2
    return out


def windowed_frames(Z, n_fft, win):
    """The fp64 windowed frames f_t = irfft(Z[:, t]) * w: (T, n_fft)."""
    return np.fft.irfft(np.asarray(Z, dtype=np.complex128).T, n=n_fft, axis=1) * window(n_fft, win)


def istft(Z, n_fft, hop, win):
    """Z (n_fft/2 + 1, T) -> x (hop*(T-1),)."""
    f = windowed_frames(Z, n_fft, win)
    T = f.shape[0]
    y = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        y[t * hop:t * hop + n_fft] += f[t]
    s = wss(T, n_fft, hop, win)
    ok = s > TINY
    y[ok] /= s[ok]
    return y[n_fft // 2:len(y) - n_fft // 2]


def polar(m, A):
    """m A/|A|, and (m, 0) where |A| == 0 (atan2(0, 0) = 0)."""
    r = np.abs(A)
    return m * np.where(r == 0, 1.0, A / np.where(r == 0, 1.0, r))


def step(x, m, n_fft, hop, win, momentum=0.0, zprev=None):
    """One iteration -> (x', Z = stft(x)); with momentum the phase comes from Z - a/(1+a) zprev and Z is the next zprev."""
    Z = stft(x, n_fft, hop, win)
    A = Z - momentum / (1.0 + momentum) * zprev if momentum > 0 else Z
    return istft(polar(m, A), n_fft, hop, win), Z


def griffin_lim(m, phase0, n_fft, hop, win, n_iters, momentum=0.0, keep=()):
    """-> x after n_iters iterations; with `keep`, {count: x} at those counts."""
    x = istft(m * np.exp(1j * np.asarray(phase0, dtype=np.float64)), n_fft, hop, win)
    zprev = np.zeros_like(m, dtype=np.complex128)
    kept = {0: x} if 0 in keep else {}
    for i in range(1, n_iters + 1):
        x, zprev = step(x, m, n_fft, hop, win, momentum, zprev)
        if i in keep:
            kept[i] = x
    return kept if keep else x


def convergence(x, m, n_fft, hop, win):
    return float(np.linalg.norm(np.abs(stft(x, n_fft, hop, win)) - m) / np.linalg.norm(m))


def mel_to_spec(mel, fb, scale=1000.0):
    """log-mel (n_mels, T), filterbank (n_mels, nbins) -> (nbins, T) = (exp(mel)^T @ fb)^T * scale, float64."""
    return (np.exp(np.asarray(mel, dtype=np.float64)).T @ np.asarray(fb, dtype=np.float64)).T * scale


# ------------------------------------------------------------------------------------------------ float32 restatement

def _fft32(z, inverse):
    """Radix-2 decimation-in-time FFT over the last axis in complex64; twiddles from fp64, rounded once.  No 1/n."""
    n = z.shape[-1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)]) if bits else np.zeros(1, int)
    s = z[..., rev].astype(np.complex64)
    sign = 1.0 if inverse else -1.0
    ln = 2
    while ln <= n:
        tw = np.exp(sign * 2j * np.pi * np.arange(ln // 2) / ln).astype(np.complex64)
        s = s.reshape(z.shape[:-1] + (n // ln, ln))
        t = (s[..., ln // 2:] * tw).astype(np.complex64)
        s = np.concatenate([s[..., :ln // 2] + t, s[..., :ln // 2] - t], axis=-1).astype(np.complex64)
        ln *= 2
    return s.reshape(z.shape)


def stft32(x, n_fft, hop, win):
    x = np.asarray(x, dtype=np.float32)
    xp = x[reflect_index(len(x), n_fft // 2)]
    T = 1 + len(x) // hop
    f = (xp[frame_index(T, n_fft, hop)] * window(n_fft, win).astype(np.float32)).astype(np.float32)
    return _fft32(f.astype(np.complex64), False)[:, :n_fft // 2 + 1].T


def istft32(Z, n_fft, hop, win):
    Z = np.asarray(Z).astype(np.complex64).T
    Z = Z.copy()
    Z[:, 0] = Z[:, 0].real
    Z[:, -1] = Z[:, -1].real
    full = np.concatenate([Z, np.conj(Z[:, -2:0:-1])], axis=1)
    w = window(n_fft, win).astype(np.float32)
    f = ((_fft32(full, True).real.astype(np.float32) / np.float32(n_fft)) * w).astype(np.float32)
    T = f.shape[0]
    y = np.zeros(n_fft + hop * (T - 1), np.float32)
    s = np.zeros_like(y)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += f[t]
        s[t * hop:t * hop + n_fft] += w * w
    ok = s > np.float32(TINY)
    y[ok] /= s[ok]
    return y[n_fft // 2:len(y) - n_fft // 2]


def griffin_lim32(m, phase0, n_fft, hop, win, n_iters, keep=()):
    m32 = np.asarray(m, dtype=np.float32)
    x = istft32(m32 * np.exp(1j * np.asarray(phase0, dtype=np.float32)).astype(np.complex64), n_fft, hop, win)
    kept = {0: x} if 0 in keep else {}
    for i in range(1, n_iters + 1):
        Z = stft32(x, n_fft, hop, win)
        r = np.abs(Z)
        x = istft32(m32 * np.where(r == 0, 1, Z / np.where(r == 0, 1, r)), n_fft, hop, win)
        if i in keep:
            kept[i] = x
    return kept if keep else x


# ------------------------------------------------------------------------------------------------ the bars of the GPU tests

def transform_bar(n_fft):
    return (8 * np.log2(n_fft) + 8) * U


def inverse_bar(Z, n_fft, hop, win, first=8):
    """Per kept sample: u / wss[n] * ((first*log2(n_fft) + 8) * sum_t ||f_t||_2 + (n_fft/hop + 3) * sum_t |w * f_t[n]|), sums over the frames
    covering n; where wss == 0 the bar is 0.  The second term is read literally: f_t is the windowed frame irfft(Z_t) * w, and it is
    multiplied by the window once more, w[n - t*hop] * f_t[n].  Since w <= 1 that is the smaller of the two possible readings (the
    other being |f_t[n]| alone), so the bar is the tighter one; the first term is larger by orders of magnitude either way."""
    f = windowed_frames(Z, n_fft, win)
    T = f.shape[0]
    norms = np.linalg.norm(f, axis=1)
    w = window(n_fft, win)
    a = np.zeros(n_fft + hop * (T - 1))
    b = np.zeros_like(a)
    for t in range(T):
        a[t * hop:t * hop + n_fft] += norms[t]
        b[t * hop:t * hop + n_fft] += np.abs(w * f[t])
    s = wss(T, n_fft, hop, win)
    div = np.where(s > TINY, s, 1.0)
    bar = U / div * ((first * np.log2(n_fft) + 8) * a + (n_fft // hop + 3) * b)
    bar = np.where(s == 0, 0.0, bar)
    return bar[n_fft // 2:len(bar) - n_fft // 2]
