"""Restatements of the two data-preparation kernels (include/ttsk.h) in numpy, fp64 by default.

`yin` follows ttsk_pitch_yin's rules one by one, vectorised over lags, and also returns a per-frame *margin*: how far the
frame's decisions were from going the other way (the smallest |d'(tau) - thr| over the lags scanned and |d'(tau+1) - d'(tau)| over
the comparisons of the walk, the one that ended it included).  A frame with a margin under 1e-4 may legitimately be decided
differently in fp32, so the GPU tests leave such frames out.  `phoneme_prosody` follows fs_two/preprocessor/preprocessor.py:215-266
with scipy's interp1d called as the reference calls it, except that a phoneme of no frames stores 0 and stays out of the
utterance statistics (the reference takes log 0 there and ends with NaN).  Both take `dtype` so that they can run in fp32:
the distance of that run from the fp64 one is the yardstick the GPU tolerances are derived from."""
import math

import numpy as np

SR, HOP, WINDOW, F0_FLOOR, F0_CEIL, THRESHOLD = 22050, 256, 1024, 71.0, 800.0, 0.15


def lags(sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    return int(math.ceil(sr / f0_ceil)), int(math.floor(sr / f0_floor))


def yin(wav, length=None, dtype=np.float64, sr=SR, hop=HOP, window=WINDOW, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, thr=THRESHOLD):
    """wav: 1-D; only wav[:length] is read.  -> (f0 (T,), margin (T,)) in fp64, T = 1 + length // hop."""
    dt = np.dtype(dtype).type
    n = len(wav) if length is None else int(length)
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    W, S = int(window), int(window) + tau_max
    y = np.zeros(max(n, S), dtype=dt)
    y[:n] = np.asarray(wav[:n]).astype(dt)
    T = 1 + n // hop
    f0, margin = np.zeros(T), np.full(T, np.inf)
    taus = np.arange(1, tau_max + 1)
    for t in range(T):
        s0 = min(max(t * hop - S // 2, 0), max(n - S, 0))
        x = y[s0:s0 + S]
        shifted = np.lib.stride_tricks.sliding_window_view(x, W)[1:tau_max + 1]       # row tau - 1 = x[tau : tau + W]
        e = x[None, :W] - shifted
        d = np.sum(e * e, axis=1, dtype=dt)
        cs = np.cumsum(d, dtype=dt)
        dp = np.ones(tau_max + 1, dtype=dt)
        nz = cs > 0
        dp[1:][nz] = d[nz] * taus.astype(dt)[nz] / cs[nz]
        found, m = -1, np.inf
        under = np.nonzero(dp[tau_min:tau_max] < dt(thr))[0]
        if len(under):
            tau = tau_min + int(under[0])
            m = float(np.min(np.abs(dp[tau_min:tau + 1].astype(np.float64) - thr)))
            while tau + 1 < tau_max and dp[tau + 1] < dp[tau]:
                m = min(m, abs(float(dp[tau + 1]) - float(dp[tau])))
                tau += 1
            if tau + 1 < tau_max:
                m = min(m, abs(float(dp[tau + 1]) - float(dp[tau])))
            found = tau
        else:
            m = float(np.min(np.abs(dp[tau_min:tau_max].astype(np.float64) - thr)))
        margin[t] = m
        if found > 0:
            a, b, c = dp[found - 1], dp[found], dp[found + 1]
            den = a - dt(2) * b + c
            off = dt(0.5) * (a - c) / den if den != 0 else dt(0)
            if abs(off) > 1:
                off = dt(0)
            f0[t] = float(dt(sr) / (dt(found) + off))
    return f0, margin


def phoneme_prosody(f0, energy, dur, T=None, dtype=np.float64):
    """One utterance: f0, energy 1-D frame level (T frames of them are valid), dur 1-D ints ->
    (status, pitch (Lp,), energy (Lp,), pitch_mean, pitch_std), zeros with a non-zero status."""
    from scipy.interpolate import interp1d
    dt = np.dtype(dtype).type
    dur = np.asarray(dur, dtype=np.int64)
    Lp = len(dur)
    T = len(f0) if T is None else int(T)
    n = int(dur.sum())
    zero = (np.zeros(Lp), np.zeros(Lp), 0.0, 0.0)
    if n > T or (dur < 0).any():
        return (2,) + zero
    pitch = np.asarray(f0[:n]).astype(dt)
    en = np.asarray(energy[:n]).astype(dt)
    if np.sum(pitch != 0) <= 1:
        return (1,) + zero
    ids = np.where(pitch != 0)[0]
    fn = interp1d(ids.astype(dt), pitch[ids], fill_value=(pitch[ids[0]], pitch[ids[-1]]), bounds_error=False)
    pitch = fn(np.arange(0, len(pitch)).astype(dt)).astype(dt)
    p_ph, e_ph = np.zeros(Lp, dtype=dt), np.zeros(Lp, dtype=dt)
    pos = 0
    for i, d in enumerate(dur):
        if d > 0:
            p_ph[i] = np.mean(pitch[pos:pos + d], dtype=dt)
            e_ph[i] = np.mean(en[pos:pos + d], dtype=dt)
        pos += d
    has = dur > 0
    logs = np.log(p_ph[has])
    mean, std = np.mean(logs, dtype=dt), np.std(logs, dtype=dt)
    if not std > 0:
        return (3,) + zero
    out = np.zeros(Lp, dtype=dt)
    out[has] = (logs - mean) / std
    return 0, out.astype(np.float64), e_ph.astype(np.float64), float(mean), float(std)


def harmonic(freq, n, amps=(1.0, 0.5, 0.3), scale=0.4, sr=SR):
    """A steady tone of harmonics k = 1.. with amplitudes `amps` and phases k, times `scale`."""
    t = np.arange(n) / sr
    return (scale * sum(a * np.sin(2 * np.pi * k * freq * t + k) for k, a in enumerate(amps, 1))).astype(np.float32)


def glide(n, rng, f_lo=120.0, swing=60.0, sr=SR, hop=HOP, noise=(35, 50), silent=(80, 90), peak=0.6):
    """The composite signal: f(t) = f_lo + swing sin(2 pi 1.3 t) + 40 t / t_end + 3 sin(2 pi 5.5 t), five harmonics
    (1, 0.6, 0.4, 0.25, 0.1) with phases k at `peak`, frames `noise` replaced by uniform noise in +-0.2, frames `silent` zero,
    Gaussian noise of sigma 0.003 on top."""
    t = np.arange(n) / sr
    f = f_lo + swing * np.sin(2 * np.pi * 1.3 * t) + 40 * t / t[-1] + 3 * np.sin(2 * np.pi * 5.5 * t)
    ph = 2 * np.pi * np.cumsum(f) / sr
    v = sum(a * np.sin(k * ph + k) for k, a in enumerate((1.0, 0.6, 0.4, 0.25, 0.1), 1))
    y = v / np.max(np.abs(v)) * peak
    if noise:
        a, b = noise[0] * hop, min(noise[1] * hop, n)
        y[a:b] = rng.uniform(-0.2, 0.2, max(b - a, 0))
    if silent:
        a, b = silent[0] * hop, min(silent[1] * hop, n)
        y[a:b] = 0
    y += rng.normal(0, 0.003, n)
    return y.astype(np.float32)
