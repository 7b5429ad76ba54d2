"""fp64 reference of the sample-rate converter (tests/test_resample_cpu.py, tests/test_resample_gpu.py): numpy only, written from the
definition and sharing no code with tts_king_amd/resample.py.

    g(k) = L * 2 fc * sinc(2 fc k) * I0(beta * sqrt(1 - (k / half)^2)) / I0(beta)  for |k| < half = Z * max(L, M),  fc = rho / (2 max(L, M))
    y[m] = sum_j x[j] * g(m * M - j * L),    m in [0, ceil(n * L / M))

by direct evaluation: no phases, no table."""
import math

import numpy as np

Z, BETA, RHO = 32, 8.6, 0.93


def factor(in_rate, out_rate):
    d = math.gcd(in_rate, out_rate)
    return out_rate // d, in_rate // d


def g(k, L, M):
    F = max(L, M)
    half = Z * F
    fc = RHO / (2.0 * F)
    k = np.asarray(k, dtype=np.float64)
    inside = np.abs(k) < half
    t = np.where(inside, k / half, 0.0)
    v = L * 2.0 * fc * np.sinc(2.0 * fc * k) * np.i0(BETA * np.sqrt(1.0 - t * t)) / np.i0(BETA)
    return np.where(inside, v, 0.0)


def _taps(n, L, M, kernel=None, half=None):
    """(j, w): for every output m the candidate input indices j[m, :] and the weights w[m, :] = kernel(m M - j L), zero where j lies
    outside [0, n) or the kernel's support."""
    half = Z * max(L, M) if half is None else half
    kernel = (lambda k: g(k, L, M)) if kernel is None else kernel
    n_out = -(-n * L // M)
    u = np.arange(n_out, dtype=np.int64) * M
    jmin = -((half - 1 - u) // L)                       # ceil((u - half + 1) / L)
    width = (2 * half - 2) // L + 1
    j = jmin[:, None] + np.arange(width, dtype=np.int64)[None, :]
    k = u[:, None] - j * L
    w = np.where((np.abs(k) < half) & (j >= 0) & (j < n), kernel(k), 0.0)
    return np.clip(j, 0, max(n - 1, 0)), w


def resample(x, L, M):
    """y (fp64) of one utterance x."""
    x = np.asarray(x, dtype=np.float64)
    j, w = _taps(len(x), L, M)
    return (x[j] * w).sum(axis=1)


def weight(x, L, M):
    """sum_j |x[j]| |g(m M - j L)| per output sample: the scale of a rounding-error bound."""
    x = np.asarray(x, dtype=np.float64)
    j, w = _taps(len(x), L, M)
    return (np.abs(x[j]) * np.abs(w)).sum(axis=1)


def table_form(x, T, L, M, C, n_out=None):
    """The kernel's formula in the arithmetic of T and x's dtype promoted to at least fp64 or int64: y[m] = sum_q T[p][q] x[j0 + C - q],
    u = m M, p = u mod L, j0 = u div L, x = 0 outside [0, n).  T is (L, P)."""
    T = np.asarray(T)
    x = np.asarray(x)
    n, P = len(x), T.shape[1]
    n_out = -(-n * L // M) if n_out is None else n_out
    u = np.arange(n_out, dtype=np.int64) * M
    p, j0 = u % L, u // L
    j = j0[:, None] + C - np.arange(P, dtype=np.int64)[None, :]
    ok = (j >= 0) & (j < n)
    xv = np.where(ok, x[np.clip(j, 0, max(n - 1, 0))], 0)
    return (T[p] * xv).sum(axis=1)
