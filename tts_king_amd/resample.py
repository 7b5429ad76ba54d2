"""Waveforms at the caller's sample rate: the polyphase filter and the segment tables of ttsk_resample (include/ttsk.h).

in = the generator's rate, out = the caller's, g = gcd(in, out), L = out / g, M = in / g, F = max(L, M).  The prototype low-pass is a
Kaiser-windowed sinc on the integers k of the upsampled domain, |k| < half = Z * F:

    g(k) = L * 2 fc * sinc(2 fc k) * I0(beta * sqrt(1 - (k / half)^2)) / I0(beta),    fc = rho / (2 F)

and the resampled signal is y[m] = sum_j x[j] g(m M - j L).  The kernel reads it as L phases of P taps, T[p][q] = g(p + (q - C) L)
(zero where |k| >= half), so that with u = m M, p = u mod L, j0 = u div L

    y[m] = sum_{q = 0 .. P-1} T[p][q] x[j0 + C - q].

C = (half + L - 2) // L taps lie before x[j0]'s and (half - 1) // L after it, P = their sum + 1: the fewest columns that hold every
k with |k| < half for every phase, so the table form IS the sum above, tap for tap.  (A phase p > 0 reaches one tap further back
than phase 0: k = p - C L is inside the support while -C L is not.  2 ((half - 1) // L) + 1 columns, centred, would drop those
taps -- up to L - 1 of them, each about 4e-6 of the passband gain -- and with them the equality with the direct sum.)

An utterance of n samples gives ceil(n L / M).  The table is built in fp64 and stored as fp32.  The segment table tells the kernel
where every utterance lies in the flat buffer and where its resampled samples go: lengths are data, a graph holds per (N, rate).
"""
import functools
import math

import numpy as np

Z = 32          # zero crossings of the sinc on either side, in periods of the lower rate (16 leaves a transition band a third of the passband wide)
BETA = 8.6      # Kaiser window
RHO = 0.93      # cutoff as a fraction of the lower Nyquist
MAX_FACTOR = 1024
ROW = 4         # int32 per segment row (TTSK_SEG_ROW): src_off, src_len, dst_off, dst_len


def check_rate(rate, what="sample_rate"):
    """`rate` as an int, or ValueError: a rate is a positive integer (Hz)."""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) <= 0:
        raise ValueError("%s must be a positive integer number of Hz, got %r" % (what, rate))
    return int(rate)


def factor(in_rate, out_rate):
    """(L, M) = (out, in) / gcd.  ValueError when either exceeds MAX_FACTOR: the table has L rows of about 64 * max(1, M / L) taps."""
    in_rate, out_rate = check_rate(in_rate, "the generator's sampling rate"), check_rate(out_rate)
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    if L > MAX_FACTOR or M > MAX_FACTOR:
        raise ValueError("sample_rate %d against %d Hz reduces to %d / %d: both terms of the reduced ratio must be at most %d"
                         % (out_rate, in_rate, L, M, MAX_FACTOR))
    return L, M


def prototype(k, L, M):
    """g(k) in fp64 for an integer array k (zero where |k| >= half)."""
    F = max(L, M)
    half = Z * F
    fc = RHO / (2.0 * F)
    k = np.asarray(k, dtype=np.float64)
    inside = np.abs(k) < half
    r = np.where(inside, k / half, 0.0)
    g = L * 2.0 * fc * np.sinc(2.0 * fc * k) * np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA)
    return np.where(inside, g, 0.0)


def table64(L, M):
    """(P, C, the (L, P) table in fp64): T[p][q] = g(p + (q - C) L)."""
    half = Z * max(L, M)
    C = (half + L - 2) // L
    P = C + (half - 1) // L + 1
    k = np.arange(L, dtype=np.int64)[:, None] + (np.arange(P, dtype=np.int64)[None, :] - C) * L
    return P, C, prototype(k, L, M)


@functools.lru_cache(maxsize=None)
def design(in_rate, out_rate):
    """(L, M, P, C, table): table (L, P) fp32, read-only, `table64` rounded once.  Cached per pair of rates."""
    L, M = factor(in_rate, out_rate)
    P, C, t64 = table64(L, M)
    table = np.ascontiguousarray(t64.astype(np.float32))
    table.setflags(write=False)
    return L, M, P, C, table


class Filter:
    """A filter on a device: L, M, P, C and `table`, the fp32 device tensor ttsk_resample reads -- tap-major, (P, L): T[p][q] at [q][p]."""

    def __init__(self, L, M, P, C, table):
        self.L, self.M, self.P, self.C, self.table = int(L), int(M), int(P), int(C), table


_on_device = {}


def filter_for(in_rate, out_rate, device):
    """The filter of a pair of rates on `device` (a torch device), its table uploaded once per device."""
    import torch
    device = torch.device(device)
    key = (int(in_rate), int(out_rate), device.type, device.index if device.index is not None else torch.cuda.current_device())
    f = _on_device.get(key)
    if f is None:
        L, M, P, C, table = design(int(in_rate), int(out_rate))
        f = _on_device[key] = Filter(L, M, P, C, torch.from_numpy(np.ascontiguousarray(table.T)).to(device))
    return f


def out_len(n, L, M):
    """Samples an utterance of n samples gives: ceil(n L / M)."""
    return -(-int(n) * int(L) // int(M))


def out_bound(n_src, rows, L, M, align=1):
    """Samples the destination of `rows` segments that share n_src source samples needs at most: a bound that depends on no length."""
    return out_len(n_src, L, M) + int(rows) * int(align)      # every segment rounds up by less than 1, then to the alignment


class Segments:
    """table    (rows, ROW) int32 numpy: one row per utterance in the order given, empty padding rows (all zero) last
       spans    per utterance (dst_off, dst_len)
       n_dst    samples of the destination the table needs (the end of the last segment, or the bound it was built for)"""

    def __init__(self, table, spans, n_dst):
        self.table, self.spans, self.n_dst = table, spans, int(n_dst)


def segments(src_offs, src_lens, L, M, rows=None, align=1, n_dst=None):
    """The segment table of utterances at `src_offs` (samples) of `src_lens` samples: every dst_len = ceil(src_len L / M), the
    dst_off ascending, non-overlapping and multiples of `align` (1: back to back).  `rows`: pad the table to that many rows;
    `n_dst`: the destination's size when it is fixed ahead (a graph's output buffer) -- a table that does not fit it is refused."""
    src_offs, src_lens = [int(o) for o in src_offs], [int(n) for n in src_lens]
    if len(src_offs) != len(src_lens) or any(o < 0 for o in src_offs) or any(n < 0 for n in src_lens) or align < 1:
        raise ValueError("segments: offsets and lengths must pair up and be non-negative, the alignment at least 1")
    rows = len(src_lens) if rows is None else int(rows)
    if rows < len(src_lens):
        raise ValueError("segments: %d utterances do not fit %d rows" % (len(src_lens), rows))
    table = np.zeros((rows, ROW), dtype=np.int64)
    spans, off = [], 0
    for r, (o, n) in enumerate(zip(src_offs, src_lens)):
        m = out_len(n, L, M)
        table[r] = (o, n, off, m) if n else (0, 0, 0, 0)
        spans.append((off, m))
        off = -(-(off + m) // align) * align
    end = max([o + m for o, m in spans], default=0)
    if n_dst is None:
        n_dst = end
    if end > n_dst or table.max(initial=0) >= 2 ** 31:
        raise ValueError("segments: the resampled utterances end at sample %d, the destination holds %d (int32 offsets)" % (end, n_dst))
    return Segments(table.astype(np.int32), spans, n_dst)


def plan_segments(plan, spf, L, M, align=1):
    """The segment table of a window plan (tts_king_amd/windows.py): one row per planned utterance, in the order of the flat
    native-rate buffer, padded to the plan's N rows; the destination is sized by N alone (`out_bound`), so a graph's table and
    output keep their shapes whatever the lengths."""
    offs = [plan.offsets[i] * spf for i in plan.planned]
    lens = [plan.lens[i] * spf for i in plan.planned]
    return segments(offs, lens, L, M, rows=plan.N, align=align, n_dst=out_bound(plan.N * plan.W * spf, plan.N, L, M, align))


def row_segments(B, n, L, M):
    """B rows of n samples each, (B, n) contiguous -> (B, ceil(n L / M)) contiguous."""
    return segments([b * n for b in range(B)], [n] * B, L, M)


def split(flat, plan, spf, short):
    """`windows.split` for a flat buffer that may have been resampled (`plan.segs` set by the route that did): the call's waveforms
    in the call's order, the planned utterances cut from the flat buffer as (1, 1, ceil(spf T_i L / M)), the others from `short`."""
    if plan.segs is None:
        from . import windows
        return windows.split(flat, plan, spf, short)
    out = [None] * len(plan.lens)
    for i, (o, m) in zip(plan.planned, plan.segs.spans):
        out[i] = flat[o:o + m].reshape(1, 1, m)
    for i, y in short.items():
        out[i] = y
    return out
