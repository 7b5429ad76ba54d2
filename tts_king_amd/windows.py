"""Windowed vocoding: utterances of any length, and ragged batches of them, as N fixed-size windows of W mel frames.

The HiFi-GAN generator is a stack of convolutions (hifi/models.py:146-210), so an output sample depends on the mel frames within a
fixed distance of it: the halo H (`receptive_halo`).  An utterance of T >= W frames is cut into overlapping windows of W frames,
the windows of all utterances of a call run through the generator as one rectangular (N, 80, W) batch, and a window contributes
the samples of the frames that lie at least H away from its cuts.  The first window starts at frame 0 and the last ends at frame
T, so the utterance's own edges meet the zero padding of a solo run, and the stitched waveform is the solo waveform up to the
rounding of a different batch shape.  The plan is an int32 table in the layout of include/ttsk.h (TTSK_WIN_ROW), consumed on
the device by ttsk_mel_windows and ttsk_wav_stitch: lengths are data, the only shape left is N, and N is rounded up to a short
ladder so that a service captures a handful of graphs instead of one per length.
"""
import numpy as np

# Frames per window.  One constant, not a config key: every value gives the same audio, so there is nothing for a caller to choose.
# Picked on an MI355X from {64, 96, 128, 192, 256} by tools/window_vocoder_time.py (profiles/window_vocoder_time.json):
# small windows spend 2H / W of the generator's work on halos, large ones send more utterances down the solo route (T < W) and round
# the batch up in coarser steps.  96 and 128 are within 2 % of each other and ahead of the rest; 96 is the faster on all three workloads.
W = 96
ROW = 8                     # int32 per plan row (TTSK_WIN_ROW)
VALID = 6                   # column of a row's valid frames (TTSK_WIN_VALID): 0 = all W, v in 1..W = a short utterance's v frames


def _get(h, key):
    return h[key] if isinstance(h, dict) else getattr(h, key)


def receptive_halo(h):
    """Mel frames on either side of an output sample's own frame that the sample depends on, for the generator configuration `h`.

    Walks the dependency radius from an output sample back to the mel: conv_post (k = 7) adds 3 samples; every stage adds its
    widest resblock (ResBlock1: a dilated and a plain conv per dilation, sum_d ((k-1)/2 d + (k-1)/2); ResBlock2: one conv per
    dilation, sum_d (k-1)/2 d; the MRF average reads the blocks side by side, so the widest counts); a ConvTranspose1d of stride
    u, kernel k, padding (k-u)/2 reaches (k+u)/2 - 1 output samples from input i's position i*u and divides the radius by u,
    rounded up; conv_pre (k = 7) adds 3 frames.  14 for the shipped V1 configuration, 12 for config_v3."""
    kind = str(_get(h, "resblock"))
    ks, ds = list(_get(h, "resblock_kernel_sizes")), [list(d) for d in _get(h, "resblock_dilation_sizes")]
    if kind == "1":
        block = max(sum((k - 1) // 2 * d + (k - 1) // 2 for d in dd) for k, dd in zip(ks, ds))
    else:
        block = max(sum((k - 1) // 2 * d for d in dd) for k, dd in zip(ks, ds))
    r = 3
    for u, k in reversed(list(zip(_get(h, "upsample_rates"), _get(h, "upsample_kernel_sizes")))):
        r += block
        r = -(-(r + (k + u) // 2 - 1) // u)
    return r + 3


def ladder(n):
    """The smallest of 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, ... (neighbours at most 1.5x apart) that is >= n."""
    if n <= 2:
        return max(1, n)
    p = 2
    while True:
        if n <= p + p // 2:
            return p + p // 2
        p *= 2
        if n <= p:
            return p


def window_starts(T, Wn, H):
    """Start frames of the windows of one utterance of T >= Wn frames: n = max(1, ceil((T - 2H) / (Wn - 2H))) of them, from 0 to
    T - Wn, spread evenly; neighbours are at most Wn - 2H apart, which is what lets every frame be kept at least H from a cut."""
    if T < Wn:
        raise ValueError("an utterance of %d frames is shorter than a window of %d" % (T, Wn))
    if Wn <= 2 * H:
        raise ValueError("window of %d frames does not exceed twice the halo %d" % (Wn, H))
    n = max(1, -(-(T - 2 * H) // (Wn - 2 * H)))
    if n == 1:
        return [0]
    return [(i * (T - Wn)) // (n - 1) for i in range(n)]


class Plan:
    """table      (N, ROW) int32 numpy, one row per window, padding rows last (include/ttsk.h: utterance, start, kept lo, kept hi,
                  output frame of lo, staging frame of the window's start or -1, valid frames of the row or 0 = all W)
       n_windows  rows that are real windows;  N = len(table) is on the ladder
       planned    indices (into `lens`) of the utterances that have rows, in table order (T >= W; with `short_rows` every T >= 1);
                  short = the others
       offsets    planned utterance -> its first frame in the staging buffer and in the flat output (both hold the planned utterances
                  back to back); frames = their total, never more than N * W
       has_short_rows  some row holds an utterance shorter than the window (0 < column VALID < W): the generator needs the row lengths
       segs       None, or, set by a route that resampled the flat output, its layout (`resample.Segments`; `resample.split` reads it)"""

    def __init__(self, table, n_windows, planned, short, offsets, frames, lens, Wn, H):
        self.table, self.n_windows, self.planned, self.short = table, n_windows, planned, short
        self.offsets, self.frames, self.lens, self.W, self.H = offsets, frames, lens, Wn, H
        self.N = int(table.shape[0])
        self.segs = None
        self.has_short_rows = bool(self.N) and bool(((table[:, VALID] > 0) & (table[:, VALID] < Wn)).any())


def plan_windows(lens, Wn=None, H=14, short_rows=False):
    """Plan the windows of a call: `lens` = mel frames of every utterance.  Utterances shorter than a window are not planned
    (`Plan.short`): a zero-padded mel is not a solo run, since the reference zero-pads the activations of every layer at the end.
    `short_rows` (for a generator whose kernels take a per-row length, `Generator.short_rows()`): an utterance of 1 <= T < W frames is
    planned too, as ONE row of its own that starts at frame 0, keeps [0, T) and carries T in column VALID — the generator then treats
    the row's frames >= T as non-existent, which is the solo run's zero padding at every layer.  Only empty utterances stay in
    `Plan.short`; a call without short utterances gets the same table either way."""
    Wn = W if Wn is None else int(Wn)
    lens = [int(t) for t in lens]
    least = 1 if short_rows else Wn
    planned = [i for i, t in enumerate(lens) if t >= least]
    short = [i for i, t in enumerate(lens) if t < least]
    rows, offsets, off = [], {}, 0
    for i in planned:
        T = lens[i]
        offsets[i] = off
        if T < Wn:
            rows.append((i, 0, 0, T, off, off, T, 0))
            off += T
            continue
        starts = window_starts(T, Wn, H)
        for j, s in enumerate(starts):
            lo = 0 if j == 0 else s + H
            hi = T if j == len(starts) - 1 else starts[j + 1] + H
            rows.append((i, s, lo, hi, off + lo, off + s, 0, 0))
        off += T
    n = len(rows)
    N = ladder(n) if n else 0
    rows += [(-1, 0, 0, 0, 0, -1, 0, 0)] * (N - n)
    table = np.asarray(rows, dtype=np.int32).reshape(N, ROW)
    return Plan(table, n, planned, short, offsets, off, lens, Wn, H)


def split(flat, plan, spf, short):
    """The call's waveforms in the call's order: the planned utterances cut from the flat buffer (device tensor or host array, as
    ttsk_wav_stitch wrote it) as (1, 1, spf * T_i), the short ones from `short` = {index: waveform}."""
    out = [None] * len(plan.lens)
    for i in plan.planned:
        o, T = plan.offsets[i], plan.lens[i]
        out[i] = flat[o * spf:(o + T) * spf].reshape(1, 1, T * spf)
    for i, y in short.items():
        out[i] = y
    return out
