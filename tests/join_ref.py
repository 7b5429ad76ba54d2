"""numpy restatement of ttsk_wav_join (include/ttsk.h): decisions and the copy in np.float32 in the stated order, the sum of
squares in fp64 besides.  Not a second implementation of the kernels' reduction: `ss` here is the fp64 sum rounded once, which is what
the device's fp32 reduction is measured against (`ss_bound`)."""
import numpy as np

from tts_king_amd import narrate

F32 = np.float32
U_ROUND = 2.0 ** -24        # unit roundoff of fp32


def ss_bound(m):
    """Relative error bound of the device's sum of squares over m samples against the exact sum.  Shape of the reduction (join.hip):
    thread t of 1024 adds the samples of quads t, t + 1024, ... one fma each, so a term passes at most 4 * ceil(m / 4096) roundings in
    its thread; then 6 butterfly steps inside the wave and at most 15 additions over the 16 waves.  All terms are >= 0, so with
    k = 4 * ceil(m / 4096) + 6 + 15 roundings on any term's path the error is at most gamma_k = k u / (1 - k u) of the sum
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), u = 2^-24."""
    k = 4 * -(-int(m) // 4096) + 6 + 15
    return k * U_ROUND / (1.0 - k * U_ROUND)


def gain_bound(m):
    """Relative bound on the device's gain in the modes "rms" / "peak" against the restatement's, which starts from the fp64 sum rounded
    once (error u) where the device's sum has ss_bound(m).  g = target / sqrt(ss / m): the square root halves the error of ss and of
    the division by m (u / 2) and adds its own rounding u, the last division adds u: each side carries e / 2 + 2.5 u, so the two
    differ by at most (ss_bound + u) / 2 + 5 u to first order; the second-order terms are below 1e-3 of that.  limit / peak is one
    division of the same two numbers on both sides, and where the two sides take different branches of the min both gains lie
    between the two values of target / rms."""
    return 1.001 * ((ss_bound(m) + U_ROUND) / 2.0 + 5.0 * U_ROUND)


def fade_weights(m, fade):
    """w(k) for the m kept samples, fp32."""
    F = min(int(fade), m // 2)
    w = np.ones(m, dtype=F32)
    if F > 0:
        k = np.arange(F)
        ramp = (2 * k + 1).astype(F32) / F32(2 * F)
        w[:F] = ramp
        w[m - F:] = ramp[::-1]
    return w


def join_ref(x_flat, table, n_dst, int16_scale=None, g_device=None):
    """x_flat fp32 array, table the (1 + rows, 8) int32 join table -> dict(out, a, b, o, peak, ss64, g, total, timing).  `g_device`: gains
    to use instead of the restatement's own (the device's, for the bit-for-bit comparison of the copy in the modes "rms" / "peak")."""
    x_flat = np.asarray(x_flat, dtype=F32)
    table = np.asarray(table, dtype=np.int32)
    mode, fade, keep, lead = (int(v) for v in table[0, :4])
    r, floor, target, limit = (F32(v) for v in np.ascontiguousarray(table[0, 4:8]).view(F32))
    fade, keep, lead = max(fade, 0), max(keep, 0), max(lead, 0)
    rows = table.shape[0] - 1
    a, b, o = np.zeros(rows, np.int64), np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    peak, g, ss64 = np.zeros(rows, F32), np.ones(rows, F32), np.zeros(rows, np.float64)
    out = np.zeros(int(n_dst), dtype=F32)
    pos = lead
    for u in range(rows):
        off, n, pause, flags = (int(v) for v in table[1 + u, :4])
        gain = np.ascontiguousarray(table[1 + u, 4:5]).view(F32)[0]
        if not (off >= 0 and n > 0 and off + n <= x_flat.size):
            n = 0
        x = x_flat[off:off + n] if n else np.zeros(0, F32)
        ax = np.abs(x)
        pk = F32(ax.max()) if n else F32(0)
        lo, hi = 0, n
        if flags & 1:
            thr = max(F32(pk * r), floor)
            hit = np.nonzero(ax >= thr)[0]
            if hit.size == 0 or not pk > 0:
                lo = hi = 0
            else:
                lo, hi = max(0, int(hit[0]) - keep), min(n, int(hit[-1]) + 1 + keep)
        m = hi - lo
        kept = x[lo:hi]
        s64 = float(np.sum(kept.astype(np.float64) ** 2))
        gu = F32(1)
        if m > 0:
            if mode == narrate.GIVEN:
                gu = gain
            elif pk > 0:
                with np.errstate(divide="ignore"):
                    if mode == narrate.RMS:
                        rms = np.sqrt(F32(F32(s64) / F32(m)))
                        gu = min(F32(target / rms), F32(limit / pk))
                    else:
                        gu = F32(limit / pk)
        if g_device is not None:
            gu = F32(g_device[u])
        a[u], b[u], o[u], peak[u], ss64[u], g[u] = lo, hi, min(pos, 2 ** 31 - 1), pk, s64, gu
        if m > 0:
            y = (kept * gu).astype(F32) * fade_weights(m, fade)
            end = min(pos + m, out.size)
            if end > pos:
                out[pos:end] = y[:end - pos]
        pos += m + max(pause, 0)
    total = min(pos, 2 ** 31 - 1)
    if int16_scale is not None:
        with np.errstate(invalid="ignore"):
            v = np.minimum(np.maximum(out * F32(int16_scale), F32(-32768.0)), F32(32767.0))
        out = np.where(np.isnan(v), F32(-32768.0), v).astype(np.int32).astype(np.int16)
    return dict(out=out, a=a, b=b, o=o, peak=peak, ss64=ss64, g=g, total=total,
                timing=[(int(o[u]), int(o[u] + b[u] - a[u])) for u in range(rows)])
