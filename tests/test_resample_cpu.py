"""CPU: the sample-rate converter's filter design, table form and segment planning (tts_king_amd/resample.py) against the fp64
reference written from the definition (tests/resample_ref.py).  The quality bars are conditions on the constants Z, beta, rho: the
reference alone meets them (DESIGN.md section 16 has the figures)."""
import inspect

import numpy as np
import pytest

from tests import resample_ref as ref
from tts_king_amd import resample, windows

IN = 22050
RATES = (8000, 11025, 16000, 24000, 32000, 44100, 48000)


def _db(v):
    return 20.0 * np.log10(max(float(v), 1e-300))


def _tone(rate, f, n=6000):
    """(y, the ideal output sine, the middle half) of a 6000-sample sine of f Hz through the fp64 reference."""
    L, M = ref.factor(IN, rate)
    y = ref.resample(np.sin(2 * np.pi * f * np.arange(n) / IN), L, M)
    to = np.arange(len(y)) / rate
    return y, np.sin(2 * np.pi * f * to), slice(len(y) // 4, 3 * len(y) // 4), to


def _rel_rms_db(e):
    return _db(np.sqrt(np.mean(e ** 2)) / np.sqrt(0.5))


def test_reference_index_convention_against_upfirdn():
    """The direct sum is scipy's upfirdn of the prototype, read from sample half - 1 on, every M-th."""
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(0).standard_normal(300)
    for rate in (8000, 16000, 44100, 48000):
        L, M = ref.factor(IN, rate)
        half = ref.Z * max(L, M)
        h = ref.g(np.arange(-half + 1, half), L, M)
        y = ref.resample(x, L, M)
        want = signal.upfirdn(h, x, up=L)[half - 1::M][:len(y)]
        assert len(want) == len(y) and np.abs(y - want).max() <= 1e-13, rate


@pytest.mark.parametrize("rate", RATES)
def test_table_form_reproduces_direct_sum(rate):
    L, M, P, C, table = resample.design(IN, rate)
    assert (L, M) == ref.factor(IN, rate)
    half = ref.Z * max(L, M)
    assert table.shape == (L, P) and table.dtype == np.float32
    P64, C64, t64 = resample.table64(L, M)
    assert (P64, C64) == (P, C) and t64.dtype == np.float64
    k = np.arange(L)[:, None] + (np.arange(P)[None, :] - C) * L
    assert np.array_equal(t64, ref.g(k, L, M))                      # the same function of k, entry by entry
    assert np.array_equal(table, t64.astype(np.float32))            # built in fp64, rounded once
    # no tap of the prototype is lost and no column is spare: every |k| < half is p + (q - C) L for exactly one (p, q), the first
    # and the last column each hold one
    inside = np.sort(k[np.abs(k) < half])
    assert np.array_equal(inside, np.arange(-half + 1, half))
    assert (np.abs(k[:, 0]) < half).any() and (np.abs(k[:, -1]) < half).any()
    rng = np.random.default_rng(rate)
    for n in (1, 2, 37, 700):
        x = rng.standard_normal(n)
        y, yt = ref.resample(x, L, M), ref.table_form(x, t64, L, M, C)
        assert yt.shape == y.shape == (-(-n * L // M),)
        # the same products in another order: fp64 summation rounding only
        assert np.all(np.abs(yt - y) <= (P + 2) * 2.0 ** -53 * ref.weight(x, L, M) + 1e-300), (rate, n)


def test_design_sizes_of_the_service_rates():
    # one column more than 2 ((half - 1) // L) + 1: the phases p > 0 reach one tap further back than phase 0
    assert resample.design(IN, 8000)[:4] == (160, 441, 178, 89)
    assert resample.design(IN, 16000)[:4] == (320, 441, 90, 45)
    assert resample.design(IN, 48000)[:4] == (320, 147, 64, 32)
    assert resample.design(IN, 44100)[:4] == (2, 1, 64, 32)
    assert resample.design(IN, 11025)[:4] == (1, 2, 127, 63)                     # L = 1: one phase, symmetric
    assert resample.design(IN, 8000)[4] is resample.design(IN, 8000)[4]          # cached per pair
    assert (resample.Z, resample.BETA, resample.RHO) == (32, 8.6, 0.93) == (ref.Z, ref.BETA, ref.RHO)


@pytest.mark.parametrize("rate", RATES)
def test_passband_error_of_the_design(rate):
    """<= -80 dB at 0.02 / 0.5 / 0.8 of the lower Nyquist, <= -60 dB at 0.85 (measured: -88.9 dB and -65.3 dB worst)."""
    nyq = min(IN, rate) / 2
    for c, bar in ((0.02, -80.0), (0.5, -80.0), (0.8, -80.0), (0.85, -60.0)):
        y, ideal, mid, _ = _tone(rate, c * nyq)
        err = _rel_rms_db((y - ideal)[mid])
        print("rate %d tone %.2f Nyquist: error %.1f dB" % (rate, c, err))
        assert err <= bar, (rate, c, err)


@pytest.mark.parametrize("rate", [r for r in RATES if r < IN])
def test_stopband_residue_when_downsampling(rate):
    """A tone at 1.05 and 1.3 of the output Nyquist leaves <= -90 dB (measured: -95.0 dB worst)."""
    for c in (1.05, 1.3):
        f = c * rate / 2
        assert f < IN / 2
        y, _, mid, _ = _tone(rate, f)
        res = _rel_rms_db(y[mid])
        print("rate %d tone %.2f output Nyquist: residue %.1f dB" % (rate, c, res))
        assert res <= -90.0, (rate, c, res)


@pytest.mark.parametrize("rate", [r for r in RATES if r > IN])
def test_images_when_upsampling(rate):
    """What is left of a 0.8 Nyquist tone after its least-squares removal (images, window ripple): measured on the reference at
    -98.5 dB (24, 32, 48 kHz) and -96.7 dB (44.1 kHz); the bar is 5 dB above the worst of them."""
    f = 0.8 * IN / 2
    y, _, mid, to = _tone(rate, f)
    A = np.stack([np.sin(2 * np.pi * f * to), np.cos(2 * np.pi * f * to)], 1)[mid]
    c = np.linalg.lstsq(A, y[mid], rcond=None)[0]
    res = _rel_rms_db(y[mid] - A @ c)
    print("rate %d: images %.1f dB" % (rate, res))
    assert res <= -91.7, (rate, res)


def test_refusals_name_the_rule():
    with pytest.raises(ValueError, match="at most 1024"):
        resample.design(IN, 22051)
    for bad in (0, -8000, 16000.0, "16000", None, True):
        with pytest.raises(ValueError, match="positive integer"):
            resample.factor(IN, bad)
    assert resample.factor(IN, np.int64(16000)) == (320, 441)


@pytest.mark.parametrize("align", [1, 1024])
def test_segment_table_of_a_window_plan(align):
    lens = [130, 20, 300, 96, 1]
    plan = windows.plan_windows(lens, windows.W, 14, short_rows=True)
    L, M = resample.factor(IN, 16000)
    sg = resample.plan_segments(plan, 256, L, M, align=align)
    t = sg.table
    assert t.dtype == np.int32 and t.shape == (plan.N, resample.ROW) and plan.N > len(lens)
    n = len(plan.planned)
    assert np.array_equal(t[:n, 0], [plan.offsets[i] * 256 for i in plan.planned])       # the stitch's layout at the native rate
    assert np.array_equal(t[:n, 1], [lens[i] * 256 for i in plan.planned])
    assert np.array_equal(t[:n, 3], [-(-lens[i] * 256 * L // M) for i in plan.planned])
    assert not t[n:].any()                                                               # padding rows are empty
    assert not (t[:n, 2] % align).any() and t[0, 2] == 0
    assert np.all(t[1:n, 2] >= t[:n - 1, 2] + t[:n - 1, 3])                              # ascending, non-overlapping
    if align == 1:
        assert np.array_equal(t[1:n, 2], t[:n - 1, 2] + t[:n - 1, 3])                    # back to back
    assert t[n - 1, 2] + t[n - 1, 3] <= sg.n_dst == resample.out_bound(plan.N * plan.W * 256, plan.N, L, M, align)
    # the destination's size depends on N alone
    other = windows.plan_windows([150, 97, 200], windows.W, 14, short_rows=True)
    if other.N == plan.N:
        assert resample.plan_segments(other, 256, L, M, align=align).n_dst == sg.n_dst


def test_output_bound_holds_for_the_fullest_plan():
    """Every row a one-frame utterance: the most round-ups a plan of N rows can hold."""
    for rate in (8000, 16000, 48000):
        L, M = resample.factor(IN, rate)
        plan = windows.plan_windows([1] * 12, windows.W, 14, short_rows=True)
        sg = resample.plan_segments(plan, 256, L, M)
        assert sg.spans[-1][0] + sg.spans[-1][1] <= sg.n_dst
    with pytest.raises(ValueError, match="destination holds"):
        resample.segments([0, 100], [100, 100], 2, 1, n_dst=399)


def test_split_returns_the_calls_order():
    lens = [20, 130, 0, 97]
    plan = windows.plan_windows(lens, windows.W, 14, short_rows=True)
    assert plan.short == [2]
    L, M = resample.factor(IN, 8000)
    plan.segs = resample.plan_segments(plan, 256, L, M, align=64)
    flat = np.full(plan.segs.n_dst, -1, dtype=np.int64)
    for i, (o, m) in zip(plan.planned, plan.segs.spans):
        flat[o:o + m] = i
    empty = np.zeros((1, 1, 0), dtype=np.int64)
    out = resample.split(flat, plan, 256, {2: empty})
    assert out[2] is empty
    for i in (0, 1, 3):
        assert out[i].shape == (1, 1, -(-lens[i] * 256 * L // M)) and (out[i] == i).all()
    # a plan nobody resampled is cut as before
    plain = windows.plan_windows(lens, windows.W, 14, short_rows=True)
    a = resample.split(np.arange(plain.frames * 256), plain, 256, {2: empty})
    b = windows.split(np.arange(plain.frames * 256), plain, 256, {2: empty})
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_equal_rows_are_contiguous():
    sg = resample.row_segments(3, 8192, 160, 441)
    m = -(-8192 * 160 // 441)
    assert sg.table.tolist() == [[b * 8192, 8192, b * m, m] for b in range(3)] and sg.n_dst == 3 * m


def test_every_waveform_route_takes_a_sample_rate_defaulting_to_none():
    from hifiapi import HIFIapi
    from tts_king import TTSKing
    from tts_king_amd.hifigan import Generator
    from tts_king_amd.synth import GraphedSynthesizer
    routes = [Generator.forward_windows, Generator.forward_ragged, Generator.forward_ragged_flat, Generator.forward_short, GraphedSynthesizer.wav,
              GraphedSynthesizer.wav_ragged, GraphedSynthesizer.wav_ragged_flat, HIFIapi.generate, HIFIapi.generate_ragged,
              HIFIapi.call_ragged, HIFIapi.__call__, TTSKing.mel_to_wav, TTSKing.speak]
    for fn in routes:
        assert inspect.signature(fn).parameters["sample_rate"].default is None, fn.__qualname__


def test_shipped_config_sets_no_output_rate():
    from tts_king_amd.config import default_config
    assert "output_sample_rate" not in default_config().mi355x
