"""CPU: the fp64 restatement of the YIN kernel finds what it should (tests/pitch_ref.py is the yardstick of tests/test_pitch_gpu.py, so
it is pinned here on signals whose pitch is known), the TextGrid reader and the reference's alignment rules on a hand-written file,
and the host statistics of the data preparation (tts_king_amd/preprocess.py) on arrays."""
import numpy as np
import pytest

from tests import pitch_ref
from tts_king_amd import preprocess, textgrid

TONES = (75.0, 80.0, 110.0, 155.3, 220.0, 331.7, 440.0, 700.0, 790.0)


@pytest.mark.parametrize("freq", TONES)
def test_restatement_finds_steady_tones(freq):
    """Three harmonics (1, 0.5, 0.3; phases k; scale 0.4), 12 hops: every frame voiced, within 1e-3 of the tone.  Measured with
    these rules: at most 5.8e-4 (790 Hz, where a period is 28 samples and the parabola through three lags is coarsest), at most
    2.3e-4 up to 440 Hz."""
    f0, _ = pitch_ref.yin(pitch_ref.harmonic(freq, pitch_ref.HOP * 12))
    assert f0.shape == (13,)
    assert (f0 > 0).all(), f0
    err = np.max(np.abs(f0 / freq - 1))
    print("%.1f Hz: max relative error %.2e" % (freq, err))
    assert err <= 1e-3


def test_restatement_fp32_is_close_to_fp64_on_a_tone():
    a, _ = pitch_ref.yin(pitch_ref.harmonic(155.3, pitch_ref.HOP * 12))
    b, _ = pitch_ref.yin(pitch_ref.harmonic(155.3, pitch_ref.HOP * 12), dtype=np.float32)
    assert (b > 0).all() and np.max(np.abs(b / a - 1)) < 1e-5


@pytest.mark.parametrize("value", [0.0, 0.37])
def test_silence_and_dc_are_unvoiced_and_finite(value):
    f0, margin = pitch_ref.yin(np.full(pitch_ref.HOP * 12 + 5, value, dtype=np.float32))
    assert np.isfinite(f0).all() and (f0 == 0).all()
    assert np.isfinite(margin).all()


def test_short_input_slides_inward_and_pads_with_zeros():
    """len < S: one window start (0), zeros from len on; frames still come out, finite."""
    f0, _ = pitch_ref.yin(pitch_ref.harmonic(220.0, 700))
    assert f0.shape == (1 + 700 // 256,) and np.isfinite(f0).all()


def test_prosody_restatement_by_hand():
    """Two phonemes of 2 and 3 frames and a zero-length one; frame 1 unvoiced between 100 and 200, the last frame after the last voiced."""
    f0 = np.array([100.0, 0.0, 200.0, 400.0, 0.0, 999.0])
    en = np.array([1.0, 3.0, 2.0, 4.0, 6.0, 99.0])
    st, p, e, mean, std = pitch_ref.phoneme_prosody(f0, en, [2, 0, 3])
    logs = np.log([125.0, (200.0 + 400.0 + 400.0) / 3])
    assert st == 0 and p[1] == 0 and e[1] == 0
    assert np.allclose([mean, std], [logs.mean(), logs.std()], rtol=1e-14)
    assert np.allclose(p[[0, 2]], (logs - logs.mean()) / logs.std(), rtol=1e-12)
    assert np.allclose(e, [2.0, 0.0, 4.0])
    assert pitch_ref.phoneme_prosody(f0, en, [4, 3])[0] == 2                     # 7 frames of durations, 6 of audio
    assert pitch_ref.phoneme_prosody(np.array([0, 0, 50.0, 0]), en[:4], [2, 2])[0] == 1
    assert pitch_ref.phoneme_prosody(np.array([50.0, 0, 50.0, 0]), en[:4], [2, 2])[0] == 3


TEXTGRID = '''File type = "ooTextFile"
Object class = "TextGrid"

xmin = 0
xmax = 1.3
tiers? <exists>
size = 2
item []:
    item [1]:
        class = "IntervalTier"
        name = "words"
        xmin = 0
        xmax = 1.3
        intervals: size = 1
        intervals [1]:
            xmin = 0
            xmax = 1.3
            text = "say ""hi"""
    item [2]:
        class = "IntervalTier"
        name = "phones"
        xmin = 0
        xmax = 1.3
        intervals: size = 7
        intervals [1]:
            xmin = 0
            xmax = 0.1
            text = "sil"
        intervals [2]:
            xmin = 0.1
            xmax = 0.25
            text = "S"
        intervals [3]:
            xmin = 0.25
            xmax = 0.5
            text = "EY1"
        intervals [4]:
            xmin = 0.5
            xmax = 0.62
            text = "sp"
        intervals [5]:
            xmin = 0.62
            xmax = 1.0
            text = "HH"
        intervals [6]:
            xmin = 1.0
            xmax = 1.190
            text = "AY1"
        intervals [7]:
            xmin = 1.190
            xmax = 1.3
            text = "sil"
'''

SHORT_TEXTGRID = 'File type = "ooTextFile short"\n"TextGrid"\n\n0\n1.3\n<exists>\n1\n"IntervalTier"\n"phones"\n0\n1.3\n1\n0\n1.3\n"A"\n'


def test_textgrid_long_format_and_alignment_rules(tmp_path):
    p = tmp_path / "u.TextGrid"
    p.write_text(TEXTGRID)
    assert textgrid.read_tier(str(p), "words") == [(0.0, 1.3, 'say "hi"')]
    ivs = textgrid.read_tier(str(p), "phones")
    assert len(ivs) == 7 and ivs[1] == (0.1, 0.25, "S")
    phones, durs, start, end = textgrid.get_alignment(ivs, 22050, 256)
    # frame marks round(t * 22050 / 256): 0.1 -> 8.61 -> 9; 0.25 -> 21.53 -> 22; 0.5 -> 43.07 -> 43; 0.62 -> 53.40 -> 53;
    # 1.0 -> 86.13 -> 86; 1.19 -> 102.498 -> 102 (just under a half); the leading and the trailing sil are dropped, the inner sp stays
    assert phones == ["S", "EY1", "sp", "HH", "AY1"]
    assert durs == [22 - 9, 43 - 22, 53 - 43, 86 - 53, int(np.round(1.19 * 22050 / 256)) - 86]
    assert durs[-1] == 16 and (start, end) == (0.1, 1.19)
    # a rounding case with an exact half: 128 / 256 = 0.5 -> 0 (half to even), 384 / 256 = 1.5 -> 2
    assert textgrid.get_alignment([(128 / 22050, 384 / 22050, "A")], 22050, 256)[1] == [int(np.round(1.5) - np.round(0.5))]
    with pytest.raises(textgrid.TextGridError, match="no interval tier named 'tones'"):
        textgrid.read_tier(str(p), "tones")


def test_textgrid_other_formats_are_refused_by_name(tmp_path):
    p = tmp_path / "s.TextGrid"
    p.write_text(SHORT_TEXTGRID)
    with pytest.raises(textgrid.TextGridError, match="short-format"):
        textgrid.read_tier(str(p))
    p.write_bytes(b"ooBinaryFile\x08TextGrid" + bytes(20))
    with pytest.raises(textgrid.TextGridError, match="binary"):
        textgrid.read_tier(str(p))
    p.write_text("hello\n")
    with pytest.raises(textgrid.TextGridError, match="not a Praat TextGrid"):
        textgrid.read_tier(str(p))


def test_only_silence_gives_an_empty_alignment():
    phones, durs, start, end = textgrid.get_alignment([(0.0, 0.5, "sil"), (0.5, 1.0, "sp")], 22050, 256)
    assert phones == [] and durs == [] and start >= end


def test_remove_outlier_is_the_1p5_iqr_rule():
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 100.0, -50.0])
    p25, p75 = np.percentile(v, 25), np.percentile(v, 75)
    keep = preprocess.remove_outlier(v)
    assert keep.tolist() == [x for x in v if p25 - 1.5 * (p75 - p25) < x < p75 + 1.5 * (p75 - p25)] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    assert preprocess.remove_outlier(np.zeros(0)).size == 0


def test_running_stats_equal_one_pass_over_everything():
    rng = np.random.default_rng(3)
    parts = [rng.normal(5.0, 2.0, n) for n in (1, 17, 300, 2)] + [np.zeros(0)]
    rs = preprocess.RunningStats()
    for p in parts:
        rs.update(p.astype(np.float32) if len(p) == 17 else p)
    allv = np.concatenate([p.astype(np.float32).astype(np.float64) if len(p) == 17 else p for p in parts])
    assert rs.n == allv.size
    assert abs(rs.mean - allv.mean()) <= 1e-13 * abs(allv.mean())
    assert abs(rs.std - allv.std()) <= 1e-13 * allv.std()


def test_normalize_pass_rewrites_the_value_files_only(tmp_path):
    d = tmp_path / "pitch"
    d.mkdir()
    a, b = np.array([1.0, 2.0, 4.0]), np.array([-3.0, 0.5], dtype=np.float32)
    np.save(d / "s-pitch-a.npy", a)
    np.save(d / "s-pitch-b.npy", b)
    np.save(d / "s-pitch-mean-a.npy", np.float64(7.0))
    np.save(d / "s-pitch-std-a.npy", np.float64(9.0))
    np.save(d / "s-cwt-pitch-a.npy", np.ones((3, 11)))
    lo, hi = preprocess.normalize_dir(str(d), 0.5, 2.0)
    assert (lo, hi) == ((-3.0 - 0.5) / 2.0, (4.0 - 0.5) / 2.0)
    assert np.array_equal(np.load(d / "s-pitch-a.npy"), (a - 0.5) / 2.0)
    assert np.load(d / "s-pitch-b.npy").dtype == np.float64
    assert float(np.load(d / "s-pitch-mean-a.npy")) == 7.0 and float(np.load(d / "s-pitch-std-a.npy")) == 9.0
    assert np.array_equal(np.load(d / "s-cwt-pitch-a.npy"), np.ones((3, 11)))


def test_peak_normalize_clamps_full_scale():
    x = np.array([-0.5, 0.25, 0.5, 0.1])
    y = preprocess.peak_normalize(x, 32768.0)
    assert y.dtype == np.float32
    assert y.tolist() == [-1.0, 16384 / 32768, 32767 / 32768, np.float32(np.trunc(0.2 * 32768) / 32768)]
    with pytest.raises(ValueError, match="silent"):
        preprocess.peak_normalize(np.zeros(4), 32768.0)
