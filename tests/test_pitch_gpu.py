"""GPU: ttsk_pitch_yin and ttsk_phoneme_prosody against their fp64 restatements (tests/pitch_ref.py).

How the comparison is made.  YIN takes decisions -- is d'(tau) under the threshold, does the walk go on --
and a decision that is closer to its boundary than fp32 can resolve may fall either way.  The restatement returns each frame's
*margin* (the distance of its closest decision from the boundary); frames with a margin under 1e-4 are left out, and a case may
leave out at most 10 % of its frames.  On every other frame the voiced / unvoiced decision must agree, and on voiced frames f0 is
compared relatively against a bar that is measured, not chosen: the restatement is also run in fp32 on the case's inputs, its
largest relative deviation from fp64 is the error the number format itself causes, and the kernel -- the same arithmetic in another
summation order over 1024 terms -- gets 16 times that.  The phoneme-level kernel's bars are made the same way, per quantity.
Every test prints its figures before it asserts.

Measured on an MI355X (case: frames, share left out, fp32-numpy deviation from fp64, kernel deviation from fp64, bar = 16 x fp32 numpy):
  composite                    121 frames  4.1 %  9.28e-08  9.36e-08  1.48e-06
  length edges (6 rows)         42 frames  0.0 %  5.62e-08  5.62e-08  9.00e-07
  range edges (7 rows)          91 frames  0.0 %  5.55e-08  5.55e-08  8.88e-07
  hop 128, W 512, 100..500 Hz   91 frames  2.2 %  7.43e-08  6.80e-08  1.19e-06
  phoneme level: pitch 5.17e-06 / 2.95e-06 / 8.27e-05, energy 7.86e-08 / 1.05e-07 / 1.26e-06, pitch_mean 1.80e-07 / 1.19e-07 / 2.88e-06,
  pitch_std 2.35e-06 / 2.38e-06 / 3.77e-05 (fp32 numpy / kernel / bar; vectors as max |x - ref| / max |ref| per row, scalars relatively)."""
import numpy as np
import pytest
import torch

from tests import pitch_ref
from tts_king_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN, CAP, FACTOR = 1e-4, 0.10, 16.0
HOP = pitch_ref.HOP
S_DEFAULT = pitch_ref.WINDOW + pitch_ref.lags()[1]


def gpu_yin(rows, lens=None, fill=0.0, **kw):
    """rows: list of 1-D arrays -> (B, T_max) numpy from one launch over the padded batch (`fill` past each row's samples)."""
    ld = max(len(r) for r in rows)
    x = np.full((len(rows), ld), fill, dtype=np.float32)
    for i, r in enumerate(rows):
        x[i, :len(r)] = r
    ln = None
    if lens is not None or any(len(r) != ld for r in rows):
        ln = torch.tensor([len(r) for r in rows] if lens is None else lens, dtype=torch.int32, device=DEV)
    args = dict(sr=kw.get("sr", pitch_ref.SR), hop=kw.get("hop", HOP), window=kw.get("window", pitch_ref.WINDOW),
                f0_floor=kw.get("f0_floor", pitch_ref.F0_FLOOR), f0_ceil=kw.get("f0_ceil", pitch_ref.F0_CEIL),
                threshold=kw.get("thr", pitch_ref.THRESHOLD))
    out = ops.pitch_yin(torch.from_numpy(x).to(DEV), ln, **args)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_case(name, rows, **kw):
    """The comparison of the module docstring over all frames of `rows` taken together; returns the figures."""
    hop = kw.get("hop", HOP)
    got = gpu_yin(rows, **kw)
    assert np.isfinite(got).all(), name
    n_all = n_out = 0
    e32 = egpu = 0.0
    for i, r in enumerate(rows):
        ref, margin = pitch_ref.yin(r, **kw)
        r32, _ = pitch_ref.yin(r, dtype=np.float32, **kw)
        T = 1 + len(r) // hop
        g = got[i, :T].astype(np.float64)
        assert (got[i, T:] == 0).all(), (name, i)
        ok = margin >= MARGIN
        n_all += T
        n_out += int((~ok).sum())
        flips = np.nonzero(ok & ((g > 0) != (ref > 0)))[0]
        assert len(flips) == 0, "%s row %d: voiced / unvoiced differs on frames %s (margins %s)" % (name, i, flips, margin[flips])
        v32 = ok & (ref > 0) & (r32 > 0)
        if v32.any():
            e32 = max(e32, float(np.max(np.abs(r32[v32] / ref[v32] - 1))))
        v = ok & (ref > 0)
        if v.any():
            egpu = max(egpu, float(np.max(np.abs(g[v] / ref[v] - 1))))
    share, bar = n_out / n_all, FACTOR * e32
    print("%s: %d frames, %.1f%% left out, fp32 numpy %.3g, kernel %.3g, bar %.3g" % (name, n_all, 100 * share, e32, egpu, bar))
    assert share <= CAP, "%s: %.1f%% of the frames are marginal in the restatement itself: change the seed" % (name, 100 * share)
    assert egpu <= bar, "%s: kernel deviates %.3g from fp64, bar %.3g = 16 x fp32 numpy's %.3g" % (name, egpu, bar, e32)
    return share, e32, egpu


def test_composite_signal():
    """hop * 120 + 77 samples: a gliding five-harmonic voice, a noise stretch, a silent stretch, a little noise on top."""
    check_case("composite", [pitch_ref.glide(HOP * 120 + 77, np.random.default_rng(0))])


def tone(freq, n, rng):
    """A steady three-harmonic tone with a little noise: voiced however short the row is."""
    return (pitch_ref.harmonic(freq, n) + rng.normal(0, 0.003, n)).astype(np.float32)


def test_length_edges():
    """One row each: shorter than S, exactly S, S + 1, S + hop - 1, and a last frame that lands on / just past the last sample.
    The rows are one case (one launch, one bar over their 42 frames); each row alone, with ld = len and no lens, gives the same bits."""
    S = S_DEFAULT
    rng = np.random.default_rng(1)
    rows = [tone(f, n, rng) for f, n in zip((131.0, 97.3, 155.3, 203.9, 251.0, 88.8), (700, S, S + 1, S + HOP - 1, HOP * 9, HOP * 9 + 1))]
    check_case("length edges", rows)
    batch = gpu_yin(rows)
    for i, r in enumerate(rows):
        T = 1 + len(r) // HOP
        assert (batch[i, :T] > 0).any(), i
        assert np.array_equal(gpu_yin([r])[0], batch[i, :T]), i


def test_ragged_batch_never_reads_past_len_and_equals_solo_runs():
    rng = np.random.default_rng(2)
    lens = [HOP * 30 + 5, 700, HOP * 17, S_DEFAULT + 3, HOP * 30 + 255]
    rows = [pitch_ref.glide(lens[0], rng, noise=(8, 11), silent=(13, 15)), tone(140.0, lens[1], rng), tone(310.0, lens[2], rng),
            tone(76.0, lens[3], rng), pitch_ref.glide(lens[4], rng, noise=(8, 11), silent=(13, 15))]
    a = gpu_yin(rows, fill=np.nan)
    b = gpu_yin(rows, fill=np.nan)
    assert not np.isnan(a).any()
    assert np.array_equal(a, b), "two runs differ"
    assert a.shape == (5, 1 + max(lens) // HOP)
    for i, r in enumerate(rows):
        T = 1 + len(r) // HOP
        assert (a[i, T:] == 0).all()
        assert (a[i, :T] > 0).any()
        padded = np.full(max(lens), np.nan, dtype=np.float32)
        padded[:len(r)] = r
        solo_same_ld = gpu_yin([padded], lens=[len(r)])
        solo_own_ld = gpu_yin([r])
        assert np.array_equal(a[i], solo_same_ld[0]), i
        assert np.array_equal(a[i, :T], solo_own_ld[0]), i


def test_range_edges():
    """Tones just inside the range, tones outside it (compared with whatever the restatement decides), a full-scale square wave,
    silence and DC."""
    n = HOP * 12
    t = np.arange(n) / pitch_ref.SR
    square = np.where(np.sin(2 * np.pi * 210.0 * t) >= 0, 1.0, -1.0).astype(np.float32)
    rows = [pitch_ref.harmonic(75.0, n), pitch_ref.harmonic(790.0, n), pitch_ref.harmonic(60.0, n), pitch_ref.harmonic(1000.0, n), square,
            np.zeros(n, dtype=np.float32), np.full(n, 0.37, dtype=np.float32)]
    check_case("range edges", rows)
    got = gpu_yin(rows)
    assert (got[5] == 0).all() and (got[6] == 0).all()
    assert (got[0] > 0).all() and abs(np.median(got[0]) / 75.0 - 1) < 1e-3
    assert (got[1] > 0).all() and abs(np.median(got[1]) / 790.0 - 1) < 1e-3


def test_non_default_parameters():
    kw = dict(hop=128, window=512, f0_floor=100.0, f0_ceil=500.0)
    check_case("hop 128, W 512, 100..500 Hz", [pitch_ref.glide(128 * 90 + 31, np.random.default_rng(4), f_lo=180.0, hop=128,
                                                                  noise=(20, 30), silent=(50, 58))], **kw)


def test_pitch_yin_refuses_before_launch():
    x = torch.zeros(1, 4096, device=DEV)
    for kw, word in ((dict(f0_ceil=30000.0), "tau_min"), (dict(window=8000), "LDS"), (dict(window=1022), "multiple of 4"),
                     (dict(f0_floor=799.0, f0_ceil=800.0), "tau_max"), (dict(hop=0), "null wav or f0|positive")):
        with pytest.raises(lib.TtskError, match=word):
            ops.pitch_yin(x, **kw)
    with pytest.raises(lib.TtskError, match="no CPU path"):
        ops.pitch_yin(torch.zeros(1, 4096))
    with pytest.raises(lib.TtskError, match="int32"):
        ops.pitch_yin(x, torch.zeros(1, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------ phoneme level


def make_row(rng, Lp, zeros=True, lead=3, trail=4, slack=5, long_run=True, dur=None):
    """(f0, energy, dur): durations 1..8 with zero-length phonemes (first, last and one inside when `zeros`), a leading and a trailing
    unvoiced run, an unvoiced run that spans several phonemes, scattered unvoiced frames, and `slack` frames past sum(dur) that hold
    values no result may depend on."""
    dur = rng.integers(1, 9, Lp) if dur is None else np.asarray(dur)
    if zeros and Lp >= 4:
        dur[0] = dur[-1] = dur[Lp // 2] = 0
    n = int(dur.sum())
    f0 = (100 + 80 * rng.random(n + slack)).astype(np.float32)
    f0[rng.random(n + slack) < 0.2] = 0
    f0[:lead] = 0
    f0[max(n - trail, 0):n] = 0
    if long_run and Lp >= 8:
        pos = np.concatenate([[0], np.cumsum(dur)])
        f0[pos[Lp // 3]:pos[Lp // 3 + 4] + 1] = 0
    f0[n:] = 1e6
    energy = (10 * rng.random(n + slack)).astype(np.float32)
    energy[n:] = -1e6
    return f0, energy, dur.astype(np.int32)


def gpu_prosody(rows):
    B = len(rows)
    ldT, ldL = max(len(r[0]) for r in rows), max(len(r[2]) for r in rows)
    f0, en, dur = np.zeros((B, ldT), np.float32), np.zeros((B, ldT), np.float32), np.full((B, ldL), 7, np.int32)
    for i, (f, e, d) in enumerate(rows):
        f0[i, :len(f)], en[i, :len(e)], dur[i, :len(d)] = f, e, d
    T = torch.tensor([len(r[0]) for r in rows], dtype=torch.int32, device=DEV)
    Lp = torch.tensor([len(r[2]) for r in rows], dtype=torch.int32, device=DEV)
    out = ops.phoneme_prosody(torch.from_numpy(f0).to(DEV), torch.from_numpy(en).to(DEV), torch.from_numpy(dur).to(DEV), T, Lp)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def vec_err(a, ref):
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def good_rows():
    rng = np.random.default_rng(5)
    rows = [make_row(rng, 2, dur=[6, 7], lead=2, trail=2)] + [make_row(rng, Lp) for Lp in (63, 64, 65, 300)]
    rows.append(make_row(rng, 5, zeros=False, lead=0, trail=0, slack=0))
    rows.append(make_row(rng, 512, slack=40))          # ~2300 frames
    f, e, d = make_row(rng, 512, zeros=False, slack=0, lead=700, trail=1)   # many frames per phoneme: up to the 4096-frame mark
    d = (d.astype(np.int64) * 0 + 8).astype(np.int32)
    f = np.resize(f, 4096).copy(); e = np.resize(e, 4096).copy()
    f[4000:] = 0
    rows.append((f, e, d))
    return rows


def test_phoneme_prosody_against_the_restatement(good_rows):
    """Errors: vectors (pitch, energy) as max |x - ref| / max |ref| per row, scalars relatively; bar = 16 x the fp32 restatement's."""
    pitch, en, pmean, pstd, status = gpu_prosody(good_rows)
    worst = {k: [0.0, 0.0] for k in ("pitch", "energy", "mean", "std")}
    for i, (f, e, d) in enumerate(good_rows):
        st, p, q, m, s = pitch_ref.phoneme_prosody(f, e, d)
        st32, p32, q32, m32, s32 = pitch_ref.phoneme_prosody(f, e, d, dtype=np.float32)
        assert st == 0 and st32 == 0 and status[i] == 0, (i, st, st32, status[i])
        Lp = len(d)
        assert (pitch[i, Lp:] == 0).all() and (en[i, Lp:] == 0).all()
        assert (pitch[i, :Lp][d == 0] == 0).all() and (en[i, :Lp][d == 0] == 0).all()
        for k, a32, ag in (("pitch", vec_err(p32, p), vec_err(pitch[i, :Lp], p)), ("energy", vec_err(q32, q), vec_err(en[i, :Lp], q)),
                           ("mean", abs(m32 / m - 1), abs(pmean[i] / m - 1)), ("std", abs(s32 / s - 1), abs(pstd[i] / s - 1))):
            worst[k][0], worst[k][1] = max(worst[k][0], a32), max(worst[k][1], float(ag))
    for k, (a32, ag) in worst.items():
        print("phoneme level %s: fp32 numpy %.3g, kernel %.3g, bar %.3g" % (k, a32, ag, FACTOR * a32))
    for k, (a32, ag) in worst.items():
        assert ag <= FACTOR * a32, (k, ag, FACTOR * a32)


def test_statuses_and_good_rows_unchanged_by_bad_neighbours(good_rows):
    rng = np.random.default_rng(6)
    f, e, d = make_row(rng, 20)
    one_voiced = f.copy(); one_voiced[:int(d.sum())] = 0; one_voiced[3] = 120.0
    too_long = (f[:int(d.sum()) - 1], e[:int(d.sum()) - 1], d)
    # constant pitch: every phoneme mean is 150 exactly, and 16 equal logs sum exactly in any pairing, so the deviation is exactly 0
    ff, fe, fd = make_row(rng, 16, zeros=False)
    flat = np.where(np.arange(len(ff)) % 3 == 0, 0, 150.0).astype(np.float32)
    single = make_row(rng, 1, lead=0, trail=0)                                # one phoneme: the deviation of one value is 0
    bad = [(one_voiced, e, d), too_long, (flat, fe, fd), single]
    want = [1, 2, 3, 3]
    for (bf, be, bd), w in zip(bad, want):
        assert pitch_ref.phoneme_prosody(bf, be, bd)[0] == w
    good = good_rows[:4]
    mixed = [bad[0], good[0], bad[1], good[1], good[2], bad[2], bad[3], good[3]]
    where_good = [1, 3, 4, 7]
    out_m = gpu_prosody(mixed)
    out_g = gpu_prosody(good)
    assert out_m[4].tolist() == [1, 0, 2, 0, 0, 3, 3, 0]
    for j in (0, 2, 5, 6):
        assert (out_m[0][j] == 0).all() and (out_m[1][j] == 0).all() and out_m[2][j] == 0 and out_m[3][j] == 0
    for j, g in zip(where_good, range(4)):
        Lp = len(good[g][2])
        assert np.array_equal(out_m[0][j, :Lp], out_g[0][g, :Lp]) and np.array_equal(out_m[1][j, :Lp], out_g[1][g, :Lp])
        assert out_m[2][j] == out_g[2][g] and out_m[3][j] == out_g[3][g]
    again = gpu_prosody(mixed)
    assert all(np.array_equal(a, b) for a, b in zip(out_m, again))


def test_phoneme_prosody_refuses_sizes_past_its_limits():
    i32 = lambda *s: torch.ones(*s, dtype=torch.int32, device=DEV)
    f = torch.zeros(1, 8193, device=DEV)
    with pytest.raises(lib.TtskError, match="8192"):
        ops.phoneme_prosody(f, f, i32(1, 4), i32(1), i32(1))
    f = torch.zeros(1, 64, device=DEV)
    with pytest.raises(lib.TtskError, match="1024"):
        ops.phoneme_prosody(f, f, i32(1, 1025), i32(1), i32(1))
    ok = ops.phoneme_prosody(torch.zeros(1, 8192, device=DEV), torch.zeros(1, 8192, device=DEV), i32(1, 1024), i32(1) * 8192, i32(1) * 1024)
    assert int(ok[4][0]) == 1                      # 1024 frames of silence: no voiced frame
