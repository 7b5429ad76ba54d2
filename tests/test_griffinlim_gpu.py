"""GPU: the fp32 FFT kernels of csrc/griffinlim.hip behind tts_king_amd/audio.py (STFT, griffin_lim, mel_to_spec, GriffinLimVocoder)
against the fp64 restatement tests/griffinlim_ref.py.  u = 2^-24; every test prints measured over bar before it asserts.

(A) transform: per frame, || mag (cos, sin)(phase) - Z ||_2 <= (8 log2 n_fft + 8) u ||Z||_2 (Higham Thm 24.2, eta ~ 6.7 u per stage with
    one-ulp twiddles; + 8 for the window product and atan2f).
(B) inverse from a given (mag, phase): per sample u / wss (( 8 log2 n_fft + 8) sum_t ||f_t||_2 + (n_fft / hop + 3) sum_t |w f_t[n]|) over the frames
    covering the sample (f_t the windowed frame, times the window once more: griffinlim_ref.inverse_bar); exactly 0 where wss == 0.
(C) one step, momentum 0 and 0.99, B = 1 and B = 2 with lens: (B)'s bar with 32 in place of the first 8; Zprev_out at (A)'s bar; x = 0 gives
    inverse(m, 0) at (B)'s bar.
(D) griffin_lim with lens on B = 2 equals each row's own call bit for bit after 4 iterations; zeros past a row's end.
(E) mel_to_spec: relative error <= (filters covering the bin + 4) u; uncovered bins exactly 0.
(F) argument refusals: an error code and text, nothing written.
(G) the loop: C(x) = || |STFT(x)| - m ||_F / ||m||_F within 1 % of the fp64 restatement's at 0, 1, 2, 4, 8, 16, 32 iterations, non-increasing.
Facade: TTSKing.mel_to_wav(vocoder="griffin_lim") sizes, peak, list == solo, and the default route's bytes unchanged; and with
`mi355x.vocoder: griffin_lim` at three other preprocess_configs (40 mels at 512 / 128 / 512 and 16 kHz, 128 mels, hop 4 with a padded window).
Shapes: T at the minimum the reflect padding allows and at 24, B = 2 with lens (24, minimum).

Measured on an MI355X (the per-configuration table is in DESIGN.md section 21): (A) 1.5e-07 .. 1.7e-07 against bars of 3.3e-06 .. 5.7e-06;
(B) at most 0.023 of its bar, the 34 and 391 samples in the gaps of (64, 32, 16) exactly 0; (C) at most 0.005 of its bar, Zprev_out
1.0e-07 .. 1.4e-07, from silence at most 0.019; (D) every sample equal; (E) 0.53 of its bar at both widths; (G) C equal to the fp64
restatement's to 1.2e-07 relative at every count, momentum 0.99 at 32 iterations 0.136 / 0.164 / 0.150 against 0.190 / 0.217 / 0.202."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import griffinlim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U
IDS = lambda c: "%d-%d-%d" % c if isinstance(c, tuple) else str(c)      # noqa: E731


@functools.lru_cache(maxsize=None)
def stft_of(cfg):
    from tts_king_amd.audio import STFT
    return STFT(*cfg)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(cfg, T, seed=3):
    """(x float32 (hop (T-1),), Z = stft(x) fp64, target m = |Z| g with g uniform in [0.5, 2] as float32, phases in [0, 2 pi) as float32)."""
    n_fft, hop, win = cfg
    x = R.signal(hop * (T - 1), seed + T)
    Z = R.stft(x, *cfg)
    r = np.random.RandomState(seed)
    m = (np.abs(Z) * r.uniform(0.5, 2.0, Z.shape)).astype(np.float32)
    ph = (r.rand(*Z.shape) * 2 * np.pi).astype(np.float32)
    return x, Z, m, ph


def shapes(cfg):
    return (R.min_frames(cfg[0], cfg[1]), 24)


# ------------------------------------------------------------------------------------------------ (A) transform

def transform_error(mag, phase, Z):
    got = mag * np.cos(phase) + 1j * mag * np.sin(phase)
    return float((np.linalg.norm(got - Z, axis=0) / np.linalg.norm(Z, axis=0)).max())


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
def test_transform(cfg):
    n_fft, hop, win = cfg
    s, bar = stft_of(cfg), R.transform_bar(n_fft)
    Tmin = shapes(cfg)[0]
    for T in shapes(cfg):
        x, Z = case(cfg, T)[:2]
        mag, phase = s.transform(dev(x[None]))
        assert mag.shape == phase.shape == (1, n_fft // 2 + 1, T)
        e = transform_error(host(mag)[0], host(phase)[0], Z)
        print("transform %s T %d: %.2e / bar %.2e" % (cfg, T, e, bar))
        assert e <= bar
    # B = 2 with lens: row 1 is the short signal, reflects about its own end and never reads what lies behind it
    x0, Z0 = case(cfg, 24)[:2]
    x1, Z1 = case(cfg, Tmin)[:2]
    y = np.full((2, len(x0)), np.nan, np.float32)
    y[0], y[1, :len(x1)] = x0, x1
    mag, phase = s.transform(dev(y), lens=[len(x0), len(x1)])
    mag, phase = host(mag), host(phase)
    e0, e1 = transform_error(mag[0], phase[0], Z0), transform_error(mag[1, :, :Tmin], phase[1, :, :Tmin], Z1)
    print("transform %s B 2 lens (24, %d): %.2e, %.2e / bar %.2e" % (cfg, Tmin, e0, e1, bar))
    assert e0 <= bar and e1 <= bar
    assert (mag[1, :, Tmin:] == 0).all() and (phase[1, :, Tmin:] == 0).all()


# ------------------------------------------------------------------------------------------------ (B) inverse

def inverse_ratio(got, m, ph, cfg, first=8):
    """max over samples of |got - istft| / bar, and whether the samples where the bar is 0 are exactly 0."""
    Y = m.astype(np.float64) * np.exp(1j * ph.astype(np.float64))
    want, bar = R.istft(Y, *cfg), R.inverse_bar(Y, *cfg, first=first)
    assert got.shape == want.shape, (got.shape, want.shape)
    gap = bar == 0
    return float((np.abs(got - want)[~gap] / bar[~gap]).max()), bool((got[gap] == 0).all()), int(gap.sum())


@pytest.mark.parametrize("cfg", R.CONFIGS + [R.GAPPED], ids=IDS)
def test_inverse(cfg):
    n_fft, hop, win = cfg
    s = stft_of(cfg)
    Tmin = shapes(cfg)[0]
    for T in shapes(cfg):
        _, _, m, ph = case(cfg, T)
        y = s.inverse(dev(m[None]), dev(ph[None]))
        assert y.shape == (1, 1, hop * (T - 1))
        ratio, zeros, n_gap = inverse_ratio(host(y)[0, 0], m, ph, cfg)
        print("inverse %s T %d: %.3f of its bar; %d samples with wss == 0, exactly 0: %s" % (cfg, T, ratio, n_gap, zeros))
        assert ratio <= 1.0 and zeros and (n_gap > 0) == (cfg == R.GAPPED)
    m0, ph0 = case(cfg, 24)[2:]
    m1, ph1 = case(cfg, Tmin)[2:]
    mb, pb = np.full((2,) + m0.shape, np.nan, np.float32), np.full((2,) + m0.shape, np.nan, np.float32)
    mb[0], pb[0], mb[1, :, :Tmin], pb[1, :, :Tmin] = m0, ph0, m1, ph1
    y = host(s.inverse(dev(mb), dev(pb), lens=[24, Tmin]))[:, 0]
    n1 = hop * (Tmin - 1)
    r0, z0, _ = inverse_ratio(y[0], m0, ph0, cfg)
    r1, z1, _ = inverse_ratio(y[1, :n1], m1, ph1, cfg)
    print("inverse %s B 2 lens (24, %d): %.3f, %.3f of the bars" % (cfg, Tmin, r0, r1))
    assert r0 <= 1.0 and r1 <= 1.0 and z0 and z1 and (y[1, n1:] == 0).all()


# ------------------------------------------------------------------------------------------------ (C) one step

def one_step(cfg, x, m, momentum=0.0, zprev=None):
    """The kernel's step from a signal: (x' (n,), Zprev_out (nbins, T) complex or None)."""
    from tts_king_amd import ops
    s = stft_of(cfg)
    win, tw = s.tables(torch.device(DEV))
    T = m.shape[1]
    out = torch.empty(1, T, cfg[0], device=DEV)
    zp = None
    if momentum > 0:
        zp = dev(np.stack([zprev.real.T, zprev.imag.T], axis=-1)[None])
    ops.griffinlim_step(dev(x[None]), dev(m[None]), None, cfg[0], cfg[1], win, tw, out, zp, momentum)
    y = host(ops.istft_ola(out, None, cfg[1], win))[0]
    if zp is None:
        return y, None
    z = host(zp)[0]
    return y, (z[..., 0] + 1j * z[..., 1]).T


def step_case(cfg, T, momentum):
    """(x, m, the given Zprev, Z = stft(x), the fp64 step's signal, its bar) for one row of (C)."""
    x, Z, m, _ = case(cfg, T)
    r = np.random.RandomState(T)
    # a given Zprev that keeps the projection well conditioned: |Zprev| <= |Z| / 2, any phase, so |A| >= 0.75 |Z| and m <= 2 |Z| < 3 |A|
    zprev = (Z * r.uniform(0, 0.5, Z.shape) * np.exp(2j * np.pi * r.rand(*Z.shape))).astype(np.complex64).astype(np.complex128)
    A = Z - momentum / (1 + momentum) * zprev if momentum > 0 else Z
    assert (m <= 2 * np.abs(Z) * (1 + 1e-6)).all() and (m <= 3 * np.abs(A)).all()
    Y = R.polar(m.astype(np.float64), A)
    return x, m, zprev, Z, R.istft(Y, *cfg), R.inverse_bar(Y, *cfg, first=32)


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
def test_one_step(cfg, momentum):
    n_fft, hop, win = cfg
    for T in shapes(cfg):
        x, m, zprev, Z, want, bar = step_case(cfg, T, momentum)
        got, zout = one_step(cfg, x, m, momentum, zprev)
        ratio = float((np.abs(got - want) / bar).max())
        line = "step %s T %d momentum %g: %.3f of its bar" % (cfg, T, momentum, ratio)
        if momentum > 0:
            ez = float((np.linalg.norm(zout - Z, axis=0) / np.linalg.norm(Z, axis=0)).max())
            line += "; Zprev_out %.2e / bar %.2e" % (ez, R.transform_bar(n_fft))
            assert ez <= R.transform_bar(n_fft), line
        print(line)
        assert ratio <= 1.0, line


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
def test_one_step_ragged_batch(cfg, momentum):
    """B = 2 with lens (24, minimum): each row of one launch is held to (C)'s bar against its own fp64 step.  Everything behind the
    short row is NaN on the way in (signal, target, Zprev), so a read past a row's end shows; its frames past its count are not
    written (the closing overlap-add gives zeros there) and its Zprev past its count stays as given."""
    from tts_king_amd import ops
    n_fft, hop, win = cfg
    s = stft_of(cfg)
    wd, tw = s.tables(torch.device(DEV))
    lens = (24, shapes(cfg)[0])
    rows = [step_case(cfg, T, momentum) for T in lens]
    nb = n_fft // 2 + 1
    xb = np.full((2, hop * 23), np.nan, np.float32)
    mb = np.full((2, nb, 24), np.nan, np.float32)
    zb = np.full((2, 24, nb, 2), np.nan, np.float32)
    for b, (T, (x, m, zprev, _, _, _)) in enumerate(zip(lens, rows)):
        xb[b, :len(x)], mb[b, :, :T] = x, m
        zb[b, :T] = np.stack([zprev.real.T, zprev.imag.T], axis=-1)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.empty(2, 24, n_fft, device=DEV)
    zp = dev(zb) if momentum > 0 else None
    ops.griffinlim_step(dev(xb), dev(mb), dl, n_fft, hop, wd, tw, out, zp, momentum)
    y = host(ops.istft_ola(out, dl, hop, wd))
    line = "step %s B 2 lens %s momentum %g:" % (cfg, lens, momentum)
    for b, (T, (_, _, _, Z, want, bar)) in enumerate(zip(lens, rows)):
        n = hop * (T - 1)
        ratio = float((np.abs(y[b, :n] - want) / bar).max())
        line += " row %d %.3f of its bar" % (b, ratio)
        assert ratio <= 1.0 and (y[b, n:] == 0).all(), line
        if momentum > 0:
            z = host(zp)[b]
            ez = float((np.linalg.norm((z[:T, :, 0] + 1j * z[:T, :, 1]).T - Z, axis=0) / np.linalg.norm(Z, axis=0)).max())
            line += ", Zprev_out %.2e / bar %.2e" % (ez, R.transform_bar(n_fft))
            assert ez <= R.transform_bar(n_fft) and np.isnan(z[T:]).all(), line
    print(line)


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
def test_one_step_from_silence(cfg):
    """x = 0: every |Z| is exactly 0, the phase is atan2(0, 0) = 0 and the step gives inverse(m, 0)."""
    T = 24
    _, _, m, _ = case(cfg, T)
    assert (m > 0).all()
    got, _ = one_step(cfg, np.zeros(cfg[1] * (T - 1), np.float32), m)
    ratio, _, _ = inverse_ratio(got, m, np.zeros_like(m), cfg)
    print("step from silence %s: %.3f of the inverse's bar" % (cfg, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ (D) batch equals solo

@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("cfg", [(64, 16, 64), (1024, 256, 1024)], ids=IDS)
def test_batch_equals_solo_bit_for_bit(cfg, momentum):
    from tts_king_amd.audio import griffin_lim
    s = stft_of(cfg)
    Tmin = shapes(cfg)[0]
    m0, ph0 = case(cfg, 24)[2:]
    m1, ph1 = case(cfg, Tmin)[2:]
    mb, pb = np.full((2,) + m0.shape, np.nan, np.float32), np.full((2,) + m0.shape, np.nan, np.float32)
    mb[0], pb[0], mb[1, :, :Tmin], pb[1, :, :Tmin] = m0, ph0, m1, ph1
    both = griffin_lim(dev(mb), s, 4, momentum=momentum, phase0=dev(pb), lens=[24, Tmin])
    a = griffin_lim(dev(m0[None]), s, 4, momentum=momentum, phase0=dev(ph0[None]))
    b = griffin_lim(dev(m1[None]), s, 4, momentum=momentum, phase0=dev(ph1[None]))
    # the same magnitudes handed over frame-major (a transposed view): the layout is the caller's
    a_t = griffin_lim(dev(np.ascontiguousarray(m0.T)).t().unsqueeze(0), s, 4, momentum=momentum, phase0=dev(ph0[None]))
    torch.cuda.synchronize()
    assert torch.equal(a_t, a)
    n1 = cfg[1] * (Tmin - 1)
    assert both.shape == (2, cfg[1] * 23) and b.shape == (1, n1)
    assert torch.isfinite(both).all()
    assert torch.equal(both[0], a[0]) and torch.equal(both[1, :n1], b[0]) and bool((both[1, n1:] == 0).all())
    print("batch == solo %s momentum %g: %d and %d samples equal bit for bit, %d zeros behind the short row" % (cfg, momentum, a.numel(), n1, cfg[1] * 23 - n1))


# ------------------------------------------------------------------------------------------------ (E) mel_to_spec

@pytest.mark.parametrize("mcfg", [(1024, 256, 1024, 80, 22050, 0, 8000), (512, 128, 512, 40, 16000, 50, 7600)], ids=["80mels", "40mels"])
def test_mel_to_spec(mcfg):
    from tts_king_amd.audio import TacotronSTFT, mel_to_spec
    st = TacotronSTFT(*mcfg, device=DEV)
    n_mels, nbins, T = mcfg[3], mcfg[0] // 2 + 1, 37
    mel = np.random.RandomState(n_mels).uniform(-9.0, 2.0, (2, n_mels, T)).astype(np.float32)
    got = host(mel_to_spec(dev(mel), st))
    fb = st.mel_basis.cpu().numpy()
    assert fb.shape == (n_mels, nbins) and fb.dtype == np.float32 and got.shape == (2, nbins, T)
    start, off = st._ex.fb_start.cpu().numpy(), st._ex.fb_off.cpu().numpy()
    k = np.arange(nbins)[None, :]
    cover = ((k >= start[:, None]) & (k < (start + np.diff(off))[:, None])).sum(axis=0)
    want = np.stack([R.mel_to_spec(mel[b], fb) for b in range(2)])
    none = cover == 0
    rel = np.abs(got[:, ~none] / want[:, ~none] - 1) / ((cover[~none] + 4) * U)[None, :, None]
    print("mel_to_spec %d mels: %.3f of its bar (%d..%d filters per covered bin), %d uncovered bins exactly 0: %s"
          % (n_mels, rel.max(), cover[~none].min(), cover.max(), none.sum(), bool((got[:, none] == 0).all())))
    assert none.any() and (got[:, none] == 0).all() and (want[:, ~none] > 0).all()
    assert rel.max() <= 1.0


def test_inv_mel_spec_writes_the_wav(tmp_path):
    """All T frames are used (the reference drops the last one): hop * (T - 1) samples, float32, at the STFT's sampling rate; and the
    audio's spectrum is nearer the target than the random-phase start is (C after 0 iterations is above 0.5 on every case of (G))."""
    from scipy.io import wavfile
    from tts_king_amd.audio import TacotronSTFT, inv_mel_spec, mel_to_spec
    st = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000, device=DEV)
    x = R.signal(256 * 23, 4)
    mel, _ = st.mel_spectrogram(dev(x[None]))
    assert mel.shape == (1, 80, 24)
    path = str(tmp_path / "out.wav")
    audio = inv_mel_spec(mel[0].cpu(), path, st, griffin_iters=8)
    rate, data = wavfile.read(path)
    assert rate == 22050 and data.dtype == np.float32 and data.shape == (256 * 23,) and np.array_equal(data, audio)
    assert np.isfinite(data).all()
    m = host(mel_to_spec(mel, st))[0]
    cfg = (1024, 256, 1024)
    c = R.convergence(data.astype(np.float64), m, *cfg)
    # the phases are torch's, so the yardstick is the fp64 restatement from three other random starts: C after 8 iterations varies by
    # about 5 % with the start (0.25 .. 0.27 here, 0.60 .. 0.65 before the first iteration); the bar is 1.25 x the largest of the three
    ref = [R.convergence(R.griffin_lim(m, np.random.RandomState(k).rand(*m.shape) * 2 * np.pi, *cfg, 8), m, *cfg) for k in range(3)]
    print("inv_mel_spec: %d samples at %d Hz, C after 8 iterations %.4f; fp64 restatement from three starts %s"
          % (len(data), rate, c, " ".join("%.4f" % v for v in ref)))
    assert c <= 1.25 * max(ref)


# ------------------------------------------------------------------------------------------------ (F) refusals

def test_entry_point_refusals():
    from tts_king_amd import lib, ops
    L = lib.load()
    s = stft_of((64, 16, 64))
    win, tw = s.tables(torch.device(DEV))
    P, S = ops._ptr, ops._stream()
    wav = torch.zeros(2, 128, device=DEV)
    mag, ph = torch.full((2, 33, 9), 7.0, device=DEV), torch.full((2, 33, 9), 7.0, device=DEV)
    frames, frames2 = torch.full((2, 9, 64), 7.0, device=DEV), torch.full((2, 9, 64), 7.0, device=DEV)
    out = torch.full((2, 128), 7.0, device=DEV)
    spec = torch.full((2, 33, 9), 7.0, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    good = dict(B=2, len=128, n_fft=64, hop=16, T=9)

    def polar(**kw):
        a = dict(good, **kw)
        return L.ttsk_stft_polar(P(wav), None, a["B"], a["len"], a["n_fft"], a["hop"], P(win), P(tw), P(mag), P(ph), a["T"], S)

    def frames_of(**kw):
        a = dict(good, **kw)
        return L.ttsk_istft_frames(P(mag), P(ph), 33 * 9, 9, 1, None, a["B"], a["T"], a["n_fft"], a["hop"], P(win), P(tw), P(frames), S)

    def ola(**kw):
        a = dict(good, **kw)
        return L.ttsk_istft_ola(P(frames), None, a["B"], a["T"], a["n_fft"], a["hop"], P(win), P(out), S)

    def step(src=None, fin=None, mom=0.0, zp=None, **kw):
        a = dict(good, **kw)
        return L.ttsk_griffinlim_step(src, 128, fin, P(mag), 33 * 9, 9, 1, None, zp, mom, a["B"], a["T"], a["n_fft"], a["hop"], P(win), P(tw),
                                      P(frames2), S)

    calls = [("ttsk_stft_polar", polar, c) for c in (dict(n_fft=96), dict(n_fft=32), dict(n_fft=4096), dict(hop=24), dict(hop=0), dict(T=8),
                                                      dict(len=32, T=3), dict(B=0), dict(B=70000))]
    calls += [("ttsk_istft_frames", frames_of, c) for c in (dict(n_fft=100), dict(hop=5), dict(T=0), dict(B=0))]
    calls += [("ttsk_istft_ola", ola, c) for c in (dict(T=1), dict(n_fft=48), dict(hop=-16))]
    calls += [("ttsk_griffinlim_step", step, c) for c in (dict(src=P(wav), fin=P(frames)), dict(), dict(fin=P(frames2)), dict(src=P(wav), mom=1.0),
                                                           dict(src=P(wav), mom=0.5), dict(src=P(wav), T=3), dict(src=P(wav), hop=7))]
    for name, fn, change in calls:
        with pytest.raises(lib.TtskError, match=name):
            lib.check(fn(**change), name)
    with pytest.raises(lib.TtskError, match="ttsk_mel_to_spec"):
        lib.check(L.ttsk_mel_to_spec(P(mag), P(wav), P(i32), P(i32), 2, 0, 33, 9, 1000.0, P(spec), S), "ttsk_mel_to_spec")
    with pytest.raises(lib.TtskError, match="ttsk_istft"):
        lib.check(L.ttsk_istft(P(mag), P(ph), 33 * 9, 9, 1, None, 2, 9, 64, 16, P(win), P(tw), None, P(out), S), "ttsk_istft")
    torch.cuda.synchronize()
    for t in (mag, ph, frames, frames2, out, spec):
        assert bool((t == 7.0).all())
    print("refusals: %d calls refused by name, nothing written" % (len(calls) + 2))


# ------------------------------------------------------------------------------------------------ (G) the loop

COUNTS = (0, 1, 2, 4, 8, 16, 32)


@pytest.mark.parametrize("cfg,T", [((64, 16, 64), 24), ((1024, 256, 1024), 12), ((256, 64, 200), 20)], ids=IDS)
def test_loop_spectral_convergence(cfg, T):
    from tts_king_amd.audio import griffin_lim
    s = stft_of(cfg)
    x = R.signal(cfg[1] * (T - 1), 11)
    m = np.abs(R.stft(x, *cfg)).astype(np.float32)
    phase0 = (np.random.RandomState(5).rand(*m.shape) * 2 * np.pi).astype(np.float32)
    m64 = m.astype(np.float64)
    want = [R.convergence(v, m64, *cfg) for v in R.griffin_lim(m64, phase0, *cfg, 32, keep=COUNTS).values()]
    got = [R.convergence(host(griffin_lim(dev(m[None]), s, n, phase0=dev(phase0[None])))[0], m64, *cfg) for n in COUNTS]
    fast = R.convergence(host(griffin_lim(dev(m[None]), s, 32, momentum=0.99, phase0=dev(phase0[None])))[0], m64, *cfg)
    print("loop %s T %d: C at %s iterations" % (cfg, T, COUNTS))
    print("  fp64   %s" % " ".join("%.4f" % c for c in want))
    print("  kernel %s   worst relative difference %.2e (bar 1e-2)" % (" ".join("%.4f" % c for c in got),
                                                                      max(abs(g / w - 1) for g, w in zip(got, want))))
    print("  momentum 0.99 at 32 iterations: %.4f (plain %.4f); a record, no bar" % (fast, got[-1]))
    assert all(abs(g / w - 1) <= 0.01 for g, w in zip(got, want))
    assert all(b <= a + 1e-6 for a, b in zip(got, got[1:]))


# ------------------------------------------------------------------------------------------------ facade

def test_facade_griffin_lim_route(tmp_path):
    import yaml
    import tts_king
    from tts_king_amd.audio import GriffinLimVocoder
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config.yaml")))
    cfg["preprocess_config"]["path"]["preprocessed_path"] = os.path.join(ROOT, "pretrained")
    cfg["mi355x"]["hip_graph"] = False
    p = tmp_path / "config.yaml"
    p.write_text(yaml.safe_dump(cfg))
    tts = tts_king.TTSKing(str(p))
    assert not isinstance(tts.vocoder, GriffinLimVocoder)
    r = np.random.RandomState(1)
    mel = torch.from_numpy(r.uniform(-8.0, 0.5, (1, 24, 80)).astype(np.float32))
    short = torch.from_numpy(r.uniform(-8.0, 0.5, (1, 9, 80)).astype(np.float32))
    wav = tts.mel_to_wav(mel, vocoder="griffin_lim", griffin_iters=8)
    peak = int(np.abs(wav.astype(np.int32)).max())
    print("facade: %s %s, peak %d (0.95 * 32767 = %d)" % (wav.dtype, wav.shape, peak, round(0.95 * 32767)))
    assert wav.dtype == np.int16 and wav.shape == (1, 1, 256 * 23) and abs(peak - round(0.95 * 32767)) <= 1
    solo = tts.mel_to_wav(short, vocoder="griffin_lim", griffin_iters=8)
    both = tts.mel_to_wav([mel, short], vocoder="griffin_lim", griffin_iters=8)
    assert solo.shape == (1, 1, 256 * 8) and len(both) == 2
    assert np.array_equal(both[0], wav) and np.array_equal(both[1], solo)
    f = tts._vocoder("griffin_lim")(mel.transpose(1, 2), griffin_iters=8)
    assert f.dtype == torch.float32 and f.shape == (1, 1, 256 * 23) and abs(float(f.abs().max()) - 0.95) <= 1e-6
    up = tts.mel_to_wav(mel, vocoder="griffin_lim", griffin_iters=8, sample_rate=44100)
    assert up.dtype == np.int16 and up.shape == (1, 1, 2 * 256 * 23)
    # the default route is the HiFi-GAN one, byte for byte
    assert np.array_equal(tts.mel_to_wav(mel), tts.vocoder.generate(mel.transpose(1, 2)))
    assert np.array_equal(tts.mel_to_wav(mel, vocoder="hifigan"), tts.mel_to_wav(mel))


# (n_mel_channels, filter_length, hop_length, win_length, sampling_rate, mel_fmin, mel_fmax): what the route exists for.  None is a
# configuration mel extraction takes together with a HiFi-GAN checkpoint: the second has more than MelExtractor's 80 mels, the third
# a hop that is no multiple of 8 and a centre-padded window.
OTHER_CONFIGS = [(40, 512, 128, 512, 16000, 50, 7600), (128, 1024, 256, 1024, 22050, 0, 8000), (24, 64, 4, 48, 8000, 0, None)]


def scaled_convergence(x, m, cfg):
    """C(a x) at the a that minimises it: the vocoder scales every utterance to a peak of 0.95, so its amplitude carries no information."""
    s = np.abs(R.stft(x, *cfg))
    return float(np.linalg.norm((s * m).sum() / (s * s).sum() * s - m) / np.linalg.norm(m))


@pytest.mark.parametrize("vc", OTHER_CONFIGS, ids=["40mels-512-128-512", "128mels-1024-256-1024", "24mels-64-4-48"])
def test_facade_at_other_configurations(monkeypatch, cfg, vc):
    """`mi355x.vocoder: griffin_lim` with another preprocess_config: TTSKing builds a GriffinLimVocoder from it and no HIFIapi (text-to-mel
    is a stub: no FastSpeech2 checkpoint exists at these widths either), and mel_to_wav runs at that width, STFT and rate.
    The filterbank and mel-to-linear are held to (E)'s bar; sizes, peak and list == solo as at the shipped configuration; and after 8
    iterations the audio's spectrum is as near the target as the fp64 restatement gets from other random starts (the phases are
    torch's).  In fp64, over 8 starts, C after 8 iterations is 0.24 .. 0.28, 0.25 .. 0.29 and 0.28 .. 0.39 at the three configurations
    and 0.50 or more before the first; the bar is 1.25 x the largest of three starts, as in test_inv_mel_spec_writes_the_wav."""
    import copy
    import tts_king
    from tts_king_amd.audio import GriffinLimVocoder, mel_to_spec, slaney_mel_filterbank
    n_mels, n_fft, hop, win, sr, fmin, fmax = vc
    scfg = (n_fft, hop, win)
    c = copy.deepcopy(cfg)
    pp = c["preprocess_config"]["preprocessing"]
    pp["stft"].update(filter_length=n_fft, hop_length=hop, win_length=win)
    pp["mel"].update(n_mel_channels=n_mels, mel_fmin=fmin, mel_fmax=fmax)
    pp["audio"]["sampling_rate"] = sr
    c["mi355x"]["vocoder"] = "griffin_lim"

    class NoTextToMel:
        speaker_names = []

        def __init__(self, config, gpu):
            pass

    def no_hifigan(config, gpu):
        raise AssertionError("mi355x.vocoder: griffin_lim must not build a HIFIapi")

    monkeypatch.setattr(tts_king, "load_config", lambda path: c)
    monkeypatch.setattr(tts_king, "FSTWOapi", NoTextToMel)
    monkeypatch.setattr(tts_king, "HIFIapi", no_hifigan)
    tts = tts_king.TTSKing("unused.yaml")
    voc = tts.vocoder
    assert isinstance(voc, GriffinLimVocoder) and voc.sampling_rate == sr and not hasattr(voc, "_ex")
    assert (voc.n_mel_channels, voc.stft_fn.filter_length, voc.stft_fn.hop_length, voc.stft_fn.win_length) == vc[:4]

    fb = slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    Tmin = R.min_frames(n_fft, hop)

    def mel_of(T, seed):                        # the log-mel of a signal, formed in fp64: (n_mels, T) float32
        return np.log(np.maximum(fb.astype(np.float64) @ np.abs(R.stft(R.signal(hop * (T - 1), seed), *scfg)), 1e-5)).astype(np.float32)

    mel, short = mel_of(24, 4), mel_of(Tmin, 5)
    # (E) on the vocoder's own filterbank
    got = host(mel_to_spec(dev(mel[None]), voc))[0]
    want = R.mel_to_spec(mel, fb)
    start, off = voc.fb.start.cpu().numpy(), voc.fb.off.cpu().numpy()
    k = np.arange(n_fft // 2 + 1)[None, :]
    cover = ((k >= start[:, None]) & (k < (start + np.diff(off))[:, None])).sum(axis=0)
    none = cover == 0
    rel = float((np.abs(got[~none] / want[~none] - 1) / ((cover[~none] + 4) * U)[:, None]).max())
    assert (want[~none] > 0).all() and (got[none] == 0).all() and rel <= 1.0, rel

    as_arg = lambda a: torch.from_numpy(np.ascontiguousarray(a.T[None]))       # noqa: E731    (1, T, n_mels), as generate_mel returns it
    wav = tts.mel_to_wav(as_arg(mel), griffin_iters=8)
    peak = int(np.abs(wav.astype(np.int32)).max())
    assert wav.dtype == np.int16 and wav.shape == (1, 1, hop * 23) and abs(peak - round(0.95 * 32767)) <= 1
    solo = tts.mel_to_wav(as_arg(short), griffin_iters=8)
    both = tts.mel_to_wav([as_arg(mel), as_arg(short)], griffin_iters=8)
    assert solo.shape == (1, 1, hop * (Tmin - 1)) and np.array_equal(both[0], wav) and np.array_equal(both[1], solo)

    y = host(voc(dev(mel[None]), griffin_iters=8))[0, 0]
    c8 = scaled_convergence(y, want, scfg)
    ref = [scaled_convergence(R.griffin_lim(want, np.random.RandomState(s).rand(*want.shape) * 2 * np.pi, *scfg, 8), want, scfg) for s in range(3)]
    print("facade %s: mel_to_spec %.3f of its bar (%d uncovered bins exactly 0), peak %d, list == solo, C after 8 iterations %.4f; "
          "fp64 restatement from three starts %s" % (vc, rel, none.sum(), peak, c8, " ".join("%.4f" % v for v in ref)))
    assert c8 <= 1.25 * max(ref)
