"""GPU: mel extraction (tts_king_amd/audio.py -> ttsk_stft_frames, ttsk_gemm in conv-A mode, ttsk_mel_from_spec) across the parameters it
accepts, against the fp64 restatement tests/mel_ref.py.  Every test prints its figures before it asserts.

(A) both call surfaces at the nine configurations of mel_ref.CONFIGS on a broadband input, at the project's stated bar (tests/test_audio_gpu.py):
    log-mel within 1e-4 absolute, energy rtol 1e-4 / atol 1e-5; and at the shortest signal each surface's reflect padding allows.
(B) the same on a tonal input.  A sparse spectrum leaves most mel channels far below the frame's largest bin, where the absolute
    error of any 22..24-bit format is a large log error, so the bar is made as tests/test_pitch_gpu.py makes its bars:
    max(1e-4, 16 x the fp32 oracle's own largest deviation from fp64 on that input), and that bar may not exceed 5e-3.
(C) ttsk_stft_frames alone, bit for bit against mel_ref.stft_rows.
(D) ttsk_mel_from_spec alone against fp64 at both instances, the mel-lane split's edges and hand-made packed tables.  A filter is a sum
    of n_m non-negative fp32 products of magnitudes that carry two roundings, so its linear value is within (n_m + 8) 2^-24
    relative: |d log-mel| <= (n_m + 8) 2^-23 + 4 * 2^-24 |ref|; energy within (nbins + 8) 2^-24 relative.
(E) what is accepted and what is refused: tap counts past 32, amplitudes above 1 on the vocoder surface, argument refusals.
(F) preprocess.Features at configuration (c).

Measured on an MI355X.  Per configuration and surface: largest log-mel deviation from fp64 of the fp32 oracle / of the kernel (/ the bar, where
it is not the fixed 1e-4); 37 frames on the vocoder surface (hifi), 38 on Tacotron's, B = 2; mel_from_spec instance launched:
  a <17>  broadband hifi 7.04e-07 / 7.38e-07, tacotron 1.47e-06 / 7.80e-07;  tonal hifi 3.41e-05 / 6.34e-05 / 5.46e-04, tacotron 6.91e-05 / 7.11e-05 / 1.11e-03
  b <17>  broadband hifi 7.51e-07 / 1.47e-06, tacotron 1.17e-06 / 1.04e-06;  tonal hifi 6.09e-05 / 8.10e-05 / 9.74e-04, tacotron 6.36e-05 / 7.38e-05 / 1.02e-03
  c <9>   broadband hifi 3.99e-07 / 8.33e-07, tacotron 7.64e-07 / 9.44e-07;  tonal hifi 2.14e-05 / 2.36e-05 / 3.42e-04, tacotron 2.93e-05 / 1.83e-05 / 4.68e-04
  d <9>   broadband hifi 4.74e-06 / 3.36e-06, tacotron 5.59e-06 / 2.04e-06;  tonal hifi 1.24e-04 / 1.58e-04 / 1.98e-03, tacotron 6.83e-05 / 1.01e-04 / 1.09e-03
  e <9>   broadband hifi 5.57e-07 / 7.54e-07, tacotron 1.10e-06 / 1.09e-06;  tonal hifi 5.99e-05 / 3.08e-05 / 9.58e-04, tacotron 4.37e-05 / 4.02e-05 / 6.99e-04
  f <9>   broadband hifi 4.98e-07 / 7.55e-07, tacotron 1.04e-06 / 7.52e-07;  tonal hifi 2.30e-05 / 2.21e-05 / 3.67e-04, tacotron 1.96e-05 / 2.63e-05 / 3.14e-04
  g <9>   broadband hifi 1.99e-06 / 1.66e-06, tacotron 1.31e-06 / 1.46e-06;  tonal hifi 3.60e-05 / 2.00e-05 / 5.77e-04, tacotron 3.23e-05 / 2.97e-05 / 5.16e-04
  h <17>  broadband hifi 5.92e-07 / 8.53e-07, tacotron 1.36e-06 / 7.10e-07;  tonal hifi 2.96e-05 / 1.21e-04 / 4.73e-04, tacotron 7.54e-05 / 8.96e-05 / 1.21e-03
  i <9>   broadband hifi 1.01e-06 / 1.17e-06, tacotron 1.32e-06 / 9.62e-07;  tonal hifi 1.44e-05 / 7.53e-05 / 2.30e-04, tacotron 3.85e-05 / 5.10e-05 / 6.17e-04
  energy, relative: fp32 oracle 1.6e-07 .. 2.5e-06, kernel 4.9e-08 .. 4.4e-07 over all of the above (bar 1e-4)
  shortest signals (1 .. 17 frames): kernel 3.3e-07 .. 6.8e-06;  y * 1e-4 at (c), (e): 2.0e-06 .. 2.2e-06;  y * 2, y * 8 at (e): 7.1e-07, 5.6e-07
  33 / 64 / 128 taps (n_fft 1056 hop 32, n_fft 1024 hop 16 and 8): hifi 9.11e-07 / 1.27e-06 / 1.39e-06, tacotron 1.04e-06 / 1.15e-06 / 1.44e-06: they run
  stft_frames: every word equal in all eight cases, the 4412 subnormal-or-zero low parts included: the device does not flush them
  mel_from_spec: log-mel at most 0.51 of its derived bar (1.95e-06 at 1..13 entries per filter), energy at most 8.5e-08 relative
  Features.frame_level at (c): 76 frames, log-mel 9.49e-07, energy 9.21e-08 relative
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import audio as OA
from tests import mel_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIDS = sorted(mel_ref.CONFIGS)
SCALE = 4096.0
SCALES = {"x2": 2.0, "x8": 8.0, "quiet": 1e-4}


# ------------------------------------------------------------------------------------------------ references, computed once

def shortest(cfg, surface):
    """The shortest signal a surface takes: reflect padding needs pad < len (torch's F.pad refuses the same), and one frame."""
    n_fft, hop = cfg[:2]
    return max(hop, (n_fft - hop) // 2 + 1) if surface == "hifi" else n_fft // 2 + 1


@functools.lru_cache(maxsize=None)
def signal(cfg, kind, surface):
    n_fft, hop = cfg[:2]
    n, seed = mel_ref.signal_length(n_fft, hop), n_fft + hop
    if kind == "tonal":
        return mel_ref.tonal(n, cfg[4], seed)
    if kind == "short":
        n = shortest(cfg, surface)
    y = mel_ref.broadband(2, n, seed)
    return y * np.float32(SCALES[kind]) if kind in SCALES else y


@functools.lru_cache(maxsize=None)
def reference(cfg, kind, surface):
    """(y, fp64 log-mel, fp64 energy or None, fp32 oracle's log-mel deviation, its relative energy deviation or None)."""
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    y = signal(cfg, kind, surface)
    yt = torch.from_numpy(y)
    if surface == "hifi":
        ref = mel_ref.hifi(y, *cfg)
        o = OA.mel_spectrogram(yt, n_fft, n_mels, sr, hop, win, fmin, fmax).numpy()
        return y, ref, None, float(np.abs(o - ref).max()), None
    ref, en = mel_ref.tacotron(y, *cfg)
    o, oe = (v.numpy() for v in OA.tacotron_mel(yt, n_fft, hop, win, n_mels, sr, fmin, fmax))
    return y, ref, en, float(np.abs(o - ref).max()), float(np.abs(oe / en - 1).max())


@functools.lru_cache(maxsize=None)
def tacotron_stft(cfg):
    from tts_king_amd.audio import TacotronSTFT
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    return TacotronSTFT(n_fft, hop, win, n_mels, sr, fmin, fmax, device=DEV)


def run(cfg, y, surface):
    from tts_king_amd.audio import mel_spectrogram
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    yd = torch.from_numpy(y).to(DEV)
    if surface == "hifi":
        mel, en = mel_spectrogram(yd, n_fft, n_mels, sr, hop, win, fmin, fmax), None
    else:
        mel, en = tacotron_stft(cfg).mel_spectrogram(yd)
    torch.cuda.synchronize()
    assert mel.dtype == torch.float32
    return mel.cpu().numpy().astype(np.float64), None if en is None else en.cpu().numpy().astype(np.float64)


def compare(name, cfg, kind, surface, bar_of=lambda e32: 1e-4):
    """One surface on one input against fp64: shapes, log-mel under bar_of(fp32 oracle's deviation), energy rtol 1e-4 / atol 1e-5."""
    n_fft, hop, win, n_mels = cfg[:4]
    y, ref, ref_en, e32, e32_en = reference(cfg, kind, surface)
    got, got_en = run(cfg, y, surface)
    T = y.shape[1] // hop + (surface == "tacotron")
    assert ref.shape == (y.shape[0], n_mels, T)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    d, bar = float(np.abs(got - ref).max()), bar_of(e32)
    line = "%s %s %s: %d frames, log-mel fp32 oracle %.2e, kernel %.2e, bar %.2e" % (name, kind, surface, T, e32, d, bar)
    if ref_en is not None:
        assert got_en.shape == ref_en.shape == (y.shape[0], T)
        line += "; energy rel fp32 oracle %.2e, kernel %.2e" % (e32_en, float(np.abs(got_en / ref_en - 1).max()))
    print(line)
    assert d < bar, line
    if ref_en is not None:
        assert np.allclose(got_en, ref_en, rtol=1e-4, atol=1e-5), line
    return d


# ------------------------------------------------------------------------------------------------ (A), (B): both surfaces

@pytest.mark.parametrize("cid", CIDS)
def test_broadband_both_surfaces(cid):
    cfg = mel_ref.CONFIGS[cid]
    compare(cid, cfg, "broadband", "hifi")
    compare(cid, cfg, "broadband", "tacotron")


@pytest.mark.parametrize("cid", CIDS)
def test_shortest_signal_both_surfaces(cid):
    """The reflect padding nearly meets the signal's length: len = pad + 1 (and at least one hop) on the vocoder surface, which is one
    frame where n_fft < 4 hop + 2; len = n_fft//2 + 1 on the Tacotron surface.  One sample less is refused, not padded wrongly."""
    from tts_king_amd.audio import mel_spectrogram
    cfg = mel_ref.CONFIGS[cid]
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    compare(cid, cfg, "short", "hifi")
    compare(cid, cfg, "short", "tacotron")
    pad = (n_fft - hop) // 2
    if pad >= hop:          # a signal of one hop would give one frame, but cannot be reflect-padded
        with pytest.raises(ValueError, match="reflect"):
            mel_spectrogram(torch.zeros(1, pad, device=DEV), n_fft, n_mels, sr, hop, win, fmin, fmax)
    with pytest.raises(ValueError, match="reflect"):
        tacotron_stft(cfg).mel_spectrogram(torch.zeros(1, n_fft // 2, device=DEV))


@pytest.mark.parametrize("cid", CIDS)
def test_tonal_both_surfaces(cid):
    cfg = mel_ref.CONFIGS[cid]

    def bar_of(e32):
        bar = max(1e-4, 16.0 * e32)
        assert bar <= 5e-3, "the fp32 oracle itself is %.2e off fp64 on this input: the bar would hide a failure" % e32
        return bar
    compare(cid, cfg, "tonal", "hifi", bar_of)
    compare(cid, cfg, "tonal", "tacotron", bar_of)


@pytest.mark.parametrize("cid", ["c", "e"])
def test_quiet_signal(cid):
    """y * 1e-4: the scaled signal's fp16 low parts are subnormal throughout; bar (A) still holds."""
    cfg = mel_ref.CONFIGS[cid]
    compare(cid, cfg, "quiet", "hifi")
    compare(cid, cfg, "quiet", "tacotron")


# ------------------------------------------------------------------------------------------------ (C): ttsk_stft_frames

def stft_input(Bsz, n, seed):
    """+-1, 0, uniform noise and a stretch of |x| in [1e-8, 1e-5] (times 4096: fp16 subnormal low parts, and subnormal high parts too),
    with the special values at both ends, where the reflection reads them."""
    r = np.random.RandomState(seed)
    x = (r.rand(Bsz, n) * 2 - 1).astype(np.float32)
    if n >= 64:
        x[:, :3] = (1.0, -1.0, 0.0)
        x[:, -3:] = (0.0, 1.0, -1.0)
        k, m = n // 3, min(40, n // 4)
        x[:, k:k + m] = (np.where(r.rand(Bsz, m) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(-8, -5, (Bsz, m))).astype(np.float32)
        x[:, 3:3 + m // 4] = x[:, k:k + m // 4]
    else:
        x[:] = np.resize(np.asarray([1.0, -3e-7, 0.0, -1.0, 2e-8, 0.37], np.float32), n)[None, :]
    return x


STFT_CASES = [    # (len, pad, hop, rows, B)
    (1000, 0, 16, 63, 2),        # no padding; rows*hop 1008 > 1000
    (301, 300, 24, 38, 1),       # pad = len - 1, the largest allowed; 912 > 901
    (2, 1, 8, 1, 1),             # the smallest signal
    (77, 20, 8, 15, 2),          # hop 8
    (1000, 140, 32, 40, 1),      # rows*hop == len + 2 pad
    (1000, 140, 32, 39, 3),      # 32 padded samples unused; B = 3
    (1000, 140, 32, 45, 2),      # 160 zeros written
    (4099, 512, 256, 24, 3),     # more than one workgroup's worth of one row; 6144 > 5123
]


@pytest.mark.parametrize("n,pad,hop,rows,Bsz", STFT_CASES)
def test_stft_frames_bit_for_bit(n, pad, hop, rows, Bsz):
    """Reflection, zero fill, the [hi | hi | lo] layout and both roundings, every fp16 word.  Subnormal low parts are kept, not flushed
    (measured: no word differs), so the low-part comparison is exact too."""
    from tts_king_amd import ops
    x = stft_input(Bsz, n, seed=n + pad)
    want = mel_ref.stft_rows(x, pad, rows, hop, SCALE).view(np.uint16)
    got = ops.stft_frames(torch.from_numpy(x).to(DEV), pad, rows, hop, SCALE)
    torch.cuda.synchronize()
    assert got.shape == (Bsz, rows, 3 * hop) and got.dtype == torch.float16
    got = got.cpu().numpy().view(np.uint16)
    hi_bad = int((got[:, :, :hop] != want[:, :, :hop]).sum())
    copy_bad = int((got[:, :, hop:2 * hop] != got[:, :, :hop]).sum())
    lo_ne = got[:, :, 2 * hop:] != want[:, :, 2 * hop:]
    sub = (want[:, :, 2 * hop:] & 0x7C00) == 0
    print("stft_frames len %d pad %d hop %d rows %d B %d: hi words differing %d, hi copies differing %d, lo words differing %d "
          "(%d of them where the expected lo is subnormal or zero; %d such words in all)"
          % (n, pad, hop, rows, Bsz, hi_bad, copy_bad, int(lo_ne.sum()), int((lo_ne & sub).sum()), int(sub.sum())))
    assert hi_bad == 0 and copy_bad == 0
    assert not lo_ne.any()


# ------------------------------------------------------------------------------------------------ (D): ttsk_mel_from_spec

def slaney_table(nbins, n_mels):
    return mel_ref.pack(OA.mel_filterbank(22050, 2 * (nbins - 1), n_mels, 0.0, None))


def hand_table(nbins, n_mels, total=None, seed=0):
    """A packed table no filterbank would give: filter 0 empty, filter 1 of one entry, filter 2 and the last one ending exactly at bin
    nbins - 1, and on the four-lane half (when present) filters of 1, 0 and 3 entries; `total` entries in all when given.  Every
    filter stays inside [0, nbins)."""
    r = np.random.RandomState(seed)
    counts = r.randint(1, min(nbins, 40) + 1, size=n_mels)
    fixed = {0: 0, 1: 1}
    if n_mels > 67:
        fixed.update({64: 1, 65: 0, 66: 3})
    for m, c in fixed.items():
        counts[m] = c
    if total is not None:
        free = [m for m in range(n_mels) if m not in fixed]
        rest = total - sum(fixed.values())
        counts[free] = rest // len(free)
        counts[free[:rest % len(free)]] += 1
    assert counts.max() <= nbins and n_mels > 3
    start = np.asarray([r.randint(0, nbins - c + 1) for c in counts])
    start[2], start[-1] = nbins - counts[2], nbins - counts[-1]
    off = np.concatenate([[0], np.cumsum(counts)])
    vals = r.uniform(1e-3, 5e-2, max(int(off[-1]), 1)).astype(np.float32)
    return vals, start.astype(np.int32), off.astype(np.int32)


MEL_CASES = [    # (nbins, n_mels, T, eps, B, table): every value of every axis, and the pairs (577, 65), (1088, 80), (576, 64), (5, 1)
    (5, 1, 1, 0.0, 1, "slaney"),
    (129, 63, 15, 1e-9, 3, "slaney"),
    (513, 79, 16, 0.0, 1, "slaney"),
    (576, 64, 17, 1e-9, 1, "slaney"),
    (577, 65, 33, 0.0, 3, "slaney"),
    (1025, 80, 17, 1e-9, 1, "slaney"),
    (1088, 80, 33, 0.0, 1, "slaney"),
    (1088, 80, 16, 1e-9, 1, "hand6144"),
    (576, 80, 15, 0.0, 3, "hand"),
    (577, 65, 1, 1e-9, 1, "hand"),
    (129, 79, 33, 0.0, 1, "hand6144"),
]


@pytest.mark.parametrize("nbins,n_mels,T,eps,Bsz,table", MEL_CASES)
def test_mel_from_spec_against_fp64(nbins, n_mels, T, eps, Bsz, table):
    from tts_king_amd import ops
    if table == "slaney":
        vals, start, off = slaney_table(nbins, n_mels)
    else:
        vals, start, off = hand_table(nbins, n_mels, 6144 if table == "hand6144" else None, seed=nbins + n_mels)
    nnz = int(off[-1])
    assert nnz <= 6144 and (table != "hand6144" or nnz == 6144)
    assert all(start[m] + off[m + 1] - off[m] <= nbins for m in range(n_mels))        # the kernel trusts its tables
    rows, ld = T + 3, (2 * nbins + 7) // 8 * 8 + 8
    r = np.random.RandomState(nbins * 100 + n_mels)
    spec = (r.randn(Bsz, rows, ld) * 10.0 ** r.uniform(-3, 1, (Bsz, rows, 1))).astype(np.float32)
    spec[:, :, 2 * nbins:] = np.nan                 # the padding columns of the extractor's `cout` are never read
    ref, ref_en, n_m = mel_ref.mel_from_spec(spec, T, nbins, vals, start, off, eps)
    dev = [torch.from_numpy(a).to(DEV) for a in (vals, start, off)]

    def launch(s):
        mel, en = ops.mel_from_spec(torch.from_numpy(s.reshape(Bsz * rows, ld)).to(DEV), Bsz, rows, T, nbins, *dev, nnz, n_mels, eps)
        torch.cuda.synchronize()
        assert mel.shape == (Bsz, n_mels, T) and en.shape == (Bsz, T)
        return mel.cpu().numpy(), en.cpu().numpy()
    mel, en = launch(spec)
    poisoned = spec.copy()
    poisoned[:, T:] = np.nan                        # rows from T on belong to no frame
    mel2, en2 = launch(poisoned)
    bar = (n_m[None, :, None] + 8) * 2.0 ** -23 + 4 * 2.0 ** -24 * np.abs(ref)
    d = np.abs(mel.astype(np.float64) - ref)
    de = np.abs(en.astype(np.float64) / ref_en - 1)
    print("mel_from_spec nbins %d n_mels %d T %d eps %g B %d %s (%d entries, %d..%d per filter): log-mel worst %.2e at %.2f of its bar, "
          "energy rel %.2e, bar %.2e" % (nbins, n_mels, T, eps, Bsz, table, nnz, n_m.min(), n_m.max(), d.max(), (d / bar).max(),
                                         de.max(), (nbins + 8) * 2.0 ** -24))
    assert np.isfinite(mel).all() and np.isfinite(en).all()
    assert (d <= bar).all()
    assert (de <= (nbins + 8) * 2.0 ** -24).all()
    empty = np.nonzero(n_m == 0)[0]
    assert (np.abs(mel[:, empty] - np.log(1e-5)) <= 4 * 2.0 ** -24 * 11.52).all()        # an empty filter sits on the clamp
    assert np.array_equal(mel.view(np.uint32), mel2.view(np.uint32)) and np.array_equal(en.view(np.uint32), en2.view(np.uint32))


# ------------------------------------------------------------------------------------------------ (E): accepted and refused

TAP_PROBES = [(1056, 32, 1056, 80, 22050, 0, 8000), (1024, 16, 1024, 80, 22050, 0, 8000), (1024, 8, 1024, 80, 22050, 0, 8000)]


@pytest.mark.parametrize("cfg", TAP_PROBES, ids=["33taps", "64taps", "128taps"])
def test_more_than_32_taps_runs(cfg):
    """Every configuration the constructor accepts runs: n_fft / hop of 33, 64 and 128 (the last at hop = 8, K = 24, less than one K
    tile).  ttsk_gemm's planner gives these to its register-staged kernels, which test tap validity on the fly past 32 taps."""
    name = "%d taps" % (cfg[0] // cfg[1])
    compare(name, cfg, "broadband", "hifi")
    compare(name, cfg, "broadband", "tacotron")


@pytest.mark.parametrize("kind", ["x2", "x8"])
def test_vocoder_surface_amplitudes_above_one(kind):
    compare("e", mel_ref.CONFIGS["e"], kind, "hifi")


def test_vocoder_surface_refuses_what_overflows_fp16():
    """The signal is scaled by 4096 before it is rounded to fp16: from |y| = 65520 / 4096 (just under 16) on that is inf."""
    from tts_king_amd.audio import mel_spectrogram
    n_fft, hop, win, n_mels, sr, fmin, fmax = mel_ref.CONFIGS["e"]
    y = signal(mel_ref.CONFIGS["e"], "broadband", "hifi").copy()
    ok = y.copy()
    ok[0, 100] = -15.99
    out = mel_spectrogram(torch.from_numpy(ok).to(DEV), n_fft, n_mels, sr, hop, win, fmin, fmax)
    assert torch.isfinite(out).all()
    for bad in (16.0, -16.0, 15.997, 1e6, float("inf"), float("nan")):
        y[1, -7] = bad
        with pytest.raises(ValueError, match="16"):
            mel_spectrogram(torch.from_numpy(y).to(DEV), n_fft, n_mels, sr, hop, win, fmin, fmax)


def test_constructor_refusals_name_the_limit():
    from tts_king_amd.audio import MelExtractor
    for args in ((1024, 80, 22050, 300, 1024, 0, 8000),       # n_fft % hop
                 (1020, 80, 22050, 204, 1020, 0, 8000),       # hop % 8
                 (1024, 80, 22050, 256, 1025, 0, 8000),       # win > n_fft
                 (1024, 81, 22050, 256, 1024, 0, 8000),       # num_mels > 80
                 (1024, 0, 22050, 256, 1024, 0, 8000),        # no filters
                 (1024, 80, 22050, 0, 1024, 0, 8000),         # no hop
                 (1024, 80, 22050, 256, 0, 0, 8000),          # no window
                 (2304, 80, 22050, 256, 2304, 0, 8000)):      # n_fft > 2048
        with pytest.raises(ValueError, match="n_fft % hop_size == 0, hop_size % 8 == 0, win_size <= n_fft <= 2048, num_mels <= 80"):
            MelExtractor(*args, pad=0, eps=0.0, device=DEV)


def test_stft_frames_argument_refusals():
    from tts_king_amd import lib, ops
    L = lib.load()
    wav = torch.zeros(2, 100, device=DEV)
    for n, pad, rows, hop in ((100, 10, 4, 12), (100, 10, 4, 0), (100, 100, 4, 16), (100, 250, 4, 16), (100, -1, 4, 16), (1, 0, 4, 16)):
        out = torch.full((2, rows, 3 * max(hop, 8)), 7.0, dtype=torch.float16, device=DEV)
        with pytest.raises(lib.TtskError, match="ttsk_stft_frames"):
            lib.check(L.ttsk_stft_frames(ops._ptr(wav), ops._ptr(out), 2, n, pad, rows, hop, SCALE, ops._stream()), "ttsk_stft_frames")
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), (n, pad, rows, hop)
    with pytest.raises(lib.TtskError, match="pad < len"):
        ops.stft_frames(wav, 100, 4, 16, SCALE)


def test_mel_from_spec_argument_refusals():
    from tts_king_amd import lib, ops
    L = lib.load()
    good = dict(ld=2184, nnz=6144, Bsz=2, rows=20, T=17, nbins=1088, n_mels=80)
    spec = torch.zeros(2 * 20, 2184, device=DEV)
    vals, start, off = torch.zeros(6145, device=DEV), torch.zeros(81, dtype=torch.int32, device=DEV), torch.zeros(82, dtype=torch.int32, device=DEV)
    for change in (dict(nbins=1089, ld=2184), dict(n_mels=81), dict(nnz=6145), dict(ld=2175), dict(rows=16), dict(T=0), dict(nbins=0), dict(nnz=-1)):
        a = dict(good, **change)
        mel = torch.full((2, 81, 17), 7.0, device=DEV)
        en = torch.full((2, 17), 7.0, device=DEV)
        with pytest.raises(lib.TtskError, match="ttsk_mel_from_spec"):
            lib.check(L.ttsk_mel_from_spec(ops._ptr(spec), a["ld"], ops._ptr(vals), ops._ptr(start), ops._ptr(off), a["nnz"], ops._ptr(mel),
                                           ops._ptr(en), a["Bsz"], a["rows"], a["T"], a["nbins"], a["n_mels"], 0.0, 1e-5, ops._stream()),
                      "ttsk_mel_from_spec")
        torch.cuda.synchronize()
        assert bool((mel == 7.0).all()) and bool((en == 7.0).all()), change


# ------------------------------------------------------------------------------------------------ (F): preprocess.Features

def test_features_frame_level_at_configuration_c():
    from tts_king_amd import preprocess
    from tts_king_amd.config import default_config
    cfg = mel_ref.CONFIGS["c"]
    n_fft, hop, win, n_mels, sr, fmin, fmax = cfg
    config = copy.deepcopy(default_config().preprocess_config)
    pp = config["preprocessing"]
    pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"] = n_fft, hop, win
    pp["mel"]["n_mel_channels"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"] = n_mels, fmin, fmax
    pp["audio"]["sampling_rate"] = sr
    n = int(0.6 * sr)
    wav = mel_ref.broadband(1, n, seed=5)[0]
    mel, energy, f0 = preprocess.Features(config, device=DEV).frame_level(wav)
    torch.cuda.synchronize()
    T = 1 + n // hop
    assert mel.shape == (1, n_mels, T) and energy.shape == (1, T) and f0.shape == (1, T)
    ref, ref_en = mel_ref.tacotron(wav[None], *cfg)
    d = float(np.abs(mel.cpu().numpy() - ref).max())
    de = float(np.abs(energy.cpu().numpy() / ref_en - 1).max())
    print("Features.frame_level at (c): %d frames, log-mel %.2e (bar 1e-4), energy rel %.2e" % (T, d, de))
    assert d < 1e-4
    assert np.allclose(energy.cpu().numpy(), ref_en, rtol=1e-4, atol=1e-5)
    assert torch.isfinite(f0).all()
