"""GPU: the sample-rate converter (csrc/resample.hip, tts_king_amd/resample.py) -- the kernel bit for bit on integer operands, against
the fp64 reference (tests/resample_ref.py) within the forward bound of an fp32 sum, its fused int16, its independence of where a
segment lies, and the routes that carry `sample_rate=` (generator, graphs, facades).

Bars.  Integer tables and inputs with |values| <= 8: every product and partial sum is an integer below 2^24, so fp32 is exact in any
order and the comparison is `torch.equal` against int64 numpy.  Designed filters: |y - y_fp64| <= (P + 2) 2^-24 sum_j |x_j| |g(m M - j L)|
per sample -- one rounding of every coefficient to fp32 (2^-24 relative) plus P fused multiply-adds in any order ((P + 1) 2^-24 to
first order on the sum of magnitudes); derived, not tuned.  Everything else is compared bit for bit against the kernel itself."""
import copy

import numpy as np
import pytest
import torch

from tests import resample_ref as ref
from tests.test_hifigan_gpu import build
from tests.test_windows_gpu import _api, _mels
from tts_king_amd import resample, windows
from tts_king_amd.synthetic import make_mel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = 22050
W = windows.W


def _filter(T, L, M, C):
    """Any (L, P) table as the kernel reads it: tap-major."""
    return resample.Filter(L, M, T.shape[1], C, torch.from_numpy(np.ascontiguousarray(T.T, dtype=np.float32)).to(DEV))


def _table_form_int(x, T, L, M, C, n_out):
    """tests/resample_ref.table_form in int64, a block of outputs at a time."""
    P, n, out = T.shape[1], len(x), np.empty(n_out, dtype=np.int64)
    q = np.arange(P, dtype=np.int64)[None, :]
    for a in range(0, n_out, 256):
        u = np.arange(a, min(a + 256, n_out), dtype=np.int64) * M
        j = (u // L)[:, None] + C - q
        xv = np.where((j >= 0) & (j < n), x[np.clip(j, 0, n - 1)], 0)
        out[a:a + len(u)] = (T[u % L] * xv).sum(axis=1)
    return out


def _lay_out(lens, L, M, src_gap, dst_gaps):
    """Segments of `lens` samples with `src_gap` samples between and around them in the source and dst_gaps[i] samples before
    segment i in the destination: (table int32 (rows, 4), samples of the source, samples of the destination)."""
    rows, so, do = [], src_gap, 0
    for i, n in enumerate(lens):
        do += dst_gaps[i % len(dst_gaps)]
        m = resample.out_len(n, L, M)
        rows.append((so, n, do, m))
        so += n + src_gap
        do += m
    return np.asarray(rows, dtype=np.int32), so, do + 9


# the issue's six, then two that leave the staged path's single-chunk case: taps that need several staged chunks per tile, and more
# taps than the staging holds (every tap then reads the source with its own bounds check)
INT_CASES = [(1, 1, 5, 2), (2, 1, 7, 3), (1, 2, 9, 4), (3, 2, 8, 3), (160, 441, 177, 88), (640, 441, 45, 22), (1, 8, 5000, 2500),
             (1, 1, 8200, 4100)]


@pytest.mark.parametrize("L,M,P,C", INT_CASES)
@pytest.mark.parametrize("to_i16", [False, True])
def test_bit_exact_on_integer_operands(L, M, P, C, to_i16):
    from tts_king_amd import ops
    rng = np.random.default_rng(1000 * L + M)
    T = rng.integers(-8, 9, size=(L, P)).astype(np.int64)
    filt = _filter(T, L, M, C)
    tile = ops.resample_tile(filt)                                # samples of dst per workgroup for this filter
    assert 256 <= tile <= 4096
    edge = tile * M // L
    lens = [1, 2, max(C, 1), C + 1, P, edge - 1, edge, edge + 1, (3 * tile + 5) * M // L]
    table, n_src, n_dst = _lay_out(lens, L, M, src_gap=3, dst_gaps=(0, 0, 5, 1, 0, 1019, 0, 2, 0))
    src = np.full(n_src, 1000, dtype=np.int64)                    # what lies between and around the segments is never signal
    want = np.full(n_dst, -777, dtype=np.int64)                   # ... and what lies between the outputs is never written
    for so, n, do, m in table:
        src[so:so + n] = rng.integers(-8, 9, size=n)
        y = _table_form_int(src[so:so + n], T, L, M, C, m)
        # int16 at scale 0.5: (int)clamp(y / 2), toward zero; the long filters' sums pass 2^16 and saturate
        want[do:do + m] = np.clip(np.trunc(y / 2.0), -32768, 32767).astype(np.int64) if to_i16 else y
    # two padding rows and one row that does not fit the source: skipped
    table = np.concatenate([table, np.zeros((2, 4), np.int32), np.asarray([[n_src - 2, 3, 0, 3]], np.int32)])
    dt = torch.int16 if to_i16 else torch.float32
    out = torch.full((n_dst,), -777, dtype=dt, device=DEV)
    got = ops.resample(torch.from_numpy(src.astype(np.float32)).to(DEV), torch.from_numpy(table).to(DEV), filt, out=out,
                       int16_scale=0.5 if to_i16 else None)
    assert got is out
    assert torch.equal(got.cpu(), torch.from_numpy(want).to(dt))


@pytest.fixture(scope="module")
def noise():
    g = torch.Generator().manual_seed(20)
    return [torch.randn(n, generator=g) for n in (2000, 37, 1)]


@pytest.mark.parametrize("rate", [8000, 16000, 44100, 48000])
def test_designed_filters_within_the_fp32_bound(rate, noise):
    from tts_king_amd import ops
    filt = resample.filter_for(IN, rate, DEV)
    L, M, P = filt.L, filt.M, filt.P
    assert (L, M, P, filt.C) == resample.design(IN, rate)[:4]
    sg = resample.segments(np.cumsum([0] + [len(x) for x in noise[:-1]]), [len(x) for x in noise], L, M)
    got = ops.resample(torch.cat(noise).to(DEV), torch.from_numpy(sg.table).to(DEV), filt).cpu().double().numpy()
    assert got.shape == (sg.n_dst,)
    for x, (o, m) in zip(noise, sg.spans):
        xd = x.double().numpy()
        y, bound = ref.resample(xd, L, M), (P + 2) * 2.0 ** -24 * ref.weight(xd, L, M)
        err = np.abs(got[o:o + m] - y)
        print("rate %d, %d samples: worst error / bound %.3f" % (rate, len(xd), (err / bound).max()))
        assert m == len(y) == -(-len(xd) * L // M) and np.all(err <= bound)


def test_fused_int16_saturates(noise):
    from tts_king_amd import ops
    filt = resample.filter_for(IN, 48000, DEV)
    n = 3000
    square = 0.999 * (1.0 - 2.0 * ((torch.arange(n) // 150) % 2).float())         # near full scale: the filter overshoots its edges
    x = torch.cat([square, 0.6 * noise[0]]).to(DEV)
    sg = resample.segments([0, n], [n, len(noise[0])], filt.L, filt.M)
    segs = torch.from_numpy(sg.table).to(DEV)
    y = ops.resample(x, segs, filt).cpu()
    y16 = ops.resample(x, segs, filt, int16_scale=32768.0).cpu()
    assert y16.dtype == torch.int16 and y16.shape == y.shape
    want = (y * 32768.0).clamp(-32768.0, 32767.0).trunc().to(torch.int16)         # clamp, then toward zero
    assert torch.equal(y16, want)
    o, m = sg.spans[0]
    over = (y[o:o + m].abs() * 32768.0 > 32768.0)
    assert int(over.sum()) > 10                                                   # the case is live: these would wrap without the clamp
    assert bool((y16[o:o + m][over].float() * y[o:o + m][over] > 0).all())        # no sample of the wrong sign
    assert set(y16[o:o + m][over].tolist()) <= {-32768, 32767}
    wrapped = (y[o:o + m][over] * 32768.0).to(torch.int32).to(torch.int16)        # the low 16 bits: what ttsk_to_int16 would give
    assert bool((wrapped.float() * y[o:o + m][over] < 0).any())


@pytest.mark.parametrize("rate", [8000, 48000])
def test_position_independence(rate):
    from tts_king_amd import ops
    filt = resample.filter_for(IN, rate, DEV)
    g = torch.Generator().manual_seed(rate)
    xs = [torch.randn(n, generator=g) for n in (2 * ops.resample_tile(filt) * filt.M // filt.L + 77, 5, 1500)]
    sg = resample.segments(np.cumsum([0] + [len(x) for x in xs[:-1]]), [len(x) for x in xs], filt.L, filt.M)
    together = ops.resample(torch.cat(xs).to(DEV), torch.from_numpy(sg.table).to(DEV), filt)
    for x, (o, m) in zip(xs, sg.spans):
        one = resample.segments([0], [len(x)], filt.L, filt.M)
        alone = ops.resample(x.to(DEV), torch.from_numpy(one.table).to(DEV), filt)
        assert alone.shape == (m,) and torch.equal(alone, together[o:o + m])


@pytest.fixture(scope="module")
def gen_and_native(cfg):
    gen = build(cfg, 3)
    mels = [m.to(DEV) for m in _mels([130, 96, 20], seed=2)]
    return gen, mels, [y.clone() for y in gen.forward_ragged(mels)]


@pytest.mark.parametrize("rate", [16000, 48000])
def test_through_the_generator(gen_and_native, rate):
    from tts_king_amd import ops
    gen, mels, native = gen_and_native
    filt = gen.resampler(rate)
    got = gen.forward_ragged(mels, sample_rate=rate)
    for y, base, T in zip(got, native, (130, 96, 20)):
        m = -(-256 * T * filt.L // filt.M)
        one = torch.from_numpy(resample.segments([0], [256 * T], filt.L, filt.M).table).to(DEV)
        assert y.shape == (1, 1, m) and y.dtype == torch.float32
        assert torch.equal(y.reshape(-1), ops.resample(base.reshape(-1).contiguous(), one, filt))


def test_native_rate_is_the_route_as_it_was(gen_and_native):
    from tts_king_amd import ops
    gen, mels, native = gen_and_native
    assert gen.resampler(None) is None and gen.resampler(IN) is None
    ops.LAUNCH_COUNTS = counts = {}
    try:
        for rate in (None, IN):
            got = gen.forward_ragged(mels, sample_rate=rate)
            assert all(torch.equal(a, b) for a, b in zip(got, native))
        assert "resample" not in counts
        gen.forward_ragged(mels, sample_rate=16000)
        assert counts["resample"] == 1                                            # one launch for the whole call
    finally:
        ops.LAUNCH_COUNTS = None
    with pytest.raises(ValueError, match="at most 1024"):
        gen.forward_ragged(mels, sample_rate=22051)
    with pytest.raises(ValueError, match="positive integer"):
        gen.forward_ragged(mels, sample_rate=16000.0)


def test_short_utterances_on_the_solo_route_are_resampled_alone(gen_and_native):
    """A generator whose kernels take no row length sends short utterances through `forward_short`: one-row tables."""
    gen, mels, native = gen_and_native
    plan = windows.plan_windows([130, 96, 20], W, gen.halo(), short_rows=False)
    assert plan.short == [2]
    got = gen.forward_short(mels, plan, sample_rate=16000)
    assert list(got) == [2]
    want = gen.resample_rows(gen(mels[2][None]), 16000)
    assert torch.equal(got[2], want) and got[2].shape == (1, 1, -(-256 * 20 * 320 // 441))


def test_one_graph_per_window_count_and_rate(cfg):
    api = _api(cfg, True)
    syn = api._synth
    calls = [[300, 200, 2 * W], [W + 5, 310, 250], [333, W, 3 * W - 60]]
    assert len({windows.plan_windows(c, W, 14).N for c in calls}) == 1
    outs = []
    for k, lens in enumerate(calls):
        mels = [m.to(DEV) for m in _mels(lens, seed=k)]
        outs.append((mels, lens, [y.clone() for y in syn.wav_ragged(mels, sample_rate=16000)]))
        assert len(syn._rag) == (0 if k == 0 else 1)                              # first sight eager, second captured, third replayed
    torch.cuda.synchronize()
    for mels, lens, got in outs:                                                  # two replays of different lengths on one graph = the eager calls
        want = api.model.forward_ragged(mels, sample_rate=16000)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert [tuple(y.shape) for y in got] == [(1, 1, -(-256 * T * 320 // 441)) for T in lens]
    mels = outs[0][0]
    for _ in range(2):
        syn.wav_ragged(mels, sample_rate=8000)
    assert len(syn._rag) == 2                                                     # another rate at the same N: one more graph
    for _ in range(2):
        y = syn.wav_ragged(mels)
    assert len(syn._rag) == 3 and all(torch.equal(a, b) for a, b in zip(y, api.model.forward_ragged(mels)))
    for _ in range(2):
        y = syn.wav_ragged(mels, sample_rate=IN)                                  # the native rate is the native graph
    assert len(syn._rag) == 3 and all(torch.equal(a, b) for a, b in zip(y, api.model.forward_ragged(mels)))


@pytest.mark.parametrize("graph", [False, True])
def test_facades(cfg, graph):
    api = _api(cfg, graph)
    mel = make_mel(2, 32, seed=8)
    m8 = -(-8192 * 160 // 441)
    floats = api.model.resample_rows(api.model(mel.to(DEV)), 8000)
    want = (floats * 32768.0).clamp(-32768.0, 32767.0).trunc().to(torch.int16).cpu().numpy()
    for rep in range(3):                                                          # eager, captured, replayed when `graph`
        a = api.generate(mel, sample_rate=8000)
        assert isinstance(a, np.ndarray) and a.dtype == np.int16 and a.shape == (2, 1, m8) and np.array_equal(a, want)
    assert torch.equal(api(mel, sample_rate=8000), floats)
    native = api.generate(mel)
    assert native.shape == (2, 1, 8192) and np.array_equal(native, api.generate(mel, sample_rate=IN))
    lens = [W + 40, 60, 400]
    mels = _mels(lens, seed=5)
    for rep in range(3):
        got = api.generate_ragged(mels, sample_rate=16000)
        floats = api.model.forward_ragged([m.to(DEV) for m in mels], sample_rate=16000)
        for g, f, T in zip(got, floats, lens):
            assert g.dtype == np.int16 and g.shape == (1, 1, -(-256 * T * 320 // 441))
            assert np.array_equal(g, (f * 32768.0).clamp(-32768.0, 32767.0).trunc().to(torch.int16).cpu().numpy())
    dev = api.call_ragged([m.to(DEV) for m in mels], sample_rate=16000)
    assert all(torch.equal(a, b) for a, b in zip(dev, floats))


def test_configured_default_rate_and_ttsking(cfg):
    from hifiapi import HIFIapi
    from tts_king import TTSKing
    c = copy.deepcopy(cfg)
    c.model_config["vocoder"]["use_cpu"] = False
    c.mi355x["hip_graph"] = False
    c.mi355x["output_sample_rate"] = 16000
    api = HIFIapi(c, "cuda:0")
    mel = make_mel(1, 40, seed=1)
    a = api.generate(mel)
    assert a.shape == (1, 1, -(-256 * 40 * 320 // 441)) and np.array_equal(a, api.generate(mel, sample_rate=16000))
    assert api.generate(mel, sample_rate=IN).shape == (1, 1, 256 * 40)            # an explicit rate wins over the default
    k = TTSKing.__new__(TTSKing)                                                  # the vocoder half only: no FastSpeech2 is built
    k.cfg, k.vocoder = cfg, _api(cfg, False)
    one = mel.transpose(1, 2).contiguous()                                        # (1, T, 80), FastSpeech2's layout
    assert np.array_equal(k.mel_to_wav(one, sample_rate=16000), a)
    got = k.mel_to_wav([one, one], sample_rate=48000)
    assert [g.shape for g in got] == [(1, 1, -(-256 * 40 * 320 // 147))] * 2 and all(g.dtype == np.int16 for g in got)
    c.mi355x["output_sample_rate"] = 22051
    with pytest.raises(ValueError, match="at most 1024"):
        HIFIapi(c, "cuda:0")
