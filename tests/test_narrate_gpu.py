"""GPU: paragraphs end to end (`TTSKing.narrate`, the vocoders' `generate_joined` / `call_joined`, `GraphedSynthesizer.wav_joined`;
DESIGN.md section 22) on the seeded random-init models the facade tests build.

With every step of the join switched off the output must be the bytes of `mel_to_wav(generate_mel([...]))` with zeros between: the
join multiplies by 1.0 (exact) and converts by the resampler's rule, which in range is the stitch's.  With the defaults it must be the
numpy restatement (tests/join_ref.py) applied to the solo float waveforms, under the terms of tests/test_join_gpu.py: decisions equal,
the gain within join_ref.gain_bound, the samples bit for bit under the device's gain."""
import numpy as np
import pytest
import torch

from tests import join_ref as ref
from tests.test_batch_synth_gpu import four_texts, make_tts
from tts_king_amd import narrate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    return make_tts(tmp_path_factory.mktemp("narrate_eager"), False)


@pytest.fixture(scope="module")
def tts_graphed(tmp_path_factory):
    return make_tts(tmp_path_factory.mktemp("narrate_graphed"), True)


def _three():
    return four_texts()[:3]                   # 48, 31 and 17 phonemes: the last one is shorter than a vocoder window


def _texts(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, 207, (L,), generator=g).numpy() for L in lens]


def _with_zeros(wavs, pauses):
    parts, spans, pos = [], [], 0
    for w, p in zip(wavs, pauses):
        w = np.asarray(w).reshape(-1)
        parts += [w, np.zeros(p, w.dtype)]
        spans.append((pos, pos + w.size))
        pos += w.size + p
    return np.concatenate(parts).reshape(1, 1, -1), spans


DC = [4.0, 3.0, 1.0]          # duration controls: the first two sentences span several vocoder windows, the third stays shorter than one


def _plain(t, texts, pauses_ms, rate, **kw):
    """narrate with every step off against mel_to_wav of the same mels with zeros between."""
    got, timing = t.narrate(texts, duration_control=DC, trim_db=None, normalize=None, fade_ms=0, pauses=pauses_ms, return_timing=True, **kw)
    mels = t.generate_mel(texts, DC)
    frames = [int(m.shape[1]) for m in mels]
    print("frames %s" % frames)
    assert frames[0] >= 2 * 96 and frames[1] >= 96 and 0 < frames[2] < 96, frames
    solo = t.mel_to_wav(mels, **kw)
    want, spans = _with_zeros(solo, [narrate.ms_to_samples(p, rate) for p in pauses_ms])
    assert got.dtype == np.int16 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert timing == spans
    assert np.abs(got).max() > 0
    return got


@pytest.mark.parametrize("kw,rate", [({}, 22050), (dict(sample_rate=16000), 16000), (dict(vocoder="griffin_lim", griffin_iters=4), 22050),
                                     (dict(vocoder="griffin_lim", griffin_iters=4, sample_rate=16000), 16000)])
def test_plain_join_is_mel_to_wav_with_zeros_between(tts, kw, rate):
    _plain(tts, _three(), [100, 0, 50], rate, **kw)


def test_plain_join_on_a_generator_without_short_rows(tts):
    gen = tts.vocoder.model
    gen.fused = False
    try:
        assert not gen.short_rows()
        mels = tts.generate_mel(_three(), DC)
        assert gen.plan([m.shape[1] for m in mels]).short == [2], "the third sentence is meant to be shorter than a window"
        _plain(tts, _three(), [100, 0, 50], 22050)
        _plain(tts, _three(), [0, 7, 1], 16000, sample_rate=16000)
    finally:
        gen.fused = True


@pytest.mark.parametrize("normalize", ["rms", "peak"])
def test_defaults_against_the_restatement_on_the_solo_waveforms(tts, normalize):
    texts = _three()
    got, timing = tts.narrate(texts, duration_control=DC, normalize=normalize, return_timing=True)
    mels = tts.generate_mel(texts, DC)
    join = narrate.Join(narrate.settings(22050, normalize=normalize), narrate.pause_plan([""] * 3, 22050))
    wav, info = tts.vocoder.generate_joined(mels, join, frames_first=True)
    assert np.array_equal(got, wav) and timing == info.timing()
    solo = [w.reshape(-1).cpu().numpy() for w in tts.speak(texts, DC)]
    lens = [w.size for w in solo]
    table = join.table(np.cumsum([0] + lens[:-1]).tolist(), lens)
    flat = np.concatenate(solo)
    own = ref.join_ref(flat, table, narrate.out_bound(table), 32768.0)
    assert info.a.tolist() == own["a"].tolist() and info.b.tolist() == own["b"].tolist()
    assert info.o.tolist() == own["o"].tolist() and info.total == own["total"] == got.shape[-1]
    assert np.array_equal(np.ascontiguousarray(info.peak).view(np.int32), own["peak"].view(np.int32))
    for u in range(3):
        m = int(info.b[u] - info.a[u])
        rel = abs(float(info.g[u]) - float(own["g"][u])) / float(own["g"][u])
        print("sentence %d: kept [%d, %d) of %d, peak %.4g, g %.6g (restatement %.6g, rel %.2g, bound %.2g)"
              % (u, info.a[u], info.b[u], lens[u], info.peak[u], info.g[u], own["g"][u], rel, ref.gain_bound(max(m, 1))))
        assert m > 0 and rel <= ref.gain_bound(m)
    want = ref.join_ref(flat, table, narrate.out_bound(table), 32768.0, g_device=info.g)
    assert np.array_equal(got.reshape(-1), want["out"][:info.total])
    # the float route: the same join without the conversion
    fl, info_f = tts.vocoder.call_joined(mels, join, frames_first=True)
    want_f = ref.join_ref(flat, table, narrate.out_bound(table), None, g_device=info_f.g)
    assert fl.shape == (1, 1, info.total) and np.array_equal(fl.reshape(-1).cpu().numpy().view(np.int32), want_f["out"][:info.total].view(np.int32))


def _phoneme_names(n, seed):
    from tts_king_amd.text import symbols
    names = [s[1:] for s in symbols() if s.startswith("@")]
    rnd = np.random.RandomState(seed)
    return " ".join(names[i] for i in rnd.randint(0, len(names), size=n))


def test_one_string_equals_the_list_of_its_sentences(tts):
    a, b = "{%s}" % _phoneme_names(14, 1), "{%s}" % _phoneme_names(9, 2)
    one, t1 = tts.narrate("%s. %s" % (a, b), return_timing=True)
    two, t2 = tts.narrate([a, b], return_timing=True)
    assert np.array_equal(one, two) and t1 == t2 and len(t1) == 2
    # the mark decides the pause: a semicolon gives 250 ms where the full stop gave 400
    semi, t3 = tts.narrate("%s; %s" % (a, b), return_timing=True)
    assert t3[0] == t1[0] and t1[1][0] - t3[1][0] == narrate.ms_to_samples(400, 22050) - narrate.ms_to_samples(250, 22050)
    with pytest.raises(ValueError, match="no sentence"):
        tts.narrate(" . ; ")
    with pytest.raises(ValueError, match="no sentence"):
        tts.narrate([])


def test_two_groups_equal_their_concatenation(tts):
    texts = _texts([5 + (3 * i) % 9 for i in range(33)], seed=8)
    spk = [i % 7 for i in range(33)]
    got, timing = tts.narrate(texts, speaker=spk, pauses=30, return_timing=True)
    first, tf = tts.narrate(texts[:32], speaker=spk[:32], pauses=30, return_timing=True)
    last, tl = tts.narrate(texts[32:], speaker=spk[32:], pauses=30, return_timing=True)
    assert np.array_equal(got, np.concatenate([first, last], axis=2))
    assert timing == tf + [(s + first.shape[-1], e + first.shape[-1]) for s, e in tl] and len(timing) == 33


def test_graph_replay_equals_eager_and_new_lengths_capture_nothing(tts, tts_graphed):
    syn = tts_graphed.vocoder._synth
    gen = tts_graphed.vocoder.model
    calls = [([20, 11, 7], [100, 0, 50]), ([9, 23, 14], [0, 300, 20]), ([25, 6, 17], [10, 10, 10]), ([12, 12, 28], [999, 1, 0])]
    counts, Ns = [], set()
    for k, (lens, pauses) in enumerate(calls):        # 1st: eager warm-up, 2nd: capture + replay, 3rd and 4th: replay
        texts = _texts(lens, seed=60 + k)
        want, tw = tts.narrate(texts, pauses=pauses, return_timing=True)
        got, tg = tts_graphed.narrate(texts, pauses=pauses, return_timing=True)
        assert np.array_equal(got, want) and tg == tw, k
        Ns.add(gen.plan([m.shape[1] for m in tts_graphed.generate_mel(texts)]).N)
        counts.append(len(syn._rag))
    assert Ns == {3}, Ns                               # three sentences shorter than a window: three rows, whatever their lengths
    assert counts == [0, 1, 1, 1], counts
    (key,) = list(syn._rag)
    assert "join" in key and key[:2] == ("rag", 3)
    # other settings are data too: no new graph, and still the eager result
    texts = _texts([8, 19, 13], seed=70)
    for kw in (dict(normalize="peak", fade_ms=1.0), dict(trim_db=None, normalize=None, fade_ms=0)):
        assert np.array_equal(tts_graphed.narrate(texts, **kw), tts.narrate(texts, **kw))
    assert len(syn._rag) == 1
    # sentences of several windows beside a short row, resampled: one more key (N, rate), captured once, replayed with other pauses
    for k, pauses in enumerate(([100, 0, 50], [5, 5, 5], [0, 0, 700])):
        kw = dict(duration_control=DC, pauses=pauses, sample_rate=16000)
        assert np.array_equal(tts_graphed.narrate(_three(), **kw), tts.narrate(_three(), **kw)), k
    assert len(syn._rag) == 2 and any("rate" in key for key in syn._rag)
