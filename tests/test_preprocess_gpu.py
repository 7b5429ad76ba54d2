"""GPU: recordings + alignments -> the trainer's dataset (tts_king_amd/preprocess.py), and a recording's prosody handed to `speak`
(`TTSKing.extract_prosody`).  The corpus is synthetic and written by the test: 2 speakers x 3 one-second utterances (harmonic glides
with a noise stretch, int16 wav files, one of them at 44 100 Hz so that the resampling step runs), long-format TextGrids and .lab files.

Tolerances.  stats.json's min / max are read back from the written files: equal.  Its mean / std are recomputed by the test from
un-normalised features that it rebuilds itself (`PitchExtractor` + `TacotronSTFT` on the device, the fp64 restatement of the
phoneme-level kernel on the host): the kernel's fp32 values differ from the restatement's by at most the bars of
tests/test_pitch_gpu.py (a few 1e-6 of the largest value), and a mean or a standard deviation of such values inherits at most that,
so 1e-5 of the largest value is the bar.  `extract_prosody` runs the same launches on the same samples, then standardises in fp64
and rounds once to fp32: one unit in the last place (2^-23 relative) against the normalised files."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import pitch_ref
from tts_king_amd import preprocess, textgrid
from tts_king_amd.config import default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PHONES = ["R", "A", "B", "O0", "T", "A"]


def write_textgrid(path, intervals, short=False):
    xmax = intervals[-1][1]
    if short:
        lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "0", str(xmax), "<exists>", "1", '"IntervalTier"', '"phones"', "0",
                 str(xmax), str(len(intervals))]
        for s, e, p in intervals:
            lines += [str(s), str(e), '"%s"' % p]
    else:
        lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %s" % xmax, "tiers? <exists>", "size = 1",
                 "item []:", "    item [1]:", '        class = "IntervalTier"', '        name = "phones"', "        xmin = 0",
                 "        xmax = %s" % xmax, "        intervals: size = %d" % len(intervals)]
        for k, (s, e, p) in enumerate(intervals, 1):
            lines += ["        intervals [%d]:" % k, "            xmin = %s" % s, "            xmax = %s" % e, '            text = "%s"' % p]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def intervals_for(k):
    """Utterance 0 is speech from the first sample to the last; the others have leading and trailing silence and an inner sp."""
    if k == 0:
        marks = [0.0, 0.15, 0.3, 0.5, 0.65, 0.85, 1.0]
        return [(marks[i], marks[i + 1], PHONES[i]) for i in range(6)]
    o = 0.01 * k
    marks = [0.0, 0.07 + o, 0.2 + o, 0.33, 0.47 + o, 0.55 + o, 0.7, 0.82 + o, 0.93, 1.0]
    names = ["sil", "R", "A", "B", "sp", "O0", "T", "A", "sil"]
    return [(marks[i], marks[i + 1], names[i]) for i in range(9)]


def write_utterance(folder, name, k, rate, rng, short=False):
    from scipy.io import wavfile
    hop = 256 * rate // 22050
    y = pitch_ref.glide(rate, rng, f_lo=110.0 + 25 * k, swing=40.0, sr=rate, hop=hop, noise=(30 + 5 * k, 38 + 5 * k), silent=None, peak=0.5)
    wavfile.write(os.path.join(folder, name + ".wav"), rate, np.round(y * 20000).astype(np.int16))
    write_textgrid(os.path.join(folder, name + ".TextGrid"), intervals_for(k), short=short)
    with open(os.path.join(folder, name + ".lab"), "w") as f:
        f.write("utterance %s\n" % name)


def make_config(raw, out, val_size=2):
    cfg = copy.deepcopy(default_config().preprocess_config)
    cfg.path.raw_path, cfg.path.preprocessed_path = str(raw), str(out)
    cfg.preprocessing.val_size = val_size
    return cfg


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    base = tmp_path_factory.mktemp("corpus")
    raw, out = base / "raw", base / "out"
    rng = np.random.default_rng(11)
    k = 0
    for spk in ("anna", "boris"):
        os.makedirs(raw / spk)
        for u in range(3):
            write_utterance(str(raw / spk), "u%d" % u, k, 44100 if (spk, u) == ("boris", 1) else 22050, rng)
            k += 1
    cfg = make_config(raw, out)
    pre = preprocess.Preprocessor(cfg, device=DEV, seed=7)
    lines = pre.build_from_path()
    return cfg, pre, lines, raw, out


def test_files_names_dtypes_shapes(corpus):
    cfg, pre, lines, raw, out = corpus
    assert pre.skipped == [] and len(lines) == 6
    assert json.load(open(out / "speakers.json")) == {"anna": 0, "boris": 1}
    for spk in ("anna", "boris"):
        for u in range(3):
            ld = lambda kind, sub: np.load(out / kind / ("%s-%s-u%d.npy" % (spk, sub, u)))
            mel, dur, pitch, energy, cwt = ld("mel", "mel"), ld("duration", "duration"), ld("pitch", "pitch"), ld("energy", "energy"), ld("pitch", "cwt-pitch")
            T = int(dur.sum())
            assert mel.dtype == np.float32 and mel.shape == (T, 80)
            assert dur.dtype == np.int64 and len(pitch) == len(dur) == len(energy)
            assert pitch.dtype == np.float64 and energy.dtype == np.float64 and np.isfinite(pitch).all() and np.isfinite(energy).all()
            assert cwt.shape == (len(dur), 11) and not cwt.any()
            pm, ps = ld("pitch", "pitch-mean"), ld("pitch", "pitch-std")
            assert pm.shape == () and ps.shape == () and pm.dtype == np.float64 and 4.0 < float(pm) < 6.5 and float(ps) > 0
    ivs = textgrid.read_tier(str(raw / "anna" / "u1.TextGrid"))
    phones, durs, _, _ = textgrid.get_alignment(ivs, 22050, 256)
    assert np.load(out / "duration" / "anna-duration-u1.npy").tolist() == durs
    assert "u1|anna|{%s}|utterance u1" % " ".join(phones) in lines


def rebuild_features(cfg, raw, spk, name):
    """Un-normalised phoneme-level (pitch, energy) of one utterance, rebuilt by the test: host steps by their formulas, the device
    extractors, the fp64 restatement of the reduction."""
    from scipy.io import wavfile
    from tts_king_amd.audio import PitchExtractor, TacotronSTFT
    rate, data = wavfile.read(raw / spk / (name + ".wav"))
    x = data.astype(np.float64)
    if rate != 22050:
        x = preprocess.to_rate(x, rate, 22050, DEV).astype(np.float64)
    x = (np.clip(np.trunc(x / np.max(np.abs(x)) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)
    phones, durs, start, end = textgrid.get_alignment(textgrid.read_tier(str(raw / spk / (name + ".TextGrid"))), 22050, 256)
    x = x[int(22050 * start):int(22050 * end)]
    y = torch.from_numpy(x).to(DEV).unsqueeze(0)
    _, energy = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000, device=DEV).mel_spectrogram(y)
    f0 = PitchExtractor(22050, 256)(y)
    st, p, e, _, _ = pitch_ref.phoneme_prosody(f0[0].cpu().numpy(), energy[0].cpu().numpy(), durs)
    assert st == 0
    return p, e


def test_stats_and_split(corpus):
    cfg, pre, lines, raw, out = corpus
    stats = json.load(open(out / "stats.json"))
    for kind in ("pitch", "energy"):
        files = [f for f in sorted(os.listdir(out / kind)) if not ("mean" in f or "std" in f or "cwt" in f)]
        assert len(files) == 6
        vals = np.concatenate([np.load(out / kind / f) for f in files])
        assert stats[kind][0] == float(vals.min()) and stats[kind][1] == float(vals.max())
    ps, es = [], []
    for spk in ("anna", "boris"):
        for u in range(3):
            p, e = rebuild_features(cfg, raw, spk, "u%d" % u)
            ps.append(preprocess.remove_outlier(p))
            es.append(preprocess.remove_outlier(e))
    for kind, parts in (("pitch", ps), ("energy", es)):
        v = np.concatenate(parts)
        scale = float(np.max(np.abs(v)))
        print("%s: stats.json mean %.9g std %.9g, recomputed %.9g %.9g" % (kind, stats[kind][2], stats[kind][3], v.mean(), v.std()))
        assert abs(stats[kind][2] - v.mean()) <= 1e-5 * scale and abs(stats[kind][3] - v.std()) <= 1e-5 * scale
    train = open(out / "train.txt").read().splitlines()
    val = open(out / "val.txt").read().splitlines()
    assert len(val) == 2 and len(train) == 4 and sorted(train + val) == sorted(lines) and val == lines[:2]


def test_dataset_reads_it_and_collates_the_15_tuple(corpus):
    from tts_king_amd.dataset import Dataset
    cfg, pre, lines, raw, out = corpus
    ds = Dataset("train.txt", cfg, {"optimizer": {"batch_size": 2}}, sort=True, drop_last=True)
    assert len(ds) == 4
    batches = ds.collate_fn([ds[i] for i in range(4)])
    assert len(batches) == 2
    b = batches[0]
    assert len(b) == 15
    L, T = b[5], b[8]
    assert b[3].shape == (2, L) and b[6].shape == (2, T, 80) and b[9].shape == (2, L) and b[10].shape == (2, L) and b[11].shape == (2, L)
    assert b[12].shape == (2, L, 11) and b[13].shape == (2,) and b[14].shape == (2,)
    assert (b[10].sum(axis=1) == b[7]).all() and set(b[2].tolist()) <= {0, 1}


def make_tts(tmp_path, preprocessed_path):
    import yaml
    import tts_king
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config.yaml")))
    cfg["preprocess_config"]["path"]["preprocessed_path"] = str(preprocessed_path)
    cfg["mi355x"]["hip_graph"] = False
    p = tmp_path / "config.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return tts_king.TTSKing(str(p))


def test_extract_prosody_gives_the_training_targets_and_speak_takes_them(corpus, tmp_path):
    from scipy.io import wavfile
    cfg, pre, lines, raw, out = corpus
    tts = make_tts(tmp_path, out)
    rate, data = wavfile.read(raw / "anna" / "u0.wav")
    dur = np.load(out / "duration" / "anna-duration-u0.npy")
    got = tts.extract_prosody(data, dur, sample_rate=rate)
    assert sorted(got) == ["durations", "energy", "pitch"] and got["durations"].tolist() == dur.tolist()
    for kind in ("pitch", "energy"):
        want = np.load(out / kind / ("anna-%s-u0.npy" % kind))
        assert got[kind].dtype == np.float32 and got[kind].shape == want.shape
        err = np.max(np.abs(got[kind] - want) / np.maximum(np.abs(want), 1e-30))
        print("extract_prosody %s: largest relative difference from the file %.3g" % (kind, err))
        assert err <= 2.0 ** -23
    wav = tts.speak("{%s}" % " ".join(PHONES), speaker="anna", **got)
    assert wav.shape[-1] == 256 * int(dur.sum())
    with pytest.raises(ValueError, match="more frames than the audio"):
        tts.extract_prosody(data[:5000], dur, sample_rate=rate)


def test_refusals_name_their_cause(tmp_path):
    raw, out = tmp_path / "raw", tmp_path / "out"
    os.makedirs(raw / "carl")
    rng = np.random.default_rng(12)
    cfg = make_config(raw, out, val_size=0)
    with pytest.raises(ValueError, match="use_cwt"):
        preprocess.Preprocessor(cfg, use_cwt=True, device=DEV)
    bad = copy.deepcopy(cfg)
    bad.preprocessing.energy.feature = "frame_level"
    with pytest.raises(ValueError, match="frame_level"):
        preprocess.Preprocessor(bad, device=DEV)
    write_utterance(str(raw / "carl"), "short", 1, 22050, rng, short=True)
    with pytest.raises(textgrid.TextGridError, match="short-format"):
        preprocess.Preprocessor(cfg, device=DEV).build_from_path()
    os.remove(raw / "carl" / "short.wav")
    write_utterance(str(raw / "carl"), "odd", 1, 22051, rng)
    with pytest.raises(ValueError, match="unsupported sample rate 22051"):
        preprocess.Preprocessor(cfg, device=DEV).build_from_path()
