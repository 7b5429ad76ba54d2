"""GPU: forced alignment end to end (tts_king_amd/align.py, `TTSKing.align`, `extract_prosody(wav, text=...)`, `Preprocessor(aligner=...)`)
on the random-init model of the default configuration: no checkpoint ships, so these tests prove that the path is optimal for the
features that went into the launch and that the plumbing is right, not that the alignment is good.

The cost bound is tests/test_dtw_gpu.py's: with g = (C + Tx + Ty + 4) 2^-24 the kernel's fp32 cost is within 2 g of its path's
fp64 cost, which lies in [A_opt, A_opt (1 + 4 g)]; together |cost - A_opt| <= ((1 + 4 g)(1 + 2 g) - 1) A_opt < 7 g A_opt."""
import os

import numpy as np
import pytest

from tests import dtw_ref, pitch_ref
from tests.test_preprocess_gpu import make_config, write_utterance
from tts_king_amd import ops, preprocess

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TEXT = "{R A B O0 T A}"


def recording(n, seed, f_lo=120.0):
    return pitch_ref.glide(n, np.random.default_rng(seed), f_lo=f_lo, swing=40.0, noise=None, silent=None, peak=0.5)


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import yaml
    import tts_king
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config.yaml")))
    cfg["preprocess_config"]["path"]["preprocessed_path"] = os.path.join(ROOT, "pretrained")
    cfg["mi355x"]["hip_graph"] = False
    p = tmp_path_factory.mktemp("cfg") / "config.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return tts_king.TTSKing(str(p))


@pytest.fixture(scope="module")
def one_second(tts):
    wav = recording(22050, 1)
    return wav, tts.align(wav, TEXT, return_mels=True)


def test_align_one_utterance(one_second):
    wav, got = one_second
    d = got["durations"]
    T = 1 + len(wav) // 256
    assert d.shape == (6,) and d.dtype == np.int64 and (d >= 0).all() and int(d.sum()) == T == got["frames"] == got["y"].shape[0]
    assert got["phonemes"].shape == (6,) and got["x"].shape == (T, 80) and got["y"].shape == (T, 80) and int(got["x_seg"].sum()) == T
    assert np.abs(got["x"].mean(axis=0)).max() < 1e-4 and np.abs(got["y"].mean(axis=0)).max() < 1e-4      # each has its own mean taken out
    A, _, path_x, dur = dtw_ref.dtw(got["x"], got["y"], got["x_seg"])
    opt, cost = A[-1, -1], got["cost_per_frame"] * T
    g = (80 + 2 * T + 4) * 2.0 ** -24
    print("align: cost %.9g, the restatement's optimum %.9g (%.3g relative, bound %.3g); durations %s from synthesized %s"
          % (cost, opt, abs(cost - opt) / opt, 7 * g, d.tolist(), got["x_seg"].tolist()))
    assert abs(cost - opt) <= 7 * g * opt
    if got["path_x"].tolist() == path_x.tolist():
        assert d.tolist() == dur.tolist()
    assert d.tolist() == dtw_ref.durations(got["path_x"], got["x_seg"]).tolist()


def test_a_list_call_gives_each_what_it_gets_alone(tts, one_second):
    wavs = [one_second[0], recording(15000, 2, 150.0), recording(30000, 3, 100.0)]
    texts = [tts.text_preprocess(t) for t in (TEXT, "{T A}", "{B O0 T A R A B}")]
    counts = {}
    ops.LAUNCH_COUNTS = counts
    try:
        both = tts._aligner.align(wavs, texts, tts.speakers[0], 22050)
    finally:
        ops.LAUNCH_COUNTS = None
    assert counts.get("dtw_align") == 1
    assert both[0]["durations"].tolist() == one_second[1]["durations"].tolist()
    for k in (1, 2):
        alone = tts.align(wavs[k], texts[k])
        assert both[k]["durations"].tolist() == alone["durations"].tolist() and both[k]["frames"] == 1 + len(wavs[k]) // 256


def test_speak_copies_the_prosody_from_recording_and_transcript(tts, one_second):
    wav, got = one_second
    pros = tts.extract_prosody(wav, text=TEXT)
    assert sorted(pros) == ["durations", "energy", "pitch"] and pros["durations"].tolist() == got["durations"].tolist()
    out = tts.speak(TEXT, **pros)
    assert out.shape[-1] == 256 * int(pros["durations"].sum())


def test_extract_prosody_with_durations_is_the_route_it_was(tts, one_second):
    """Compared with a direct call of the stages; no alignment launch on that route."""
    wav = one_second[0]
    durs = [15, 14, 0, 20, 18, 20]
    counts = {}
    ops.LAUNCH_COUNTS = counts
    try:
        got = tts.extract_prosody(wav, durs)
    finally:
        ops.LAUNCH_COUNTS = None
    assert "dtw_align" not in counts
    feats = preprocess.Features(tts.cfg.preprocess_config, DEV)
    y = feats.prepare(np.asarray(wav).reshape(-1), 22050, "test")
    _, energy, f0 = feats.frame_level(y)
    st, pitch, energy_ph, _, _ = feats.phoneme_level(f0, energy, durs)
    assert st == 0
    pm, ps = tts._stats["pitch"][2:4]
    em, es = tts._stats["energy"][2:4]
    assert got["durations"].tolist() == durs
    assert np.array_equal(got["pitch"], ((pitch.astype(np.float64) - pm) / ps).astype(np.float32))
    assert np.array_equal(got["energy"], ((energy_ph.astype(np.float64) - em) / es).astype(np.float32))


def test_corpus_with_an_utterance_that_has_no_textgrid(tts, one_second, tmp_path):
    from tts_king_amd.dataset import Dataset
    raw, out = tmp_path / "raw", tmp_path / "out"
    os.makedirs(raw / "anna")
    rng = np.random.default_rng(21)
    for u in range(2):
        write_utterance(str(raw / "anna"), "u%d" % u, u, 22050, rng)
    os.remove(raw / "anna" / "u1.TextGrid")
    (raw / "anna" / "u1.lab").write_text(TEXT + "\n")
    cfg = make_config(raw, out, val_size=0)
    pre = preprocess.Preprocessor(cfg, device=DEV, seed=7)
    assert len(pre.build_from_path()) == 1 and pre.skipped == [("anna", "u1", "no TextGrid")]
    cfg2 = make_config(raw, tmp_path / "out2", val_size=0)
    pre = preprocess.Preprocessor(cfg2, device=DEV, seed=7, aligner=tts._aligner)
    lines = pre.build_from_path()
    assert pre.skipped == [] and sorted(l.split("|")[0] for l in lines) == ["u0", "u1"]
    assert "u1|anna|%s|%s" % (TEXT, TEXT) in lines
    dur = np.load(tmp_path / "out2" / "duration" / "anna-duration-u1.npy")
    mel = np.load(tmp_path / "out2" / "mel" / "anna-mel-u1.npy")
    assert len(dur) == 6 and int(dur.sum()) == mel.shape[0] == 1 + 22050 // 256 and mel.shape[1] == 80
    ds = Dataset("train.txt", cfg2, {"optimizer": {"batch_size": 2}}, sort=True, drop_last=False)
    assert len(ds) == 2
    batch = ds.collate_fn([ds[0], ds[1]])[0]
    assert (batch[10].sum(axis=1) == batch[7]).all()
    # without phonemes and without g2p the utterance is left out, with g2p it is taken; a cost limit leaves it out by name
    (raw / "anna" / "u1.lab").write_text("plain words\n")
    pre = preprocess.Preprocessor(make_config(raw, tmp_path / "out3", val_size=0), device=DEV, aligner=tts._aligner)
    assert len(pre.build_from_path()) == 1 and pre.skipped == [("anna", "u1", "no TextGrid and no phonemes")]
    ids = tts.text_preprocess(TEXT)[0]
    pre = preprocess.Preprocessor(make_config(raw, tmp_path / "out4", val_size=0), device=DEV, aligner=tts._aligner, g2p=lambda line: ids)
    assert len(pre.build_from_path()) == 2 and np.load(tmp_path / "out4" / "duration" / "anna-duration-u1.npy").tolist() == dur.tolist()
    pre = preprocess.Preprocessor(make_config(raw, tmp_path / "out5", val_size=0), device=DEV, aligner=tts._aligner, g2p=lambda line: ids,
                                  align_max_cost=0.0)
    assert len(pre.build_from_path()) == 1 and pre.skipped[0][:2] == ("anna", "u1") and "align_max_cost" in pre.skipped[0][2]


def test_a_recording_past_max_seq_len_is_refused_by_name(tts):
    with pytest.raises(ValueError, match="max_seq_len is 1000 frames"):
        tts.align(recording(256 * 1001, 4), TEXT)
