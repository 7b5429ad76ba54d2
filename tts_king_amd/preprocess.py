"""Data preparation for the FS2 trainer: recordings + alignments -> the files `tts_king_amd/dataset.py` reads.

reference: fs_two/preprocessor/preprocessor.py (`Preprocessor(config).build_from_path()`, `process_utterance`), prepare_data.py.
Input: `raw_path/<speaker>/<name>.wav`, `.lab` (the raw text, first line) and `.TextGrid` (tier "phones", Praat long text format).
Output under `preprocessed_path`: `mel/`, `pitch/`, `energy/`, `duration/` with `<speaker>-<kind>-<name>.npy`, `stats.json`,
`speakers.json`, `train.txt`, `val.txt`, with the reference's names, dtypes and orientation.

The features come from the device: mel and energy from `TacotronSTFT`, F0 from `PitchExtractor` (YIN, not the reference's DIO:
the values differ from pyworld's), the phoneme-level reduction from `ops.phoneme_prosody`.  The corpus statistics are fp64 numpy
on the host.  Departures from the reference, each deliberate:
  * the peak-normalised signal stays in memory (the reference overwrites the input file) and full scale is clamped to int16's range
    (the reference's `astype(int16)` wraps +32768 to -32768);
  * a phoneme of no frames stores 0 and stays out of the utterance's pitch statistics (the reference takes log 0 -> NaN);
  * `cwt-pitch` is written as zeros (Lp, 11): a `use_cwt: False` model ignores it, `use_cwt: True` is refused;
  * `feature: "frame_level"` is refused; the running statistics are only updated by utterances that were written."""
import json
import os
import random

import numpy as np

from . import textgrid

STATUS_TEXT = {1: "fewer than two voiced frames", 2: "the alignment has more frames than the audio", 3: "constant pitch"}
MAX_FRAMES, MAX_PHONEMES = 8192, 1024      # ttsk_phoneme_prosody's limits


def remove_outlier(values):
    """The values strictly inside [p25 - 1.5 IQR, p75 + 1.5 IQR] (preprocessor.py:351-359)."""
    values = np.asarray(values)
    if values.size == 0:
        return values
    p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
    lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
    return values[np.logical_and(values > lower, values < upper)]


class RunningStats:
    """Mean and population standard deviation over batches of values, in fp64 (what sklearn's StandardScaler.partial_fit keeps):
    batches are merged by their counts, means and sums of squared deviations."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, 0.0, 0.0

    def update(self, values):
        v = np.asarray(values, dtype=np.float64).ravel()
        if v.size == 0:
            return
        mb = float(v.mean())
        m2b = float(((v - mb) ** 2).sum())
        tot = self.n + v.size
        delta = mb - self.mean
        self.m2 += m2b + delta * delta * self.n * v.size / tot
        self.mean += delta * v.size / tot
        self.n = tot

    @property
    def std(self):
        return float(np.sqrt(self.m2 / self.n)) if self.n else 0.0


def normalize_dir(in_dir, mean, std):
    """(x - mean) / std over the per-utterance files of `in_dir` (not the -mean-, -std-, cwt- ones), in place -> (min, max)."""
    lo, hi = np.finfo(np.float64).max, np.finfo(np.float64).min
    for name in sorted(os.listdir(in_dir)):
        if "std" in name or "mean" in name or "cwt" in name:
            continue
        path = os.path.join(in_dir, name)
        values = (np.load(path) - np.float64(mean)) / np.float64(std)       # fp64 whatever the file held, as with the reference's numpy scalars
        np.save(path, values)
        if values.size:
            lo, hi = min(lo, float(values.min())), max(hi, float(values.max()))
    return lo, hi


def peak_normalize(x, max_wav_value):
    """clip(trunc(x / max|x| * max_wav_value), -32768, 32767) / 32768 as fp32: the int16 file the reference writes, read back."""
    x = np.asarray(x, dtype=np.float64)
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    if peak == 0.0:
        raise ValueError("a silent recording cannot be peak-normalised")
    return (np.clip(np.trunc(x / peak * max_wav_value), -32768, 32767) / 32768.0).astype(np.float32)


def to_rate(x, rate, target, device, what="recording"):
    """x: 1-D float numpy at `rate` Hz -> 1-D fp32 numpy at `target` Hz through the device resampler; a ratio it refuses is refused here."""
    import torch
    from . import ops, resample
    if int(rate) == int(target):
        return np.asarray(x, dtype=np.float32)
    try:
        filt = resample.filter_for(int(rate), int(target), device)
    except ValueError as e:
        raise ValueError("%s: unsupported sample rate %d Hz (wanted %d Hz): %s" % (what, rate, target, e)) from None
    segs = resample.row_segments(1, len(x), filt.L, filt.M)
    src = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    out = torch.empty(segs.n_dst, dtype=torch.float32, device=device)
    ops.resample(src, torch.from_numpy(segs.table).to(device), filt, out=out)
    return out.cpu().numpy()


def read_wav(path):
    """(rate, 1-D float64 samples) of a mono PCM / float wav file."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.ndim != 1:
        raise ValueError("%s: %d channels; only mono recordings are read" % (path, data.shape[1]))
    return int(rate), data.astype(np.float64)


class Features:
    """The device stages of one utterance, shared by `Preprocessor` and `TTSKing.extract_prosody`."""

    def __init__(self, config, device="cuda:0"):
        from .audio import PitchExtractor, TacotronSTFT
        pp = config["preprocessing"]
        self.device = device
        self.sampling_rate = int(pp["audio"]["sampling_rate"])
        self.max_wav_value = float(pp["audio"]["max_wav_value"])
        self.hop_length = int(pp["stft"]["hop_length"])
        self.stft = TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"], pp["mel"]["n_mel_channels"],
                                 self.sampling_rate, pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"], device=device)
        pc = pp["pitch"]
        self.pitch = PitchExtractor(self.sampling_rate, self.hop_length, window=int(pc.get("window", 1024)), f0_floor=float(pc.get("f0_floor", 71.0)),
                                    f0_ceil=float(pc.get("f0_ceil", 800.0)), threshold=float(pc.get("threshold", 0.15)))

    def prepare(self, samples, rate, what="recording"):
        """Raw samples at `rate` -> the fp32 signal the features are taken from: at the model's rate, peak-normalised."""
        return peak_normalize(to_rate(samples, rate, self.sampling_rate, self.device, what), self.max_wav_value)

    def frame_level(self, wav):
        """wav: 1-D fp32 numpy in [-1, 1] -> (mel (1, 80, T), energy (1, T), f0 (1, T)) on the device, T = 1 + len // hop.  One
        utterance per call: the reflect padding meets the utterance's own end."""
        import torch
        y = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(self.device).unsqueeze(0)
        mel, energy = self.stft.mel_spectrogram(y)
        return mel, energy, self.pitch(y)

    def phoneme_level(self, f0, energy, duration):
        """f0, energy (1, T) on the device, duration: ints per phoneme -> (status, pitch (Lp,), energy (Lp,), pitch_mean, pitch_std)
        as numpy fp32 / floats: `ops.phoneme_prosody` on the first sum(duration) frames."""
        import torch
        from . import ops
        T, Lp = f0.shape[1], len(duration)
        if T > MAX_FRAMES or Lp > MAX_PHONEMES or Lp < 1:
            raise ValueError("an utterance of %d frames and %d phonemes; the phoneme-level reduction takes 1..%d phonemes and at most %d frames"
                             % (T, Lp, MAX_PHONEMES, MAX_FRAMES))
        dur = torch.tensor([list(duration)], dtype=torch.int32, device=f0.device)
        Tn = torch.tensor([T], dtype=torch.int32, device=f0.device)
        Ln = torch.tensor([Lp], dtype=torch.int32, device=f0.device)
        p, e, pm, ps, st = ops.phoneme_prosody(f0.contiguous(), energy.contiguous(), dur, Tn, Ln)
        return int(st[0]), p[0].cpu().numpy(), e[0].cpu().numpy(), float(pm[0]), float(ps[0])


def lab_phonemes(line, g2p=None):
    """The phoneme-id sequence of a `.lab` line: the line itself when it is in the frontend's "{R A B O0 T ...}" notation, else
    `g2p(line)` (a callable returning the ids), else None."""
    from .text import text_to_sequence
    line = line.strip()
    if line.startswith("{") and line.endswith("}"):
        return np.asarray(text_to_sequence(line, []), dtype=np.int64)
    if g2p is not None:
        return np.asarray(g2p(line), dtype=np.int64).reshape(-1)
    return None


def align_speaker(speaker, known, new_speaker_init=None):
    """The model's speaker an utterance of folder `speaker` is synthesized with for alignment: the folder's name when the model
    knows it, else `mi355x.new_speaker_init` when set, else the model's first speaker."""
    if speaker in known:
        return speaker
    return new_speaker_init if new_speaker_init is not None else known[0]


class Preprocessor:
    def __init__(self, config, use_cwt=None, device="cuda:0", seed=1234, aligner=None, g2p=None, align_max_cost=None, new_speaker_init=None):
        """`aligner` (an `align.Aligner`): an utterance without a `.TextGrid` is then aligned on the device instead of being
        skipped: its phonemes are `lab_phonemes(.lab line, g2p)`, its durations the aligner's over the whole recording (no cut)
        with `align_speaker(folder name, ...)`; one whose cost per frame exceeds `align_max_cost` (`mi355x.align_max_cost`;
        None: no limit) is skipped with that reason."""
        self.config = config
        self.aligner, self.g2p, self.align_max_cost, self.new_speaker_init = aligner, g2p, align_max_cost, new_speaker_init
        self.in_dir = config["path"]["raw_path"]
        self.out_dir = config["path"]["preprocessed_path"]
        pp = config["preprocessing"]
        self.val_size = int(pp["val_size"])
        self.seed = seed
        if use_cwt is None:
            use_cwt = bool(pp["pitch"].get("use_cwt", False)) if hasattr(pp["pitch"], "get") else False
        if use_cwt:
            raise ValueError("use_cwt: True is not prepared here: the CWT of the pitch contour (transform_cwt) is out of scope, cwt-pitch files "
                             "are written as zeros for use_cwt: False models")
        for kind in ("pitch", "energy"):
            feat = pp[kind]["feature"]
            if feat == "frame_level":
                raise ValueError('%s feature: "frame_level" is not prepared here; only "phoneme_level" (the shipped configuration) is' % kind)
            if feat != "phoneme_level":
                raise ValueError('%s feature must be "phoneme_level", got %r' % (kind, feat))
        self.pitch_normalization = bool(pp["pitch"]["normalization"])
        self.energy_normalization = bool(pp["energy"]["normalization"])
        self.features = Features(config, device)
        self.sampling_rate, self.hop_length = self.features.sampling_rate, self.features.hop_length
        self.skipped = []                      # (speaker, basename, reason) of the utterances left out

    def build_from_path(self):
        for d in ("mel", "pitch", "energy", "duration"):
            os.makedirs(os.path.join(self.out_dir, d), exist_ok=True)
        out, n_frames = [], 0
        pitch_stats, energy_stats = RunningStats(), RunningStats()
        speakers = {}
        names = sorted(d for d in os.listdir(self.in_dir) if os.path.isdir(os.path.join(self.in_dir, d)))
        for i, speaker in enumerate(names):
            speakers[speaker] = i
            for wav_name in sorted(os.listdir(os.path.join(self.in_dir, speaker))):
                if not wav_name.endswith(".wav"):
                    continue
                basename = wav_name[:-4]
                if os.path.exists(os.path.join(self.in_dir, speaker, basename + ".TextGrid")):
                    ret = self.process_utterance(speaker, basename)
                elif self.aligner is not None:
                    ret = self.process_unaligned(speaker, basename)
                else:
                    self.skipped.append((speaker, basename, "no TextGrid"))
                    continue
                if ret is None:
                    continue
                info, pitch, energy, n = ret
                out.append(info)
                pitch_stats.update(pitch)
                energy_stats.update(energy)
                n_frames += n
        if not out:
            raise ValueError("no utterance under %s could be prepared: %s" % (self.in_dir, self.skipped))
        pitch_mean, pitch_std = (pitch_stats.mean, pitch_stats.std) if self.pitch_normalization else (0.0, 1.0)
        energy_mean, energy_std = (energy_stats.mean, energy_stats.std) if self.energy_normalization else (0.0, 1.0)
        pitch_min, pitch_max = normalize_dir(os.path.join(self.out_dir, "pitch"), pitch_mean, pitch_std)
        energy_min, energy_max = normalize_dir(os.path.join(self.out_dir, "energy"), energy_mean, energy_std)
        with open(os.path.join(self.out_dir, "speakers.json"), "w") as f:
            f.write(json.dumps(speakers))
        with open(os.path.join(self.out_dir, "stats.json"), "w") as f:
            f.write(json.dumps({"pitch": [float(pitch_min), float(pitch_max), float(pitch_mean), float(pitch_std)],
                                "energy": [float(energy_min), float(energy_max), float(energy_mean), float(energy_std)]}))
        self.hours = n_frames * self.hop_length / self.sampling_rate / 3600
        random.Random(self.seed).shuffle(out)
        with open(os.path.join(self.out_dir, "train.txt"), "w", encoding="utf-8") as f:
            for m in out[self.val_size:]:
                f.write(m + "\n")
        with open(os.path.join(self.out_dir, "val.txt"), "w", encoding="utf-8") as f:
            for m in out[:self.val_size]:
                f.write(m + "\n")
        return out

    def _skip(self, speaker, basename, reason):
        self.skipped.append((speaker, basename, reason))
        return None

    def process_utterance(self, speaker, basename):
        base = os.path.join(self.in_dir, speaker, basename)
        phone, duration, start, end = textgrid.get_alignment(textgrid.read_tier(base + ".TextGrid", "phones"), self.sampling_rate,
                                                             self.hop_length)
        if start >= end:
            return self._skip(speaker, basename, "no speech in the alignment")
        text = "{" + " ".join(phone) + "}"
        rate, samples = read_wav(base + ".wav")
        wav = self.features.prepare(samples, rate, base + ".wav")
        wav = wav[int(self.sampling_rate * start):int(self.sampling_rate * end)]
        with open(base + ".lab", "r", encoding="utf-8") as f:
            raw_text = f.readline().strip("\n")
        n = int(sum(duration))
        if len(wav) < 2 or n < 1:
            return self._skip(speaker, basename, "nothing left after the cut")
        return self._write_utterance(speaker, basename, wav, duration, text, raw_text)

    def process_unaligned(self, speaker, basename):
        """An utterance without a `.TextGrid`: phonemes from the `.lab` line, durations from the aligner over the whole recording."""
        from .text import sequence_to_text
        base = os.path.join(self.in_dir, speaker, basename)
        with open(base + ".lab", "r", encoding="utf-8") as f:
            raw_text = f.readline().strip("\n")
        ids = lab_phonemes(raw_text, self.g2p)
        if ids is None or len(ids) < 1:
            return self._skip(speaker, basename, "no TextGrid and no phonemes")
        rate, samples = read_wav(base + ".wav")
        name = align_speaker(speaker, self.aligner.tts.speaker_names, self.new_speaker_init)
        got = self.aligner.align([samples], [ids], [name], [rate])[0]
        if self.align_max_cost is not None and got["cost_per_frame"] > float(self.align_max_cost):
            return self._skip(speaker, basename, "alignment cost per frame %.6g exceeds align_max_cost %.6g" % (got["cost_per_frame"], float(self.align_max_cost)))
        wav = self.features.prepare(samples, rate, base + ".wav")
        return self._write_utterance(speaker, basename, wav, got["durations"].tolist(), sequence_to_text(ids.tolist()), raw_text)

    def _write_utterance(self, speaker, basename, wav, duration, text, raw_text):
        n = int(sum(duration))
        mel, energy, f0 = self.features.frame_level(wav)
        status, pitch, energy_ph, pitch_mean, pitch_std = self.features.phoneme_level(f0, energy, duration)
        if status:
            return self._skip(speaker, basename, STATUS_TEXT[status])
        mel = mel[0, :, :n].cpu().numpy().astype(np.float32)
        pitch = pitch.astype(np.float64)
        save = lambda kind, sub, arr: np.save(os.path.join(self.out_dir, kind, "%s-%s-%s.npy" % (speaker, sub, basename)), arr)
        save("duration", "duration", np.asarray(duration))
        save("pitch", "pitch", pitch)
        save("pitch", "cwt-pitch", np.zeros((len(duration), 11)))
        save("pitch", "pitch-mean", np.float64(pitch_mean))
        save("pitch", "pitch-std", np.float64(pitch_std))
        save("energy", "energy", energy_ph.astype(np.float32))
        save("mel", "mel", mel.T)
        return "|".join([basename, speaker, text, raw_text]), remove_outlier(pitch), remove_outlier(energy_ph), mel.shape[1]
