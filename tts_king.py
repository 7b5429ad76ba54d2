"""TTSKing — the reference's top-level synthesis surface (reference: tts_king.py:18-66) on MI355X.

`TTSKing(config_path)`, `.generate_mel(text, d, p, e, speaker)`, `.mel_to_wav(mel)`, `.speakers`, `.text_preprocess`,
`.to_torch_device` keep the reference signatures.  The text frontend (russian_g2p / g2p_en, fs_two/text) is outside this
build's G2P dependency list: `text` may be a phoneme-id array (1, L) (what `text_preprocess` returns in the reference), a
phoneme string "{R A B O0 T ...}" (tts_king_amd/text.py, pinned by the notebook's known-answer vector), or — when the
optional `russian_g2p` package is importable — plain Russian text.
"""
import numpy as np
import torch

from tts_king_amd.config import load_config
from fsapi import FSTWOapi
from hifiapi import HIFIapi
from tts_king_amd.audio import GriffinLimVocoder


class TTSKing:
    def __init__(self, config_path="./config.yaml"):
        self.cfg = load_config(config_path)
        self.tts = FSTWOapi(self.cfg, self.cfg.gpu)
        self.vocoder = self._build_vocoder(self._configured_vocoder())   # "hifigan", or "griffin_lim": no `hifi` checkpoint is then needed
        self.speakers = self.tts.speaker_names

    def _configured_vocoder(self):
        """`mi355x.vocoder`: "hifigan" (the default) or "griffin_lim"."""
        from tts_king_amd.audio import vocoder_name
        return vocoder_name((self.cfg.get("mi355x", None) or {}).get("vocoder", None))

    def _build_vocoder(self, name):
        return (HIFIapi if name == "hifigan" else GriffinLimVocoder)(self.cfg, self.cfg.gpu)

    def _vocoder(self, name):
        """The vocoder object of `name`: None or the configured name is `self.vocoder`, the other one is built on first use."""
        from tts_king_amd.audio import vocoder_name
        configured = self._configured_vocoder()
        name = vocoder_name(name, configured)
        if name == configured:
            return self.vocoder
        if "_other_vocoder" not in self.__dict__:
            self._other_vocoder = self._build_vocoder(name)
        return self._other_vocoder

    def generate_mel(self, text, duration_control=1.0, pitch_control=1.0, energy_control=1.0, speaker=0, durations=None, pitch=None,
                     energy=None, target_frames=None, return_prosody=False):
        """One text -> (1, T, 80) mel (reference: tts_king.py:25-45).  A list of texts -> a list of such mels, run together
        (`FSTWOapi.generate_batch`): each is what its text gives alone; `speaker` and the controls may then be lists, one per text.

        Per-phoneme prosody (`FSTWOapi.generate_batch`): for one text a control may be a 1-D array over its
        phonemes, `durations` / `pitch` / `energy` a scalar or such an array (NaN = keep the prediction) and `target_frames` the exact
        number of frames wanted; for a list of texts each of these is a list with one entry per text.  `return_prosody`: (mel,
        {"logd", "dur", "pitch", "energy"}) -- lists of both for a list of texts.  One text with any of this runs as a batch of one."""
        new = dict(durations=durations, pitch=pitch, energy=energy, target_frames=target_frames, return_prosody=return_prosody)
        if isinstance(text, (list, tuple)):
            from tts_king_amd import batching
            phonemes = [t if isinstance(t, np.ndarray) else self.text_preprocess(t) for t in text]
            names = [self.speakers[s] if isinstance(s, (int, np.integer)) else s
                     for s in batching.per_utterance_names(speaker, len(phonemes), "speaker")]
            return self.tts.generate_batch(phonemes, duration_control, pitch_control, energy_control, speaker_names=names, **new)
        controls = (duration_control, pitch_control, energy_control)
        if return_prosody or any(v is not None for v in (durations, pitch, energy, target_frames)) or any(np.ndim(c) > 0 for c in controls):
            one = lambda v: None if v is None else [v]
            out = self.generate_mel([text], *[one(c) for c in controls], speaker=[speaker], durations=one(durations), pitch=one(pitch),
                                    energy=one(energy), target_frames=one(target_frames), return_prosody=return_prosody)
            return (out[0][0], out[1][0]) if return_prosody else out[0]
        phonemes = text if isinstance(text, np.ndarray) else self.text_preprocess(text)
        if isinstance(speaker, int):
            speaker = self.speakers[speaker]
        return self.tts.generate(phonemes, duration_control, pitch_control, energy_control, speaker_name=speaker)

    def mel_to_wav(self, mel_spec, sample_rate=None, vocoder=None, griffin_iters=60):
        """(1, T, 80) mel -> int16 ndarray (1, 1, 256 T).  reference: tts_king.py:47-49.
        A list of (1, T_i, 80) mels of any lengths -> a list of such arrays, vocoded together as fixed-size windows
        (`HIFIapi.generate_ragged`); a one-element list is how a single long utterance gets onto the bounded graph set.
        `sample_rate` (Hz): the waveform at that rate, ceil(256 T L / M) samples, resampled on the device (`HIFIapi.generate`).
        `vocoder`: "hifigan", "griffin_lim" or None for `mi355x.vocoder` (default "hifigan").  "griffin_lim" needs no checkpoint and
        takes the preprocess_config's `n_mel_channels` up to 1024 and STFT parameters with filter_length a power of two in 64..2048
        and hop_length a divisor of it (`audio.GriffinLimVocoder`, which refuses anything else by the config key's name; DESIGN.md
        section 21): `griffin_iters` iterations, hop_length * (T - 1) samples, every utterance scaled to a peak of 0.95; a list runs
        as one batch and each array equals its solo call's."""
        voc = self._vocoder(vocoder)
        extra = dict(griffin_iters=griffin_iters) if isinstance(voc, GriffinLimVocoder) else {}
        if isinstance(mel_spec, (list, tuple)):
            return voc.generate_ragged(mel_spec, frames_first=True, sample_rate=sample_rate, **extra)
        return voc.generate(mel_spec.transpose(1, 2), sample_rate=sample_rate, **extra)

    def speak(self, text, duration_control=1.0, pitch_control=1.0, energy_control=1.0, speaker=0, durations=None, pitch=None, energy=None,
              target_frames=None, return_prosody=False, sample_rate=None, vocoder=None, griffin_iters=60):
        """reference: tts_king.py:51-57 calls a missing `generate_mel_batch`; here: mel -> float waveform.  A list of texts -> a list
        of float waveforms (1, 1, 256 T_i) on the device: the batched mels go straight into the vocoder's ragged route.  The prosody
        arguments are `generate_mel`'s (`target_frames` frames are 256 * target_frames samples); `return_prosody`: (waveforms, prosody).
        `sample_rate` (Hz): the waveforms at that rate (`HIFIapi.__call__` / `call_ragged`).  `vocoder`, `griffin_iters`: as in
        `mel_to_wav`; the Griffin-Lim route returns float waveforms too, hop_length * (T_i - 1) samples each."""
        out = self.generate_mel(text, duration_control, pitch_control, energy_control, speaker, durations=durations, pitch=pitch, energy=energy,
                                target_frames=target_frames, return_prosody=return_prosody)
        mels, prosody = out if return_prosody else (out, None)
        voc = self._vocoder(vocoder)
        extra = dict(griffin_iters=griffin_iters) if isinstance(voc, GriffinLimVocoder) else {}
        if isinstance(text, (list, tuple)):
            wav = voc.call_ragged(mels, frames_first=True, sample_rate=sample_rate, **extra)
        else:
            wav = voc(mels.transpose(1, 2), sample_rate=sample_rate, **extra)
        return (wav, prosody) if return_prosody else wav

    def narrate(self, text, speaker=0, duration_control=1.0, pitch_control=1.0, energy_control=1.0, pauses=None, trim_db=-45.0,
                trim_keep_ms=15.0, fade_ms=5.0, normalize="rms", target_db=-23.0, peak_limit=0.95, sample_rate=None, vocoder=None,
                griffin_iters=60, return_timing=False):
        """A paragraph in one call -> int16 ndarray (1, 1, total): the text cut into sentences (tts_king_amd/narrate.py: at . ? ! … ; :
        outside {...}, a piece of more than 200 phonemes also at its commas; a list of strings or phoneme-id arrays is taken as
        already split), the sentences synthesized as batches of at most `mi355x.narrate_batch` (32) through `generate_mel([...])` and
        the vocoder's ragged route, and joined on the device: per sentence the silence at either end below
        `trim_db` dB of the sentence's peak is cut but for `trim_keep_ms`, the level is set (`normalize`: "rms" = `target_db` dB RMS
        re full scale under a peak of `peak_limit`, "peak" = a peak of `peak_limit`, None = left as it is), both cuts get a linear
        fade of `fade_ms`, and a pause follows: 400 ms after . ? ! …, 250 ms after ; :, 120 ms after a comma cut
        (`mi355x.narrate_pauses`: {end, half, comma} in ms), or `pauses` = one number of ms or one per sentence.  Pauses and the
        other times are samples at the OUTPUT rate (`sample_rate`, as in `mel_to_wav`).  `trim_db=None` / `normalize=None` switch
        those steps off.  `speaker` and the three controls may be lists, one per sentence.  `return_timing`: also a list of
        (start_sample, end_sample) per sentence, in the order given.  A text that yields no sentence raises ValueError."""
        from tts_king_amd import batching, narrate
        mi = self.cfg.get("mi355x", None) or {}
        voc = self._vocoder(vocoder)
        extra = dict(griffin_iters=griffin_iters) if isinstance(voc, GriffinLimVocoder) else {}
        count = lambda piece: int(np.asarray(self.text_preprocess(piece)).size)
        max_ph = min(narrate.MAX_PHONEMES, int(self.tts.model.max_seq_len))
        pieces, marks = narrate.split_text(text, max_ph, count)
        n = len(pieces)
        if n == 0:
            raise ValueError("narrate: the text yields no sentence")
        rate = voc.output_rate(sample_rate)
        join = narrate.Join(narrate.settings(rate, trim_db, trim_keep_ms, fade_ms, normalize, target_db, peak_limit),
                            narrate.pause_plan(marks, rate, pauses, mi.get("narrate_pauses", None)))
        per = lambda v, name: v if np.ndim(v) == 0 else list(batching.per_utterance_names(v, n, name))
        spk = per(speaker, "speaker")
        ctl = [per(c, name) for c, name in ((duration_control, "duration_control"), (pitch_control, "pitch_control"),
                                            (energy_control, "energy_control"))]
        cut = lambda v, lo, hi: v[lo:hi] if isinstance(v, list) else v
        wavs, timing, base = [], [], 0
        for lo, hi in narrate.groups(n, int(mi.get("narrate_batch", narrate.BATCH))):
            mels = self.generate_mel(pieces[lo:hi], *[cut(c, lo, hi) for c in ctl], speaker=cut(spk, lo, hi))
            wav, info = voc.generate_joined(mels, join.part(lo, hi), frames_first=True, sample_rate=sample_rate, **extra)
            wavs.append(wav)
            timing += [(base + s, base + e) for s, e in info.timing()]
            base += info.total
        wav = wavs[0] if len(wavs) == 1 else np.concatenate(wavs, axis=2)
        return (wav, timing) if return_timing else wav

    def _device_features(self):
        import json
        import os
        from tts_king_amd import preprocess
        if not hasattr(self, "_features"):
            self._features = preprocess.Features(self.cfg.preprocess_config, self.cfg.gpu)
            with open(os.path.join(self.cfg.preprocess_config.path.preprocessed_path, "stats.json")) as f:
                self._stats = json.load(f)
        return self._features

    def align(self, wav, text, speaker=0, sample_rate=22050, return_mels=False):
        """A recording's frames per phoneme from the recording and its transcript alone (tts_king_amd/align.py, DESIGN.md section
        19): the transcript is synthesized at the recording's frame count and the two mels are aligned by dynamic time warping on
        the device.  `wav`: 1-D samples at `sample_rate` Hz; `text`: anything `generate_mel` takes.  -> {"durations" (one integer
        per phoneme, summing to "frames"), "phonemes", "cost_per_frame", "frames"}.  The recording is taken whole: silence at its
        ends lands in the first and last phoneme."""
        from tts_king_amd.align import Aligner
        if not hasattr(self, "_aligner"):
            self._aligner = Aligner(self.tts, self.cfg.preprocess_config, self.cfg.gpu, features=self._device_features())
        phonemes = text if isinstance(text, np.ndarray) else self.text_preprocess(text)
        name = self.speakers[speaker] if isinstance(speaker, (int, np.integer)) else speaker
        return self._aligner.align([wav], [phonemes], [name], [sample_rate], return_mels=return_mels)[0]

    def extract_prosody(self, wav, durations=None, sample_rate=22050, *, text=None, speaker=0):
        """A recording's per-phoneme prosody in the form `speak` / `generate_mel` take: {"durations", "pitch", "energy"}, one
        value per phoneme.  `wav`: 1-D samples (numpy or torch, any scale) at `sample_rate` Hz covering exactly the aligned speech;
        `durations`: frames per phoneme (e.g. `textgrid.get_alignment`), or None with `text` (and `speaker`) given: the durations
        then come from `align(wav, text, speaker, sample_rate)`, so that `speak(text, **tts.extract_prosody(wav, text=text))` copies
        a recording's prosody from the recording and its transcript alone.  Exactly one of `durations` and `text` must be given.
        The recording goes through the data-preparation stages
        (tts_king_amd/preprocess.py: resample to the model's rate, peak-normalise, energy from `TacotronSTFT`, F0 from
        `PitchExtractor` (YIN), the phoneme-level reduction on the device), then `(x - mean) / std` with the pitch and energy mean
        and std of the model's stats.json: exactly what the normalisation pass writes into the training targets.  Those are the
        units of `pitch=` and `energy=` (a set value is used as is, `scaled[l] = value[l]`, and bucketed
        against the stats.json range), so `speak(text, **tts.extract_prosody(wav, durations))` reproduces the recording's prosody.
        Raises ValueError when the recording has no usable pitch (fewer than two voiced frames, constant pitch) or fewer frames
        than the durations ask for."""
        from tts_king_amd import preprocess
        if (durations is None) == (text is None):
            raise ValueError("extract_prosody: give exactly one of `durations` (frames per phoneme) and `text` (the transcript, aligned "
                             "to the recording by `align`); got %s" % ("neither" if durations is None else "both"))
        self._device_features()
        if torch.is_tensor(wav):
            wav = wav.detach().cpu().numpy()
        wav = np.asarray(wav).reshape(-1)
        if durations is None:
            durations = self.align(wav, text, speaker=speaker, sample_rate=sample_rate)["durations"]
        durations = np.asarray(durations).reshape(-1).astype(np.int64)
        y = self._features.prepare(wav, int(sample_rate), "extract_prosody")
        _, energy, f0 = self._features.frame_level(y)
        status, pitch, energy_ph, _, _ = self._features.phoneme_level(f0, energy, durations.tolist())
        if status:
            raise ValueError("extract_prosody: %s (%d samples, %d frames of durations)" % (preprocess.STATUS_TEXT[status], len(y), int(durations.sum())))
        pm, ps = self._stats["pitch"][2:4]
        em, es = self._stats["energy"][2:4]
        return {"durations": durations, "pitch": ((pitch.astype(np.float64) - pm) / ps).astype(np.float32),
                "energy": ((energy_ph.astype(np.float64) - em) / es).astype(np.float32)}

    def text_preprocess(self, text):
        """reference: tts_king.py:59-60 -> input_process.preprocess_rus (needs russian_g2p).  A string that already is in
        the phoneme notation of the reference's frontend, "{R A B O0 T ...}", is converted directly."""
        from input_process import preprocess_rus
        from tts_king_amd.text import text_to_sequence
        if "{" in text:
            return np.array([text_to_sequence(text, [])])
        return np.array([preprocess_rus(text)])

    def text_preprocess_eng(self, text):
        """reference: tts_king.py:62-63."""
        from input_process import preprocess_eng
        return np.array([preprocess_eng(text, self.cfg.preprocess_config)])

    def to_torch_device(self, items):
        return [torch.tensor(t).to(self.cfg.gpu) for t in items]
