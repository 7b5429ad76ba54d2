"""Forced alignment on the device: the frames per phoneme of a recording, from the recording and its transcript alone
(DESIGN.md section 19).

The model is itself a description of what each phoneme sounds like: synthesize the transcript with exactly as many frames as the
recording's mel has (`target_frames`), so that every synthesized frame belongs to a known phoneme, then align the synthesized
frames to the recording's by dynamic time warping (`ops.dtw_align`, one launch for all utterances) and count the recording's
frames per phoneme.  The recording is taken whole: leading or trailing silence lands in the first and last phoneme (trimming is
out of scope).  How good the alignment is depends on the model; nothing here measures that."""
import numpy as np
import torch


class Aligner:
    """`Aligner(tts, preprocess_config, device)`: `tts` is an `FSTWOapi`, the features are `preprocess.Features` of the config."""

    def __init__(self, tts, preprocess_config, device="cuda:0", features=None):
        from . import preprocess
        self.tts = tts
        self.device = device
        self.features = features if features is not None else preprocess.Features(preprocess_config, device)
        self.max_frames = int(tts.model.max_seq_len)

    def recording_mel(self, wav, sample_rate, what="align"):
        """1-D samples at `sample_rate` -> the recording's mel (T, 80) fp32 on the device: `Features.prepare` (resample, peak
        normalisation) and `TacotronSTFT`, one call per recording as data preparation does."""
        if torch.is_tensor(wav):
            wav = wav.detach().cpu().numpy()
        y = self.features.prepare(np.asarray(wav).reshape(-1), int(sample_rate), what)
        src = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(self.device).unsqueeze(0)
        mel, _ = self.features.stft.mel_spectrogram(src)
        return mel[0].transpose(0, 1).contiguous()

    def align(self, wavs, texts, speakers=None, sample_rates=22050, return_mels=False):
        """wavs: a list of 1-D recordings; texts: a list of phoneme-id arrays; speakers: a name or a list of names (None: the first
        speaker); sample_rates: one rate or one per recording -> a list of {"durations" (L,) int64: the recording's frames per
        phoneme, summing to "frames"; "phonemes" (L,) int64; "cost_per_frame": the path's cost / frames, by which a caller can
        reject a bad match (a wrong transcript, noise); "frames"}.

        Both mels are fp32 (T, 80); from each its own per-channel mean over its frames is subtracted (a torch op on the device),
        which takes out level and channel differences between the model's output and the recording.  `return_mels`: also "x" and
        "y", the two feature arrays (numpy) that went into the launch, "x_seg" (the synthesized frames per phoneme) and "path_x".
        All texts go through one `generate_batch(..., target_frames=...)` call; a text for which the model predicts no frame at
        all (nothing for the frame budget to scale) goes through a second one with the frames shared equally among its phonemes.
        The recording is taken whole: silence at its ends lands in the first and last phoneme.  A recording of more than
        max_seq_len frames and a non-finite cost raise ValueError."""
        from . import batching, ops
        Bn = len(wavs)
        if Bn == 0 and len(texts) == 0:
            return []
        ids = batching.as_id_rows(texts)
        if len(ids) != Bn:
            raise ValueError("align: %d recordings and %d texts" % (Bn, len(ids)))
        names = batching.per_utterance_names(speakers, Bn, "speakers")
        rates = [int(sample_rates)] * Bn if np.ndim(sample_rates) == 0 else [int(r) for r in sample_rates]
        if len(rates) != Bn:
            raise ValueError("align: %d recordings and %d sample rates" % (Bn, len(rates)))
        ys = []
        for k in range(Bn):
            mel = self.recording_mel(wavs[k], rates[k], "align: recording %d" % k)
            if mel.shape[0] > self.max_frames:
                raise ValueError("align: recording %d has %d frames; the model's max_seq_len is %d frames" % (k, mel.shape[0], self.max_frames))
            ys.append(mel)
        Ty = [int(m.shape[0]) for m in ys]
        mels, pros = self.tts.generate_batch(ids, speaker_names=names, target_frames=Ty, return_prosody=True)
        # The frame budget scales the model's own durations; a text for which the model predicts no frame at all has nothing to scale
        # (such phonemes stay at 0).  Those utterances are synthesized once more with the frames shared equally.
        short = [k for k in range(Bn) if pros[k] is None or mels[k].shape[1] != Ty[k]]
        if short:
            even = [np.full(len(ids[k]), Ty[k] // len(ids[k]), dtype=np.float64) + (np.arange(len(ids[k])) < Ty[k] % len(ids[k])) for k in short]
            m2, p2 = self.tts.generate_batch([ids[k] for k in short], speaker_names=[names[k] for k in short], durations=even, return_prosody=True)
            for r, k in enumerate(short):
                mels[k], pros[k] = m2[r], p2[r]
        xs = [m[0].float() for m in mels]
        for k in range(Bn):
            if pros[k] is None or xs[k].shape[0] != Ty[k]:
                raise ValueError("align: utterance %d could not be synthesized at %d frames (got %d)" % (k, Ty[k], xs[k].shape[0]))
        C = ys[0].shape[1]
        ldx, ldy, ldL = max(x.shape[0] for x in xs), max(Ty), max(len(r) for r in ids)
        x = torch.zeros(Bn, ldx, C, dtype=torch.float32, device=self.device)
        y = torch.zeros(Bn, ldy, C, dtype=torch.float32, device=self.device)
        seg = torch.zeros(Bn, ldL, dtype=torch.int32, device=self.device)
        for k in range(Bn):
            x[k, :xs[k].shape[0]] = xs[k] - xs[k].mean(dim=0, keepdim=True)
            y[k, :Ty[k]] = ys[k] - ys[k].mean(dim=0, keepdim=True)
            seg[k, :len(ids[k])] = pros[k]["dur"].to(torch.int32)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        path_x, cost, status, dur = ops.dtw_align(x, y, i32([t.shape[0] for t in xs]), i32(Ty), seg, i32([len(r) for r in ids]))
        cost, status, dur = cost.cpu().numpy(), status.cpu().numpy(), dur.cpu().numpy()
        out = []
        for k in range(Bn):
            if status[k] != 0:
                raise ValueError("align: utterance %d: dtw_align status %d" % (k, int(status[k])))
            if not np.isfinite(cost[k]):
                raise ValueError("align: utterance %d: the alignment's cost is not finite (%r)" % (k, float(cost[k])))
            one = {"durations": dur[k, :len(ids[k])].astype(np.int64), "phonemes": np.asarray(ids[k], dtype=np.int64),
                   "cost_per_frame": float(cost[k]) / Ty[k], "frames": Ty[k]}
            if return_mels:
                one["x"], one["y"] = x[k, :xs[k].shape[0]].cpu().numpy(), y[k, :Ty[k]].cpu().numpy()
                one["x_seg"], one["path_x"] = seg[k, :len(ids[k])].cpu().numpy(), path_x[k, :Ty[k]].cpu().numpy()
            out.append(one)
        return out
