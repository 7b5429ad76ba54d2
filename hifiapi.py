"""HIFIapi — the reference's vocoder facade (reference: hifiapi.py:11-52) over the MI355X HiFi-GAN generator.

Same constructor, attributes (`.model .cfg .device`), `__call__(x)` (float waveform, (B,1,256T)) and
`generate(mel_specs)` (int16 ndarray, C truncation toward zero after *MAX_WAV_VALUE).  The generator runs only on a
HIP device: `model_config.vocoder.use_cpu: true` (the reference default) is rejected loudly, there is no CPU path.
Every route takes `sample_rate=` (Hz): the waveform resampled on the device (tts_king_amd/resample.py); None = the optional
`mi355x.output_sample_rate`, or without it `hifi.sampling_rate`, at which nothing changes.
"""
import torch

from tts_king_amd import ops
from tts_king_amd.hifigan import Generator


class AttrDict(dict):
    """reference: hifiapi.py:5-8."""

    def __init__(self, *args, **kwargs):
        super(AttrDict, self).__init__(*args, **kwargs)
        self.__dict__ = self


def _device_of(device):
    if device in ("gpu", None):
        return torch.device("cuda:0")
    if isinstance(device, int):
        return torch.device("cuda:%d" % device)
    return torch.device(device)


class HIFIapi:
    def __init__(self, config, device="gpu"):
        if config.model_config["vocoder"]["use_cpu"]:
            raise ops.L.TtskError("model_config.vocoder.use_cpu: true — this build runs the HiFi-GAN generator on hand-written "
                                  "MI355X kernels only; set use_cpu: false and gpu: 'cuda:0'")
        device = _device_of(device)
        if device.type != "cuda":
            raise ops.L.TtskError("HIFIapi needs a HIP device (gpu: 'cuda:0'), got %s" % device)
        weights_path = config.hifi.weights_path
        self.model = Generator(config.hifi)
        if weights_path is not None:
            checkpoint = torch.load(weights_path, map_location="cpu")
            self.model.load_state_dict(checkpoint["generator"])
        else:
            self.model.reset_parameters(int(config.hifi.get("seed", 1234)))      # no checkpoint ships with the repo
        self.cfg = config
        self.device = device
        self.model.to(device)
        self.model.remove_weight_norm()
        self.model.eval()
        mi = config.get("mi355x", {}) if hasattr(config, "get") else {}
        self._synth = None
        self.output_sample_rate = mi.get("output_sample_rate", None) if mi else None
        self.model.resampler(self.output_sample_rate)                              # a rate the resampler refuses fails here, not at the first call
        if mi and mi.get("hip_graph", False):
            from tts_king_amd.synth import GraphedSynthesizer
            self._synth = GraphedSynthesizer(None, self.model)

    def train(self):
        """reference: hifiapi.py:32-33 raises (`NotImplemented(...)` is not callable -> TypeError there)."""
        raise NotImplementedError(" Train for HiFi was not implemented yet")

    def _rate(self, sample_rate):
        """The rate to resample to, or None for the generator's own (`sample_rate` None: the configured default)."""
        rate = self.output_sample_rate if sample_rate is None else sample_rate
        return None if self.model.resampler(rate) is None else int(rate)

    def __call__(self, x, sample_rate=None):
        """mel (B,80,T) -> float waveform (B,1,256T) on the device; `sample_rate`: (B,1,ceil(256 T L / M)) at that rate."""
        x = x.to(self.device)
        rate = self._rate(sample_rate)
        if rate is None:
            return self.model(x)
        with torch.no_grad():
            return self.model.resample_rows(self.model(x), rate)

    def generate(self, mel_specs, sample_rate=None):
        """mel (B,80,T) -> int16 ndarray (B,1,256T) on the host.  reference: hifiapi.py:40-52.  `sample_rate`: (B,1,ceil(256 T L / M))
        at that rate, every row resampled on the device as an utterance of its own and converted there (saturating)."""
        self.model.eval()
        rate = self._rate(sample_rate)
        scale = float(self.cfg.hifi.MAX_WAV_VALUE)
        with torch.no_grad():
            mel_specs = mel_specs.to(self.device)
            if rate is not None:
                if self._synth is not None:
                    audio = self._synth.wav(mel_specs.float(), rate, scale)
                else:
                    audio = self.model.resample_rows(self.model(mel_specs), rate, scale)
                return ops.to_host(audio).numpy()
            audio = self._synth.wav(mel_specs.float()) if self._synth is not None else self.model(mel_specs)
            audio = ops.to_int16(audio, scale)                                     # scale + truncate toward zero on device
            audio = ops.to_host(audio).numpy()                                     # D2H through a pinned staging buffer
        return audio

    def call_ragged(self, mels, frames_first=False, sample_rate=None):
        """The ragged counterpart of `__call__`: a list of mels of any lengths (layouts as in `generate_ragged`) -> a list of float
        waveforms (1, 1, 256 T_i) on the device, through the same windowed route; device mels are not taken to the host.
        `sample_rate`: (1, 1, ceil(256 T_i L / M)) at that rate."""
        self.model.eval()
        rate = self._rate(sample_rate)
        with torch.no_grad():
            if self._synth is not None:
                return self._synth.wav_ragged(mels, frames_first, sample_rate=rate)
            return self.model.forward_ragged(mels, frames_first, sample_rate=rate)

    def generate_ragged(self, mels, frames_first=False, sample_rate=None):
        """mels: a list of (80, T_i) or (1, 80, T_i) mels of any lengths (`frames_first`: FastSpeech2's (T_i, 80) / (1, T_i, 80) rows) ->
        a list of int16 ndarrays (1, 1, 256 T_i) on the host, each the truncation of what the generator gives for that mel alone.
        The utterances run together as fixed-size windows of `tts_king_amd.windows.W` frames (`Generator.forward_ragged`; with
        `hip_graph` one replayed graph per window count) and come back in ONE device-to-host copy; a shorter one is a row of the same
        batch with its own length, and goes through the generator alone only where `Generator.short_rows()` is False.
        `sample_rate`: arrays of ceil(256 T_i L / M) samples at that rate, resampled and converted (saturating) by one more launch
        before the copy, which then carries the resampled samples only."""
        from tts_king_amd import resample
        self.model.eval()
        scale = float(self.cfg.hifi.MAX_WAV_VALUE)
        rate = self._rate(sample_rate)
        mels = list(mels)
        with torch.no_grad():
            if self._synth is not None:
                flat, plan, spf = self._synth.wav_ragged_flat(mels, frames_first, scale, rate)
                short = self.model.forward_short(mels, plan, frames_first, scale, forward=self._synth.wav, sample_rate=rate)
            else:
                flat, plan, spf = self.model.forward_ragged_flat(mels, frames_first, scale, rate)
                short = self.model.forward_short(mels, plan, frames_first, scale, sample_rate=rate)
            host = None if flat is None else ops.to_host(flat).numpy()              # one D2H copy; its shape repeats with N
            short = {i: ops.to_host(y).numpy() for i, y in short.items()}
        return resample.split(host, plan, spf, short)

    def output_rate(self, sample_rate=None):
        """The rate (Hz) of what a call with `sample_rate` returns."""
        rate = self._rate(sample_rate)
        return int(self.cfg.hifi.sampling_rate) if rate is None else rate

    def _joined(self, mels, join, frames_first, sample_rate, scale):
        self.model.eval()
        rate = self._rate(sample_rate)
        with torch.no_grad():
            if self._synth is not None:
                return self._synth.wav_joined(mels, join, frames_first, scale, rate)
            return self.model.forward_joined(mels, join, frames_first, scale, rate)

    def call_joined(self, mels, join, frames_first=False, sample_rate=None):
        """The mels of `call_ragged` as ONE float waveform (1, 1, total) on the device, joined there by `join` (a
        `tts_king_amd.narrate.Join`: per utterance trim, level, fade, pause; `Generator.forward_joined`, with `hip_graph` part of the
        ragged graph) -> (waveform, `narrate.Info`: every utterance's kept range, place, peak and gain, read from the device table)."""
        from tts_king_amd import narrate
        mels = list(mels)
        out, info, _ = self._joined(mels, join, frames_first, sample_rate, None)
        info = narrate.Info(ops.to_host(info).numpy(), len(mels))
        return out[:info.total].clone().reshape(1, 1, info.total), info

    def generate_joined(self, mels, join, frames_first=False, sample_rate=None):
        """`call_joined` as an int16 ndarray (1, 1, total) on the host (saturating): the join's launch converts, and the waveform
        crosses to the host in one copy, the table in another of 32 bytes per utterance."""
        from tts_king_amd import narrate
        mels = list(mels)
        out, info, _ = self._joined(mels, join, frames_first, sample_rate, float(self.cfg.hifi.MAX_WAV_VALUE))
        host = ops.to_host(out).numpy()
        info = narrate.Info(ops.to_host(info).numpy(), len(mels))
        return host[:info.total].reshape(1, 1, info.total), info
