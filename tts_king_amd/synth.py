"""hipGraph-captured synthesis: text ids -> mel -> waveform with two host-visible steps.

reference path: tts_king.py:25-49 (`generate_mel` -> `mel_to_wav`), fsapi.py:38-82, hifiapi.py:40-52.  The reference
launches ~400 small ATen ops per utterance and syncs per phoneme in the LengthRegulator; here the path is three replayed
graphs: A = encoder + variance adaptor + duration totals (shape key: phonemes L, controls), then ONE host read of the
frame count T (the only data-dependent shape), B = LengthRegulator + decoder + PostNet (key: L, T), C = HiFi-GAN
generator (key: T; `wav_ragged`: the windowed generator, key: the number of windows N, whatever the lengths).  Graphs are cached per key (utterances of equal L and T replay the same graphs); a key's first call
runs eagerly once (warm-up: lazy allocations, weight packing) and is captured on the second.
"""
import torch

from . import ops
from . import windows


class _Graph:
    def __init__(self, fn, static_inputs):
        self.static = static_inputs
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = fn(*self.static)

    def run(self, *inputs):
        for dst, src in zip(self.static, inputs):
            if torch.is_tensor(dst):
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.out


class GraphedSynthesizer:
    def __init__(self, fs2, vocoder=None, max_graphs=32):
        self.fs2, self.vocoder, self.max_graphs = fs2, vocoder, max_graphs
        self._front, self._back, self._voc, self._rag = {}, {}, {}, {}
        self._seen = set()

    def _get(self, cache, key, fn, inputs):
        """Eager on first sight of `key`, captured on the second, replayed afterwards."""
        if key is None:                 # not capturable (host-side position table for > max_seq_len): plain launches
            return fn(*inputs)
        g = cache.get(key)
        if g is not None:
            return g.run(*inputs)
        if key not in self._seen:
            self._seen.add(key)
            return fn(*inputs)
        if len(cache) >= self.max_graphs:
            cache.pop(next(iter(cache)))
        static = [t.clone() if torch.is_tensor(t) else t for t in inputs]
        torch.cuda.synchronize()
        g = cache[key] = _Graph(fn, static)
        return g.run(*inputs)

    @torch.no_grad()
    def mel(self, speaker, texts, p_control=1.0, e_control=1.0, d_control=1.0):
        """speaker (B,) int64, texts (B, L) int64 on the device -> (postnet mel (B, T, 80) fp32, mel_lens (B,))."""
        m = self.fs2
        m.eval()
        Bn, Lp = texts.shape
        src_lens = torch.full((Bn,), Lp, dtype=torch.int64, device=texts.device)
        ctl = (float(p_control), float(e_control), float(d_control))
        front = lambda spk, txt, sl: m.eval_front(spk, txt, sl, Lp, *ctl)
        kf = ("front", Bn, Lp) + ctl if Lp <= m.max_seq_len else None
        x3, dur, total, _ = self._get(self._front, kf, front, (speaker, texts, src_lens))
        T = max(int(total.max().item()), 1)                 # the path's one host read
        back = lambda x, dd: m.eval_back(x, dd, Lp, T)
        kb = ("back", Bn, Lp, T) if T <= m.max_seq_len else None
        mel, post, mel_lens, _ = self._get(self._back, kb, back, (x3, dur))
        # a replayed graph returns its private static buffers: hand out copies, or the caller's mel changes at the next call
        return post.clone(), mel_lens.clone()

    @torch.no_grad()
    def wav(self, mel_bct):
        """mel (B, 80, T) fp32 on the device -> waveform (B, 1, 256 T) fp32."""
        Bn, _, T = mel_bct.shape
        return self._get(self._voc, ("voc", Bn, T), lambda x: self.vocoder(x), (mel_bct.contiguous(),)).clone()

    @torch.no_grad()
    def wav_ragged(self, mels, frames_first=False, int16_scale=None):
        """mels: a list of (80, T_i) mels of any lengths (`frames_first`: (T_i, 80)) -> a list of (1, 1, 256 T_i) waveforms on the device,
        fp32, or int16 = truncation of waveform * `int16_scale`.  The utterances of at least `windows.W` frames run as N fixed-size
        windows (tts_king_amd/windows.py) on ONE graph per ladder value of N: gather -> generator -> stitch, with the mel staging buffer
        and the plan table as its static inputs, so calls with different lengths and the same N replay the same graph.  Shorter
        utterances go through `wav`, one at a time."""
        mels = list(mels)
        flat, plan, spf = self.wav_ragged_flat(mels, frames_first, int16_scale)
        flat = None if flat is None else flat.clone()          # the graph's private output buffer: hand out a copy, as `wav` does
        return windows.split(flat, plan, spf, self.vocoder.forward_short(mels, plan, frames_first, int16_scale, forward=self.wav))

    @torch.no_grad()
    def wav_ragged_flat(self, mels, frames_first=False, int16_scale=None):
        """The windowed part of `wav_ragged`: (flat buffer of N * W * 256 samples or None when no utterance fills a window, plan, samples
        per frame).  After a replay the buffer is the graph's own: valid until the next call with the same N."""
        gen = self.vocoder
        mels, lens = gen.ragged_mels(mels, frames_first)
        plan = windows.plan_windows(lens, windows.W, gen.halo())
        spf = gen.samples_per_frame()
        if not plan.planned:
            return None, plan, spf
        key = ("rag", plan.N, plan.W, bool(frames_first), None if int16_scale is None else float(int16_scale))
        table = torch.from_numpy(plan.table)
        g = self._rag.get(key)
        if g is None:
            stage = gen.stage_mels(mels, plan, frames_first)
            table = table.to(stage.device)
            fn = lambda st, tb: gen.forward_windows(st, tb, frames_first, int16_scale)
            if key not in self._seen:                      # first sight: eager (lazy allocations, weight packing)
                self._seen.add(key)
                return fn(stage, table), plan, spf
            if len(self._rag) >= self.max_graphs:
                self._rag.pop(next(iter(self._rag)))
            torch.cuda.synchronize()
            g = self._rag[key] = _Graph(fn, [stage, table])
        else:
            gen.stage_mels(mels, plan, frames_first, g.static[0])
            g.static[1].copy_(table, non_blocking=True)
        g.graph.replay()
        return g.out, plan, spf
