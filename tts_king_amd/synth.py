"""hipGraph-captured synthesis: text ids -> mel -> waveform with two host-visible steps.

reference path: tts_king.py:25-49 (`generate_mel` -> `mel_to_wav`), fsapi.py:38-82, hifiapi.py:40-52.  The reference
launches ~400 small ATen ops per utterance and syncs per phoneme in the LengthRegulator; here the path is three replayed
graphs: A = encoder + variance adaptor + duration totals (shape key: phonemes L, controls), then ONE host read of the
frame count T (the only data-dependent shape), B = LengthRegulator + decoder + PostNet (key: L, T), C = HiFi-GAN
generator (key: T; `wav_ragged`: the windowed generator, key: the number of windows N, whatever the lengths).  `mel_ragged` runs texts of
different lengths as one call on graphs keyed by shape buckets only (tts_king_amd/batching.py).  Graphs are cached per key (utterances of equal L and T replay the same graphs); a key's first call
runs eagerly once (warm-up: lazy allocations, weight packing) and is captured on the second.
"""
import torch

import numpy as np

from . import batching
from . import ops
from . import resample
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
    def __init__(self, fs2, vocoder=None, max_graphs=32, graphs=True, l_bucket=batching.L_BUCKET, t_bucket=batching.T_BUCKET):
        """`graphs=False`: the same kernels launched plainly, nothing captured (the facades' `hip_graph: false`)."""
        self.fs2, self.vocoder, self.max_graphs = fs2, vocoder, max_graphs
        self.graphs, self.l_bucket, self.t_bucket = graphs, int(l_bucket), int(t_bucket)
        self._front, self._back, self._voc, self._rag = {}, {}, {}, {}
        self._seen = set()

    def _get(self, cache, key, fn, inputs):
        """Eager on first sight of `key`, captured on the second, replayed afterwards."""
        if key is None or not self.graphs:      # not capturable (host-side position table for > max_seq_len), or graphs off: plain launches
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
        # "exact": T here is the frame count itself; `mel_ragged` keeps ("back", B, L_bucket, T_bucket) in the same cache, and the two graphs differ
        kb = ("back", Bn, Lp, T, "exact") if T <= m.max_seq_len else None
        mel, post, mel_lens, _ = self._get(self._back, kb, back, (x3, dur))
        # a replayed graph returns its private static buffers: hand out copies, or the caller's mel changes at the next call
        return post.clone(), mel_lens.clone()

    @torch.no_grad()
    def mel_ragged(self, speakers, texts, p_control=1.0, e_control=1.0, d_control=1.0, aux=False, durations=None, pitch=None, energy=None,
                   target_frames=None):
        """Texts of different lengths in one call, every utterance as the model gives it alone (not as the reference's padded batch
        gives it: DESIGN.md section 12).  speakers: one id or one per utterance; texts: a list of 1-D phoneme-id arrays; each control
        a scalar or one value per utterance.  -> (a list of (T_u, 80) fp32 postnet mels on the device, the frame counts [T_u]).
        The texts are padded to `l_bucket` phonemes and the frames to `t_bucket`, and the graph keys are ("front", B, L_bucket) and
        ("back", B, L_bucket, T_bucket): speakers, lengths and the control arrays are static inputs copied in before replay, so
        neither a new length nor a new control value captures anything.  One host read (the B frame totals).  An utterance whose
        text or predicted frame count exceeds max_seq_len leaves the batch for `mel`.  An utterance predicted to have no frame at all comes
        back as an empty (0, 80) mel with count 0 (`mel` returns one padding frame there, which is no frame of the utterance either); its
        decoder rows then attend over zero keys in the batched graph, and nothing reads what they produce.  `aux`: also a list of per-utterance dicts
        (logd, pitch, energy, dur over the utterance's own phonemes, mel = the pre-PostNet mel; None for an utterance that left the batch).

        Per-phoneme prosody: a control may also hold, per utterance, an array over its phonemes; `pitch`,
        `energy`, `durations` set explicit values (per utterance None, a scalar or an array with NaN = not set; a set value is used as
        is, no control on it) and `target_frames` a frame budget per utterance the durations are fitted to.  A call that uses any of
        this runs the front with the per-row kernels under ONE more key per shape, ("front", B, L_bucket, "rows"), every input a static
        device array; a call that uses none of it runs exactly what it ran before.  On that route the aux of an utterance whose frame
        count passes max_seq_len is filled too; a text of more than max_seq_len phonemes with per-phoneme inputs is refused."""
        m = self.fs2
        m.eval()
        rows = batching.as_id_rows(texts)
        Bn = len(rows)
        spk = batching.per_utterance(speakers.cpu().numpy() if torch.is_tensor(speakers) else speakers, Bn, "speakers", np.int64)
        if batching.wants_rows(Bn, (p_control, e_control, d_control), (pitch, energy, durations), target_frames):
            pros = batching.plan_prosody([len(r) for r in rows], p_control, e_control, d_control, pitch, energy, durations, target_frames)
            mels, lens, extra = [None] * Bn, [0] * Bn, ([None] * Bn if aux else None)
            self._ragged_rows(rows, spk, pros, list(range(Bn)), mels, lens, extra)
            return (mels, lens, extra) if aux else (mels, lens)
        ctl = [batching.per_utterance(c, Bn, n) for c, n in ((p_control, "p_control"), (e_control, "e_control"), (d_control, "d_control"))]
        mels, lens, extra = [None] * Bn, [0] * Bn, ([None] * Bn if aux else None)
        self._ragged(rows, spk, ctl, list(range(Bn)), mels, lens, extra)
        return (mels, lens, extra) if aux else (mels, lens)

    def _solo(self, rows, spk, ctl, i, mels, lens):
        dev = self.fs2.device
        post, ml = self.mel(torch.from_numpy(spk[i:i + 1]).to(dev), torch.from_numpy(rows[i][None]).to(dev), float(ctl[0][i]), float(ctl[1][i]),
                            float(ctl[2][i]))
        mels[i], lens[i] = post[0], int(post.shape[1])

    def _ragged(self, rows, spk, ctl, only, mels, lens, extra):
        m, dev = self.fs2, self.fs2.device
        plan = batching.plan_texts(rows, m.max_seq_len, self.l_bucket, only)
        for i in plan.solo:
            self._solo(rows, spk, ctl, i, mels, lens)
        if not plan.batch:
            return
        Bn, Lp = len(plan.batch), plan.L
        sel = np.asarray(plan.batch)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        inputs = (up(spk[sel]), up(plan.ids), up(plan.lens), up(ctl[0][sel]), up(ctl[1][sel]), up(ctl[2][sel]))
        front = lambda s, t, sl, pc, ec, dc: m.eval_front_ragged(s, t, sl, Lp, pc, ec, dc)
        x3, dur, total, (pitch, energy, logd) = self._get(self._front, plan.key, front, inputs)
        totals = total.cpu().tolist()                        # the path's one host read
        keep, over, T = batching.plan_frames(totals, m.max_seq_len, self.t_bucket)
        if over:            # a predicted frame count past the position table: those utterances alone, the others again as their own batch
            for r in over:
                self._solo(rows, spk, ctl, plan.batch[r], mels, lens)
            if keep:
                self._ragged(rows, spk, ctl, [plan.batch[r] for r in keep], mels, lens, extra)
            return
        back = lambda x, dd: m.eval_back_ragged(x, dd, Lp, T)
        mel_pre, post, _ = self._get(self._back, batching.back_key(Bn, Lp, T), back, (x3, dur))
        for r, i in enumerate(plan.batch):
            # slices of a replayed graph's private buffers: hand out copies
            n, Lu = max(totals[r], 0), int(plan.lens[r])
            mels[i], lens[i] = post[r, :n].clone(), n
            if extra is not None:
                extra[i] = {"logd": logd[r, :Lu].clone(), "pitch": pitch[r, :Lu].clone(), "energy": energy[r, :Lu].clone(),
                            "dur": dur.view(Bn, Lp)[r, :Lu].clone(), "mel": mel_pre[r, :n].clone()}

    def _ragged_rows(self, rows, spk, pros, only, mels, lens, extra):
        """`_ragged` on the per-phoneme front (`FastSpeech2.eval_front_rows`); the back half and its keys are `_ragged`'s."""
        m, dev = self.fs2, self.fs2.device
        plan = batching.plan_texts(rows, m.max_seq_len, self.l_bucket, only)
        for i in plan.solo:
            ctl = pros.plain(i)
            if ctl is None:
                raise ValueError("utterance %d has %d phonemes: per-phoneme prosody (arrays, explicit values, a frame budget) is limited to "
                                 "texts of at most max_seq_len = %d phonemes" % (i, len(rows[i]), m.max_seq_len))
            self._solo(rows, spk, [np.full((len(rows),), c, np.float32) for c in ctl], i, mels, lens)
        if not plan.batch:
            return
        Bn, Lp = len(plan.batch), plan.L
        sel = np.asarray(plan.batch)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        inputs = (up(spk[sel]), up(plan.ids), up(plan.lens)) + tuple(up(a) for a in pros.padded(plan.batch, Lp))
        front = lambda s, t, sl, *pr: m.eval_front_rows(s, t, sl, Lp, pr)
        x3, dur, total, (pitch, energy, logd) = self._get(self._front, batching.rows_key(Bn, Lp), front, inputs)
        totals = total.cpu().tolist()                        # the path's one host read
        keep, over, T = batching.plan_frames(totals, m.max_seq_len, self.t_bucket)

        def hand_out(i, r, post, mel_pre, n):
            Lu = int(plan.lens[r])
            mels[i], lens[i] = post[:n].clone(), n
            if extra is not None:
                extra[i] = {"logd": logd[r, :Lu].clone(), "pitch": pitch[r, :Lu].clone(), "energy": energy[r, :Lu].clone(),
                            "dur": dur.view(Bn, Lp)[r, :Lu].clone(), "mel": mel_pre[:n].clone()}

        if over:            # past the position table: this utterance's rows of the front, alone through `eval_back` with the exact T and a host-built table
            d = x3.shape[-1]
            for r in over:
                x3_r, dur_r = x3.view(Bn, Lp, d)[r].clone(), dur.view(Bn, Lp)[r:r + 1].clone()
                mel_pre, post, _, _ = m.eval_back(x3_r, dur_r, Lp, totals[r])
                hand_out(plan.batch[r], r, post[0], mel_pre[0], totals[r])
            if keep:        # the others again as their own batch (a smaller B: its own keys)
                self._ragged_rows(rows, spk, pros, [plan.batch[r] for r in keep], mels, lens, extra)
            return
        back = lambda x, dd: m.eval_back_ragged(x, dd, Lp, T)
        mel_pre, post, _ = self._get(self._back, batching.back_key(Bn, Lp, T), back, (x3, dur))
        for r, i in enumerate(plan.batch):
            hand_out(i, r, post[r], mel_pre[r], max(totals[r], 0))

    @torch.no_grad()
    def wav(self, mel_bct, sample_rate=None, int16_scale=None):
        """mel (B, 80, T) fp32 on the device -> waveform (B, 1, 256 T) fp32.  `sample_rate` (other than the vocoder's): every row
        resampled as an utterance of its own, (B, 1, ceil(256 T L / M)), by one more launch in the graph, whose key the rate joins;
        `int16_scale` (with such a rate only): that launch writes saturated int16."""
        Bn, _, T = mel_bct.shape
        gen = self.vocoder
        if gen.resampler(sample_rate) is None:
            if int16_scale is not None:
                raise ValueError("wav: int16_scale belongs to the resampling launch; at the vocoder's own rate convert with ops.to_int16")
            return self._get(self._voc, ("voc", Bn, T), lambda x: gen(x), (mel_bct.contiguous(),)).clone()
        sc = None if int16_scale is None else float(int16_scale)
        key = ("voc", Bn, T, int(sample_rate), sc)
        g = self._voc.get(key)
        # the B-row segment table is a constant of the key: uploaded until the graph exists, the graph's own copy afterwards
        segs = g.static[1] if g is not None else gen.row_segments(Bn, T * gen.samples_per_frame(), sample_rate)
        fn = lambda x, sgt: gen.resample_rows(gen(x), sample_rate, sc, sgt)
        return self._get(self._voc, key, fn, (mel_bct.contiguous(), segs)).clone()

    @torch.no_grad()
    def wav_ragged(self, mels, frames_first=False, int16_scale=None, sample_rate=None):
        """mels: a list of (80, T_i) mels of any lengths (`frames_first`: (T_i, 80)) -> a list of (1, 1, 256 T_i) waveforms on the device,
        fp32, or int16 = truncation of waveform * `int16_scale`.  The utterances of at least `windows.W` frames run as N fixed-size
        windows (tts_king_amd/windows.py) on ONE graph per ladder value of N: gather -> generator -> stitch, with the mel staging buffer
        and the plan table as its static inputs, so calls with different lengths and the same N replay the same graph.  An utterance
        shorter than a window is a row of the same batch (its length is one more number in the table; such calls share one graph per
        N of their own); only on a generator without `short_rows()` does it go through `wav`, alone.
        `sample_rate` (other than the vocoder's): waveforms of ceil(256 T_i L / M) samples; the resampling launch and its segment table
        join the graph, still one per (N, rate) whatever the lengths; int16 is then saturated."""
        mels = list(mels)
        flat, plan, spf = self.wav_ragged_flat(mels, frames_first, int16_scale, sample_rate)
        flat = None if flat is None else flat.clone()          # the graph's private output buffer: hand out a copy, as `wav` does
        short = self.vocoder.forward_short(mels, plan, frames_first, int16_scale, forward=self.wav, sample_rate=sample_rate)
        return resample.split(flat, plan, spf, short)

    @torch.no_grad()
    def wav_joined(self, mels, join, frames_first=False, int16_scale=None, sample_rate=None):
        """`Generator.forward_joined` on the ragged graph: gather -> generator -> stitch (-> resample) -> the two join launches, with the
        join table (`narrate.Join.table`, padded to the plan's N rows: an utterance has at least one window) as one more static
        input.  The key is `wav_ragged_flat`'s (N[, rate]) plus the join flag, the output type and the pause budget: the output
        buffer holds the flat buffer's samples plus lead and pauses rounded up to a whole number of N seconds, so that sentence
        lengths, pauses up to a second each, gains and settings are all data and capture nothing.  -> (out, info, bound) as
        `forward_joined`; after a replay both are the graph's own, valid until the next call with the same key.
        A call with an utterance outside the windowed batch (a generator without `short_rows()`) launches plainly."""
        gen = self.vocoder
        mels = list(mels)
        if len(join) != len(mels):
            raise ValueError("wav_joined: the join names %d utterances, the call has %d" % (len(join), len(mels)))
        m2, lens = gen.ragged_mels(mels, frames_first)
        plan = gen.plan(lens)
        if not self.graphs or not plan.planned or plan.short:
            return gen.forward_joined(mels, join, frames_first, int16_scale, sample_rate)
        spf = gen.samples_per_frame()
        rl = plan.has_short_rows
        sc = None if int16_scale is None else float(int16_scale)
        filt = gen.resampler(sample_rate)
        table = torch.from_numpy(plan.table)
        flat_cap, rate = plan.N * plan.W * spf, int(windows._get(gen.h, "sampling_rate"))
        extra = []
        if filt is not None:
            extra = [torch.from_numpy(gen.plan_resample(plan, filt).table)]
            flat_cap, rate = resample.out_bound(flat_cap, plan.N, filt.L, filt.M), int(sample_rate)
        unit = plan.N * rate
        budget = max(1, -(-join.pause_total() // unit)) * unit
        cap = flat_cap + budget
        jt = torch.from_numpy(join.table(*gen.join_spans(plan, spf, 0, {}), rows=plan.N))
        key = ("rag", plan.N, plan.W, bool(frames_first), None) + (("rows",) if rl else ()) + (("rate", rate) if filt is not None else ())
        key += ("join", sc, budget)
        g = self._rag.get(key)
        if g is None:
            stage = gen.stage_mels(m2, plan, frames_first)
            dev = stage.device
            if filt is None:
                fn = lambda st, tb, jn: ops.wav_join(gen.forward_windows(st, tb, frames_first, None, rl), jn, n_dst=cap, int16_scale=sc)
            else:
                fn = lambda st, tb, sgt, jn: ops.wav_join(gen.forward_windows(st, tb, frames_first, None, rl, sample_rate, sgt), jn, n_dst=cap,
                                                          int16_scale=sc)
            inputs = [stage, table.to(dev)] + [t.to(dev) for t in extra] + [jt.to(dev)]
            if key not in self._seen:                      # first sight: eager (lazy allocations, weight packing)
                self._seen.add(key)
                return fn(*inputs) + (cap,)
            if len(self._rag) >= self.max_graphs:
                self._rag.pop(next(iter(self._rag)))
            torch.cuda.synchronize()
            g = self._rag[key] = _Graph(fn, inputs)
        else:
            gen.stage_mels(m2, plan, frames_first, g.static[0])
            for dst, src in zip(g.static[1:], [table] + extra + [jt]):
                dst.copy_(src, non_blocking=True)
        g.graph.replay()
        return g.out + (cap,)

    @torch.no_grad()
    def wav_ragged_flat(self, mels, frames_first=False, int16_scale=None, sample_rate=None):
        """The windowed part of `wav_ragged`: (flat buffer of N * W * 256 samples or None when no utterance fills a window, plan, samples
        per frame).  After a replay the buffer is the graph's own: valid until the next call with the same N.
        `sample_rate` (other than the vocoder's): the buffer holds ceil(N W 256 L / M) + N samples, the resampled utterances where
        `plan.segs` puts them (`resample.split`); the segment table is the graph's third static input, refreshed like the plan table."""
        gen = self.vocoder
        mels, lens = gen.ragged_mels(mels, frames_first)
        plan = gen.plan(lens)
        spf = gen.samples_per_frame()
        if not plan.planned:
            return None, plan, spf
        # short rows: the same N on the kernels that read each row's length from the table (a call of full windows keeps its own graph)
        rl = plan.has_short_rows
        key = ("rag", plan.N, plan.W, bool(frames_first), None if int16_scale is None else float(int16_scale)) + (("rows",) if rl else ())
        table = torch.from_numpy(plan.table)
        filt = gen.resampler(sample_rate)
        if filt is not None:
            key += ("rate", int(sample_rate))
            sg = gen.plan_resample(plan, filt)
            segs = torch.from_numpy(sg.table)
        g = self._rag.get(key)
        if g is None:
            stage = gen.stage_mels(mels, plan, frames_first)
            table = table.to(stage.device)
            if filt is None:
                fn, inputs = (lambda st, tb: gen.forward_windows(st, tb, frames_first, int16_scale, rl)), [stage, table]
            else:
                fn = lambda st, tb, sgt: gen.forward_windows(st, tb, frames_first, int16_scale, rl, sample_rate, sgt)
                inputs = [stage, table, segs.to(stage.device)]
            if key not in self._seen:                      # first sight: eager (lazy allocations, weight packing)
                self._seen.add(key)
                return fn(*inputs), plan, spf
            if len(self._rag) >= self.max_graphs:
                self._rag.pop(next(iter(self._rag)))
            torch.cuda.synchronize()
            g = self._rag[key] = _Graph(fn, inputs)
        else:
            gen.stage_mels(mels, plan, frames_first, g.static[0])
            g.static[1].copy_(table, non_blocking=True)
            if filt is not None:
                g.static[2].copy_(segs, non_blocking=True)
        g.graph.replay()
        return g.out, plan, spf
