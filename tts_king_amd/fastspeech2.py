"""FastSpeech2 on MI355X: the reference's module surface (`FastSpeech2(preprocess_config, model_config, n_speakers)`,
`forward(...) -> 12-tuple`, reference `state_dict` keys) over hand-written gfx950 kernels.

reference: fs_two/model/fastspeech2.py:12-119 (model graph), fs_two/transformer/Models.py (Encoder/Decoder),
Layers.py (FFTBlock, PostNet), SubLayers.py (MHA, FFN), model/modules.py (VarianceAdaptor, LengthRegulator,
VariancePredictor).  Every numbered step of `_forward` / `_backward` cites the lines it restates.

Forward AND backward are explicit sequences of kernel launches on the current HIP stream (no autograd graph
inside): activations are bf16 channels-last [B*T][C], accumulation is fp32, parameters are fp32 masters in one
flat buffer with a bf16 shadow.  `torch.autograd` only sees one node (`_Bridge`) so that the reference's
`loss.backward()` call site keeps working.
"""
import json
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import fs2_plan
from . import ops
from . import params as P
from . import switches
from .ops import bf16

N_VOCAB = 207  # len(symbols) + 1 — reference: fs_two/transformer/Models.py:40, fs_two/text/symbols.py


class _Saved(namedtuple("_Saved", "pre x qkv probs o z1 mean1 rstd1 x1 h z2 mean2 rstd2 Bn S lens H p site o32")):
    """What a block's forward keeps for its backward: twenty fields, and beside them the attribute `plan`, the block's
    fs2_plan.Block, so that the backward reads which kernels the forward ran instead of guessing it from the tensors."""


def sinusoid_table(n_position, d_hid):
    """reference: fs_two/transformer/Models.py:10-30 (float64, cast to fp32)."""
    pos = torch.arange(n_position, dtype=torch.float64)[:, None]
    j = torch.arange(d_hid)[None, :]
    angle = pos / torch.pow(torch.tensor(10000.0, dtype=torch.float64), 2.0 * (j // 2).double() / d_hid)
    tab = torch.empty_like(angle)
    tab[:, 0::2] = torch.sin(angle[:, 0::2])
    tab[:, 1::2] = torch.cos(angle[:, 1::2])
    return tab.float()


def get_speakers_number(preprocess_config):
    """reference: fs_two/model/fastspeech2.py:122-137."""
    path = os.path.join(preprocess_config["path"]["preprocessed_path"], "speakers.json")
    if not os.path.exists(path):
        raise Exception("Model is multispeaker but number of speakers was not provided explicitly")
    with open(path) as f:
        return len(json.load(f))


class _Bridge(torch.autograd.Function):
    """The single autograd node: forwards the natively computed outputs, routes their gradients into the native
    backward, which accumulates into the flat gradient buffer (the `.grad` views of the parameters)."""

    @staticmethod
    def forward(ctx, anchor, model, mel, post, pitch, energy, logd, *heads):
        # `heads` (CWT branch only): the (B, 1) pitch_mean / pitch_std predictions
        ctx.model = model
        ctx.step_ctx = model._ctx
        return (mel.view_as(mel), post.view_as(post), pitch.view_as(pitch), energy.view_as(energy), logd.view_as(logd)) + \
            tuple(h.view_as(h) for h in heads)

    @staticmethod
    def backward(ctx, dmel, dpost, dpitch, denergy, dlogd, *dheads):
        ctx.model._backward_from_autograd(ctx.step_ctx, dmel, dpost, dpitch, denergy, dlogd, *dheads)
        return (None,) * (7 + len(dheads))


class _Ctx:
    """Activations kept for the backward of one step."""
    pass


class _GroupNotifier:
    """backward_native's contract with a data-parallel reducer: `done(name)` is called when every gradient of parameter group
    `name` has been ENQUEUED OR QUEUED; the queued part (grouped dW GEMMs, deferred reducers) must be flushed before the reducer
    may all-reduce the bucket.  Flushing at every group would cut the step's single grouped weight-gradient launch into 13; the
    notifier asks the reducer (`ready(name)`) whether a bucket actually completes with this group and only then flushes and
    announces.  Groups must arrive in `order` (checked: a reordering of backward would silently break the overlap contract)."""

    def __init__(self, order, on_bucket, flush, mark=None):
        self.order, self.on_bucket, self.flush = list(order), on_bucket, flush
        self.ready = getattr(getattr(on_bucket, "__self__", None), "ready", None)
        self.pos = 0
        self.flushes = 0
        # `mark(name)` (the "side" / "late" schedules): instead of flushing and announcing now, the caller notes the group and does
        # both later (FastSpeech2._launch_dw_side_buckets / the end of backward_native)
        self.mark = mark

    def done(self, name):
        if self.pos >= len(self.order) or self.order[self.pos] != name:
            raise RuntimeError("backward announced group %r, expected %r" % (name, self.order[self.pos] if self.pos < len(self.order) else None))
        self.pos += 1
        if self.on_bucket is None:
            return
        if self.mark is not None:
            self.mark(name)
            return
        if self.ready is not None and not self.ready(name):
            return                      # no gradient bucket completes with this group: keep queueing
        self.flush()
        self.flushes += 1
        self.on_bucket(name)


class FastSpeech2(nn.Module):
    def __init__(self, preprocess_config, model_config, n_speakers=None, device=None, seed=1234):
        super().__init__()
        self.model_config = model_config
        self.preprocess_config = preprocess_config
        if not model_config["multi_speaker"]:
            # reference: fastspeech2.py:72-88 raises NameError on this path; only multi-speaker works there too
            raise NotImplementedError("multi_speaker: False is not a working path in the reference either")
        # CWT pitch (modules.py:26-36,104-130): the pitch predictor has 11 outputs and a dropout of its own (0.1 by its constructor call,
        # whatever variance_predictor.dropout says), the pitch_mean / pitch_std heads compute, the embedding row comes from the
        # PREDICTED coefficients in training too
        self.use_cwt = bool(model_config["use_cwt"])
        self.p_pitch = 0.1
        if n_speakers is None:
            n_speakers = get_speakers_number(preprocess_config)
        if device is None or device == "gpu":
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        if isinstance(device, int):
            device = "cuda:%d" % device
        device = torch.device(device)
        tr = model_config["transformer"]
        self.d = tr["encoder_hidden"]
        self.d_ff = tr["conv_filter_size"]
        self.k1, self.k2 = tr["conv_kernel_size"]
        self.n_head_enc, self.n_head_dec = tr["encoder_head"], tr["decoder_head"]
        self.n_enc, self.n_dec = tr["encoder_layer"], tr["decoder_layer"]
        self.p_enc, self.p_dec = float(tr["encoder_dropout"]), float(tr["decoder_dropout"])
        self.p_var = float(model_config["variance_predictor"]["dropout"])
        self.k_var = model_config["variance_predictor"]["kernel_size"]
        self.p_post = 0.5                                                       # hard-coded in Layers.py:137-141
        self.max_seq_len = model_config["max_seq_len"]
        self.n_mel = preprocess_config["preprocessing"]["mel"]["n_mel_channels"]
        self.n_speakers = n_speakers

        # (raises params.ConfigError, naming the key, for every configuration the kernels have no instance for: params.validate_config)
        entries = P.build_entries(model_config, self.n_mel, n_speakers, N_VOCAB)
        self._table, self._n_flat = P.layout(entries)
        self._flat = torch.zeros(self._n_flat, dtype=torch.float32, device=device)
        self._flat_grad = torch.zeros(self._n_flat, dtype=torch.float32, device=device)
        self._shadow = torch.zeros(self._n_flat, dtype=bf16, device=device)
        self._shadow_version = -1
        self._anchor = torch.zeros((), requires_grad=True)
        self._ctx = None
        self._deferred = None           # the step's ops.DeferQueue: weight-gradient problems and split-K slabs awaiting their launches (backward only)
        self._deferred_fin = None       # gradient column-sum partials awaiting the batched finalize
        # The five kernel toggles (properties, below the class; DESIGN.md 7.2 says what each decides): which kernel runs which site
        # follows from them and the dimensions in ONE place, fs2_plan.build_plan; `self.plan` is that record.  The window kernel
        # (csrc/ffn_conv.hip) wants its weights in MFMA-fragment order: `_w1_packed` holds such copies of the weights the plan routes
        # there — for an input gradient the transposed, tap-flipped weight — all rewritten by ONE launch whenever the bf16 shadow is.
        self._toggles = {"window_ffn": switches.get("TTSK_WINDOW_FFN") != "0", "flash_attention": True, "fused_ln": True,
                         "postnet_ends_win": True, "dwconv": switches.get("TTSK_DWCONV") != "0"}
        self._dims = fs2_plan.dims_of(model_config, self.n_mel)
        self._plan_cache = None         # (the packs, their tables and the optimizer's Adam items: _build_packs, at the end of this)
        # Speaker adaptation (set_trainable): the units that are trained, None = all of them
        self._trainable = None
        self._optimizer_built = False
        # the optimizer step's device tables over the trainable ranges of the flat buffer (ops.optim_tables; None on the CPU), and what
        # refresh_after_step has to do behind it (_build_optim_tables)
        self._optim_tables = None
        self._repack_after_step = False
        self._odd_after_step = None
        self.group_predictors = not self.use_cwt    # training with targets: the three VariancePredictors run as grouped launches (the CWT
                                                    # branch picks its pitch embedding from the prediction: sequential by construction)
        # The weight-gradient GEMMs of PostNet + decoder (88 % of the step's dW FLOPs) are complete once the decoder's backward is;
        # what follows on the dX path (length regulator, variance adaptor, encoder: ~0.5 ms of 32-128-workgroup kernels) fills a
        # fraction of the chip.  So that group is launched there on a second stream with its grid capped at `dw_side_wgs` workgroups
        # (one per CU: the other CUs stay free for the dX chain) and joined before the optimizer.  0 = launch it at the end instead.
        self.dw_side_wgs = int(switches.get("TTSK_DW_SIDE_WGS"))
        # ... and only `dw_side_frac` of that group's FLOPs go there: the dX chain that runs beside it is shorter (0.39 ms) than the
        # capped group (0.57 ms), the rest joins the encoder-side group that runs on the whole chip once the dX chain is done
        # (measured: 1.0 -> 3.03 ms/step, 0.85 / 0.75 -> 3.00, 0.65 -> 3.02, 0.55 -> 3.11)
        # (round 3: w_1's gradients left the grouped queue for csrc/dwconv.hip, which runs first on that stream: re-measured below)
        self.dw_side_frac = float(switches.get("TTSK_DW_SIDE_FRAC"))
        self._dw_side = None
        self._dw_side_pending = False
        # Data-parallel schedule (backward_native(on_bucket=...)), TTSK_DP_SCHEDULE:
        #   "side"  (default) the single-GPU schedule kept: nothing is flushed during the PostNet / decoder backward; after it the queued
        #           weight-gradient work runs on the second stream (capped grid, its split-K reducer behind it) and the all-reduces of
        #           the buckets it completes are issued from there, beside the encoder-side dX chain; the rest after the chain;
        #   "late"  the single-GPU schedule untouched, every all-reduce after the last flush (no overlap with backward).
        # (Round 2's "early" schedule — a flush on the main stream whenever a bucket completes — measured 22 % more compute per step and
        # was deleted in round 4; without a second stream, dw_side_wgs = 0, buckets are still flushed one by one as they complete.)
        self.dp_schedule = switches.get("TTSK_DP_SCHEDULE")
        self._fin_side = None
        # Training with targets: the three VariancePredictors' outputs feed nothing but the loss (the embeddings are picked by the TARGET
        # pitch / energy, the length regulator takes the TARGET durations: modules.py:158-205), and their backward needs nothing but the
        # loss's gradients until its last step.  Both run on a stream of their own: the forward beside the decoder's first block, the
        # backward beside the PostNet's — 1,024-row kernels of 96 workgroups that the 212-256-workgroup chain kernels leave room for.
        self.pred_side = switches.get("TTSK_PRED_SIDE")     # "1" both, "f" forward only, "b" backward only, "0" neither
        self._pred_stream = None
        self._pred_fwd_pending = False
        self._var_on_pred = False           # the loss was taken in two halves (graph.make_enqueue): the variance gradients live on the predictors' stream
        self._loss_finalize = None          # ... and this makes the loss values, on a stream that has waited for both halves (backward_native)
        self.split_loss = True              # training steps built by graph.make_enqueue take the loss that way when the predictors have their stream
        # Does the flat gradient buffer hold an unfinished accumulation (micro-steps of a grad_acc_step cycle)?  False after an optimizer
        # update or zero_grad(): the next backward then overwrites instead of accumulating (see backward_native).
        self.grads_partial = False
        self._acc = True
        self._rng_state = None          # device block shared with the optimizer (ops.optim_state)
        self._seed = seed
        self._modules_by_key = {}
        for en in entries:
            self._register(en, device)
        self._init_constants(preprocess_config, model_config)
        self.reset_parameters(seed)
        # the three predictors sit back to back in the flat buffer with identical internal layouts: constant stride
        va = "variance_adaptor."
        o = [self._table[va + n + "_predictor.conv_layer.conv1d_1.conv.weight"].offset for n in ("duration", "pitch", "energy")]
        self._pred_stride = o[1] - o[0]
        if self.use_cwt:
            self._pred_stride = None        # the 11-output pitch predictor is longer than its neighbours: no grouped launches
            hm = [self._table[va + "pitch_mean." + k].offset for k in
                  ("flat_one.net.0.weight", "flat_one.net.0.bias", "flat_one.net.2.weight", "flat_one.net.2.bias", "flat_two.net.0.weight",
                   "flat_two.net.0.bias", "flat_two.net.2.weight", "flat_two.net.2.bias", "linear.weight", "linear.bias")]
            assert tuple(h - hm[0] for h in hm) == ops.CNNSCALAR_OFFSETS, "CNNscalar block layout (include/ttsk.h)"
            assert self._table[va + "pitch_std.flat_one.net.0.weight"].offset - hm[0] == ops.CNNSCALAR_FLOATS
        else:
            assert o[2] - o[1] == self._pred_stride and self._pred_stride % 8 == 0
        self._build_packs()

    # ------------------------------------------------------------------ parameter plumbing
    def _register(self, en, device):
        mod = self
        parts = en.key.split(".")
        for name in parts[:-1]:
            if name not in mod._modules:
                mod.add_module(name, nn.Module())
            mod = mod._modules[name]
        leaf = parts[-1]
        if en.kind == P.TRAIN:
            par = nn.Parameter(self._view(self._flat, en), requires_grad=True)
            par.grad = self._view(self._flat_grad, en)
            mod.register_parameter(leaf, par)
        elif en.kind in (P.FROZEN, P.UNUSED):
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(en.shape, device=device), requires_grad=en.kind == P.UNUSED))
        else:
            dt = torch.int64 if en.dtype == "int64" else torch.float32
            mod.register_buffer(leaf, torch.zeros(en.shape, dtype=dt, device=device))
        self._modules_by_key[en.key] = (mod, leaf)

    @staticmethod
    def _view(flat, en):
        v = flat[en.offset:en.offset + en.numel].view(en.storage_shape)
        return v.permute(0, 2, 1) if en.conv else v

    def _rebind(self):
        """After the flat buffers moved (`.to()`, `.cuda()`): new Parameters over the new views.  `par.data = view` would keep
        the parameter's OWN version counter, so a later `load_state_dict` / `param.copy_()` would no longer bump
        `_flat._version` and the bf16 shadow would go stale; a Parameter built from a view shares the buffer's counter."""
        for en in self._table.values():
            if en.kind == P.TRAIN:
                mod, leaf = self._modules_by_key[en.key]
                par = nn.Parameter(self._view(self._flat, en), requires_grad=True)
                par.grad = self._view(self._flat_grad, en)
                mod._parameters[leaf] = par
        self._shadow_version = -1
        self._apply_trainable_flags()

    # ------------------------------------------------------------------ trainable units (speaker adaptation)
    def set_trainable(self, units=None):
        """Train only the parameter groups `units` and freeze the rest (torch: `requires_grad_(False)` on the rest).  Units:
        `params.unit_names` — postnet, mel_linear, decoder.0 .., variance_adaptor, speaker_emb, encoder.0 .., embedding; the prefixes
        "decoder" / "encoder" name every block of the stack.  None, or every unit: today's path, unchanged.  A frozen unit gets no
        parameter-gradient work in backward_native, input gradients stop at the lowest trainable unit, and the optimizer's clip / Adam
        cover the trainable ranges only.  "Frozen" covers parameters: in train mode BatchNorm still takes batch statistics and moves
        its running ones, and dropout still runs.  Must be called before a ScheduledOptim is built on the model."""
        if self._optimizer_built:
            raise RuntimeError("set_trainable must be called before a ScheduledOptim is built on the model (its Adam state, tables and "
                               "checkpoint layout follow the trainable units)")
        tu = P.parse_units(units, self.n_enc, self.n_dec)
        if tu is not None and self.use_cwt:
            raise NotImplementedError("train_only together with use_cwt: True is not supported")
        self._trainable = tu
        self._apply_trainable_flags()
        self._build_optim_tables()

    @property
    def trainable_units(self):
        """The trainable units in backward order, or None when everything is trained."""
        if self._trainable is None:
            return None
        return tuple(u for u in P.unit_names(self.n_enc, self.n_dec) if u in self._trainable)

    def trainable_ranges(self):
        """Sorted [start, end) ranges of the flat buffers the optimizer updates: cut at entry boundaries (each entry's padding to 8
        floats included), adjacent ones merged.  Everything trainable: [(0, n_flat)]."""
        return P.unit_ranges(self._table, self._n_flat, self._trainable)

    def trainable_keys(self):
        """state_dict keys of the parameters that are trained."""
        return [k for k, en in self._table.items() if en.kind == P.TRAIN and self._unit_on(P.unit_of(k))]

    def _unit_on(self, unit):
        return self._trainable is None or unit in self._trainable

    def _apply_trainable_flags(self):
        """requires_grad / .grad of the parameters as the trainable units say (a frozen parameter has no .grad: its stretch of the
        flat gradient buffer is never written to a defined value)."""
        for en in self._table.values():
            if en.kind == P.TRAIN:
                par = self.get(en.key)
                on = self._unit_on(P.unit_of(en.key))
                par.requires_grad_(on)
                par.grad = self._view(self._flat_grad, en) if on else None

    def _build_optim_tables(self, adam_writes_packs=True):
        """The optimizer step's device tables (host -> device copies: at construction, set_trainable, `_apply` and a toggle that
        changes `plan.packs`, never inside a step): the trainable ranges of the flat buffer — everything trained: one range — and the
        trainable packed weights as the Adam launch's items (their packs are written there, the frozen weights' packs are left alone).
        The trainable 80-channel ends, which that launch cannot write, get a pack table of their own.  When the items cannot be used —
        a packed weight that does not tile, one with two packs of a kind, or `adam_writes_packs` False (tests: the same step with
        the pack launch behind it) — Adam walks the plain ranges and every pack is rewritten from the shadow afterwards."""
        self._optim_tables, self._repack_after_step, self._odd_after_step = None, False, None
        if not self._flat.is_cuda:
            return
        dev, ranges, tables = self._flat.device, self.trainable_ranges(), None
        packed = bool(self.plan.packs)
        if packed and adam_writes_packs and self._adam_items is not None:
            tables = ops.optim_tables(ranges, [tuple(v) for k, v in self._adam_items.items() if self._unit_on(P.unit_of(k))], dev)
        if tables is None:
            tables, self._repack_after_step = ops.optim_tables(ranges, [], dev), packed
        self._optim_tables = tables
        if packed and not self._repack_after_step:
            odd = [(W, pk, tr) for key, W, pk, tr in self._odd_items if self._unit_on(P.unit_of(key))]
            if len(odd) == len(self._odd_items):
                self._odd_after_step = self._odd_pack_table
            elif odd:
                self._odd_after_step = ops.win_conv_pack_table(odd, dev)

    def refresh_after_step(self):
        """Behind the optimizer step, which rewrote the bf16 shadow: the window kernels' packs that step did not write itself — every
        pack when its Adam launch had no items, else the trainable 80-channel ends in one small launch (_build_optim_tables: neither
        when the plan has no packs)."""
        if self._repack_after_step:
            self.refresh_packed()
        elif self._odd_after_step is not None:
            ops.win_conv_pack_run(*self._odd_after_step)

    def mark_dirty(self):
        """Call after writing the fp32 masters through anything torch cannot see (raw pointers): the next forward
        refreshes the bf16 shadow."""
        self._shadow_version = -1

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._shadow_version = -1
        return out

    def _apply(self, fn, recurse=True):
        flat, grad, shadow = fn(self._flat), fn(self._flat_grad), fn(self._shadow)
        if flat.dtype != torch.float32:
            raise TypeError("FastSpeech2 masters stay fp32 (bf16 shadows are managed internally)")
        super()._apply(fn, recurse)
        self._flat, self._flat_grad = flat, grad
        self._shadow = shadow.to(bf16) if shadow.dtype != bf16 else shadow
        self._rng_state = None
        self._dw_side = self._fin_side = self._pred_stream = None
        self._rebind()
        self._build_packs()
        return self

    def get(self, key):
        mod, leaf = self._modules_by_key[key]
        return mod._parameters[leaf] if leaf in mod._parameters else mod._buffers[leaf]

    def _init_constants(self, pc, mc):
        tab = sinusoid_table(mc["max_seq_len"] + 1, self.d)[None]
        with open(os.path.join(pc["path"]["preprocessed_path"], "stats.json")) as f:     # modules.py:55-60
            stats = json.load(f)
        nb = mc["variance_embedding"]["n_bins"]
        ve = mc["variance_embedding"]
        with torch.no_grad():
            self.get("encoder.position_enc").copy_(tab)
            self.get("decoder.position_enc").copy_(tab)
            for name, key in (("pitch", "pitch_bins"), ("energy", "energy_bins")):
                lo, hi = stats[name][:2]
                if ve[name + "_quantization"] == "log":
                    import numpy as np
                    bins = torch.exp(torch.linspace(np.log(lo), np.log(hi), nb - 1))
                else:
                    bins = torch.linspace(lo, hi, nb - 1)
                self.get("variance_adaptor." + key).copy_(bins)
            for i in range(5):
                self.get("postnet.convolutions.%d.1.running_var" % i).fill_(1.0)

    def reset_parameters(self, seed=1234):
        """Seeded random init (weights_path: null).  Statistics follow tts_king_amd.synthetic.seeded_fill;
        the PAD row of the phoneme embedding is zero as in nn.Embedding(padding_idx=0)."""
        from .synthetic import seeded_fill
        sd = {k: v for k, v in self.state_dict().items()}
        cpu = {k: torch.zeros(v.shape, dtype=v.dtype) for k, v in sd.items()}
        for k, v in sd.items():
            if any(s in k for s in ("position_enc", "_bins", "running_", "num_batches")):
                cpu[k] = v.detach().cpu().clone()
        seeded_fill(cpu, seed)
        cpu["encoder.src_word_emb.weight"][0].zero_()
        with torch.no_grad():
            for k, v in sd.items():
                if not any(s in k for s in ("position_enc", "_bins", "running_", "num_batches")):
                    v.copy_(cpu[k])

    @property
    def device(self):
        return self._flat.device

    def flat_buffers(self):
        """(params fp32, grads fp32, bf16 shadow): the trainable state as three flat tensors."""
        return self._flat, self._flat_grad, self._shadow

    def grad_buckets(self, bucket_mb=24):
        return P.buckets(self._table, self._n_flat, int(bucket_mb * (1 << 20) / 4))

    def group_offsets(self):
        """name -> lowest flat offset of the parameter group announced by backward_native(on_bucket=...)."""
        def lo(prefixes):
            return min(en.offset for k, en in self._table.items() if en.kind == P.TRAIN and k.startswith(prefixes))
        g = {"postnet": lo(("postnet.",)), "mel_linear": lo(("mel_linear.",)),
             "variance_adaptor": lo(("variance_adaptor.", "speaker_emb.")), "embedding": 0}
        for i in range(self.n_dec):
            g["decoder.%d" % i] = lo(("decoder.layer_stack.%d." % i,))
        for i in range(self.n_enc):
            g["encoder.%d" % i] = lo(("encoder.layer_stack.%d." % i,))
        return g

    def attach_state(self, state):
        """Share the optimizer's device state block (dropout counters live in it)."""
        self._rng_state = state

    def _state(self):
        if self._rng_state is None:
            self._rng_state = ops.optim_state(self.device, seed=self._seed)
        return self._rng_state

    def sync_shadow(self, force=False):
        """bf16 copies of the masters, refreshed when anything wrote to them through torch (load_state_dict, init)."""
        if force or self._shadow_version != self._flat._version:
            ops.cast_bf16(self._flat, self._shadow)
            self._shadow_version = self._flat._version
            self.refresh_packed()

    @property
    def plan(self):
        """fs2_plan.build_plan for this model as it is toggled now: rebuilt after a toggle changed, the same object otherwise.  Needs no device."""
        if self._plan_cache is None:
            self._plan_cache = fs2_plan.build_plan(self._dims, fs2_plan.Toggles(**self._toggles))
        return self._plan_cache

    def _set_toggle(self, name, on):
        """A toggle drops the cached plan; one that changes `plan.packs` rebuilds the packs and the optimizer's tables at once (host ->
        device copies: a toggle is set between steps, never inside one)."""
        if bool(on) != self._toggles[name]:
            self._toggles[name] = bool(on)
            self._plan_cache = None
            if self._shadow.is_cuda and self.plan.packs != self._planned_packs:
                self._build_packs()

    def routes(self):
        """The plan's route names per site as plain lists (fs2_plan.routes): {"encoder" / "decoder": {site: [per block]}, "postnet":
        {site: [per layer]}, "mel_linear": {"train", "eval", "dx"}}."""
        return fs2_plan.routes(self.plan)

    def refresh_packed(self):
        """Rewrite the fragment-major weight copies the window conv kernel reads (csrc/ffn_conv.hip) from the bf16 shadow — one launch
        over a device-resident item table.  Called by everything that writes the shadow: `sync_shadow` and
        `ScheduledOptim.step_and_update_lr`."""
        if self._pack_table is not None:
            ops.win_conv_pack_run(*self._pack_table)
        if self._odd_pack_table is not None:       # the PostNet's 80-channel ends: one small launch
            ops.win_conv_pack_run(*self._odd_pack_table)

    def _build_packs(self):
        """Allocate the packs and their item table (host -> device copy: not capturable, so this runs at construction and after
        `_apply` and from a toggle's setter, never inside a forward): exactly `plan.packs`, none on the CPU.  The odd ones -- the PostNet's
        ends and mel_linear, 80 channels: neither a multiple of 32 storage rows nor of 256 storage columns -- Adam's tile walk cannot
        write; they get one small launch of their own behind the optimizer step (refresh_after_step).  The packs are empty until the
        next `sync_shadow`, which this asks for."""
        dev = self._shadow.device
        self._planned_packs = self.plan.packs if self._shadow.is_cuda else ()
        main = [p for p in self._planned_packs if not p.odd]
        buf = torch.empty(sum(self.pack_numel(p) for p in main), dtype=bf16, device=dev)
        self._w1_packed, self._pack_items, self._odd_items, off = {} if self._planned_packs else None, [], [], 0
        for p in main:
            n = self.pack_numel(p)
            self._w1_packed[(p.tag, p.key)] = buf[off:off + n]
            self._pack_items.append((p.key, p.fused_rows, buf[off:off + n], p.transpose))
            off += n
        for p in self._planned_packs:
            if p.odd:
                pk = torch.empty(self.pack_numel(p), dtype=bf16, device=dev)
                self._w1_packed[(p.tag, p.key)] = pk
                self._odd_items.append((p.key, self._pack_source(p.key), pk, p.transpose))
        # the shadow views and the packs keep their addresses until _apply: a device-resident item table, one pack launch per step
        self._pack_table = ops.win_conv_pack_table([(self._pack_source(key, fr), out, tr) for key, fr, out, tr in self._pack_items],
                                                   dev) if self._pack_items else None
        self._odd_pack_table = ops.win_conv_pack_table([(W, pk, tr) for _, W, pk, tr in self._odd_items], dev) if self._odd_items else None
        # ... and the items with which the optimizer's Adam launch writes these packs itself (ttsk_optim_step): per weight its flat
        # offset, storage shape and its plain / transposed packs.  A weight with more than one pack of a kind (w_1's transposed pack
        # exists once) leaves `_adam_items` None: every pack is then rewritten behind the step (_build_optim_tables).
        self._adam_items = None
        if self._pack_items:
            by_key, ok = {}, True
            for key, fr, out, tr in self._pack_items:
                W = self._pack_source(key, fr)
                ent = by_key.setdefault(key, [self._table[key].offset, tuple(W.shape), None, None])
                if ent[1] != tuple(W.shape) or ent[3 if tr else 2] is not None:
                    ok = False
                ent[3 if tr else 2] = out
            if ok:
                self._adam_items = by_key
        self._shadow_version = -1
        self._build_optim_tables()

    def pack_numel(self, p):
        """Elements of pack `p` (an fs2_plan.Pack), from the parameter table alone."""
        en = self._table[p.key]
        cs, k, ds = en.storage_shape if en.conv else (p.fused_rows or en.shape[0], 1, en.shape[1])
        return ops.win_pack_numel(cs, k, ds, p.transpose) if p.odd else cs * k * ds

    def _pack(self, tag, key):
        """The window kernel's pack `(tag, key)`: a route of the plan that reads a pack finds it here, or the packs are not the plan's."""
        if self._w1_packed is None or (tag, key) not in self._w1_packed:
            raise ops.L.TtskError("the plan routes %s to the window kernel, but its pack %r is missing" % (key, tag))
        return self._w1_packed[(tag, key)]

    def _pack_source(self, key, fused_rows=None):
        """The tap-major bf16 shadow of `key` as a (Cs, k, Ds) tensor (a Linear weight is k = 1; `fused_rows`: the q|k|v rows as one)."""
        W = self._w(key, fused_rows) if fused_rows is not None else self._w(key)
        return W.view(W.shape[0], 1, W.shape[1]) if W.dim() == 2 else W

    # views into the flat buffers ------------------------------------------------------------------
    def _w(self, key, rows=None):
        """bf16 shadow of a weight as a 2-D/3-D tensor in STORAGE layout; `rows` widens it over the following
        keys (fused q|k|v)."""
        en = self._table[key]
        shp = en.storage_shape
        if rows is not None:
            return self._shadow[en.offset:en.offset + rows * shp[1]].view(rows, shp[1])
        return self._shadow[en.offset:en.offset + en.numel].view(shp)

    def _m(self, key, n=None):
        """fp32 master (vectors / tables) — `n` widens over the following keys."""
        en = self._table[key]
        if n is not None:
            return self._flat[en.offset:en.offset + n]
        return self._flat[en.offset:en.offset + en.numel].view(en.storage_shape)

    def _g(self, key, n=None):
        en = self._table[key]
        if n is not None:
            return self._flat_grad[en.offset:en.offset + n]
        return self._flat_grad[en.offset:en.offset + en.numel].view(en.storage_shape)

    # ------------------------------------------------------------------ forward
    def forward(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
                e_targets=None, d_targets=None, pitches_raw=None, pitches_cwt=None, pitches_mean=None,
                pitches_std=None, p_control=1.0, e_control=1.0, d_control=1.0):
        """reference: fs_two/model/fastspeech2.py:43-119.  Same arguments, same 12-tuple."""
        if not self._flat.is_cuda:
            raise ops.L.TtskError("FastSpeech2.forward needs the model on a HIP device (gpu: 'cuda:0'); there is no CPU path")
        train = self.training
        dev = self.device
        speakers, texts = speakers.to(dev).long().contiguous(), texts.to(dev).long().contiguous()
        src_lens = src_lens.to(dev).long().contiguous()
        with torch.no_grad():
            out, ctx = self._forward(train, speakers, texts, src_lens, int(max_src_len), mel_lens, max_mel_len, e_targets,
                                     d_targets, pitches_raw, float(p_control), float(e_control), float(d_control))
        mel, pitch, energy, logd, d_rounded, src_masks, mel_masks, mel_lens_out, post = out[:9]
        self._ctx = ctx
        pm = ps = None
        if self.use_cwt:                 # slots 10, 11: the (B, 1) head predictions (fastspeech2.py:117-118)
            pm, ps = out[9][0].view(-1, 1), out[9][1].view(-1, 1)
        if train and torch.is_grad_enabled():
            if self.use_cwt:
                mel, post, pitch, energy, logd, pm, ps = _Bridge.apply(self._anchor, self, mel, post, pitch, energy, logd, pm, ps)
            else:
                mel, post, pitch, energy, logd = _Bridge.apply(self._anchor, self, mel, post, pitch, energy, logd)
        return (mel, pitch, energy, logd, d_rounded, src_masks, mel_masks, src_lens, mel_lens_out, post, pm, ps)

    def _stack_fwd(self, name, x, Bn, S, lens, p=0.0, site0=None, rng=None, ctx_list=None, out=None):
        """The FFT blocks of stack `name` ("encoder" / "decoder"), each on the kernels of its plan record.  Dropout sites of block i:
        site0 + 2 i and + 1 (None, the inference halves: site 0 everywhere).  `out`: where the last block writes its output."""
        blocks = getattr(self.plan, name)
        H = self.n_head_enc if name == "encoder" else self.n_head_dec
        qkv = None
        for i, B in enumerate(blocks):
            nxt = "%s.layer_stack.%d." % (name, i + 1) if i + 1 < len(blocks) else None
            x, qkv = self._fft_fwd(B, "%s.layer_stack.%d." % (name, i), x, Bn, S, lens, H, p, 0 if site0 is None else site0 + 2 * i, rng,
                                   ctx_list, out=out if nxt is None else None, qkv=qkv, next_pre=nxt)
        return x

    def _fft_fwd(self, B, pre, x, Bn, S, lens, H, p, site, rng, ctx_list, out=None, qkv=None, next_pre=None):
        """One FFTBlock on the kernels of `B`, its fs2_plan.Block.  reference: Layers.py:25-34, SubLayers.py:31-65 (MHA), :93-101 (FFN),
        Modules.py:14-24.  Returns (x2, qkv_next); qkv_next (w2_ln "win_ln_proj"): the q|k|v projection of this block's output for
        `next_pre`, the block that follows in the stack, out of this block's last kernel -- the caller hands it to that block as `qkv`."""
        d, rows = self.d, Bn * S
        dk = d // H
        a, f = pre + "slf_attn.", pre + "pos_ffn."
        Sp = (S + 7) // 8 * 8
        dev = x.device
        # (1) q|k|v projections as one GEMM into a [rows][3d] buffer: SubLayers.py:41-43
        if B.qkv == "win":
            qkv = ops.win_conv(x.view(Bn, S, d), self._pack("qkv", a + "w_qs.weight"), 3 * d, 1, bias=self._m(a + "w_qs.bias", 3 * d)).view(rows, 3 * d)   # window kernel, k = 1
        elif B.qkv == "gemm":
            qkv = ops.linear(x, self._w(a + "w_qs.weight", 3 * d), self._m(a + "w_qs.bias", 3 * d))
        # ("chained": `qkv` came out of the previous block's last kernel)
        if B.attn == "flash":
            # (2)-(4) one kernel, no S x S tensor: scores, key-padding mask, online softmax, P V, heads merged (Modules.py:15-22,
            # SubLayers.py:57-60); the backward recomputes P from the per-row log-sum-exp kept in `probs`'s slot
            o, probs, o32 = ops.flash_attention_fwd(qkv, lens, Bn, H, S, want_lse=ctx_list is not None)
        else:
            o32 = None
            # (2) scores = Q K^T / sqrt(dk) per (batch, head), head h = columns [h*dk, (h+1)*dk): Modules.py:15-16
            scores = torch.empty(Bn * H, S, Sp, dtype=torch.float32, device=dev)
            ops.gemm(qkv, qkv[:, d:], scores, S, S, dk, 3 * d, 3 * d, Sp, alpha=dk ** -0.5, nz1=Bn, nz2=H,
                     sA=(S * 3 * d, dk), sB=(S * 3 * d, dk), sC=(H * S * Sp, S * Sp))
            # (3) key-padding mask + softmax: Modules.py:18-21
            probs = ops.softmax_fwd(scores, lens, H)
            # (4) O = P V, heads merged back into [rows][d]: Modules.py:22, SubLayers.py:57-60
            o = torch.empty(rows, d, dtype=bf16, device=dev)
            ops.gemm(probs, qkv[:, 2 * d:], o, S, dk, S, Sp, 3 * d, d, flags=ops.B_TR, nz1=Bn, nz2=H,
                     sA=(H * S * Sp, S * Sp), sB=(S * 3 * d, dk), sC=(S * d, dk))
        qkv_next = None
        # (5) fc, dropout, +residual, LayerNorm, zero PAD rows: SubLayers.py:62-63, Layers.py:29 — one kernel when d = 256
        ln = (x, self._m(a + "layer_norm.weight"), self._m(a + "layer_norm.bias"), lens, S)
        kw = dict(p_pre=p, site_pre=site, rng=rng, save_z=ctx_list is not None)
        if B.fc_ln == "win_ln":
            x1, z1, mean1, rstd1 = ops.win_ln_fwd(o, self._pack("fc", a + "fc.weight"), self._m(a + "fc.bias"), *ln, **kw)
        elif B.fc_ln == "gemm_ln":
            x1, z1, mean1, rstd1 = ops.gemm_ln_fwd(o, self._w(a + "fc.weight"), self._m(a + "fc.bias"), *ln, **kw)
        else:
            y = ops.linear(o, self._w(a + "fc.weight"), self._m(a + "fc.bias"))
            x1, z1, mean1, rstd1, _ = ops.layernorm_fwd(y, *ln, **kw)
        # (6) FFN: Conv1d(k=9)+ReLU, Conv1d(k=1), dropout, +residual, LayerNorm, zero PAD rows: SubLayers.py:96-99, Layers.py:32
        W1 = self._w(f + "w_1.weight")
        if B.w1 == "ffn":
            h = ops.ffn_conv_fwd(x1.view(Bn, S, d), W1, self._m(f + "w_1.bias"), relu=True, packed=self._pack("w1", f + "w_1.weight"))      # window kernel (csrc/ffn_conv.hip)
        elif B.w1 == "win":
            # d = 512: ttsk_ffn_conv_fwd is the 256-channel entry point; the same pack runs on the window kernel's 512-channel instance
            h = ops.win_conv(x1.view(Bn, S, d), self._pack("w1", f + "w_1.weight"), W1.shape[0], self.k1, bias=self._m(f + "w_1.bias"), relu=True)
        else:
            h = ops.conv1d(x1.view(Bn, S, d), W1, self._m(f + "w_1.bias"), flags=ops.RELU)
        ln = (x1, self._m(f + "layer_norm.weight"), self._m(f + "layer_norm.bias"), lens, S)
        kw.update(site_pre=site + 1, out=out)
        if B.w2_ln == "win_ln_proj":
            proj = (self._pack("qkv", next_pre + "slf_attn.w_qs.weight"), self._m(next_pre + "slf_attn.w_qs.bias", 3 * d))
            x2, z2, mean2, rstd2, qkv_next = ops.win_ln_fwd(h.view(rows, -1), self._pack("w2", f + "w_2.weight"), self._m(f + "w_2.bias"), *ln, proj=proj, **kw)
        elif B.w2_ln == "win_ln":
            x2, z2, mean2, rstd2 = ops.win_ln_fwd(h.view(rows, -1), self._pack("w2", f + "w_2.weight"), self._m(f + "w_2.bias"), *ln, **kw)
        elif B.w2_ln == "gemm_ln":
            x2, z2, mean2, rstd2 = ops.gemm_ln_fwd(h.view(rows, -1), self._w(f + "w_2.weight"), self._m(f + "w_2.bias"), *ln, **kw)
        else:
            y2 = ops.conv1d(h, self._w(f + "w_2.weight"), self._m(f + "w_2.bias"))
            x2, z2, mean2, rstd2, _ = ops.layernorm_fwd(y2.view(rows, d), *ln, **kw)
        if ctx_list is not None:
            ctx_list.append(_Saved(pre, x, qkv, probs, o, z1, mean1, rstd1, x1, h, z2, mean2, rstd2, Bn, S, lens, H, p, site, o32))
            ctx_list[-1].plan = B
        return x2, qkv_next

    def _predictor_fwd(self, pre, x, Bn, Lp, lens, p, site, rng, ctx, hidden_lens=None):
        """VariancePredictor.  reference: model/modules.py:255-309.  `hidden_lens` (batched synthesis): the hidden rows between the two
        convs are zero past each utterance's own length, as the second conv's zero padding is when the utterance runs alone."""
        d, rows = self.d, Bn * Lp
        c = pre + "conv_layer."
        h1 = ops.conv1d(x.view(Bn, Lp, d), self._w(c + "conv1d_1.conv.weight"), self._m(c + "conv1d_1.conv.bias"), flags=ops.RELU)
        a1, _, m1, r1, _ = ops.layernorm_fwd(h1.view(rows, -1), None, self._m(c + "layer_norm_1.weight"), self._m(c + "layer_norm_1.bias"),
                                             hidden_lens, Lp if hidden_lens is not None else 0, p_post=p, site_post=site, rng=rng, save_z=False)
        h2 = ops.conv1d(a1.view(Bn, Lp, -1), self._w(c + "conv1d_2.conv.weight"), self._m(c + "conv1d_2.conv.bias"), flags=ops.RELU)
        hw, hb = self._m(pre + "linear_layer.weight"), self._m(pre + "linear_layer.bias")
        if hb.numel() > 1:              # the CWT pitch predictor's Linear(256 -> 11): csrc/cwt.hip
            m2, r2, out = ops.layernorm_head_fwd(h2.view(rows, -1), self._m(c + "layer_norm_2.weight"), self._m(c + "layer_norm_2.bias"),
                                                 lens, Lp, hw, hb, p_post=p, site_post=site + 1, rng=rng)
        else:
            _, _, m2, r2, out = ops.layernorm_fwd(h2.view(rows, -1), None, self._m(c + "layer_norm_2.weight"), self._m(c + "layer_norm_2.bias"),
                                                  lens, Lp, p_post=p, site_post=site + 1, rng=rng, save_z=False, want_out=False,
                                                  head=(hw.view(-1), hb))
        if ctx is not None:
            ctx[pre] = (x, h1, m1, r1, a1, h2, m2, r2, Bn, Lp, lens, p, site)
        return out.view(Bn, Lp, -1) if hb.numel() > 1 else out.view(Bn, Lp)

    def _predictors_fwd_grouped(self, stack, Bn, Lp, lens, p, rng, ctx, row_limit=None):
        """The duration / pitch / energy VariancePredictors (model/modules.py:255-309) as ONE chain of grouped launches: with
        targets given (training) their inputs x, x + speaker, x + speaker + pitch_emb[target] do not depend on each other's
        outputs (modules.py:158-193).  stack (3, rows, d) bf16 holds the three inputs.  Returns (3, B, L) fp32 = (log-duration,
        pitch, energy) predictions."""
        d, rows, ps = self.d, Bn * Lp, self._pred_stride
        pre = "variance_adaptor.duration_predictor."
        c = pre + "conv_layer."
        W1, W2 = self._w(c + "conv1d_1.conv.weight"), self._w(c + "conv1d_2.conv.weight")
        Fh = W1.shape[0]
        dev = stack.device
        h1 = torch.empty(3, rows, Fh, dtype=bf16, device=dev)
        ops.conv1d(stack[0].view(Bn, Lp, d), W1, self._m(c + "conv1d_1.conv.bias"), flags=ops.RELU, out=h1[0].view(Bn, Lp, Fh),
                   nz1=3, sA=(rows * d, 0), sB=(ps, 0), sC=(rows * Fh, 0), s_bias1=ps)
        # row_limit (bucketed L): hidden rows past the batch's own longest text are zero rows — the second conv's zero padding
        a1, m1, r1, _ = ops.layernorm_fwd_grouped(h1.view(3 * rows, Fh), self._m(c + "layer_norm_1.weight"), self._m(c + "layer_norm_1.bias"),
                                                  3, ps, 2, row_limit, Lp if row_limit is not None else 0, p_post=p, site_post=200, rng=rng)
        h2 = torch.empty(3, rows, Fh, dtype=bf16, device=dev)
        ops.conv1d(a1[:rows].view(Bn, Lp, Fh), W2, self._m(c + "conv1d_2.conv.bias"), flags=ops.RELU, out=h2[0].view(Bn, Lp, Fh),
                   nz1=3, sA=(rows * Fh, 0), sB=(ps, 0), sC=(rows * Fh, 0), s_bias1=ps)
        _, m2, r2, out = ops.layernorm_fwd_grouped(h2.view(3 * rows, Fh), self._m(c + "layer_norm_2.weight"), self._m(c + "layer_norm_2.bias"),
                                                   3, ps, 2, lens, Lp, p_post=p, site_post=201, rng=rng, want_out=False,
                                                   head=(self._m(pre + "linear_layer.weight").view(-1), self._m(pre + "linear_layer.bias")))
        if ctx is not None:
            ctx["grouped"] = (stack, h1, m1, r1, a1, h2, m2, r2, Bn, Lp, lens, p, row_limit)
        return out.view(3, Bn, Lp)

    def _predictors_bwd_grouped(self, saved, dstack, rng, dx3, dxin=None):
        """Backward of _predictors_fwd_grouped; dstack (3, B, L) fp32 = gradients of (log-duration, pitch, energy) predictions,
        dx3 = gradient of the LengthRegulator input.  Returns (dx2, dx1, dx): gradients of x2 (what pitch_embedding collects),
        x1 (speaker_emb) and of the encoder output.  `dxin`: the three predictors' input gradients if _predictors_bwd_inputs ran already."""
        if dxin is None:
            dxin = self._predictors_bwd_inputs(saved, dstack, rng)
        Lp, row_limit = saved[9], saved[12]
        return ops.va_combine(dx3, dxin, Lp, row_limit)

    def _predictors_bwd_inputs(self, saved, dstack, rng, train=True, need_dur_dx=True):
        """Everything of the predictors' backward that needs only the loss's gradients: (3, rows, d) fp32 input gradients, and the
        parameter-gradient work queued.  `train` False (the variance adaptor is frozen): no parameter-gradient work, the LayerNorm
        partials the kernels emit are dropped.  `need_dur_dx` False (nothing of the encoder is trained): the duration predictor's
        input gradient, which feeds nothing but the encoder, is not computed — slot 0 of the result is not written."""
        (stack, h1, m1, r1, a1, h2, m2, r2, Bn, Lp, lens, p, row_limit) = saved
        d, rows, ps = self.d, Bn * Lp, self._pred_stride
        names = ("duration", "pitch", "energy")
        pre = "variance_adaptor.duration_predictor."
        c = pre + "conv_layer."
        W1, W2 = self._w(c + "conv1d_1.conv.weight"), self._w(c + "conv1d_2.conv.weight")
        Fh = W1.shape[0]
        dev = dstack.device
        dh2, part, nblk = ops.layernorm_bwd_grouped(None, h2.view(3 * rows, Fh), m2, r2, self._m(c + "layer_norm_2.weight"),
                                                    self._m(c + "layer_norm_2.bias"), 3, ps, 2, lens, Lp, relu_in=True, p_post=p,
                                                    site_post=201, rng=rng, dhead=dstack.view(-1),
                                                    head_w=self._m(pre + "linear_layer.weight").view(-1))
        dh2 = dh2.view(3, rows, Fh)
        for g, n in enumerate(names if train else ()):
            cg = "variance_adaptor.%s_predictor.conv_layer." % n
            self._finalize_ln(part[g], nblk, 4 * Fh + 1, cg + "conv1d_2.conv.bias")
            ops.queue_dw(self._deferred, dh2[g].view(Bn, Lp, Fh), a1[g * rows:(g + 1) * rows].view(Bn, Lp, Fh), self._g(cg + "conv1d_2.conv.weight"),
                         None, self._acc, k=self.k_var, use_dwgemm=self._use_dwconv)
        da1 = torch.empty(3, rows, Fh, dtype=bf16, device=dev)
        ops.conv1d_dx(dh2[0].view(Bn, Lp, Fh), W2, out=da1[0].view(Bn, Lp, Fh), nz1=3, sA=(rows * Fh, 0), sB=(ps, 0), sC=(rows * Fh, 0))
        dh1, part, nblk = ops.layernorm_bwd_grouped(da1.view(3 * rows, Fh), h1.view(3 * rows, Fh), m1, r1, self._m(c + "layer_norm_1.weight"),
                                                    self._m(c + "layer_norm_1.bias"), 3, ps, 2, row_limit, Lp if row_limit is not None else 0,
                                                    relu_in=True, p_post=p, site_post=200, rng=rng)
        dh1 = dh1.view(3, rows, Fh)
        for g, n in enumerate(names if train else ()):
            cg = "variance_adaptor.%s_predictor.conv_layer." % n
            self._finalize_ln(part[g], nblk, 3 * Fh, cg + "conv1d_1.conv.bias")
            ops.queue_dw(self._deferred, dh1[g].view(Bn, Lp, Fh), stack[g].view(Bn, Lp, d), self._g(cg + "conv1d_1.conv.weight"), None,
                         self._acc, k=self.k_var, use_dwgemm=self._use_dwconv)
        dxin = torch.empty(3, rows, d, dtype=torch.float32, device=dev)
        if need_dur_dx:
            ops.conv1d_dx(dh1[0].view(Bn, Lp, Fh), W1, out=dxin[0].view(Bn, Lp, d), nz1=3, sA=(rows * Fh, 0), sB=(ps, 0), sC=(rows * d, 0))
        else:       # the pitch and energy predictors only
            ops.conv1d_dx(dh1[1].view(Bn, Lp, Fh), self._w("variance_adaptor.pitch_predictor.conv_layer.conv1d_1.conv.weight"),
                          out=dxin[1].view(Bn, Lp, d), nz1=2, sA=(rows * Fh, 0), sB=(ps, 0), sC=(rows * d, 0))
        return dxin

    def _forward(self, train, speakers, texts, src_lens, Lp, mel_lens, max_mel_len, e_targets, d_targets, pitches_raw,
                 p_control, e_control, d_control, frame_limit=None, phoneme_limit=None, defer_pred_join=False):
        """`defer_pred_join` (training): leave the predictors' stream un-joined (`_pred_fwd_pending` stays set) — for a caller that takes the
        loss in two halves (ops.fs2_loss_split: the frame-level half needs nothing of the predictors) and joins that stream itself.
        `phoneme_limit` (device int64[B], every entry = the batch's own longest text, training only): phoneme positions beyond it
        exist only because the batch was padded to a shape bucket; the predictors treat them as the zero padding the reference's
        batch has there.  `frame_limit` (device int32[1], training only): the batch was padded to a shape bucket (tts_king_amd/engine.py);
        frames t >= frame_limit[0] of every utterance do not exist in the reference's batch — the PostNet's BatchNorm statistics,
        its zero padding and (in the loss) the mel denominators are taken as if the batch ended there."""
        if self.use_cwt and phoneme_limit is not None:
            # the CNNscalar heads pool over the padded length as the reference's batch has it (modules.py:360-364): a text axis padded
            # further would change their result, so the CWT branch takes texts at their own longest length (train.py: l_bucket 1)
            raise ops.L.TtskError("use_cwt: texts padded to a phoneme bucket are not supported (mi355x.l_bucket must be 1)")
        self.sync_shadow()
        dev, d = self.device, self.d
        Bn = texts.shape[0]
        ctx = _Ctx() if train else None
        rng = ops.rng_of(self._state()) if train else None
        p_enc, p_dec, p_var, p_post = (self.p_enc, self.p_dec, self.p_var, self.p_post) if train else (0.0, 0.0, 0.0, 0.0)
        p_pitch = (self.p_pitch if train else 0.0) if self.use_cwt else p_var
        heads = heads_saved = None
        blocks = [] if train else None
        preds = {} if train else None

        # ---- masks: fastspeech2.py:62-69.  Nothing on the device reads them (every kernel takes the lengths): when the training forward
        # has its predictor stream, they are produced there (below) instead of opening the main chain with two dependent launches
        grouped = (train and self.group_predictors and pitches_raw is not None and e_targets is not None and Lp <= self.max_seq_len)
        masks_aside = grouped and self.pred_side in ("1", "f") and mel_lens is not None and d_targets is not None and max_mel_len is not None
        src_masks = None if masks_aside else ops.length_mask(src_lens, Lp)
        # ---- encoder: phoneme embedding + position table, 4 FFT blocks: Models.py:79-112
        if Lp > self.max_seq_len:
            pe_enc = sinusoid_table(Lp, d).to(dev)        # eval-only long input: Models.py:88-99
        else:
            pe_enc = self.get("encoder.position_enc")[0]
        x = ops.gather_add(None, self._m("encoder.src_word_emb.weight"), texts, pe=pe_enc, pe_mod=Lp, rows=Bn * Lp)
        stack = torch.empty(3, Bn * Lp, d, dtype=bf16, device=dev) if grouped else None
        x = self._stack_fwd("encoder", x, Bn, Lp, src_lens, p_enc, 0, rng, blocks, out=stack[0] if grouped else None)
        # ---- variance adaptor: modules.py:142-217 (duration BEFORE the speaker embedding; energy sees the pitch embedding)
        va = "variance_adaptor."
        if grouped:
            # training with targets: the embeddings are picked by the TARGET pitch / energy, so the three predictor inputs are
            # known up front — one pass builds them (and x3), then the predictors run as grouped launches
            x3, pidx, eidx = ops.va_embed(stack, speakers, self._m("speaker_emb.weight"), Lp, pitches_raw.to(dev).float().contiguous(),
                                          self.get(va + "pitch_bins"), self._m(va + "pitch_embedding.weight"),
                                          e_targets.to(dev).float().contiguous(), self.get(va + "energy_bins"),
                                          self._m(va + "energy_embedding.weight"), row_limit=phoneme_limit)
            if self.pred_side in ("1", "f"):
                if self._pred_stream is None:
                    self._pred_stream = torch.cuda.Stream(device=dev)
                self._pred_stream.wait_stream(torch.cuda.current_stream())
                mel_masks_aside = None
                with torch.cuda.stream(self._pred_stream):
                    pred = self._predictors_fwd_grouped(stack, Bn, Lp, src_lens, p_var, rng, preds, row_limit=phoneme_limit)
                    if masks_aside:
                        T_m = min(int(max_mel_len), self.max_seq_len)
                        src_masks = ops.length_mask(src_lens, Lp)
                        mel_masks_aside = ops.length_mask(mel_lens.to(dev).long().contiguous(), T_m)
                self._pred_fwd_pending = True          # joined at the end of this forward: the loss is the first reader
            else:
                pred = self._predictors_fwd_grouped(stack, Bn, Lp, src_lens, p_var, rng, preds, row_limit=phoneme_limit)
            logd, pitch, energy = pred[0], pred[1], pred[2]
        else:
            logd = self._predictor_fwd(va + "duration_predictor.", x, Bn, Lp, src_lens, p_var, 200, rng, preds)
            x1 = ops.gather_add(x, self._m("speaker_emb.weight"), speakers, idx_div=Lp)          # fastspeech2.py:72-75
            pitch = self._predictor_fwd(va + "pitch_predictor.", x1, Bn, Lp, src_lens, p_pitch, 202, rng, preds)
            if self.use_cwt:
                pidx, heads, heads_saved = self._cwt_pitch_rows(x1, pitch, Bn, Lp, p_control)
            elif pitches_raw is not None:
                pidx = ops.bucketize(pitches_raw.to(dev).float(), self.get(va + "pitch_bins"))
            else:
                pidx, pitch = ops.bucketize(pitch, self.get(va + "pitch_bins"), p_control, want_scaled=True)
            x2 = ops.gather_add(x1, self._m(va + "pitch_embedding.weight"), pidx.view(-1))
            energy = self._predictor_fwd(va + "energy_predictor.", x2, Bn, Lp, src_lens, p_var, 204, rng, preds)
            if e_targets is not None:
                eidx = ops.bucketize(e_targets.to(dev).float(), self.get(va + "energy_bins"))
            else:
                eidx, energy = ops.bucketize(energy, self.get(va + "energy_bins"), e_control, want_scaled=True)
            x3 = ops.gather_add(x2, self._m(va + "energy_embedding.weight"), eidx.view(-1))
        # ---- length regulator (+ decoder position table, fused): modules.py:196-205,225-252; Models.py:172-178
        if d_targets is not None:
            dur = d_targets.to(dev).long().contiguous()
            d_rounded = d_targets
        else:
            dur = ops.duration_round(logd, d_control)
            d_rounded = dur
        if d_targets is not None and max_mel_len is not None:
            T_full = int(max_mel_len)
        else:
            _, _, _, total = ops.length_regulator_fwd(x3.view(Bn, Lp, d), dur, 1, want_idx=False)
            T_full = max(int(total.max().item()), 1)       # data-dependent output length: one host read, as in the reference
        eval_long = (not train) and T_full > self.max_seq_len
        T = T_full if eval_long else min(T_full, self.max_seq_len)
        pe_dec = sinusoid_table(T, d).to(dev) if eval_long else self.get("decoder.position_enc")[0]
        dec_in, _, cs, mel_lens_out = ops.length_regulator_fwd(x3.view(Bn, Lp, d), dur, T, pe=pe_dec, want_idx=False)
        mlens = mel_lens.to(dev).long().contiguous() if mel_lens is not None else mel_lens_out
        if masks_aside and mel_masks_aside is not None and mel_masks_aside.shape[1] == T:
            mel_masks = mel_masks_aside
        else:
            mel_masks = ops.length_mask(mlens, T)
        # ---- decoder: Models.py:157-189
        y = dec_in.view(Bn * T, d)
        n_enc_blocks = len(blocks) if train else 0
        y = self._stack_fwd("decoder", y, Bn, T, mlens, p_dec, 100, rng, blocks)
        # ---- mel_linear (fp32 output + bf16 copy for the PostNet): fastspeech2.py:102
        rows = Bn * T
        plan = self.plan
        if plan.mel_fwd == "win_dual":
            mel, mel16 = ops.win_conv_dual(y.view(Bn, T, d), self._pack("lin", "mel_linear.weight"), self.n_mel, 1, bias=self._m("mel_linear.bias"))      # window kernel, k = 1
            mel, mel16 = mel.view(rows, self.n_mel), mel16.view(rows, self.n_mel)
        else:
            mel16 = torch.empty(rows, self.n_mel, dtype=bf16, device=dev)
            mel = ops.linear(y, self._w("mel_linear.weight"), self._m("mel_linear.bias"), out_dtype=torch.float32, C2=mel16)
        fl = (frame_limit, T) if (frame_limit is not None and train) else None
        if fl is not None:
            ops.zero_frames_from(mel16, fl)          # the PostNet's first conv sees zero padding past the batch's own length
        # ---- PostNet: Layers.py:133-143, + mel: fastspeech2.py:104
        post, pn = self._postnet_fwd(mel, mel16, Bn, T, train, p_post, 300, rng, fl)
        if self._pred_fwd_pending and not defer_pred_join:
            torch.cuda.current_stream().wait_stream(self._pred_stream)
            self._pred_fwd_pending = False
        if train:
            ctx.blocks, ctx.preds, ctx.pn = blocks, preds, pn
            ctx.plan = plan                 # the backward runs the routes this forward ran, whatever is toggled in between
            ctx.n_enc_blocks = n_enc_blocks
            ctx.dims = (Bn, Lp, T)
            ctx.texts, ctx.speakers, ctx.pidx, ctx.eidx, ctx.cs = texts, speakers, pidx, eidx, cs
            ctx.dec_out = y
            ctx.frame_limit = fl
            ctx.used = False
            ctx.heads_saved = heads_saved
        out = (mel.view(Bn, T, self.n_mel), pitch, energy, logd, d_rounded, src_masks, mel_masks, mel_lens_out,
               post.view(Bn, T, self.n_mel))
        if self.use_cwt:
            out = out + (heads,)            # (2, B) fp32: pitch_mean row, pitch_std row
        return out, ctx

    def _postnet_fwd(self, mel, mel16, Bn, T, train=False, p=0.0, site0=None, rng=None, fl=None, lens=None):
        """PostNet + mel on the plan's routes (Layers.py:133-143, fastspeech2.py:104): the train forward (batch statistics; `fl`: the
        frame limit of a bucketed batch), the eval forward and the inference halves (running statistics; `lens`, batched synthesis:
        frames past an utterance's own length come out as zero rows).  Dropout site of layer i: site0 + i (None: 0).  Returns
        (postnet mel, per layer what the backward needs)."""
        rows, pn = Bn * T, []
        xin = mel16.view(Bn, T, self.n_mel)
        for i, layer in enumerate(self.plan.postnet):
            pp = "postnet.convolutions.%d." % i
            route, stats, last = layer.conv if train else layer.conv_eval, None, i == 4
            C, k, _ = self._table[pp + "0.conv.weight"].storage_shape
            # conv output stays fp32: BatchNorm divides by the batch std, which amplifies a bf16 rounding of it
            if route == "gemm":
                yc = ops.conv1d(xin, self._w(pp + "0.conv.weight"), self._m(pp + "0.conv.bias"), out_dtype=torch.float32)
            elif route == "win_stats":       # window kernel; the BatchNorm statistics partials of its output come out of its epilogue
                yc, stats = ops.win_conv_stats(xin, self._pack("pn", pp + "0.conv.weight"), C, k, bias=self._m(pp + "0.conv.bias"), frame_limit=fl)
            else:
                yc = ops.win_conv(xin, self._pack("pn", pp + "0.conv.weight"), C, k, bias=self._m(pp + "0.conv.bias"), out_dtype=torch.float32)
            run = (self.get(pp + "1.running_mean"), self.get(pp + "1.running_var"), self.get(pp + "1.num_batches_tracked").view(1))
            gb = (self._m(pp + "1.weight"), self._m(pp + "1.bias"), not last)
            kw = dict(resid=mel if last else None, out_f32=last)
            site, keep = 0 if site0 is None else site0 + i, None
            if train and layer.bn == "slab":
                # statistics partials, then one kernel that finishes mean / rstd per channel slab and normalises
                nxt, mean, rstd, keep = ops.bn_train(yc.view(rows, C), *run, *gb, p=p, site=site, rng=rng, frame_limit=fl, want_keep=True, partials=stats, **kw)
            else:
                mean, rstd = ops.bn_train_stats(yc.view(rows, C), *run, frame_limit=fl) if train else (run[0], ops.rsqrt_eps(run[1]))
                if lens is not None:
                    nxt = ops.bn_apply_lens(yc.view(rows, C), mean, rstd, *gb, lens, T, **kw)
                else:
                    nxt = ops.bn_apply(yc.view(rows, C), mean, rstd, *gb, p=p, site=site, rng=rng, frame_limit=fl, **kw)
            pn.append((pp, xin, yc, mean, rstd, keep))
            xin = nxt.view(Bn, T, C) if not last else nxt
        return xin, pn

    def _cwt_pitch_rows(self, x1, pitch_cwt, Bn, Lp, p_control):
        """get_pitch_embedding_cwt behind the predictor (modules.py:118-129): both CNNscalar heads on (x + speaker, prediction) in one
        launch, then the coefficients -> pitch -> embedding row.  Returns (rows (B, L) int32, heads (2, B), what the heads' backward
        needs).  `self._cwt_pitch`: the fp32 pitch of the last call, `self._cwt_head_inputs`: what the heads read in it (the facade and
        the tests read them)."""
        va = "variance_adaptor."
        heads, saved = ops.cnnscalar_fwd(x1, pitch_cwt, self._m(va + "pitch_mean.flat_one.net.0.weight", 2 * ops.CNNSCALAR_FLOATS), Bn, Lp)
        self._cwt_head_inputs = (x1, pitch_cwt)
        self._cwt_pitch, pidx = ops.cwt_pitch(pitch_cwt, heads, self.get(va + "pitch_bins"), p_control)
        return pidx, heads, saved

    # ------------------------------------------------------------------ inference in two capturable halves
    def eval_front(self, speakers, texts, src_lens, Lp, p_control=1.0, e_control=1.0, d_control=1.0):
        """Encoder + variance adaptor of the free-running inference path (reference: fastspeech2.py:62-99 with no
        targets, modules.py:142-205) up to the per-utterance frame totals.  Only enqueues kernels (hipGraph-capturable);
        the caller reads `total.max()` on the host — the one data-dependent shape of the path — and calls `eval_back`."""
        return self._eval_front(speakers, texts, src_lens, Lp, p_control, e_control, d_control, ragged=False)

    def eval_back(self, x3, dur, Lp, T):
        """LengthRegulator + decoder + mel_linear + PostNet for a known frame count T (reference: modules.py:199-205,
        Models.py:157-189, fastspeech2.py:101-104).  Capturable; returns (mel, postnet mel, mel_lens, mel_masks)."""
        return self._eval_back(x3, dur, Lp, T, ragged=False)

    # ---- batched inference: every utterance as if run alone
    def eval_front_ragged(self, speakers, texts, src_lens, Lp, p_control, e_control, d_control):
        """`eval_front` for texts of different lengths padded to Lp phonemes, each utterance computed as the model computes it
        alone.  The reference's padded batch is not that: its predictors' second conv reads non-zero padded
        rows.  Here every tensor a predictor conv reads as a neighbour is zero past src_lens[u]: the encoder output (its last
        LayerNorm zeroes PAD rows), + speaker (`gather_add_lens`), + pitch embedding (`embed_step`), and the hidden rows
        (`layernorm_fwd` given the lengths).  speakers / src_lens (B,) int64, the controls (B,) fp32 device tensors: values, not
        shapes, so one captured graph serves every setting.  Returns (x3, dur, total, (pitch, energy, logd)): no masks."""
        if self.use_cwt:
            # inverse_batch_cwt standardises over the batch axis (cwt_utils.py:40-66, x.mean(0)) and the CNNscalar heads pool over the
            # padded length (modules.py:360-364): the reference defines no batch-independent result for this branch
            raise ops.L.TtskError("use_cwt: batched synthesis of different-length texts is not defined -- the reference's CWT pitch "
                                  "standardises over the batch axis and its scalar heads pool over the padded length; synthesize one text per call")
        if Lp > self.max_seq_len:
            raise ops.L.TtskError("eval_front_ragged: %d phonemes exceed max_seq_len %d; longer texts take the single-utterance path" % (Lp, self.max_seq_len))
        return self._eval_front(speakers, texts, src_lens, Lp, p_control, e_control, d_control, ragged=True)

    def eval_front_rows(self, speakers, texts, src_lens, Lp, rows):
        """`eval_front_ragged` with per-phoneme prosody.  `rows`: ten device tensors, all VALUES of one graph --
        (p_control, pitch, has_pitch, e_control, energy, has_energy, d_control, durations, has_durations) each (B, Lp), fp32 and uint8
        flags, and target_frames (B,) int32 (< 0: no budget); `batching.plan_prosody` builds them with neutral padding.  Where a flag is
        set the value replaces prediction * control (the reference's targets, modules.py:92-101,131-140,195-205); the energy predictor
        reads the pitch embedding picked that way.  The durations are then fitted to the budget (`ops.duration_fit`).  Neutral inputs
        give `eval_front_ragged`'s bits.  Returns what it returns; pitch / energy / dur report what was used."""
        if self.use_cwt:
            raise ops.L.TtskError("use_cwt: batched synthesis of different-length texts is not defined -- the reference's CWT pitch "
                                  "standardises over the batch axis and its scalar heads pool over the padded length; synthesize one text per call")
        if Lp > min(self.max_seq_len, ops.FIT_MAX_L):
            raise ops.L.TtskError("eval_front_rows: %d phonemes exceed the limit %d (max_seq_len %d, duration_fit %d)"
                                  % (Lp, min(self.max_seq_len, ops.FIT_MAX_L), self.max_seq_len, ops.FIT_MAX_L))
        if len(rows) != 10:
            raise ops.L.TtskError("eval_front_rows: rows must hold 10 tensors (three controls, three values, three flags, the targets), got %d" % len(rows))
        return self._eval_front(speakers, texts, src_lens, Lp, None, None, None, ragged=True, rows=rows)

    def eval_back_ragged(self, x3, dur, Lp, T):
        """`eval_back` for a frame count T that is a bucket (>= every utterance's own count): frames t >= mel_lens[u] of the PostNet's
        input and of its layers' outputs are zero rows, the zero padding each k = 5 conv meets when utterance u runs alone (in the
        reference's batch mel_linear's bias sits there, Layers.py:133-143).  Returns (mel, postnet mel, mel_lens); only frames
        t < mel_lens[u] of the two mels mean anything."""
        if T > self.max_seq_len:
            raise ops.L.TtskError("eval_back_ragged: %d frames exceed max_seq_len %d" % (T, self.max_seq_len))
        return self._eval_back(x3, dur, Lp, T, ragged=True)[:3]

    def _eval_front(self, speakers, texts, src_lens, Lp, p_control, e_control, d_control, ragged, rows=None):
        """The body of `eval_front` (`ragged` False: scalar controls, the reference's padded-batch semantics), of
        `eval_front_ragged` (True: control tensors, per-utterance limits on everything a predictor conv reads) and of
        `eval_front_rows` (`rows`: the ragged front with the per-row kernels and the duration fit)."""
        self.sync_shadow()
        d = self.d
        Bn = texts.shape[0]
        va = "variance_adaptor."
        src_masks = None if ragged else ops.length_mask(src_lens, Lp)       # nothing on the device reads the masks
        pe_enc = sinusoid_table(Lp, d).to(self.device) if Lp > self.max_seq_len else self.get("encoder.position_enc")[0]
        x = ops.gather_add(None, self._m("encoder.src_word_emb.weight"), texts, pe=pe_enc, pe_mod=Lp, rows=Bn * Lp)
        x = self._stack_fwd("encoder", x, Bn, Lp, src_lens)
        hl = src_lens if ragged else None
        logd = self._predictor_fwd(va + "duration_predictor.", x, Bn, Lp, src_lens, 0.0, 0, None, None, hidden_lens=hl)
        if ragged:
            x1 = ops.gather_add_lens(x, self._m("speaker_emb.weight"), speakers, src_lens, Lp)
        else:
            x1 = ops.gather_add(x, self._m("speaker_emb.weight"), speakers, idx_div=Lp)
        pitch = self._predictor_fwd(va + "pitch_predictor.", x1, Bn, Lp, src_lens, 0.0, 0, None, None, hidden_lens=hl)
        heads = None
        if rows is not None:
            pc, pv, ph, ec, ev, eh, dc, dv, dh, target = rows
            x2, pitch, _ = ops.embed_step_rows(pitch, pc, pv, ph, self.get(va + "pitch_bins"), self._m(va + "pitch_embedding.weight"), x1, src_lens, Lp)
        elif ragged:
            x2, pitch, _ = ops.embed_step(pitch, p_control, self.get(va + "pitch_bins"), self._m(va + "pitch_embedding.weight"), x1, src_lens, Lp)
        else:
            if self.use_cwt:
                pidx, heads, _ = self._cwt_pitch_rows(x1, pitch, Bn, Lp, p_control)
            else:
                pidx, pitch = ops.bucketize(pitch, self.get(va + "pitch_bins"), p_control, want_scaled=True)
            x2 = ops.gather_add(x1, self._m(va + "pitch_embedding.weight"), pidx.view(-1))
        energy = self._predictor_fwd(va + "energy_predictor.", x2, Bn, Lp, src_lens, 0.0, 0, None, None, hidden_lens=hl)
        if rows is not None:
            x3, energy, _ = ops.embed_step_rows(energy, ec, ev, eh, self.get(va + "energy_bins"), self._m(va + "energy_embedding.weight"), x2, src_lens, Lp)
            dur = ops.duration_fit(ops.duration_rows(logd, dc, dv, dh), dh, target, src_lens)
        elif ragged:
            x3, energy, _ = ops.embed_step(energy, e_control, self.get(va + "energy_bins"), self._m(va + "energy_embedding.weight"), x2, src_lens, Lp)
            dur = ops.duration_round_dev(logd, d_control)
        else:
            eidx, energy = ops.bucketize(energy, self.get(va + "energy_bins"), e_control, want_scaled=True)
            x3 = ops.gather_add(x2, self._m(va + "energy_embedding.weight"), eidx.view(-1))
            dur = ops.duration_round(logd, d_control)
        _, _, _, total = ops.length_regulator_fwd(x3.view(Bn, Lp, d), dur, 1, want_idx=False)
        if ragged:
            return x3, dur, total, (pitch, energy, logd)
        if self.use_cwt:
            return x3, dur, total, (pitch, energy, logd, src_masks, heads)     # pitch: the (B, L, 11) prediction; heads (2, B)
        return x3, dur, total, (pitch, energy, logd, src_masks)

    def _eval_back(self, x3, dur, Lp, T, ragged):
        """The body of `eval_back` and (`ragged`: per-utterance frame limits in the PostNet, no mask) of `eval_back_ragged`."""
        d = self.d
        Bn = x3.shape[0] // Lp
        dev = self.device
        pe_dec = sinusoid_table(T, d).to(dev) if T > self.max_seq_len else self.get("decoder.position_enc")[0]
        dec_in, _, _, mel_lens = ops.length_regulator_fwd(x3.view(Bn, Lp, d), dur, T, pe=pe_dec, want_idx=False)
        mel_masks = None if ragged else ops.length_mask(mel_lens, T)
        y = self._stack_fwd("decoder", dec_in.view(Bn * T, d), Bn, T, mel_lens)
        rows = Bn * T
        # (plan.mel_eval: "gemm" -- the forward's "win_dual" has not been taken here)
        mel16 = torch.empty(rows, self.n_mel, dtype=bf16, device=dev)
        mel = ops.linear(y, self._w("mel_linear.weight"), self._m("mel_linear.bias"), out_dtype=torch.float32, C2=mel16)
        if ragged:
            ops.zero_frames_lens(mel16, mel_lens, T)     # the path's one zero-fill pass: the GEMM's bf16 copy carries the bias in padded frames
        post, _ = self._postnet_fwd(mel, mel16, Bn, T, lens=mel_lens if ragged else None)
        return mel.view(Bn, T, self.n_mel), post.view(Bn, T, self.n_mel), mel_lens, mel_masks

    # ------------------------------------------------------------------ backward
    def _backward_from_autograd(self, ctx, dmel, dpost, dpitch, denergy, dlogd, dpm=None, dps=None):
        dev = self.device
        Bn, Lp, T = ctx.dims

        def f32(g, shape):
            if g is None:
                return torch.zeros(shape, dtype=torch.float32, device=dev)
            return g.to(torch.float32).contiguous()
        dmel, dpost = f32(dmel, (Bn, T, self.n_mel)), f32(dpost, (Bn, T, self.n_mel))
        with torch.no_grad():
            dmel_sum = ops.add_f32(dmel, dpost)
            dheads = None
            if self.use_cwt:
                dheads = torch.stack([f32(dpm, (Bn, 1)).view(-1), f32(dps, (Bn, 1)).view(-1)])      # device copies, no arithmetic
            self.backward_native(ctx, dmel_sum, dpost, f32(dpitch, (Bn, Lp, ops.CWT_CHANNELS) if self.use_cwt else (Bn, Lp)),
                                 f32(denergy, (Bn, Lp)), f32(dlogd, (Bn, Lp)), dheads=dheads)
            # one dropout-counter tick per micro-step, as main_train_step / graph.make_enqueue do: Philox masks are a
            # function of (seed, step, site, element), so without it every `loss.backward()` step would reuse one mask
            ops.rng_advance(self._state())

    def _finalize_ln(self, partials, nblk, ncol, first_key):
        """partials [nblk][ncol] = dbias | dgamma | dbeta (| dhead_w | dhead_b) -> the flat gradient buffer, where the
        sub-layer bias, LayerNorm weight and LayerNorm bias (and the predictor head) sit back to back in that order
        starting at `first_key` (params.py builds them so): ONE finalize launch per LayerNorm."""
        off = self._table[first_key].offset
        ops.colsum_finalize(partials, nblk, ncol, ncol, self._flat_grad[off:off + ncol], accumulate=self._acc, defer=self._deferred_fin)

    def _fft_bwd(self, saved, dx2, rng, raw_out=False, train=True, need_dx=True):
        """Backward of one FFTBlock, on the kernels of `saved.plan` (the forward's fs2_plan.Block).  `dx2`: gradient of the block
        output as the block behind hands it over (its `qkv_dx`) — a bf16 tensor; (Slabs, residual) when the dX GEMM that produced it
        left its split-K partial tiles un-reduced: the LayerNorm backward sums them while it reads its rows, so no reducer launch and
        no bf16 copy of that gradient exist; or ("pre") (dqkv, packed transposed q|k|v weight, residual): this block's first kernel
        multiplies by the weight itself.  Returns the gradient of the block input in the form its own `qkv_dx` names; `raw_out`: the
        caller has a block of the stack in front of this one to hand it to (checked against the plan's position).  `train` False
        (the block is frozen): none of its parameter-gradient work is issued (the LayerNorm / bias partials the fused kernels emit are
        dropped).  `need_dx` False (nothing in front of the block is trained): the block's input gradient is not computed, the
        result is None."""
        pre, x, qkv, probs, o, z1, mean1, rstd1, x1, h, z2, mean2, rstd2, Bn, S, lens, H, p, site, o32 = saved
        B = saved.plan
        if bool(raw_out) != (B.qkv_dx in ("pre", "win_split", "gemm_raw")):
            raise ops.L.TtskError("%s: the plan hands its input gradient over as %r, the caller asked with raw_out=%r" % (pre, B.qkv_dx, raw_out))
        d, rows = self.d, Bn * S
        dk = d // H
        a, f = pre + "slf_attn.", pre + "pos_ffn."
        dev = z2.device
        # ---- FFN tail: LN backward (PAD rows carry no gradient), dropout mask regenerated
        pre2 = None
        if isinstance(dx2, tuple) and len(dx2) == 3:
            if B.w2_bwd != "ln_proj":
                raise ops.L.TtskError("%s: handed a \"pre\" input gradient, which only its \"ln_proj\" route consumes (plan: %r)" % (pre, B.w2_bwd))
            pre2, sl2, r2, dd2 = (dx2[0], dx2[1]), None, dx2[2], None
        else:
            sl2, r2, dd2 = (dx2[0], dx2[1], None) if isinstance(dx2, tuple) else (None, None, dx2)
        if B.w2_bwd == "ln_proj":
            # (the q|k|v input gradient of the block behind +) LN backward + w_2's dX (ReLU gate on the way out) in one launch
            dz2, dy2, part, nblk, dh = ops.layernorm_bwd_proj(dd2, z2, mean2, rstd2, self._m(f + "layer_norm.weight"), self._pack("w2T", f + "w_2.weight"),
                                                              h.shape[-1], lens, S, p_pre=p, site_pre=site + 1, rng=rng, slabs=sl2, R=r2, gate=h, pre=pre2)
            dh = dh.view(Bn, S, -1)
        else:
            dz2, dy2, part, nblk = ops.layernorm_bwd(dd2, z2, mean2, rstd2, self._m(f + "layer_norm.weight"), self._m(f + "layer_norm.bias"),
                                                     lens, S, p_pre=p, site_pre=site + 1, rng=rng, slabs=sl2, R=r2)
        # ---- w_2 (k=1): dW, dX gated by the ReLU
        if train:
            self._finalize_ln(part, nblk, 3 * d, f + "w_2.bias")
            ops.queue_dw(self._deferred, dy2.view(Bn, S, d), h, self._g(f + "w_2.weight"), lens, self._acc, k=self.k2, use_dwgemm=self._use_dwconv)
        if B.w2_bwd == "win":
            dh = ops.win_conv(dy2.view(Bn, S, d), self._pack("w2T", f + "w_2.weight"), h.shape[-1], 1, gate=h)     # dX as a forward conv on the transposed pack, ReLU gate on the way out
        elif B.w2_bwd == "gemm":
            dh = ops.conv1d_dx(dy2.view(Bn, S, d), self._w(f + "w_2.weight"), G=h)
        # ---- w_1 (k=9): bias, dW, dX + residual gradient; the dX stays in split-K form for the attention LayerNorm's backward
        if train:
            ops.colsum_into(dh.view(rows, -1), self._g(f + "w_1.bias"), defer=self._deferred_fin, accumulate=self._acc)
            if B.w1_dw == "dwconv" and self._use_dwconv and Bn <= 64:
                # the taps share one fetch of dh and one window of x1 (csrc/dwconv.hip); dh is zero at PAD rows (the LayerNorm backward
                # that produced dy2 gives them no gradient), so only the rows of each utterance's own length are walked
                self._deferred.dwconv.append((dh, x1.view(Bn, S, d), self._g(f + "w_1.weight"), lens, self._acc))
            else:
                ops.conv1d_dw(dh, x1.view(Bn, S, d), self._g(f + "w_1.weight"), k=self.k1, defer=self._deferred, accumulate=self._acc)
        # ---- attention tail
        if B.w1_dx == "win_split":
            sl = ops.win_conv_split(dh, self._pack("w1T", f + "w_1.weight"), d, self.k1)       # four 256-channel slices of the 1024-channel contraction, one launch
        else:
            sl = ops.conv1d_dx(dh, self._w(f + "w_1.weight"), raw=True)
        # the attention backward's delta = rowsum(dO o O) per head comes out of the kernel that stores dO (B.fc_delta), given the
        # forward's fp32 O
        delta = torch.empty(Bn * H, S, dtype=torch.float32, device=dev) if (B.fc_delta and o32 is not None) else None
        dkw = dict(delta_o32=o32 if delta is not None else None, delta_out=delta)
        fc_bwd = "win" if (B.fc_bwd == "ln_proj" and lens is None) else B.fc_bwd
        if fc_bwd == "ln_proj":
            # LN backward + fc's dX (+ delta) in one launch
            dz1, dy1, part, nblk, do = ops.layernorm_bwd_proj(None, z1, mean1, rstd1, self._m(a + "layer_norm.weight"), self._pack("fcT", a + "fc.weight"),
                                                              d, lens, S, p_pre=p, site_pre=site, rng=rng, slabs=sl, R=dz2, **dkw)
        else:
            dz1, dy1, part, nblk = ops.layernorm_bwd(None, z1, mean1, rstd1, self._m(a + "layer_norm.weight"), self._m(a + "layer_norm.bias"),
                                                     lens, S, p_pre=p, site_pre=site, rng=rng, slabs=sl, R=dz2)
        if train:
            self._finalize_ln(part, nblk, 3 * d, a + "fc.bias")
            ops.queue_dw(self._deferred, dy1.view(Bn, S, d), o.view(Bn, S, d), self._g(a + "fc.weight"), lens, self._acc, use_dwgemm=self._use_dwconv)
        if fc_bwd == "win":
            do = ops.win_conv(dy1.view(Bn, S, d), self._pack("fcT", a + "fc.weight"), d, 1, **dkw).view(rows, d)
        elif fc_bwd == "gemm":
            do = ops.linear_dx(dy1, self._w(a + "fc.weight"))
        # ---- attention core: dP = dO V^T ; dS = softmax'(P, dP)/sqrt(dk) ; dQ = dS K ; dK = dS^T Q ; dV = P^T dO
        if B.attn == "flash":
            dqkv = ops.flash_attention_bwd(qkv, o, do, probs, lens, Bn, H, S, o32=o32, delta=delta)      # P recomputed per tile; dQ, dK, dV in two launches
        else:
            Sp = probs.shape[2]
            dqkv = torch.empty(rows, 3 * d, dtype=bf16, device=dev)
            dP = torch.empty(Bn * H, S, Sp, dtype=torch.float32, device=dev)
            ops.gemm(do, qkv[:, 2 * d:], dP, S, S, dk, d, 3 * d, Sp, nz1=Bn, nz2=H, sA=(S * d, dk), sB=(S * 3 * d, dk),
                     sC=(H * S * Sp, S * Sp))
            dS = ops.softmax_bwd(probs, dP, dk ** -0.5)
            ops.gemm(dS, qkv[:, d:], dqkv, S, dk, S, Sp, 3 * d, 3 * d, flags=ops.B_TR, nz1=Bn, nz2=H,
                     sA=(H * S * Sp, S * Sp), sB=(S * 3 * d, dk), sC=(S * 3 * d, dk))
            kv = ops.GemmGroup()         # dK and dV are independent: one grouped launch
            ops.gemm(dS, qkv, dqkv[:, d:], S, dk, S, Sp, 3 * d, 3 * d, flags=ops.A_TR | ops.B_TR, nz1=Bn, nz2=H,
                     sA=(H * S * Sp, S * Sp), sB=(S * 3 * d, dk), sC=(S * 3 * d, dk), group=kv)
            ops.gemm(probs, do, dqkv[:, 2 * d:], S, dk, S, Sp, d, 3 * d, flags=ops.A_TR | ops.B_TR, nz1=Bn, nz2=H,
                     sA=(H * S * Sp, S * Sp), sB=(S * d, dk), sC=(S * 3 * d, dk), group=kv)
            kv.flush()
        # ---- q|k|v projections
        if train:
            ops.colsum_into(dqkv, self._g(a + "w_qs.bias", 3 * d), defer=self._deferred_fin, accumulate=self._acc)
            ops.queue_dw(self._deferred, dqkv.view(Bn, S, 3 * d), x.view(Bn, S, d), self._g(a + "w_qs.weight", 3 * d * d).view(3 * d, d), lens,
                         self._acc, use_dwgemm=self._use_dwconv)
        if not need_dx:
            return None
        if B.qkv_dx == "pre":
            return (dqkv, self._pack("qkvT", a + "w_qs.weight"), dz1)     # the consumer (the block in front's first backward kernel) multiplies by the weight itself
        if B.qkv_dx == "win_split":
            return (ops.win_conv_split(dqkv.view(Bn, S, 3 * d), self._pack("qkvT", a + "w_qs.weight"), d, 1), dz1)
        if B.qkv_dx == "gemm_raw":
            return (ops.linear_dx(dqkv, self._w(a + "w_qs.weight", 3 * d), raw=True), dz1)
        if B.qkv_dx == "qkv_dx":
            return ops.qkv_dx(dqkv, self._pack("qkvT", a + "w_qs.weight"), R=dz1)       # the first block of the stack: the same 32-row product as a kernel of its own
        return ops.linear_dx(dqkv, self._w(a + "w_qs.weight", 3 * d), R=dz1)

    def _predictor_bwd(self, pre, saved, dout, rng, R, train=True, need_dx=True):
        """`train` / `need_dx`: as for _fft_bwd."""
        (x, h1, m1, r1, a1, h2, m2, r2, Bn, Lp, lens, p, site) = saved
        d, rows = self.d, Bn * Lp
        c = pre + "conv_layer."
        Fh = h1.shape[-1]
        hw = self._m(pre + "linear_layer.weight")
        n_out = hw.shape[0]
        if n_out > 1:                   # the CWT pitch predictor: dout (B, L, 11)
            dh2, part, nblk = ops.layernorm_head_bwd(dout.contiguous().view(rows, n_out), hw, h2.view(rows, Fh), m2, r2,
                                                     self._m(c + "layer_norm_2.weight"), self._m(c + "layer_norm_2.bias"), lens, Lp,
                                                     p_post=p, site_post=site + 1, rng=rng)
        else:
            dh2, _, part, nblk = ops.layernorm_bwd(None, h2.view(rows, Fh), m2, r2, self._m(c + "layer_norm_2.weight"),
                                                   self._m(c + "layer_norm_2.bias"), lens, Lp, relu_in=True, p_post=p,
                                                   site_post=site + 1, rng=rng, dhead=dout.contiguous().view(-1), head_w=hw.view(-1))
        if train:
            self._finalize_ln(part, nblk, (3 + n_out) * Fh + n_out, c + "conv1d_2.conv.bias")
            ops.conv1d_dw(dh2.view(Bn, Lp, Fh), a1.view(Bn, Lp, Fh), self._g(c + "conv1d_2.conv.weight"), k=self.k_var, defer=self._deferred, accumulate=self._acc)
        da1 = ops.conv1d_dx(dh2.view(Bn, Lp, Fh), self._w(c + "conv1d_2.conv.weight"))
        dh1, _, part, nblk = ops.layernorm_bwd(da1.view(rows, Fh), h1.view(rows, Fh), m1, r1, self._m(c + "layer_norm_1.weight"),
                                               self._m(c + "layer_norm_1.bias"), None, 0, relu_in=True, p_post=p,
                                               site_post=site, rng=rng)
        if train:
            self._finalize_ln(part, nblk, 3 * Fh, c + "conv1d_1.conv.bias")
            ops.conv1d_dw(dh1.view(Bn, Lp, Fh), x.view(Bn, Lp, d), self._g(c + "conv1d_1.conv.weight"), k=self.k_var, defer=self._deferred, accumulate=self._acc)
        if not need_dx:
            return None
        return ops.conv1d_dx(dh1.view(Bn, Lp, Fh), self._w(c + "conv1d_1.conv.weight"), R=R)

    def _finalize_loss(self):
        if self._loss_finalize is not None:
            fin, self._loss_finalize = self._loss_finalize, None
            fin()

    def abort_step(self):
        """Forget the stream bookkeeping of a step whose Python ran only in part (a hipGraph capture of it was aborted)."""
        self._ctx = None
        self._dw_side_pending = False
        self._pred_fwd_pending = False
        self._var_on_pred, self._loss_finalize = False, None

    def backward_group_order(self):
        """The parameter groups in the order backward_native completes their gradients (= reverse forward order; the flat
        gradient buffer is laid out in forward order, so everything at or above a finished group's offset is final)."""
        return (["postnet", "mel_linear"] + ["decoder.%d" % i for i in range(self.n_dec - 1, -1, -1)] + ["variance_adaptor"] +
                ["encoder.%d" % i for i in range(self.n_enc - 1, -1, -1)] + ["embedding"])

    def _launch_dw_side(self, everything=False):
        """The weight-gradient work queued so far (PostNet, mel_linear, decoder, predictors), after the decoder's backward, on the second
        stream beside the encoder-side dX chain on the main stream: w_1's six gradients (dwconv, 192 workgroups = one per CU on 3/4 of
        the chip), then the other 256-multiple ones (dwgemm, grid capped at `dw_side_wgs`) with their slab reducer.  The column sums and
        the few 128 x 128-tile grouped problems (80-channel outputs) wait for the final phase (measured: beside dwconv / dwgemm their HBM
        traffic slows the whole step).
        `everything` (the data-parallel "side" schedule): nothing may stay queued — neither the share `dw_side_frac` leaves for the
        final flush nor those grouped problems: the caller reduces every split-K slab and announces the buckets right behind this."""
        if self._dw_side is None:
            self._dw_side = torch.cuda.Stream(device=self.device)
        self._dw_side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._dw_side):
            ops.stamp("side.start")
            self._deferred.flush_gemms(max_wgs=self.dw_side_wgs, frac=1.0 if everything else self.dw_side_frac, small_too=everything)
            ops.stamp("side.end")
        self._dw_side_pending = True

    def _mark_bucket(self, name):
        """The notifier's `mark` in the "side" / "late" data-parallel schedules: group `name` is complete once everything queued so far
        has been flushed — remember it for the announcement behind that flush."""
        self._dp_marks.append(name)

    def _launch_dw_side_buckets(self, on_bucket):
        """Data-parallel "side" schedule, after the decoder's backward: exactly the single-GPU schedule's second-stream work (`_launch_dw_side`:
        w_1's gradients on dwconv, the other 256-multiple ones on dwgemm with their slab reducer, the few grouped problems, the column
        sums — everything queued so far, so every PostNet / mel_linear / decoder gradient is final when it ends), and behind it, FROM THAT
        STREAM, the all-reduce of every bucket those groups complete — beside the encoder-side dX chain on the main stream, ahead of the
        final flush, which announces the encoder-side groups.  (Round 3 first cut this work at the bucket boundaries, a launch set per
        bucket: with dwconv / dwgemm covering all six blocks in one launch each that only added launches: 3.47 vs 3.09 ms on one GPU.)"""
        self._launch_dw_side(everything=True)
        q = self._deferred
        if q.group or q.dwconv or q.dwgemm:
            # a problem still queued would write its gradient (or its split-K slabs) AFTER the reduce / all-reduce below read them
            raise RuntimeError("data-parallel side schedule: %d grouped / %d dwconv / %d dwgemm weight-gradient problems still queued "
                               "before the buckets are announced" % (len(q.group), len(q.dwconv), len(q.dwgemm)))
        # the split-K slabs of the grouped problems just launched: summed here, not with the final flush (the buckets must be final)
        marks, self._dp_marks = self._dp_marks, []
        with torch.cuda.stream(self._dw_side):
            q.reduce_queued()
            if self._deferred_fin:                                  # the column sums queued so far belong to these buckets too
                q.keep.extend(k for _, k in self._deferred_fin)     # (read on this stream: alive until the queue's final flush)
                ops.flush_finalize(self._deferred_fin)
            for name in marks:
                on_bucket(name)               # groups in completion order: a bucket goes out when its lowest group has been announced
        self._dw_side_pending = True

    def _flush_param_grads(self):
        """Run the queued weight-gradient work (grouped dW GEMMs, split-K reducers, column sums, scatter-sums)."""
        if self._dw_side_pending and self._trainable is not None:
            # a subset step (set_trainable): what is still queued may be a few problems or none, so the three-way fork below could open
            # branches with nothing in them — the second stream is joined and the rest runs on this one
            torch.cuda.current_stream().wait_stream(self._dw_side)
            self._dw_side_pending = False
        if self._dw_side_pending:
            # The main stream gets here ~0.1 ms before the capped dW group on the side stream ends.  The column sums / scatter-sums read
            # only activations and gradients the main chain produced: they run now, beside the side stream; the encoder-side dW group
            # queues behind the first one on the side stream; the join comes last, before the split-K reducer.
            cur = torch.cuda.current_stream()
            launch = self._deferred.upload_gemms()     # the tables now, on this stream
            # Three branches from here (a replayed graph runs at most three queues side by side): the encoder blocks' w_1 gradients
            # (dwconv, 128 workgroups) and behind them the few grouped problems (80-channel outputs) on one stream; the encoder side's
            # dwgemm problems on the side stream (behind the decoder's work there); the column sums on this one.
            if self._fin_side is None:
                self._fin_side = torch.cuda.Stream(device=self.device)
            self._fin_side.wait_stream(cur)
            with torch.cuda.stream(self._fin_side):
                self._deferred.flush_dwconv()
                ops.stamp("fin.dwconv")
                launch()
                ops.stamp("fin.small")
            self._dw_side.wait_stream(cur)
            with torch.cuda.stream(self._dw_side):
                self._deferred.flush_dwgemm()
                ops.stamp("fin.dwgemm")
            ops.flush_finalize(self._deferred_fin)
            ops.stamp("fin.colsum")
            self._finalize_loss()       # the two-stream loss's values: behind the column sums, on the branch of the final phase that ends first
            cur.wait_stream(self._dw_side)
            cur.wait_stream(self._fin_side)
            self._dw_side_pending = False
        self._deferred.flush()
        ops.flush_finalize(self._deferred_fin)

    @staticmethod
    def _stack3(dlogd, dpitch, denergy):
        """(3, B, L) fp32 = (dlogd, dpitch, denergy).  ops.fs2_loss hands them out as the three slices of one buffer (no copy);
        gradients that arrive separately (the autograd bridge) are copied into one."""
        base = dlogd._base
        n = dlogd.numel()
        if (base is not None and dpitch._base is base and denergy._base is base and base.dim() == 3 and base.shape[0] == 3 and
                base.is_contiguous() and dlogd.data_ptr() == base.data_ptr() and dpitch.data_ptr() == base.data_ptr() + 4 * n and
                denergy.data_ptr() == base.data_ptr() + 8 * n):
            return base
        out = torch.empty((3,) + tuple(dlogd.shape), dtype=torch.float32, device=dlogd.device)
        for i, t in enumerate((dlogd, dpitch, denergy)):
            out[i].copy_(t)               # a device-to-device copy, no arithmetic
        return out

    def backward_native(self, ctx, dmel_sum, dpost, dpitch, denergy, dlogd, on_bucket=None, accumulate=None, dheads=None):
        """d(loss)/d(params) into the flat gradient buffer.
        dmel_sum = dL/dmel (direct terms) + dL/dpost, dpost = dL/dpost — fp32 (B,T,n_mel); dpitch/denergy/dlogd fp32 (B,L).
        CWT branch: dpitch is (B,L,11) and `dheads` (2,B) fp32 holds the gradients of the pitch_mean / pitch_std predictions.
        `on_bucket(name)` is called when the gradients of a top-level group are complete (data-parallel overlap).
        `accumulate`: True adds to what the buffer holds (the reference's `.grad +=`, train.py:43-44, micro-steps 2.. of a
        `grad_acc_step` cycle); False OVERWRITES every gradient element (the first micro-step after an update: the buffer need not be
        zero, so the optimizer's kernel need not zero it — 4 B per parameter less on the step's serial tail, and no read of the old
        value in the weight-gradient epilogues); None: whatever `grads_partial` says the buffer holds."""
        if ctx is None or ctx.used:
            raise RuntimeError("backward called without a matching training forward")
        ctx.used = True
        self._acc = bool(self.grads_partial if accumulate is None else accumulate)
        self.grads_partial = True
        rng = ops.rng_of(self._state())
        Bn, Lp, T = ctx.dims
        d, rows, nm = self.d, Bn * T, self.n_mel
        # split-K slabs of the weight-gradient GEMMs are summed by ONE batched reducer launch per parameter group when a
        # data-parallel reducer is waiting for finished buckets, otherwise once at the end (only Adam reads them)
        self._deferred = ops.DeferQueue()
        self._deferred_fin = []
        if self.dp_schedule not in ("side", "late"):
            raise ValueError("dp_schedule must be 'side' or 'late' (got %r)" % (self.dp_schedule,))
        dp_side = on_bucket is not None and self.dw_side_wgs > 0
        self._dp_marks = []
        # w_1's weight gradients on the tap-sharing kernel: one launch for the six decoder blocks (192 workgroups) and one for the encoder's;
        # not when buckets are flushed one by one (no second stream): those flushes would launch them two at a time
        self._use_dwconv = self.dwconv and (on_bucket is None or dp_side)
        notifier = _GroupNotifier(self.backward_group_order(), on_bucket, self._flush_param_grads, mark=self._mark_bucket if dp_side else None)
        notify = notifier.done
        # ---- trainable units (set_trainable): which parameter gradients are wanted, and how far down the input gradients must go.
        # With everything trainable every flag below is True and every stop index 0: the launches are today's.
        on = self._unit_on
        subset = self._trainable is not None
        if subset:
            if on_bucket is not None:
                raise NotImplementedError("train_only together with a gradient reducer is not supported (its buckets and group "
                                          "announcements assume every group completes)")
            notify = lambda name: None          # noqa: E731  (no reducer listens; groups that are skipped are never announced)
        dec_on = [on("decoder.%d" % i) for i in range(self.n_dec)]
        enc_on = [on("encoder.%d" % i) for i in range(self.n_enc)]
        pn_on, mel_on, va_on, spk_on, emb_on = on("postnet"), on("mel_linear"), on("variance_adaptor"), on("speaker_emb"), on("embedding")
        need_enc = emb_on or any(enc_on)                           # does anything of the encoder want a gradient?
        enc_stop = 0 if emb_on else (enc_on.index(True) if need_enc else self.n_enc)
        need_below = need_enc or va_on or spk_on                   # ... anything below the decoder?
        dec_stop = 0 if need_below else (dec_on.index(True) if any(dec_on) else self.n_dec)
        need_dec = need_below or any(dec_on)                       # does the decoder's backward run at all?
        need_mel = need_dec or mel_on                              # ... mel_linear's?
        # (arguments beyond today's only where a unit is frozen or a gradient stops: a full step calls the block functions as it always did)
        pkw = {} if (va_on and need_enc) else {"train": va_on, "need_dur_dx": need_enc}

        def bkw(train, need_dx):
            return {} if (train and need_dx) else {"train": train, "need_dx": need_dx}
        ops.stamp("bwd.start")
        # ---- the predictors' backward up to their input gradients, on a stream of its own beside the PostNet's (see pred_side); not in
        # the schedules that flush the deferred queue before the decoder is done; not at all when nothing below the decoder is trained
        pred_dxin = None
        if self.pred_side in ("1", "b") and "grouped" in ctx.preds and (on_bucket is None or dp_side) and need_below:
            if self._pred_stream is None:
                self._pred_stream = torch.cuda.Stream(device=self.device)
            if not self._var_on_pred:             # (the two-stream loss left dlogd / dpitch / denergy ON that stream: nothing of this one is needed)
                self._pred_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._pred_stream):
                pred_dxin = self._predictors_bwd_inputs(ctx.preds["grouped"], self._stack3(dlogd, dpitch, denergy), rng, **pkw)
        elif self._var_on_pred:                   # the predictors' backward runs on this stream: it needs the two-stream loss's other half
            torch.cuda.current_stream().wait_stream(self._pred_stream)
            self._finalize_loss()
        self._var_on_pred = False
        # ---- PostNet (last layer first)
        dout = dpost.view(rows, nm)
        dmel_tot = None
        bn_partials = None          # BatchNorm-backward statistics of layer i, when conv i+1's input-gradient kernel emitted them
        for i in range(4, -1, -1):
            pp, xin, yc, mean, rstd, keep = ctx.pn[i]
            C = yc.shape[2]
            dy = ops.bn_bwd(dout, yc.view(rows, C), mean, rstd, self._m(pp + "1.weight"), self._m(pp + "1.bias"), i < 4,
                            p=self.p_post, site=300 + i, rng=rng, dgamma=self._g(pp + "1.weight") if pn_on else None,
                            dbeta=self._g(pp + "1.bias") if pn_on else None,
                            frame_limit=ctx.frame_limit, keep=keep, accumulate=self._acc, partials=bn_partials)
            bn_partials = None
            if pn_on:
                ops.colsum_into(dy, self._g(pp + "0.conv.bias"), defer=self._deferred_fin, accumulate=self._acc)
                # (no `lens`: the PostNet's BatchNorm runs over the PAD rows too, Layers.py:133-143 — its gradients there are not zero)
                ops.queue_dw(self._deferred, dy.view(Bn, T, C), xin, self._g(pp + "0.conv.weight"), None, self._acc, k=5,
                             use_dwgemm=self._use_dwconv)
            route = ctx.plan.postnet[i].dx
            cw = self._table[pp + "0.conv.weight"].storage_shape
            if route == "gemm" and i > 0:
                dout = ops.conv1d_dx(dy.view(Bn, T, C), self._w(pp + "0.conv.weight")).view(rows, -1)
            elif i > 0:
                pkt = self._pack("pnT", pp + "0.conv.weight")
                pb, _, ycb, meanb, rstdb, keepb = ctx.pn[i - 1]
                if route == "win_bnb" and (keepb is not None or self.p_post == 0.0):
                    # ... which also sums the BatchNorm-backward statistics of the layer below over its output tile
                    dout, bn_partials = ops.win_conv_bnb(dy.view(Bn, T, C), pkt, cw[2], cw[1], ycb.view(rows, cw[2]), meanb, rstdb,
                                                         self._m(pb + "1.weight"), self._m(pb + "1.bias"), True, p=self.p_post, keep=keepb,
                                                         frame_limit=ctx.frame_limit)
                    dout = dout.view(rows, -1)
                else:
                    dout = ops.win_conv(dy.view(Bn, T, C), pkt, cw[2], cw[1]).view(rows, -1)   # dX as a forward conv on the transposed pack
            elif need_mel:
                if route == "win_resid":     # the first conv's input gradient (512 -> 80) + the mel terms' own gradient, on the window kernel
                    dmel_tot = ops.win_conv_resid(dy.view(Bn, T, C), self._pack("pnT", pp + "0.conv.weight"), dmel_sum.view(Bn, T, nm), cw[2], cw[1]).view(rows, nm)
                else:
                    dmel_tot = ops.conv1d_dx(dy.view(Bn, T, C), self._w(pp + "0.conv.weight"), R=dmel_sum.view(Bn, T, nm)).view(rows, nm)
                if ctx.frame_limit is not None:
                    ops.zero_frames_from(dmel_tot, ctx.frame_limit)      # the conv's reach past the batch's own length is not a frame
        notify("postnet")
        ops.stamp("bwd.postnet_done")
        # ---- mel_linear
        if mel_on:
            ops.colsum_into(dmel_tot, self._g("mel_linear.bias"), defer=self._deferred_fin, accumulate=self._acc)
            ops.linear_dw(dmel_tot, ctx.dec_out, self._g("mel_linear.weight"), defer=self._deferred, accumulate=self._acc)
        dx = None
        if need_dec:
            if ctx.plan.mel_dx == "win":
                dx = ops.win_conv(dmel_tot.view(Bn, T, nm), self._pack("linT", "mel_linear.weight"), d, 1).view(rows, d)      # mel_linear's input gradient: a k = 1 conv on the transposed pack
            else:
                dx = ops.linear_dx(dmel_tot, self._w("mel_linear.weight"))
        notify("mel_linear")
        # ---- decoder: down to the lowest block whose gradient anything wants
        for i in range(self.n_dec - 1, dec_stop - 1, -1):
            dx = self._fft_bwd(ctx.blocks[ctx.n_enc_blocks + i], dx, rng, raw_out=i > 0, **bkw(dec_on[i], need_below or i > dec_stop))
            notify("decoder.%d" % i)
        ops.stamp("bwd.decoder_done")
        if pred_dxin is not None:
            torch.cuda.current_stream().wait_stream(self._pred_stream)    # long done; its queued dW work joins the second stream's
        q = self._deferred
        if dp_side and self.dp_schedule == "side":
            self._launch_dw_side_buckets(on_bucket)
        elif self.dw_side_wgs > 0 and (not subset or (need_below and (q.group or q.dwconv or q.dwgemm))):
            # (a subset step opens the second stream only when it has work for it and a chain to run beside: no empty branch)
            self._launch_dw_side()
        if need_below:
            # ---- length regulator: segment sums (the position table has no parameters)
            dx3 = ops.length_regulator_bwd(dx.view(Bn, T, d), ctx.cs, Lp).view(Bn * Lp, d)
            # ---- variance adaptor, reverse order of modules.py:158-193
            va = "variance_adaptor."
            if va_on:
                ops.scatter_sum(dx3, ctx.eidx.view(-1), self._g(va + "energy_embedding.weight"), defer=self._deferred_fin, accumulate=self._acc)
            if "grouped" in ctx.preds:
                if pred_dxin is None and pkw:
                    pred_dxin = self._predictors_bwd_inputs(ctx.preds["grouped"], self._stack3(dlogd, dpitch, denergy), rng, **pkw)
                dx2, dx1, dxe = self._predictors_bwd_grouped(ctx.preds["grouped"], None if pred_dxin is not None else
                                                             self._stack3(dlogd, dpitch, denergy), rng, dx3, dxin=pred_dxin)
                if va_on:
                    ops.scatter_sum(dx2, ctx.pidx.view(-1), self._g(va + "pitch_embedding.weight"), defer=self._deferred_fin, accumulate=self._acc)
                if spk_on:
                    ops.scatter_sum(dx1, ctx.speakers, self._g("speaker_emb.weight"), idx_div=Lp, defer=self._deferred_fin, accumulate=self._acc)
            else:
                dx2 = self._predictor_bwd(va + "energy_predictor.", ctx.preds[va + "energy_predictor."], denergy, rng, dx3.view(Bn, Lp, d), **bkw(va_on, True))
                if va_on:
                    ops.scatter_sum(dx2.view(Bn * Lp, d), ctx.pidx.view(-1), self._g(va + "pitch_embedding.weight"), defer=self._deferred_fin, accumulate=self._acc)
                dx1 = self._predictor_bwd(va + "pitch_predictor.", ctx.preds[va + "pitch_predictor."], dpitch, rng, dx2, **bkw(va_on, True))
                if self.use_cwt:
                    # the heads read detached inputs (modules.py:118-119): parameter gradients only, from their own loss terms; the twenty
                    # tensors are one stretch of the flat buffer, summed over the utterances in order by the deferred finalize
                    if dheads is None:
                        raise RuntimeError("use_cwt: backward_native needs dheads (the gradients of the pitch_mean / pitch_std predictions)")
                    hk = va + "pitch_mean.flat_one.net.0.weight"
                    hpart = ops.cnnscalar_bwd(dheads, ctx.heads_saved, self._m(hk, 2 * ops.CNNSCALAR_FLOATS))
                    self._finalize_ln(hpart, Bn, 2 * ops.CNNSCALAR_FLOATS, hk)
                if spk_on:
                    ops.scatter_sum(dx1.view(Bn * Lp, d), ctx.speakers, self._g("speaker_emb.weight"), idx_div=Lp, defer=self._deferred_fin, accumulate=self._acc)
                dxe = None
                if va_on or need_enc:       # (the duration predictor's input gradient feeds nothing but the encoder)
                    dxe = self._predictor_bwd(va + "duration_predictor.", ctx.preds[va + "duration_predictor."], dlogd, rng, dx1,
                                              **bkw(va_on, need_enc))
        notify("variance_adaptor")
        # ---- encoder: down to the lowest block whose gradient anything wants
        if need_enc:
            dx = dxe.view(Bn * Lp, d)
            for i in range(self.n_enc - 1, enc_stop - 1, -1):
                dx = self._fft_bwd(ctx.blocks[i], dx, rng, raw_out=i > 0, **bkw(enc_on[i], emb_on or i > enc_stop))
                notify("encoder.%d" % i)
            if emb_on:
                ops.scatter_sum(dx, ctx.texts.view(-1), self._g("encoder.src_word_emb.weight"), skip_row=0, defer=self._deferred_fin, accumulate=self._acc)   # padding_idx=0
        notify("embedding")
        ops.stamp("bwd.chain_done")
        self._flush_param_grads()
        ops.stamp("bwd.flushed")
        if dp_side:
            for name in self._dp_marks:    # everything is in the buffer now: the remaining buckets, in completion order
                on_bucket(name)
            self._dp_marks = []
        self._finalize_loss()       # (a schedule without the second stream: here, where this stream has seen both halves of the loss)
        self._ctx = None


for _name in fs2_plan.TOGGLES:          # window_ffn, flash_attention, fused_ln, postnet_ends_win, dwconv
    setattr(FastSpeech2, _name, property(lambda self, n=_name: self._toggles[n], lambda self, on, n=_name: self._set_toggle(n, on)))
