"""Parameter inventory of FastSpeech2 with the reference's `state_dict` key names, and the flat storage
that backs it.

All trainable parameters live in ONE fp32 buffer (`flat`), their gradients in a second one of the same layout
(`flat_grad`) and their bf16 copies, which the MFMA kernels read, in a third (`shadow`).  Consequences:
gradient clipping is one norm over one buffer, Adam is one kernel launch, the data-parallel all-reduce works on
contiguous buckets, and the bf16 shadow is refreshed by the Adam kernel itself.

Conv1d weights are stored tap-major, (Cout, k, Cin), because the implicit-GEMM kernel wants the input channels
contiguous per tap; the `nn.Parameter` users see is a permuted VIEW with the reference's shape (Cout, Cin, k),
so `state_dict()` / `load_state_dict()` round-trip reference checkpoints without copies.
"""
from collections import OrderedDict

TRAIN, FROZEN, UNUSED, BUFFER = "train", "frozen", "unused", "buffer"


class Entry:
    __slots__ = ("key", "shape", "kind", "conv", "offset", "dtype")

    def __init__(self, key, shape, kind, conv=False, dtype="float32"):
        self.key, self.shape, self.kind, self.conv, self.dtype = key, tuple(shape), kind, conv, dtype
        self.offset = -1

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def storage_shape(self):
        """(Cout, k, Cin) for conv weights, the reference shape otherwise."""
        if self.conv:
            co, ci, k = self.shape
            return (co, k, ci)
        return self.shape


def _fft_block(pre, d, d_ff, k1, k2):
    a, f = pre + "slf_attn.", pre + "pos_ffn."
    return [
        Entry(a + "w_qs.weight", (d, d), TRAIN), Entry(a + "w_ks.weight", (d, d), TRAIN), Entry(a + "w_vs.weight", (d, d), TRAIN),
        Entry(a + "w_qs.bias", (d,), TRAIN), Entry(a + "w_ks.bias", (d,), TRAIN), Entry(a + "w_vs.bias", (d,), TRAIN),
        Entry(a + "fc.weight", (d, d), TRAIN), Entry(a + "fc.bias", (d,), TRAIN),
        Entry(a + "layer_norm.weight", (d,), TRAIN), Entry(a + "layer_norm.bias", (d,), TRAIN),
        Entry(f + "w_1.weight", (d_ff, d, k1), TRAIN, conv=True), Entry(f + "w_1.bias", (d_ff,), TRAIN),
        Entry(f + "w_2.weight", (d, d_ff, k2), TRAIN, conv=True), Entry(f + "w_2.bias", (d,), TRAIN),
        Entry(f + "layer_norm.weight", (d,), TRAIN), Entry(f + "layer_norm.bias", (d,), TRAIN),
    ]


def _predictor(pre, d, filt, k, n_out=1):
    c = pre + "conv_layer."
    return [
        Entry(c + "conv1d_1.conv.weight", (filt, d, k), TRAIN, conv=True), Entry(c + "conv1d_1.conv.bias", (filt,), TRAIN),
        Entry(c + "layer_norm_1.weight", (filt,), TRAIN), Entry(c + "layer_norm_1.bias", (filt,), TRAIN),
        Entry(c + "conv1d_2.conv.weight", (filt, filt, k), TRAIN, conv=True), Entry(c + "conv1d_2.conv.bias", (filt,), TRAIN),
        Entry(c + "layer_norm_2.weight", (filt,), TRAIN), Entry(c + "layer_norm_2.bias", (filt,), TRAIN),
        Entry(pre + "linear_layer.weight", (n_out, filt), TRAIN), Entry(pre + "linear_layer.bias", (n_out,), TRAIN),
    ]


CWT_CHANNELS = 11      # outputs of the CWT pitch predictor (reference: model/modules.py:27-29)


def _cnn_scalar(pre, size_one, size_two, reduce=30, kind=UNUSED):
    """CWT pitch mean/std heads (reference: model/modules.py:358-385).  `kind`: UNUSED (use_cwt False: the parameters exist, compute
    is off) or TRAIN (use_cwt True): then the ten tensors of a head sit back to back in the flat buffer, in this order, each at a
    multiple of 8 floats — the parameter block csrc/cwt.hip reads (include/ttsk.h: ttsk_cnnscalar_fwd).  The 1x1 conv weight
    (1, size, 1) is stored as it is: with one output channel and one tap the tap-major layout is the same memory."""
    out = []
    for name, size in (("flat_one", size_one), ("flat_two", size_two)):
        out += [Entry(pre + name + ".net.0.weight", (1, size, 1), kind), Entry(pre + name + ".net.0.bias", (1,), kind),
                Entry(pre + name + ".net.2.weight", (reduce,), kind), Entry(pre + name + ".net.2.bias", (reduce,), kind)]
    out += [Entry(pre + "linear.weight", (1, reduce), kind), Entry(pre + "linear.bias", (1,), kind)]
    return out


class ConfigError(ValueError):
    """A model / preprocess configuration the kernels have no instance for: names the key, its value and the accepted values."""

    def __init__(self, key, value, accepted):
        self.key, self.value, self.accepted = key, value, accepted
        super().__init__("%s = %r is not supported; accepted: %s" % (key, value, accepted))


FILTER_SIZES = (256, 512, 768, 1024)       # csrc/layernorm.hip: D = 256..1024 in steps of 256
# ... and of those the block widths whose every launch has an instance: at 768 / 1024 the q|k|v input gradient (a contraction over
# 3 d channels) would be 9 / 12 slabs of ttsk_win_conv_split, which takes at most 8, and no test runs the rest of their route
HIDDEN_SIZES = (256, 512)
MAX_KERNEL_SIZE = 15                       # csrc/dwgemm.hip: odd tap counts up to 15 (the window kernel: up to 9, else the implicit GEMM)
MAX_FILTER_SIZE = 1024                     # csrc/layernorm.hip: a bias gradient's column sum holds at most 1024 columns per pass


def validate_config(model_config, n_mel):
    """Refuse, by key, what the kernel entry points would refuse at the first forward or backward (each limit is the TTSK_REQUIRE
    or `*_supported` it cites).  Called by build_entries, so FastSpeech2.__init__ raises before it allocates anything."""
    tr, vp = model_config["transformer"], model_config["variance_predictor"]
    d = tr["encoder_hidden"]
    if d not in HIDDEN_SIZES:              # ttsk_layernorm_fwd / _bwd: "D must be 256..1024 step 256"; ttsk_win_conv_split: nsplit <= 8
        raise ConfigError("transformer.encoder_hidden", d, "one of %s" % (HIDDEN_SIZES,))
    for key in ("decoder_hidden", "variance_hidden"):      # one residual width from the embedding to mel_linear: no projection between the stacks
        if tr[key] != d:
            raise ConfigError("transformer." + key, tr[key], "the value of transformer.encoder_hidden (%d)" % d)
    for key in ("encoder_head", "decoder_head"):
        # the scores / P V GEMMs step from head to head by d_k elements: ttsk_gemm wants batch strides in multiples of 8
        h = tr[key]
        if not (isinstance(h, int) and h >= 1 and d % h == 0 and (d // h) % 8 == 0):
            raise ConfigError("transformer." + key, h, "a divisor of the hidden size %d that leaves a head size in multiples of 8 "
                              "(head size 128 runs flash attention, every other one the softmax route)" % d)
    for key in ("encoder_layer", "decoder_layer"):
        if not (isinstance(tr[key], int) and tr[key] >= 1):
            raise ConfigError("transformer." + key, tr[key], "an integer >= 1")
    ks = list(tr["conv_kernel_size"])
    if len(ks) != 2 or any((not isinstance(k, int)) or k < 1 or k % 2 == 0 or k > MAX_KERNEL_SIZE for k in ks):
        # "same" padding (k - 1) / 2 on both sides: SubLayers.py:82-93; an even k changes the sequence length in the reference itself
        raise ConfigError("transformer.conv_kernel_size", ks, "two odd kernel sizes in 1..%d" % MAX_KERNEL_SIZE)
    ff = tr["conv_filter_size"]
    if not (isinstance(ff, int) and 8 <= ff <= MAX_FILTER_SIZE and ff % 8 == 0):      # ttsk_gemm: 16-byte rows; ttsk_colsum: C <= 1024
        raise ConfigError("transformer.conv_filter_size", ff, "a multiple of 8 in 8..%d" % MAX_FILTER_SIZE)
    if vp["filter_size"] not in FILTER_SIZES:              # the predictors' LayerNorms: ttsk_layernorm_fwd_grouped / _fwd
        raise ConfigError("variance_predictor.filter_size", vp["filter_size"], "one of %s" % (FILTER_SIZES,))
    if vp["kernel_size"] != 3:
        # the reference pads the predictor's second conv by 1 whatever the kernel size (model/modules.py:290): with any other size its
        # own forward fails on the shortened sequence, so there is nothing to reproduce
        raise ConfigError("variance_predictor.kernel_size", vp["kernel_size"], "3 (the only size the reference's predictor runs with: its second conv pads by 1)")
    nb = model_config["variance_embedding"]["n_bins"]
    if not (isinstance(nb, int) and nb >= 2):              # ttsk_bucketize / ttsk_va_embed: at least one bin edge
        raise ConfigError("variance_embedding.n_bins", nb, "an integer >= 2")
    if not (isinstance(model_config["max_seq_len"], int) and model_config["max_seq_len"] >= 1):
        raise ConfigError("max_seq_len", model_config["max_seq_len"], "an integer >= 1")
    # mel rows are GEMM operands (mel_linear's output, the PostNet's ends: 16-byte rows of bf16 = 8 channels; ttsk_zero_frames_from
    # the same), the loss and BatchNorm take 4 at a time, a bias gradient's column sum at most 1024
    if not (isinstance(n_mel, int) and 8 <= n_mel <= 1024 and n_mel % 8 == 0):
        raise ConfigError("preprocessing.mel.n_mel_channels", n_mel, "a multiple of 8 in 8..1024")
    if model_config["use_cwt"] and (d != 256 or vp["filter_size"] != 256):
        # csrc/cwt.hip: the CNNscalar heads and the 11-output predictor head are built for 256 channels
        key, val = ("transformer.encoder_hidden", d) if d != 256 else ("variance_predictor.filter_size", vp["filter_size"])
        raise ConfigError(key, val, "256 when use_cwt is True (the CWT pitch kernels handle 256 channels)")


def build_entries(model_config, n_mel, n_speakers, n_vocab):
    """Entries in FORWARD order (the flat buffer follows it, so backward completes buckets from the end).
    reference shapes: fs_two/transformer/{Models,Layers,SubLayers}.py, fs_two/model/{fastspeech2,modules}.py.
    Raises ConfigError for a configuration the kernels cannot run (validate_config)."""
    validate_config(model_config, n_mel)
    tr = model_config["transformer"]
    d = tr["encoder_hidden"]
    d_ff = tr["conv_filter_size"]
    k1, k2 = tr["conv_kernel_size"]
    n_pos = model_config["max_seq_len"] + 1
    vp = model_config["variance_predictor"]
    n_bins = model_config["variance_embedding"]["n_bins"]
    e = [Entry("encoder.position_enc", (1, n_pos, d), FROZEN), Entry("encoder.src_word_emb.weight", (n_vocab, d), TRAIN)]
    for i in range(tr["encoder_layer"]):
        e += _fft_block("encoder.layer_stack.%d." % i, d, d_ff, k1, k2)
    e.append(Entry("speaker_emb.weight", (n_speakers, d), TRAIN))
    va = "variance_adaptor."
    cwt = bool(model_config["use_cwt"])
    for name in ("duration_predictor", "pitch_predictor", "energy_predictor"):
        e += _predictor(va + name + ".", d, vp["filter_size"], vp["kernel_size"], CWT_CHANNELS if (cwt and name == "pitch_predictor") else 1)
    hk = TRAIN if cwt else UNUSED
    e += _cnn_scalar(va + "pitch_mean.", d, CWT_CHANNELS, kind=hk) + _cnn_scalar(va + "pitch_std.", d, CWT_CHANNELS, kind=hk)
    e += [Entry(va + "pitch_bins", (n_bins - 1,), FROZEN), Entry(va + "energy_bins", (n_bins - 1,), FROZEN),
          Entry(va + "pitch_embedding.weight", (n_bins, d), TRAIN), Entry(va + "energy_embedding.weight", (n_bins, d), TRAIN),
          Entry("decoder.position_enc", (1, n_pos, d), FROZEN)]
    for i in range(tr["decoder_layer"]):
        e += _fft_block("decoder.layer_stack.%d." % i, d, d_ff, k1, k2)
    e += [Entry("mel_linear.weight", (n_mel, d), TRAIN), Entry("mel_linear.bias", (n_mel,), TRAIN)]
    chans = [n_mel, 512, 512, 512, 512, n_mel]                       # PostNet(): Layers.py:76-82
    for i in range(5):
        p = "postnet.convolutions.%d." % i
        ci, co = chans[i], chans[i + 1]
        e += [Entry(p + "0.conv.weight", (co, ci, 5), TRAIN, conv=True), Entry(p + "0.conv.bias", (co,), TRAIN),
              Entry(p + "1.weight", (co,), TRAIN), Entry(p + "1.bias", (co,), TRAIN),
              Entry(p + "1.running_mean", (co,), BUFFER), Entry(p + "1.running_var", (co,), BUFFER),
              Entry(p + "1.num_batches_tracked", (), BUFFER, dtype="int64")]
    return e


def layout(entries, align=8):
    """Assign flat offsets to the TRAIN entries (each aligned to `align` elements = 16 bytes of bf16).
    Returns (OrderedDict key -> Entry, total padded length)."""
    off = 0
    table = OrderedDict()
    for en in entries:
        if en.kind == TRAIN:
            en.offset = off
            off += (en.numel + align - 1) // align * align
        table[en.key] = en
    return table, off


def buckets(table, total, bucket_elems):
    """Contiguous [start, end) ranges of the flat gradient buffer, at most ~bucket_elems long, cut at parameter
    boundaries, listed from the END of the buffer (the order in which backward finishes them)."""
    cuts = sorted({en.offset for en in table.values() if en.kind == TRAIN} | {total})
    out, end = [], total
    start_candidates = cuts[:-1]
    i = len(start_candidates) - 1
    while end > 0:
        j = i
        while j > 0 and end - start_candidates[j - 1] <= bucket_elems:
            j -= 1
        start = start_candidates[j]
        out.append((start, end))
        end = start
        i = j - 1
    return out


def reference_parameter_keys(entries_table):
    """Keys in the order of the reference model's `model.parameters()` — the indices torch.optim.Adam's `state_dict()`
    uses (reference: fs_two/model/optimizer.py:10-15 builds Adam over `model.parameters()`, train.py:221 saves its
    `state_dict()`).  Order there (a module's own Parameters, then its children in registration order): encoder (position_enc, src_word_emb, layer_stack) ->
    variance_adaptor (own Parameters pitch_bins / energy_bins first, then predictors, pitch_mean / pitch_std,
    embeddings: model/modules.py:20-90) -> decoder -> mel_linear -> speaker_emb -> postnet (model/fastspeech2.py:21-41);
    inside a block w_qs, w_ks, w_vs, layer_norm, fc (SubLayers.py:14-29), each weight before its bias.
    BatchNorm running statistics are buffers, not parameters."""
    keys = [k for k, en in entries_table.items() if en.kind != BUFFER]

    def rank(k):
        parts = k.split(".")
        top = {"encoder": 0, "variance_adaptor": 1, "decoder": 2, "mel_linear": 3, "speaker_emb": 4, "postnet": 5}[parts[0]]
        r = [top]
        if parts[0] in ("encoder", "decoder"):
            if parts[1] == "position_enc":      # a Parameter of Encoder/Decoder itself: before the children's
                r += [0]
            elif parts[1] == "src_word_emb":
                r += [1]
            else:
                sub = parts[3] + "." + parts[4]
                order = ["slf_attn.w_qs", "slf_attn.w_ks", "slf_attn.w_vs", "slf_attn.layer_norm", "slf_attn.fc", "pos_ffn.w_1",
                         "pos_ffn.w_2", "pos_ffn.layer_norm"]
                r += [2, int(parts[2]), order.index(sub), 0 if parts[-1] == "weight" else 1]
        elif parts[0] == "variance_adaptor":
            names = ["pitch_bins", "energy_bins", "duration_predictor", "pitch_predictor", "energy_predictor", "pitch_mean", "pitch_std",
                     "pitch_embedding", "energy_embedding"]
            r += [names.index(parts[1])]
            if parts[1].endswith("_predictor"):
                sub = ".".join(parts[2:-1])
                order = ["conv_layer.conv1d_1.conv", "conv_layer.layer_norm_1", "conv_layer.conv1d_2.conv", "conv_layer.layer_norm_2", "linear_layer"]
                r += [order.index(sub), 0 if parts[-1] == "weight" else 1]
            elif parts[1] in ("pitch_mean", "pitch_std"):
                sub = ".".join(parts[2:-1])
                order = ["flat_one.net.0", "flat_one.net.2", "flat_two.net.0", "flat_two.net.2", "linear"]
                r += [order.index(sub), 0 if parts[-1] == "weight" else 1]
        elif parts[0] == "postnet":
            r += [int(parts[2]), int(parts[3]), 0 if parts[-1] == "weight" else 1]
        else:
            r += [0 if parts[-1] == "weight" else 1]
        return r
    return sorted(keys, key=rank)


# ------------------------------------------------------------------------------------------- trainable units (speaker adaptation)
# A unit is trained or frozen as a whole (FastSpeech2.set_trainable): the groups of FastSpeech2.backward_group_order() with the
# speaker table split out of the variance adaptor.  torch: requires_grad_(False) on everything else.
def unit_names(n_enc, n_dec):
    """The units in backward order (the order in which backward_native completes their gradients)."""
    return (["postnet", "mel_linear"] + ["decoder.%d" % i for i in range(n_dec - 1, -1, -1)] + ["variance_adaptor", "speaker_emb"] +
            ["encoder.%d" % i for i in range(n_enc - 1, -1, -1)] + ["embedding"])


def unit_of(key):
    """The unit a state_dict key belongs to (None: encoder.position_enc / decoder.position_enc, which belong to none)."""
    parts = key.split(".")
    if parts[0] in ("postnet", "mel_linear", "variance_adaptor", "speaker_emb"):
        return parts[0]
    if parts[0] in ("encoder", "decoder") and parts[1] == "layer_stack":
        return "%s.%s" % (parts[0], parts[2])
    if key == "encoder.src_word_emb.weight":
        return "embedding"
    return None


def parse_units(units, n_enc, n_dec):
    """`units` (None = everything, or an iterable of unit names; the prefixes "decoder" / "encoder" name every block of the stack) ->
    None when every unit is named, else a frozenset of unit names.  Unknown names and an empty selection raise."""
    if units is None:
        return None
    if isinstance(units, str):
        units = [units]
    valid = unit_names(n_enc, n_dec)
    out = set()
    for u in units:
        if u in ("decoder", "encoder"):
            out.update(v for v in valid if v.startswith(u + "."))
        elif u in valid:
            out.add(u)
        else:
            raise ValueError("unknown trainable unit %r; valid: %s (and the prefixes 'decoder', 'encoder')" % (u, ", ".join(valid)))
    if not out:
        raise ValueError("train_only names no unit; valid: %s (and the prefixes 'decoder', 'encoder')" % ", ".join(valid))
    return None if len(out) == len(valid) else frozenset(out)


def unit_ranges(table, total, units, align=8):
    """Sorted, merged [start, end) ranges of the flat buffer that hold the TRAIN entries of `units` (None: one range over everything),
    cut at entry boundaries with each entry's alignment padding included."""
    if units is None:
        return [(0, total)]
    out = []
    for key, en in table.items():
        if en.kind != TRAIN or unit_of(key) not in units:
            continue
        end = en.offset + (en.numel + align - 1) // align * align
        if out and out[-1][1] == en.offset:
            out[-1] = (out[-1][0], end)
        else:
            out.append((en.offset, end))
    return out
