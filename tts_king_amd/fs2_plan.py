"""Which kernel runs which site of FastSpeech2: `build_plan`, a pure function of the model's dimensions and its five kernel toggles.

The weight packs (`FastSpeech2._build_packs`), the forward, the backward, the optimizer's tables and `FastSpeech2.routes()` all read
the record it returns; nothing else decides a route.  No tensor is touched: every `ops.*_supported` is a host predicate of the library.
What depends on a call -- train / eval, batch size, whether a gradient is wanted, whether dropout drew a mask -- stays at the call
site, written against a field of this record."""
from collections import namedtuple

from . import ops

TOGGLES = ("window_ffn", "flash_attention", "fused_ln", "postnet_ends_win", "dwconv")
Toggles = namedtuple("Toggles", TOGGLES)
Dims = namedtuple("Dims", "d d_ff k1 k2 heads_enc heads_dec n_enc n_dec pred_filter pred_kernel n_mel use_cwt")

# One FFT block of a stack, per position (the first and the last block differ from the middle ones).  Forward: qkv "chained" (out of
# the previous block's win_ln_proj_fwd) | "win" | "gemm"; attn "flash" | "softmax"; fc_ln (fc + dropout + residual + LayerNorm) "win_ln" |
# "gemm_ln" | "split" (linear + layernorm_fwd); w1 "ffn" (ttsk_ffn_conv_fwd, d = 256) | "win" (d = 512) | "gemm"; w2_ln "win_ln_proj"
# (+ the next block's q|k|v) | "win_ln" | "gemm_ln" | "split".  Backward: w2_bwd (LayerNorm backward + w_2's dX) "ln_proj" (one launch;
# the only consumer of a "pre" hand-over) | "win" | "gemm"; w1_dx "win_split" | "gemm_raw" (split-K slabs either way); w1_dw "dwconv" |
# "queue" (per call: the step's `_use_dwconv`, B <= 64); fc_bwd (LayerNorm backward + fc's dX) "ln_proj" | "win" | "gemm", fc_delta: the
# attention backward's delta comes out of that kernel; qkv_dx (the q|k|v input gradient as handed to the block in front) "pre" (dqkv
# itself: that block's "ln_proj" multiplies by the weight) | "win_split" | "gemm_raw", the first block of a stack "qkv_dx" | "gemm"
Block = namedtuple("Block", "qkv attn fc_ln w1 w2_ln w2_bwd w1_dx w1_dw fc_bwd fc_delta qkv_dx")
# One PostNet layer.  conv (train) "win_stats" (BatchNorm partials out of the conv's epilogue) | "win" | "gemm"; conv_eval "win" | "gemm";
# bn (train) "slab" | "two_step"; dx "win_bnb" (+ the BatchNorm-backward partials of the layer below; per call: that layer kept its
# dropout bits or drew none) | "win" | "gemm", layer 0 "win_resid" | "gemm"
PostNetLayer = namedtuple("PostNetLayer", "conv conv_eval bn dx")
# mel_fwd: mel_linear in `_forward`, "win_dual" | "gemm"; mel_eval: in eval_back, "gemm"; mel_dx "win" | "gemm"; packs: what those routes
# read, in allocation order, each (tag, key, rows of a fused view over the following keys (q|k|v) or None, transposed with flipped taps,
# odd: the 80-channel ends, which Adam's tile walk cannot write)
Plan = namedtuple("Plan", "encoder decoder mel_fwd mel_eval mel_dx postnet packs")
Pack = namedtuple("Pack", "tag key fused_rows transpose odd")

POSTNET_C, POSTNET_K, POSTNET_LAYERS = 512, 5, 5        # PostNet(): Layers.py:76-82


def dims_of(model_config, n_mel):
    tr, vp = model_config["transformer"], model_config["variance_predictor"]
    k1, k2 = tr["conv_kernel_size"]
    return Dims(tr["encoder_hidden"], tr["conv_filter_size"], k1, k2, tr["encoder_head"], tr["decoder_head"], tr["encoder_layer"],
                tr["decoder_layer"], vp["filter_size"], vp["kernel_size"], n_mel, bool(model_config["use_cwt"]))


def build_plan(dims, t):
    """The `Plan` of a model of dimensions `dims` (a `Dims`) toggled as `t` (a `Toggles`)."""
    d, d_ff, k1, k2 = dims.d, dims.d_ff, dims.k1, dims.k2

    def win(cin, cout, k):
        return t.window_ffn and ops.win_conv_supported(cin, cout, k)

    # the window kernel's packs of a block's weights: as they are (forward), transposed with flipped taps (input gradients); w_1's and
    # q|k|v's input gradients contract over d_ff / 3 d channels in 256-channel slices (ops.win_conv_split)
    has = {"w1": win(d, d_ff, k1), "qkv": win(d, 3 * d, 1), "fcT": win(d, d, 1), "w2T": win(d, d_ff, k2),
           "w1T": d_ff % 256 == 0 and win(256, d, k1), "fc": t.window_ffn and ops.win_ln_supported(d, d),
           "w2": t.window_ffn and k2 == 1 and ops.win_ln_supported(d_ff, d), "qkvT": (3 * d) % 256 == 0 and win(256, d, 1)}
    fuse = t.fused_ln and d == 256               # the projection + LayerNorm kernels are built for 256 channels
    fuse_bwd = d == 256 and k2 == 1              # ... and so is ttsk_layernorm_bwd_proj

    def stack(n, heads):
        attn = "flash" if t.flash_attention and d // heads == 128 else "softmax"
        fc_bwd = "gemm" if not has["fcT"] else "ln_proj" if fuse_bwd else "win"
        shared = dict(attn=attn, fc_ln=("win_ln" if has["fc"] else "gemm_ln") if fuse else "split",
                      w1=("ffn" if d == 256 else "win") if has["w1"] else "gemm",
                      w2_bwd="gemm" if not (has["w2T"] and k2 == 1) else "ln_proj" if fuse_bwd and d_ff == 1024 else "win",
                      w1_dx="win_split" if has["w1T"] else "gemm_raw",
                      w1_dw="dwconv" if t.dwconv and ops.dwconv_supported(d_ff, d, k1) else "queue",
                      fc_bwd=fc_bwd, fc_delta=attn == "flash" and fc_bwd != "gemm")
        blocks = []
        for i in range(n):
            if not (fuse and k2 == 1):
                w2_ln = "split"
            elif not has["w2"]:
                w2_ln = "gemm_ln"
            else:
                w2_ln = "win_ln_proj" if has["qkv"] and i + 1 < n else "win_ln"
            if i == 0:
                qkv, qkv_dx = "win" if has["qkv"] else "gemm", "qkv_dx" if has["qkvT"] and d == 256 else "gemm"
            else:
                front = blocks[-1]                # the block that hands this one its q|k|v, and takes its input gradient
                qkv = "chained" if front.w2_ln == "win_ln_proj" else "win" if has["qkv"] else "gemm"
                qkv_dx = "gemm_raw" if not has["qkvT"] else "pre" if front.w2_bwd == "ln_proj" else "win_split"
            blocks.append(Block(qkv=qkv, w2_ln=w2_ln, qkv_dx=qkv_dx, **shared))
        return tuple(blocks)

    enc, dec = stack(dims.n_enc, dims.heads_enc), stack(dims.n_dec, dims.heads_dec)
    chans = [dims.n_mel] + [POSTNET_C] * (POSTNET_LAYERS - 1) + [dims.n_mel]
    postnet = []
    for i in range(POSTNET_LAYERS):
        cin, cout = chans[i], chans[i + 1]
        on = t.postnet_ends_win or 0 < i < POSTNET_LAYERS - 1
        fwd, bwd = on and win(cin, cout, POSTNET_K), on and win(cout, cin, POSTNET_K)
        if i == 0:
            dx = "win_resid" if bwd else "gemm"
        else:
            dx = "gemm" if not bwd else "win_bnb" if cout in (512, 80) and cin == 512 and ops.bn_slab_supported(cin) else "win"
        postnet.append(PostNetLayer(conv="gemm" if not fwd else "win_stats" if cin in (512, 80) and ops.bn_slab_supported(cout) else "win",
                                    conv_eval="win" if fwd else "gemm", bn="slab" if ops.bn_slab_supported(cout) else "two_step", dx=dx))
    lin, linT = t.postnet_ends_win and win(d, dims.n_mel, 1), t.postnet_ends_win and win(dims.n_mel, d, 1)

    pres = ["decoder.layer_stack.%d." % i for i in range(dims.n_dec)] + ["encoder.layer_stack.%d." % i for i in range(dims.n_enc)]
    packs = []
    for tag, leaf, rows in (("w1", "pos_ffn.w_1.weight", None), ("qkv", "slf_attn.w_qs.weight", 3 * d), ("fcT", "slf_attn.fc.weight", None),
                            ("w2T", "pos_ffn.w_2.weight", None), ("w1T", "pos_ffn.w_1.weight", None), ("fc", "slf_attn.fc.weight", None),
                            ("w2", "pos_ffn.w_2.weight", None), ("qkvT", "slf_attn.w_qs.weight", 3 * d)):
        if has[tag]:
            packs += [Pack(tag, p + leaf, rows, tag.endswith("T"), False) for p in pres]
    pn = "postnet.convolutions.%d.0.conv.weight"
    ends = (0, POSTNET_LAYERS - 1)
    packs += [Pack("pn", pn % i, None, False, False) for i, l in enumerate(postnet) if i not in ends and l.conv_eval == "win"]
    packs += [Pack("pnT", pn % i, None, True, False) for i, l in enumerate(postnet) if i not in ends and l.dx != "gemm"]
    for i in ends:
        packs += [Pack("pn", pn % i, None, False, True)] * (postnet[i].conv_eval == "win") + [Pack("pnT", pn % i, None, True, True)] * (postnet[i].dx != "gemm")
    packs += [Pack("lin", "mel_linear.weight", None, False, True)] * bool(lin) + [Pack("linT", "mel_linear.weight", None, True, True)] * bool(linT)
    return Plan(encoder=enc, decoder=dec, mel_fwd="win_dual" if lin else "gemm", mel_eval="gemm", mel_dx="win" if linT else "gemm",
                postnet=tuple(postnet), packs=tuple(packs))


def routes(plan):
    """The plan's route names per site as plain lists (per block, per PostNet layer), for tests and debugging."""
    out = {}
    for name, blocks in (("encoder", plan.encoder), ("decoder", plan.decoder)):
        out[name] = {f: [getattr(b, f) for b in blocks] for f in Block._fields}
    out["postnet"] = {f: [getattr(l, f) for l in plan.postnet] for f in PostNetLayer._fields}
    out["mel_linear"] = {"train": plan.mel_fwd, "eval": plan.mel_eval, "dx": plan.mel_dx}
    return out
