"""HiFi-GAN generator inference on MI355X (V1 and V3 configurations): the reference's `Generator(h)` surface (constructor, weight-normed
`state_dict` keys, `remove_weight_norm()`, `forward((B,80,T)) -> (B,1,T*prod(upsample_rates))`) over hand-written
gfx950 kernels.

reference: hifi/models.py:146-210 (Generator), :12-95 (ResBlock1), :98-143 (ResBlock2), hifiapi.py:11-52.

Activations are bf16 channels-last [B*len][C] (each conv is an implicit GEMM whose contraction index — the input
channel — is contiguous in memory), accumulation is fp32, weights are folded (weight-norm removed), repacked tap-major
and cast to bf16 once.  Forward only: the reference's generator is used for inference (hifiapi.py:32-33 `train`
raises).
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import ops
from . import resample
from . import switches
from . import windows
from .ops import bf16, f16

LRELU_SLOPE = 0.1          # reference: hifi/models.py:9


def get_padding(kernel_size, dilation=1):
    """reference: hifi/vocoder/utils.py:36-37."""
    return int((kernel_size * dilation - dilation) / 2)


# ---------------------------------------------------------------------------------------------------- which kernel runs what
# The kernel-family switches of a Generator: plain attributes, read by `Generator._plan()` and nowhere else.
TOGGLES = ("window_conv", "conv_pair", "conv_pair_small", "pair_ws", "pair_ws_min_tiles", "fused", "stream_upsample", "window_upsample",
           "loop_upsample", "mrf_fused", "resblock2_fused")
_Toggles = namedtuple("_Toggles", TOGGLES)
# conv_pre: "win" | "gemm"; conv_post: "fused" (inside the mrf32_post launch) | "stream" | "gemm"; refusal: None, or why `_prepare` raises
_Plan = namedtuple("_Plan", "key c0 conv_pre stages conv_post refusal")
# One upsampler + MRF stage.  C: its channels; ups: "loop" | "win" | "stream" | "gemm"; act_copy: the upsampler also writes lrelu(x);
# route: "resblock2" | "pair" | "fused" | "mrf32_post" | "gemm"; gemm (that route only): "window" | "lockstep" | "blocks";
# fused_for: kernel sizes of a pair stage that go to the six-conv kernel; nxt_slope: the LeakyReLU of whatever reads the stage's output
_Stage = namedtuple("_Stage", "C stride ksize ups act_copy route gemm fused_for nxt_slope ws_min_tiles blocks")
# One ResBlock.  win (gemm route): its convs on the window kernel; ws_ok (pair route, None = never): frames per utterance -> the
# weights-stationary kernel has an instance and its 32-bit offsets reach
_Block = namedtuple("_Block", "kind k dilation win ws_ok")
K_PRE = K_POST = 7          # conv_pre / conv_post kernel size, hard-coded in the reference (hifi/models.py:152, :183)
# The weight packs of a plan (`Generator._prepare`).  pre / post: (weight, bias); per stage ups: (weight, bias) as its planned upsampler
# reads them, blocks: per ResBlock what its planned route reads
_Packs = namedtuple("_Packs", "key plan pre stages post")
_StagePacks = namedtuple("_StagePacks", "ups blocks")


def build_plan(h, dt, t, key=None):
    """Which kernel runs conv_pre, every upsampler, every MRF stage and conv_post: a pure function of the configuration `h`, the storage
    type `dt` and the toggles `t` (a `_Toggles`).  No tensor is touched: every `ops.hifi_*_supported` is a host predicate of the library.
    The weight packs (`Generator._prepare`), `forward_ntc`, `stage_routes()` and `short_rows()` all read the record this returns."""
    c0, kind, n_up = int(h.upsample_initial_channel), str(h.resblock), len(h.upsample_rates)
    kds = [(int(k), tuple(d)) for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes)]
    ks, nk = [k for k, _ in kds], len(kds)
    win16 = t.window_upsample and dt == torch.float16            # conv_pre and the upsamplers on the window-conv kernels: fp16 instances only
    stages, refusal = [], None
    for i, (u, ku) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
        u, ku, Cin, C = int(u), int(ku), c0 // 2 ** i, c0 // 2 ** (i + 1)
        six = kind == "1" and all(ops.hifi_resblock1_supported(C, k) for k in ks)          # the six-conv fused kernel covers every block
        # C = 32: the fused kernel is as fast or faster for every kernel size (86 / 143 / 181 us against 102 / 139 / 178)
        want_pair = (t.conv_pair and t.window_conv) if C >= 128 else (t.conv_pair_small and t.fused and C == 64)
        if t.resblock2_fused and nk >= 2 and kind == "2" and all(len(d) == 2 and ops.hifi_resblock2_supported(C, k, *d) for k, d in kds):
            route = "resblock2"
        elif want_pair and nk >= 2 and kind == "1" and all(ops.hifi_conv_pair_supported(C, k, dd) for k, d in kds for dd in d):
            route = "pair"
        elif t.fused and nk >= 2 and six:
            # the whole last stage — three blocks, their average, LeakyReLU(0.01), conv_post, tanh — in one launch
            last = t.mrf_fused and i + 1 == n_up and ops.hifi_mrf32_post_supported(C, ks, K_POST)
            route = "mrf32_post" if last else "fused"
        else:
            route = "gemm"
            if nk != 3 and refusal is None:
                refusal = ("HiFi-GAN stage %d runs conv by conv, where the MRF average is written for 3 resblock kernels per stage "
                           "(got %d)" % (i, nk))
        # as measured and shipped: the fused and mrf32_post routes choose their upsampler from {stream, gemm} only, the pair and
        # resblock2 routes from {loop, win, stream, gemm}; the conv-by-conv route needs the polyphase GEMMs' second, activated output
        if route in ("pair", "resblock2") and win16 and ops.hifi_upsample_win_supported(Cin, C, u, ku):
            ups = "loop" if t.loop_upsample and ops.hifi_upsample_loop_supported(Cin, C, u, ku) else "win"
        elif route != "gemm" and t.stream_upsample and ops.hifi_upsample2_supported(Cin, C, u, ku):
            ups = "stream"
        else:
            ups = "gemm"
        # conv by conv: the window kernel where it has an instance (C = 128), else every block's conv m as one grouped launch (equal
        # dilation counts), else block after block
        win = [route == "gemm" and t.window_conv and kind == "1" and all(ops.hifi_conv_window_supported(C, k, dd) for dd in d) for k, d in kds]
        gemm = None
        if route == "gemm":
            gemm = "window" if all(win) else "lockstep" if kind == "1" and len({len(d) for _, d in kds}) == 1 else "blocks"
            if gemm == "lockstep":
                win = [False] * nk

        def ws_ok(k, d, C=C):           # the predicate also bounds the utterance length, which only a call knows
            return lambda ln: all(ops.hifi_conv_pair_ws_supported(C, k, dd, ln) for dd in d)

        blocks = tuple(_Block(kind, k, d, w, ws_ok(k, d) if route == "pair" and t.pair_ws else None) for (k, d), w in zip(kds, win))
        # measured per block at the bench shape (tools/debug/convpair_micro.py): three pair launches beat the six-conv fused kernel at
        # C = 64 for k = 7, 11 (228 vs 242 us, 290 vs 370 us) and lose at k = 3 (158 vs 141 us: the block is then bound by its HBM
        # passes, and the fused kernel makes one instead of three)
        fused_for = (3,) if route == "pair" and C == 64 and six else ()
        # slope of the activation that consumes this stage's output: 0.1 before the next upsampler, F.leaky_relu's default 0.01 before
        # conv_post (hifi/models.py:197)
        stages.append(_Stage(C, u, ku, ups, route == "gemm", route, gemm, fused_for, LRELU_SLOPE if i + 1 < n_up else 0.01,
                             t.pair_ws_min_tiles, blocks))
    conv_pre = "win" if win16 and ops.hifi_conv_pre_win_supported(80, c0, K_PRE) else "gemm"
    conv_post = "fused" if stages and stages[-1].route == "mrf32_post" else "stream" if c0 // 2 ** n_up <= 128 else "gemm"
    return _Plan(key, c0, conv_pre, tuple(stages), conv_post, refusal)


def _dense(t, stage):
    """A stage's input is a fresh `torch.empty` output of an `ops` wrapper (conv1d, hifi_conv_pre_win, avg3, the MRF kernels' `out`; the
    upsamplers' outputs likewise), and the planned kernels index it densely: anything else is refused, there are no fall-back packs."""
    if not t.is_contiguous():
        raise ops.L.TtskError("HiFi-GAN stage %d: the activation tensor is not contiguous" % stage)
    return t


class _WNConv(nn.Module):
    """Parameter holder for one weight-normed Conv1d / ConvTranspose1d with the reference's key names:
    `weight_g`, `weight_v`, `bias` before `remove_weight_norm()`, `weight`, `bias` after."""

    def __init__(self, shape, n_bias):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(n_bias), requires_grad=False)          # reference key order: bias, weight_g, weight_v
        self.weight_g = nn.Parameter(torch.ones(shape[0], 1, 1), requires_grad=False)
        self.weight_v = nn.Parameter(torch.zeros(shape), requires_grad=False)

    def fold(self):
        if "weight_g" not in self._parameters:
            return
        g, v = self.weight_g, self.weight_v
        if v.is_cuda:
            w = ops.weight_norm_fold(v.data, g.data.view(-1))
        else:   # folding before .to(device): plain tensor math on the host (load-time only, not the hot path)
            w = v.data * (g.data / v.data.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1))
        del self._parameters["weight_g"], self._parameters["weight_v"]
        self.weight = nn.Parameter(w, requires_grad=False)

    def folded_weight(self):
        if "weight" in self._parameters:
            return self.weight.data
        if not self.weight_v.is_cuda:
            raise ops.L.TtskError("HiFi-GAN generator needs its weights on a HIP device")
        return ops.weight_norm_fold(self.weight_v.data, self.weight_g.data.view(-1))


class _ResBlock(nn.Module):
    """ResBlock1 (three (dilated, plain) conv pairs) or ResBlock2 (two dilated convs).
    reference: hifi/models.py:12-95, :98-143."""

    def __init__(self, channels, kernel_size, dilation, kind):
        super().__init__()
        self.kind, self.k, self.dilation = kind, kernel_size, tuple(dilation)
        mk = lambda: _WNConv((channels, channels, kernel_size), channels)
        if kind == "1":
            self.convs1 = nn.ModuleList([mk() for _ in self.dilation])
            self.convs2 = nn.ModuleList([mk() for _ in self.dilation])
        else:
            self.convs = nn.ModuleList([mk() for _ in self.dilation])

    def all_convs(self):
        return (list(self.convs1) + list(self.convs2)) if self.kind == "1" else list(self.convs)

    def remove_weight_norm(self):
        for c in self.all_convs():
            c.fold()


class Generator(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            ops.check_upsampler(int(k), int(u), "HiFi-GAN upsampler %d" % i)
        c0 = h.upsample_initial_channel
        self.conv_pre = _WNConv((c0, 80, K_PRE), c0)                       # 80 is hard-coded in the reference (:152)
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            self.ups.append(_WNConv((c0 // (2 ** i), c0 // (2 ** (i + 1)), k), c0 // (2 ** (i + 1))))
        self.resblocks = nn.ModuleList()
        ch = c0
        for i in range(self.num_upsamples):
            ch = c0 // (2 ** (i + 1))
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(_ResBlock(ch, k, d, str(h.resblock)))
        self.conv_post = _WNConv((1, ch, K_POST), 1)
        self._packed = None           # weight packs in kernel layouts (`_prepare`)
        self._plan_memo = None        # (`_plan`)
        self.act_dtype = f16         # storage type of activations and packed weights (fp32 accumulate); bf16 also works
        self.window_conv = True      # window-conv kernel at the C = 128 stage; False = implicit-GEMM convs
        self.conv_pair = True        # each (c1, c2) pair of a ResBlock1 as one launch (ttsk_hifi_conv_pair) at C = 128 ...
        self.conv_pair_small = True  # ... and at C = 64 / 32, instead of the six-conv fused kernel
        self.pair_ws = True          # the pairs on the weights-stationary persistent kernel (csrc/pairws.hip, round 6): C = 64 every kernel size, C = 128 k = 3
        self.pair_ws_min_tiles = 1024    # ... for stage tensors of at least this many of its tiles (192 frames at C = 64, 96 at C = 128)
        self.fused = True            # fused ResBlock1 kernel where an instance exists (C in {32,64}); False = conv-by-conv
        self.stream_upsample = True  # stride-2 upsamplers (128->64, 64->32) on the streaming kernel; False = polyphase implicit GEMMs
        self.window_upsample = switches.get("TTSK_HIFI_UPS8") != "0"   # stride-8 upsamplers and 128 -> 64 on the window-conv kernel (fp16); 0 = polyphase GEMMs / streaming kernel
        self.loop_upsample = True         # the 256 -> 128 upsampler on ups_loop_kernel (False: win_conv_kernel, one channel group per workgroup)
        self.mrf_fused = True        # the last stage (C = 32: three ResBlock1s + average + LeakyReLU + conv_post + tanh) as ONE launch (csrc/mrf32.hip)
        self.resblock2_fused = True  # each ResBlock2 (V3) as ONE launch with the MRF average folded in (csrc/resblock2.hip); False = conv by conv

    # ------------------------------------------------------------------ reference surface
    def remove_weight_norm(self):
        """reference: hifi/models.py:203-210 — fold g*v/||v|| into `weight`; keys lose `_g/_v`."""
        for l in self.ups:
            l.fold()
        for l in self.resblocks:
            l.remove_weight_norm()
        self.conv_pre.fold()
        self.conv_post.fold()
        self._packed = None

    def reset_parameters(self, seed=1234):
        """Seeded random init (weights_path: null): tts_king_amd.synthetic.seeded_fill statistics."""
        from .synthetic import seeded_fill
        sd = self.state_dict()
        cpu = {k: torch.zeros(v.shape, dtype=v.dtype) for k, v in sd.items()}
        seeded_fill(cpu, seed)
        with torch.no_grad():
            for k, v in sd.items():
                v.copy_(cpu[k])
        self._packed = None

    def _all_convs(self):
        out = [self.conv_pre] + list(self.ups)
        for rb in self.resblocks:
            out += rb.all_convs()
        return out + [self.conv_post]

    def _weights_key(self):
        return tuple((id(p), p._version) for c in self._all_convs() for p in c._parameters.values())

    def _plan(self, refuse=True):
        """`build_plan` for this generator as it is toggled now: rebuilt when `act_dtype` or one of TOGGLES changed since the last call, the
        same object otherwise.  Needs no device.  `refuse`: raise the plan's refusal (NotImplementedError naming the stage), if any."""
        key = (self.act_dtype,) + tuple(getattr(self, n) for n in TOGGLES)
        if self._plan_memo is None or self._plan_memo.key != key:
            self._plan_memo = build_plan(self.h, key[0], _Toggles(*key[1:]), key)
        if refuse and self._plan_memo.refusal:
            raise NotImplementedError(self._plan_memo.refusal)
        return self._plan_memo

    def _prepare(self):
        """16-bit copies of the folded weights in the layouts the planned kernels read (tap-major for the implicit-GEMM convs and the
        streaming kernels, MFMA-fragment-major for the window, pair and fused kernels), stage by stage: rebuilt when a parameter was
        written or the plan changed, otherwise the same objects with no allocation and no launch (captured graphs hold their addresses)."""
        plan = self._plan()
        key = (self._weights_key(), plan.key)
        if self._packed is not None and self._packed.key == key:
            return self._packed
        dt = self.act_dtype
        tap = lambda c, transposed=False: ops.pack_conv_weight(c.folded_weight(), transposed=transposed, dtype=dt)
        frag = lambda c: ops.pack_resblock_weight(c.folded_weight(), dtype=dt)
        pre = tap(self.conv_pre)
        if plan.conv_pre == "win":
            pre = ops.hifi_conv_pre_win_pack(pre)
        rbs, stages = iter(self.resblocks), []
        for st, up in zip(plan.stages, self.ups):
            ups = (tap(up, True), up.bias.data)
            if st.ups in ("loop", "win"):       # a two-tap conv over the input frames with stride * Cout phase-major channels
                ups = ops.hifi_upsample_win_pack(ups[0], ups[1], st.stride)
            blocks = []
            for blk, rb in zip(st.blocks, rbs):
                convs = rb.all_convs()
                if st.route == "gemm":          # ([(tap-major weight, bias)] convs1 then convs2, the window kernel's packs or None)
                    blocks.append(([(tap(c), c.bias.data) for c in convs], [frag(c) for c in convs] if blk.win else None))
                    continue
                if rb.kind == "1":              # launch order: c1_0, c2_0, c1_1, c2_1, ...
                    n = len(rb.dilation)
                    convs = [convs[m // 2 + (n if m % 2 else 0)] for m in range(2 * n)]
                blocks.append(([frag(c) for c in convs], [c.bias.data for c in convs]))
            stages.append(_StagePacks(ups, blocks))
        self._packed = _Packs(key, plan, (pre, self.conv_pre.bias.data), stages, (tap(self.conv_post), self.conv_post.bias.data))
        return self._packed

    # ------------------------------------------------------------------ forward
    def _resblock(self, rb, packed, x, xl, wpacks=None):
        """reference: hifi/models.py:88-95 (ResBlock1) / :136-140 (ResBlock2), conv by conv on the implicit-GEMM kernel, or (`wpacks`:
        ResBlock1 at C = 128) on the window kernel.  x = block input, xl = lrelu(x).  Every LeakyReLU is applied by the PRODUCING conv's
        epilogue (LRELU_OUT, or a second output C2 = lrelu(v) next to the raw v the residual path needs), the residual add is an epilogue
        too."""
        nd = len(rb.dilation)
        for m, d in enumerate(rb.dilation):
            lastp = m == nd - 1
            xl_next = None if lastp else torch.empty_like(x)
            if wpacks is not None:
                # one window-conv launch per conv (activation window in LDS, weights streamed)
                tl = ops.hifi_conv_window(xl, wpacks[m], packed[m][1], rb.k, d, lrelu_out=True, slope=LRELU_SLOPE)
                x = ops.hifi_conv_window(tl, wpacks[nd + m], packed[nd + m][1], rb.k, 1, R=x, out2=xl_next, slope=LRELU_SLOPE)
            elif rb.kind == "1":
                w1, b1 = packed[m]
                w2, b2 = packed[nd + m]
                tl = ops.conv1d(xl, w1, b1, dilation=d, flags=ops.LRELU_OUT, out_slope=LRELU_SLOPE)
                x = ops.conv1d(tl, w2, b2, R=x, C2=xl_next, flags=0 if lastp else ops.C2_LRELU, out_slope=LRELU_SLOPE)
            else:
                w, b = packed[m]
                x = ops.conv1d(xl, w, b, dilation=d, R=x, C2=xl_next, flags=0 if lastp else ops.C2_LRELU, out_slope=LRELU_SLOPE)
            xl = xl_next
        return x

    def _mrf_blocks(self, st, packs, a, rows=None):
        """The resblock2, fused and pair routes: the stage's ResBlocks on kernels that fold the MRF average (hifi/models.py:190-197) into their
        epilogue.  Every block's (last) launch adds into `out` (modes 0 / 1 / 2), the last block's scales by 1/num_kernels and applies the
        consumer's LeakyReLU.  a = the raw upsampler output: the kernels activate it themselves.  packs[j] = (weight packs, biases) in launch
        order.  Pair route (per block three launches, each c1 dilated -> lrelu -> c2 -> + x): blocks whose kernel size is in `st.fused_for`
        run on the six-conv fused kernel instead (same packs, same modes), unless the weights-stationary kernel takes them.
        `rows`: per-row lengths (ops._row_args): the kernels store nothing past a row's end, so `out` starts as zeros — what the next
        upsampler must read there."""
        nk = len(st.blocks)
        out = torch.empty_like(a) if rows is None else torch.zeros_like(a)
        # the persistent kernel walks runs of 192-frame tiles (96 at C = 128), one workgroup per CU, and pays a pipeline fill and drain of one tile each per
        # launch: worth it from ~4 tiles per CU on (the bench batch: 8); one utterance of 5 s is 299 tiles at the last stage and stays on the round-5 kernels
        tt = ops.hifi_conv_pair_ws_tile(st.C)
        tiles = a.shape[0] * ((a.shape[1] + tt - 1) // tt)
        for j, (blk, (ws, bs)) in enumerate(zip(st.blocks, packs)):
            last = j == nk - 1
            mrf = dict(mode=0 if j == 0 else (2 if last else 1), scale=1.0 / nk, final_slope=st.nxt_slope if last else 1.0)
            if st.route == "resblock2":
                ops.hifi_resblock2(a, ws[0], bs[0], ws[1], bs[1], blk.k, blk.dilation, slope=LRELU_SLOPE, out=out, rows=rows, **mrf)
                continue
            ws_kernel = blk.ws_ok is not None and tiles >= st.ws_min_tiles and blk.ws_ok(a.shape[1])
            if st.route == "fused" or (blk.k in st.fused_for and not ws_kernel):
                ops.hifi_resblock1(a, ws, bs, blk.dilation, out, blk.k, slope=LRELU_SLOPE, rows=rows, **mrf)
                continue
            x, nd = a, len(blk.dilation)
            for m, d in enumerate(blk.dilation):
                kw = dict(out=out, **mrf) if m == nd - 1 else {}
                x = ops.hifi_conv_pair(x, ws[2 * m], bs[2 * m], ws[2 * m + 1], bs[2 * m + 1], blk.k, d, slope=LRELU_SLOPE, ws=ws_kernel, rows=rows, **kw)
        return out

    def _resblocks_lockstep(self, rbs, packs, x, xl):
        """The stage's ResBlock1s (one per MRF kernel size, hifi/models.py:190-196) advanced conv by conv TOGETHER: they read
        the same stage input and never each other's outputs, so conv m of every block is one grouped launch (three 192-
        workgroup problems at the C = 256 stage -> one 576-workgroup grid).  Same epilogue fusions as `_resblock`."""
        nd = len(rbs[0].dilation)
        xs, xls = [x] * len(rbs), [xl] * len(rbs)
        for m in range(nd):
            lastp = m == nd - 1
            g1, tls = ops.GemmGroup(), []
            for rb, pk, xlj in zip(rbs, packs, xls):
                tls.append(ops.conv1d(xlj, pk[m][0], pk[m][1], dilation=rb.dilation[m], flags=ops.LRELU_OUT, out_slope=LRELU_SLOPE, group=g1))
            g1.flush()
            g2, nxt = ops.GemmGroup(), []
            for j, (rb, pk) in enumerate(zip(rbs, packs)):
                xl_next = None if lastp else torch.empty_like(x)
                xs[j] = ops.conv1d(tls[j], pk[nd + m][0], pk[nd + m][1], R=xs[j], C2=xl_next, flags=0 if lastp else ops.C2_LRELU,
                                   out_slope=LRELU_SLOPE, group=g2)
                nxt.append(xl_next)
            g2.flush()
            xls = nxt
        return xs

    def _upsample(self, st, packs, al):
        """ConvTranspose1d of a stage (hifi/models.py:189) on its planned kernel -> (x, lrelu(x) where the plan asks for that copy, else None):
        the looped / window kernels (fp16: stride 8 from 256 / 512 channels, 128 -> 64 at stride 2), the streaming stride-2 kernel (both
        phases from one read of `al`), else the polyphase implicit GEMMs."""
        w, b = packs
        if st.ups == "loop":
            return ops.hifi_upsample_loop(al, w, b, st.C, st.stride), None       # 256 -> 128: channel groups looped per frame tile
        if st.ups == "win":
            return ops.hifi_upsample_win(al, w, b, st.C, st.stride), None
        if st.ups == "stream":
            return ops.hifi_upsample2(al, w, b), None
        if not st.act_copy:
            return ops.conv_transpose1d(al, w, b, st.stride, st.ksize), None
        axl = torch.empty(al.shape[0], al.shape[1] * st.stride, st.C, dtype=al.dtype, device=al.device)
        return ops.conv_transpose1d(al, w, b, st.stride, st.ksize, C2=axl, flags=ops.C2_LRELU, out_slope=LRELU_SLOPE), axl

    _stage_marks = None     # bench.py's per-stage timing: a list to which forward appends (name, HIP event) at stage boundaries

    def _mark(self, name):
        if self._stage_marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._stage_marks.append((name, ev))

    def forward(self, x):
        """x (B, 80, T) mel on a HIP device -> (B, 1, T*prod(upsample_rates)) fp32.  reference: hifi/models.py:185-201.

        Dataflow: `al` always holds LeakyReLU(stage output) — the only thing the next ConvTranspose1d / conv_post reads
        (hifi/models.py:188,197) — produced by conv_pre's epilogue, then by the MRF average of each stage."""
        if not x.is_cuda:
            raise ops.L.TtskError("HiFi-GAN Generator.forward needs a HIP device tensor (gpu: 'cuda:0'); there is no CPU path")
        pk = self._prepare()
        with torch.no_grad():
            self._mark("start")
            a0 = ops.nct_to_ntc(x.float(), self.act_dtype)                                 # (B, T, 80) 16-bit
            return self.forward_ntc(a0, pk)

    def forward_ntc(self, a0, pk=None, row_frames=None):
        """`forward` from the channels-last 16-bit mel on: a0 (B, T, 80) in `act_dtype`, what `ops.nct_to_ntc` and `ops.mel_windows` write.

        `row_frames` (1-D int32 device tensor or view of B entries, e.g. column `windows.VALID` of a plan table; needs `short_rows()`):
        row b holds an utterance of row_frames[b] frames (0 = all T) and its waveform is what the utterance gives alone — at a stage
        with s samples per frame the positions >= row_frames[b] * s are zero padding for every conv.  a0 must be zero
        there (ttsk_mel_windows writes it so); the samples of the output past a row's end are unspecified.

        Every kernel is the plan's; only what depends on the shapes is decided here (`rows`, the weights-stationary pair kernel)."""
        if pk is None:
            pk = self._prepare()
        plan, rows, spf = pk.plan, None, 1
        with torch.no_grad():
            w, b = pk.pre
            if plan.conv_pre == "win":
                al = ops.hifi_conv_pre_win(a0, w, b, plan.c0, K_PRE, LRELU_SLOPE)             # lrelu(conv_pre(x)), window kernel
            else:
                al = ops.conv1d(a0, w, b, flags=ops.LRELU_OUT, out_slope=LRELU_SLOPE)
            if row_frames is not None:
                # conv_pre and the upsamplers know no row length: what conv_pre leaves past a row's end (bias, the taps that reach back)
                # is zeroed here, every MRF stage below masks its reads of the upsampler's output and hands on zeros past the end
                ops.zero_rows_past(al, (row_frames, 1))
            for i, (st, sp) in enumerate(zip(plan.stages, pk.stages)):
                self._mark("conv_pre" if i == 0 else "mrf%d" % (i - 1))
                spf *= st.stride
                if row_frames is not None:
                    if st.route == "gemm":
                        raise ops.L.TtskError("HiFi-GAN stage %d runs conv by conv, which takes no per-row length (Generator.short_rows() is False)" % i)
                    rows = (row_frames, spf)
                a, axl = self._upsample(st, sp.ups, _dense(al, i))
                self._mark("ups%d" % i)
                if st.route == "mrf32_post":
                    # x is read once, the waveform written once (hifi/models.py:190-199)
                    y = ops.hifi_mrf32_post(a, [w for p in sp.blocks for w in p[0]], [b for p in sp.blocks for b in p[1]],
                                            [blk.dilation for blk in st.blocks], [blk.k for blk in st.blocks], pk.post[0], pk.post[1],
                                            slope=LRELU_SLOPE, final_slope=st.nxt_slope, scale=1.0 / len(st.blocks), rows=rows)
                    self._mark("mrf%d" % i)
                    self._mark("conv_post")
                    return y
                if st.route != "gemm":
                    al = self._mrf_blocks(st, sp.blocks, a, rows)
                    continue
                if st.gemm == "lockstep":
                    outs = self._resblocks_lockstep(st.blocks, [taps for taps, _ in sp.blocks], a, axl)
                else:
                    outs = [self._resblock(blk, taps, a, axl, wpacks) for blk, (taps, wpacks) in zip(st.blocks, sp.blocks)]
                al = ops.avg3(outs[0], outs[1], outs[2], 1.0 / 3.0, slope=st.nxt_slope)         # lrelu(xs / num_kernels); three blocks: `build_plan`
            wp, bp = pk.post
            self._mark("mrf%d" % (len(plan.stages) - 1))
            if plan.conv_post == "stream":
                y = ops.hifi_conv_post(al, wp, bp)                                         # conv_post -> tanh, streaming kernel
                self._mark("conv_post")
                return y
            Bn, Tout, C = al.shape
            y = torch.empty(Bn * Tout, 1, dtype=torch.float32, device=al.device)
            ops.conv1d(al, wp, bp, out=y.view(Bn, Tout, 1), flags=ops.TANH)
        return y.view(Bn, 1, Tout)

    # ------------------------------------------------------------------ ragged batches, any length
    def halo(self):
        return windows.receptive_halo(self.h)

    def samples_per_frame(self):
        n = 1
        for u in self.h.upsample_rates:
            n *= int(u)
        return n

    def short_rows(self):
        """True when an utterance shorter than a window can run as a row of the windowed batch: every MRF stage of this configuration, with
        the kernel families as they are toggled on this object, runs on kernels that take a per-row length (ResBlock2 fused, the conv
        pairs, the fused ResBlock1 / last-stage kernel).  False for a stage on the conv-by-conv implicit-GEMM path: such a generator keeps
        the solo route for short utterances (`forward_short`).  From the plan (`_plan`, kept per toggle setting): no walk over the
        parameters, so a replayed list call plans for nothing."""
        return self.conv_pre.bias.device.type == "cuda" and "gemm" not in self.stage_routes()

    def stage_routes(self):
        """Per MRF stage, the kernel family `forward_ntc` runs it on: "resblock2" (fused ResBlock2), "pair" (conv pairs), "fused" (the
        six-conv ResBlock1 kernel / the fused last stage) or "gemm" (conv by conv on the implicit-GEMM kernel).  From the configuration
        and the toggles on this object alone (`_plan`)."""
        return ["fused" if st.route == "mrf32_post" else st.route for st in self._plan(refuse=False).stages]

    def plan(self, lens):
        """The window plan of a call on this generator: short utterances as rows of the batch where `short_rows()` allows."""
        return windows.plan_windows(lens, windows.W, self.halo(), short_rows=self.short_rows())

    def stage_mels(self, mels, plan, frames_first, stage=None):
        """The planned utterances back to back in the fp32 staging buffer the gather reads (N * W frames): (80, frames) rows, or,
        `frames_first`, (frames, 80) rows.  One copy per utterance (host or device source); frames past the call's own stay as they are,
        no window reads them."""
        frames = plan.N * plan.W
        dev = self.conv_pre.bias.device
        if stage is None:
            stage = torch.empty(frames * 80, dtype=torch.float32, device=dev)
        v = stage.view(frames, 80) if frames_first else stage.view(80, frames)
        for i in plan.planned:
            o, T = plan.offsets[i], plan.lens[i]
            (v[o:o + T] if frames_first else v[:, o:o + T]).copy_(mels[i], non_blocking=True)
        return stage

    def resampler(self, sample_rate):
        """None for `sample_rate` None or the generator's own rate (the native route: no launch is added), otherwise the filter from
        `h.sampling_rate` to `sample_rate` on the generator's device (`resample.Filter`; ValueError for a rate it refuses)."""
        if sample_rate is None:
            return None
        native = int(windows._get(self.h, "sampling_rate"))
        if resample.check_rate(sample_rate) == native:
            return None
        return resample.filter_for(native, int(sample_rate), self.conv_pre.bias.device)

    def row_segments(self, Bn, n, sample_rate):
        """The segment table of B rows of n samples each for `sample_rate`, (B, 4) int32 on the generator's device."""
        filt = self.resampler(sample_rate)
        return torch.from_numpy(resample.row_segments(Bn, n, filt.L, filt.M).table).to(self.conv_pre.bias.device)

    def resample_rows(self, y, sample_rate, int16_scale=None, segs=None):
        """y (B, 1, n) fp32 waveforms at the generator's rate -> (B, 1, ceil(n L / M)) at `sample_rate` (a rate `resampler` has a
        filter for), every row resampled as an utterance of its own: fp32, or with `int16_scale` saturated int16.  `segs`: the
        table `row_segments(B, n, sample_rate)` gave (a caller that repeats a shape, or captures the call, keeps it)."""
        filt = self.resampler(sample_rate)
        Bn, n = int(y.shape[0]), int(y.shape[-1])
        if segs is None:
            segs = self.row_segments(Bn, n, sample_rate)
        n_dst = Bn * resample.out_len(n, filt.L, filt.M)
        out = torch.empty(n_dst, dtype=torch.float32 if int16_scale is None else torch.int16, device=y.device)
        ops.resample(y.contiguous().view(-1), segs, filt, out=out, int16_scale=int16_scale)
        return out.view(Bn, 1, n_dst // Bn)

    def forward_windows(self, stage, table, frames_first=False, int16_scale=None, row_lengths=False, sample_rate=None, segs=None):
        """Gather -> generator -> stitch on device-resident inputs (capturable: nothing here depends on a length): the staging buffer
        and the plan table (N, 8) int32 -> one flat buffer of N * W * 256 samples, the kept samples of every utterance back to back.
        `row_lengths` (a plan with `has_short_rows`): the generator reads every row's valid frames from the table's column VALID, on
        the kernels that take a per-row length; without it the launches are those of a batch of full windows.
        `sample_rate` (other than the generator's) with `segs`, the plan's segment table (N, 4) int32 on the device (`plan_resample`):
        the stitch writes fp32 at the generator's rate and one more launch resamples that buffer by the table (and converts to int16
        when asked, saturating): the flat buffer, ceil(N W 256 L / M) + N samples, holds the utterances where the table's dst_off put them."""
        with torch.no_grad():
            a0 = ops.mel_windows(stage, table, windows.W, self.act_dtype, frames_first)
            y = self.forward_ntc(a0, row_frames=table[:, windows.VALID] if row_lengths else None)
            filt = self.resampler(sample_rate)
            if filt is None:
                return ops.wav_stitch(y, table, windows.W, int16_scale=int16_scale)
            if segs is None or tuple(segs.shape) != (table.shape[0], resample.ROW):
                raise ops.L.TtskError("forward_windows: sample_rate needs `segs`, the plan's (N, 4) segment table on the device")
            flat = ops.wav_stitch(y, table, windows.W)
            n_dst = resample.out_bound(flat.numel(), table.shape[0], filt.L, filt.M)
            out = torch.empty(n_dst, dtype=torch.float32 if int16_scale is None else torch.int16, device=flat.device)
            return ops.resample(flat, segs, filt, out=out, int16_scale=int16_scale)

    def plan_resample(self, plan, filt):
        """The segment table of `plan` for `filt` (kept on the plan as `plan.segs`, where `resample.split` finds it)."""
        plan.segs = resample.plan_segments(plan, self.samples_per_frame(), filt.L, filt.M)
        return plan.segs

    @staticmethod
    def ragged_mels(mels, frames_first=False):
        """The call's mels as 2-D tensors ((80, T_i), or (T_i, 80) when `frames_first`; a leading batch dimension of 1 is dropped) and their lengths."""
        out = []
        for m in mels:
            if m.dim() == 3 and m.shape[0] == 1:
                m = m[0]
            if m.dim() != 2 or m.shape[1 if frames_first else 0] != 80:
                raise ops.L.TtskError("ragged vocoding takes mels of shape %s, got %s" % ("(T, 80)" if frames_first else "(80, T)", tuple(m.shape)))
            out.append(m)
        return out, [int(m.shape[0 if frames_first else 1]) for m in out]

    def forward_ragged_flat(self, mels, frames_first=False, int16_scale=None, sample_rate=None):
        """The windowed part of `forward_ragged`: (flat buffer of the planned utterances' samples, back to back, or None when no
        utterance fills a window; the plan; samples per frame).  `int16_scale`: the buffer is int16, truncation of waveform * scale.
        `sample_rate` (other than the generator's): the buffer holds the resampled utterances as `plan.segs` lays them out (cut it
        with `resample.split`), int16 saturated."""
        mels, lens = self.ragged_mels(mels, frames_first)
        dev = self.conv_pre.bias.device
        if dev.type != "cuda":
            raise ops.L.TtskError("HiFi-GAN ragged vocoding needs the generator's weights on a HIP device; there is no CPU path")
        filt = self.resampler(sample_rate)                  # a rate the resampler refuses fails before any launch
        plan = self.plan(lens)
        if not plan.planned:
            return None, plan, self.samples_per_frame()
        stage = self.stage_mels(mels, plan, frames_first)
        table = torch.from_numpy(plan.table).to(dev)
        segs = None
        if filt is not None:
            segs = torch.from_numpy(self.plan_resample(plan, filt).table).to(dev)
        return self.forward_windows(stage, table, frames_first, int16_scale, plan.has_short_rows, sample_rate, segs), plan, self.samples_per_frame()

    def forward_short(self, mels, plan, frames_first=False, int16_scale=None, forward=None, sample_rate=None):
        """The utterances the plan left out (`plan.short`: those shorter than a window on a generator without `short_rows()`), each
        through `forward` (or the caller's `forward`) on its own: {index: waveform}.  `sample_rate`: each is then resampled alone, with
        a one-row segment table."""
        mels, _ = self.ragged_mels(mels, frames_first)
        filt = self.resampler(sample_rate)
        out = {}
        for i in plan.short:
            m = mels[i].to(self.conv_pre.bias.device).float()
            y = (forward or self.forward)((m.t() if frames_first else m).unsqueeze(0))
            if filt is not None:
                out[i] = self.resample_rows(y, sample_rate, int16_scale)
            else:
                out[i] = y if int16_scale is None else ops.to_int16(y, float(int16_scale))
        return out

    def forward_ragged(self, mels, frames_first=False, sample_rate=None):
        """mels: a list of (80, T_i) or (1, 80, T_i) tensors of any lengths (`frames_first`: (T_i, 80) / (1, T_i, 80), FastSpeech2's
        layout) -> a list of (1, 1, 256 T_i) fp32 waveforms, each what `forward` gives for that mel alone (tts_king_amd/windows.py).

        The utterances run together as fixed-size windows: one gather launch, the generator on (N, W, 80), one stitch launch.  An
        utterance shorter than a window is one row of that batch with its own length (a padded mel is not a solo run: the kernels
        treat what lies past the row's end as the zero padding of every layer).  On a generator configuration whose
        kernels take no row length (`short_rows()` False) it goes through `forward` on its own instead, one utterance per call.

        `sample_rate` (Hz; None or `h.sampling_rate`: the route above, unchanged): the waveforms at that rate, (1, 1, ceil(256 T_i L / M)),
        each resampled as an utterance of its own by one more launch on the flat buffer (tts_king_amd/resample.py)."""
        mels = list(mels)
        flat, plan, spf = self.forward_ragged_flat(mels, frames_first, sample_rate=sample_rate)
        return resample.split(flat, plan, spf, self.forward_short(mels, plan, frames_first, sample_rate=sample_rate))

    @staticmethod
    def join_spans(plan, spf, flat_samples, short):
        """Where the call's utterances lie for the join, in the call's order: (offsets, lengths) in samples of the flat buffer followed
        by the waveforms of `short` = {index: waveform} in the order of their indices (`torch.cat`).  A resampled plan (`plan.segs`)
        gives its destination columns."""
        offs, lens = [0] * len(plan.lens), [0] * len(plan.lens)
        if plan.segs is not None:
            for i, (o, m) in zip(plan.planned, plan.segs.spans):
                offs[i], lens[i] = o, m
        else:
            for i in plan.planned:
                offs[i], lens[i] = plan.offsets[i] * spf, plan.lens[i] * spf
        pos = int(flat_samples)
        for i in sorted(short):
            offs[i], lens[i] = pos, int(short[i].numel())
            pos += lens[i]
        return offs, lens

    def forward_joined(self, mels, join, frames_first=False, int16_scale=None, sample_rate=None):
        """The utterances of `forward_ragged` as ONE waveform (tts_king_amd/narrate.py): `forward_ragged_flat` in fp32,
        then the two join launches on the flat buffer by `join` (a `narrate.Join`: settings, pauses, gains), which trim, level, fade
        and lay the utterances out behind each other in the call's order.  -> (out, info, bound): `out` the flat waveform, fp32 or
        with `int16_scale` saturated int16, `bound` = `narrate.out_bound` samples of which the first `info[U, 0]` are the waveform and
        the rest zeros; `info` the (U + 1, 8) int32 device table (`narrate.Info`).  With `sample_rate` the resampled buffer is joined
        by the segment table's destination columns.  Utterances that a generator without `short_rows()` vocodes alone are placed
        behind the flat buffer before the join: the same two launches."""
        mels = list(mels)
        if len(join) != len(mels):
            raise ValueError("forward_joined: the join names %d utterances, the call has %d" % (len(join), len(mels)))
        flat, plan, spf = self.forward_ragged_flat(mels, frames_first, None, sample_rate)
        short = {}
        if any(plan.lens[i] > 0 for i in plan.short):
            short = self.forward_short(mels, plan, frames_first, None, sample_rate=sample_rate)
        return self.join_flat(flat, plan, spf, short, join, int16_scale)

    def join_flat(self, flat, plan, spf, short, join, int16_scale=None, rows=None):
        """The join of `forward_joined` on a flat fp32 buffer that `forward_ragged_flat` (or a replayed graph) left, plus `short`."""
        from . import narrate
        dev = self.conv_pre.bias.device
        offs, lens = self.join_spans(plan, spf, 0 if flat is None else flat.numel(), short)
        with torch.no_grad():
            parts = ([] if flat is None else [flat]) + [short[i].reshape(-1) for i in sorted(short)]
            src = parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.zeros(1, dtype=torch.float32, device=dev)
            table = join.table(offs, lens, rows)
            bound = narrate.out_bound(table)
            out, info = ops.wav_join(src, torch.from_numpy(table).to(dev), n_dst=max(bound, 1), int16_scale=int16_scale)
        return out, info, bound
