"""GPU: every FS2 block of one train step against fp64 math on the block's OWN HIP inputs.

tests/test_step_shapes_gpu.py compares the whole step with the fp32 oracle; every figure there carries the drift of up to ten
bf16 blocks and train-mode BatchNorm, and its bars are wide (up to 45-63 %).  Here the drift is removed instead of tolerated: one
default-path step (`_forward(True, ...)`, `ops.fs2_loss`, `backward_native(accumulate=False)`, no switch changed) is run, and

* the activations the forward keeps for the backward (ctx.blocks, ctx.preds["grouped"], ctx.pn, ctx.dec_out, the embedding
  indices) are cloned before the backward;
* the upstream gradient that reaches each unit's backward is recorded from the outside: `_fft_bwd`,
  `_predictors_bwd_inputs` and `_predictors_bwd_grouped` are wrapped on the instance, `ops.bn_bwd` (the PostNet's per-layer
  entry) for the duration of the step; arguments and return values are cloned at call time on the stream the call runs on;
* each unit is then recomputed in float64 on the CPU from ITS saved HIP input and ITS recorded upstream gradient, through the
  oracle's own block functions (oracle/fs2.py: fft_block, variance_predictor; the PostNet layer and the embedding / length
  regulator sums are restated from postnet / variance_adaptor / length_regulator there), with the very dropout keep-masks the
  kernels draw (tests/test_parity_gpu.py hip_dropout_masks).

The reference reads the operands exactly as the kernels do: matrices from the bf16 shadow, vectors / LayerNorm / BatchNorm
parameters and embedding tables from the fp32 masters, activations as saved.  A unit's error is then its own, and the bars sit
at bf16 rounding:

* outputs (rows x channels, over valid rows): rel-RMS <= OUT_TAU and, per element, |diff| <= ULPS bf16 ulps of max(|ref|, RMS); rows the
  reference zeroes (PAD rows of block outputs, frames past `frame_limit` of the PostNet's input) exactly zero;
* parameter gradients: every one is a sum G = sum_i a_i b_i of products of a gradient signal and an activation (over rows and
  taps: dW, bias, LayerNorm / BatchNorm gamma and beta, embedding rows).  Each product reaches the kernel through at most
  C = 12 bf16 roundings of relative size <= U = 2^-8 (its two operands and the signal's own chain inside the unit), each an
  independent error of variance U^2 / 3, so the error of an element is ~ U sqrt(C / 3) sqrt(sum_i (a_i b_i)^2) = 2 U R.  The
  bar is  |G_hip - G_ref| <= max(TAU |G_ref|, KAPPA U |R|)  with KAPPA = 4 (2 x that standard deviation's factor, a 2-sigma
  margin per element that the Frobenius norm over a tensor only tightens) and TAU = 2 % (an error that small is below the
  rounding of the tensor's own bf16 copy in the optimizer's shadow, 2^-8 = 0.4 %, times the C above).  R is what makes a
  near-cancelling sum testable: the duration head's bias, the PostNet conv biases in front of train-mode BatchNorm (true
  gradient zero), BatchNorm gamma.  Where the backward itself cancels before the product — train-mode BatchNorm's
  g - mean(g) - x_hat mean(g x_hat) — the signal in R is the magnitude of those terms, not their difference;
* input gradients: |dx_hip - dx_ref| <= DX_TAU |dx_ref| (+ the same magnitude term through a BatchNorm);
* attention's q / k path: the flash kernel rounds P and dS to bf16 inside, and under the near-uniform attention of random
  weights dS = P o (dP - rowsum(P dP)) nearly cancels, so a rounding there is not a rounding of the result.  For the query /
  key projections' gradients and the block's input gradient, the bar may instead come from the same fp64 block restated with
  the flash kernel's backward modelled (P in fp32, P V and dV with P in bf16, delta = rowsum(dO o O32) from the bf16-P output,
  dS in fp32 rounded to bf16) and every stored bf16 gradient rounded (dq|dk|dv, dO, the fc / w_2 output gradients, dh, the
  residual's gradient): bar = max(bar above, CAL x that reference's own deviation from the plain one), CAL = 1.5, as the
  step-level tests calibrate.  The non-calibrated part of that bar may not be wider than QK_CAP = 5 % of the gradient
  (checked; measured on MI355X: at most 3.4 %, the calibrated bars at most 5.0 %, the HIP figures at most 1.4 %).  The
  calibration is one realization of many independent roundings (of P for P V and delta, of dS), which the norm over a tensor
  averages.
  It stops being a statistic where every utterance of the unit has at most FEW_KEYS = 2 keys (case "smallest": L = 1,
  T = 2).  With one key, dS is zero in exact arithmetic and the HIP figure is fp32 noise.  With two, dS_t = [a, -a] and the
  error is a handful of rounding events, so one realization of the model can miss the HIP one by any factor (measured: 5.5 %
  against a calibration below 1.4 %).  Only there does R of the q / k tensors take the worst case of those few terms, dS's
  magnitude P o (|dP - delta| + rowsum(P |dP|)) through |K| / |Q| (_FlashMag), and no cap applies.

Every trainable key of the model is checked by exactly the unit that owns it; the covered set is asserted equal to the
trainable set.  The per-unit table (figure and bar, relative to the reference's norm) is printed with -s."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import fs2 as ofs2
from tests.oracle_util import fs2_state_dict
from tests.test_parity_gpu import oracle_with_masks
from tests.test_step_shapes_gpu import CASES, HipStep, exact_batch

pytestmark = pytest.mark.gpu
U = 2.0 ** -8
TAU, KAPPA = 0.02, 4.0
OUT_TAU, DX_TAU, ULPS = 0.01, 0.02, 8
CAL = 1.5
# the query / key projections' max(TAU |G|, KAPPA U |R|) may not be wider than QK_CAP of the gradient (their calibrated term is
# CAL x the modelled reference's deviation); a unit whose utterances have at most FEW_KEYS keys takes their R from dS's magnitude
# instead, with no cap (see the module docstring)
QK_CAP, FEW_KEYS = 0.05, 2

# the seams of the window conv (64 / 112-frame tiles) and flash attention (64-row tiles), the bucketed batch, dropout at every site,
# the 1000-frame cut, B = 1 x 1 phoneme, and both sides of ln_bwd256_proj's two-workgroup split
NAMES = ("smallest", "65", "113", "129_225", "bucketed", "dropout", "truncation", "split_on_B32_L63", "split_off_B32_L64")


# ------------------------------------------------------------------------------------------------ recording the HIP side

def _clone(t):
    from tts_king_amd.ops import Slabs
    if torch.is_tensor(t):
        return t.detach().clone()
    if isinstance(t, Slabs):
        return Slabs(t.ws.detach().clone(), t.splits, t.stride)
    if isinstance(t, (tuple, list)):
        return type(t)(_clone(v) for v in t)
    return t


class Recorder:
    """Wraps the model's bound methods (calls go through `self.`) and ops.bn_bwd for one backward."""

    def __init__(self, m):
        from tts_king_amd import ops
        self.m, self.ops = m, ops
        self.fft, self.pred_inputs, self.pred_grouped, self.bn = {}, [], [], []
        fft, pin, pgr, self.bn_bwd = m._fft_bwd, m._predictors_bwd_inputs, m._predictors_bwd_grouped, ops.bn_bwd

        def fft_bwd(saved, dx2, rng, raw_out=False):
            up = _clone(dx2)
            r = fft(saved, dx2, rng, raw_out=raw_out)
            self.fft[saved[0]] = (up, _clone(r))
            return r

        def predictors_bwd_inputs(saved, dstack, rng):
            up = _clone(dstack)
            r = pin(saved, dstack, rng)
            self.pred_inputs.append((up, _clone(r)))
            return r

        def predictors_bwd_grouped(saved, dstack, rng, dx3, dxin=None):
            up = _clone(dx3)
            r = pgr(saved, dstack, rng, dx3, dxin=dxin)
            self.pred_grouped.append((up, _clone(r)))
            return r

        def bn_bwd(dout, *a, **kw):
            self.bn.append(_clone(dout))                 # layers 4, 3, ..., 0
            return self.bn_bwd(dout, *a, **kw)
        m._fft_bwd, m._predictors_bwd_inputs, m._predictors_bwd_grouped = fft_bwd, predictors_bwd_inputs, predictors_bwd_grouped
        ops.bn_bwd = bn_bwd

    def close(self):
        for n in ("_fft_bwd", "_predictors_bwd_inputs", "_predictors_bwd_grouped"):
            self.m.__dict__.pop(n, None)
        self.ops.bn_bwd = self.bn_bwd


def dense(up, m, pre):
    """An upstream gradient as its consumer reads it -> (rows, d) fp64, by exact math on the stored values: a tensor as is;
    (Slabs, residual) = the split-K partial tiles summed + residual; the "pre" triple (dqkv, packed W_qkv^T, dz1) of block `pre`
    (fastspeech2.py _fft_bwd: the consumer's ttsk_layernorm_bwd_proj multiplies by the weight itself) = dqkv W_qkv + dz1, W_qkv the
    bf16 shadow of that block's fused q|k|v weight."""
    d = m.d
    if torch.is_tensor(up):
        return up.double().cpu().reshape(-1, d)
    if len(up) == 3:
        dqkv, _, dz1 = up
        W = m._w(pre + "slf_attn.w_qs.weight", 3 * d).double().cpu()
        return dqkv.double().cpu() @ W + dz1.double().cpu().reshape(-1, d)
    sl, res = up
    rows = res.numel() // d
    ws = sl.ws.reshape(-1)[:sl.splits * sl.stride].view(sl.splits, sl.stride)       # [splits][stride] fp32 partial tiles (ops.Slabs)
    return ws[:, :rows * d].double().cpu().sum(0).reshape(rows, d) + res.double().cpu().reshape(rows, d)


def ref_params(m):
    """key -> fp64 leaf in the reference's shape, as the kernels read it: matrices from the bf16 shadow, vectors, LayerNorm /
    BatchNorm parameters, the predictors' 256 -> 1 heads and the embedding tables from the fp32 masters."""
    P = {}
    for k, en in m._table.items():
        if en.kind != "train":
            continue
        shadow = len(en.shape) >= 2 and not k.endswith("emb.weight") and "_embedding." not in k and "linear_layer" not in k
        v = (m._w(k) if shadow else m._m(k)).detach()
        if en.conv:
            v = v.permute(0, 2, 1)
        P[k] = v.double().cpu().contiguous().requires_grad_(True)
    return P


# ------------------------------------------------------------------------------------------------ fp64 references

class Tape:
    """Passed as `Fn` to fft_restated / predictor_restated in place of `torch.nn.functional`: every op that takes a parameter keeps
    its activation operand and its output (gradient retained), so that R = sqrt(sum_i (a_i b_i)^2) of each parameter gradient can
    be formed after the backward."""

    def __init__(self):
        self.ops = []

    def __getattr__(self, n):
        return getattr(F, n)

    def linear(self, x, w, b=None):
        y = F.linear(x, w, b)
        y.retain_grad()
        self.ops.append(("lin", x.detach(), w, b, y))
        return y

    def conv1d(self, x, w, b=None, padding=0):
        y = F.conv1d(x, w, b, padding=padding)
        y.retain_grad()
        self.ops.append(("conv", x.detach(), w, b, padding, y))
        return y

    def layer_norm(self, x, shape, w, b, eps=1e-5):
        y = F.layer_norm(x, shape, w, b, eps=eps)
        y.retain_grad()
        xd = x.detach()
        xh = (xd - xd.mean(-1, keepdim=True)) / (xd.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
        self.ops.append(("ln", xh, w, b, y))
        return y

    def scales(self, P):
        ids = {id(v): k for k, v in P.items()}
        sq = {}

        def add(w, s):
            if w is not None and id(w) in ids:
                k = ids[id(w)]
                sq[k] = sq.get(k, 0.0) + s
        for op in self.ops:
            g = op[-1].grad
            if g is None:
                continue
            g2 = g.detach() ** 2
            if op[0] == "lin":
                _, x, w, b, _ = op
                add(w, g2.reshape(-1, g2.shape[-1]).t() @ (x ** 2).reshape(-1, x.shape[-1]))
                add(b, g2.reshape(-1, g2.shape[-1]).sum(0))
            elif op[0] == "conv":
                _, x, w, b, pad, _ = op
                add(w, torch.nn.grad.conv1d_weight(x ** 2, w.shape, g2, padding=pad))
                add(b, g2.sum((0, 2)))
            else:
                _, xh, w, b, _ = op
                add(w, (g2 * xh ** 2).reshape(-1, xh.shape[-1]).sum(0))
                add(b, g2.reshape(-1, g2.shape[-1]).sum(0))
        return {k: v.sqrt() for k, v in sq.items()}


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    """Identity whose forward value (fwd) and / or backward gradient (bwd) is rounded to bf16: a HIP storage point."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_bf(g) if ctx.bwd else g), None, None


class _FlashCore(torch.autograd.Function):
    """Attention's core as the flash kernel's backward computes it (csrc/flash_attn.hip): P in fp32, P V and dV = P~^T dO with
    P~ = P in bf16, delta = rowsum(dO o O32) with O32 = P~ V in fp32, dS = P (dP - delta) in fp32, rounded to bf16 for dQ / dK.
    (delta from P~ does not cancel against dP from P: the q / k path's error is set by this, not by a rounding of dS alone.)"""

    @staticmethod
    def forward(ctx, q, k, v, kpad):
        s = (q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])).masked_fill(kpad[:, None, None, :], float("-inf"))
        P = torch.softmax(s.float(), -1)
        Pb = _bf(P)
        ctx.save_for_backward(q, k, v, P, Pb)
        return Pb.double() @ v

    @staticmethod
    def backward(ctx, do):
        q, k, v, P, Pb = ctx.saved_tensors
        do32 = do.float()
        dP = do32 @ v.float().transpose(-1, -2)
        delta = (do32 * (Pb @ v.float())).sum(-1, keepdim=True)
        dS = _bf(P * (dP - delta) / math.sqrt(q.shape[-1])).double()
        return dS @ k, dS.transpose(-1, -2) @ q, Pb.double().transpose(-1, -2) @ do, None


class _FlashMag(torch.autograd.Function):
    """Attention's core whose backward returns, instead of dQ / dK, their MAGNITUDE through dS: what a relative error U in the
    terms of dS = P o (dP - delta) can move them by, |dS|_mag = P o (|dP - delta| + rowsum(P |dP|)), times |K| / |Q|.  (With one
    or two keys per utterance, dS cancels to nothing and a handful of such errors, not a statistic, is all there is.)"""

    @staticmethod
    def forward(ctx, q, k, v, kpad):
        s = (q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])).masked_fill(kpad[:, None, None, :], float("-inf"))
        P = torch.softmax(s, -1)
        ctx.save_for_backward(q, k, v, P)
        return P @ v

    @staticmethod
    def backward(ctx, do):
        q, k, v, P = ctx.saved_tensors
        dP = do @ v.transpose(-1, -2)
        delta = (P * dP).sum(-1, keepdim=True)
        mag = P * ((dP - delta).abs() + (P * dP.abs()).sum(-1, keepdim=True)) / math.sqrt(q.shape[-1])
        return mag @ k.abs(), mag.transpose(-1, -2) @ q.abs(), torch.zeros_like(v), None


def fft_restated(P, pre, x, pad, H, keeps, p, rounded, hip=None, Fn=F):
    """oracle/fs2.py fft_block (multi_head_attention + positionwise_ffn, PAD rows zeroed) restated (with hip=None and
    rounded=False it is fft_block itself: checked against it in every case).  `hip`: the block's saved HIP activations (qkv, o,
    x1, h) stand in for the computed ones (forward value HIP's, gradient passed through) — the backward then sees the operands
    the kernels read, ReLU gates included (a bf16 rounding of x1 flips a few gates of h, which moves w_1's and the attention
    side's gradients by 2-3 % rel-RMS: not a kernel error).  `rounded`: the backward's gradients are rounded to bf16 where the
    HIP path stores them.  Returns (output, {qkv, o, x1, h} as computed from the (HIP) inputs of each)."""
    R = (lambda t, f, b: _Round.apply(t, f, b)) if rounded is True else (lambda t, f, b: t)
    inter = {}

    def sub(name, t):
        inter[name] = t.detach()
        if hip is not None:
            t = t + (hip[name].reshape(t.shape) - t).detach()
        return t
    B, S, D = x.shape
    dk = D // H
    a, f = pre + "slf_attn.", pre + "pos_ffn."
    qkv = torch.cat([Fn.linear(x, P[a + n + ".weight"], P[a + n + ".bias"]) for n in ("w_qs", "w_ks", "w_vs")], -1)
    qkv = R(sub("qkv", qkv), False, True)
    q, k, v = (t.reshape(B, S, H, dk).transpose(1, 2) for t in qkv.split(D, -1))
    if rounded == "mag":
        core = _FlashMag.apply(q, k, v, pad)
    elif rounded:
        core = _FlashCore.apply(q, k, v, pad)
    else:
        s = (q @ k.transpose(-1, -2) / math.sqrt(dk)).masked_fill(pad[:, None, None, :], float("-inf"))
        core = torch.softmax(s, -1) @ v
    o = R(sub("o", core.transpose(1, 2).reshape(B, S, D)), False, True)
    y1 = R(Fn.linear(o, P[a + "fc.weight"], P[a + "fc.bias"]), False, True)
    if p > 0:
        y1 = y1 * keeps[0][0].double() / (1.0 - p)
    x1 = Fn.layer_norm(y1 + R(x, False, True), (D,), P[a + "layer_norm.weight"], P[a + "layer_norm.bias"]).masked_fill(pad[..., None], 0)
    x1 = sub("x1", x1)
    w1 = P[f + "w_1.weight"]
    h = F.relu(Fn.conv1d(x1.transpose(1, 2), w1, P[f + "w_1.bias"], padding=(w1.shape[2] - 1) // 2))
    h = R(sub("h", h.transpose(1, 2)).transpose(1, 2), False, True)
    w2 = P[f + "w_2.weight"]
    y2 = R(Fn.conv1d(h, w2, P[f + "w_2.bias"], padding=(w2.shape[2] - 1) // 2).transpose(1, 2), False, True)
    if p > 0:
        y2 = y2 * keeps[1][0].double() / (1.0 - p)
    out = Fn.layer_norm(y2 + R(x1, False, True), (D,), P[f + "layer_norm.weight"], P[f + "layer_norm.bias"]).masked_fill(pad[..., None], 0)
    return out, inter


def predictor_restated(P, pre, x, pad, keeps, p, hip=None, Fn=F):
    """oracle/fs2.py variance_predictor restated (hip=None: itself, checked in every case); `hip` as in fft_restated: the saved
    h1 (ReLU(conv1)), a1 (LayerNorm 1 + dropout) and h2 (ReLU(conv2)) stand in for the computed ones."""
    inter = {}

    def sub(name, t):
        inter[name] = t.detach()
        if hip is not None:
            t = t + (hip[name].reshape(t.shape) - t).detach()
        return t
    c = pre + "conv_layer."
    h = x
    for i in (1, 2):
        w, b = P[c + "conv1d_%d.conv.weight" % i], P[c + "conv1d_%d.conv.bias" % i]
        h = sub("h%d" % i, F.relu(Fn.conv1d(h.transpose(1, 2), w, b, padding=(w.shape[2] - 1) // 2).transpose(1, 2)))
        h = Fn.layer_norm(h, (h.shape[-1],), P[c + "layer_norm_%d.weight" % i], P[c + "layer_norm_%d.bias" % i])
        if p > 0:
            h = h * keeps[i - 1][0].double() / (1.0 - p)
        if i == 1:
            h = sub("a1", h)
    out = Fn.linear(h, P[pre + "linear_layer.weight"], P[pre + "linear_layer.bias"]).squeeze(-1)
    return out.masked_fill(pad, 0.0), inter


def _zero_grads(P, *more):
    for t in list(P.values()) + list(more):
        t.grad = None


def _keys_of(P, prefix):
    return [k for k in P if k.startswith(prefix)]


# ------------------------------------------------------------------------------------------------ bars and the table

class Report:
    def __init__(self, name):
        self.name, self.rows, self.fails, self.covered = name, [], [], set()

    def add(self, unit, what, fig, bar, ok, note=""):
        self.rows.append((unit, what, fig, bar, ok, note))
        if not ok:
            self.fails.append("%s %s / %s: %s > %s %s" % (self.name, unit, what, fig, bar, note))

    def out(self, unit, what, hip, ref, valid=None, zero=None, tau=OUT_TAU):
        """hip / ref (rows, C); valid: bool rows compared; zero: bool rows the reference zeroes (exactly 0 in HIP)."""
        h, r = hip.double().cpu().reshape(ref.shape[0], -1), ref.detach().double().reshape(ref.shape[0], -1)
        if valid is not None:
            hv, rv = h[valid], r[valid]
        else:
            hv, rv = h, r
        rms = float(rv.pow(2).mean().sqrt()) if rv.numel() else 0.0
        rel = float((hv - rv).pow(2).mean().sqrt()) / max(rms, 1e-300) if rv.numel() else 0.0
        self.add(unit, what + " rel-RMS", "%.4f%%" % (100 * rel), "%.2f%%" % (100 * tau), rel <= tau)
        if rv.numel() and rms > 0:
            # per element: ULPS bf16 ulps of max(|ref|, RMS) — an element's own rounding scales with it, a small one's with the tensor's
            ulp = torch.exp2(torch.floor(torch.log2(rv.abs().clamp_min(rms))) - 7)
            q = (hv - rv).abs() / (ULPS * ulp)
            j = int(q.argmax())
            self.add(unit, what + " max-abs", "%.3g" % float((hv - rv).abs().flatten()[j]), "%.3g" % float(ULPS * ulp.flatten()[j]),
                     float(q.max()) <= 1.0, "(worst element vs %d ulp of max(|ref|, RMS %.3g))" % (ULPS, rms))
        if zero is not None and bool(zero.any()):
            nz = int((h[zero] != 0).any(1).sum())
            self.add(unit, what + " PAD rows", "%d nonzero" % nz, "0", nz == 0)

    def grad(self, unit, k, hip, ref, scale, cal=None, cap=None):
        """|G_hip - G_ref| <= max(TAU |G_ref|, KAPPA U |R|[, CAL |G_cal - G_ref|]); `cap`: max(TAU |G_ref|, KAPPA U |R|) may not
        exceed cap |G_ref| (the calibration's term is bounded by its own rule: CAL x the modelled reference's deviation)."""
        self.covered.add(k)
        err = float((hip.double() - ref.detach()).norm())
        gn = float(ref.detach().norm())
        bar = max(TAU * gn, KAPPA * U * float(scale.norm()))
        if cap is not None:
            self.add(unit, k + " R-bar width", "%.3f%%" % (100 * bar / gn), "%.1f%%" % (100 * cap), bar <= cap * gn)
        note = ""
        if cal is not None and CAL * cal > bar:
            bar, note = CAL * cal, "(calibrated %.3g)" % cal
        if gn > 0:
            self.add(unit, k, "%.3f%%" % (100 * err / gn), "%.3f%%" % (100 * bar / gn), err <= bar, note)
        else:
            self.add(unit, k, "%.3g abs" % err, "%.3g abs" % bar, err <= bar, note)

    def dx(self, unit, what, hip, ref, cal=None, mag=None):
        """input gradients: |dx_hip - dx_ref| <= max(DX_TAU |dx_ref|, KAPPA U |mag|, CAL |dx_cal - dx_ref|)."""
        hip, ref = hip.double().cpu().reshape(ref.shape), ref.detach()
        err, gn = float((hip - ref).norm()), float(ref.norm())
        bar, note = DX_TAU * gn, ""
        if mag is not None and KAPPA * U * float(mag.norm()) > bar:
            bar, note = KAPPA * U * float(mag.norm()), "(magnitude)"
        if cal is not None and CAL * cal > bar:
            bar, note = CAL * cal, "(calibrated %.3g)" % cal
        self.add(unit, what, "%.3f%%" % (100 * err / max(gn, 1e-300)), "%.3f%%" % (100 * bar / max(gn, 1e-300)), err <= bar, note)

    def print(self):
        print("\ncase %s: %d checks" % (self.name, len(self.rows)))
        for unit, what, fig, bar, ok, note in self.rows:
            print("  %-4s %-30s %-58s %14s  bar %12s %s" % ("ok" if ok else "FAIL", unit, what, fig, bar, note))


# ------------------------------------------------------------------------------------------------ the step

class Step:
    """One default-path training step of HipStep's model, with the saved activations and the recorded upstream gradients."""

    def __init__(self, cfg, name):
        src, mel, dropout, bucketed = CASES[name]
        self.b = exact_batch(src, mel, seed=1000 + sum(src) + 7 * sum(mel))
        if src[0] >= 3:
            # the PAD token at a valid position too: nn.Embedding(padding_idx=0) still gives its row no gradient there (at PAD
            # positions the encoder's input gradient is exactly zero, so only this shows whether the scatter skips the row)
            self.b[3][0, 1] = 0
        self.hs = hs = HipStep(cfg, self.b, dropout, bucketed)
        m = self.m = hs.m
        self.src = list(src)
        self.Lb = max(src)                                       # the reference batch's own lengths (a bucketed batch is padded past them)
        self.Tb = min(max(mel), m.max_seq_len)
        sdm = m.state_dict()
        self.bn0 = {k: v.detach().cpu().clone() for k, v in sdm.items() if "running_" in k}
        sv = {}

        def keep(ctx, dmel_sum, dpost):
            sv["blocks"] = [tuple(_clone(t) for t in blk) for blk in ctx.blocks]
            sv["n_enc"] = ctx.n_enc_blocks
            sv["grouped"] = _clone(ctx.preds["grouped"])
            sv["pn"] = [_clone(e) for e in ctx.pn]
            sv["dec_out"] = _clone(ctx.dec_out)
            sv["pidx"], sv["eidx"], sv["texts"], sv["speakers"] = (_clone(t) for t in (ctx.pidx, ctx.eidx, ctx.texts, ctx.speakers))
            sv["dims"] = ctx.dims
            sv["dmel_sum"], sv["dpost"] = _clone(dmel_sum), _clone(dpost)
        self.rec = Recorder(m)
        try:
            self.losses, self.outs, flat = hs.run(on_ctx=keep)
        finally:
            self.rec.close()
        torch.cuda.synchronize()
        self.sv = sv
        self.bn1 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "running_" in k}
        self.keys = ofs2.trainable_keys(fs2_state_dict(cfg, 7))
        self.hip = hs.grads(flat, self.keys)
        self.P = ref_params(m)
        self.masks = hs.masks


def _site_masks(step, kind, i):
    """(keep, p) pairs of a unit's dropout sites, in hip_dropout_masks' order (encoder blocks, predictors, decoder blocks, PostNet)."""
    if step.masks is None:
        return None
    m = step.m
    base = {"enc": 2 * i, "pred": 2 * m.n_enc + 2 * i, "dec": 2 * m.n_enc + 6 + 2 * i, "pn": 2 * m.n_enc + 6 + 2 * m.n_dec + i}[kind]
    return step.masks[base:base + (1 if kind == "pn" else 2)]


def check_fft_blocks(step, rep):
    m, P, sv = step.m, step.P, step.sv
    blocks, n_enc = sv["blocks"], sv["n_enc"]
    for bi, blk in enumerate(blocks):
        (pre, x, qkv, probs, o, z1, mean1, rstd1, x1, h, z2, mean2, rstd2, Bn, S, lens, H, p, site, o32) = blk
        enc = bi < n_enc
        i = bi if enc else bi - n_enc
        last = (bi == n_enc - 1) or (bi == len(blocks) - 1)
        unit = pre[:-1].replace("layer_stack.", "")
        d = m.d
        pad = torch.arange(S)[None, :] >= lens.cpu()[:, None]
        valid = ~pad.reshape(-1)
        keeps = _site_masks(step, "enc" if enc else "dec", i)
        # the block's output as the next unit reads it
        if not last:
            nxt = blocks[bi + 1][1]
        elif enc:
            nxt = sv["grouped"][0][0]
        else:
            nxt = sv["dec_out"]
        bkeys = _keys_of(P, pre)
        up, ret = step.rec.fft[pre]
        g_up = dense(up, m, blocks[bi + 1][0] if not last else None).reshape(Bn, S, d)
        x64 = x.double().cpu().reshape(Bn, S, d)
        acts = {"qkv": qkv.double().cpu(), "o": o.double().cpu(), "x1": x1.double().cpu(), "h": h.double().cpu()}
        # ---- the whole block from its input, through the oracle's fft_block (and the restatement, which must equal it)
        with torch.no_grad():
            with (oracle_with_masks(keeps) if p > 0 else _nothing()):
                out_o = ofs2.fft_block(P, pre, x64, pad, H, p, True)
            out_s, _ = fft_restated(P, pre, x64, pad, H, keeps, p, rounded=False)
        assert float((out_s - out_o).abs().max()) <= 1e-9 * max(1.0, float(out_o.abs().max())), "restatement != oracle fft_block"
        # ---- teacher-forced fp64 (every activation the kernels read is HIP's), with the tape for R
        _zero_grads(P)
        xr = x64.clone().requires_grad_(True)
        tape = Tape()
        out, inter = fft_restated(P, pre, xr, pad, H, keeps, p, rounded=False, hip=acts, Fn=tape)
        out.backward(g_up)
        ref = {k: P[k].grad.clone() for k in bkeys}
        dx_ref = xr.grad.clone()
        sc = tape.scales(P)
        # ---- the same with the backward's bf16 storage points rounded: the calibration of the q / k path
        _zero_grads(P)
        xm = x64.clone().requires_grad_(True)
        out_r, _ = fft_restated(P, pre, xm, pad, H, keeps, p, rounded=True, hip=acts)
        out_r.backward(g_up)
        cal = {k: float((P[k].grad - ref[k]).norm()) for k in bkeys}
        cal_dx = float((xm.grad - dx_ref).norm())
        # ---- at most two keys in every utterance: dS's magnitude through the q / k path, for R of the query / key projections
        few_keys = int(lens.cpu().clamp(max=S).max()) <= FEW_KEYS
        if few_keys:
            _zero_grads(P)
            tape_m = Tape()
            out_m, _ = fft_restated(P, pre, x64.clone().requires_grad_(True), pad, H, keeps, p, rounded="mag", hip=acts, Fn=tape_m)
            out_m.backward(g_up)
            sc = dict(sc, **{k: v for k, v in tape_m.scales(P).items() if ".w_qs." in k or ".w_ks." in k})
        _zero_grads(P)
        # ---- forward: each stored activation from the HIP inputs of its own kernel, and the block output
        rows = Bn * S
        rep.out(unit, "qkv = x W_qkv + b", qkv, inter["qkv"].reshape(rows, -1), valid)
        rep.out(unit, "o = attention(qkv)", o, inter["o"].reshape(rows, -1), valid)
        rep.out(unit, "x1 = LN(o W_fc + b + x)", x1, inter["x1"].reshape(rows, -1), valid, zero=pad.reshape(-1))
        rep.out(unit, "h = ReLU(w_1 * x1)", h, inter["h"].reshape(rows, -1), valid)
        rep.out(unit, "output = LN(w_2 h + x1)", nxt, out.detach().reshape(rows, -1), valid, zero=pad.reshape(-1))
        r = float((nxt.double().cpu().reshape(rows, -1)[valid] - out_o.reshape(rows, -1)[valid]).pow(2).mean().sqrt() /
                  out_o.reshape(rows, -1)[valid].pow(2).mean().sqrt())
        rep.add(unit, "output from x (fft_block) rel-RMS", "%.4f%%" % (100 * r), "%.2f%%" % (100 * OUT_TAU), r <= OUT_TAU)
        # ---- backward
        for k in bkeys:
            qk = ".w_qs." in k or ".w_ks." in k
            rep.grad(unit, k, step.hip[k], ref[k], sc.get(k, torch.zeros(1)), cal=cal[k] if qk else None,
                     cap=QK_CAP if (qk and not few_keys and not k.endswith("w_ks.bias")) else None)
        rep.dx(unit, "input gradient", dense(ret, m, pre), dx_ref.reshape(rows, d), cal=cal_dx)


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def check_predictors_and_adaptor(step, rep):
    """The grouped VariancePredictors (stack -> three predictions, back), the variance-adaptor sums, the LengthRegulator, and the
    four embedding tables."""
    m, P, sv = step.m, step.P, step.sv
    (stack, h1, m1, r1, a1, h2, m2, r2, Bn, Lp, lens, p, row_limit) = sv["grouped"]
    d, Lb = m.d, step.Lb
    B = Bn
    va = "variance_adaptor."
    src_l = torch.tensor(step.src)
    pad = torch.arange(Lb)[None, :] >= src_l[:, None]
    valid = ~pad
    names = ("duration", "pitch", "energy")
    preds_hip = {"duration": step.outs[4], "pitch": step.outs[2], "energy": step.outs[3]}
    dstack, dxin = step.rec.pred_inputs[-1]
    st = stack.double().cpu().reshape(3, B, Lp, d)
    for g, n in enumerate(names):
        pre = va + n + "_predictor."
        keeps = _site_masks(step, "pred", g)
        if keeps is not None:
            keeps = [(k[:, :Lb].contiguous(), pk) for k, pk in keeps]
        x64 = st[g, :, :Lb].clone()
        with torch.no_grad():
            with (oracle_with_masks(keeps) if p > 0 else _nothing()):
                out_o = ofs2.variance_predictor(P, pre, x64, pad, p, True)
            out_s, _ = predictor_restated(P, pre, x64, pad, keeps, p)
        assert float((out_s - out_o).abs().max()) <= 1e-9 * max(1.0, float(out_o.abs().max())), "restatement != oracle variance_predictor"
        acts = {"h1": h1.double().cpu().reshape(3, B, Lp, -1)[g, :, :Lb], "a1": a1.double().cpu().reshape(3, B, Lp, -1)[g, :, :Lb],
                "h2": h2.double().cpu().reshape(3, B, Lp, -1)[g, :, :Lb]}
        xr = x64.clone().requires_grad_(True)
        _zero_grads(P)
        tape = Tape()
        out, inter = predictor_restated(P, pre, xr, pad, keeps, p, hip=acts, Fn=tape)
        for nm_ in ("h1", "a1", "h2"):
            rep.out(n + "_predictor", nm_, acts[nm_].reshape(-1, acts[nm_].shape[-1]), inter[nm_].reshape(-1, acts[nm_].shape[-1]), valid.reshape(-1))
        # forward: the prediction; its magnitude term is the 256 -> 1 head's sum (a near-cancelling one for small predictions)
        head = [op for op in tape.ops if op[0] == "lin"][-1]
        mag = (head[1] ** 2 * head[2].detach()[0] ** 2).sum(-1).sqrt()[valid]
        hp, rp = preds_hip[n][:, :Lb].double()[valid], out.detach()[valid]
        err, bar = float((hp - rp).norm()), max(OUT_TAU * float(rp.norm()), KAPPA * U * float(mag.norm()))
        rep.add(n + "_predictor", "prediction |diff|", "%.3g" % err, "%.3g" % bar, err <= bar, "(|ref| %.3g)" % float(rp.norm()))
        out.backward(dstack[g].double().cpu()[:, :Lb])
        sc = tape.scales(P)
        for k in _keys_of(P, pre):
            rep.grad(n + "_predictor", k, step.hip[k], P[k].grad, sc.get(k, torch.zeros(1)))
        rep.dx(n + "_predictor", "input gradient", dxin[g].reshape(B, Lp, d)[:, :Lb], xr.grad)
    _zero_grads(P)
    # ---- variance-adaptor sums (modules.py order: x, x + speaker, + pitch embedding, + energy embedding) and the indices
    b = step.b
    pitch_t, energy_t = b[11], b[9]
    pidx_ref = torch.bucketize(pitch_t, m.get(va + "pitch_bins").cpu())
    eidx_ref = torch.bucketize(energy_t, m.get(va + "energy_bins").cpu())
    pidx, eidx = sv["pidx"].cpu().long().reshape(B, Lp)[:, :Lb], sv["eidx"].cpu().long().reshape(B, Lp)[:, :Lb]
    rep.add("variance_adaptor", "pitch / energy bin indices", "%d differ" % int((pidx != pidx_ref).sum() + (eidx != eidx_ref).sum()), "0",
            bool(torch.equal(pidx, pidx_ref) and torch.equal(eidx, eidx_ref)))
    spk = sv["speakers"].cpu().long()
    E_spk, E_p, E_e = (P[k].detach() for k in ("speaker_emb.weight", va + "pitch_embedding.weight", va + "energy_embedding.weight"))
    x0 = st[0, :, :Lb]
    x1 = x0 + E_spk[spk][:, None, :]
    x2 = x1 + E_p[pidx]
    x3 = x2 + E_e[eidx]
    allv = torch.ones(B * Lb, dtype=torch.bool)
    rep.out("variance_adaptor", "x + speaker (pitch input)", st[1, :, :Lb].reshape(-1, d), x1.reshape(-1, d), allv)
    rep.out("variance_adaptor", "+ pitch emb (energy input)", st[2, :, :Lb].reshape(-1, d), x2.reshape(-1, d), allv)
    # ---- LengthRegulator + position table -> decoder block 0's input
    blocks, n_enc = sv["blocks"], sv["n_enc"]
    Bn_, Lp_, T = sv["dims"]
    dur = b[10]
    idx, _ = ofs2.length_regulator_index(dur, T)
    gath = torch.gather(x3, 1, idx.clamp(min=0)[..., None].expand(-1, -1, d)) * (idx >= 0)[..., None]
    dec_in = gath + m.get("decoder.position_enc").detach().cpu().double()[:, :T]
    rep.out("length_regulator", "decoder input", blocks[n_enc][1], dec_in.reshape(-1, d))
    # ---- backward: segment sums of decoder block 0's input gradient
    dec0 = blocks[n_enc][0]
    dx_dec = dense(step.rec.fft[dec0][1], m, dec0).reshape(B, T, d)
    dx3_ref = torch.zeros(B, Lp, d, dtype=torch.float64)
    ok = idx >= 0
    bb = torch.arange(B)[:, None].expand(B, T)
    dx3_ref.index_put_((bb[ok], idx[ok]), dx_dec[ok], accumulate=True)
    dx3, (dx2, dx1, dxe) = step.rec.pred_grouped[-1]
    rep.out("length_regulator", "segment sums dx3", dx3, dx3_ref.reshape(-1, d))
    # ---- the adaptor's gradient sums (ops.va_combine) over the reference batch's positions
    dxin3 = dxin.double().cpu().reshape(3, B, Lp, d)[:, :, :Lb]
    dx3b = dx3.double().cpu().reshape(B, Lp, d)[:, :Lb]
    r2 = dx3b + dxin3[2]
    r1 = r2 + dxin3[1]
    r0 = r1 + dxin3[0]
    for what, hip, ref in (("dx2 = dx3 + d(energy input)", dx2, r2), ("dx1 = dx2 + d(pitch input)", dx1, r1), ("dx = dx1 + d(duration input)", dxe, r0)):
        rep.out("variance_adaptor", what, hip.reshape(B, Lp, d)[:, :Lb].reshape(-1, d), ref.reshape(-1, d), allv)

    # ---- embedding tables: sums of the recorded gradient rows (all positions of the reference batch, PAD included)
    def table(rows_g, ix, V):
        G = torch.zeros(V, d, dtype=torch.float64).index_add_(0, ix.reshape(-1), rows_g.reshape(-1, d))
        R = torch.zeros(V, d, dtype=torch.float64).index_add_(0, ix.reshape(-1), rows_g.reshape(-1, d) ** 2).sqrt()
        return G, R
    for k, rows_g, ix in ((va + "energy_embedding.weight", dx3b, eidx), (va + "pitch_embedding.weight", dx2.double().cpu().reshape(B, Lp, d)[:, :Lb], pidx),
                          ("speaker_emb.weight", dx1.double().cpu().reshape(B, Lp, d)[:, :Lb], spk[:, None].expand(B, Lb))):
        G, R = table(rows_g, ix, P[k].shape[0])
        rep.grad("embeddings", k, step.hip[k], G, R)
    # encoder.src_word_emb from encoder block 0's input gradient; padding_idx 0 gets nothing
    enc0 = blocks[0][0]
    dx_emb = dense(step.rec.fft[enc0][1], m, enc0).reshape(B, Lp, d)[:, :Lb]
    tx = sv["texts"].cpu().long().reshape(B, Lp)[:, :Lb]
    k = "encoder.src_word_emb.weight"
    G, R = table(dx_emb, tx, P[k].shape[0])
    G[0] = 0
    R[0] = 0
    rep.grad("embeddings", k, step.hip[k], G, R)
    nz0 = int((step.hip[k][0] != 0).sum())
    rep.add("embeddings", "src_word_emb padding_idx row", "%d nonzero" % nz0, "0", nz0 == 0)


def check_postnet_and_mel_linear(step, rep):
    """The PostNet layer by layer (conv, train-mode BatchNorm over the B x T rows the reference has, tanh, dropout: oracle/fs2.py
    postnet), its BatchNorm running statistics, and mel_linear behind it."""
    m, P, sv = step.m, step.P, step.sv
    Bn, Lp, T = sv["dims"]
    Tb = step.Tb                                # = frame_limit for a bucketed batch
    nm, d = m.n_mel, m.d
    pn = sv["pn"]
    douts = list(reversed(step.rec.bn))         # dout of layer i = the gradient of its output
    mel32 = step.outs[0].double()[:, :Tb]
    post = step.outs[1].double()[:, :Tb]
    dx_prev = None
    allrows = torch.ones(Bn * Tb, dtype=torch.bool)
    for i in range(5):
        pp, xin, yc, mean, rstd, keep = pn[i]
        unit = "postnet.%d" % i
        last = i == 4
        Cin = xin.shape[-1]
        C = yc.shape[-1]
        pk = _site_masks(step, "pn", i)
        p = m.p_post if pk is not None else 0.0
        kp = pk[0][0][:, :, :Tb].double() if pk is not None else None
        w, bconv, gam, bet = (P[pp + s] for s in ("0.conv.weight", "0.conv.bias", "1.weight", "1.bias"))
        xr = xin.double().cpu().reshape(Bn, T, Cin)[:, :Tb].clone().requires_grad_(True)
        if i == 0 and Tb < T:
            z = xin.reshape(Bn, T, Cin)[:, Tb:]
            rep.add(unit, "mel16 past frame_limit", "%d nonzero" % int((z != 0).sum()), "0", not bool((z != 0).any()))
        _zero_grads(P)
        ycr = F.conv1d(xr.transpose(1, 2), w, bconv, padding=(w.shape[2] - 1) // 2)
        ycr.retain_grad()
        ycs = ycr + (yc.double().cpu().reshape(Bn, T, C)[:, :Tb].transpose(1, 2) - ycr).detach()     # the BatchNorm reads HIP's fp32 conv output
        mu = ycs.mean((0, 2), keepdim=True)
        var = ycs.var((0, 2), unbiased=False, keepdim=True)
        rs = (var + 1e-5).rsqrt()
        xh = (ycs - mu) * rs
        ybn = xh * gam[None, :, None] + bet[None, :, None]
        ybn.retain_grad()
        y = ybn if last else torch.tanh(ybn)
        if p > 0:
            y = y * kp / (1.0 - p)
        # forward: the conv output, and the layer's output from the HIP conv output
        rep.out(unit, "conv output (fp32)", yc.reshape(Bn, T, C)[:, :Tb].reshape(-1, C), ycr.detach().transpose(1, 2).reshape(-1, C), allrows)
        with torch.no_grad():
            yh = yc.double().cpu().reshape(Bn, T, C)[:, :Tb].transpose(1, 2)
            muh, varh = yh.mean((0, 2), keepdim=True), yh.var((0, 2), unbiased=False, keepdim=True)
            o = (yh - muh) * (varh + 1e-5).rsqrt() * gam[None, :, None] + bet[None, :, None]
            o = o if last else torch.tanh(o)
            if p > 0:
                o = o * kp / (1.0 - p)
            o = o.transpose(1, 2)
            if last:
                rep.out(unit, "postnet mel = BN + mel", post.reshape(-1, nm), (o + mel32).reshape(-1, nm), allrows)
            else:
                rep.out(unit, "BN, tanh, dropout -> next input", pn[i + 1][1].reshape(Bn, T, C)[:, :Tb].reshape(-1, C), o.reshape(-1, C), allrows)
            n = yh.shape[0] * yh.shape[2]
            for s, ref in (("running_mean", 0.9 * step.bn0[pp + "1.running_mean"].double() + 0.1 * muh.flatten()),
                           ("running_var", 0.9 * step.bn0[pp + "1.running_var"].double() + 0.1 * varh.flatten() * n / max(n - 1, 1))):
                diff = float((step.bn1[pp + "1." + s].double() - ref).abs().max())
                bar = 1e-5 + 1e-4 * float(ref.abs().max())
                rep.add(unit, "BatchNorm " + s, "%.3g" % diff, "%.3g" % bar, diff <= bar)
        # backward from the recorded gradient of the layer's output
        g = douts[i].double().cpu().reshape(Bn, T, C)[:, :Tb]
        y.transpose(1, 2).backward(g)
        with torch.no_grad():
            gb = ybn.grad
            gy = gb * gam[None, :, None]
            # train-mode BatchNorm's backward: rstd (gy - mean(gy) - x_hat mean(gy x_hat)) cancels; the magnitude of its terms
            gmag = rs * (gy.abs() + gy.mean((0, 2), keepdim=True).abs() + xh.abs() * (gy * xh).mean((0, 2), keepdim=True).abs())
            x2 = xr.detach().transpose(1, 2) ** 2
            sc = {pp + "0.conv.weight": torch.nn.grad.conv1d_weight(x2, w.shape, gmag ** 2, padding=(w.shape[2] - 1) // 2).sqrt(),
                  pp + "0.conv.bias": (gmag ** 2).sum((0, 2)).sqrt(),
                  pp + "1.weight": ((gb * xh) ** 2).sum((0, 2)).sqrt(), pp + "1.bias": (gb ** 2).sum((0, 2)).sqrt()}
            dmag = F.conv_transpose1d(gmag ** 2, w.detach() ** 2, padding=(w.shape[2] - 1) // 2).sqrt().transpose(1, 2)
        for k in (pp + "0.conv.weight", pp + "0.conv.bias", pp + "1.weight", pp + "1.bias"):
            rep.grad(unit, k, step.hip[k], P[k].grad, sc[k])
        if i > 0:
            rep.dx(unit, "input gradient", douts[i - 1].reshape(Bn, T, Cin)[:, :Tb], xr.grad, mag=dmag)
        else:
            dx_prev = xr.grad.detach().clone()
    _zero_grads(P)
    # ---- mel_linear: dmel_tot = PostNet layer 0's input gradient (reference) + the mel terms' own gradient (dmel_sum), zero past Tb
    dmel = torch.zeros(Bn, T, nm, dtype=torch.float64)
    dmel[:, :Tb] = dx_prev + sv["dmel_sum"].double().cpu().reshape(Bn, T, nm)[:, :Tb]
    y = sv["dec_out"].double().cpu().reshape(Bn * T, d)
    W, bl = P["mel_linear.weight"].detach(), P["mel_linear.bias"].detach()
    rep.out("mel_linear", "mel (fp32)", step.outs[0][:, :Tb].reshape(-1, nm), (y @ W.t() + bl).reshape(Bn, T, nm)[:, :Tb].reshape(-1, nm))
    rep.out("mel_linear", "mel16 (PostNet input)", pn[0][1].reshape(Bn, T, nm)[:, :Tb].reshape(-1, nm),
            (y @ W.t() + bl).reshape(Bn, T, nm)[:, :Tb].reshape(-1, nm))
    g2 = dmel.reshape(-1, nm)
    rep.grad("mel_linear", "mel_linear.weight", step.hip["mel_linear.weight"], g2.t() @ y, (g2 ** 2).t().mm(y ** 2).sqrt())
    rep.grad("mel_linear", "mel_linear.bias", step.hip["mel_linear.bias"], g2.sum(0), (g2 ** 2).sum(0).sqrt())
    dec_last = sv["blocks"][-1][0]
    rep.dx("mel_linear", "input gradient", dense(step.rec.fft[dec_last][0], m, None), g2 @ W)


@pytest.mark.parametrize("name", NAMES)
def test_blocks_vs_fp64_on_their_own_inputs(cfg, name):
    step = Step(cfg, name)
    Bn, Lp, T = step.sv["dims"]
    print("case %s: B=%d L=%d T=%d (HIP %d / %d)" % (name, Bn, step.Lb, step.Tb, Lp, T))
    rep = Report(name)
    check_fft_blocks(step, rep)
    check_predictors_and_adaptor(step, rep)
    check_postnet_and_mel_linear(step, rep)
    rep.print()
    missing, extra = set(step.keys) - rep.covered, rep.covered - set(step.keys)
    assert not missing and not extra, ("covered key set != trainable key set", sorted(missing), sorted(extra))
    assert not rep.fails, "\n".join(rep.fails)
