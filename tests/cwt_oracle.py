"""The CWT pitch branch (model_config.use_cwt: True) restated on top of oracle.fs2's functions: plain torch, any float dtype, autograd.

reference: fs_two/model/modules.py:104-130 (get_pitch_embedding_cwt), :358-385 (CNNflat / CNNscalar), fs_two/cwt/cwt_utils.py:41-66
(inverse_batch_cwt and its batch-axis scaler), fs_two/model/loss.py:65-124, fs_two/model/fastspeech2.py:43-119.

`pitch_rows` (optional, (B, L) integer tensor): rows of the pitch embedding that replace the oracle's own bucketize result — a
position whose pitch sits next to a bin edge may land on the other side of it in another arithmetic, and everything downstream
then compares different embeddings; handing over the other side's rows keeps the rest of the comparison meaningful (the rows
themselves are compared separately).
`head_inputs` (optional, (x (B, L, 256), prediction (B, L, 11))): what the two CNNscalar heads read instead of the oracle's own
(x + speaker, prediction).  The reference detaches both inputs (modules.py:118-119), so the heads are a side branch: their outputs
reach only the pitch rows and their own two loss terms, their gradients reach only their own parameters.  pitch_std's gradients
are sums over the batch of (prediction - target) x Jacobian with terms of both signs that cancel to a small remainder, so a
0.2 % difference in the heads' INPUTS (bf16 activations) moves those tensors by tens of per cent; on the other side's inputs the
comparison is as well conditioned as any other.  Fixture helpers at the bottom are shared by the CPU and GPU tests and tools/make_goldens_cwt.py.
"""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fs2 as ofs2
from tts_king_amd.synthetic import make_batch, seeded_fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P_PITCH = 0.1          # VariancePredictor(model_config, output_size=11, dropout=0.1): modules.py:27-29
N_CWT = 11


def cnn_flat(sd, pre, x):
    """Conv1d(C, 1, 1) over time -> AdaptiveAvgPool1d(30) -> LayerNorm(30) -> ReLU.  x (B, L, C) -> (B, 1, 30)."""
    h = F.conv1d(x.transpose(1, 2), sd[pre + "net.0.weight"], sd[pre + "net.0.bias"])
    h = F.adaptive_avg_pool1d(h, 30)
    return F.relu(F.layer_norm(h, (30,), sd[pre + "net.2.weight"], sd[pre + "net.2.bias"]))


def cnn_scalar(sd, pre, x_one, x_two):
    """modules.py:373-385 -> (B, 1)."""
    s = cnn_flat(sd, pre + "flat_one.", x_one) + cnn_flat(sd, pre + "flat_two.", x_two)
    return F.relu(F.linear(s, sd[pre + "linear.weight"], sd[pre + "linear.bias"])).squeeze(1)


def inverse_batch_cwt(c):
    """cwt_utils.py:53-66: 10 of the 11 channels, weights (i + 3.5) ** -2.5, then (s - mean_b) / (std_b + 1e-12) over the BATCH axis."""
    w = torch.tensor([(i + 1 + 2.5) ** (-2.5) for i in range(10)], dtype=c.dtype)
    s = (c[:, :, :10] * w).sum(-1)
    return (s - s.mean(0, keepdim=True)) / (s.std(0, unbiased=False, keepdim=True) + 1e-12)


def variance_adaptor_cwt(sd, x, spk, src_pad, max_len, energy_t, dur_t, controls, mc, train, pitch_rows=None, head_inputs=None):
    p_c, e_c, d_c = controls
    pv = mc["variance_predictor"]["dropout"]
    va = "variance_adaptor."
    logd = ofs2.variance_predictor(sd, va + "duration_predictor.", x, src_pad, pv, train)
    x = x + spk
    cwt = ofs2.variance_predictor(sd, va + "pitch_predictor.", x, src_pad[..., None].repeat(1, 1, N_CWT), P_PITCH, train)
    hx, hc = (x.detach(), cwt.detach()) if head_inputs is None else (head_inputs[0].to(x.dtype), head_inputs[1].to(x.dtype))
    pm = cnn_scalar(sd, va + "pitch_mean.", hx, hc)
    ps = cnn_scalar(sd, va + "pitch_std.", hx, hc)
    pitch = inverse_batch_cwt(cwt) * ps + pm
    own_rows = torch.bucketize((pitch * p_c).detach(), sd[va + "pitch_bins"].to(pitch.dtype))
    rows = own_rows if pitch_rows is None else pitch_rows.long()
    x = x + F.embedding(rows, sd[va + "pitch_embedding.weight"])
    energy = ofs2.variance_predictor(sd, va + "energy_predictor.", x, src_pad, pv, train)
    if energy_t is not None:
        eidx = torch.bucketize(energy_t.to(energy.dtype), sd[va + "energy_bins"].to(energy.dtype))
    else:
        energy = energy * e_c
        eidx = torch.bucketize(energy, sd[va + "energy_bins"].to(energy.dtype))
    x = x + F.embedding(eidx, sd[va + "energy_embedding.weight"])
    if dur_t is not None:
        d_rounded = dur_t
        x, mel_len = ofs2.length_regulator(x, dur_t, max_len)
        mel_pad = None
    else:
        d_rounded = torch.clamp(torch.round(torch.exp(logd) - 1) * d_c, min=0)
        x, mel_len = ofs2.length_regulator(x, d_rounded, max_len)
        mel_pad = ofs2.mask_from_lengths(mel_len)
    return x, cwt, energy, logd, d_rounded, mel_len, mel_pad, pm, ps, pitch.detach(), own_rows


def fs2_forward_cwt(sd, mc, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None, e_targets=None,
                    d_targets=None, pitches_raw=None, pitches_cwt=None, pitches_mean=None, pitches_std=None, p_control=1.0,
                    e_control=1.0, d_control=1.0, train=False, bn_buffers=None, pitch_rows=None, head_inputs=None):
    """The reference's 12-tuple (slot 1 = the (B, L, 11) prediction, slots 10 / 11 = the (B, 1) heads) + (pitch (B, L), own rows)."""
    src_pad = ofs2.mask_from_lengths(src_lens, max_src_len)
    mel_pad = ofs2.mask_from_lengths(mel_lens, max_mel_len) if mel_lens is not None else None
    x = ofs2.encoder(sd, texts, src_pad, mc, train)
    spk = F.embedding(speakers, sd["speaker_emb.weight"])[:, None, :]
    x, cwt, energy, logd, d_rounded, mel_lens_out, mel_pad2, pm, ps, pitch, rows = variance_adaptor_cwt(
        sd, x, spk, src_pad, max_mel_len, e_targets, d_targets, (p_control, e_control, d_control), mc, train, pitch_rows, head_inputs)
    if mel_pad is None:
        mel_pad = mel_pad2
    x, mel_pad = ofs2.decoder(sd, x, mel_pad, mc, train)
    mel = F.linear(x, sd["mel_linear.weight"], sd["mel_linear.bias"])
    post = ofs2.postnet(sd, mel, train, bn_buffers) + mel
    return (mel, cwt, energy, logd, d_rounded, src_pad, mel_pad, src_lens, mel_lens_out, post, pm, ps, pitch, rows)


def fs2_loss_cwt(batch, out):
    """loss.py:24-134 with use_cwt: the 7-tuple, slots 5 / 6 = mean / std pitch terms."""
    mel_t, _, _, energy_t, dur_t = batch[6:11]
    cwt_t, mean_t, std_t = batch[12], batch[13], batch[14]
    mel, cwt, energy, logd, _, src_pad, mel_pad, _, _, post, pm, ps = out[:12]
    dt = mel.dtype
    src_ok, mel_ok = ~src_pad, ~mel_pad
    logd_t = torch.log(dur_t.to(dt) + 1)
    mel_t = mel_t.to(dt)[:, : mel_ok.shape[1], :] * mel_ok[..., None]
    mel = mel * mel_ok[..., None]
    post = post * mel_ok[..., None]
    mel_total = F.mse_loss(mel, mel_t) + F.l1_loss(mel, mel_t) + F.l1_loss(post, mel_t)
    ok11 = src_ok[..., None].repeat(1, 1, N_CWT)
    pitch_l = F.mse_loss(cwt.masked_select(ok11), cwt_t.to(dt).masked_select(ok11))
    energy_l = F.mse_loss(energy.masked_select(src_ok), energy_t.to(dt).masked_select(src_ok))
    dur_l = F.mse_loss(logd.masked_select(src_ok), logd_t.masked_select(src_ok))
    std_l = F.mse_loss(ps, std_t.to(dt)[:, None])
    mean_l = F.mse_loss(pm, mean_t.to(dt)[:, None])
    total = mel_total + dur_l + pitch_l + energy_l + mean_l + std_l
    return total, mel_total, pitch_l, energy_l, dur_l, mean_l, std_l


def trainable_keys_cwt(sd):
    skip = ("position_enc", "pitch_bins", "energy_bins", "running_mean", "running_var", "num_batches_tracked")
    return [k for k in sd if not any(s in k for s in skip)]


class CwtOracleTrainer(ofs2.OracleTrainer):
    """OracleTrainer on the CWT graph: the heads train too.  `rows_feed` (optional callable: micro-step index -> (B, L) rows, or
    (rows, head_inputs), or None)."""

    def __init__(self, sd, mc, tc, current_step=0, rows_feed=None):
        super().__init__(sd, mc, tc, current_step)
        for k in trainable_keys_cwt(self.sd):
            if k not in self.keys:
                self.keys.append(k)
                self.sd[k].requires_grad_(True)
                self.m[k] = torch.zeros_like(self.sd[k])
                self.v[k] = torch.zeros_like(self.sd[k])
        self.rows_feed, self.calls = rows_feed, 0

    def train_step(self, batch, step, train_mode=True):
        acc = self.tc["optimizer"]["grad_acc_step"]
        buffers = {}
        rows = self.rows_feed(self.calls) if self.rows_feed is not None else None
        rows, head_inputs = rows if isinstance(rows, tuple) else (rows, None)
        self.calls += 1
        out = fs2_forward_cwt(self.sd, self.mc, *batch[2:], train=train_mode, bn_buffers=buffers, pitch_rows=rows, head_inputs=head_inputs)
        losses = fs2_loss_cwt(batch, out)
        (losses[0] / acc).sum().backward()
        with torch.no_grad():
            for k, v in buffers.items():
                self.sd[k].copy_(v)
            for k in self.sd:
                if k.endswith("num_batches_tracked"):
                    self.sd[k] += 1
        vals = [float(l.sum()) / acc for l in losses[1:]]
        if step % acc == 0:
            self.optimizer_step()
        return vals, out


# ----------------------------------------------------------------------------------------------- fixtures
def _shape(s):
    return tuple(int(x) for x in s.split(";")) if s else ()


def cwt_config(cfg):
    c = copy.deepcopy(cfg)
    c.model_config["use_cwt"] = True
    return c


def revive_heads(sd):
    """With seeded_fill alone the last ReLU of pitch_std is dead for every row (prediction 0, all-zero gradients for the whole head): a
    broken head kernel would pass.  The parity fixtures make both heads' last layer positive."""
    for h in ("pitch_mean", "pitch_std"):
        pre = "variance_adaptor.%s.linear." % h
        with torch.no_grad():
            sd[pre + "weight"].copy_(0.25 * sd[pre + "weight"].abs())
            sd[pre + "bias"].fill_(0.25)
    return sd


def cwt_state_dict(cfg, weight_seed, n_speakers=65):
    """The CWT model's state_dict from the committed key / shape spec (fs2_cwt_state_dict_spec.npz), seeded_fill, heads revived."""
    import json
    spec = np.load(os.path.join(GOLDEN, "fs2_cwt_state_dict_spec.npz"))
    sd = {}
    for k, s, dt in zip(spec["keys"], spec["shapes"], spec["dtypes"]):
        sd[str(k)] = torch.zeros(_shape(str(s)), dtype=torch.int64 if "int64" in str(dt) else torch.float32)
    mc = cfg.model_config
    d = mc["transformer"]["encoder_hidden"]
    tab = ofs2.sinusoid_table(mc["max_seq_len"] + 1, d)[None]
    sd["encoder.position_enc"] = tab.clone()
    sd["decoder.position_enc"] = tab.clone()
    with open(os.path.join(cfg.preprocess_config.path.preprocessed_path, "stats.json")) as f:
        stats = json.load(f)
    nb = mc["variance_embedding"]["n_bins"]
    sd["variance_adaptor.pitch_bins"] = torch.linspace(stats["pitch"][0], stats["pitch"][1], nb - 1)
    sd["variance_adaptor.energy_bins"] = torch.linspace(stats["energy"][0], stats["energy"][1], nb - 1)
    if sd["speaker_emb.weight"].shape[0] != n_speakers:
        sd["speaker_emb.weight"] = torch.zeros(n_speakers, d)
    seeded_fill(sd, weight_seed)
    return revive_heads(sd)


def cwt_batch(B, L, seed, ragged=True, **kw):
    """make_batch with seeded random CWT targets instead of its zeros / 0 / 1 (which would test the three new loss terms next to nothing)."""
    b = list(make_batch(B, L, seed=seed, ragged=ragged, **kw))
    g = torch.Generator().manual_seed(seed + 7919)
    b[12] = torch.randn(B, L, N_CWT, generator=g)
    b[13] = 5.0 + 0.3 * torch.randn(B, generator=g)
    b[14] = 0.5 + torch.rand(B, generator=g)
    return tuple(b)


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def edge_between(bins, a, b):
    """Is there a bin edge e with min(a, b) < e <= max(a, b) (bucketize(right=False) gives a and b different rows exactly then)?"""
    lo, hi = torch.minimum(a, b).double(), torch.maximum(a, b).double()
    return torch.bucketize(lo, bins.double()) != torch.bucketize(hi, bins.double())
