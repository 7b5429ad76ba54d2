"""FastSpeech2Loss with the reference's call signature, computed (value AND gradient) by one fused HIP kernel.

reference: fs_two/model/loss.py:5-134.  `forward(inputs, predictions)` takes the 15-tuple batch and the model's
12-tuple and returns `(total, mel_total, pitch, energy, duration, mean_pitch, std_pitch)`; `total` has shape (1,)
as in the reference (it adds `torch.tensor([0])` twice, loss.py:114-124).
"""
import torch
import torch.nn as nn

from . import ops


class _LossFn(torch.autograd.Function):
    """Autograd face of the fused kernel: only d(total) is propagated (that is what train.py:43-44 uses)."""

    @staticmethod
    def forward(ctx, mel, post, pitch, energy, logd, targets):
        losses, *_ = ops.fs2_loss(mel.detach(), post.detach(), *targets[:2], pitch.detach(), energy.detach(), logd.detach(),
                                  *targets[2:], grad_scale=1.0)
        ctx.save_for_backward(mel, post, pitch, energy, logd)
        ctx.targets = targets
        return losses

    @staticmethod
    def backward(ctx, dlosses):
        mel, post, pitch, energy, logd = ctx.saved_tensors
        scale = float(dlosses[0])           # host read: compatibility path only (train_step.py has the sync-free path)
        _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(mel.detach(), post.detach(), *ctx.targets[:2], pitch.detach(),
                                                      energy.detach(), logd.detach(), *ctx.targets[2:], grad_scale=scale)
        dmel = ops.add_f32(dmel_sum, dpost, scale_b=-1.0)
        return dmel, dpost, dp, de, dd, None


class _LossFnCwt(torch.autograd.Function):
    """The same for the CWT branch (loss.py:65-124 with use_cwt): the (B, L, 11) prediction and the two (B, 1) heads."""

    @staticmethod
    def forward(ctx, mel, post, pitch, energy, logd, pm, ps, targets, cwt_targets):
        heads = torch.stack([pm.detach().reshape(-1), ps.detach().reshape(-1)]).float().contiguous()
        losses, *_ = ops.fs2_loss_cwt(mel.detach(), post.detach(), *targets[:2], pitch.detach().contiguous(), heads, energy.detach(),
                                      logd.detach(), *cwt_targets, *targets[3:], grad_scale=1.0)
        ctx.save_for_backward(mel, post, pitch, energy, logd, pm, ps)
        ctx.targets, ctx.cwt_targets = targets, cwt_targets
        return losses

    @staticmethod
    def backward(ctx, dlosses):
        mel, post, pitch, energy, logd, pm, ps = ctx.saved_tensors
        scale = float(dlosses[0])           # host read: compatibility path only
        heads = torch.stack([pm.detach().reshape(-1), ps.detach().reshape(-1)]).float().contiguous()
        _, dmel_sum, dpost, dc, de, dd, dh = ops.fs2_loss_cwt(mel.detach(), post.detach(), *ctx.targets[:2], pitch.detach().contiguous(), heads,
                                                              energy.detach(), logd.detach(), *ctx.cwt_targets, *ctx.targets[3:],
                                                              grad_scale=scale)
        dmel = ops.add_f32(dmel_sum, dpost, scale_b=-1.0)
        return dmel, dpost, dc, de, dd, dh[0].view_as(pm), dh[1].view_as(ps), None, None


class FastSpeech2Loss(nn.Module):
    def __init__(self, preprocess_config, model_config):
        super().__init__()
        self.pitch_feature_level = preprocess_config["preprocessing"]["pitch"]["feature"]
        self.energy_feature_level = preprocess_config["preprocessing"]["energy"]["feature"]
        self.use_cwt = bool(model_config["use_cwt"])

    @staticmethod
    def cwt_targets_of(inputs, device):
        """(pitches_cwt (B, L, 11), pitches_mean (B,), pitches_std (B,)) of the 15-tuple batch, fp32 on `device` (NaN -> 0 as in to_device)."""
        f = lambda t: torch.nan_to_num(torch.as_tensor(t).to(device).float(), nan=0.0).contiguous()
        return (f(inputs[12]), f(inputs[13]), f(inputs[14]))

    @staticmethod
    def targets_of(inputs, device):
        """(mel_target, mel_lens, pitch_t, energy_t, dur_t, src_lens) from the 15-tuple batch, on `device`."""
        mel_t, mel_lens, energy_t, dur_t, pitch_t = inputs[6], inputs[7], inputs[9], inputs[10], inputs[11]
        src_lens = inputs[4]
        f = lambda t: t.to(device).float().contiguous()
        i = lambda t: t.to(device).long().contiguous()
        return (f(mel_t), i(mel_lens), f(pitch_t), f(energy_t), i(dur_t), i(src_lens))

    def forward(self, inputs, predictions):
        mel, pitch, energy, logd = predictions[0], predictions[1], predictions[2], predictions[3]
        post = predictions[9]
        targets = self.targets_of(inputs, mel.device)
        if self.use_cwt:
            losses = _LossFnCwt.apply(mel, post, pitch, energy, logd, predictions[10], predictions[11], targets,
                                      self.cwt_targets_of(inputs, mel.device))
            return (losses[0:1], losses[1], losses[2], losses[3], losses[4], losses[5], losses[6])
        losses = _LossFn.apply(mel, post, pitch, energy, logd, targets)
        zero = torch.zeros(1, dtype=torch.int64, device=mel.device)
        return (losses[0:1], losses[1], losses[2], losses[3], losses[4], zero, zero)
