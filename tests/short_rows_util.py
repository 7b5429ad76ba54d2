"""A generator with per-row lengths, restated on the CPU: the contract the *_rows kernels implement.

`generator_rows(sd, h, mel, lens)` is tests.test_windows_cpu.generator_any (hifi/models.py:185-201, ResBlock1 or ResBlock2) on a
rectangular batch whose row b holds an utterance of lens[b] frames: before EVERY convolution the activations of a row are set to
zero from lens[b] * (samples per frame at that stage) on, so each conv meets, at the row's end, the zero padding it meets at the
end of that utterance run alone.  The first lens[b] * 256 samples of row b are then the solo waveform."""
import torch
import torch.nn.functional as F

SPF = 256
ROW_LENS = (1, 13, 14, 15, 50, 95, 96)          # the batch of the CPU statement: one frame, around the V1 halo, mid, W - 1, W


def _masked(x, lens, s):
    """x (B, C, T * s) with the positions >= lens[b] * s of row b set to zero."""
    t = torch.arange(x.shape[2]).view(1, 1, -1)
    edge = (torch.as_tensor(lens) * s).view(-1, 1, 1)
    return torch.where(t < edge, x, torch.zeros((), dtype=x.dtype))


def generator_rows(sd, h, mel, lens, mask=True):
    """mel (B, 80, T), lens[b] <= T valid frames of row b -> (B, 1, 256 T).  `mask=False`: the plain generator on the same batch (a
    zero-padded mel without the per-layer masks: the negative control)."""
    m = (lambda x, s: _masked(x, lens, s)) if mask else (lambda x, s: x)
    lr = lambda t: F.leaky_relu(t, 0.1)
    x = F.conv1d(m(mel, 1), sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    nk = len(h["resblock_kernel_sizes"])
    s = 1
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(m(lr(x), s), sd["ups.%d.weight" % i], sd["ups.%d.bias" % i], stride=u, padding=(k - u) // 2)
        s *= u
        xs = 0
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p, y = "resblocks.%d." % (i * nk + j), x
            for n, d in enumerate(rd):
                if str(h["resblock"]) == "1":
                    t = F.conv1d(m(lr(y), s), sd[p + "convs1.%d.weight" % n], sd[p + "convs1.%d.bias" % n], dilation=d, padding=(rk * d - d) // 2)
                    y = F.conv1d(m(lr(t), s), sd[p + "convs2.%d.weight" % n], sd[p + "convs2.%d.bias" % n], padding=(rk - 1) // 2) + y
                else:
                    y = F.conv1d(m(lr(y), s), sd[p + "convs.%d.weight" % n], sd[p + "convs.%d.bias" % n], dilation=d, padding=(rk * d - d) // 2) + y
            xs = xs + y
        x = xs / nk
    return torch.tanh(F.conv1d(m(F.leaky_relu(x), s), sd["conv_post.weight"], sd["conv_post.bias"], padding=3))


def padded_batch(mels, T):
    """The (1, 80, T_b) mels as one (B, 80, T) batch, zero-padded."""
    out = torch.zeros(len(mels), mels[0].shape[1], T, dtype=mels[0].dtype)
    for b, mm in enumerate(mels):
        out[b, :, :mm.shape[2]] = mm[0]
    return out
