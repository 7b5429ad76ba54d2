"""What tests/test_hifigan_generic_gpu.py compares the conv-by-conv HiFi-GAN route with, and what tests/test_hifigan_v2_cpu.py runs
its negative controls on: the published V2 configuration (config_v2: V1's ResBlock1s and upsamplers from 128 channels, so the last
two stages are 16 and 8 channels wide), fp64 references of the implicit-GEMM conv and the polyphase transposed conv with the
epilogues that route uses, and the expected 16-bit outputs of an integer-valued case.

`mutation` puts one deliberate defect into a reference, in the manner of tests/flash_ref.py's `reference(mutation=...)`:
  "drop_tap"            the last tap of phase 0 of a transposed conv is lost
  "zero_cols"           output channels 8..15 of a conv stay zero
  "c2_before_residual"  the second (activated) output is taken from the conv before the residual is added
`generator_any(mutation=...)` in tests/test_windows_cpu.py has the same three for the whole generator."""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hifigan as ohifi
from tests.oracle_util import GOLDEN
from tts_king_amd.synthetic import seeded_fill

V2 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])
V2_GOLDEN = os.path.join(GOLDEN, "hifi_v2_b2_t32.npz")

# the whole-generator bars held for V1 (tests/test_hifigan_gpu.py): rel-RMS, max-abs at fp16 storage; rel-RMS at bf16 storage
V1_BAR_F16 = (0.005, 0.01)
V1_BAR_BF16 = 0.015
CAL_FACTOR = 1.5


def v2_config(cfg):
    c = copy.deepcopy(cfg)
    for k, v in V2.items():
        c.hifi[k] = copy.deepcopy(v)
    return c


def v2_state_dict_wn(weight_seed):
    g = np.load(V2_GOLDEN)
    sd = {str(k): torch.zeros(tuple(int(x) for x in str(s).split(";"))) for k, s in zip(g["wn_keys"], g["wn_shapes"])}
    seeded_fill(sd, weight_seed)
    return sd


def v2_folded(weight_seed):
    return ohifi.fold_weight_norm(v2_state_dict_wn(weight_seed))


def calibration(sd, h, mel, dt):
    """(rel-RMS, max-abs) of the fp64 restatement with its weights and every stored activation rounded to `dt`, against the plain
    one: what the storage type alone costs at this configuration and shape.  Returns the plain waveform too."""
    from tests.oracle_util import rel_rms
    from tests.test_windows_cpu import generator_any
    sd64 = {k: v.double() for k, v in sd.items()}
    sdq = {k: (v.to(dt).double() if k.endswith("weight") else v.double()) for k, v in sd.items()}
    with torch.no_grad():
        want = generator_any(sd64, h, mel.double())
        got = generator_any(sdq, h, mel.to(dt).double(), q=lambda t: t.to(dt).double())
    return rel_rms(got, want), float((got - want).abs().max()), want


def lrelu32(v, slope):
    """LeakyReLU as the kernels' epilogues compute it: in fp32, the slope an fp32 value."""
    v = v.float()
    return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))


def conv1d_ref(x, w, b, dil, R=None, mutation=None):
    """'same' Conv1d in fp64 on channels-last x (B, T, Cin), w (Cout, Cin, k), b (Cout,), residual R (B, T, Cout) or None ->
    (v, v2): v = conv + bias (+ R), what the first output stores (after LRELU_OUT where set), and v2, what the second output
    activates — the same tensor unless a mutation says otherwise."""
    assert mutation in (None, "zero_cols", "c2_before_residual")
    k = w.shape[2]
    c = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), dilation=dil, padding=dil * (k - 1) // 2).transpose(1, 2)
    if mutation == "zero_cols":
        c = c.clone()
        c[:, :, 8:16] = 0
    v = c if R is None else c + R.double()
    return v, (c if mutation == "c2_before_residual" else v)


def conv_transpose_ref(x, w, b, s, k, mutation=None):
    """ConvTranspose1d(stride s, padding (k - s) // 2) in fp64 on channels-last x (B, T, Cin), w (Cin, Cout, k) -> (B, T * s, Cout)."""
    assert mutation in (None, "drop_tap")
    w = w.double()
    if mutation == "drop_tap":
        w = w.clone()
        w[:, :, (k // s - 1) * s] = 0                 # phase 0 owns taps 0, s, 2 s, ...
    return F.conv_transpose1d(x.double().transpose(1, 2), w, b.double(), stride=s, padding=(k - s) // 2).transpose(1, 2)


def stored(v, dt, slope=None):
    """The 16-bit tensor an epilogue stores for the fp32 value v (an integer-valued case: v is exact in fp32): optionally
    LeakyReLU in fp32, then one rounding."""
    v = v.float()
    return (v if slope is None else lrelu32(v, slope)).to(dt)
