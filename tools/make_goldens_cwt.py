#!/usr/bin/env python3
"""Generate tests/golden/fs2_cwt_*.npz by running the REFERENCE implementation with `use_cwt: True` (build container only).

The reference is imported the way tools/make_goldens.py imports it (stub modules for the preprocessing-only dependencies), its weights
come from `seeded_fill` (weight seed 7) with both CNNscalar heads' last layer made positive (tests/cwt_oracle.py: revive_heads — with
the plain fill pitch_std's final ReLU is dead for every row), the batches from tests/cwt_oracle.py: cwt_batch (make_batch with seeded
random CWT targets).  Only data is stored: inputs are regenerated from seeds, outputs are arrays.

    python tools/make_goldens_cwt.py        # rewrites tests/golden/fs2_cwt_*.npz
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
for name in ("pycwt", "unidecode", "inflect"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["unidecode"].unidecode = lambda s: s
sys.modules["inflect"].engine = lambda: None

from tts_king_amd.synthetic import seeded_fill  # noqa: E402
from tests.cwt_oracle import cwt_batch, revive_heads  # noqa: E402


class AD(dict):
    def __init__(self, d):
        super().__init__({k: AD(v) if isinstance(v, dict) else v for k, v in d.items()})
    __getattr__ = dict.__getitem__


cfg = AD(yaml.safe_load(open(os.path.join(REF, "config.yaml"))))
cfg.preprocess_config.path["preprocessed_path"] = os.path.join(REF, "pretrained")
cfg.model_config["use_cwt"] = True

from fs_two.model import FastSpeech2, FastSpeech2Loss  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
N_SPK = 65
WEIGHT_SEED = 7
SMALL = ["variance_adaptor.pitch_mean.flat_one.net.0.weight", "variance_adaptor.pitch_mean.flat_two.net.0.weight",
         "variance_adaptor.pitch_mean.flat_one.net.2.weight", "variance_adaptor.pitch_mean.linear.weight",
         "variance_adaptor.pitch_std.flat_one.net.0.bias", "variance_adaptor.pitch_std.flat_two.net.2.bias",
         "variance_adaptor.pitch_std.flat_two.net.0.weight", "variance_adaptor.pitch_std.linear.bias",
         "variance_adaptor.pitch_predictor.linear_layer.weight", "variance_adaptor.pitch_predictor.linear_layer.bias",
         "variance_adaptor.energy_predictor.conv_layer.layer_norm_1.bias", "mel_linear.bias"]


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def new_model():
    torch.manual_seed(0)
    m = FastSpeech2(cfg.preprocess_config, cfg.model_config, N_SPK)
    sd = m.state_dict()
    seeded_fill(sd, WEIGHT_SEED)
    revive_heads(sd)
    return m


def pitch_of(m, o):
    """The (B, L) pitch the reference buckets, recomputed from its outputs with its own function."""
    from fs_two.cwt.cwt_utils import inverse_batch_cwt
    return inverse_batch_cwt(o[1].detach().clone()) * o[11].detach() + o[10].detach()


def spec():
    m = new_model()
    sd = m.state_dict()
    np.savez_compressed(os.path.join(OUT, "fs2_cwt_state_dict_spec.npz"), keys=np.array(list(sd.keys())),
                        shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
                        dtypes=np.array([str(v.dtype) for v in sd.values()]),
                        trainable=np.array([k for k, p in m.named_parameters() if p.requires_grad]),
                        n_params=sum(p.numel() for p in m.parameters()))
    print("spec keys", len(sd))


def eval_tf():
    m = new_model().eval()
    b = cwt_batch(4, 64, 11)
    with torch.no_grad():
        o = m(*b[2:])
    pitch = pitch_of(m, o)
    np.savez_compressed(os.path.join(OUT, "fs2_cwt_eval.npz"), B=4, L=64, seed=11, weight_seed=WEIGHT_SEED, cwt=npy(o[1]), energy=npy(o[2]),
                        logd=npy(o[3]), pitch_mean=npy(o[10]), pitch_std=npy(o[11]), pitch=npy(pitch), mel_lens=npy(o[8]),
                        mel=npy(o[0][:2]), post=npy(o[9][:2]))
    print("eval heads", o[10].view(-1).tolist(), o[11].view(-1).tolist(), "buckets", len(torch.bucketize(pitch, m.variance_adaptor.pitch_bins).unique()))


def train_p0():
    import torch.nn.functional as F
    orig = F.dropout
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    try:
        m = new_model().train()
        loss_fn = FastSpeech2Loss(cfg.preprocess_config, cfg.model_config)
        b = cwt_batch(4, 64, 11)
        o = m(*b[2:])
        ls = loss_fn(b, o)
        ls[0].backward()
    finally:
        F.dropout = orig
    named = dict(m.named_parameters())
    keys = sorted(k for k, p in named.items() if p.grad is not None)
    gn = np.array([float(named[k].grad.norm()) for k in keys])
    grads = {("grad/" + k): npy(named[k].grad) for k in SMALL}
    grads["grad/variance_adaptor.pitch_embedding.weight[:, :8]"] = npy(named["variance_adaptor.pitch_embedding.weight"].grad[:, :8])
    np.savez_compressed(os.path.join(OUT, "fs2_cwt_train_p0.npz"), B=4, L=64, seed=11, weight_seed=WEIGHT_SEED,
                        losses=np.array([float(l.sum()) for l in ls]), grad_keys=np.array(keys), grad_norms=gn, cwt=npy(o[1]),
                        energy=npy(o[2]), logd=npy(o[3]), pitch_mean=npy(o[10]), pitch_std=npy(o[11]), pitch=npy(pitch_of(m, o)),
                        mel=npy(o[0][:2]), post=npy(o[9][:2]), **grads)
    print("train losses", [round(float(l.sum()), 5) for l in ls], "n_grads", len(keys))


DUR_BIAS = 1.3


def eval_free_b1():
    m = new_model().eval()
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.linear_layer.bias.fill_(DUR_BIAS)
    b = cwt_batch(1, 48, 12, ragged=False)
    with torch.no_grad():
        o = m(b[2], b[3], b[4], b[5], d_control=0.9, p_control=1.5, e_control=1.2)
    np.savez_compressed(os.path.join(OUT, "fs2_cwt_free_b1.npz"), B=1, L=48, seed=12, weight_seed=WEIGHT_SEED, controls=np.array([0.9, 1.5, 1.2]),
                        dur_bias=DUR_BIAS, cwt=npy(o[1]), energy=npy(o[2]), logd=npy(o[3]), d_rounded=npy(o[4]), mel_lens=npy(o[8]),
                        pitch_mean=npy(o[10]), pitch_std=npy(o[11]), pitch=npy(pitch_of(m, o)), mel=npy(o[0]), post=npy(o[9]))
    print("free B=1 mel", tuple(o[0].shape), "pitch const", float(pitch_of(m, o).std()))


if __name__ == "__main__":
    spec()
    eval_tf()
    train_p0()
    eval_free_b1()
