"""CPU: the HiFi-GAN V3 generator (`hifi: resblock: "2"` with the published config_v3 hyper-parameters) has the reference's
weight-normed and folded state-dict keys and shapes, as recorded from the reference in tests/golden/hifi_v3_b2_t32.npz, so that a
V3 checkpoint of the reference loads (hifi/models.py:104-143, :146-210)."""
import copy
import os

import numpy as np
import torch

from tests.oracle_util import GOLDEN

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])


def _shapes(arr):
    return [tuple(int(x) for x in str(s).split(";")) for s in arr]


def test_v3_state_dict_keys_and_shapes_match_the_reference(cfg):
    from tts_king_amd.hifigan import Generator
    g = np.load(os.path.join(GOLDEN, "hifi_v3_b2_t32.npz"))
    c = copy.deepcopy(cfg)
    for k, v in V3.items():
        c.hifi[k] = v
    gen = Generator(c.hifi)
    assert all(rb.kind == "2" and len(rb.dilation) == 2 for rb in gen.resblocks) and len(gen.resblocks) == 9
    sd = gen.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["wn_keys"]] and len(sd) == int(g["n_wn_keys"])
    assert [tuple(v.shape) for v in sd.values()] == _shapes(g["wn_shapes"])
    # a reference checkpoint (weight-normed) loads strictly; folding on the host gives the reference's folded layout
    ckpt = {k: torch.full(v.shape, 0.5) for k, v in sd.items()}
    gen.load_state_dict(ckpt, strict=True)
    gen.remove_weight_norm()
    sdf = gen.state_dict()
    assert list(sdf.keys()) == [str(k) for k in g["keys"]] and len(sdf) == int(g["n_folded_keys"])
    assert [tuple(v.shape) for v in sdf.values()] == _shapes(g["shapes"])
