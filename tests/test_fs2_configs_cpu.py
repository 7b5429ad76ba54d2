"""CPU: the configurations of tests/fs2_configs.py against what the reference recorded for them (tests/golden/fs2_cfg_<name>.npz,
tools/make_goldens.py: g14_fs2_configs), and the configurations the constructor refuses.

* `params.build_entries` lists exactly the reference's state-dict keys, shapes and dtypes for every configuration (in its own, forward, order);
* the oracle reproduces each recorded eval forward within tests/test_oracle_golden.py's tolerance (it takes every shape from the
  state dict, so the same oracle then serves tests/test_fs2_configs_gpu.py);
* every configuration the kernels cannot run is refused by `params.build_entries` and by `FastSpeech2.__init__` (constructed on
  the CPU: no kernel runs) with a `params.ConfigError` that names the key, the value and the accepted values -- none gets as far
  as a kernel entry point's own check at the first forward."""
import os

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests import fs2_configs as FC
from tests.oracle_util import GOLDEN
from tests.test_oracle_golden import close
from tts_king_amd import params as P
from tts_king_amd.fastspeech2 import N_VOCAB


def golden(name):
    return np.load(os.path.join(GOLDEN, "fs2_cfg_%s.npz" % name))


def golden_inputs(g):
    """The recorded batch as the 15-tuple of tts_king_amd.synthetic.make_batch (CPU tensors)."""
    t = {k: torch.from_numpy(g[k]) for k in ("speakers", "texts", "src_lens", "mels", "mel_lens", "energies", "durations", "pitches")}
    B, L = t["texts"].shape
    ids = ["utt%04d" % i for i in range(B)]
    return (ids, ids, t["speakers"], t["texts"], t["src_lens"], L, t["mels"], t["mel_lens"], int(t["mels"].shape[1]), t["energies"],
            t["durations"], t["pitches"], torch.zeros(B, L, 11), torch.zeros(B), torch.ones(B))


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_build_entries_match_the_reference(cfg, name):
    g = golden(name)
    c = FC.config(cfg, name)
    entries = P.build_entries(c.model_config, FC.n_mel_of(c), FC.N_SPK, N_VOCAB)
    assert len(entries) == len(g["keys"]) and sorted(e.key for e in entries) == sorted(str(k) for k in g["keys"])
    want = {str(k): (tuple(int(x) for x in str(s).split(";")) if str(s) else (), str(dt)) for k, s, dt in zip(g["keys"], g["shapes"], g["dtypes"])}
    for e in entries:
        shape, dt = want[e.key]
        assert e.shape == shape, (e.key, e.shape, shape)
        assert ("int64" in dt) == (e.dtype == "int64"), (e.key, dt)


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_golden_batch_is_the_tables(cfg, name):
    """The recorded inputs are what tests/fs2_configs.py builds today (the GPU module feeds the HIP model from the table)."""
    g = golden(name)
    b, rec = FC.golden_batch(FC.config(cfg, name), name), golden_inputs(g)
    for i in (2, 3, 4, 6, 7, 9, 10, 11):
        assert torch.equal(b[i], rec[i]), i


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_oracle_reproduces_the_reference(cfg, name):
    g = golden(name)
    c = FC.config(cfg, name)
    sd = FC.state_dict_from_spec(c, g["keys"], g["shapes"], g["dtypes"], int(g["weight_seed"]))
    b = golden_inputs(g)
    with torch.no_grad():
        o = ofs2.fs2_forward(sd, c.model_config, *b[2:], train=False)
    close(o[0], g["mel"]); close(o[9], g["post"]); close(o[1], g["pitch"]); close(o[2], g["energy"]); close(o[3], g["logd"])
    assert o[8].tolist() == g["out_mel_lens"].tolist()
    if name == "short_table":             # the case is there for lengths past the table
        assert int(b[5]) > c.model_config["max_seq_len"] and o[0].shape[1] > c.model_config["max_seq_len"]


@pytest.mark.parametrize("name", list(FC.REFUSED))
def test_unsupported_configurations_are_refused_by_name(cfg, name):
    from tts_king_amd.fastspeech2 import FastSpeech2
    delta, n_mel, key = FC.REFUSED[name]
    c = FC.apply_delta(cfg, delta, n_mel)
    with pytest.raises(P.ConfigError) as e1:
        P.build_entries(c.model_config, FC.n_mel_of(c), FC.N_SPK, N_VOCAB)
    with pytest.raises(P.ConfigError) as e2:
        FastSpeech2(c.preprocess_config, c.model_config, FC.N_SPK, device="cpu")
    for e in (e1.value, e2.value):
        assert e.key == key, (e.key, key)
        assert key in str(e) and "accepted" in str(e) and e.accepted and repr(e.value) in str(e), str(e)


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_supported_configurations_construct_on_the_cpu(cfg, name):
    """... and the table's own entries are not refused: the model builds (its parameters carry the reference's shapes)."""
    from tts_king_amd.fastspeech2 import FastSpeech2
    g = golden(name)
    c = FC.config(cfg, name)
    m = FastSpeech2(c.preprocess_config, c.model_config, FC.N_SPK, device="cpu")
    sd = m.state_dict()
    assert sorted(sd.keys()) == sorted(str(k) for k in g["keys"])
    for k, s in zip(g["keys"], g["shapes"]):
        assert tuple(sd[str(k)].shape) == (tuple(int(x) for x in str(s).split(";")) if str(s) else ()), k
