"""CPU: the ground the batched text -> mel path (GraphedSynthesizer.mel_ragged) stands on.

1. The premise, on the oracle (pinned bit for bit to the reference): in the reference's padded batch an utterance that is not the
   longest gets a different last phoneme and a different length than it gets alone, because the variance predictors run
   Conv1d(k=3) -> ReLU -> LayerNorm twice with no mask in between (model/modules.py:255-309) and padded rows are non-zero.
2. The host-only bucket / key logic (tts_king_amd/batching.py).
3. The new kernels are declared in include/ttsk.h and exported by the library.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests.oracle_util import fs2_state_dict
from tts_king_amd import batching, lib
from tts_king_amd.config import default_config

LENS = (48, 31, 17, 40)
SPEAKERS = (5, 9, 2, 30)
LOGD_BAR = 0.06          # the project's HIP-vs-oracle log-duration bar (tests/test_facade_gpu.py)


def four_texts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(1, 207, (L,), generator=g) for L in LENS]


def oracle_weights():
    cfg = copy.deepcopy(default_config())
    sd = fs2_state_dict(cfg, 7, n_speakers=66)
    sd["variance_adaptor.duration_predictor.linear_layer.bias"].fill_(1.3)
    return cfg, sd


def test_reference_padded_batch_differs_from_solo_runs():
    cfg, sd = oracle_weights()
    texts = four_texts()
    Lmax = max(LENS)
    ids = torch.zeros(4, Lmax, dtype=torch.int64)
    for u, t in enumerate(texts):
        ids[u, :LENS[u]] = t
    with torch.no_grad():
        batch = ofs2.fs2_forward(sd, cfg.model_config, torch.tensor(SPEAKERS), ids, torch.tensor(LENS), Lmax)
        for u, t in enumerate(texts):
            solo = ofs2.fs2_forward(sd, cfg.model_config, torch.tensor([SPEAKERS[u]]), t[None], torch.tensor([LENS[u]]), LENS[u])
            L = LENS[u]
            d_logd = (batch[3][u, :L] - solo[3][0]).abs()
            d_pitch = float((batch[1][u, :L] - solo[1][0]).abs().max())
            T_b, T_s = int(batch[8][u]), int(solo[8][0])
            print("utterance %d: L %d, T in the batch %d, alone %d, max |dlogd| %.2g (last phoneme %.2g), max |dpitch| %.2g"
                  % (u, L, T_b, T_s, float(d_logd.max()), float(d_logd[-1]), d_pitch))
            if u == 0:                   # the longest has no padded rows: fp32 rounding only
                assert float(d_logd.max()) < 1e-4 and T_b == T_s
            else:
                assert float(d_logd[-1]) > LOGD_BAR, (u, float(d_logd[-1]))
                assert T_b != T_s, (u, T_b)
                assert float(d_logd[:-2].max()) < 1e-4          # two k = 3 convs reach two phonemes back, no further


def test_buckets_and_keys():
    rng = np.random.RandomState(0)
    mk = lambda lens: [rng.randint(1, 207, size=L) for L in lens]
    a = batching.plan_texts(mk((17, 31, 40, 48)), 1000)
    b = batching.plan_texts(mk((20, 25, 33, 41)), 1000)
    assert a.key == b.key == ("front", 4, 48)
    assert a.ids.shape == (4, 48) and a.ids.dtype == np.int64 and a.lens.tolist() == [17, 31, 40, 48]
    assert (a.ids[0, 17:] == 0).all() and (a.ids[0, :17] > 0).all()
    assert batching.plan_texts(mk((49, 3)), 1000).key == ("front", 2, 56)          # one past a bucket edge
    assert batching.plan_texts(mk((48, 3)), 1000).key == ("front", 2, 48)          # on it
    # frame buckets: totals within one 32-bucket share a key, whatever the individual lengths
    k1, o1, T1 = batching.plan_frames([232, 157, 61, 217], 1000)
    k2, o2, T2 = batching.plan_frames([225, 30, 256, 1], 1000)
    assert (k1, o1, T1) == ([0, 1, 2, 3], [], 256) and T2 == 256 and o2 == []
    assert batching.back_key(4, 48, T1) == batching.back_key(4, 48, T2) == ("back", 4, 48, 256)
    assert batching.plan_frames([257, 3], 1000)[2] == 288
    assert batching.plan_frames([0, 0], 1000)[2] == 32
    # both buckets are capped at max_seq_len, which is not a multiple of 32
    assert batching.bucket(995, 32, 1000) == 1000 and batching.bucket(999, 8, 1000) == 1000 and batching.bucket(1000, 8, 1000) == 1000
    assert batching.plan_texts(mk((999,)), 1000).L == 1000
    with pytest.raises(ValueError):
        batching.bucket(1001, 8, 1000)
    # an utterance over max_seq_len is split off, on either axis
    p = batching.plan_texts(mk((30, 1200, 12)), 1000)
    assert p.batch == [0, 2] and p.solo == [1] and p.key == ("front", 2, 32) and p.lens.tolist() == [30, 12]
    keep, over, T = batching.plan_frames([100, 1001, 40], 1000)
    assert keep == [0, 2] and over == [1] and T == 128
    assert batching.plan_frames([1001], 1000) == ([], [0], 0)
    assert batching.plan_texts(mk((1200,)), 1000).batch == []
    # `only`: the sub-batch that is run again after a split
    p = batching.plan_texts(mk((30, 50, 12)), 1000, only=[0, 2])
    assert p.batch == [0, 2] and p.L == 32


def test_controls_and_lists():
    c = batching.per_utterance(1.5, 4, "p_control")
    assert c.dtype == np.float32 and c.tolist() == [1.5] * 4
    assert batching.per_utterance([0.9, 1.0, 1.1, 1.0], 4, "d_control").tolist() == [np.float32(0.9), 1.0, np.float32(1.1), 1.0]
    assert batching.per_utterance(3, 2, "speakers", np.int64).tolist() == [3, 3]
    with pytest.raises(ValueError):
        batching.per_utterance([1.0, 1.0, 1.0], 4, "p_control")
    with pytest.raises(ValueError):
        batching.per_utterance([[1.0, 1.0]], 2, "p_control")
    assert batching.per_utterance_names("bea", 3, "speaker_names") == ["bea"] * 3
    assert batching.per_utterance_names(None, 2, "speaker_names") == [None, None]
    with pytest.raises(ValueError):
        batching.per_utterance_names(["a", "b"], 3, "speaker_names")
    rows = batching.as_id_rows([np.arange(1, 5), np.arange(1, 9)[None], [3, 4]])
    assert [r.shape for r in rows] == [(4,), (8,), (2,)] and all(r.dtype == np.int64 for r in rows)
    with pytest.raises(ValueError):
        batching.as_id_rows([])
    with pytest.raises(ValueError):
        batching.as_id_rows([np.zeros((2, 3), np.int64)])
    with pytest.raises(ValueError):
        batching.as_id_rows([np.zeros((0,), np.int64)])


NEW_SYMBOLS = ("ttsk_gather_add_lens", "ttsk_embed_step", "ttsk_duration_round_dev", "ttsk_zero_frames_lens", "ttsk_bn_apply_lens")


def test_new_entry_points_are_declared_and_exported():
    protos = lib.declared_prototypes()
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert name in protos and protos[name], name
        assert hasattr(l, name), name
        zero = [(None if a is lib.C.c_void_p else (0.0 if a in (lib.C.c_float, lib.C.c_double) else 0)) for a in protos[name]]
        assert getattr(l, name)(*zero) != 0, name + " accepted an all-null / all-zero argument list"
