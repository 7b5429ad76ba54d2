"""CPU: speaker adaptation's host side — trainable units (FastSpeech2.set_trainable), their ranges of the flat buffer, the optimizer's
checkpoint layout under frozen units (torch's: parameters without gradients carry no state), speaker-table growth in get_model, and
the combinations that are refused.  The device side is tests/test_adapt_optim_gpu.py (the range kernel) and tests/test_adapt_gpu.py."""
import copy
import json
import os
import shutil

import pytest
import torch

from tts_king_amd import params as P
from tts_king_amd.fastspeech2 import FastSpeech2
from tts_king_amd.optimizer import ScheduledOptim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_UNITS = ["postnet", "mel_linear", "decoder.5", "decoder.4", "decoder.3", "decoder.2", "decoder.1", "decoder.0", "variance_adaptor",
             "speaker_emb", "encoder.3", "encoder.2", "encoder.1", "encoder.0", "embedding"]


def _model(cfg, n_speakers=65):
    return FastSpeech2(cfg.preprocess_config, cfg.model_config, n_speakers, device="cpu")


def test_unit_names_prefixes_and_unknown_names(cfg):
    m = _model(cfg)
    assert P.unit_names(m.n_enc, m.n_dec) == ALL_UNITS
    assert m.trainable_units is None                                   # the default: everything
    m.set_trainable(["speaker_emb", "decoder"])
    assert m.trainable_units == ("decoder.5", "decoder.4", "decoder.3", "decoder.2", "decoder.1", "decoder.0", "speaker_emb")
    m.set_trainable(["encoder", "embedding"])
    assert m.trainable_units == ("encoder.3", "encoder.2", "encoder.1", "encoder.0", "embedding")
    m.set_trainable(None)
    assert m.trainable_units is None
    m.set_trainable(ALL_UNITS)                                         # every unit named: today's path
    assert m.trainable_units is None
    m.set_trainable(["postnet", "mel_linear", "decoder", "variance_adaptor", "speaker_emb", "encoder", "embedding"])
    assert m.trainable_units is None
    with pytest.raises(ValueError) as e:
        m.set_trainable(["speaker_emb", "speaker"])
    assert "'speaker'" in str(e.value) and all(u in str(e.value) for u in ALL_UNITS)
    with pytest.raises(ValueError):
        m.set_trainable(["decoder.6"])                                 # finer or other granularity than the units
    with pytest.raises(ValueError):
        m.set_trainable(["variance_adaptor.duration_predictor"])
    with pytest.raises(ValueError):
        m.set_trainable([])


def test_every_trainable_key_has_one_unit(cfg):
    m = _model(cfg)
    for k, en in m._table.items():
        u = P.unit_of(k)
        if en.kind == P.TRAIN:
            assert u in ALL_UNITS, k
    assert P.unit_of("speaker_emb.weight") == "speaker_emb" and P.unit_of("encoder.src_word_emb.weight") == "embedding"
    assert P.unit_of("variance_adaptor.pitch_embedding.weight") == "variance_adaptor"
    assert P.unit_of("decoder.layer_stack.3.pos_ffn.w_1.weight") == "decoder.3"


@pytest.mark.parametrize("units", [["speaker_emb"], ["speaker_emb", "variance_adaptor"], ["speaker_emb", "variance_adaptor", "decoder"],
                                   ["postnet", "mel_linear"], ["embedding", "encoder.2", "decoder.0", "postnet"]])
def test_trainable_ranges(cfg, units):
    m = _model(cfg)
    n = m._n_flat
    assert m.trainable_ranges() == [(0, n)]                            # None: one full range
    m.set_trainable(units)
    r = m.trainable_ranges()
    assert r == sorted(r) and all(a < b and a % 8 == 0 and b % 8 == 0 for a, b in r)
    assert all(r[i][1] < r[i + 1][0] for i in range(len(r) - 1)), "adjacent or overlapping ranges are merged"
    # with their complement they cover [0, n): every TRAIN entry lies wholly inside a range (trainable) or wholly outside (frozen)
    inside = torch.zeros(n, dtype=torch.bool)
    for a, b in r:
        assert 0 <= a and b <= n
        inside[a:b] = True
    want = torch.zeros(n, dtype=torch.bool)
    starts = set()
    for k, en in m._table.items():
        if en.kind != P.TRAIN:
            continue
        on = P.unit_of(k) in set(m.trainable_units)
        want[en.offset:en.offset + (en.numel + 7) // 8 * 8] = on
        starts.add(en.offset)
        assert m.get(k).requires_grad == on and (m.get(k).grad is not None) == on, k
    assert torch.equal(inside, want)
    assert all(a in starts for a, _ in r), "ranges are cut at entry boundaries"
    assert sorted(m.trainable_keys()) == sorted(k for k, en in m._table.items() if en.kind == P.TRAIN and P.unit_of(k) in set(m.trainable_units))
    if units == ["speaker_emb"]:
        en = m._table["speaker_emb.weight"]
        assert r == [(en.offset, en.offset + 65 * 256)]
    if units == ["postnet", "mel_linear"]:
        assert r == [(m._table["mel_linear.weight"].offset, n)]        # neighbours in the buffer: one merged range


def test_set_trainable_after_the_optimizer_raises(cfg):
    m = _model(cfg)
    m.set_trainable(["speaker_emb"])
    ScheduledOptim(m, cfg.train_config, cfg.model_config, 0)
    with pytest.raises(RuntimeError) as e:
        m.set_trainable(None)
    assert "before" in str(e.value)
    assert m.trainable_units == ("speaker_emb",)


def _fill(opt, seed, t):
    g = torch.Generator().manual_seed(seed)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g))
    opt.state[0], opt.state[1] = t, t
    opt._host_step = t


def test_optimizer_state_dict_holds_the_trainable_indices_only(cfg):
    m = _model(cfg)
    m.set_trainable(["speaker_emb", "variance_adaptor"])
    opt = ScheduledOptim(m, cfg.train_config, cfg.model_config, 0)
    _fill(opt, 3, 5)
    sd = opt.state_dict()
    keys = P.reference_parameter_keys(m._table)
    want = {i for i, k in enumerate(keys) if m._table[k].kind == P.TRAIN and P.unit_of(k) in ("speaker_emb", "variance_adaptor")}
    assert set(sd["state"]) == want and keys.index("speaker_emb.weight") in want
    assert sd["param_groups"][0]["params"] == list(range(len(keys)))
    # torch's own Adam over the reference's parameters, the frozen ones without gradients, accepts it
    ref = [torch.nn.Parameter(torch.zeros(m._table[k].shape), requires_grad=i in want) for i, k in enumerate(keys)]
    adam = torch.optim.Adam(ref, betas=opt.betas, eps=opt.eps)
    adam.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    i = keys.index("speaker_emb.weight")
    en = m._table["speaker_emb.weight"]
    assert torch.equal(adam.state_dict()["state"][i]["exp_avg"], opt.exp_avg[en.offset:en.offset + en.numel].view(65, 256))


def test_full_state_dict_loads_into_a_subset_optimizer(cfg):
    full = _model(cfg)
    of = ScheduledOptim(full, cfg.train_config, cfg.model_config, 0)
    _fill(of, 4, 9)
    sd = of.state_dict()
    assert len(sd["state"]) > 200
    m = _model(cfg)
    m.set_trainable(["speaker_emb"])
    opt = ScheduledOptim(m, cfg.train_config, cfg.model_config, 0)
    opt.load_state_dict(sd)
    en = m._table["speaker_emb.weight"]
    sl = slice(en.offset, en.offset + en.numel)
    assert torch.equal(opt.exp_avg[sl], of.exp_avg[sl]) and torch.equal(opt.exp_avg_sq[sl], of.exp_avg_sq[sl])
    rest = torch.ones(m._n_flat, dtype=torch.bool)
    rest[sl] = False
    assert float(opt.exp_avg[rest].abs().max()) == 0.0 and float(opt.exp_avg_sq[rest].abs().max()) == 0.0     # what is frozen is ignored
    assert int(opt.state[1]) == 9 and opt.current_step == 9
    assert set(opt.state_dict()["state"]) == {P.reference_parameter_keys(m._table).index("speaker_emb.weight")}


# ---------------------------------------------------------------------------------------------------- new speakers
def _prep(tmp_path, n_names):
    root = str(tmp_path / ("prep%d" % n_names))
    os.makedirs(root, exist_ok=True)
    shutil.copy(os.path.join(ROOT, "pretrained", "stats.json"), os.path.join(root, "stats.json"))
    with open(os.path.join(root, "speakers.json"), "w") as f:
        json.dump({"spk%d" % i: i for i in range(n_names)}, f)
    return root


def _small(cfg, tmp_path, n_names):
    c = copy.deepcopy(cfg)
    c.preprocess_config.path.preprocessed_path = _prep(tmp_path, n_names)
    c.model_config["transformer"]["encoder_layer"] = c.model_config["transformer"]["decoder_layer"] = 1
    return c


def _checkpoint(c, tmp_path, name):
    from tts_king_amd.train_step import get_model, save_checkpoint
    m = get_model(c, "cpu")
    path = str(tmp_path / name)
    save_checkpoint(m, None, path)
    return m, path


def test_speaker_table_growth(cfg, tmp_path):
    from tts_king_amd.train_step import get_model
    c64 = _small(cfg, tmp_path, 64)
    old, path = _checkpoint(c64, tmp_path, "ck64.pth.tar")
    emb = old.get("speaker_emb.weight").detach().clone()
    assert emb.shape == (64, 256)
    c66 = _small(cfg, tmp_path, 66)
    c66.tts["load_path"] = path
    c66.mi355x["train_only"] = ["speaker_emb"]
    m, opt = get_model(c66, "cpu", train=True)
    assert m.trainable_units == ("speaker_emb",) and opt._subset
    got = m.get("speaker_emb.weight").detach()
    assert got.shape == (66, 256) and torch.equal(got[:64], emb)                    # the loaded rows keep their indices, bit for bit
    mean = emb.double().mean(0)
    assert torch.equal(got[64], got[65]) and float((got[64].double() - mean).abs().max()) <= 1e-6 * float(mean.abs().max())
    m2 = get_model(c66, "cpu")
    assert torch.equal(m2.get("speaker_emb.weight"), got)                           # deterministic
    for k in old.state_dict():
        if k != "speaker_emb.weight":
            assert torch.equal(m.state_dict()[k], old.state_dict()[k]), k
    # ... or a copy of a named speaker's row
    c66.mi355x["new_speaker_init"] = "spk7"
    m3 = get_model(c66, "cpu")
    g3 = m3.get("speaker_emb.weight").detach()
    assert torch.equal(g3[:64], emb) and torch.equal(g3[64], emb[7]) and torch.equal(g3[65], emb[7])
    c66.mi355x["new_speaker_init"] = "nobody"
    with pytest.raises(ValueError) as e:
        get_model(c66, "cpu")
    assert "nobody" in str(e.value)
    c66.mi355x["new_speaker_init"] = "spk65"                                        # a name, but not one of the loaded rows
    with pytest.raises(ValueError):
        get_model(c66, "cpu")


def test_more_rows_than_names_raises_with_both_counts(cfg, tmp_path):
    from tts_king_amd.train_step import get_model
    c64 = _small(cfg, tmp_path, 64)
    _, path = _checkpoint(c64, tmp_path, "ck64.pth.tar")
    c60 = _small(cfg, tmp_path, 60)
    c60.tts["load_path"] = path
    with pytest.raises(ValueError) as e:
        get_model(c60, "cpu")
    assert "64" in str(e.value) and "60" in str(e.value)


# ---------------------------------------------------------------------------------------------------- refusals
def test_train_only_with_cwt_is_refused(cfg):
    c = copy.deepcopy(cfg)
    c.model_config["use_cwt"] = True
    m = FastSpeech2(c.preprocess_config, c.model_config, 65, device="cpu")
    with pytest.raises(NotImplementedError) as e:
        m.set_trainable(["speaker_emb"])
    assert "use_cwt" in str(e.value)
    m.set_trainable(None)                                                           # everything: nothing to refuse


def test_train_only_with_a_reducer_is_refused(cfg, tmp_path):
    from tts_king_amd.engine import TrainEngine
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.parallel import GradReducer
    from tts_king_amd.train_step import get_model, main_train_step
    c = _small(cfg, tmp_path, 3)
    c.mi355x["train_only"] = ["speaker_emb"]
    c.mi355x["gpus"] = 2
    with pytest.raises(NotImplementedError) as e:
        get_model(c, "cpu", train=True)
    assert "gpus" in str(e.value)
    c.mi355x["gpus"] = 1
    m, opt = get_model(c, "cpu", train=True)
    red = GradReducer(m.flat_buffers()[1], m.grad_buckets(24), m.group_offsets())
    loss = FastSpeech2Loss(c.preprocess_config, c.model_config)
    with pytest.raises(NotImplementedError):
        TrainEngine(m, opt, c, loss, reducer=red)
    with pytest.raises(NotImplementedError):
        main_train_step(m, None, 1, opt, c, loss, reducer=red)
    ctx = type("Ctx", (), {"used": False, "dims": (1, 8, 8), "preds": {}})()
    with pytest.raises(NotImplementedError):          # (refused before anything is launched)
        m.backward_native(ctx, None, None, None, None, None, on_bucket=red.on_group_done)


def test_weight_decay_is_still_refused(cfg):
    c = copy.deepcopy(cfg)
    c.train_config["optimizer"]["weight_decay"] = 0.01
    m = _model(c)
    m.set_trainable(["speaker_emb"])
    with pytest.raises(NotImplementedError):
        ScheduledOptim(m, c.train_config, c.model_config, 0)
