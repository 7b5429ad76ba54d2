"""CPU: the CWT pitch branch (use_cwt: True) — parameter inventory against the reference's state_dict spec, and the helper oracle
(tests/cwt_oracle.py) against the reference's recorded outputs, losses and gradients (tests/golden/fs2_cwt_*.npz, written by
tools/make_goldens_cwt.py).

Tolerance: fp32 vs fp32 on the same torch build, a few ops in another association order: rtol 1e-4 / atol 2e-5, as
tests/test_oracle_golden.py uses for the plain branch."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests import cwt_oracle as CO
from tests.oracle_util import GOLDEN
from tts_king_amd import params as P

RT, AT = 1e-4, 2e-5


def close(a, b, rtol=RT, atol=AT):
    np.testing.assert_allclose(np.asarray(a.detach() if torch.is_tensor(a) else a), np.asarray(b), rtol=rtol, atol=atol)


def _entries(cfg, cwt):
    mc = copy.deepcopy(cfg.model_config)
    mc["use_cwt"] = cwt
    return P.build_entries(mc, 80, 65, 207)


def _check_spec(entries, spec):
    want = {str(k): str(s) for k, s in zip(spec["keys"], spec["shapes"])}
    got = {e.key: ";".join(map(str, e.shape)) for e in entries}
    assert got == want and len(entries) == len(want)


def test_entries_with_flag_match_reference_spec(cfg):
    spec = np.load(os.path.join(GOLDEN, "fs2_cwt_state_dict_spec.npz"))
    entries = _entries(cfg, True)
    _check_spec(entries, spec)
    by = {e.key: e for e in entries}
    assert by["variance_adaptor.pitch_predictor.linear_layer.weight"].shape == (11, 256)
    assert by["variance_adaptor.pitch_predictor.linear_layer.bias"].shape == (11,)
    heads = [e for e in entries if e.key.startswith(("variance_adaptor.pitch_mean.", "variance_adaptor.pitch_std."))]
    assert len(heads) == 20 and all(e.kind == P.TRAIN for e in heads)
    # every parameter the reference trains is in the flat buffer now
    table, total = P.layout(entries)
    train = sorted(k for k, e in table.items() if e.kind == P.TRAIN)
    assert train == sorted(str(k) for k in spec["trainable"] if not any(s in str(k) for s in ("position_enc", "_bins")))
    # forward order: the heads follow the predictors and precede the embeddings; each head is one 456-float block
    keys = [e.key for e in entries]
    assert keys.index("variance_adaptor.energy_predictor.linear_layer.bias") < keys.index(heads[0].key) < keys.index(heads[-1].key) < \
        keys.index("variance_adaptor.pitch_embedding.weight")
    assert table[heads[10].key].offset - table[heads[0].key].offset == 456
    # the buckets cover the heads
    bk = P.buckets(table, total, 1 << 20)
    lo, hi = table[heads[0].key].offset, table[heads[-1].key].offset
    assert any(s <= lo < e for s, e in bk) and any(s <= hi < e for s, e in bk)
    assert bk[0][1] == total and bk[-1][0] == 0 and all(a[0] == b[1] for a, b in zip(bk, bk[1:]))
    # Adam's parameter indices follow the reference's model.parameters() order
    assert [k for k in P.reference_parameter_keys(table) if table[k].kind == P.TRAIN] == [str(k) for k in spec["trainable"]]


def test_entries_without_flag_unchanged(cfg):
    spec = np.load(os.path.join(GOLDEN, "fs2_state_dict_spec.npz"))
    entries = _entries(cfg, False)
    _check_spec(entries, spec)
    table, total = P.layout(entries)
    assert sum(e.numel for e in table.values() if e.kind == P.TRAIN) == 34624395 - 840
    assert all(e.kind == P.UNUSED for k, e in table.items() if ".pitch_mean." in k or ".pitch_std." in k)
    assert table["variance_adaptor.pitch_predictor.linear_layer.weight"].shape == (1, 256)
    # the same order, kinds and offsets as the flagged inventory outside the pitch predictor's head and the CNNscalar heads
    flagged, _ = P.layout(_entries(cfg, True))
    assert list(flagged) == list(table)
    first = table["variance_adaptor.pitch_predictor.linear_layer.weight"].offset
    for k, e in table.items():
        if e.kind == P.TRAIN and e.offset < first:
            assert flagged[k].offset == e.offset and flagged[k].kind == e.kind, k


def _golden_case(cfg, name):
    g = np.load(os.path.join(GOLDEN, name))
    c = CO.cwt_config(cfg)
    sd = CO.cwt_state_dict(c, int(g["weight_seed"]))
    return g, c, sd


def test_fixture_heads_alive_and_buckets_stable(cfg):
    """The three fixture conditions: no row of either head is dead, the pitch spans many buckets, and the fp32 oracle picks the
    bucket its fp64 self picks at every position — at both parity fixtures."""
    c = CO.cwt_config(cfg)
    sd = CO.cwt_state_dict(c, 7)
    sd64 = CO.to64(sd)
    for (B, L, seed), min_buckets in (((4, 64, 11), 40), ((16, 64, 1234), 60)):
        b = CO.cwt_batch(B, L, seed)
        with torch.no_grad():
            o = CO.fs2_forward_cwt(sd, c.model_config, *b[2:], train=False)
            o64 = CO.fs2_forward_cwt(sd64, c.model_config, *b[2:], train=False)
        pm, ps = o[10].view(-1), o[11].view(-1)
        print("B=%d heads mean %s std %s buckets %d" % (B, [round(float(v), 3) for v in pm], [round(float(v), 3) for v in ps], len(o[13].unique())))
        assert float(pm.min()) > 0.5 and float(ps.min()) > 0.5, (pm, ps)          # no dead row (a dead ReLU gives exactly 0)
        assert len(o[13].unique()) >= min_buckets
        assert torch.equal(o[13], o64[13])
        print("fp32 oracle pitch vs fp64: max abs %.3g" % float((o[12].double() - o64[12]).abs().max()))
    # and what the fixture repairs: with the plain fill pitch_std is dead at B = 4
    plain = CO.cwt_state_dict(c, 7)
    from tts_king_amd.synthetic import seeded_fill
    seeded_fill(plain, 7)
    b = CO.cwt_batch(4, 64, 11)
    with torch.no_grad():
        o = CO.fs2_forward_cwt(plain, c.model_config, *b[2:], train=False)
    assert float(o[11].abs().max()) == 0.0


def test_oracle_eval_matches_reference(cfg):
    g, c, sd = _golden_case(cfg, "fs2_cwt_eval.npz")
    b = CO.cwt_batch(int(g["B"]), int(g["L"]), int(g["seed"]))
    with torch.no_grad():
        o = CO.fs2_forward_cwt(sd, c.model_config, *b[2:], train=False)
    assert tuple(o[1].shape) == (4, 64, 11) and tuple(o[10].shape) == (4, 1) and tuple(o[11].shape) == (4, 1)
    close(o[1], g["cwt"]); close(o[2], g["energy"]); close(o[3], g["logd"])
    close(o[10], g["pitch_mean"]); close(o[11], g["pitch_std"])
    close(o[12], g["pitch"], atol=2e-4)        # ill-conditioned where a column's batch std is small (fp32 vs fp32 in another order)
    assert o[8].tolist() == g["mel_lens"].tolist()
    close(o[0][:2], g["mel"]); close(o[9][:2], g["post"])
    # PAD rows of the prediction are zero in all 11 channels
    pad = ofs2.mask_from_lengths(b[4], b[5])
    assert float(o[1][pad].abs().max()) == 0.0


def test_oracle_train_matches_reference(cfg):
    g, c, sd = _golden_case(cfg, "fs2_cwt_train_p0.npz")
    keys = CO.trainable_keys_cwt(sd)
    assert sorted(keys) == sorted(str(k) for k in g["grad_keys"])
    for k in keys:
        sd[k].requires_grad_(True)
    b = CO.cwt_batch(int(g["B"]), int(g["L"]), int(g["seed"]))
    keep = ofs2._drop
    ofs2._drop = lambda x, p, train: x
    try:
        o = CO.fs2_forward_cwt(sd, c.model_config, *b[2:], train=True, bn_buffers={})
        ls = CO.fs2_loss_cwt(b, o)
        ls[0].backward()
    finally:
        ofs2._drop = keep
    close(np.array([float(l.detach()) for l in ls]), g["losses"], rtol=1e-4)
    assert float(ls[5]) > 1.0 and float(ls[6]) > 0.01          # the two head terms are live
    close(o[1], g["cwt"]); close(o[10], g["pitch_mean"]); close(o[11], g["pitch_std"])
    close(o[0][:2], g["mel"]); close(o[9][:2], g["post"])
    gn = dict(zip((str(k) for k in g["grad_keys"]), g["grad_norms"]))
    for k in keys:
        np.testing.assert_allclose(float(sd[k].grad.norm()), gn[k], rtol=2e-4, atol=1e-7, err_msg=k)
    n = 0
    for name in g.files:
        if not name.startswith("grad/"):
            continue
        k = name[5:]
        if k.endswith("[:, :8]"):
            got = sd[k[:-7]].grad[:, :8]
        else:
            got = sd[k].grad
        close(got, g[name], rtol=2e-4, atol=2e-6)
        n += 1
    assert n == 13
    # the heads send nothing back and the pitch embedding collects at the PREDICTED rows only
    pe = sd["variance_adaptor.pitch_embedding.weight"].grad
    used = torch.zeros(pe.shape[0], dtype=torch.bool)
    used[o[13].view(-1)] = True
    assert float(pe[~used].abs().max()) == 0.0 and float(pe[used].abs().sum()) > 0


def test_oracle_b1_constant_pitch_and_lonely_column(cfg):
    g, c, sd = _golden_case(cfg, "fs2_cwt_free_b1.npz")
    sd["variance_adaptor.duration_predictor.linear_layer.bias"].fill_(float(g["dur_bias"]))
    b = CO.cwt_batch(int(g["B"]), int(g["L"]), int(g["seed"]), ragged=False)
    dc, pc, ec = [float(x) for x in g["controls"]]
    with torch.no_grad():
        o = CO.fs2_forward_cwt(sd, c.model_config, b[2], b[3], b[4], b[5], d_control=dc, p_control=pc, e_control=ec, train=False)
    np.testing.assert_array_equal(o[4].numpy(), g["d_rounded"])
    assert o[8].tolist() == g["mel_lens"].tolist()
    close(o[1], g["cwt"]); close(o[10], g["pitch_mean"]); close(o[11], g["pitch_std"]); close(o[0], g["mel"]); close(o[9], g["post"])
    # B = 1: z = 0 / 1e-12 = 0 exactly, the pitch is the predicted mean at every phoneme
    assert torch.equal(o[12], o[10].expand_as(o[12]))
    close(o[12], g["pitch"])
    # a column where every row but one is padding: its batch statistics come from one value and B - 1 zeros
    c4 = torch.zeros(4, 6, 11)
    c4[2, 5, :] = torch.arange(11.0) - 3.0
    c4[:, :5, :] = torch.randn(4, 5, 11, generator=torch.Generator().manual_seed(3))
    z = CO.inverse_batch_cwt(c4)
    s = float((c4[2, 5, :10] * torch.tensor([(i + 3.5) ** -2.5 for i in range(10)])).sum())
    mean, std = s / 4, (3 * (s / 4) ** 2 / 4 + (s - s / 4) ** 2 / 4) ** 0.5
    np.testing.assert_allclose(z[:, 5].numpy(), [(0 - mean) / std] * 2 + [(s - mean) / std] + [(0 - mean) / std], rtol=1e-5)
    assert torch.equal(CO.inverse_batch_cwt(torch.zeros(3, 4, 11)), torch.zeros(3, 4))      # an all-PAD column: 0 / 1e-12


def test_abi_exports_cwt_symbols():
    from tts_king_amd import lib
    names = lib.declared_symbols()
    want = ["ttsk_layernorm_head_fwd", "ttsk_layernorm_head_bwd", "ttsk_layernorm_head_bwd_nblocks", "ttsk_cnnscalar_fwd", "ttsk_cnnscalar_bwd",
            "ttsk_cwt_pitch", "ttsk_fs2_loss_cwt"]
    l = lib.load()
    for n in want:
        assert n in names and hasattr(l, n), n
    assert set(lib.declared_prototypes()) == set(names)


def test_model_constructs_with_flag_on_cpu(cfg):
    """Construction, state_dict round trip with the reference's keys and shapes, and the loss module — no device work."""
    from tts_king_amd.fastspeech2 import FastSpeech2
    from tts_king_amd.loss import FastSpeech2Loss
    c = CO.cwt_config(cfg)
    m = FastSpeech2(c.preprocess_config, c.model_config, 65, device="cpu")
    assert m.use_cwt and not m.group_predictors and m.p_pitch == 0.1
    sd = CO.cwt_state_dict(c, 7)
    m.load_state_dict(sd)
    out = m.state_dict()
    assert set(out) == set(sd)
    for k in ("variance_adaptor.pitch_predictor.linear_layer.weight", "variance_adaptor.pitch_std.linear.weight",
              "variance_adaptor.pitch_mean.flat_one.net.0.weight", "variance_adaptor.pitch_mean.flat_two.net.2.bias"):
        assert torch.equal(out[k], sd[k]) and out[k].shape == sd[k].shape, k
    # the twenty head tensors are views of the flat buffer, with gradient views
    p = m.get("variance_adaptor.pitch_std.flat_two.net.0.weight")
    assert p.requires_grad and p.grad is not None and p.grad.shape == (1, 11, 1)
    assert p.data_ptr() >= m._flat.data_ptr() and p.data_ptr() < m._flat.data_ptr() + 4 * m._flat.numel()
    FastSpeech2Loss(c.preprocess_config, c.model_config)
    with pytest.raises(NotImplementedError):
        c2 = CO.cwt_config(cfg)
        c2.model_config["multi_speaker"] = False
        FastSpeech2(c2.preprocess_config, c2.model_config, 65, device="cpu")
