"""GPU: speaker adaptation — FastSpeech2.set_trainable(units): the chosen parameter groups are trained, the rest stays frozen.

Per unit set ([speaker_emb], [speaker_emb, variance_adaptor, decoder], [postnet, mel_linear]): frozen state stays put over a
grad_acc_step = 4 cycle and two more updates; the updates follow the oracle restricted to the same units (the bars of
tests/test_parity_gpu.py::test_grad_acc_step_4_cycle_vs_oracle: losses 1 %, update norm ratio 10 %, cosine > 0.9; the clipped norm
within 2 %, that file's bar for the global norm); the trainable gradients equal the full backward's; the launches a frozen unit
would have caused are absent.  Then: rows of speakers that never appear do not move, the graph-replayed engine equals the eager one
bit for bit, and a checkpoint of a 64-speaker model grows to 65 speakers, trains its table and synthesizes with the new voice.

Shapes: B = 3 ragged, 24-48 phonemes, the seeded weights of fs2_state_dict(cfg, 7) — what the neighbouring tests use."""
import copy
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests.adapt_util import DEV, restrict_oracle, step_log
from tests.oracle_util import fs2_state_dict
from tests.test_parity_gpu import build, hip_dropout_masks, oracle_with_masks
from tts_king_amd import params as P
from tts_king_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"spk": ["speaker_emb"], "spk_va_dec": ["speaker_emb", "variance_adaptor", "decoder"], "post_mel": ["postnet", "mel_linear"]}
BN = ("running_mean", "running_var", "num_batches_tracked")
# for the gradient comparison also sets whose backward stops inside a stack or skips units in the middle
GRAD_SETS = dict(SETS, dec3=["decoder.3"], mixed=["embedding", "encoder.2", "decoder.0", "postnet"], enc1_va=["encoder.1", "variance_adaptor"])


def _units(m):
    return set(m.trainable_units)


def _dev(b):
    return [t.to(DEV) if torch.is_tensor(t) else t for t in b]


def _eval_mel(m, b):
    m.eval()
    with torch.no_grad():
        o = m(*_dev(b)[2:6])
    torch.cuda.synchronize()
    m.train()
    return o[9].float().cpu().clone(), o[8].cpu().clone()


# ---------------------------------------------------------------------------------------------------- the cycle, once per unit set
@pytest.fixture(scope="module")
def cycles(cfg):
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.optimizer import ScheduledOptim
    from tts_king_amd.train_step import main_train_step, to_device
    c = copy.deepcopy(cfg)
    assert c.train_config["optimizer"]["grad_acc_step"] == 4
    loss_fn = FastSpeech2Loss(c.preprocess_config, c.model_config)
    sd0 = fs2_state_dict(c, 7)
    batches = [make_batch(3, 24 + 8 * i, seed=60 + i, ragged=True) for i in range(4)]
    # a full-training run of the same four micro-steps: what the BatchNorm buffers do while no weight has moved yet
    full = build(c, 7, dropout=True)
    fopt = ScheduledOptim(full, c.train_config, c.model_config, 1000)
    for step in range(1, 4):
        main_train_step(full, to_device(batches[step - 1], DEV), step, fopt, c, loss_fn)
    torch.cuda.synchronize()
    bn_full = {k: v.detach().cpu().clone() for k, v in full.state_dict().items() if k.endswith(BN)}
    out = {"sd0": sd0, "bn_full3": bn_full, "cfg": c}
    for name, units in SETS.items():
        m = build(c, 7, dropout=True)
        m.set_trainable(units)
        opt = ScheduledOptim(m, c.train_config, c.model_config, 1000)
        m.sync_shadow()
        shadow0 = m.flat_buffers()[2].cpu().clone()
        tr = restrict_oracle(ofs2.OracleTrainer(sd0, copy.deepcopy(c.model_config), c.train_config, current_step=1000), _units(m))
        onorm, orig = [], tr.optimizer_step

        def rec(tr=tr, onorm=onorm, orig=orig):
            onorm.append(tr.grad_norm())
            orig()
        tr.optimizer_step = rec
        losses, bn3 = [], None
        for step in range(1, 5):
            b = batches[step - 1]
            masks = hip_dropout_masks(m, 3, int(b[5]), int(b[8]))
            vals, _ = main_train_step(m, to_device(b, DEV), step, opt, c, loss_fn)
            with oracle_with_masks(masks) as feeder:
                ovals, _ = tr.train_step(b, step)
            assert feeder.pos == 31
            losses.append((vals[:4], ovals[:4]))
            if step == 3:
                torch.cuda.synchronize()
                bn3 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k.endswith(BN)}
        torch.cuda.synchronize()
        gnorm = opt.grad_norm()
        sd4 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        for step in range(5, 13):                        # two more updates
            main_train_step(m, to_device(batches[step % 4], DEV), step, opt, c, loss_fn)
        torch.cuda.synchronize()
        out[name] = dict(m=m, opt=opt, tr=tr, losses=losses, gnorm=gnorm, onorm=onorm, sd4=sd4, bn3=bn3, shadow0=shadow0, batch=batches[0])
    return out


@pytest.mark.parametrize("name", list(SETS))
def test_frozen_state_stays_put(cycles, name):
    """After a grad_acc_step = 4 cycle and two more updates (dropout on): every frozen tensor of state_dict() holds its starting
    bits, so does its bf16 shadow; the trainable ones moved.  BatchNorm buffers are state, not parameters: through the first three
    micro-steps, before any weight has moved, they are bit for bit those of a full-training run on the same batches (afterwards
    the two runs have different weights, so only their count compares).  And shadow and packs are consistent: an eval forward
    equals, bit for bit, that of a fresh model loaded from the resulting state_dict()."""
    r, sd0, c = cycles[name], cycles["sd0"], cycles["cfg"]
    m, units = r["m"], _units(r["m"])
    assert r["opt"].current_step == 1003
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    moved = 0
    for k, v in sd.items():
        if k.endswith(BN):
            continue
        if P.unit_of(k) in units and m._table[k].kind == P.TRAIN:
            moved += int(not torch.equal(v, sd0[k]))
        else:
            assert torch.equal(v, sd0[k]), "frozen %s moved" % k
    assert moved >= max(1, len(m.trainable_keys()) - 8), "trainable tensors that did not move: %d of %d" % (len(m.trainable_keys()) - moved, len(m.trainable_keys()))
    for k, v in r["bn3"].items():
        assert torch.equal(v, cycles["bn_full3"][k]), k
    assert int(sd["postnet.convolutions.0.1.num_batches_tracked"]) == 12
    shadow = m.flat_buffers()[2].cpu()
    inside = torch.zeros(m._n_flat, dtype=torch.bool)
    for a, b in m.trainable_ranges():
        inside[a:b] = True
    assert torch.equal(shadow[~inside], r["shadow0"][~inside]) and not torch.equal(shadow[inside], r["shadow0"][inside])
    assert torch.equal(shadow[inside], m.flat_buffers()[0].cpu()[inside].to(torch.bfloat16))
    mel, lens = _eval_mel(m, r["batch"])
    fresh = build(c, 7, dropout=True)
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()})
    mel2, lens2 = _eval_mel(fresh, r["batch"])
    assert torch.equal(lens, lens2) and torch.equal(mel, mel2), "shadow / packs do not match the masters"


@pytest.mark.parametrize("name", list(SETS))
def test_updates_follow_the_restricted_oracle(cycles, name):
    """The first cycle against OracleTrainer with requires_grad_(False) on the frozen parameters, micro-step by micro-step under the
    keep-masks the HIP path draws."""
    r, sd0 = cycles[name], cycles["sd0"]
    tr, sd4 = r["tr"], r["sd4"]
    for i, (vals, ovals) in enumerate(r["losses"]):
        print("micro-step %d losses" % (i + 1), [round(v, 5) for v in vals], [round(v, 5) for v in ovals])
        np.testing.assert_allclose(vals, ovals, rtol=0.01)
    assert len(r["onorm"]) == 1 and tr.current_step == 1001
    print("%s: clipped norm HIP %.6f, restricted oracle %.6f" % (name, r["gnorm"], r["onorm"][0]))
    assert abs(r["gnorm"] - r["onorm"][0]) <= 0.02 * r["onorm"][0]
    assert sorted(tr.keys) == sorted(r["m"].trainable_keys())
    cos_min, worst = 1.0, None
    for k in tr.keys:
        if "w_ks.bias" in k or ("postnet" in k and k.endswith("conv.bias")):
            continue                                                         # true gradient 0: Adam normalises pure noise
        mine = (sd4[k] - sd0[k]).flatten().double()
        ref = (tr.sd[k].detach() - sd0[k]).flatten().double()
        cos = float((mine @ ref) / (mine.norm() * ref.norm() + 1e-30))
        if cos < cos_min:
            cos_min, worst = cos, k
        assert abs(float(mine.norm()) / float(ref.norm()) - 1) < 0.1, k
    print("%s: min cosine(update, oracle update) %.4f at %s" % (name, cos_min, worst))
    assert cos_min > 0.9
    for k in sd0:                                                            # the oracle's frozen parameters did not move either
        if k not in tr.keys and not k.endswith(BN):
            assert torch.equal(tr.sd[k].detach(), sd0[k]), k


# ---------------------------------------------------------------------------------------------------- one step: gradients, launches
def _one_backward(cfg, units, b, attrs=None, want_log=False):
    from tts_king_amd import ops
    m = build(cfg, 7, dropout=True).train()
    if units != "never":
        m.set_trainable(units)
    for k, v in (attrs or {}).items():
        setattr(m, k, v)
    d = _dev(b)
    if want_log:
        return m, step_log(m, b, d)
    with torch.no_grad():
        out, ctx = m._forward(True, d[2], d[3], d[4], int(b[5]), d[7], b[8], d[9], d[10], d[11], 1.0, 1.0, 1.0)
        _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(out[0], out[8], d[6], d[7], out[1], out[2], out[3], d[11], d[9], d[10], d[4], grad_scale=1.0)
        m.backward_native(ctx, dmel_sum, dpost, dp, de, dd, accumulate=False)
    torch.cuda.synchronize()
    return m, {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def full_grads(cfg):
    from tests.dw_schedule_util import CONFIGS
    b = make_batch(3, 40, seed=21, ragged=True)
    _, g = _one_backward(cfg, None, b)
    _, g2 = _one_backward(cfg, None, b, attrs=CONFIGS["no_side_stream"][0])
    return b, g, g2


@pytest.mark.parametrize("name", list(GRAD_SETS))
def test_trainable_gradients_equal_the_full_backwards(cfg, full_grads, name):
    """Same batch, same dropout state: a subset step's gradients of the trainable tensors are those of the full backward_native, bit
    for bit where the tensor's split-K partition is the same.  Where the smaller queue changed a partition, the bar is twice the
    distance the same tensor shows between the schedule configurations `default` and `no_side_stream` (tests/dw_schedule_util.py:
    the same sums in another slab order; the factor 2 for the different slab count)."""
    from tests.oracle_util import rel_rms
    b, g, g2 = full_grads
    m, sub = _one_backward(cfg, GRAD_SETS[name], b)
    assert sorted(sub) == sorted(m.trainable_keys())
    differ = []
    for k in sub:
        if torch.equal(sub[k], g[k]):
            continue
        bar = 2.0 * rel_rms(g2[k], g[k])
        got = rel_rms(sub[k], g[k])
        differ.append((k, got, bar))
        assert got <= bar, (k, got, bar)
    print("%s: %d of %d trainable gradient tensors bit-identical to the full backward's; the others %s" % (name, len(sub) - len(differ), len(sub), differ))


def _names(log):
    return [e[0] for e in log]


def test_launches_speaker_emb_only(cfg):
    """[speaker_emb]: no weight-gradient launch of any kind, the attention backward once per decoder block and never for an encoder
    block (the text axis is 40 phonemes long, the frame axis is not), one scatter-sum target (the speaker table)."""
    b = make_batch(3, 40, seed=21, ragged=True)
    m, log = _one_backward(cfg, ["speaker_emb"], b, want_log=True)
    names = _names(log)
    assert not [n for n in names if n in ("ttsk_dwgemm_batch", "ttsk_dwconv_batch", "ttsk_gemm_reduce_batch") or n.startswith("ttsk_gemm_group_launch")], names
    T, L = int(b[8]), int(b[5])
    assert T != L
    fa = [e for e in log if e[0] == "ttsk_flash_attention_bwd"]
    assert len(fa) == m.n_dec and all(T in e[2] and L not in e[2] for e in fa), fa
    sc = [e for e in log if e[0] == "ttsk_scatter_sum_batch"]
    assert len(sc) == 1 and sc[0][2][0] == 1, sc
    assert "ttsk_colsum_batch" not in names and "ttsk_colsum_finalize_batch" not in names
    assert len({e[1] for e in log}) <= 2, "main stream and the predictors' stream only"


def test_launches_postnet_mel_linear(cfg):
    """[postnet, mel_linear]: the decoder's backward does not run, nor the predictors' or anything below."""
    b = make_batch(3, 40, seed=21, ragged=True)
    _, log = _one_backward(cfg, ["postnet", "mel_linear"], b, want_log=True)
    names = _names(log)
    for n in ("ttsk_flash_attention_bwd", "ttsk_scatter_sum_batch", "ttsk_length_regulator_bwd", "ttsk_va_combine", "ttsk_layernorm_bwd_grouped"):
        assert n not in names, n
    assert "ttsk_dwgemm_batch" in names


def test_launches_default_equal_never_called(cfg):
    """set_trainable(None) — and every unit named — is today's path: the same launches on the same streams with the same counts."""
    b = make_batch(3, 40, seed=21, ragged=True)
    _, never = _one_backward(cfg, "never", b, want_log=True)
    _, none = _one_backward(cfg, None, b, want_log=True)
    _, every = _one_backward(cfg, ["postnet", "mel_linear", "decoder", "variance_adaptor", "speaker_emb", "encoder", "embedding"], b, want_log=True)
    assert len(never) > 100 and "ttsk_dwgemm_batch" in _names(never)
    assert none == never and every == never


# ---------------------------------------------------------------------------------------------------- rows of unseen speakers
def test_unseen_speaker_rows_do_not_move(cfg):
    """[speaker_emb], fresh optimizer state, batches of speaker 64 only: a row whose speaker never appears has g = m = v = 0, Adam's
    update of it is exactly zero — rows 0-63 keep their bits over three updates, row 64 moves."""
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.optimizer import ScheduledOptim
    from tts_king_amd.train_step import main_train_step, to_device
    c = copy.deepcopy(cfg)
    c.train_config["optimizer"]["grad_acc_step"] = 1
    m = build(c, 7, dropout=True)
    m.set_trainable(["speaker_emb"])
    opt = ScheduledOptim(m, c.train_config, c.model_config, 1000)
    loss_fn = FastSpeech2Loss(c.preprocess_config, c.model_config)
    w0 = m.get("speaker_emb.weight").detach().cpu().clone()
    for step in range(1, 4):
        b = list(make_batch(3, 24 + 8 * step, seed=80 + step, ragged=True))
        b[2] = torch.full_like(torch.as_tensor(b[2]), 64)
        main_train_step(m, to_device(tuple(b), DEV), step, opt, c, loss_fn)
    torch.cuda.synchronize()
    w = m.get("speaker_emb.weight").detach().cpu()
    assert opt.current_step == 1003
    assert torch.equal(w[:64], w0[:64]) and not torch.equal(w[64], w0[64])
    en = m._table["speaker_emb.weight"]
    assert float(opt.exp_avg[en.offset:en.offset + 64 * 256].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- the graph-replayed engine
@pytest.mark.parametrize("name", ["spk", "spk_va_dec"])
def test_graphed_engine_equals_eager(cfg, name):
    """Six steps of one shape through TrainEngine, hip_graph on (eager, capture, four replays) and off: the same weights, moments
    and losses, bit for bit."""
    from tests.test_engine_gpu import padded_device_batch
    from tts_king_amd.engine import TrainEngine
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.optimizer import ScheduledOptim
    c = copy.deepcopy(cfg)
    c.train_config["optimizer"]["grad_acc_step"] = 1
    finals = []
    for graphed in (True, False):
        m = build(c, 7, dropout=True)
        m.set_trainable(SETS[name])
        opt = ScheduledOptim(m, c.train_config, c.model_config, 50)
        eng = TrainEngine(m, opt, c, FastSpeech2Loss(c.preprocess_config, c.model_config), hip_graph=graphed)
        seen = []
        for step in range(1, 7):
            b = make_batch(3, 30, seed=500 + step, ragged=True, dur_hi=6)
            losses, _ = eng.step(padded_device_batch(b, 8, 64), step)
            seen.append(losses.cpu().tolist())
        torch.cuda.synchronize()
        finals.append((m.flat_buffers()[0].clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), seen, dict(eng.stats), opt.current_step))
    g, e = finals
    print("engine stats graphed", g[4], "eager", e[4])
    assert g[4]["captured"] == 1 and g[4]["replayed"] == 4 and g[4].get("capture_failed", 0) == 0 and e[4]["captured"] == 0
    assert g[5] == e[5] == 56
    assert g[3] == e[3], "losses differ between the graphed and the eager loop"
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])
    assert not torch.equal(g[0], build(c, 7).flat_buffers()[0])


# ---------------------------------------------------------------------------------------------------- a new voice, end to end
def test_new_speaker_end_to_end(cfg, tmp_path):
    """A checkpoint of a 64-speaker model, loaded by get_model under a speakers.json of 65 names with train_only: [speaker_emb]: two
    steps on the new speaker's batches, saved; loaded the way FSTWOapi loads a checkpoint (fsapi.py: the embedding re-inserted), the
    result synthesizes with speaker 64."""
    from tts_king_amd.fastspeech2 import FastSpeech2
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.train_step import get_model, main_train_step, save_checkpoint, to_device

    def conf(n):
        c = copy.deepcopy(cfg)
        root = str(tmp_path / ("prep%d" % n))
        os.makedirs(root, exist_ok=True)
        shutil.copy(os.path.join(ROOT, "pretrained", "stats.json"), os.path.join(root, "stats.json"))
        with open(os.path.join(root, "speakers.json"), "w") as f:
            json.dump({"spk%d" % i: i for i in range(n)}, f)
        c.preprocess_config.path.preprocessed_path = root
        c.train_config["optimizer"]["grad_acc_step"] = 1
        c.model_config["transformer"]["encoder_layer"] = c.model_config["transformer"]["decoder_layer"] = 2      # keep it quick
        return c
    c64 = conf(64)
    old = get_model(c64, DEV)
    ck64 = str(tmp_path / "ck64.pth.tar")
    save_checkpoint(old, None, ck64)
    c65 = conf(65)
    c65.tts["load_path"] = ck64
    c65.mi355x["train_only"] = ["speaker_emb"]
    m, opt = get_model(c65, DEV, train=True)
    assert m.n_speakers == 65 and m.trainable_units == ("speaker_emb",)
    w0 = m.get("speaker_emb.weight").detach().cpu().clone()
    assert torch.equal(w0[:64], old.get("speaker_emb.weight").detach().cpu())
    loss_fn = FastSpeech2Loss(c65.preprocess_config, c65.model_config)
    for step in (1, 2):
        b = list(make_batch(3, 32, seed=90 + step, ragged=True))
        b[2] = torch.full_like(torch.as_tensor(b[2]), 64)
        vals, _ = main_train_step(m, to_device(tuple(b), DEV), step, opt, c65, loss_fn)
        assert all(np.isfinite(vals[:4]))
    ck65 = str(tmp_path / "ck65.pth.tar")
    save_checkpoint(m, opt, ck65)
    ck = torch.load(ck65, map_location="cpu")
    assert ck["embedding"].shape == (65, 256) and torch.equal(ck["embedding"][:64], w0[:64]) and not torch.equal(ck["embedding"][64], w0[64])
    assert set(ck["optimizer"]["state"]) == {P.reference_parameter_keys(m._table).index("speaker_emb.weight")}
    for k, v in ck["model"].items():
        if not k.endswith(BN):
            assert torch.equal(v, old.state_dict()[k].cpu()), k
    api = FastSpeech2(c65.preprocess_config, c65.model_config, 65, device=DEV)
    state = ck["model"]
    state["speaker_emb.weight"] = ck["embedding"]
    api.load_state_dict(state)
    api.eval()
    ph = torch.arange(150, 170).view(1, -1).to(DEV)
    with torch.no_grad():
        new = api(torch.tensor([64], device=DEV), ph, torch.tensor([20], device=DEV), 20)[9].float().cpu()
        other = api(torch.tensor([3], device=DEV), ph, torch.tensor([20], device=DEV), 20)[9].float().cpu()
    assert new.shape[0] == 1 and new.shape[2] == 80 and new.shape[1] > 0 and bool(torch.isfinite(new).all())
    assert new.shape != other.shape or not torch.equal(new, other)
