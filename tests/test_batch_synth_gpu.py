"""GPU: batched text -> mel for texts of different lengths, every utterance as if run alone (`FSTWOapi.generate_batch`,
`GraphedSynthesizer.mel_ragged`, `TTSKing.generate_mel` / `speak` with lists).

The yardstick is the reference's SOLO run through the oracle, with the bars tests/test_facade_gpu.py::
test_free_running_second_control_setting_through_to_the_waveform already holds: log-durations within 0.06, durations obeying the
reference's rounding rule, every disagreement across a rounding boundary, mel rel-RMS <= 1.5 % against the oracle teacher-forced on
the HIP path's own durations / pitch / energy.  The reference's PADDED batch misses the log-duration bar by 0.75-0.9 at the last
phoneme of every utterance that is not the longest (tests/test_batch_synth_cpu.py), and so does the existing `model(...)` forward,
which follows the reference: that is the negative control here.

Against the HIP solo run the predictions must be bit-equal and the mels within twice the yardstick the EXISTING batching shows
(profiles/batch_synth_parity.json, measured on the parent commit by tools/batch_synth_parity.py; torch.equal if it is exactly 0).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests.oracle_util import rel_rms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENS = (48, 31, 17, 40)
SPEAKERS = (5, 9, 2, 30)
DC = (0.9, 1.0, 1.1, 1.0)
PC = (1.5, 1.0, 0.8, 1.2)
EC = (1.2, 1.0, 1.0, 0.9)
LOGD_BAR = 0.06
VOCODER_SOLO_BAR = 1e-3          # windowed vocoder vs `forward` on the utterance alone (tests/test_windows_gpu.py)


def make_tts(tmp_path, hip_graph, use_cwt=False):
    import yaml
    import tts_king
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config.yaml")))
    cfg["preprocess_config"]["path"]["preprocessed_path"] = os.path.join(ROOT, "pretrained")
    cfg["mi355x"]["hip_graph"] = hip_graph
    if use_cwt:
        cfg["model_config"]["use_cwt"] = True
    p = tmp_path / ("config_%d_%d.yaml" % (hip_graph, use_cwt))
    p.write_text(yaml.safe_dump(cfg))
    t = tts_king.TTSKing(str(p))
    with torch.no_grad():       # random-init duration head predicts ~0 frames: shift it so utterances have a few frames per phoneme
        t.tts.model.get("variance_adaptor.duration_predictor.linear_layer.bias").fill_(1.3)
    return t


def four_texts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(1, 207, (L,), generator=g).numpy() for L in LENS]


def mel_bar():
    with open(os.path.join(ROOT, "profiles", "batch_synth_parity.json")) as f:
        return 2.0 * float(json.load(f)["yardstick_rel_rms"])


def assert_mel(got, want, what):
    """The mel bar against the HIP solo run, on ALL valid frames."""
    bar = mel_bar()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    r = rel_rms(got.cpu(), want.cpu())
    print("%s: rel-RMS %.3e (bar %.3e)%s" % (what, r, bar, "  bit-equal" if torch.equal(got, want) else ""))
    if bar == 0.0:
        assert torch.equal(got, want), what
    else:
        assert r <= bar, (what, r, bar)


def solo(tts, text, u_spk, dc, pc, ec):
    """The HIP solo run of one text, as `GraphedSynthesizer.mel` runs it: eval_front + eval_back on (1, L)."""
    m = tts.tts.model
    m.eval()
    dev = m.device
    L = len(text)
    with torch.no_grad():
        x3, dur, total, aux = m.eval_front(torch.tensor([u_spk], device=dev), torch.from_numpy(text[None]).long().to(dev),
                                           torch.tensor([L], device=dev), L, pc, ec, dc)
        T = max(int(total.max().item()), 1)
        mel, post, _, _ = m.eval_back(x3, dur, L, T)
    return {"pitch": aux[0][0], "energy": aux[1][0], "logd": aux[2][0], "dur": dur.view(-1), "mel": mel[0], "post": post[0], "T": T}


def boundary_between(vr, vh):
    bnd = math.floor(vr) + 0.5
    if abs(vr - bnd) > 0.5:
        bnd += 1.0
    return min(vr, vh) - 1e-5 <= bnd <= max(vr, vh) + 1e-5


def test_each_utterance_against_the_reference_solo_run(tmp_path):
    tts = make_tts(tmp_path, False)
    texts = four_texts()
    names = [tts.speakers[s] for s in SPEAKERS]
    mels, aux = tts.tts.generate_batch(texts, list(DC), list(PC), list(EC), names, aux=True)
    m = tts.tts.model
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    mc = tts.cfg.model_config
    last = []
    for u, text in enumerate(texts):
        L, dc, pc, ec = LENS[u], DC[u], PC[u], EC[u]
        spk, ids, sl = torch.tensor([SPEAKERS[u]]), torch.from_numpy(text[None]).long(), torch.tensor([L])
        with torch.no_grad():
            ref = ofs2.fs2_forward(sd, mc, spk, ids, sl, L, p_control=pc, e_control=ec, d_control=dc)        # the reference, ALONE
        logd_h, logd_r = aux[u]["logd"].float().cpu()[None], ref[3].float()
        diff = (logd_h - logd_r).abs()
        last.append(float(diff[0, -1]))
        print("utterance %d (L %d): max |logd - solo oracle| %.4f, at the last phoneme %.4f" % (u, L, float(diff.max()), last[-1]))
        assert float(diff.max()) <= LOGD_BAR, (u, float(diff.max()))
        d_h, d_r = aux[u]["dur"].float().cpu()[None], ref[4].float()
        v_h, v_r = torch.exp(logd_h) - 1.0, torch.exp(logd_r) - 1.0
        rule = torch.clamp(torch.round(v_h) * dc, min=0.0)
        assert bool((((v_h - torch.floor(v_h) - 0.5).abs() < 1e-5) | (rule == d_h)).all()), u
        for bi, li in (d_h != d_r).nonzero().tolist():
            assert boundary_between(float(v_r[bi, li]), float(v_h[bi, li])), (u, li, float(v_h[bi, li]), float(v_r[bi, li]))
        T = mels[u].shape[1]
        assert mels[u].shape == (1, T, 80) and mels[u].dtype == torch.float32
        assert int(d_h.clamp(min=0).trunc().sum()) == T, (u, T)
        with torch.no_grad():      # the oracle teacher-forced on the HIP path's own durations, pitch and energy (they only pick rows)
            ref = ofs2.fs2_forward(sd, mc, spk, ids, sl, L, d_targets=d_h, max_mel_len=T, mel_lens=torch.tensor([T]),
                                   pitches_raw=aux[u]["pitch"].float().cpu()[None], e_targets=aux[u]["energy"].float().cpu()[None])
        r = rel_rms(mels[u].cpu(), ref[9])
        print("utterance %d: T %d, mel vs the solo oracle on the HIP durations / pitch / energy: rel-RMS %.3f%%" % (u, T, 100 * r))
        assert r <= 0.015, (u, r)
    print("last-phoneme |logd - solo oracle| of the four utterances: %s (the reference's padded batch: 0.75-0.9 for 1-3)"
          % ", ".join("%.4f" % x for x in last))


def test_each_utterance_against_the_hip_solo_run_and_negative_control(tmp_path):
    tts = make_tts(tmp_path, False)
    texts = four_texts()
    names = [tts.speakers[s] for s in SPEAKERS]
    mels, aux = tts.tts.generate_batch(texts, list(DC), list(PC), list(EC), names, aux=True)
    m = tts.tts.model
    # negative control: the existing forward on the same padded batch follows the reference (one control setting per call there)
    Lmax = max(LENS)
    ids = np.zeros((4, Lmax), dtype=np.int64)
    for u, t in enumerate(texts):
        ids[u, :LENS[u]] = t
    with torch.no_grad():
        padded = m(torch.tensor(SPEAKERS), torch.from_numpy(ids), torch.tensor(LENS), Lmax)
        mels1, aux1 = tts.tts.generate_batch(texts, 1.0, 1.0, 1.0, names, aux=True)
    for u, text in enumerate(texts):
        s = solo(tts, text, SPEAKERS[u], DC[u], PC[u], EC[u])
        L = LENS[u]
        for k in ("logd", "pitch", "energy", "dur"):
            same = torch.equal(aux[u][k], s[k])
            print("utterance %d %s: %s, max |diff| %.3e" % (u, k, "bit-equal" if same else "DIFFERS", float((aux[u][k] - s[k]).abs().max())))
            assert same, (u, k)
        assert mels[u].shape[1] == s["T"], (u, mels[u].shape, s["T"])
        one = tts.tts.generate(text[None], DC[u], PC[u], EC[u], speaker_name=names[u])
        assert torch.equal(one[0], s["post"]), u                 # `generate` IS that solo run
        assert_mel(aux[u]["mel"], s["mel"], "utterance %d pre-PostNet mel, batched vs solo" % u)
        assert_mel(mels[u][0], s["post"], "utterance %d postnet mel, batched vs solo" % u)
        # the control: solo at controls 1.0 against the padded forward and against the new path
        s1 = solo(tts, text, SPEAKERS[u], 1.0, 1.0, 1.0)
        d_pad = float((padded[3][u, L - 1] - s1["logd"][L - 1]).abs())
        d_new = float((aux1[u]["logd"][L - 1] - s1["logd"][L - 1]).abs())
        print("utterance %d last-phoneme |logd - HIP solo|: padded forward %.4f, batched path %.4g" % (u, d_pad, d_new))
        assert d_new <= LOGD_BAR
        if u > 0:
            assert d_pad > LOGD_BAR, "the padded forward agrees with the solo run: the inputs of this control are wrong"
        else:
            assert d_pad <= LOGD_BAR


def _rand_bf16(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).cuda()


def test_kernels_with_a_filled_control_array_equal_the_scalar_forms():
    from tts_king_amd import ops
    g = torch.Generator().manual_seed(21)
    B, L, D, nb = 3, 96, 256, 255
    rows = B * L
    bins = torch.linspace(-2.5, 9.0, nb).cuda()
    table = torch.randn(nb + 1, D, generator=g).cuda()
    x = _rand_bf16(g, rows, D)
    pred = (torch.randn(B, L, generator=g) * 3.0).cuda()
    full = torch.full((B,), L, dtype=torch.int64).cuda()
    for c in (1.0, 1.5, 0.8):
        p = pred.clone()
        p.view(-1)[:nb] = bins / c                      # predictions whose scaled value lands on (or a rounding away from) every bin edge
        p.view(-1)[nb] = float("nan")
        idx, scaled = ops.bucketize(p, bins, c, want_scaled=True)
        want = ops.gather_add(x, table, idx.view(-1))
        got, gs, gi = ops.embed_step(p, torch.full((B,), c).cuda(), bins, table, x, full, L)
        assert torch.equal(gi, idx) and torch.equal(gs.nan_to_num(7.0), scaled.nan_to_num(7.0)) and torch.equal(got, want), c
        assert int(gi.view(-1)[nb]) == nb
        # duration: values on x.5 boundaries of exp(logd) - 1
        logd = (torch.randn(B, L, generator=g) * 0.7 + 1.3).cuda()
        logd.view(-1)[:20] = torch.log(torch.arange(20).float() + 1.5).cuda()
        assert torch.equal(ops.duration_round_dev(logd, torch.full((B,), c).cuda()), ops.duration_round(logd, c)), c
    # per-utterance controls select per utterance
    ctl = torch.tensor([1.5, 1.0, 0.8]).cuda()
    got, gs, gi = ops.embed_step(pred, ctl, bins, table, x, full, L)
    dur = ops.duration_round_dev(pred * 0.3, ctl)
    for u, c in enumerate(ctl.tolist()):
        idx, scaled = ops.bucketize(pred[u], bins, c, want_scaled=True)
        assert torch.equal(gi[u], idx) and torch.equal(gs[u], scaled)
        assert torch.equal(got.view(B, L, D)[u], ops.gather_add(x.view(B, L, D)[u].contiguous(), table, idx.view(-1)))
        assert torch.equal(dur[u], ops.duration_round((pred * 0.3)[u].contiguous(), c))
    # the limits: rows past lens[u] are zero rows, the others untouched; lens > seg_len, lens <= 0 and B = 1 are clamped
    spk_table = torch.randn(7, D, generator=g).cuda()
    spk = torch.tensor([3, 0, 6]).cuda()
    for lens in ([17, L, 1], [L + 9, 0, -4]):
        lt = torch.tensor(lens, dtype=torch.int64).cuda()
        eff = [min(max(v, 0), L) for v in lens]
        live = torch.zeros(B, L, 1, dtype=torch.bool)
        for u, n in enumerate(eff):
            live[u, :n] = True
        live = live.cuda()
        z = torch.zeros((), dtype=torch.bfloat16).cuda()
        want = torch.where(live, ops.gather_add(x, spk_table, spk, idx_div=L).view(B, L, D), z)
        assert torch.equal(ops.gather_add_lens(x, spk_table, spk, lt, L).view(B, L, D), want), lens
        idx = ops.bucketize(pred, bins, 1.0)
        want = torch.where(live, ops.gather_add(x, table, idx.view(-1)).view(B, L, D), z)
        got, _, gi = ops.embed_step(pred, torch.ones(B).cuda(), bins, table, x, lt, L)
        assert torch.equal(got.view(B, L, D), want) and torch.equal(gi, idx), lens
        for dt in (torch.bfloat16, torch.float32):
            y = torch.randn(rows, 80, generator=g).to(dt).cuda()
            want = torch.where(live, y.view(B, L, 80), torch.zeros((), dtype=dt).cuda())
            assert torch.equal(ops.zero_frames_lens(y.clone(), lt, L).view(B, L, 80), want), (lens, dt)
        for C, use_tanh, resid in ((512, True, False), (80, False, True)):
            yc = torch.randn(rows, C, generator=g).cuda()
            mean, rstd = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
            gamma, beta = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
            r = torch.randn(rows, C, generator=g).cuda() if resid else None
            ref = ops.bn_apply(yc, mean, rstd, gamma, beta, use_tanh, resid=r, out_f32=resid)
            got = ops.bn_apply_lens(yc, mean, rstd, gamma, beta, use_tanh, lt, L, resid=r, out_f32=resid)
            want = torch.where(live, ref.view(B, L, C), torch.zeros((), dtype=ref.dtype).cuda())
            assert torch.equal(got.view(B, L, C), want), (lens, C)
    one = torch.tensor([5], dtype=torch.int64).cuda()          # B = 1
    got = ops.gather_add_lens(x[:L].contiguous(), spk_table, spk[:1].contiguous(), one, L)
    assert torch.equal(got[:5], ops.gather_add(x[:5].contiguous(), spk_table, spk[:1].contiguous(), idx_div=L)) and not bool(got[5:].any())


def test_filled_control_arrays_through_the_facade(tmp_path):
    tts = make_tts(tmp_path, False)
    texts = four_texts()
    a = tts.generate_mel(texts, 0.9, 1.5, 1.2, speaker=9)
    b = tts.generate_mel(texts, [0.9] * 4, [1.5] * 4, [1.2] * 4, speaker=[9, 9, 9, tts.speakers[9]])
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        tts.generate_mel(texts, [0.9] * 3)
    with pytest.raises(ValueError):
        tts.generate_mel(texts, speaker=[1, 2])


def test_bounded_graphs(tmp_path):
    """Calls with different texts, lengths and control values whose buckets coincide share ONE front and ONE back graph."""
    from tts_king_amd import batching
    eager = make_tts(tmp_path, False)
    graphed = make_tts(tmp_path, True)
    g = torch.Generator().manual_seed(31)
    # candidate calls: three texts each, lengths within one phoneme bucket (41..48); the frame bucket is data, so group by it
    groups = {}
    for c in range(24):
        lens = [int(torch.randint(41, 49, (1,), generator=g)), int(torch.randint(20, 49, (1,), generator=g)), int(torch.randint(5, 30, (1,), generator=g))]
        texts = [torch.randint(1, 207, (L,), generator=g).numpy() for L in lens]
        ctl = ([0.9, 1.0, 1.1][c % 3], [1.5, 1.0, 0.8][c % 3], [1.2, 1.0, 0.9][c % 3])
        mels = eager.tts.generate_batch(texts, *ctl, speaker_names=eager.speakers[c])
        key = batching.back_key(3, 48, batching.bucket(max(x.shape[1] for x in mels), 32, 1000))
        groups.setdefault(key, []).append((texts, ctl, eager.speakers[c], mels))
    key, calls = max(groups.items(), key=lambda kv: (len({c[1] for c in kv[1]}), len(kv[1])))
    picked = []                                    # calls with control settings not seen before come first
    for c in calls:
        if c[1] not in [k[1] for k in picked]:
            picked.append(c)
    calls = (picked + [c for c in calls if all(c is not k for k in picked)])[:3]
    print("bounded graphs: key %s, lengths %s, controls %s" % (key, [[len(t) for t in c[0]] for c in calls], [c[1] for c in calls]))
    assert len(calls) == 3 and len({c[1] for c in calls}) == 3, "no frame bucket holds all three control settings: widen the candidate set"
    assert len({tuple(len(t) for t in c[0]) for c in calls}) == 3
    held = []
    for texts, ctl, name, want in calls[:3]:       # 1st: eager warm-up, 2nd: capture + replay, 3rd: replay
        got = graphed.tts.generate_batch(texts, *ctl, speaker_names=name)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        held.append((got, [x.clone() for x in got]))
    s = graphed.tts._synth
    assert list(s._front) == [("front", 3, 48)] and list(s._back) == [key], (list(s._front), list(s._back))
    texts, ctl, name, want = calls[1]
    again = graphed.tts.generate_batch(texts, *ctl, speaker_names=name)
    assert len(s._front) == 1 and len(s._back) == 1
    for a, b in zip(again, want):
        assert torch.equal(a, b)
    for got, snap in held:                          # returned mels survive later calls: copies, not views of graph-owned buffers
        for a, b in zip(got, snap):
            assert torch.equal(a, b)
    assert again[0].data_ptr() != held[1][0][0].data_ptr()


def test_edges(tmp_path):
    tts = make_tts(tmp_path, False)
    g = torch.Generator().manual_seed(41)
    t48, t49, t1, t30 = [torch.randint(1, 207, (L,), generator=g).numpy() for L in (48, 49, 1, 30)]
    name = tts.speakers[7]
    gen = lambda t: tts.tts.generate(t[None], 1.0, 1.2, 0.9, speaker_name=name)
    # B = 1 list
    one = tts.tts.generate_batch([t30], 1.0, 1.2, 0.9, name)
    assert len(one) == 1
    assert_mel(one[0], gen(t30), "B = 1 list vs generate")
    # the same text twice, an L = 1 utterance, L on a bucket edge and one past it
    mels = tts.tts.generate_batch([t30, t1, t48, t30, t49], 1.0, 1.2, 0.9, name)
    assert torch.equal(mels[0], mels[3])
    for i, t in enumerate((t30, t1, t48, t30, t49)):
        assert_mel(mels[i], gen(t), "L = %d in a batch padded to 56 vs generate" % len(t))
    mels = tts.tts.generate_batch([t48, t30], 1.0, 1.2, 0.9, name)
    assert_mel(mels[0], gen(t48), "L = 48 in a batch padded to 48 vs generate")
    # an utterance with no frame at all (duration control 0) comes back empty and leaves its neighbour as it is alone
    mels = tts.tts.generate_batch([t30, t48], [0.0, 1.0], 1.2, 0.9, name)
    assert mels[0].shape == (1, 0, 80)
    assert_mel(mels[1], gen(t48), "L = 48 beside an utterance of zero frames")
    # a text longer than max_seq_len leaves the batch for the solo route
    n_max = tts.tts.model.max_seq_len
    long_text = torch.randint(1, 207, (n_max + 1,), generator=g).numpy()
    mels = tts.tts.generate_batch([t30, long_text, t1], 1.0, 1.2, 0.9, name)
    assert torch.equal(mels[1], gen(long_text))
    assert_mel(mels[0], gen(t30), "L = 30 beside a text over max_seq_len")
    assert_mel(mels[2], gen(t1), "L = 1 beside a text over max_seq_len")


def test_solo_and_batched_routes_share_a_graphed_object(tmp_path):
    """`generate(text)` keys its back graph by the exact (B, L, T), `generate_batch` by (B, L_bucket, T_bucket): a text whose L is a
    multiple of 8 and whose T is a multiple of 32 gives both routes the same numbers.  The graphs differ (per-utterance limits, three
    results against four), so the keys must not meet: both routes, interleaved on one hip_graph object, keep giving the eager mel."""
    eager = make_tts(tmp_path, False)
    graphed = make_tts(tmp_path, True)
    name = eager.speakers[3]
    g = torch.Generator().manual_seed(51)
    text = want = None
    for _ in range(400):
        t = torch.randint(1, 207, (48,), generator=g).numpy()
        mel = eager.tts.generate(t[None], speaker_name=name)
        if mel.shape[1] % 32 == 0:
            text, want = t, mel
            break
    assert text is not None, "no 48-phoneme text with a frame count on a 32-bucket edge among 400: widen the search"
    print("shared object: L 48, T %d" % want.shape[1])
    for route in "sssbbbsbsb":                     # each route: eager warm-up, capture, replay; then interleaved replays
        if route == "s":
            got = graphed.tts.generate(text[None], speaker_name=name)
        else:
            got = graphed.tts.generate_batch([text], speaker_names=name)[0]
        assert torch.equal(got, want), route
    s = graphed.tts._synth
    assert len(s._back) == 2 and len(s._front) == 2, (list(s._front), list(s._back))


def test_use_cwt_is_refused(tmp_path):
    from tts_king_amd.lib import TtskError
    tts = make_tts(tmp_path, False, use_cwt=True)
    g = torch.Generator().manual_seed(43)
    texts = [torch.randint(1, 207, (L,), generator=g).numpy() for L in (12, 9)]
    with pytest.raises(TtskError, match="batch"):
        tts.generate_mel(texts)


@pytest.mark.parametrize("hip_graph", [False, True])
def test_speak_a_list(tmp_path, hip_graph):
    tts = make_tts(tmp_path, hip_graph)
    texts = four_texts()
    spk = list(SPEAKERS)
    for _ in range(3 if hip_graph else 1):       # graphs: eager warm-up, capture, replay
        wavs = tts.speak(texts, list(DC), list(PC), list(EC), spk)
        mels = tts.generate_mel(texts, list(DC), list(PC), list(EC), spk)
    assert len(wavs) == 4
    ragged = tts.vocoder.call_ragged(mels, frames_first=True)
    for u, text in enumerate(texts):
        T = solo(tts, text, SPEAKERS[u], DC[u], PC[u], EC[u])["T"]
        assert mels[u].shape == (1, T, 80)
        assert wavs[u].shape == (1, 1, 256 * T) and wavs[u].dtype == torch.float32, (u, wavs[u].shape)
        assert torch.equal(wavs[u], ragged[u]), u          # the hand-over: the vocoder's ragged route on the batched path's own mel
        alone = tts.vocoder(mels[u].transpose(1, 2))
        r = rel_rms(wavs[u].cpu(), alone.cpu())
        print("utterance %d (T %d, %s route): waveform vs the vocoder on that mel alone: rel-RMS %.2e" % (u, T, "solo" if T < 96 else "windowed", r))
        assert r <= VOCODER_SOLO_BAR, (u, r)
    assert mels[2].shape[1] < 96, "utterance 2 is meant to be shorter than one vocoder window"
