"""GPU: per-phoneme prosody -- per-phoneme controls, explicit pitch / energy / durations and a frame budget.

Kernels (`ttsk_embed_step_rows`, `ttsk_duration_rows`, `ttsk_duration_fit`) against the scalar forms they generalise and against the
properties the fit rule defines; then the route through `FSTWOapi.generate_batch` / `TTSKing.generate_mel` / `speak` against the
reference's solo run through the oracle with (1, L) control tensors, with the bars tests/test_batch_synth_gpu.py and
tests/test_facade_gpu.py hold (log-durations within 0.06, the rounding rule, bin edges, mel rel-RMS <= 1.5 % teacher-forced).
"""
import os

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests.oracle_util import rel_rms
from tests.test_batch_synth_gpu import LENS, LOGD_BAR, SPEAKERS, boundary_between, four_texts
from tests.test_prosody_cpu import fit_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ kernels
def _kernel_inputs(seg_len, seed):
    g = torch.Generator().manual_seed(seed)
    B, D, nb = 3, 256, 255
    rows = B * seg_len
    bins = torch.linspace(-2.5, 9.0, nb).cuda()
    table = torch.randn(nb + 1, D, generator=g).cuda()            # a 256-row table
    x = torch.randn(rows, D, generator=g).to(torch.bfloat16).cuda()
    pred = (torch.randn(B, seg_len, generator=g) * 3.0)
    logd = (torch.randn(B, seg_len, generator=g) * 0.7 + 1.3)
    logd.view(-1)[:6] = torch.log(torch.arange(6).float() + 1.5)   # on the x.5 boundaries of exp(logd) - 1
    return g, B, D, nb, bins, table, x, pred.cuda(), logd.cuda()


def _lens_cases(seg_len):
    return [(seg_len, 5, 1), (0, seg_len + 3, 2)]       # the second: the clamps


@pytest.mark.parametrize("seg_len", [8, 40])
def test_constant_rows_without_values_equal_the_scalar_kernels(seg_len):
    from tts_king_amd import ops
    g, B, D, nb, bins, table, x, pred, logd = _kernel_inputs(seg_len, 61)
    zeros, none = torch.zeros(B, seg_len).cuda(), torch.zeros(B, seg_len, dtype=torch.uint8).cuda()
    for lens in _lens_cases(seg_len):
        lt = torch.tensor(lens, dtype=torch.int64).cuda()
        for c in (0.5, 1.0, 1.7):
            p = pred.clone()
            k = min(nb, p.numel() - 1)
            p.view(-1)[:k] = bins[:k] / c                   # scaled values on (or a rounding away from) bin edges
            p.view(-1)[k] = NAN
            want, ws, wi = ops.embed_step(p, torch.full((B,), c).cuda(), bins, table, x, lt, seg_len)
            got, gs, gi = ops.embed_step_rows(p, torch.full((B, seg_len), c).cuda(), zeros, none, bins, table, x, lt, seg_len)
            assert torch.equal(got, want) and torch.equal(gi, wi) and torch.equal(gs.nan_to_num(7.0), ws.nan_to_num(7.0)), (lens, c)
            assert int(gi.view(-1)[k]) == nb
            assert torch.equal(ops.duration_rows(logd, torch.full((B, seg_len), c).cuda(), zeros, none),
                               ops.duration_round_dev(logd, torch.full((B,), c).cuda())), c


@pytest.mark.parametrize("seg_len", [8, 40])
def test_varying_rows_and_set_values(seg_len):
    from tts_king_amd import ops
    g, B, D, nb, bins, table, x, pred, logd = _kernel_inputs(seg_len, 62)
    cs = (0.5, 1.0, 1.7)
    pick = torch.randint(0, 3, (B, seg_len), generator=g)
    ctl = torch.tensor(cs)[pick].cuda()
    has = (torch.rand(B, seg_len, generator=g) < 0.3)
    has.view(-1)[:2] = True                                    # rows 0 and 1 carry the edge value and the NaN prediction below
    value = (torch.randn(B, seg_len, generator=g) * 3.0)
    value.view(-1)[0] = float(bins[17])                       # a set value exactly on a bin edge
    durs = torch.round(torch.rand(B, seg_len, generator=g) * 9) + 0.25
    pred = pred.clone()
    pred.view(-1)[1] = NAN                                     # a NaN prediction under a set value is ignored
    has_d, value_d, durs_d = has.to(torch.uint8).cuda(), value.cuda(), durs.cuda()
    z = torch.zeros((), dtype=torch.bfloat16).cuda()
    for lens in _lens_cases(seg_len):
        lt = torch.tensor(lens, dtype=torch.int64).cuda()
        live = torch.zeros(B, seg_len, 1, dtype=torch.bool)
        for u, n in enumerate(lens):
            live[u, :min(max(n, 0), seg_len)] = True
        live = live.cuda()
        got, gs, gi = ops.embed_step_rows(pred, ctl, value_d, has_d, bins, table, x, lt, seg_len)
        dur = ops.duration_rows(logd, ctl, durs_d, has_d)
        free = ~has.cuda()
        for j, c in enumerate(cs):                            # every row equals the scalar kernel run with that row's control
            rows_c = (pick == j).cuda() & free
            want, ws, wi = ops.embed_step(pred, torch.full((B,), c).cuda(), bins, table, x, lt, seg_len)
            assert torch.equal(got.view(B, seg_len, D)[rows_c], want.view(B, seg_len, D)[rows_c]), (lens, c)
            assert torch.equal(gs[rows_c], ws[rows_c]) and torch.equal(gi[rows_c], wi[rows_c]), (lens, c)
            assert torch.equal(dur[rows_c], ops.duration_round_dev(logd, torch.full((B,), c).cuda())[rows_c]), c
        hs = has.cuda()
        assert torch.equal(gs[hs], value_d[hs]) and not bool(torch.isnan(gs[hs]).any())          # reported back bit for bit
        widx = ops.bucketize(value_d, bins)
        assert torch.equal(gi[hs], widx[hs]) and int(gi.view(-1)[0]) == 17
        wx = torch.where(live, ops.gather_add(x, table, widx.view(-1)).view(B, seg_len, D), z)
        assert torch.equal(got.view(B, seg_len, D)[hs], wx[hs]), lens
        assert torch.equal(dur[hs], durs_d[hs])
        assert not bool(got.view(B, seg_len, D)[~live[..., 0]].any())                             # zero rows past lens[u]


def _fit_case(kind, n, rng):
    """(v (n,) fp32, has (n,) bool, target) of one utterance of n phonemes."""
    v = (np.round(rng.rand(n) * 6) * 0.9).astype(np.float32)        # fractional (a control of 0.9), some zeros
    v[0] = np.float32(2.7)
    has = rng.rand(n) < 0.2
    v[has] = (np.round(rng.rand(int(has.sum())) * 5) + 0.6).astype(np.float32)
    F = float(np.trunc(v[has].astype(np.float64)).sum())
    free = ~has
    if kind == "none":
        return v, has, -1
    if kind == "zero":
        return v, has, 0
    if kind == "one":
        has[:] = False
        return v, has, 1
    if kind == "below_nonzero":
        has[:] = False
        return v, has, int((v > 0).sum()) // 2
    if kind == "S0":
        v[free] = 0.0
        return v, has, int(F) + 11
    if kind == "all_fixed":
        has[:] = True
        return v, has, int(np.trunc(v.astype(np.float64)).sum()) + 5
    if kind == "below_F":
        has[0], v[0] = True, np.float32(4.6)
        return v, has, int(np.trunc(v[has].astype(np.float64)).sum()) - 2
    if kind == "large":
        return v, has, int(8 * float(v.astype(np.float64).sum()))
    raise KeyError(kind)


FIT_KINDS = ("none", "zero", "one", "below_nonzero", "S0", "all_fixed", "below_F", "large")


def _check_fit(out, v, has, target, n, what):
    """The properties the rule defines, for one utterance's own n phonemes (fp64, from the kernel's own v)."""
    out, v, has = out[:n].astype(np.float64), v[:n].astype(np.float64), has[:n].astype(bool)
    if target < 0:
        assert np.array_equal(out, v), what
        return
    F = np.trunc(v[has]).sum()
    free = ~has & (v > 0)
    S = v[free].sum()
    total = max(float(target), F) if S > 0 else F
    assert out.sum() == total, (what, out.sum(), total)
    assert np.array_equal(out[has], np.trunc(v[has])), what                 # fixed phonemes untouched
    assert not out[~has & (v == 0)].any(), what                             # v = 0 stays 0
    assert (out == np.floor(out)).all() and (out >= 0).all(), what
    if S > 0:
        q = v[free] * max(float(target) - F, 0.0) / S
        assert (np.abs(out[free] - q) < 1 + 1e-3).all(), (what, float(np.abs(out[free] - q).max()))


@pytest.mark.parametrize("seg_len", [1, 7, 256, 257, 1000])
def test_duration_fit_properties(seg_len):
    from tts_king_amd import ops
    rng = np.random.RandomState(1000 + seg_len)
    for group in (FIT_KINDS[:4], FIT_KINDS[4:]):                 # B = 4, mixed cases in one launch
        B = 4
        lens = [seg_len, max(seg_len - 3, 1), seg_len, max(seg_len // 2, 1)]
        v = (rng.rand(B, seg_len) * 5 + 0.5).astype(np.float32)            # what lies past an utterance's end must not count
        has = rng.rand(B, seg_len) < 0.5
        target = np.zeros((B,), np.int32)
        for u, kind in enumerate(group):
            v[u, :lens[u]], has[u, :lens[u]], target[u] = _fit_case(kind, lens[u], rng)
        dv, dh = torch.from_numpy(v).cuda(), torch.from_numpy(has.astype(np.uint8)).cuda()
        out = ops.duration_fit(dv, dh, torch.from_numpy(target).cuda(), torch.tensor(lens, dtype=torch.int64).cuda())
        if "none" in group:
            assert torch.equal(out[0], dv[0])
        o = out.cpu().numpy()
        for u, kind in enumerate(group):
            _check_fit(o[u], v[u], has[u], int(target[u]), lens[u], (seg_len, kind))
            assert np.array_equal(o[u, lens[u]:], v[u, lens[u]:]), (seg_len, kind)          # past the end: as it came


def test_duration_fit_hand_worked_cases_and_placement():
    from tts_king_amd import ops
    no = [False] * 4
    cases = [([1, 1, 1], no[:3], 4), ([2, 2, 2, 2], no, 6), ([3, 1], no[:2], 6), ([0, 2, 0, 1], no, 2), ([2, 3, 4], no[:3], 1),
             ([0, 0, 3], [False, False, True], 10), ([5, 2], [True, False], 3), ([5.9, 2], [True, False], 9), ([2.7, 1.2], [True, True], 9),
             ([2.7, 0.3], no[:2], -1), ([2, 3], no[:2], 0)]
    B, L = len(cases), 8
    v, has, target, lens = np.zeros((B, L), np.float32), np.zeros((B, L), np.uint8), np.zeros((B,), np.int32), np.zeros((B,), np.int64)
    for u, (a, h, t) in enumerate(cases):
        v[u, :len(a)], has[u, :len(a)], target[u], lens[u] = a, h, t, len(a)
    cu = lambda a: torch.from_numpy(a).cuda()
    out = ops.duration_fit(cu(v), cu(has), cu(target), cu(lens)).cpu().numpy()
    for u, (a, h, t) in enumerate(cases):          # small integers: every sum is exact, so the kernel must give the numpy rule's frames
        assert out[u, :len(a)].tolist() == fit_rule(a, h, t).tolist(), (a, h, t, out[u])
    # the same utterance in another row, alone, and padded to another bucket: bit-equal
    rng = np.random.RandomState(9)
    n = 23
    a, h, t = _fit_case("large", n, rng)
    t = t // 3 + 1

    def run(B, L, row):
        v = (rng.rand(B, L) * 5).astype(np.float32)
        has = (rng.rand(B, L) < 0.5).astype(np.uint8)
        lens = rng.randint(1, L + 1, size=B).astype(np.int64)
        target = rng.randint(0, 200, size=B).astype(np.int32)
        v[row, :n], has[row, :n], lens[row], target[row] = a, h, n, t
        v[row, n:], has[row, n:] = 0.0, 0                   # padded positions contribute zeros
        return ops.duration_fit(cu(v), cu(has), cu(target), cu(lens))[row, :n]

    first = run(4, 40, 0)
    _check_fit(first.cpu().numpy(), a, h, t, n, "placement")
    for B, L, row in ((4, 40, 3), (1, 40, 0), (4, 24, 2), (1, 24, 0), (2, 1000, 1)):
        assert torch.equal(run(B, L, row), first), (B, L, row)


# ------------------------------------------------------------------------------------------------ model and facades
def make_tts(tmp_path, hip_graph, use_cwt=False, max_seq_len=None):
    import yaml
    import tts_king
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config.yaml")))
    cfg["preprocess_config"]["path"]["preprocessed_path"] = os.path.join(ROOT, "pretrained")
    cfg["mi355x"]["hip_graph"] = hip_graph
    if use_cwt:
        cfg["model_config"]["use_cwt"] = True
    if max_seq_len:
        cfg["model_config"]["max_seq_len"] = max_seq_len
    p = tmp_path / ("config_%d_%d_%s.yaml" % (hip_graph, use_cwt, max_seq_len))
    p.write_text(yaml.safe_dump(cfg))
    t = tts_king.TTSKing(str(p))
    with torch.no_grad():       # random-init duration head predicts ~0 frames: shift it so utterances have a few frames per phoneme
        t.tts.model.get("variance_adaptor.duration_predictor.linear_layer.bias").fill_(1.3)
    return t


@pytest.fixture(scope="module")
def eager(tmp_path_factory):
    return make_tts(tmp_path_factory.mktemp("prosody"), False)


def names_of(tts):
    return [tts.speakers[s] for s in SPEAKERS]


def rand_controls(seed):
    rng = np.random.RandomState(seed)
    return [[(rng.rand(L) * 1.0 + 0.5).astype(np.float32) for L in LENS] for _ in range(3)]       # dc, pc, ec per utterance


def edge_between(name, h, r_, bins, where):
    """Rows (among `where`) in which the HIP path and the oracle pick different bins lie across a bin edge (tests/test_facade_gpu.py)."""
    bh, br = torch.bucketize(h, bins), torch.bucketize(r_, bins)
    n = 0
    for bi, li in ((bh != br) & where).nonzero().tolist():
        lo, hi = min(float(h[bi, li]), float(r_[bi, li])), max(float(h[bi, li]), float(r_[bi, li]))
        assert bool(((bins >= lo - 1e-6) & (bins <= hi + 1e-6)).any()), (name, bi, li, lo, hi)
        assert hi - lo <= 0.1 * max(1.0, abs(hi)), (name, bi, li, lo, hi)
        n += 1
    return n


def against_the_oracle(tts, texts, mels, aux, dcs, pcs, ecs, set_p=None, set_e=None, set_d=None):
    """Each utterance against the reference's solo run with (1, L) control tensors.  set_*: per utterance a bool mask of the explicitly
    set positions (their values are the HIP aux's own, checked by the caller)."""
    m = tts.tts.model
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    mc = tts.cfg.model_config
    va = "variance_adaptor."
    for u, text in enumerate(texts):
        L = len(text)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))[None]
        dc, pc, ec = t(dcs[u]), t(pcs[u]), t(ecs[u])
        free = lambda s: torch.ones(1, L, dtype=torch.bool) if s is None else ~torch.from_numpy(np.asarray(s[u], bool))[None]
        spk, ids, sl = torch.tensor([SPEAKERS[u]]), torch.from_numpy(text[None]).long(), torch.tensor([L])
        with torch.no_grad():
            ref = ofs2.fs2_forward(sd, mc, spk, ids, sl, L, p_control=pc, e_control=ec, d_control=dc)
        logd_h, logd_r = aux[u]["logd"].float().cpu()[None], ref[3].float()
        diff = float((logd_h - logd_r).abs().max())
        assert diff <= LOGD_BAR, (u, diff)
        d_h, d_r = aux[u]["dur"].float().cpu()[None], ref[4].float()
        v_h, v_r = torch.exp(logd_h) - 1.0, torch.exp(logd_r) - 1.0
        rule = torch.clamp(torch.round(v_h) * dc, min=0.0)
        fd = free(set_d)
        assert bool((((v_h - torch.floor(v_h) - 0.5).abs() < 1e-5) | (rule == d_h) | ~fd).all()), u
        nd = 0
        for bi, li in ((d_h != d_r) & fd).nonzero().tolist():
            assert boundary_between(float(v_r[bi, li]), float(v_h[bi, li])), (u, li, float(v_h[bi, li]), float(v_r[bi, li]))
            nd += 1
        T = mels[u].shape[1]
        assert mels[u].shape == (1, T, 80) and int(d_h.clamp(min=0).trunc().sum()) == T, (u, T)
        pitch_h, energy_h = aux[u]["pitch"].float().cpu()[None], aux[u]["energy"].float().cpu()[None]
        n_p = edge_between("pitch", pitch_h, ref[1].float(), sd[va + "pitch_bins"], free(set_p))
        with torch.no_grad():      # the oracle on the HIP pitch (set values included): its energy predictor sees the same embedding rows
            ref = ofs2.fs2_forward(sd, mc, spk, ids, sl, L, pitches_raw=pitch_h, e_control=ec, d_control=dc)
        n_e = edge_between("energy", energy_h, ref[2].float(), sd[va + "energy_bins"], free(set_e))
        with torch.no_grad():      # teacher-forced on the HIP durations, pitch and energy
            ref = ofs2.fs2_forward(sd, mc, spk, ids, sl, L, d_targets=d_h, max_mel_len=T, mel_lens=torch.tensor([T]), pitches_raw=pitch_h,
                                   e_targets=energy_h)
        r = rel_rms(mels[u].cpu(), ref[9])
        print("utterance %d (L %d, T %d): max |logd - oracle| %.4f; %d durations / %d pitch / %d energy rows differ (each across a boundary); "
              "mel rel-RMS %.3f%%" % (u, L, T, diff, nd, n_p, n_e, 100 * r))
        assert r <= 0.015, (u, r)


def test_neutral_inputs_equal_the_existing_route(eager):
    texts = four_texts()
    ones = [np.ones(L, np.float32) for L in LENS]
    want, waux = eager.tts.generate_batch(texts, 1.0, 1.0, 1.0, names_of(eager), aux=True)
    got, gaux = eager.tts.generate_batch(texts, ones, ones, ones, names_of(eager), aux=True)
    for u in range(4):
        assert torch.equal(got[u], want[u]), u
        for k in ("logd", "pitch", "energy", "dur", "mel"):
            assert torch.equal(gaux[u][k], waux[u][k]), (u, k)
    # constant rows of another value, against per-utterance scalars
    cd, cp, ce = (0.9, 1.0, 1.1, 1.0), (1.5, 1.0, 0.8, 1.2), (1.2, 1.0, 1.0, 0.9)
    want = eager.tts.generate_batch(texts, list(cd), list(cp), list(ce), names_of(eager))
    rows = lambda cs: [np.full(L, c, np.float32) for L, c in zip(LENS, cs)]
    got = eager.tts.generate_batch(texts, rows(cd), rows(cp), rows(ce), names_of(eager))
    for u in range(4):
        assert torch.equal(got[u], want[u]), u


def test_per_phoneme_controls_against_the_reference(eager):
    texts = four_texts()
    dcs, pcs, ecs = rand_controls(71)
    mels, aux = eager.tts.generate_batch(texts, dcs, pcs, ecs, names_of(eager), aux=True)
    against_the_oracle(eager, texts, mels, aux, dcs, pcs, ecs)
    plain = eager.tts.generate_batch(texts, 1.0, 1.0, 1.0, names_of(eager))
    assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(mels, plain))


def test_explicit_values(eager):
    texts = four_texts()
    dcs, pcs, ecs = rand_controls(72)
    rng = np.random.RandomState(73)
    pitch, energy, durs = [], [], []
    for L in LENS:
        p = np.where(rng.rand(L) < 0.4, rng.randn(L) * 1.5, NAN).astype(np.float32)
        e = np.where(rng.rand(L) < 0.4, rng.randn(L) * 1.5, NAN).astype(np.float32)
        d = np.where(rng.rand(L) < 0.4, np.round(rng.rand(L) * 9), NAN).astype(np.float32)
        p[0], e[1], d[2] = 0.75, -0.5, 11.0
        pitch.append(p), energy.append(e), durs.append(d)
    energy[1] = None                               # nothing set for one utterance
    durs[3] = 4.0                                  # a scalar: every phoneme of that utterance
    mels, aux = eager.tts.generate_batch(texts, dcs, pcs, ecs, names_of(eager), aux=True, pitch=pitch, energy=energy, durations=durs)
    sets = {"pitch": [], "energy": [], "dur": []}
    for u, L in enumerate(LENS):
        for key, given in (("pitch", pitch[u]), ("energy", energy[u]), ("dur", durs[u])):
            g = np.full(L, NAN, np.float32) if given is None else np.broadcast_to(np.asarray(given, np.float32), (L,))
            s = ~np.isnan(g)
            sets[key].append(s)
            got = aux[u][key].cpu().numpy()
            assert got[s].tobytes() == g[s].tobytes(), (u, key)          # the set positions come back bit for bit
    against_the_oracle(eager, texts, mels, aux, dcs, pcs, ecs, set_p=sets["pitch"], set_e=sets["energy"], set_d=sets["dur"])
    plain = eager.tts.generate_batch(texts, dcs, pcs, ecs, names_of(eager))
    for u in range(4):                              # negative control: the edit is audible in the mel
        assert mels[u].shape != plain[u].shape or not torch.equal(mels[u], plain[u]), u


def test_round_trip(eager):
    texts = four_texts()
    dcs, pcs, ecs = rand_controls(74)
    mels, pros = eager.tts.generate_batch(texts, dcs, pcs, ecs, names_of(eager), return_prosody=True)
    assert all(sorted(p) == ["dur", "energy", "logd", "pitch"] and p["dur"].shape == (L,) for p, L in zip(pros, LENS))
    again = eager.tts.generate_batch(texts, speaker_names=names_of(eager), durations=[p["dur"] for p in pros], pitch=[p["pitch"] for p in pros],
                                     energy=[p["energy"] for p in pros])
    for u in range(4):
        assert torch.equal(again[u], mels[u]), u
    # one text through TTSKing: a 1-D array is per phoneme; edit one phoneme and re-synthesize
    mel, p = eager.generate_mel(texts[2], pitch_control=pcs[2], speaker=SPEAKERS[2], return_prosody=True)
    assert mel.shape[0] == 1 and p["pitch"].shape == (LENS[2],)
    d = p["dur"].cpu().numpy().copy()
    d[5] += 7
    longer = eager.generate_mel(texts[2], speaker=SPEAKERS[2], durations=d, pitch=p["pitch"], energy=p["energy"])
    assert longer.shape[1] == mel.shape[1] + 7


def test_frame_budget(eager):
    texts = four_texts()
    names = names_of(eager)
    natural = [m.shape[1] for m in eager.tts.generate_batch(texts, speaker_names=names)]
    targets = [natural[0] - 17, natural[1] + 23, 2 * natural[2], max(natural[3] // 2, 1)]
    print("frame budget: natural lengths %s, targets %s" % (natural, targets))
    mels, pros = eager.tts.generate_batch(texts, speaker_names=names, target_frames=targets, return_prosody=True)
    for u in range(4):
        assert mels[u].shape == (1, targets[u], 80), (u, mels[u].shape)
        assert float(pros[u]["dur"].sum()) == targets[u]
        alone = eager.tts.generate_batch([texts[u]], speaker_names=names[u], target_frames=[targets[u]])[0]
        assert torch.equal(alone, mels[u]), u                               # batched equals the same request alone
    one = eager.generate_mel(texts[1], speaker=SPEAKERS[1], target_frames=targets[1])
    assert torch.equal(one, mels[1])
    # None leaves an utterance free; explicit durations are fixed and the others share what is left
    d = np.full(LENS[0], NAN, np.float32)
    d[3], d[7] = 20.0, 0.0
    mixed, pros = eager.tts.generate_batch(texts[:2], speaker_names=names[:2], target_frames=[targets[0], None], durations=[d, None],
                                          return_prosody=True)
    assert mixed[0].shape[1] == targets[0] and mixed[1].shape[1] == natural[1]
    assert float(pros[0]["dur"][3]) == 20.0 and float(pros[0]["dur"][7]) == 0.0
    wavs = eager.speak(texts, speaker=list(SPEAKERS), target_frames=targets)
    for u in range(4):
        assert wavs[u].shape == (1, 1, 256 * targets[u]), (u, wavs[u].shape)
    wav = eager.speak(texts[1], speaker=SPEAKERS[1], target_frames=targets[1])
    assert wav.shape == (1, 1, 256 * targets[1])


def test_frame_count_past_the_position_table(tmp_path):
    from tts_king_amd import ops
    tts = make_tts(tmp_path, False, max_seq_len=64)
    g = torch.Generator().manual_seed(81)
    t20, t12 = [torch.randint(1, 207, (L,), generator=g).numpy() for L in (20, 12)]
    pc = np.linspace(0.6, 1.4, 20).astype(np.float32)
    mels, pros = tts.generate_mel([t12, t20], pitch_control=[1.0, pc], speaker=[3, 4], target_frames=[None, 100], return_prosody=True)
    assert mels[1].shape == (1, 100, 80) and bool(torch.isfinite(mels[1]).all())
    p = pros[1]
    assert p is not None and float(p["dur"].sum()) == 100.0
    # its durations are the fit's: the kernels on the reported log-durations
    z, n = torch.zeros(1, 20).cuda(), torch.zeros(1, 20, dtype=torch.uint8).cuda()
    v = ops.duration_rows(p["logd"][None].contiguous(), torch.ones(1, 20).cuda(), z, n)
    fit = ops.duration_fit(v, n, torch.tensor([100], dtype=torch.int32).cuda(), torch.tensor([20]).cuda())
    assert torch.equal(fit[0], p["dur"])
    assert torch.equal(p["pitch"], tts.generate_mel(t20, pitch_control=pc, speaker=4, return_prosody=True)[1]["pitch"])
    alone = tts.generate_mel(t12[None], speaker=3)          # the untouched single-text form takes (1, L)
    assert mels[0].shape == alone.shape
    # a text of more than max_seq_len phonemes that carries per-phoneme inputs is refused, naming the limit
    t65 = torch.randint(1, 207, (65,), generator=g).numpy()
    with pytest.raises(ValueError, match="max_seq_len = 64"):
        tts.generate_mel([t12, t65], speaker=[3, 4], target_frames=[None, 100])
    with pytest.raises(ValueError, match="max_seq_len = 64"):
        tts.generate_mel(t65, pitch_control=np.linspace(0.5, 1.5, 65))
    both = tts.generate_mel([t12, t65], speaker=[3, 4], target_frames=[30, None])       # a plain long text still takes the solo route
    assert both[0].shape[1] == 30 and torch.equal(both[1], tts.generate_mel(t65[None], speaker=4))


def test_bounded_graphs(tmp_path, eager):
    graphed = make_tts(tmp_path, True)
    g = torch.Generator().manual_seed(91)
    rng = np.random.RandomState(92)
    calls = []
    for c in range(20):
        lens = [int(torch.randint(41, 49, (1,), generator=g)), int(torch.randint(20, 49, (1,), generator=g)), int(torch.randint(5, 30, (1,), generator=g))]
        texts = [torch.randint(1, 207, (L,), generator=g).numpy() for L in lens]
        kw = {}
        if c % 2 == 0:
            kw["pitch_control"] = [(rng.rand(L) + 0.5).astype(np.float32) for L in lens]
        if c % 3 == 0:
            kw["duration_control"] = [1.0, (rng.rand(lens[1]) + 0.5).astype(np.float32), 0.9]
        if c % 4 == 1:
            kw["energy"] = [None, np.where(rng.rand(lens[1]) < 0.5, rng.randn(lens[1]), NAN).astype(np.float32), 0.3]
        if c % 5 == 2:
            kw["durations"] = [np.where(rng.rand(lens[0]) < 0.3, 6.0, NAN).astype(np.float32), None, None]
        if c % 3 != 1:
            kw["target_frames"] = list([(150, 100, 60), (160, None, 33), (129, 97, 64)][(c // 3) % 3])
        if not kw:
            kw["pitch"] = [None, 1.25, None]
        calls.append((texts, kw))
    s = graphed.tts._synth
    for texts, kw in calls:
        want = eager.tts.generate_batch(texts, speaker_names=eager.speakers[4], **kw)
        got = graphed.tts.generate_batch(texts, speaker_names=graphed.speakers[4], **kw)
        for a, b in zip(got, want):
            assert torch.equal(a, b)                     # replayed results equal the hip_graph: false run
    assert list(s._front) == [("front", 3, 48, "rows")], list(s._front)          # ONE front graph for the new route
    assert all(k[:3] == ("back", 3, 48) and len(k) == 4 for k in s._back), list(s._back)
    # the existing route: its graphs and keys as before, beside the new one
    texts = calls[0][0]
    for _ in range(3):
        got = graphed.tts.generate_batch(texts, 0.9, 1.5, 1.2, speaker_names=graphed.speakers[4])
    want = eager.tts.generate_batch(texts, 0.9, 1.5, 1.2, speaker_names=eager.speakers[4])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert sorted(s._front, key=len) == [("front", 3, 48), ("front", 3, 48, "rows")], list(s._front)


def test_refusals(tmp_path, eager):
    from tts_king_amd.lib import TtskError
    texts = four_texts()
    with pytest.raises(ValueError, match=r"p_control\[1\]"):
        eager.generate_mel(texts, pitch_control=[1.0, np.ones(LENS[1] + 1), 1.0, 1.0])
    with pytest.raises(ValueError, match=r"durations\[0\].*>= 0"):
        eager.generate_mel(texts[0], durations=np.where(np.arange(LENS[0]) == 4, -1.0, NAN))
    with pytest.raises(ValueError, match=r"durations\[2\].*finite"):
        eager.generate_mel(texts, durations=[None, None, float("inf"), None])
    with pytest.raises(ValueError, match=r"pitch\[0\]"):
        eager.generate_mel(texts[0], pitch=np.ones(LENS[0] - 1))
    with pytest.raises(ValueError, match=r"target_frames\[3\]"):
        eager.generate_mel(texts, target_frames=[None, None, None, -5])
    cwt = make_tts(tmp_path, False, use_cwt=True)
    with pytest.raises(TtskError, match="batch"):
        cwt.generate_mel(texts[:2], target_frames=[50, 60])
    with pytest.raises(TtskError, match="batch"):
        cwt.generate_mel(texts[2], pitch_control=np.ones(LENS[2]))
