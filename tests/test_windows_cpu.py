"""CPU: windowed vocoding (tts_king_amd/windows.py) — the halo against the generators' measured reach, the plan's properties, and
stitched-against-whole on the CPU oracle.

The V1 generator is oracle/hifigan.py.  The oracle has no ResBlock2, so the V3 generator (hifi/models.py:104-143, :185-201) is
restated here in plain torch (`generator_any`, which also runs V1) and pinned to the reference's own output,
tests/golden/hifi_v3_b2_t32.npz, before it is used.

Bars: a sample at >= H frames from a perturbed mel frame does not change AT ALL (fp64: a far tap cannot vanish in rounding) and
H <= ceil(measured reach) + 1; stitched vs whole <= 1e-6 max-abs in fp32 (measured 1.5e-7: a different conv algorithm per shape,
nothing else); the same stitch with the kept range 6 frames from the cuts must exceed 1e-4 (the test can see a wrong halo)."""
import copy
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hifigan as ohifi
from tests.oracle_util import GOLDEN, hifi_state_dict_wn
from tests.test_hifigan_v3_cpu import V3
from tts_king_amd import windows
from tts_king_amd.synthetic import make_mel, seeded_fill

SPF = 256


def generator_any(sd, h, mel, q=None, mutation=None):
    """hifi/models.py:185-201 with ResBlock1 (:88-95) or ResBlock2 (:134-140), folded weights, any dtype.

    `q`: a rounding applied to every tensor the HIP path stores between layers (conv outputs, residual sums, activated copies, the
    MRF average): the calibration of a storage type's error (tests/test_hifigan_generic_gpu.py).  `mutation`: one deliberate defect
    of the conv-by-conv route, for the negative controls (tests/test_hifigan_v2_cpu.py): "drop_tap" (the last tap of phase 0 of the
    third upsampler is lost), "zero_cols" (output channels 8..15 of the first conv of the first C = 16 block stay zero) or
    "c2_before_residual" (a ResBlock1 pair hands on lrelu(conv) in place of lrelu(conv + x) at the C = 16 and C = 8 stages)."""
    assert mutation in (None, "drop_tap", "zero_cols", "c2_before_residual")
    q = q or (lambda t: t)
    lr = lambda t: q(F.leaky_relu(t, 0.1))
    x = q(F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3))
    nk = len(h["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        wu = sd["ups.%d.weight" % i]
        if mutation == "drop_tap" and i == 2:
            wu = wu.clone()
            wu[:, :, (k - u) // 2 + (k // u - 1) * u] = 0              # phase 0 = taps p, p + u, ...: its last one
        x = q(F.conv_transpose1d(lr(x), wu, sd["ups.%d.bias" % i], stride=u, padding=(k - u) // 2))
        xs = 0
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p, y = "resblocks.%d." % (i * nk + j), x
            yl = lr(y)
            for m, d in enumerate(rd):
                if str(h["resblock"]) == "1":
                    t = F.conv1d(yl, sd[p + "convs1.%d.weight" % m], sd[p + "convs1.%d.bias" % m], dilation=d, padding=(rk * d - d) // 2)
                    if mutation == "zero_cols" and (i, j, m) == (2, 0, 0):
                        t = t.clone()
                        t[:, 8:16] = 0
                    c = F.conv1d(lr(q(t)), sd[p + "convs2.%d.weight" % m], sd[p + "convs2.%d.bias" % m], padding=(rk - 1) // 2)
                else:
                    c = F.conv1d(yl, sd[p + "convs.%d.weight" % m], sd[p + "convs.%d.bias" % m], dilation=d, padding=(rk * d - d) // 2)
                y = q(c + y)
                yl = lr(c) if mutation == "c2_before_residual" and i >= 2 else lr(y)
            xs = xs + y
        x = q(xs / nk)
    return torch.tanh(F.conv1d(q(F.leaky_relu(x)), sd["conv_post.weight"], sd["conv_post.bias"], padding=3))


def v3_hifi(cfg):
    h = copy.deepcopy(cfg.hifi)
    for k, v in V3.items():
        h[k] = v
    return h


def v3_folded(weight_seed):
    g = np.load(os.path.join(GOLDEN, "hifi_v3_b2_t32.npz"))
    sd = {str(k): torch.zeros(tuple(int(x) for x in str(s).split(";"))) for k, s in zip(g["wn_keys"], g["wn_shapes"])}
    seeded_fill(sd, weight_seed)
    return ohifi.fold_weight_norm(sd)


def test_v3_restatement_matches_the_reference_golden(cfg):
    g = np.load(os.path.join(GOLDEN, "hifi_v3_b2_t32.npz"))
    mel = make_mel(int(g["B"]), int(g["T"]), seed=int(g["seed"]))
    with torch.no_grad():
        wav = generator_any(v3_folded(int(g["weight_seed"])), v3_hifi(cfg), mel)
    d = float((wav - torch.from_numpy(g["wav"])).abs().max())
    print("V3 restatement vs reference golden: max-abs %.3g" % d)
    assert wav.shape == (2, 1, 8192) and d <= 1e-5


def test_restatement_is_the_oracle_for_v1(cfg):
    sd = ohifi.fold_weight_norm(hifi_state_dict_wn(11))
    mel = make_mel(1, 40, seed=2)
    with torch.no_grad():
        assert float((generator_any(sd, cfg.hifi, mel) - ohifi.generator(sd, cfg.hifi, mel)).abs().max()) <= 1e-6


def _reach(gen, sd, h, T=120, frame=60):
    """Frames from the perturbed frame's own samples to the farthest output sample that changed, and the changed-sample mask."""
    sd64 = {k: v.double() for k, v in sd.items()}
    mel = make_mel(1, T, seed=5).double()
    mel2 = mel.clone()
    mel2[:, :, frame] += 1.0
    with torch.no_grad():
        changed = (gen(sd64, h, mel) != gen(sd64, h, mel2)).view(-1).nonzero().view(-1)
    first, last = frame * SPF, frame * SPF + SPF - 1
    dist = torch.maximum(first - changed, changed - last).clamp_min(0)      # samples beyond the frame's own, either side
    return float(dist.max()) / SPF, dist


@pytest.mark.parametrize("which", ["v1", "v3"])
def test_halo_covers_the_measured_reach_and_is_not_padded(cfg, which):
    if which == "v1":
        gen, sd, h = ohifi.generator, ohifi.fold_weight_norm(hifi_state_dict_wn(11)), cfg.hifi
    else:
        gen, sd, h = generator_any, v3_folded(11), v3_hifi(cfg)
    H = windows.receptive_halo(h)
    reach, dist = _reach(gen, sd, h)
    print("%s: halo %d frames, measured reach %.2f frames" % (which, H, reach))
    assert reach > 0
    assert int((dist >= H * SPF).sum()) == 0, "a sample %d frames away changed: halo %d is too small" % (math.ceil(reach), H)
    assert H <= math.ceil(reach) + 1
    assert H in ((13, 14) if which == "v1" else (11, 12))


def _check_plan(lens, Wn, H):
    plan = windows.plan_windows(lens, Wn, H)
    assert plan.N == windows.ladder(plan.n_windows) and plan.N >= plan.n_windows
    assert plan.N in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512)
    assert plan.short == [i for i, t in enumerate(lens) if t < Wn] and plan.planned == [i for i, t in enumerate(lens) if t >= Wn]
    assert plan.table.dtype == np.int32 and plan.table.shape == (plan.N, windows.ROW)
    assert plan.frames == sum(lens[i] for i in plan.planned) <= plan.N * Wn
    rows = plan.table[:plan.n_windows]
    for r in plan.table[plan.n_windows:]:                       # padding windows: nothing kept, nothing read
        assert r[2] == r[3] and r[5] == -1
    off = 0
    for i in plan.planned:
        T = lens[i]
        mine = rows[rows[:, 0] == i]
        assert len(mine) == max(1, -(-(T - 2 * H) // (Wn - 2 * H)))
        assert plan.offsets[i] == off
        assert mine[0, 1] == 0 and mine[-1, 1] == T - Wn and bool((np.diff(mine[:, 1]) >= 0).all())
        kept = np.zeros(T, dtype=np.int64)
        for u, s, lo, hi, dst, src, _, _ in mine:
            assert 0 <= s and s + Wn <= T                        # the window lies inside the utterance
            assert s <= lo <= hi <= s + Wn
            kept[lo:hi] += 1
            assert lo == 0 or lo - s >= H                        # a cut that is not the utterance's own edge is at least H away
            assert hi == T or (s + Wn) - hi >= H
            assert (lo == 0) == (s == 0) and (hi == T) == (s + Wn == T)
            assert dst == off + lo and src == off + s
        assert bool((kept == 1).all())                           # every frame by exactly one window
        off += T
    return plan


def test_plan_properties_every_length():
    Wn = windows.W
    for H in (14, 12):
        for T in range(Wn, 4 * Wn + 4):
            _check_plan([T], Wn, H)
    for Wn in (64, 96, 192, 256):
        for T in range(Wn, 4 * Wn + 4):
            _check_plan([T], Wn, 14)


def test_plan_properties_ragged_batches():
    rnd = random.Random(1234)
    for _ in range(50):
        lens = [rnd.randint(1, 1200) for _ in range(rnd.randint(1, 40))]
        _check_plan(lens, windows.W, 14)
    assert windows.plan_windows([5, 7], windows.W, 14).N == 0
    assert [windows.ladder(n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 17, 25, 33)] == [1, 2, 3, 4, 6, 6, 8, 8, 12, 16, 24, 32, 48]
    with pytest.raises(ValueError):
        windows.window_starts(100, 28, 14)


def _stitched(sd, h, mel, Wn, H):
    """Windows through the oracle as one batch, stitched by the plan."""
    T = mel.shape[2]
    plan = windows.plan_windows([T], Wn, H)
    rows = plan.table[:plan.n_windows]
    batch = torch.cat([mel[:, :, s:s + Wn] for s in rows[:, 1]], dim=0)
    with torch.no_grad():
        y = ohifi.generator(sd, h, batch)
    return torch.cat([y[r:r + 1, :, (lo - s) * SPF:(hi - s) * SPF] for r, (u, s, lo, hi) in enumerate(rows[:, :4].tolist())], dim=2)


def test_stitched_equals_whole_on_the_oracle(cfg):
    sd = ohifi.fold_weight_norm(hifi_state_dict_wn(11))
    Wn, H = windows.W, windows.receptive_halo(cfg.hifi)
    for T in (Wn, Wn + 1, 2 * Wn - 2 * H, 2 * Wn - 2 * H + 1, 333):
        mel = make_mel(1, T, seed=T)
        with torch.no_grad():
            whole = ohifi.generator(sd, cfg.hifi, mel)
        got = _stitched(sd, cfg.hifi, mel, Wn, H)
        d = float((got - whole).abs().max())
        print("T=%d: stitched vs whole max-abs %.3g (signal RMS %.3g)" % (T, d, float(whole.pow(2).mean().sqrt())))
        assert got.shape == whole.shape and d <= 1e-6


def test_a_short_halo_is_seen(cfg):
    """Negative control at the issue's case (W = 64, T = 200, seed 11): kept ranges only 6 frames from the cuts differ from the whole by > 1e-4."""
    sd = ohifi.fold_weight_norm(hifi_state_dict_wn(11))
    mel = make_mel(1, 200, seed=200)
    with torch.no_grad():
        whole = ohifi.generator(sd, cfg.hifi, mel)
    d = float((_stitched(sd, cfg.hifi, mel, 64, 6) - whole).abs().max())
    ok = float((_stitched(sd, cfg.hifi, mel, 64, windows.receptive_halo(cfg.hifi)) - whole).abs().max())
    print("W=64 T=200: halo 6 max-abs %.3g, halo %d max-abs %.3g" % (d, windows.receptive_halo(cfg.hifi), ok))
    assert d > 1e-4 and ok <= 1e-6
