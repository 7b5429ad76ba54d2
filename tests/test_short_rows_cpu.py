"""CPU: utterances shorter than a window as rows of the windowed batch — the opt-in plan's properties, and the
contract of the per-row-length kernels stated on the CPU generators (tests/short_rows_util.py).

Bars.  Masked batch vs solo run: the two differ by the rounding of another conv shape only, the level DESIGN.md 11 records for the
stitched windows (1.6e-7 max-abs in fp32).  Measured here: V1 1.23e-7, V3 1.49e-7 max-abs over the seven rows (signal RMS 0.012 -
0.039); the bar is twice the larger, 3.0e-7.  The negative control (zero-padded mel, no masks) misses the solo run's last frame by
0.02 - 0.07 at every T < W (printed), which is the size of the signal itself; it is asserted to exceed 1e-3."""
import random

import numpy as np
import pytest
import torch

from oracle import hifigan as ohifi
from tests.oracle_util import hifi_state_dict_wn
from tests.short_rows_util import ROW_LENS, SPF, generator_rows, padded_batch
from tests.test_windows_cpu import generator_any, v3_folded, v3_hifi
from tts_king_amd import windows
from tts_king_amd.synthetic import make_mel

LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512)
MASKED_BAR = 3.0e-7


def _check_short_plan(lens, Wn, H):
    plan = windows.plan_windows(lens, Wn, H, short_rows=True)
    assert plan.planned == [i for i, t in enumerate(lens) if t >= 1] and plan.short == [i for i, t in enumerate(lens) if t < 1]
    assert plan.N == windows.ladder(plan.n_windows) and plan.N in LADDER
    assert plan.table.dtype == np.int32 and plan.table.shape == (plan.N, windows.ROW)
    assert plan.frames == sum(lens[i] for i in plan.planned) <= plan.N * Wn
    rows = plan.table[:plan.n_windows]
    for r in plan.table[plan.n_windows:]:                       # padding rows: marked by [5] = -1, nothing kept, full length
        assert r[5] == -1 and r[2] == r[3] and r[windows.VALID] == 0
    off = 0
    for i in plan.planned:
        T = lens[i]
        mine = rows[rows[:, 0] == i]
        assert plan.offsets[i] == off                            # staging and output offsets back to back
        kept = np.zeros(T, dtype=np.int64)
        if T < Wn:
            assert len(mine) == 1
            assert mine[0].tolist() == [i, 0, 0, T, off, off, T, 0]
        for u, s, lo, hi, dst, src, v, z in mine:
            if T >= Wn:
                assert v in (0, Wn) and 0 <= s and s + Wn <= T
            assert s <= lo <= hi <= s + Wn and dst == off + lo and src == off + s and z == 0
            kept[lo:hi] += 1
        assert bool((kept == 1).all())                           # every frame kept exactly once
        off += T
    assert plan.has_short_rows == any(0 < t < Wn for t in lens)
    if not any(t < Wn for t in lens):                            # no short utterance: today's plan
        old = windows.plan_windows(lens, Wn, H)
        assert plan.N == old.N and np.array_equal(plan.table[:, :6], old.table[:, :6]) and plan.offsets == old.offsets
    return plan


def test_short_plan_every_length_alone_and_mixed():
    Wn = windows.W
    rnd = random.Random(77)
    for H in (14, 12):
        for T in range(1, 4 * Wn + 4):
            _check_short_plan([T], Wn, H)
            _check_short_plan([rnd.randint(1, 400), T, rnd.randint(1, Wn - 1), rnd.randint(Wn, 900)], Wn, H)
    for _ in range(50):
        _check_short_plan([rnd.randint(0, 1200) for _ in range(rnd.randint(1, 40))], Wn, 14)
    assert windows.plan_windows([5, 7], Wn, 14, short_rows=True).N == 2


def test_default_plan_is_unchanged():
    """Without the opt-in the short utterances stay out of the table and column VALID stays zero."""
    plan = windows.plan_windows([5, 300, 95, 96], windows.W, 14)
    assert plan.short == [0, 2] and plan.planned == [1, 3] and not plan.has_short_rows
    assert not plan.table[:, windows.VALID].any()


def _generators(cfg, which):
    if which == "v1":
        return ohifi.fold_weight_norm(hifi_state_dict_wn(11)), cfg.hifi
    return v3_folded(11), v3_hifi(cfg)


@pytest.mark.parametrize("which", ["v1", "v3"])
def test_masked_rows_reproduce_the_solo_runs(cfg, which):
    sd, h = _generators(cfg, which)
    mels = [make_mel(1, T, seed=100 + T) for T in ROW_LENS]
    batch = padded_batch(mels, windows.W)
    with torch.no_grad():
        solo = [generator_any(sd, h, m) for m in mels]
        got = generator_rows(sd, h, batch, ROW_LENS)
        plain = generator_rows(sd, h, batch, ROW_LENS, mask=False)
    worst = 0.0
    for b, T in enumerate(ROW_LENS):
        d = float((got[b:b + 1, :, :T * SPF] - solo[b]).abs().max())
        tail = slice(max(T - 1, 0) * SPF, T * SPF)
        c = float((plain[b:b + 1, :, tail] - solo[b][:, :, tail]).abs().max())
        print("%s T=%2d: masked vs solo max-abs %.3g; zero-padded mel, no masks, last frame: %.3g (signal RMS %.3g)"
              % (which, T, d, c, float(solo[b].pow(2).mean().sqrt())))
        worst = max(worst, d)
        if T < windows.W:
            assert c > 1e-3, "the negative control does not see the missing masks at T=%d" % T
    print("%s: worst masked-vs-solo max-abs %.3g (bar %.3g)" % (which, worst, MASKED_BAR))
    assert worst <= MASKED_BAR
