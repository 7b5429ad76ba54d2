"""GPU: `ttsk_optim_step` — the optimizer step over element ranges of the flat buffers — on a synthetic buffer, not the model.
reference: train.py:47-54 with `requires_grad_(False)` on part of the parameters: clip_grad_norm_ and torch.optim.Adam skip those.

The range table holds a range at offset 0, an 8-float range, two ranges separated by an 8-float frozen gap, a range much longer
than one workgroup's share of a launch (20,000 floats; a workgroup takes 256 groups of four per pass) and a range that ends at n.

Bars.  The norm against an fp64 sum: 1e-5 relative, the bar of tests/test_optim_gpu.py.  Against Adam restated in fp64 on the subset:
the bars of tests/test_rowops_gpu.py::test_clip_adam_lr (one range over the whole buffer) for the same kernel arithmetic (update rtol
2e-3 / atol 6e-7 = an fp32 ulp of |p| <= 4;
the shadow is the bf16 rounding of the parameters, exactly); the moments are three fp32 multiply-adds away from fp64: rtol 1e-5, plus a few ulps of their
largest operand where the two terms cancel: 2e-8 for |m| <= 0.05, 1e-10 for v <= 2e-4).  With packed items in the tables
(test_items_*): bit for bit the same ranges without items, and the items' packs bit for bit the pack launch's from the shadow."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
N = 65536
RANGES = [(0, 64), (128, 136), (144, 20144), (40000, N)]
SCHED = (256, 4000, [300000, 400000, 500000], 0.7)
B1, B2, EPS = 0.95, 0.999, 1e-5


def _mask():
    m = torch.zeros(N, dtype=torch.bool)
    for a, b in RANGES:
        m[a:b] = True
    return m


def _buffers(seed, gscale, n=N):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * gscale * (1 + t) / n ** 0.5 for t in range(3)]
    m0, v0 = 0.01 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)
    return p, grads, m0, v0


def _run(ranges, p, grads, m0, v0, zero_grad, start=0, items=()):
    """Three steps of ttsk_optim_step from (p, m0, v0); the shadow starts as a recognisable pattern.  `items`: the packed items of
    the tables (ops.optim_tables)."""
    from tts_king_amd import ops
    n = p.numel()
    st = ops.optim_state(DEV, seed=1, sched_step=start)
    dp, dm, dv = p.to(DEV), m0.to(DEV), v0.to(DEV)
    dg = torch.empty(n, device=DEV)
    sh = torch.full((n,), -7.0, dtype=BF, device=DEV)
    part = torch.empty(1024, device=DEV)
    tables = ops.optim_tables(ranges, list(items), DEV)
    assert tables is not None and tables["n_items"] == len(items)
    norms, after = [], []
    for g in grads:
        dg.copy_(g)
        ops.optim_step(dp, dg, dm, dv, sh, st, part, 1.0, B1, B2, EPS, *SCHED, tables, zero_grad=zero_grad, advance_rng=True)
        torch.cuda.synchronize()
        norms.append(float(st[6:7].view(torch.float32)[0]))
        after.append(dg.cpu().clone())
    return {"p": dp.cpu(), "m": dm.cpu(), "v": dv.cpu(), "sh": sh.cpu(), "g": after, "norms": norms, "st": st.cpu()}


@pytest.fixture(scope="module")
def runs():
    out = {}
    for scale in (1e-3, 3.0):                   # below and above the clip threshold (max_norm 1.0)
        buf = _buffers(5, scale)
        out[scale] = (buf, _run(RANGES, *buf, zero_grad=True), _run(RANGES, *buf, zero_grad=True))
    return out


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_trainable_elements_follow_adam_with_clip_over_the_subset(runs, scale):
    from oracle import fs2 as ofs2
    (p, grads, m0, v0), r, _ = runs[scale]
    mk = _mask()
    pr, mr, vr = p.double()[mk], m0.double()[mk], v0.double()[mk]
    for t, g in enumerate(grads, 1):
        gg = g.double()[mk]
        norm = float(gg.norm())                                      # fp64 sum over the ranges
        print("step %d: norm %.9g, kernel %.9g" % (t, norm, r["norms"][t - 1]))
        assert abs(r["norms"][t - 1] - norm) <= 1e-5 * norm
        gg = gg * min(1.0, 1.0 / (norm + 1e-6))
        mr = B1 * mr + (1 - B1) * gg
        vr = B2 * vr + (1 - B2) * gg * gg
        pr = pr - ofs2.lr_at(t) / (1 - B1 ** t) * mr / (vr.sqrt() / math.sqrt(1 - B2 ** t) + EPS)
        assert float(r["g"][t - 1][mk].abs().max()) == 0.0          # zero_grad: the trainable gradients are zeroed
    assert (scale > 1.0) == (float(torch.stack([g.double()[mk].norm() for g in grads]).min()) > 1.0), "the two cases sit on either side of the clip"
    np.testing.assert_allclose((r["p"].double()[mk] - p.double()[mk]).numpy(), (pr - p.double()[mk]).numpy(), rtol=2e-3, atol=6e-7)
    np.testing.assert_allclose(r["m"].double()[mk].numpy(), mr.numpy(), rtol=1e-5, atol=2e-8)
    np.testing.assert_allclose(r["v"].double()[mk].numpy(), vr.numpy(), rtol=1e-5, atol=1e-10)
    assert torch.equal(r["sh"][mk], r["p"][mk].to(BF))
    assert int(r["st"][0]) == 3 and int(r["st"][1]) == 3 and int(r["st"][3]) == 3      # scheduler, Adam and dropout counters advanced


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_frozen_elements_are_untouched_and_runs_repeat(runs, scale):
    (p, grads, m0, v0), r, r2 = runs[scale]
    fz = ~_mask()
    assert int(fz.sum()) == N - (64 + 8 + 20000 + (N - 40000))
    assert torch.equal(r["p"][fz], p[fz]) and torch.equal(r["m"][fz], m0[fz]) and torch.equal(r["v"][fz], v0[fz])
    assert torch.equal(r["sh"][fz], torch.full((int(fz.sum()),), -7.0, dtype=BF))
    for t, g in enumerate(grads):
        assert torch.equal(r["g"][t][fz], g[fz]), "frozen gradients are not zeroed either"
    for k in ("p", "m", "v", "sh", "st"):
        assert torch.equal(r[k], r2[k]), k                           # two runs: the same bits
    assert r["norms"] == r2["norms"]


def test_keep_grads_leaves_the_gradients():
    buf = _buffers(6, 1e-3)
    r = _run(RANGES, *buf, zero_grad=False)
    for t, g in enumerate(buf[1]):
        assert torch.equal(r["g"][t], g)


# ---- packed items in the tables.  A (32, 1, 256) with both packs: one tile; B (64, 3, 512) with the transposed pack only: two row
# tiles x two column blocks x three taps, the taps flipped in the pack — the smallest shapes that take every index of the tile walk
# past zero.  Gaps before, between and after the items; a frozen stretch between the two ranges, which holds a third item C whose
# pack no launch may touch; a frozen tail.
N2 = 131072
ITEMS = {"A": (64, (32, 1, 256)), "C": (8384, (32, 1, 256)), "B": (16704, (64, 3, 512))}
RANGES2 = [(0, 8320), (16640, 120000)]


def _item_views(sh):
    return {k: sh[off:off + cs * kk * ds].view(cs, kk, ds) for k, (off, (cs, kk, ds)) in ITEMS.items()}


@pytest.fixture(scope="module")
def item_runs():
    from tts_king_amd import ops
    out = {}
    for scale in (1e-3, 3.0):
        buf = _buffers(9, scale, N2)
        packs = {(k, tr): torch.full((ops.win_pack_numel(*ITEMS[k][1], tr),), 3.0, dtype=BF, device=DEV)
                 for k, tr in (("A", False), ("A", True), ("B", True), ("C", False))}
        items = [(*ITEMS["A"], packs["A", False], packs["A", True]), (*ITEMS["B"], None, packs["B", True])]
        with_items = _run(RANGES2, *buf, zero_grad=True, items=items)
        plain = _run(RANGES2, *buf, zero_grad=True)
        # the pack launch on the shadow the step left
        sh = with_items["sh"].to(DEV)
        want = {k: torch.empty_like(v) for k, v in packs.items() if k[0] != "C"}
        W = _item_views(sh)
        ops.win_conv_pack_run(*ops.win_conv_pack_table([(W[k], want[k, tr], tr) for k, tr in want], DEV))
        torch.cuda.synchronize()
        out[scale] = (buf, with_items, plain, {k: v.cpu() for k, v in packs.items()}, {k: v.cpu() for k, v in want.items()})
    return out


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_items_leave_the_bits_of_the_same_ranges_without_items(item_runs, scale):
    _, r, plain, _, _ = item_runs[scale]
    for k in ("p", "m", "v", "sh", "st"):
        assert torch.equal(r[k], plain[k]), k
    assert r["norms"] == plain["norms"]
    for a, b in zip(r["g"], plain["g"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_items_packs_equal_the_pack_launch_from_the_shadow(item_runs, scale):
    _, r, _, packs, want = item_runs[scale]
    assert set(want) == {("A", False), ("A", True), ("B", True)}
    for k in want:
        assert not torch.equal(want[k], torch.full_like(want[k], 3.0)), "the pack launch wrote something"
        assert torch.equal(packs[k], want[k]), k
    # ... and that shadow is the bf16 rounding of the updated parameters
    off, (cs, kk, ds) = ITEMS["B"]
    assert torch.equal(r["sh"][off:off + cs * kk * ds], r["p"][off:off + cs * kk * ds].to(BF))


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_items_frozen_item_and_frozen_elements_are_untouched(item_runs, scale):
    (p, grads, m0, v0), r, _, packs, _ = item_runs[scale]
    fz = torch.ones(N2, dtype=torch.bool)
    for a, b in RANGES2:
        fz[a:b] = False
    off, (cs, kk, ds) = ITEMS["C"]
    assert bool(fz[off:off + cs * kk * ds].all()) and int(fz.sum()) == N2 - 8320 - (120000 - 16640)
    assert torch.equal(packs["C", False], torch.full_like(packs["C", False], 3.0))
    assert torch.equal(r["p"][fz], p[fz]) and torch.equal(r["m"][fz], m0[fz]) and torch.equal(r["v"][fz], v0[fz])
    assert torch.equal(r["sh"][fz], torch.full((int(fz.sum()),), -7.0, dtype=BF))
    for t, g in enumerate(grads):
        assert torch.equal(r["g"][t][fz], g[fz])
        assert float(r["g"][t][~fz].abs().max()) == 0.0


def test_bad_tables_are_refused():
    from tts_king_amd import lib, ops
    p, grads, m0, v0 = _buffers(8, 1e-3)
    dp, dm, dv, dg = p.to(DEV), m0.to(DEV), v0.to(DEV), grads[0].to(DEV)
    sh, part, st = torch.zeros(N, dtype=BF, device=DEV), torch.empty(1024, device=DEV), ops.optim_state(DEV)
    empty = ops.optim_tables([], [], DEV)
    assert empty["n_ranges"] == 0
    with pytest.raises(lib.TtskError) as e:                          # zero ranges
        ops.optim_step(dp, dg, dm, dv, sh, st, part, 1.0, B1, B2, EPS, *SCHED, empty)
    assert "no trainable range" in str(e.value)
    too_long = dict(ops.optim_tables([(0, 64)], [], DEV), range_floats=N + 4)
    with pytest.raises(lib.TtskError):
        ops.optim_step(dp, dg, dm, dv, sh, st, part, 1.0, B1, B2, EPS, *SCHED, too_long)
    past_end = ops.optim_tables([(N - 64, N + 64)], [], DEV)
    with pytest.raises(lib.TtskError):                               # a range past the end of the buffers
        ops.optim_step(dp, dg, dm, dv, sh, st, part, 1.0, B1, B2, EPS, *SCHED, past_end)
    assert ops.optim_tables([(0, 64), (32, 128)], [], DEV) is None          # overlapping
    assert ops.optim_tables([(0, 66)], [], DEV) is None                     # not a multiple of four floats
    torch.cuda.synchronize()
    assert torch.equal(dp.cpu(), p) and int(st.cpu()[0]) == 0                     # nothing ran
