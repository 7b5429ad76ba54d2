"""GPU: ttsk_dtw_align against its fp64 restatement (tests/dtw_ref.py).

Exact cases use integer-valued features in {-2..2}: a local cost is at most 80 * 16, so every cumulative cost stays below
80 * 16 * (Tx + Ty) <= 2.8e6 < 2^24 and fp32 is exact: path_x, cost and dur must EQUAL the restatement's, ties included.

Real-valued cases: every D and A is a sum of non-negative fp32 terms, so any path's computed cost is within (1 +- g) of its exact
cost, g = (C + Tx + Ty + 4) * 2^-24.  The DP's result is at most the computed cost of the true optimum, hence the fp64 cost of the
kernel's path K obeys A(K) <= A(O) (1 + g) / (1 - g); the bound leaves a factor 4 for contraction and summation order:
A(K) <= A(O) (1 + 4 g), and |cost - A(K)| <= 2 g cost.

The kernel hands back path_x only.  `dtw_ref.path_from_path_x` rebuilds the path: where path_x moves on between two columns the
path takes the diagonal step -- a left step followed by an up step through (path_x[j-1], j) is never chosen, because that cell's
cumulative cost is then its left neighbour's plus a non-negative term (also after fp32 rounding), so "up" could not be STRICTLY
smaller than the diagonal."""
import numpy as np
import pytest
import torch

from tests import dtw_ref
from tts_king_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = [(1, 1, 3), (1, 7, 1), (7, 1, 80), (2, 2, 128), (63, 65, 3), (64, 64, 80), (65, 63, 128), (130, 257, 1)]
EXACT = SMALL + [(1100, 1030, 80)]


def int_features(Tx, Ty, Cc, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, size=(Tx, Cc)).astype(np.float32), rng.integers(-2, 3, size=(Ty, Cc)).astype(np.float32)


def segments(rng, Tx, n):
    """n phoneme lengths summing to Tx, some of them zero."""
    cuts = np.sort(rng.integers(0, Tx + 1, size=n - 1))
    return np.diff(np.concatenate([[0], cuts, [Tx]])).astype(np.int32)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def solo(x, y, seg=None):
    out = ops.dtw_align(dev(x[None]), dev(y[None]), x_seg=None if seg is None else dev(seg[None]))
    torch.cuda.synchronize()
    return [o[0].cpu().numpy() for o in out]


_cases = {}


def exact_case(Tx, Ty, Cc):
    """(x, y, seg, restatement's path_x / cost / dur, the kernel's solo result), computed once per shape."""
    key = (Tx, Ty, Cc)
    if key not in _cases:
        x, y = int_features(Tx, Ty, Cc, seed=Tx * 7919 + Ty * 31 + Cc)
        seg = segments(np.random.default_rng(Tx + Ty), Tx, min(9, Tx + 2))
        A, _, path_x, dur = dtw_ref.dtw(x, y, seg)
        _cases[key] = (x, y, seg, path_x, A[-1, -1], dur, solo(x, y, seg))
    return _cases[key]


@pytest.mark.parametrize("Tx,Ty,Cc", EXACT)
def test_exact_on_integer_features(Tx, Ty, Cc):
    x, y, seg, want_px, want_cost, want_dur, (px, cost, st, dur) = exact_case(Tx, Ty, Cc)
    assert st == 0
    assert float(cost) == want_cost
    assert px.tolist() == want_px.tolist()
    assert dur.tolist() == want_dur.tolist() and int(dur.sum()) == Ty


def test_exact_without_segments_returns_three():
    x, y = int_features(9, 12, 5, seed=2)
    out = solo(x, y)
    assert len(out) == 3 and out[0].tolist() == dtw_ref.dtw(x, y)[2].tolist()


def test_batch_rows_equal_their_solo_results():
    """One launch of all the smaller shapes together (a launch has one channel count: C = 80, fresh features): ld larger than any
    length, NaN in the padding, zero-length phonemes in x_seg."""
    shapes = [(Tx, Ty) for Tx, Ty, _ in SMALL]
    Cc, ldx, ldy, ldL = 80, 140, 270, 12
    B = len(shapes)
    x = np.full((B, ldx, Cc), np.nan, dtype=np.float32)
    y = np.full((B, ldy, Cc), np.nan, dtype=np.float32)
    seg = np.full((B, ldL), -7, dtype=np.int32)              # entries from n_seg on are never read
    n_seg, rows = [], []
    for b, (Tx, Ty) in enumerate(shapes):
        xb, yb = int_features(Tx, Ty, Cc, seed=50 + b)
        sb = segments(np.random.default_rng(b), Tx, 5 + b)
        sb[1] += sb[2]
        sb[2] = 0                                            # at least one zero-length phoneme
        x[b, :Tx], y[b, :Ty], seg[b, :len(sb)] = xb, yb, sb
        n_seg.append(len(sb))
        rows.append((xb, yb, sb))
    px, cost, st, dur = ops.dtw_align(dev(x), dev(y), dev([s[0] for s in shapes], torch.int32), dev([s[1] for s in shapes], torch.int32),
                                      dev(seg), dev(n_seg, torch.int32))
    torch.cuda.synchronize()
    px, cost, st, dur = px.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), dur.cpu().numpy()
    assert st.tolist() == [0] * B
    for b, (Tx, Ty) in enumerate(shapes):
        xb, yb, sb = rows[b]
        spx, scost, sst, sdur = solo(xb, yb, sb)
        A, _, want_px, want_dur = dtw_ref.dtw(xb, yb, sb)
        assert px[b, :Ty].tolist() == spx.tolist() == want_px.tolist() and (px[b, Ty:] == -1).all()
        assert cost[b] == scost == A[-1, -1]
        assert dur[b, :len(sb)].tolist() == sdur.tolist() == want_dur.tolist() and not dur[b, len(sb):].any()
        assert dur[b, 2] == 0


@pytest.mark.parametrize("Tx,Ty", [(300, 290), (1100, 1030)])
def test_real_valued_path_is_optimal_within_the_rounding_bound(Tx, Ty):
    Cc = 80
    rng = np.random.default_rng(Tx)
    x, y = rng.standard_normal((Tx, Cc)).astype(np.float32), rng.standard_normal((Ty, Cc)).astype(np.float32)
    px, cost, st = solo(x, y)
    assert st == 0
    A = dtw_ref.dtw(x, y)[0]
    opt = A[-1, -1]
    path = dtw_ref.path_from_path_x(px, Tx)
    mine = dtw_ref.path_cost(x, y, path)                     # also checks that the path is a warping path
    g = (Cc + Tx + Ty + 4) * 2.0 ** -24
    print("(%d, %d): optimum %.9g, the kernel's path in fp64 %.9g (excess %.3g relative, bound %.3g), its fp32 cost %.9g (off by %.3g relative, bound %.3g)"
          % (Tx, Ty, opt, mine, mine / opt - 1, 4 * g, float(cost), abs(float(cost) - mine) / float(cost), 2 * g))
    assert mine <= opt * (1 + 4 * g)
    assert abs(float(cost) - mine) <= 2 * g * float(cost)


def test_status_rows_leave_the_others_alone():
    Cc, ld = 3, 20
    xa, ya = int_features(11, 17, Cc, seed=9)
    x = np.full((3, ld, Cc), np.nan, dtype=np.float32)
    y = np.full((3, ld, Cc), np.nan, dtype=np.float32)
    for b in range(3):
        x[b, :11], y[b, :17] = xa, ya
    seg = np.array([[5, 6, 0], [5, 6, 0], [5, 5, 0]], dtype=np.int32)          # row 2 sums to 10, not 11
    px, cost, st, dur = [o.cpu().numpy() for o in ops.dtw_align(dev(x), dev(y), dev([11, 0, 11], torch.int32), dev([17, 17, 17], torch.int32),
                                                                 dev(seg))]
    A, _, want_px, want_dur = dtw_ref.dtw(xa, ya, [5, 6, 0])
    assert st.tolist() == [0, 2, 3]
    assert px[0, :17].tolist() == want_px.tolist() and cost[0] == A[-1, -1] and dur[0].tolist() == want_dur.tolist()
    assert (px[1] == -1).all() and np.isposinf(cost[1]) and not dur[1].any()
    assert px[2, :17].tolist() == want_px.tolist() and cost[2] == A[-1, -1] and not dur[2].any()
    neg = np.array([[12, -1, 0]], dtype=np.int32)
    st = ops.dtw_align(dev(x[:1]), dev(y[:1]), dev([11], torch.int32), dev([17], torch.int32), dev(neg))[2]
    assert st.cpu().tolist() == [3]
    st = ops.dtw_align(dev(x[:1]), dev(y[:1]), dev([11], torch.int32), dev([0], torch.int32))[2]
    assert st.cpu().tolist() == [2]


def test_warp_recovery():
    rng = np.random.default_rng(3)
    Tx, Ty = 200, 330
    x = rng.standard_normal((Tx, 80)).astype(np.float32)
    w = dtw_ref.make_warp(rng, Tx, Ty)
    seg = segments(rng, Tx, 30)
    px, cost, st, dur = solo(x, x[w], seg)
    assert st == 0 and float(cost) == 0.0 and px.tolist() == w.tolist()
    assert dur.tolist() == dtw_ref.histogram_over_segments(w, seg).tolist()
