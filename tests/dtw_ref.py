"""fp64 numpy restatement of ttsk_dtw_align's definition (include/ttsk.h), vectorised by anti-diagonal.

D(i, j) = sum_c (x[i, c] - y[j, c])^2; A(0, 0) = D(0, 0); A(i, j) = D(i, j) + min over the predecessors that exist, taken in the
order (i-1, j-1), (i-1, j), (i, j-1), a later one replacing an earlier one only if it is strictly smaller.  The path is walked back
from (Tx-1, Ty-1); path_x[j] is the largest i with (i, j) on it; dur[l] counts the j whose path_x[j] lies in phoneme l's span of x."""
import numpy as np


def local_cost(x, y):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    D = np.zeros((x.shape[0], y.shape[0]))
    for c in range(x.shape[1]):                  # channel by channel: the direct form, without a (Tx, Ty, C) temporary
        D += (x[:, c, None] - y[None, :, c]) ** 2
    return D


def durations(path_x, x_seg):
    """Columns per phoneme: phoneme l spans rows [sum x_seg[:l], sum x_seg[:l+1])."""
    edges = np.concatenate([[0], np.cumsum(np.asarray(x_seg, dtype=np.int64))])
    return np.diff(np.searchsorted(np.asarray(path_x), edges, side="left")).astype(np.int64)


def dtw(x, y, x_seg=None):
    """x (Tx, C), y (Ty, C) -> (A (Tx, Ty) fp64, path [(i, j), ...] from (0, 0) to (Tx-1, Ty-1), path_x (Ty,), dur or None)."""
    D = local_cost(x, y)
    Tx, Ty = D.shape
    A = np.full((Tx, Ty), np.inf)
    bp = np.zeros((Tx, Ty), dtype=np.int8)
    A[0, 0] = D[0, 0]
    for k in range(1, Tx + Ty - 1):
        i = np.arange(max(0, k - Ty + 1), min(k, Tx - 1) + 1)
        j = k - i
        best = np.full(i.shape, np.inf)
        choice = np.zeros(i.shape, dtype=np.int8)
        m = (i > 0) & (j > 0)
        best[m] = A[i[m] - 1, j[m] - 1]
        m = i > 0
        up = np.full(i.shape, np.inf)
        up[m] = A[i[m] - 1, j[m]]
        take = m & ((up < best) | (j == 0))
        best[take], choice[take] = up[take], 1
        m = j > 0
        left = np.full(i.shape, np.inf)
        left[m] = A[i[m], j[m] - 1]
        take = m & ((left < best) | (i == 0))
        best[take], choice[take] = left[take], 2
        A[i, j] = D[i, j] + best
        bp[i, j] = choice
    i, j = Tx - 1, Ty - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = bp[i, j]
        if c == 0:
            i, j = i - 1, j - 1
        elif c == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    path.reverse()
    path_x = np.full(Ty, -1, dtype=np.int64)
    for i, j in path:
        path_x[j] = max(path_x[j], i)
    return A, path, path_x, (None if x_seg is None else durations(path_x, x_seg))


def path_from_path_x(path_x, Tx):
    """The full monotone path that path_x (largest i per column) stands for: in column j the rows from the previous column's
    last row (diagonal step when it moved on, else the same row) up to path_x[j]."""
    path, prev = [], 0
    for j, last in enumerate(np.asarray(path_x).tolist()):
        first = prev if (j == 0 or last == prev) else prev + 1
        path.extend((i, j) for i in range(first, last + 1))
        prev = last
    return path


def path_cost(x, y, path):
    """The fp64 cost of `path` over D(x, y), after checking that it is a warping path: starts at (0, 0), ends at (Tx-1, Ty-1), and
    every step is one of (1, 1), (1, 0), (0, 1)."""
    D = local_cost(x, y)
    Tx, Ty = D.shape
    p = np.asarray(path, dtype=np.int64)
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (Tx - 1, Ty - 1), "endpoints %s .. %s" % (p[0], p[-1])
    steps = np.diff(p, axis=0)
    ok = ((steps >= 0) & (steps <= 1)).all(axis=1) & (steps.sum(axis=1) >= 1)
    assert ok.all(), "not unit monotone steps at %s" % np.nonzero(~ok)[0][:5]
    return float(D[p[:, 0], p[:, 1]].sum())


def brute_force(x, y):
    """All monotone paths by recursion (tiny sizes only) -> (optimal cost, the optimal paths as lists of (i, j))."""
    D = local_cost(x, y)
    Tx, Ty = D.shape
    best, paths = [np.inf], []

    def walk(i, j, acc, trail):
        acc = acc + D[i, j]
        trail = trail + [(i, j)]
        if (i, j) == (Tx - 1, Ty - 1):
            if acc < best[0]:
                best[0] = acc
                paths[:] = [trail]
            elif acc == best[0]:
                paths.append(trail)
            return
        if i + 1 < Tx and j + 1 < Ty:
            walk(i + 1, j + 1, acc, trail)
        if i + 1 < Tx:
            walk(i + 1, j, acc, trail)
        if j + 1 < Ty:
            walk(i, j + 1, acc, trail)

    walk(0, 0, 0.0, [])
    return best[0], paths


def tie_rule_pick(paths):
    """Among optimal paths (all of one cost), the one the backward walk of the tie rule follows: from the end, at every cell prefer
    the predecessor (i-1, j-1), then (i-1, j), then (i, j-1) among those that lie on SOME optimal path through this suffix."""
    alive = [list(p) for p in paths]
    pos = 1
    while True:
        cells = {p[-pos] for p in alive}
        assert len(cells) == 1
        i, j = next(iter(cells))
        if (i, j) == (0, 0):
            return alive[0]
        pos += 1
        for pred in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            keep = [p for p in alive if p[-pos] == pred]
            if keep:
                alive = keep
                break


def make_warp(rng, Tx, Ty):
    """w (Ty,): non-decreasing, steps in {0, 1}, w[0] = 0, w[-1] = Tx - 1 (Ty >= Tx)."""
    steps = np.zeros(Ty - 1, dtype=np.int64)
    steps[rng.choice(Ty - 1, size=Tx - 1, replace=False)] = 1
    return np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def histogram_over_segments(w, x_seg):
    """How many entries of w fall into each phoneme's span of rows (by the row -> phoneme map, so zero-length phonemes get 0)."""
    x_seg = np.asarray(x_seg, dtype=np.int64)
    owner = np.repeat(np.arange(len(x_seg)), x_seg)
    return np.bincount(owner[np.asarray(w)], minlength=len(x_seg))
