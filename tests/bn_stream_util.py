"""Cases and runner shared by tools/make_goldens_bn_stream.py and tests/test_bn_stream_bits_gpu.py: the slab BatchNorm kernels
(ttsk_bn_stats_slab / ttsk_bn_train_apply, ttsk_bn_bwd_stats_slab / ttsk_bn_bwd_apply_slab) at the smallest shapes at which they can
go wrong, every output reduced to a sha256.

A case is (width, rows, nblk of the hand-made partial table, frames per utterance or None).  Its inputs come from a seeded numpy
generator on the CPU.  The forward runs twice over the same inputs: once on the partial rows ttsk_bn_stats_slab writes, once on a
hand-made table of `nblk` rows (the kernel sums whatever rows it is given); the backward runs from the stored keep bytes and from rng,
accumulating onto non-zero dgamma / dbeta and overwriting them, and once more on a hand-made table.

The hand-made tables are built so that the ORDER of the fp64 additions shows in the fp32 results: every column holds a few pairs
+L, -L with L around 2^40 at scattered rows between values of order one (a spread of 2^40 >= the 2^30 asked for).  While a pair is open
the running sum sits at 2^40, where an fp64 ulp is 2^-12, so each small value added then is rounded at 2^-12; the pairs cancel exactly
and the total is of order one again, carrying rounding errors that depend on which additions met an open pair: far above the fp32 ulp
of the published mean / rstd / dgamma / dbeta.  order_sensitive() checks that on the CPU (two orders, different fp32 bits)."""
import hashlib

import numpy as np
import torch

DEV = "cuda:0"
SEED = 0x5DEECE66D1234567
STEP = (1 << 40) + 3
SITE = 40

# width -> (x dtype, dout dtype, tanh, p, residual + fp32 out)
WIDTHS = {
    512: (torch.float32, torch.bfloat16, True, 0.5, False),       # the PostNet's first four layers: fp32 conv output, bf16 out, keep bytes
    80: (torch.float32, torch.float32, False, 0.0, True),         # its last layer: residual, fp32 out
    64: (torch.bfloat16, torch.bfloat16, True, 0.5, False),       # one slab, bf16 input
    128: (torch.float32, torch.bfloat16, True, 0.5, False),       # two slabs
}
FULL = (16, 423)
# (C, rows, nblk, seg): rows at the iteration / chunk edges (C = 512: 16 rows per iteration, 64 per chunk; C = 80: 12 and 48), each with one
# of the table sizes 1, 6, 16, 17, 112, 128, 129, 200 (one row; the 16-loads-per-thread batch; the training count; the second pass of the
# row loop); seg: frame limit seg - 7 over utterances of seg frames
CASES = [(512, r, n, None) for r, n in zip((1, 15, 16, 17, 63, 64, 65, 225), (1, 6, 16, 17, 112, 128, 129, 200))]
CASES += [(80, 47, 6, None), (80, 48, 17, None), (80, 49, 129, None), (80, 225, 200, None)]
CASES += [(64, 225, 200, None), (128, 225, 16, None)]
CASES += [(C, 225, 112, 75) for C in (512, 80, 64, 128)]
CASES += [(C, FULL[0] * FULL[1], 112, seg) for C in (512, 80) for seg in (None, FULL[1])]
CASES += [(C, FULL[0] * FULL[1], 128, None) for C in (64, 128)]


def case_id(case):
    C, rows, nblk, seg = case
    return "C%d-rows%d-nblk%d-%s" % (C, rows, nblk, "all" if seg is None else "seg%d" % seg)


def hand_table(rng, nblk, C, n_live):
    """[nblk][2C] fp32: order-one values (second half: positive, so that the variance stays positive) and cancelling pairs of ~2^40."""
    t = np.empty((nblk, 2 * C), dtype=np.float32)
    t[:, :C] = rng.standard_normal((nblk, C), dtype=np.float32)
    t[:, C:] = (n_live / nblk) * (0.5 + rng.random((nblk, C), dtype=np.float32))
    if nblk >= 4:
        for c in range(2 * C):
            rows = rng.permutation(nblk)[:2 * min(4, nblk // 4)]
            big = np.float32(2.0 ** 40) * (1 + rng.random(len(rows) // 2, dtype=np.float32))
            t[rows[0::2], c] = big
            t[rows[1::2], c] = -big
    return t


def totals(table, G):
    """The kernels' order: group g adds rows g, g + G, ... ascending; the groups are added in ascending g.  fp64."""
    out = np.zeros(table.shape[1], dtype=np.float64)
    for g in range(min(G, table.shape[0])):
        acc = np.zeros(table.shape[1], dtype=np.float64)
        for r in range(g, table.shape[0], G):
            acc = acc + table[r].astype(np.float64)
        out = out + acc
    return out


def order_sensitive(table, G):
    """(plain, reversed): whether adding the rows in plain ascending order, or the table upside down in the kernels' order, changes the
    fp32 value of a column total.  (With no more than G rows the kernels' order IS plain ascending.)"""
    a = totals(table, G).astype(np.float32)
    b = totals(table, 1).astype(np.float32)
    c = totals(table[::-1], G).astype(np.float32)
    return bool((a != b).any()), bool((a != c).any())


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def make_inputs(case):
    C, rows, nblk, seg = case
    xdt, ddt, tanh, p, resid = WIDTHS[C]
    rng = np.random.default_rng([C, rows, nblk, 0 if seg is None else seg])
    n_live = rows if seg is None else (rows // seg) * (seg - 7)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))
    d = {"x": (0.5 + 1.5 * f(rows, C)).to(xdt), "dout": f(rows, C).to(ddt), "gamma": 1 + 0.1 * f(C), "beta": 0.1 * f(C),
         "run_mean": 0.1 * f(C), "run_var": 1 + 0.1 * f(C).abs(), "dgamma0": f(C), "dbeta0": f(C),
         "resid": f(rows, C) if resid else None,
         "table_f": torch.from_numpy(hand_table(rng, nblk, C, n_live)), "table_b": torch.from_numpy(hand_table(rng, nblk, C, n_live))}
    return d


def run_case(case):
    """-> {output name: sha256}.  Names: f_* forward on the kernel's own partial rows, ft_* forward on the hand-made table, b_keep_* / b_rng_*
    backward from the keep bytes (accumulate) / from rng (overwrite), bt_* backward on the hand-made table."""
    from tts_king_amd import ops
    C, rows, nblk, seg = case
    xdt, ddt, tanh, p, resid = WIDTHS[C]
    d = {k: (v.to(DEV) if v is not None else None) for k, v in make_inputs(case).items()}
    st = ops.optim_state(DEV, seed=SEED)
    st[3] = STEP
    rng = ops.rng_of(st) if p > 0 else None
    fl = None if seg is None else (torch.tensor([seg - 7], dtype=torch.int32, device=DEV), seg)
    out = {}

    def fwd(tag, partials):
        run = (d["run_mean"].clone(), d["run_var"].clone(), torch.full((1,), 5, dtype=torch.int64, device=DEV))
        o, mean, rstd, keep = ops.bn_train(d["x"], *run, d["gamma"], d["beta"], tanh, p=p, site=SITE, rng=rng, resid=d["resid"], out_f32=resid,
                                           frame_limit=fl, partials=partials, want_keep=True)
        assert (keep is not None) == (p > 0)
        if fl is not None:          # frames past the limit: zero rows, keep 0
            dead = (torch.arange(rows, device=DEV) % seg) >= seg - 7
            assert not bool(o[dead].any()) and (keep is None or not bool(keep[dead].any())), "%s: a dead row is not zero" % tag
        for name, t in (("out", o), ("mean", mean), ("rstd", rstd), ("keep", keep), ("run_mean", run[0]), ("run_var", run[1]), ("nbt", run[2])):
            if t is not None:
                out["%s_%s" % (tag, name)] = sha(t)
        return mean, rstd, keep

    def bwd(tag, mean, rstd, keep, accumulate, partials):
        dg, db = d["dgamma0"].clone(), d["dbeta0"].clone()
        dx = ops.bn_bwd(d["dout"], d["x"], mean, rstd, d["gamma"], d["beta"], tanh, p=p, site=SITE, rng=rng, dgamma=dg, dbeta=db,
                        frame_limit=fl, keep=keep, accumulate=accumulate, partials=partials)
        out["%s_dx" % tag], out["%s_dgamma" % tag], out["%s_dbeta" % tag] = sha(dx), sha(dg), sha(db)

    mean, rstd, keep = fwd("f", None)
    bwd("b_keep", mean, rstd, keep, True, None)
    bwd("b_rng", mean, rstd, None, False, None)
    bwd("bt", mean, rstd, keep, True, d["table_b"])
    fwd("ft", d["table_f"])
    torch.cuda.synchronize()
    return out
