"""Cases and runner shared by tools/make_goldens_pair_bits.py and tests/test_pair_bits_gpu.py: the HiFi-GAN pair kernels
(ttsk_hifi_conv_pair at C = 256 / 128 / 64 / 32: conv_pair256_kernel, conv_pair_kernel, conv_pair_fs_kernel) and the ResBlock2 kernel
(ttsk_hifi_resblock2, every instance its dispatch can pick) at the smallest shapes at which a stage of theirs can go wrong, every
output reduced to a sha256.

A case is one (kernel, C, K, dilations, 16-bit type).  Its inputs and weights come from a numpy generator on the CPU seeded by the
case (weights scaled (C * K) ** -0.5).  For every length of the case, on a batch of two rows: the mode-0 output, then a mode-1 call
onto a non-zero `out`, then a mode-2 call onto that with scale = 1/3 and final_slope = 0.01.  Then the same three calls through the
*_rowlen entry point on three rows of ROWS_LN positions: one shorter than every tile, one full, one whose edge falls inside a tile;
what lies past a row's end is NaN in x and a sentinel in `out` (both are part of the hashed bytes: a read or a store there shows).

Lengths.  conv_pair / conv_pair256 store 96 frames per workgroup: 5 is one partial tile padded on both sides, 96 never takes the
no-padding path of the t store, 193 has a middle tile that does.  conv_pair_fs stores 176 (192 computed, 8 guard rows each side).
ResBlock2: Rb2Geom::TT of the instance, minus 1, exact, plus 1, and 13."""
import hashlib

import numpy as np
import torch

DEV = "cuda:0"
SENTINEL = 7.0
KD = [(3, 1), (7, 3), (11, 5)]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
PAIR_LNS = {256: (5, 95, 96, 97, 193), 128: (5, 95, 96, 97, 193), 64: (7, 175, 176, 177, 353), 32: (7, 175, 176, 177, 353)}
# (C, K, d0, d1, conv1 halo (K - 1) / 2 * d1 = the edge that selects the instance, Rb2Geom<C, EW>::TT)
RB2 = [(128, 3, 1, 8, 8, 96), (128, 5, 3, 8, 16, 96), (128, 5, 8, 20, 40, 64), (64, 3, 16, 16, 16, 192), (64, 7, 5, 16, 48, 192),
       (32, 5, 2, 16, 32, 192), (32, 3, 1, 64, 64, 192)]
# the rows call: ROWS_SPF samples per frame, rows of 7 frames (56 < every tile), all, and 30 frames (240: inside a tile of 64 / 96 / 176 / 192)
ROWS_SPF, ROWS_VS = 8, (7, 0, 30)
ROWS_LN = 37 * ROWS_SPF

CASES = [("pair", C, K, dil, 1, dt) for C in (256, 128, 64, 32) for K, dil in KD for dt in DTYPES]
CASES += [("rb2", C, K, d0, d1, dt) for C, K, d0, d1, _, _ in RB2 for dt in DTYPES]


def case_id(case):
    kind, C, K, d0, d1, dt = case
    return "%s-C%d-K%d-d%d%s-%s" % (kind, C, K, d0, "" if kind == "pair" else "_%d" % d1, dt)


def lengths(case):
    kind, C, K, d0, d1, dt = case
    if kind == "pair":
        return PAIR_LNS[C]
    tt = [r[5] for r in RB2 if r[:4] == (C, K, d0, d1)][0]
    return (13, tt - 1, tt, tt + 1)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def rows_table(n, vs):
    """The int32 length column inside a plan-shaped table, as tests/test_short_rows_gpu.py builds it."""
    from tts_king_amd import windows
    table = torch.zeros(n, windows.ROW, dtype=torch.int32)
    table[:, windows.VALID] = torch.tensor(vs, dtype=torch.int32)
    return table.to(DEV)[:, windows.VALID]


def run_case(case):
    """-> {"ln<len>_m<mode>" / "rows_m<mode>": sha256 of the whole `out`}."""
    from tts_king_amd import ops
    kind, C, K, d0, d1, dtn = case
    dt = DTYPES[dtn]
    rng = np.random.default_rng([C, K, d0, d1, int(dtn == "f16"), int(kind == "pair")])
    f = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))
    wA, wB = f(C, C, K) * (C * K) ** -0.5, f(C, C, K) * (C * K) ** -0.5
    bA, bB = (0.1 * f(C)).to(DEV), (0.1 * f(C)).to(DEV)
    pA, pB = ops.pack_resblock_weight(wA.to(DEV), dtype=dt), ops.pack_resblock_weight(wB.to(DEV), dtype=dt)

    def call(x, out, mode, rows):
        kw = dict(out=out, mode=mode, scale=1.0 / 3.0 if mode == 2 else 1.0, final_slope=0.01 if mode == 2 else 1.0, rows=rows)
        if kind == "pair":
            return ops.hifi_conv_pair(x, pA, bA, pB, bB, K, d0, **kw)
        return ops.hifi_resblock2(x, pA, bA, pB, bB, K, (d0, d1), **kw)

    def three(tag, x, prev, rows, out):
        out["%s_m0" % tag] = sha(call(x, torch.full_like(x, SENTINEL), 0, rows))
        acc = prev.clone()
        out["%s_m1" % tag] = sha(call(x, acc, 1, rows))
        out["%s_m2" % tag] = sha(call(x, acc, 2, rows))

    res = {}
    for ln in lengths(case):
        x, prev = (0.5 * f(2, ln, C)).to(dt).to(DEV), (0.5 * f(2, ln, C)).to(dt).to(DEV)
        three("ln%d" % ln, x, prev, None, res)
    n = len(ROWS_VS)
    x, prev = (0.5 * f(n, ROWS_LN, C)).to(dt), (0.5 * f(n, ROWS_LN, C)).to(dt)
    for b, v in enumerate(ROWS_VS):
        if v:
            x[b, v * ROWS_SPF:] = float("nan")
            prev[b, v * ROWS_SPF:] = SENTINEL
    three("rows", x.to(DEV), prev.to(DEV), (rows_table(n, ROWS_VS), ROWS_SPF), res)
    torch.cuda.synchronize()
    return res
