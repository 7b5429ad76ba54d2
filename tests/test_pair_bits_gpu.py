"""GPU: the HiFi-GAN pair kernels (ttsk_hifi_conv_pair at C = 256 / 128 / 64 / 32) and the ResBlock2 kernel (ttsk_hifi_resblock2, every
instance) give the bits of the commit recorded in tests/golden/pair_bits_digests.json (tools/make_goldens_pair_bits.py), in both
16-bit types, the three MRF modes and through the *_rowlen entry points, at the lengths of tests/pair_bits_util.py, and the same
bytes on a second run.

CPU: the golden file covers the cases, and the cases cover every kernel, instance and edge they are meant to."""
import json
import os

import pytest

from tests import pair_bits_util as U

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_bits_digests.json")
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_golden_file_covers_the_cases(gold):
    assert sorted(gold["cases"]) == sorted(U.case_id(c) for c in U.CASES) and len(gold["commit"]) == 40
    for c in U.CASES:
        want = {"%s_m%d" % (t, m) for t in ["ln%d" % ln for ln in U.lengths(c)] + ["rows"] for m in (0, 1, 2)}
        assert set(gold["cases"][U.case_id(c)]) == want, U.case_id(c)


def test_cases_cover_every_kernel_and_edge():
    pairs = {(c[1], c[2], c[3], c[5]) for c in U.CASES if c[0] == "pair"}
    assert pairs == {(C, K, d, dt) for C in (256, 128, 64, 32) for K, d in ((3, 1), (7, 3), (11, 5)) for dt in ("f16", "bf16")}
    assert all(U.PAIR_LNS[C] == (5, 95, 96, 97, 193) for C in (256, 128)) and all(U.PAIR_LNS[C] == (7, 175, 176, 177, 353) for C in (64, 32))
    # ResBlock2: one case per instance, at the conv1 halo that is the instance's upper edge; TT as csrc/resblock2.hip's Rb2Geom has it
    assert [(C, h1) for C, _, _, _, h1, _ in U.RB2] == [(128, 8), (128, 16), (128, 40), (64, 16), (64, 48), (32, 32), (32, 64)]
    for (C, K, d0, d1, h1, tt), ew in zip(U.RB2, (1, 2, 5, 1, 3, 1, 2)):
        fg = 4 // (C // 32 if C >= 64 else 1)
        nf2 = 3 if C == 32 else (4 if C == 128 and ew > 2 else 6)
        assert (K - 1) // 2 * d1 == h1 == 8 * fg * ew and (K - 1) // 2 * d0 <= 16 and tt == fg * nf2 * 16
        assert U.lengths(("rb2", C, K, d0, d1, "f16")) == (13, tt - 1, tt, tt + 1)
    # the rows call: a row shorter than every tile, a full one, and an edge strictly inside a tile of every kernel
    short, edge = U.ROWS_VS[0] * U.ROWS_SPF, U.ROWS_VS[2] * U.ROWS_SPF
    assert U.ROWS_VS[1] == 0 and all(short < tt and edge % tt != 0 and edge < U.ROWS_LN for tt in (64, 96, 176, 192))


@gpu
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_bits_of_the_recorded_commit(case, gold):
    from tts_king_amd import ops
    kind, C, K, d0, d1, _ = case
    assert ops.hifi_conv_pair_supported(C, K, d0) if kind == "pair" else ops.hifi_resblock2_supported(C, K, d0, d1)
    want = gold["cases"][U.case_id(case)]
    got = U.run_case(case)
    again = U.run_case(case)
    for k in sorted(want):
        print("%-12s %s %s" % (k, got.get(k), "ok" if got.get(k) == want[k] else "DIFFERS from " + want[k]))
    assert got == again, sorted(k for k in got if got[k] != again[k])
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
