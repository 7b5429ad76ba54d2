"""GPU: the slab BatchNorm kernels (ttsk_bn_train_apply, ttsk_bn_bwd_apply_slab and the statistics kernels in front of them) give the
bits of the commit recorded in tests/golden/bn_stream_digests.json (tools/make_goldens_bn_stream.py), at the rows, widths, partial-row
counts and frame limits of tests/bn_stream_util.py, and the same bytes on a second run.

CPU: the hand-made partial tables do show a wrong addition order in fp32 (otherwise the digests would pin nothing about the order)."""
import json
import os

import numpy as np
import pytest

from tests import bn_stream_util as U

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_stream_digests.json")
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_golden_file_covers_the_cases(gold):
    assert sorted(gold["cases"]) == sorted(U.case_id(c) for c in U.CASES) and len(gold["commit"]) == 40
    assert {n for c in U.CASES for n in [c[2]]} == {1, 6, 16, 17, 112, 128, 129, 200}


@pytest.mark.parametrize("nblk", [6, 16, 17, 112, 128, 129, 200])
@pytest.mark.parametrize("C", [64, 80])
def test_hand_tables_show_the_addition_order(C, nblk):
    """The kernels' order against plain ascending rows and against the table upside down: different fp32 totals in some column."""
    G = 256 // ((64 if C % 64 == 0 else C) // 2)
    t = U.hand_table(np.random.default_rng([C, nblk]), nblk, C, 1000)
    col = np.abs(t)
    assert (col.max(axis=0) / col.min(axis=0) >= 2.0 ** 30).all()
    plain, rev = U.order_sensitive(t, G)
    assert rev and (plain or nblk <= G)


@gpu
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_bits_of_the_recorded_commit(case, gold):
    want = gold["cases"][U.case_id(case)]
    got = U.run_case(case)
    again = U.run_case(case)
    for k in sorted(want):
        print("%-14s %s %s" % (k, got.get(k), "ok" if got.get(k) == want[k] else "DIFFERS from " + want[k]))
    assert got == again, sorted(k for k in got if got[k] != again[k])
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
